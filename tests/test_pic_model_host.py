"""tests/pic_model.py, the numpy yardstick of the descriptor ingest and output (tests/test_gpu_pictures.py), pinned against
tests/pad_model.py and against itself.  No GPU."""
import numpy as np
import pytest

import pad_model as pm
import pic_model as pic

SIZES = [(48, 32, 48, 32), (48, 32, 46, 18), (48, 32, 34, 30), (64, 32, 50, 32), (16, 16, 2, 2)]


@pytest.mark.parametrize("W,H,dw,dh", SIZES)
def test_tight_i420_gather_is_pad_picture(W, H, dw, dh):
    rng = np.random.default_rng(W + dw + dh)
    fsz = dw * dh * 3 // 2
    frames = rng.integers(0, 256, (3, fsz), dtype=np.uint8)
    buf = np.concatenate([np.full(7, 0xEE, np.uint8), frames.ravel()])
    pics = [pic.tight_pic(pic.I420, dw, dh, 7 + s * fsz) for s in range(3)]
    got = pic.gather([buf], pics, pic.I420, dw, dh, W, H)
    for s in range(3):
        assert np.array_equal(got[s], pm.pad_picture(frames[s], dw, dh, W, H))


def _pitched(rng, fmt, dw, dh, extra, fill):
    """three streams: planes of stream 0 in one buffer, of stream 2 in three, stream 1 absent; odd bases"""
    crow = dw // 2 if fmt == pic.I420 else dw
    py, pc = dw + extra, crow + extra
    nb = pic.slot_bytes(fmt, py, pc, dh)
    bufs = [np.full(nb + 40, fill, np.uint8)] + [np.full(py * dh + 40, fill, np.uint8) for _ in range(3)]
    p0 = pic.slot_pic(fmt, py, pc, dh, base=5, buf=0)
    p2 = [(1, 3, py), (2, 1, pc)] + ([(3, 15, pc)] if fmt == pic.I420 else [])
    return bufs, [p0, None, p2]


@pytest.mark.parametrize("fmt", [pic.I420, pic.NV12])
@pytest.mark.parametrize("extra", [0, 1, 3, 61])
@pytest.mark.parametrize("W,H,dw,dh", SIZES)
def test_scatter_then_gather_round_trips_and_gaps_survive(fmt, extra, W, H, dw, dh):
    rng = np.random.default_rng(extra + dw)
    frames = rng.integers(0, 256, (3, dw * dh * 3 // 2), dtype=np.uint8)
    res = []
    for fill in (0x00, 0xFF):
        bufs, pics = _pitched(rng, fmt, dw, dh, extra, fill)
        out = pic.scatter(bufs, pics, fmt, frames, dw, dh)
        # every byte is either a written sample or still the fill, and exactly dw*dh*3/2 bytes per present stream were samples
        touched = sum(int((o != b).sum()) for o, b in zip(out, bufs))
        expect = sum(int((frames[s] != fill).sum()) for s in (0, 2))
        assert touched == expect
        got = pic.gather(out, pics, fmt, dw, dh, W, H)
        assert got[1] is None
        for s in (0, 2):
            assert np.array_equal(got[s], pm.pad_picture(frames[s], dw, dh, W, H))
            assert np.array_equal(pm.window(got[s], W, H, 0, 0, dw, dh), frames[s])  # scatter is gather's inverse on the window
        res.append(got)
    for s in (0, 2):
        assert np.array_equal(res[0][s], res[1][s])  # what lies in the gaps and around the planes does not matter


def test_nv12_interleaves_cb_and_cr():
    dw, dh = 4, 2
    frame = np.arange(dw * dh * 3 // 2, dtype=np.uint8) + 10  # Y 10..17, Cb 18 19, Cr 20 21
    buf = np.zeros(pic.slot_bytes(pic.NV12, 6, 7, dh), np.uint8)
    out = pic.scatter([buf], [pic.slot_pic(pic.NV12, 6, 7, dh)], pic.NV12, [frame], dw, dh)[0]
    assert out.tolist() == [10, 11, 12, 13, 0, 0, 14, 15, 16, 17, 0, 0, 18, 20, 19, 21, 0, 0, 0]
    assert pic.slot_bytes(pic.I420, 6, 7, dh) == 12 + 14


def test_nv12_literal_at_an_odd_base_and_pitch():
    """written out by hand, independent of the model's own index arithmetic: gather pads, scatter writes rows only"""
    dw, dh, W, H = 2, 4, 4, 6  # (the model knows no macroblock grid)
    #        Y at 3, pitch 5              CbCr at 27, pitch 3 (one pair per row)
    buf = np.array([0, 0, 0, 10, 11, 0, 0, 0, 12, 13, 0, 0, 0, 14, 15, 0, 0, 0, 16, 17, 0, 0, 0, 0, 0, 0, 0, 30, 40, 0, 31, 41, 0], np.uint8)
    p = [[(0, 3, 5), (0, 27, 3)]]
    got = pic.gather([buf], p, pic.NV12, dw, dh, W, H)[0]
    y = [10, 11, 11, 11, 12, 13, 13, 13, 14, 15, 15, 15, 16, 17, 17, 17, 16, 17, 17, 17, 16, 17, 17, 17]
    cb, cr = [30, 30, 31, 31, 31, 31], [40, 40, 41, 41, 41, 41]
    assert got.tolist() == y + cb + cr
    tight = np.array([1, 2, 3, 4, 5, 6, 7, 8, 50, 51, 60, 61], np.uint8)  # Y 2x4, Cb 50 51, Cr 60 61
    out = pic.scatter([np.full(33, 9, np.uint8)], p, pic.NV12, [tight], dw, dh)[0]
    assert out.tolist() == [9, 9, 9, 1, 2, 9, 9, 9, 3, 4, 9, 9, 9, 5, 6, 9, 9, 9, 7, 8, 9, 9, 9, 9, 9, 9, 9, 50, 60, 9, 51, 61, 9]
    # the same samples as I420 with Cb at an odd base: the planes land where NV12's pairs did not
    out = pic.scatter([np.full(33, 9, np.uint8)], [[(0, 3, 5), (0, 23, 3), (0, 28, 2)]], pic.I420, [tight], dw, dh)[0]
    assert out.tolist() == [9, 9, 9, 1, 2, 9, 9, 9, 3, 4, 9, 9, 9, 5, 6, 9, 9, 9, 7, 8, 9, 9, 9, 50, 9, 9, 51, 9, 60, 9, 61, 9, 9]


def test_check_refuses_short_pitches():
    for fmt, bad in [(pic.I420, [(0, 0, 15), (0, 0, 8), (0, 0, 8)]), (pic.I420, [(0, 0, 16), (0, 0, 7), (0, 0, 8)]),
                     (pic.NV12, [(0, 0, 16), (0, 0, 15)])]:
        with pytest.raises(AssertionError):
            pic.check([bad], fmt, 16)
