"""The GPU decoder against the oracle decoder on the streams of tests/slice_synth.py: real CAVLC residuals in every
coeff_token class, escapes and the suffixLength climb, intra macroblocks in P slices at every neighbour kind, QPy over
0..51 with wraps, chroma_qp_index_offset, the largest levels, the state carried across pictures, other header widths.
Every plan goes through ferhip_decode_streams, ferhip_dec_nal, ferhip_decs_decode (uneven chunks) and
ferhip_decs_decode_dev, and every picture must equal the oracle's bit for bit.  test_slice_synth_host.py pins the
streams (and that the plans contain that syntax) without a GPU."""
import numpy as np
import pytest

import slice_synth as ss

pytestmark = pytest.mark.gpu
E_STATE, E_UNSUP = -3, -4
FILL = 0xA5
_cache = {}


def plan(fo, name):
    """-> [(stream, oracle pictures [T][fsz])] * 2, W, H"""
    if name not in _cache:
        out = []
        for stream, _, types in ss.plan_streams(name):
            n, frames, _ = fo.decode_stream_trace(stream)
            assert n == len(types)
            out.append((stream, np.stack(frames)))
        cfg = dict(ss.CFG_DEFAULT, **ss.PLANS[name][0])
        _cache[name] = (out, cfg["mbw"] * 16, cfg["mbh"] * 16)
    return _cache[name]


def _same(got, ref, what):
    assert got.shape == ref.shape, f"{what}: {got.shape[0]} pictures, the oracle has {ref.shape[0]}"
    for t in range(ref.shape[0]):
        assert np.array_equal(got[t], ref[t]), f"{what}: picture {t} differs, first at byte {int(np.nonzero(got[t] != ref[t])[0][0])}"


@pytest.mark.parametrize("name", sorted(ss.PLANS))
def test_decode_streams_batch_of_two(pkg, fo, name):
    (a, b), W, H = plan(fo, name)
    T = max(a[1].shape[0], b[1].shape[0])
    out, pics, w, h = pkg.decode_streams([a[0], b[0]], T)
    assert (w, h) == (W, H) and pics == [a[1].shape[0], b[1].shape[0]]
    for s, (_, ref) in enumerate((a, b)):
        _same(out[:pics[s], s], ref, f"{name} stream {s}")


@pytest.mark.parametrize("name", sorted(ss.PLANS))
def test_streaming_decoder_nal_by_nal(pkg, fo, name):
    (a, _), W, H = plan(fo, name)
    d = pkg.Decoder()
    got = [p for p in (d.nal(*pkg.unescape_nal(n)) for n in pkg.split_nals(a[0])) if p is not None]
    d.close()
    assert (d.W, d.H) == (W, H)
    _same(np.stack(got), a[1], name)


def _uneven(n0, n1):
    """access units per call of the two streams: never the same number twice in a row, calls where one stream gives none"""
    pat0, pat1 = (2, 0, 3, 1, 1, 4), (1, 2, 0, 3, 1, 0)
    sched, k = [], 0
    while n0 > 0 or n1 > 0:
        c0, c1 = min(pat0[k % 6], n0), min(pat1[k % 6], n1)
        k += 1
        if c0 == 0 and c1 == 0:
            continue
        sched.append((c0, c1))
        n0, n1 = n0 - c0, n1 - c1
    return sched


@pytest.mark.parametrize("device_in", [False, True], ids=["host_chunks", "device_chunks"])
@pytest.mark.parametrize("name", sorted(ss.PLANS))
def test_live_decoder_uneven_chunks(pkg, fo, name, device_in):
    streams, W, H = plan(fo, name)
    aus = [pkg.access_units(s) for s, _ in streams]
    assert [len(a) for a in aus] == [r.shape[0] for _, r in streams]
    P, fsz = 4, W * H * 3 // 2
    dec = pkg.LiveDecoder(2, W, H, P)
    pitch = (max(len(s) for s, _ in streams) + 79) & ~15
    buf = pkg.DeviceBuffer(2 * pitch + 64) if device_in else None
    got, pos = [[], []], [0, 0]
    for call in _uneven(len(aus[0]), len(aus[1])):
        chunks = [b"".join(aus[s][pos[s]:pos[s] + call[s]]) or None for s in range(2)]
        out = np.full((P, 2, fsz), FILL, np.uint8)
        if device_in:
            ptrs, lens = [], []
            for s, c in enumerate(chunks):
                off = s * pitch + 2 * s + 1  # odd addresses
                if c:
                    buf.upload(np.frombuffer(c, np.uint8), off)
                ptrs.append(buf.ptr + off if c else None)
                lens.append(len(c) if c else 0)
            _, pics, status = dec.decode_dev(ptrs, lens, out)
        else:
            _, pics, status = dec.decode(chunks, out)
        assert status == [0, 0] and pics == list(call)
        for s in range(2):
            pos[s] += call[s]
            got[s] += [out[k, s].copy() for k in range(pics[s])]
            assert (out[pics[s]:, s] == FILL).all()
    dec.close()
    if buf:
        buf.free()
    for s, (_, ref) in enumerate(streams):
        _same(np.stack(got[s]), ref, f"{name} stream {s}")


@pytest.mark.parametrize("slice_type", ["I", "P"])
def test_i_pcm_is_reported_and_stays_in_its_stream(pkg, fo, slice_type):
    """mb_type 25 in an I slice / 30 in a P slice: the stream reports FERHIP_E_UNSUP, its neighbour in the batch decodes
    bit-exactly, and the library decodes a clean stream right after"""
    bad, ngood, good = ss.unsupported_stream(slice_type)
    clean, _, _ = ss.make_stream(9, dict(mbw=3, mbh=2), ss.PLANS["headers_wide"][1] + ss.PLANS["headers_wide"][1][1:])
    n, frames, _ = fo.decode_stream_trace(clean)
    ref = np.stack(frames)
    nb, bframes, _ = fo.decode_stream_trace(good)  # (the oracle, like the reference, has no I_PCM: it never sees the bad picture)
    assert nb == ngood
    W, H, fsz = 48, 32, 48 * 32 * 3 // 2
    with pytest.raises(pkg.FerHipError, match=f"code {E_UNSUP}"):
        pkg.decode_streams([bad, clean], n)
    dec = pkg.LiveDecoder(2, W, H, 1)
    aus = [pkg.access_units(bad), pkg.access_units(clean)]
    assert len(aus[0]) == ngood + 1 and len(aus[1]) == n >= ngood + 2
    for c in range(n):
        out = np.full((1, 2, fsz), FILL, np.uint8)
        _, pics, status = dec.decode([aus[0][c] if c < len(aus[0]) else None, aus[1][c]], out)
        assert status[1] == 0 and pics[1] == 1 and np.array_equal(out[0, 1], ref[c]), f"call {c}: the clean neighbour"
        if c < ngood:
            assert status[0] == 0 and pics[0] == 1 and np.array_equal(out[0, 0], bframes[c]), f"call {c}"
        else:
            assert status[0] == (E_UNSUP if c == ngood else 0) and pics[0] == 0 and (out[0, 0] == FILL).all(), f"call {c}"
    dec.close()
    out, pics, w, h = pkg.decode_streams([clean], n)
    assert pics == [n] and np.array_equal(out[:, 0], ref)
