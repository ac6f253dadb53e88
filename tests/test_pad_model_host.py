"""The model the display-size tests rest on (tests/pad_model.py), pinned without a GPU: the padding rule against np.pad,
synth.pad_to_mb against the rule, the SPS model against the oracle's SPS, and the property the decoder tests use -- the
oracle decoder stops reading an SPS after frame_mbs_only_flag, so a cropping SPS changes nothing it decodes."""
import numpy as np
import pytest

import pad_model as pm

SIZES = [(2, 2), (16, 2), (18, 30), (50, 38), (66, 48), (80, 34), (48, 32), (162, 130)]


def _coded(dw, dh):
    return (dw + 15) & ~15, (dh + 15) & ~15


@pytest.mark.parametrize("dw,dh", SIZES)
def test_pad_rule_is_edge_padding(dw, dh):
    W, H = _coded(dw, dh)
    f = np.random.default_rng(dw * 1000 + dh).integers(0, 256, dw * dh * 3 // 2, dtype=np.uint8)
    want = []
    for p, (PW, PH) in zip(pm.planes(f, dw, dh), ((W, H), (W // 2, H // 2), (W // 2, H // 2))):
        want.append(np.pad(p, ((0, PH - p.shape[0]), (0, PW - p.shape[1])), mode="edge").ravel())
    got = pm.pad_picture(f, dw, dh, W, H)
    assert np.array_equal(got, np.concatenate(want))
    assert np.array_equal(pm.window(got, W, H, 0, 0, dw, dh), f)


@pytest.mark.parametrize("dw,dh", SIZES)
def test_synth_pad_to_mb_is_the_model(pkg, dw, dh):
    W, H = _coded(dw, dh)
    f = np.random.default_rng(7 + dw * dh).integers(0, 256, dw * dh * 3 // 2, dtype=np.uint8)
    got, w, h = pkg.pad_to_mb(f, dw, dh)
    assert (w, h) == (W, H)
    assert np.array_equal(got, pm.pad_picture(f, dw, dh, W, H))


@pytest.fixture(scope="module")
def oracle_streams(fo):
    """(W, H) -> (Annex-B stream of 2 pictures, its NAL units, the oracle's own decode of it)"""
    out = {}
    for W, H in ((16, 16), (80, 48), (176, 144)):
        o = fo.Oracle(W, H, qp=20, window=16, maxdiff=3, intra_every=30)
        frames = np.stack([fo.gen_frame(W, H, t, 99, 2) for t in range(2)])
        stream, _ = o.encode_stream(frames)
        o.close()
        n, pics, st = fo.decode_stream_md5(stream)
        out[(W, H)] = (stream, pm.split_nals(stream), (n, pics, st))
    return out


@pytest.mark.parametrize("W,H", [(16, 16), (80, 48), (176, 144)])
def test_sps_model_without_crop_is_the_oracles(oracle_streams, W, H):
    nals = oracle_streams[(W, H)][1]
    assert nals[0][4] & 31 == 7
    assert pm.sps_nal(W, H) == nals[0]
    assert pm.sps_nal(W, H, W, H) == nals[0]  # the display size of the default writes no cropping


@pytest.mark.parametrize("W,H,dw,dh", [(16, 16, 2, 2), (80, 48, 66, 34), (80, 48, 80, 34), (176, 144, 162, 130)])
def test_sps_model_with_crop_shares_the_bits_in_front_of_the_flag(oracle_streams, W, H, dw, dh):
    plain, before = pm.sps_bits(W, H)
    crop, before2 = pm.sps_bits(W, H, (0, W - dw, 0, H - dh))
    assert before == before2 and plain.b[:before] == crop.b[:before]
    assert plain.b[before] == 0 and crop.b[before] == 1
    # ... and those are the oracle's bits: its SPS, unescaped (none of these has an emulation prevention byte), MSB first
    body = oracle_streams[(W, H)][1][0][5:]
    assert b"\x00\x00\x03" not in body
    obits = list(np.unpackbits(np.frombuffer(body, np.uint8)))
    assert obits[:before] == crop.b[:before]
    # the offsets that follow, read back
    b, pos = crop.b, [before + 1]

    def ue():
        z = 0
        while b[pos[0]] == 0:
            z += 1
            pos[0] += 1
        v = int("".join(map(str, b[pos[0]:pos[0] + z + 1])), 2) - 1
        pos[0] += z + 1
        return v

    assert [ue() for _ in range(4)] == [0, (W - dw) // 2, 0, (H - dh) // 2]
    assert b[pos[0]] == 0 and pos[0] + 1 == len(b)


@pytest.mark.parametrize("W,H,crop", [(16, 16, (0, 14, 0, 14)), (80, 48, (0, 14, 0, 14)), (80, 48, (4, 2, 6, 8)),
                                      (176, 144, (0, 14, 0, 14)), (176, 144, (100, 100, 0, 0))])
def test_oracle_decoder_ignores_the_cropping(fo, oracle_streams, W, H, crop):
    stream, _, (n, pics, st) = oracle_streams[(W, H)]
    swapped = pm.swap_sps(stream, pm.sps_nal(W, H, crop=crop))
    assert swapped != stream
    n2, pics2, st2 = fo.decode_stream_md5(swapped)
    assert n2 == n == 2 and st2 == st and (st["W"], st["H"]) == (W, H)
    for a, b in zip(pics, pics2):
        assert np.array_equal(a, b)
