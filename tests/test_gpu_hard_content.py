"""GPU parity on hard content (tests/hard_content.py): saturated, directional, chroma-rich mosaics, bit exact against the oracle.

The pictures of synth.gen_frame() leave most of k_intra_mb's Intra4x4 chain, the directional Intra16x16 and chroma modes, the
partial-CBP neighbour rules of the coder, chroma residuals of P macroblocks and every clip255 of fer_intra.hip, fer_resid.hip
and fer_refprep.hip without input.  tests/test_hard_content_host.py shows on the oracle alone that the runs below reach them;
here the device only has to agree, picture by picture: RBSP bytes, reconstruction, macroblock types, CBP, TotalCoeff, Intra4x4
modes, both coded_mb_size estimates, vectors, the counters, and the decoder on the streams the device encoder wrote.

The comparison itself is tests/enc_parity.py (shared with test_gpu_qp_sweep.py); the three places where the reference leaves a
side array undefined, and the comparison leaves it out, are stated there.
"""
import numpy as np
import pytest

import hard_content as hc
from enc_parity import compare_stream, device_run

pytestmark = pytest.mark.gpu

SEEDS = (5, 6, 7)
QPS = (12, 17, 22, 27, 32, 37, 51)
# (W, H, seeds = streams of one context, qp, window)
CASES = ([(176, 144, SEEDS, qp, 16) for qp in QPS] + [(176, 144, SEEDS, 12, 32)]
         + [(176, 16, (5,), 12, 16), (176, 16, (5,), 28, 16), (16, 144, (5,), 12, 16), (16, 144, (5,), 28, 16)]
         + [(64, 48, tuple(range(20, 36)), 12, 16)])   # 16 streams: the per-XCD queues the benchmark runs
IDS = ["%dx%d_S%d_qp%d_w%d" % (c[0], c[1], len(c[2]), c[3], c[4]) for c in CASES]
_device = {}


def _device_run(pkg, case):
    """Four pictures of every stream through set_frames / encode_picture with explicit types -> per picture a dict of what the
    device produced ([S] leading); run once per case and shared by the tests."""
    if case not in _device:
        W, H, seeds, qp, window = case
        seqs = np.stack([hc.sequence(W, H, s) for s in seeds], 1)   # [4][S][fsz]
        _device[case] = device_run(pkg, W, H, seqs, qp, window)
    return _device[case]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_encoder_matches_oracle_on_hard_content(pkg, fo, case):
    W, H, seeds, qp, window = case
    dev = _device_run(pkg, case)
    for s, seed in enumerate(seeds):
        compare_stream(dev, s, hc.oracle_run(fo, W, H, seed, qp, window), f"seed {seed}")
    assert dev["status"] == [0] * len(seeds)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decoder_matches_oracle_decoder_on_hard_streams(pkg, fo, case):
    """The streams the device encoder wrote, through the device decoder, against the oracle decoder -- not against the encoder's
    reconstruction: the reference decoder re-applies stale ChromaACLevel to macroblocks of CBP 0 (F/residual.cpp:28-49), and its
    more_rbsp_data heuristic can stop before the last macroblocks of a slice that ends in a skip run; both are decoder behaviour
    the device decoder reproduces."""
    W, H, seeds, qp, window = case
    streams = _device_run(pkg, case)["streams"]
    out, pics, w, h = pkg.decode_streams(streams, 4)
    assert pics == [4] * len(seeds) and (w, h) == (W, H)
    ys = W * H
    for s, seed in enumerate(seeds):
        n, dec, _ = fo.decode_stream_md5(streams[s])
        assert n == 4
        for t in range(4):
            for name, a, b in (("Y", 0, ys), ("Cb", ys, ys + ys // 4), ("Cr", ys + ys // 4, ys * 3 // 2)):
                bad = np.flatnonzero(out[t, s][a:b] != dec[t][a:b])
                assert bad.size == 0, f"seed {seed} picture {t} {name}: {bad.size} samples differ, first at {bad[:8]}"


@pytest.mark.parametrize("W,H", [(176, 144), (176, 16), (16, 144)])
def test_refprep_matches_oracle_on_a_mosaic_reference(pkg, fo, W, H):
    """test_refprep_matches_oracle's comparison with a reference picture whose 6-tap sums leave 0..255 on both sides"""
    f0, f1 = hc.mosaic(W, H, 5), hc.mosaic(W, H, 5, (2, -2))
    o = fo.Oracle(W, H, qp=12, window=16)
    o.set_dpb(f0)
    o.fill_interpolated()
    g = pkg.FerHip(W, H, 1, qp=12, window=16)
    g.set_reference(f0[None])
    g.set_frames(f1[None])
    g.fill_interpolated()
    gi = g.read("INTERP").reshape(16, H, W)
    oi = np.stack([o.interp(f) for f in range(16)])
    assert (oi[1:] == 0).sum() >= 100 and (oi[1:] == 255).sum() >= 100, "the clip of the 6-tap filter gets no input"
    for f in range(16):
        assert np.array_equal(gi[f], oi[f]), f"interp plane {f}"
    gf = g.read("FEAT").reshape(H, W, 16, 6)
    for f in range(16):
        for k in range(5):
            assert np.array_equal(gf[:, :, f, k].astype(np.int32), o.kar(k, f)), (f, k)
    assert np.array_equal(g.read("KOLIKO")[:16384], o.koliko()[:16384])
    sp = g.read("SORTPOS")
    assert np.array_equal((sp >> 16).astype(np.int32), o.sorted(2))
    assert np.array_equal((sp & 0xFFFF).astype(np.int32), o.sorted(1))
    assert g.status() == [0]
    g.close()
    o.close()
