"""Does the hard content (tests/hard_content.py) reach the encoder's paths?  Decided on the CPU oracle alone.

test_gpu_hard_content.py compares the device with the oracle on these very runs; that comparison is worth what the oracle
exercises, so this test counts it: prediction modes, CBP values, macroblock types, vectors that leave the picture or are
fractional, samples that the clips of reconstruction and interpolation produce.  The floors are conditions on the generator
(change tiles or seeds if one is missed, never a floor).  Every run also stays under the largest level a 12-bit escape suffix
carries (2063): above it the reference's CAVLC writer is not pinned.
"""
import hashlib

import numpy as np
import pytest

import hard_content as hc

W, H = 176, 144
SEEDS = (5, 6, 7)
QPS = (12, 17, 22, 27, 32, 37, 51)   # every class of qp % 6
MAX_LEVEL = 2063                     # level_prefix 15 at suffixLength 0: levelCode 30 + 4095 at the most, |level| 2063
P_TYPES = {"P_L0_16x16": (0,), "P_L0_L0_16x8": (1,), "P_L0_L0_8x16": (2,), "P_8x8": (3, 4), "P_Skip": (31,)}
# partitions (x, y, w, h, index into Oracle.mv()'s four 8x8 quadrants) of the inter macroblock types
PARTS = {0: ((0, 0, 16, 16, 0),), 1: ((0, 0, 16, 8, 0), (0, 8, 16, 8, 2)), 2: ((0, 0, 8, 16, 0), (8, 0, 8, 16, 1)),
         3: ((0, 0, 8, 8, 0), (8, 0, 8, 8, 1), (0, 8, 8, 8, 2), (8, 8, 8, 8, 3))}
PARTS[4] = PARTS[3]
MD5_BASE = "1b05da098a54c0eeac2a9f5233bc2eb0"      # mosaic(176, 144, 5)
MD5_SHIFTED = "826582c3f5d7cce89e250dc511096bfe"   # mosaic(176, 144, 7, (6, 2))


def test_generator_is_pinned():
    assert hashlib.md5(hc.mosaic(W, H, 5).tobytes()).hexdigest() == MD5_BASE
    assert hashlib.md5(hc.mosaic(W, H, 7, (6, 2)).tobytes()).hexdigest() == MD5_SHIFTED
    a, b = hc.mosaic(W, H, 6), hc.mosaic(W, H, 6, (2, -2))
    ys = W * H
    assert np.array_equal(np.roll(a[:ys].reshape(H, W), (-2, 2), (0, 1)), b[:ys].reshape(H, W))
    assert np.array_equal(np.roll(a[ys:ys + ys // 4].reshape(H // 2, W // 2), (-1, 1), (0, 1)), b[ys:ys + ys // 4].reshape(H // 2, W // 2))
    seq = hc.sequence(W, H, 5)
    assert seq.shape == (4, ys * 3 // 2) and np.array_equal(seq[2], seq[3]) and not np.array_equal(seq[1], seq[2])


def _count(run, w, h):
    """what one oracle run reaches -> dict of counters (numpy arrays or ints)"""
    mbw = w // 16
    c = dict(i16=np.zeros(4, int), i4=np.zeros(9, int), i4_mbs=0, i_mbs=0, i4_cbp=set(), i16_cbp=set(), i_cbpc=np.zeros(3, int),
             p_type={k: 0 for k in P_TYPES}, p_cbpl=np.zeros(16, int), p_cbpc=np.zeros(3, int), leaves=0, fractional=0, end_skip=0,
             rec0=0, rec255=0, int0=0, int255=0)
    for k, r in enumerate(run):
        mt, cbp = r["mb_type"], r["cbp"]
        c["rec0"] += int((r["recon"] == 0).sum())
        c["rec255"] += int((r["recon"] == 255).sum())
        c["int0"] += r["interp_sat"][0]
        c["int255"] += r["interp_sat"][1]
        if k == 0:
            i4 = mt == 0
            c["i_mbs"] += mt.size
            c["i4_mbs"] += int(i4.sum())
            c["i16"] += np.bincount((mt[~i4] - 1) % 4, minlength=4)
            c["i4"] += np.bincount(r["i4mode"][i4].ravel(), minlength=9)
            c["i4_cbp"] |= set(int(v) for v in cbp[i4, 0])
            c["i16_cbp"] |= set(int(v) for v in cbp[~i4, 0])
            c["i_cbpc"] += np.bincount(cbp[:, 1], minlength=3)
            continue
        for name, vals in P_TYPES.items():
            c["p_type"][name] += int(np.isin(mt, vals).sum())
        coded = mt != 31   # a P_Skip macroblock has no CBP
        c["p_cbpl"] += np.bincount(cbp[coded, 0], minlength=16)
        c["p_cbpc"] += np.bincount(cbp[coded, 1], minlength=3)
        c["end_skip"] += int(mt[-1] == 31)
        for mb in np.flatnonzero(coded):
            for (px, py, pw, ph, q) in PARTS[int(mt[mb])]:
                vx, vy = (int(v) for v in r["mv"][mb, q])
                frac = (vx & 3) != 0 or (vy & 3) != 0
                x0, y0 = (mb % mbw) * 16 + px + (vx >> 2), (mb // mbw) * 16 + py + (vy >> 2)
                # the samples the prediction reads: one more column / row when that component is fractional
                x1, y1 = x0 + pw + ((vx & 3) != 0), y0 + ph + ((vy & 3) != 0)
                c["fractional"] += frac
                c["leaves"] += x0 < 0 or y0 < 0 or x1 > w or y1 > h
    return c


def test_hard_content_reaches_the_paths(fo):
    runs = {(s, q): _count(hc.oracle_run(fo, W, H, s, q, 16, planes=True), W, H) for s in SEEDS for q in QPS}
    for (s, q) in runs:
        for k, r in enumerate(hc.oracle_run(fo, W, H, s, q, 16)):
            assert r["max_level"] <= MAX_LEVEL, (s, q, k, r["max_level"])
    cs = list(runs.values())

    def total(key):
        return sum(c[key] for c in cs)

    i16, i4 = total("i16"), total("i4")
    print("Intra16x16 modes", i16, "Intra4x4 modes", i4, "Intra4x4 macroblocks", total("i4_mbs"), "of", total("i_mbs"))
    assert (i16 >= 10).all(), i16
    assert (i4 >= 50).all(), i4
    assert total("i4_mbs") * 10 >= total("i_mbs") * 3
    i4_cbp = set().union(*(c["i4_cbp"] for c in cs))
    i16_cbp = set().union(*(c["i16_cbp"] for c in cs))
    print("Intra4x4 luma CBP", sorted(i4_cbp), "Intra16x16 luma CBP", sorted(i16_cbp), "I cbpC", total("i_cbpc"))
    assert len(i4_cbp) >= 8, sorted(i4_cbp)
    assert {0, 15} <= i16_cbp
    assert (total("i_cbpc") >= 5).all(), total("i_cbpc")
    p_type = {k: sum(c["p_type"][k] for c in cs) for k in P_TYPES}
    print("P types", p_type, "P luma CBP", total("p_cbpl"), "P cbpC", total("p_cbpc"))
    assert all(v >= 5 for v in p_type.values()), p_type
    assert (total("p_cbpl") >= 1).all(), total("p_cbpl")
    assert (total("p_cbpc") >= 5).all(), total("p_cbpc")
    print("partitions leaving the picture", total("leaves"), "fractional", total("fractional"), "P pictures ending in a skip run",
          total("end_skip"))
    assert total("leaves") >= 50
    assert total("fractional") >= 100
    assert total("end_skip") >= 1
    print("reconstructed samples at 0 / 255", total("rec0"), total("rec255"), "interpolated", total("int0"), total("int255"))
    assert total("rec0") >= 1000 and total("rec255") >= 1000
    assert total("int0") >= 100 and total("int255") >= 100
    for q in QPS:   # per QP, over the three seeds: every mode at least once
        a = sum(runs[(s, q)]["i16"] for s in SEEDS)
        b = sum(runs[(s, q)]["i4"] for s in SEEDS)
        assert (a >= 1).all() and (b >= 1).all(), (q, a, b)


@pytest.mark.parametrize("w,h,seed,qp,window", [(176, 144, s, 12, 32) for s in SEEDS] + [(176, 16, 5, 12, 16), (176, 16, 5, 28, 16), (16, 144, 5, 12, 16), (16, 144, 5, 28, 16)]
                                                + [(64, 48, 20 + s, 12, 16) for s in range(16)])
def test_other_shapes_stay_under_the_level_guard(fo, w, h, seed, qp, window):
    """the further runs of test_gpu_hard_content.py: window 32, one macroblock high, one macroblock wide, the 16 small streams"""
    run = hc.oracle_run(fo, w, h, seed, qp, window)
    assert [len(r["rbsp"]) > 0 for r in run] == [True] * 4
    assert max(r["max_level"] for r in run) <= MAX_LEVEL
    assert (run[0]["mb_type"] < 31).all() and (run[0]["recon"] != hc.sequence(w, h, seed)[0]).any()
