"""What tests/route_content.py reaches, shown on the oracle and the list model alone (no GPU), and the bounds that put
the remaining routes of the selection out of reach.

  * every generator is pinned (CRC-32 of its two pictures);
  * on every new pair, at windows 16 and 32, the model equals the oracle's recording on EVERY searched partition, all three
    stages, as in test_me_model_host.py;
  * every pair reaches what route_content.REACHES names for it on at least one partition that the oracle searched, none of
    them in a P_Skip macroblock.  The counts are printed; DESIGN.md holds them;
  * no metric of any stage reaches 2^26 and no local metric reaches 2^21 (test_metric_bounds).
"""
import itertools
import zlib

import numpy as np
import pytest
import route_content as rc
from me_model import predict_8x8
from test_me_model_host import assert_list

CRC = {
    "far_below": (2864117850, 1275814746), "far_above": (949439014, 1275814746), "far_all": (973453154, 953217407),
    "many_flats": (1236564098, 1709830717), "noisy_bucket": (1991236638, 514054968), "many_listed": (1212273755, 1989430117),
    "pan_listed": (2300315261, 2200263083), "pan_noisy": (1974988020, 3181191433), "wide_noisy": (2622352252, 127396716),
}


@pytest.mark.parametrize("name", sorted(rc.PAIRS))
def test_generators_are_pinned(name):
    W, H, _ = rc.PAIRS[name]
    ref, src = rc.pair(name)
    assert ref.dtype == src.dtype == np.uint8 and ref.size == src.size == W * H * 3 // 2
    assert (W, H) in ((176, 144), (272, 48))  # QCIF, and one 48-high wide picture no wider than 280
    assert (zlib.crc32(ref.tobytes()), zlib.crc32(src.tobytes())) == CRC[name], name


def test_far_mismatch_is_what_it_says():
    """the numbers of the construction: D = 16320 between probe and tile, tiles at L1 distance 124 and 125, the metrics
    2088960 < 2^21 <= 2105280"""
    from me_model import box_sums
    for variant, n_le_124 in (("below", 17), ("above", 16), ("all_far", 0)):
        tiles, (px, py) = rc.far_tiles(variant)
        r = sorted(abs(x - px) + abs(y - py) for x, y in tiles)
        assert sum(v <= 124 for v in r) == n_le_124 and 125 in r and (124 in r) == (n_le_124 > 0), (variant, r)
        ref, src = rc.far_mismatch(variant)
        W, H = rc.QCIF
        s = box_sums(src[: W * H].reshape(H, W), px, py)
        k = box_sums(ref[: W * H].reshape(H, W), *tiles[0])
        assert s == [8160, 4080, 4080, 8160, 4080] and k == [8160, 4080, 4080, 0, 4080]
        D = abs(s[0] - k[0]) + sum(abs(s[i] - k[i]) + abs((s[0] - s[i]) - (k[0] - k[i])) for i in range(1, 5))
        assert D == 16320 and 128 * D == 2088960 < 1 << 21 <= 129 * D == 2105280


@pytest.mark.parametrize("window", [16, 32])
@pytest.mark.parametrize("name", sorted(rc.PAIRS))
def test_model_equals_the_oracle_and_routes_are_reached(fo, name, window):
    W, H, _ = rc.PAIRS[name]
    an = rc.analysis(fo, name, window)
    _, rec, mbt, mv, skips = an["orc"]
    m = an["model"]
    searched = np.nonzero(rec["searched"])[0]
    assert searched.size > 0
    field = mv.reshape(-1, 2)
    for p in searched:
        p = int(p)
        assert m.sums(p) == rec["suma"][p].tolist(), (name, p)
        mvpx, mvpy = (int(v) for v in rec["mvp"][p])
        assert predict_8x8(field, W // 16, p) == (mvpx, mvpy), (name, p)
        assert_list(m.stage3(p), rec, p, 2, "stage 3")
        assert_list(m.stage1(p, mvpx >> 2, mvpy >> 2), rec, p, 0, "stage 1")
        assert_list(m.stage2(p, mvpx >> 2, mvpy >> 2), rec, p, 1, "stage 2")
        # what test_metric_bounds rests its stage-2 claim on: every listed vector of every stage points at a block whose
        # origin lies inside the picture, so no vector, hence no median of vectors, is longer than the picture
        sx, sy = m.origin(p)
        for st in range(3):
            n = int(rec["n"][p, st])
            x, y = sx + (rec["bx"][p, st, :n] >> 2), sy + (rec["by"][p, st, :n] >> 2)
            assert ((x >= 0) & (x < W) & (y >= 0) & (y < H)).all(), (name, p, st, "a listed vector leaves the picture")
        assert abs(mvpx >> 2) + abs(mvpy >> 2) <= W + H <= 1715, (name, p, "centre")
    c = an["counts"]
    print("route_content", name, window, "P_Skip macroblocks", skips, c)
    for what in rc.REACHES[name]:
        assert c[what] > 0, (name, window, what, "not reached", c)
    assert c["max_metric"] < 1 << 26
    if name.startswith("far_"):
        # the probe's candidates are the tiles and nothing else, twice each, around the centre (0, 0)
        (p, r), = [(p, r) for p, r in an["routes"].items() if 0 < r["n"] <= 384]
        assert r["n"] == 2 * len(rc.far_tiles({"far_below": "below", "far_above": "above", "far_all": "all_far"}[name])[0])
        assert rec["mvp"][p].tolist() == [0, 0]
        assert r["nth"] == {"far_below": 2088960, "far_above": 2105280}.get(name, r["nth"])
        assert r["nth"] >= 1 << 21 or name == "far_below"


def _dist(s, k):
    return abs(s[0] - k[0]) + sum(abs(s[i] - k[i]) + abs((s[0] - s[i]) - (k[0] - k[i])) for i in range(1, 5))


def test_metric_bounds():
    """A metric is weight * D, D the nine-term feature distance of two 8x8 blocks of 8-bit samples.

    D.  A block's sum lies in 0..16320 and each of its four half sums, as the sum of the rest, in 0..8160.  D is convex in the
    ten sums, so over that box-shaped set its maximum sits on a vertex: all 1024 are tried.  D_MAX = 5 * 16320 = 81600.
    Inside the bucket walk (stage 2) a candidate also has |s0 - k0| <= 180 and |s1 - k1|, |s2 - k2| <= 99, so
    D <= 180 + 2 * (99 + 99 + 180) + 2 * 16320 = 33576 = D_WALK.
    Weights.  Stage 1 and the local part of stage 3: |tx - cx| + |ty - cy| + 4 over a square of half width WindowSize / 16:
    at most 2 * 3 + 4 = 10 at window 48.  The wide part of stage 3: half width WindowSize / 2, at most 48 + 4 = 52.
    Stage 2: |tx - genx| + |ty - geny| + 4 with |tx| + |ty| <= 279, at most 283 + |genx| + |geny|.
    Hence: local metrics <= 10 * 81600 = 816000 < 2^21 (a selection with 33 local candidates in 33 lanes has T0 < 2^21);
    stage 3 <= 52 * 81600 < 2^26; stage 2 < 2^26 AS LONG AS the centre is at most 1715 samples (L1) from the block.  That
    is all this test checks about stage 2.  That every centre is that near in a picture with W + H <= 1715 is an argument,
    not a check: a centre is a predictor >> 2, a median of final vectors, and every candidate of every stage is a block
    whose origin lies inside the picture (the searches drop the others; stage 2 walks picture positions), so no component
    is longer than the picture.  test_model_equals_the_oracle_and_routes_are_reached checks both halves on the oracle's
    recording of the new pairs (every listed vector inside, every centre within W + H), no more.  In a larger picture --
    the benchmark's 1080p is one -- a metric >= 2^26 needs a predictor longer than 1715 samples; nothing shows that it
    cannot happen there, no test codes it, and select_topk_ex keeps its guard for it."""
    full = []
    for s0, k0 in itertools.product((0, 16320), repeat=2):
        for hs in itertools.product(*[(max(0, s0 - 8160), min(s0, 8160))] * 4):
            for hk in itertools.product(*[(max(0, k0 - 8160), min(k0, 8160))] * 4):
                full.append(_dist((s0,) + hs, (k0,) + hk))
    assert len(full) == 1024
    D_MAX, D_WALK = max(full), 180 + 2 * (99 + 99 + 180) + 2 * 16320
    assert D_MAX == 5 * 16320 == 81600 and D_WALK == 33576
    # the walk's bound, tried on the vertices of its own constraints around extreme sums
    for s0, j, e1, e2 in itertools.product((180, 8160, 16140), (-180, 180), (-99, 99), (-99, 99)):
        a = s0 + j
        half = lambda t: (max(0, t - 8160), min(t, 8160))  # the ends of a half sum's range in a block of sum t
        for s3, s4 in itertools.product(half(s0), repeat=2):
            for k3, k4 in itertools.product(half(a), repeat=2):
                s = (s0, s0 // 2, s0 // 2, s3, s4)
                assert _dist(s, (a, s[1] + e1, s[2] + e2, k3, k4)) <= D_WALK
    for window in (16, 32, 48):
        w_local, w_wide = 2 * (window // 16) + 4, 2 * (window // 2) + 4
        assert w_local <= 10 and w_wide <= 52
        assert w_local * D_MAX < 1 << 21, "a local metric can reach 2^21"
        assert w_wide * D_MAX < 1 << 26
    assert 10 * D_MAX == 816000
    far = ((1 << 26) - 1) // D_WALK - 283  # the longest centre (L1) at which no stage-2 metric reaches 2^26
    assert far == 1715 and (283 + far) * D_WALK < 1 << 26
    for W, H, _ in rc.PAIRS.values():
        assert W + H <= far
    print("bounds: D_MAX", D_MAX, "D_WALK", D_WALK, "weights: local 10, wide 52, stage 2 283 + |centre|; stage 2 < 2^26 up to |centre| =", far)
