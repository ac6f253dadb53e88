"""(reference, source) picture pairs that reach the data-dependent routes of the motion search no other content reaches.

Every pair is handed to the search directly -- the reference through set_reference (the oracle's set_dpb), the source
through set_frames -- so the feature sums are the ones written here, not blurred by a coded reconstruction.  All pairs
run with MAXDIFF 0: a macroblock is P_Skip only where the source equals its prediction, so every macroblock touched below
is searched.  Chroma is flat 128 unless the pair pans.  No 8x8 window of any reference sums to 0.

far_mismatch(variant)   stage-2 metrics around and above 2^21 (select_topk_ex: the T0 guard and the general route).
    The reference is flat 100 with isolated 8x8 tiles lit (255 over 0) on rows {2, 3, 6, 7}; the source is flat 100 with
    ONE probe partition lit on rows {0, 1, 4, 5}.  Probe and tile agree in the sum and both half sums and differ in the
    row feature alone: D = 16320 exactly, while every window that only overlaps a tile is more than 180 away from the
    probe's sum 8160.  So the walk's candidates are the tiles, twice each (bucket su[0] is visited from both sides), and
    the metric of a tile at L1 distance r from the centre (0, 0) is (r + 4) * 16320: 2088960 at r = 124, 2105280 at
    r = 125, 2^21 = 2097152 between them.
      "below"    17 tiles at r <= 124, the farthest of them AT 124, and tiles from 125 on: 34 candidates below 2^21, the
                 33rd smallest metric just below it (T0 = 2088960, the fast route at its edge)
      "above"    16 tiles at r <= 124, one AT 124, and tiles from 125 on: the 33rd smallest is 2105280, T0 = 1 << 21 with
                 metrics on both sides in the registers
      "all_far"  every tile at r >= 125, one AT 125, seen from a probe in the picture's corner
many_flats()     cause (a) of the crowded fallback: five flat bands 98..102, each far more than 1024 positions, whose
    buckets lie 0, 64 and 128 from the probe's sum.  The probes (bright over dark halves, 109 / 91) fail the walk's
    half-sum test against every flat position, so the walk passes all five buckets and stops at step 160 in a band tiled
    with rows 111 / 94, period 8, whose windows of three of the eight phases pass.
noisy_bucket()   cause (b): a flat area of level 100 left of an area tiled with a zero-sum pattern of period 8 in both
    directions.  All windows sum to 6400; the flat ones are the modal class, the thousands of tiled ones are outside it.
    Every macroblock's first partition has one sample raised by 5: bucket 6400 is five steps away, hence big.
many_listed()    cause (c) with no big bucket: flat squares of fewer than 1024 positions in a textured picture, one sample
    of every macroblock's first partition raised by 5: the square's bucket is small, read and listed, and too long.
panned(kind)     "listed" / "noisy" above inside a texture, the source being the reference seen PAN samples further down
    right: the neighbours' vectors, hence the centres of the crowded partitions, are dozens of samples long.
wide_noisy()     noisy_bucket at 272 x 48: as wide as crowded_summary's claims go.
"""
import numpy as np

import pan_content

QCIF = (176, 144)
PAN = (36, 20)
PROBE_ROWS, TILE_ROWS = [0, 1, 4, 5], [2, 3, 6, 7]
FAR_PROBE = {"below": (80, 64), "above": (80, 64), "all_far": (8, 8)}


def pack(y, cb=None, cr=None):
    H, W = y.shape
    c = np.full((H // 2, W // 2), 128, np.uint8)
    return np.concatenate([y.astype(np.uint8).ravel(), (c if cb is None else cb).astype(np.uint8).ravel(), (c if cr is None else cr).astype(np.uint8).ravel()])


def far_tiles(variant):
    """tile origins of far_mismatch(variant), and the probe's origin"""
    W, H = QCIF
    px, py = FAR_PROBE[variant]
    # a 24-sample lattice through the probe, the probe's own neighbourhood left out
    slots = [(x, y) for y in range(py % 24, H - 7, 24) for x in range(px % 24, W - 7, 24) if max(abs(x - px), abs(y - py)) >= 24]
    r = lambda t: abs(t[0] - px) + abs(t[1] - py)
    if variant == "all_far":
        tiles = [t for t in slots if r(t) >= 125] + [(px + 101, py + 24)]  # the last one off the lattice: r = 125
    else:
        near = sorted((t for t in slots if r(t) <= 120), key=lambda t: (r(t), t))[:16 if variant == "below" else 15]
        far = [t for t in slots if r(t) >= 140]
        # off the lattice, 12 samples from its rows: r = 124 and r = 125
        tiles = near + [(px - 64, py + 60), (px + 65, py + 60)] + far
    assert all(0 <= x <= W - 8 and 0 <= y <= H - 8 for x, y in tiles)
    assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 12 for i, a in enumerate(tiles) for b in tiles[:i]), "tiles too close"
    return tiles, (px, py)


def far_mismatch(variant):
    W, H = QCIF
    tiles, (px, py) = far_tiles(variant)
    ref = np.full((H, W), 100, np.uint8)
    for x, y in tiles:
        ref[y:y + 8, x:x + 8] = 0
        ref[[y + k for k in TILE_ROWS], x:x + 8] = 255
    src = np.full((H, W), 100, np.uint8)
    src[py:py + 8, px:px + 8] = 0
    src[[py + k for k in PROBE_ROWS], px:px + 8] = 255
    return pack(ref), pack(src)


def _raise_one_sample(y, by=5):
    """one sample of the first partition of every macroblock, at a place that moves with the macroblock"""
    H, W = y.shape
    out = y.copy()
    for my in range(H // 16):
        for mx in range(W // 16):
            r, c = my * 16 + (mx + 2 * my) % 8, mx * 16 + (3 * mx + my) % 8
            out[r, c] = min(int(out[r, c]) + by, 255)
    return out


def many_flats():
    W, H = QCIF
    ref = np.empty((H, W), np.uint8)
    for k, v in enumerate((98, 99, 100, 101, 102)):
        ref[k * 20:(k + 1) * 20] = v
    rows = np.arange(100, H)
    ref[100:] = np.where((rows - 100) % 8 < 4, 111, 94)[:, None]
    src = ref.copy()
    for mx, my in ((2, 1), (5, 2), (8, 3), (4, 4), (7, 0)):  # probes in the first partition of a few macroblocks
        src[my * 16:my * 16 + 4, mx * 16:mx * 16 + 8] = 109
        src[my * 16 + 4:my * 16 + 8, mx * 16:mx * 16 + 8] = 91
    return pack(ref), pack(src)


_A = np.array([6, 6, 2, 2, -2, -2, -6, -6])
_B = np.array([5, -5, 3, -3, 1, -1, 4, -4])


def _noisy(W, H, xs):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where(xx < xs, 100, 100 + _A[yy % 8] + _B[xx % 8]).astype(np.uint8)


def noisy_bucket():
    ref = _noisy(*QCIF, 112)
    return pack(ref), pack(_raise_one_sample(ref))


def wide_noisy():
    ref = _noisy(272, 48, 160)
    return pack(ref), pack(_raise_one_sample(ref))


def _texture(W, H, seed):
    f = pan_content.picture(W, H, seed, (0, 0))
    return f[:W * H].reshape(H, W).copy(), f[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), f[W * H * 5 // 4:].reshape(H // 2, W // 2)


def many_listed():
    W, H = QCIF
    ref, cb, cr = _texture(W, H, 21)
    ref[24:54, 40:70] = 100
    ref[80:110, 100:130] = 140
    return pack(ref, cb, cr), pack(_raise_one_sample(ref), cb, cr)


def panned(kind):
    """the reference is the top left window of a canvas, the source the window PAN further down right"""
    W, H = QCIF
    dx, dy = PAN
    y, cb, cr = _texture(W + 48, H + 32, 22 if kind == "listed" else 23)
    if kind == "listed":
        y[50:80, 70:100] = 100
        y[100:130, 130:160] = 140
    else:
        assert kind == "noisy"
        yy, xx = np.mgrid[0:y.shape[0], 0:y.shape[1]]
        area = (yy >= 40) & (xx >= 60) & (xx < 190)
        y[area] = np.where(xx < 130, 100, 100 + _A[yy % 8] + _B[xx % 8])[area]
    win = lambda a, x0, y0, w, h: a[y0:y0 + h, x0:x0 + w]
    ref = pack(win(y, 0, 0, W, H), win(cb, 0, 0, W // 2, H // 2), win(cr, 0, 0, W // 2, H // 2))
    src = pack(_raise_one_sample(win(y, dx, dy, W, H)), win(cb, dx // 2, dy // 2, W // 2, H // 2), win(cr, dx // 2, dy // 2, W // 2, H // 2))
    return ref, src


# name -> (W, H, generator); what each is for is asserted in test_route_content_host.py
PAIRS = {
    "far_below": (176, 144, lambda: far_mismatch("below")),
    "far_above": (176, 144, lambda: far_mismatch("above")),
    "far_all": (176, 144, lambda: far_mismatch("all_far")),
    "many_flats": (176, 144, many_flats),
    "noisy_bucket": (176, 144, noisy_bucket),
    "many_listed": (176, 144, many_listed),
    "pan_listed": (176, 144, lambda: panned("listed")),
    "pan_noisy": (176, 144, lambda: panned("noisy")),
    "wide_noisy": (272, 48, wide_noisy),
}
MAXDIFF = 0
_cache = {}
# what each pair must reach on at least one partition the oracle searched (none of them in a P_Skip macroblock), at
# windows 16 and 32: keys of analysis()["counts"]
REACHES = {
    "far_below": ("straddle",), "far_above": ("mixed_t0",), "far_all": ("general_t0",),
    "many_flats": ("a", "classes_off"), "noisy_bucket": ("b", "classes_off"), "many_listed": ("c", "rewalk"),
    "pan_listed": ("c", "rewalk", "far_rewalk"), "pan_noisy": ("b", "c", "far_rewalk", "far_classes_off"), "wide_noisy": ("b",),
}
_analysis = {}


def analysis(fo, name, window):
    """The oracle's P picture of a pair with recording, the list model of the pair, and the route predicates of every
    partition; computed once per (name, window) and shared, callers leave it unchanged.
      orc       oracle_pair_ref(): (reference, recorded lists, mb_type, mv, P_Skip count)
      model     the MeModel of (reference, source)
      routes    {p: MeModel.stage2_routes at the oracle's centre} for the searched partitions
      crowded   {p: MeModel.crowded_summary} for EVERY crowded partition (the walk does not depend on the neighbours)
      counts    over the partitions the oracle searched: how many hold each predicate; rewalk / classes_off = a decided
                fallback with nbig == 0 / > 0 (the two consumers of the bit); far_* = the same at a centre more than
                16 samples (L1) out; far_crowded; max_metric"""
    key = (name, window)
    if key in _analysis:
        return _analysis[key]
    from me_model import model_for, oracle_pair_ref
    W, H, _ = PAIRS[name]
    ref, src = pair(name)
    orc = oracle_pair_ref(fo, ref, src, W, H, window, MAXDIFF)
    rec, mbt = orc[1], orc[2]
    m = model_for(fo, ref, src, W, H, window)
    cnt = dict(searched=0, general_t0=0, straddle=0, mixed_t0=0, crowded=0, undecided=0, a=0, b=0, c=0, rewalk=0, classes_off=0,
               far_crowded=0, far_rewalk=0, far_classes_off=0, max_metric=0)
    routes, crowded = {}, {}
    for p in range(4 * (W // 16) * (H // 16)):
        cand = m.stage2_candidates(p)
        if cand[0].size > 384:
            crowded[p] = m.crowded_summary(p)
        if not rec["searched"][p]:
            continue
        assert mbt[p // 4] != pan_content.P_SKIP
        cnt["searched"] += 1
        gx, gy = int(rec["mvp"][p, 0]) >> 2, int(rec["mvp"][p, 1]) >> 2
        r = routes[p] = m.stage2_routes(p, gx, gy, cand)
        for k in ("general_t0", "straddle", "mixed_t0"):
            cnt[k] += r[k]
        cnt["max_metric"] = max(cnt["max_metric"], r["max_metric"])
        if p in crowded:
            cs, far = crowded[p], abs(gx) + abs(gy) > 16
            cnt["crowded"] += 1
            cnt["far_crowded"] += far
            if cs["undecided"]:
                cnt["undecided"] += 1
                continue
            for k in "abc":
                cnt[k] += cs[k]
            if cs["fallback"]:
                k = "rewalk" if cs["nbig"] == 0 else "classes_off"
                cnt[k] += 1
                cnt["far_" + k] += far
    _analysis[key] = dict(orc=orc, model=m, routes=routes, crowded=crowded, counts=cnt)
    return _analysis[key]


def pair(name):
    """(reference, source) of PAIRS[name]; computed once and shared, callers leave them unchanged"""
    if name not in _cache:
        _cache[name] = PAIRS[name][2]()
    return _cache[name]
