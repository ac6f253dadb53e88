"""Does the panned content (tests/pan_content.py) reach long vectors?  Decided on the CPU oracle alone.

test_gpu_pan.py compares the device with the oracle on these very runs; that comparison is worth what the oracle exercises, so
this test pins the generator (against a sample-serial restatement of its definition, to 1..255, to the absence of sum-0 blocks)
and counts, per named sequence, what the oracle's P pictures reach: long vectors, long predictors, reference blocks that hang
over the right and bottom edges, long vector differences, macroblock types, P_Skip macroblocks with a long derived vector,
speculation hits and misses of the list model, and the largest level.  A "partition" is one 8x8 quadrant of a macroblock, the
unit interEncoding searches (nmb * 4 a picture).  The conditions on the far sequences are conditions on the generator: change
seeds or content if one is missed, never the condition.  The other floors are about one fifth of the measured counts (DESIGN.md,
"panned content", holds them).  The same counters on gen_frame() and on a shifted mosaic are printed beside them.

Further down: every oracle run of test_gpu_pan.py stays under the level guard (2063) and off the sum-0 bucket layout; the streams
its decoder tests use decode, on the reference decoder, to the encoder's reconstruction; and the list model of me_model.py gives the
oracle's recorded lists at the oracle's own far centres on the pairs the GPU list tests run.
"""
import hashlib

import numpy as np
import pytest

import pan_content as pc
from me_model import model_for, predict_8x8

MAX_LEVEL = 2063
M64 = (1 << 64) - 1
P_TYPES = {"P_L0_16x16": (0,), "P_L0_L0_16x8": (1,), "P_L0_L0_8x16": (2,), "P_8x8": (3, 4), "P_Skip": (31,)}
MD5 = {"qcif_se40": "1ac6664cc75469b133beaf04e66ddb84", "tall": "5c44bd4989453cae428ec5b81ad8c51b"}   # all pictures of the sequence


# ---------------------------------------------------------------- the generator
def _lcg1(s):
    return (s * 6364136223846793005 + 1442695040888963407) & M64


def _mix1(z):
    z = _lcg1(z)
    z ^= z >> 29
    return _lcg1(z) >> 33


def _master1(plane, seed, X, Y):
    """the docstring of pan_content.py, one sample at a time, in Python integers"""
    s0 = _lcg1((seed ^ 0x9E3779B97F4A7C15) & M64)
    v = 128
    for k in range(4):
        B, A = pc.BLOCK[plane][k], pc.AMP[plane][k]
        key = _lcg1((s0 + 8 * plane + k) & M64)
        cell = (((Y // B) & 0xFFFFF) << 20) | ((X // B) & 0xFFFFF)   # Python's // floors, also below zero
        v += _mix1((key + cell) & M64) % A - (A - 1) // 2
    return min(max(v, 1), 255)


@pytest.mark.parametrize("offset", [(0, 0), (-37, 21), (181, -61)])
def test_generator_equals_its_definition(offset):
    W, H, seed = 16, 12, 11
    ox, oy = offset
    got = pc.picture(W, H, seed, offset)
    want = []
    for plane, n, pw, ph in ((0, 2, W, H), (1, 4, W // 2, H // 2), (2, 4, W // 2, H // 2)):
        for r in range(ph):
            for c in range(pw):
                s = sum(_master1(plane, seed, ox + n * c + i, oy + n * r + j) for j in range(n) for i in range(n))
                want.append((s + n * n // 2) >> (2 if n == 2 else 4))
    assert got.tolist() == want


def test_generator_is_pinned():
    for name, md5 in MD5.items():
        assert hashlib.md5(pc.frames(name).tobytes()).hexdigest() == md5, name
    # a window that moves by whole luma samples shows the same samples, moved
    W, H = 64, 48
    a, b = pc.picture(W, H, 3, (0, 0)), pc.picture(W, H, 3, (24, -16))
    ya, yb = a[:W * H].reshape(H, W), b[:W * H].reshape(H, W)
    assert np.array_equal(ya[:H - 8, 12:], yb[8:, :W - 12])
    ca, cb = a[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), b[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)
    assert np.array_equal(ca[:H // 2 - 4, 6:], cb[4:, :W // 2 - 6])
    assert not np.array_equal(pc.picture(W, H, 3, (1, 0)), a)


def _block_sums(y, W, H):
    """sums of all 8x8 blocks of a luma plane at every position (the feature the bucket table is sorted by)"""
    c = np.zeros((H + 1, W + 1), np.int64)
    c[1:, 1:] = y.reshape(H, W).astype(np.int64).cumsum(0).cumsum(1)
    return c[8:, 8:] - c[:-8, 8:] - c[8:, :-8] + c[:-8, :-8]


@pytest.mark.parametrize("name", sorted(pc.SEQS))
def test_sources_stay_in_range_and_off_the_sum_0_layout(fo, name):
    W, H, _, _ = pc.SEQS[name]
    f = pc.frames(name)
    assert f.min() >= 1 and f.max() <= 255
    for r in pc.oracle_run(fo, name, record=True):
        assert _block_sums(r["recon"][:W * H], W, H).min() > 0, "a sum-0 block would put the stream on the mis-filed bucket layout"
    for p in f:
        assert _block_sums(p[:W * H], W, H).min() > 0


# ---------------------------------------------------------------- what the oracle reaches
def _count_picture(fo, r, prev, cur, W, H, window, model):
    """counters of one P picture r coded after `prev` (the previous picture's dict) from source picture cur"""
    mbw = W // 16
    mt, mv, me = r["mb_type"], r["mv"], r["me"]
    assert np.isin(mt, (0, 1, 2, 3, 4, 31)).all()
    c = dict(parts=mt.size * 4, gt64=0, gt256=0, maxv=0, maxmvp=0, hangs=0, mvd255=0, maxmvd=0, skip_nz=0, skip_gt64=0, hit=0, miss=0,
             types={k: int(np.isin(mt, v).sum()) for k, v in P_TYPES.items()}, max_level=r["max_level"])
    for mb in range(mt.size):
        skip = mt[mb] == pc.P_SKIP
        if skip:
            v = tuple(int(x) for x in mv[mb, 0])
            assert (mv[mb] == mv[mb, 0]).all() and v == pc.skip_vector(mv, mbw, mb), ("the P_Skip rule", mb)
            c["skip_nz"] += v != (0, 0)
            c["skip_gt64"] += max(abs(v[0]), abs(v[1])) > 64
            continue
        for q in range(4):
            vx, vy = (int(x) for x in mv[mb, q])
            a = max(abs(vx), abs(vy))
            c["gt64"] += a > 64
            c["gt256"] += a > 256
            c["maxv"] = max(c["maxv"], a)
            x1 = (mb % mbw) * 16 + (q & 1) * 8 + (vx >> 2) + 8 + ((vx & 3) != 0)
            y1 = (mb // mbw) * 16 + (q >> 1) * 8 + (vy >> 2) + 8 + ((vy & 3) != 0)
            c["hangs"] += x1 > W or y1 > H
    searched = np.flatnonzero(me["searched"])
    assert set(searched // 4) == set(np.flatnonzero(mt != pc.P_SKIP)), "searched macroblocks are the ones that are not P_Skip"
    c["maxmvp"] = int(np.abs(me["mvp"][searched]).max()) if searched.size else 0
    d = np.abs(pc.mvd_of(mv, mt, mbw))
    c["mvd255"] = int((d > 255).sum())
    c["maxmvd"] = int(d.max())
    if model:
        # k_me_spec's guess: the predictor rules over V0, the first entry of smallest SAD of every partition's stage-3 list
        m = model_for(fo, prev["recon"], cur, W, H, window)
        v0 = np.zeros((mt.size * 4, 2), np.int64)
        for p in range(mt.size * 4):
            if me["searched"][p]:
                n = int(me["n"][p, 2])
                vx, vy, sad = me["bx"][p, 2, :n], me["by"][p, 2, :n], me["sad"][p, 2, :n]
            else:
                l = m.stage3(p)
                vx, vy, sad = l["vx"], l["vy"], l["sad"]
            if len(sad):
                k = int(np.argmin(sad))
                v0[p] = (vx[k], vy[k])
        for p in searched:
            gx, gy = predict_8x8(v0, mbw, int(p))
            hit = (gx >> 2, gy >> 2) == (int(me["mvp"][p, 0]) >> 2, int(me["mvp"][p, 1]) >> 2)
            c["hit" if hit else "miss"] += 1
    return c


_counts = {}
SUMS = ("gt64", "gt256", "hangs", "mvd255", "skip_nz", "skip_gt64", "hit", "miss")
MAXES = ("maxv", "maxmvp", "maxmvd", "max_level")


def _count_frames(fo, tag, pics, W, H, window, run=None):
    """per P picture the counters, and their totals over the run (sums, maxima, macroblock types)"""
    run = run or pc.oracle_frames(fo, W, H, pics, 12, window, 3, record=True)
    cs = [_count_picture(fo, run[t], run[t - 1], pics[t], W, H, window, True) for t in range(1, len(run))]
    tot = {k: sum(c[k] for c in cs) for k in SUMS}
    tot.update({k: max(c[k] for c in cs) for k in MAXES})
    tot.update({k: sum(c["types"][k] for c in cs) for k in P_TYPES})
    for t, c in enumerate(cs):
        print("pan", tag, "window", window, "picture", t + 1, c)
    print("pan", tag, "window", window, "total", tot)
    return cs, tot


def _counts_of(fo, name, window=16):
    if (name, window) not in _counts:
        W, H, _, _ = pc.SEQS[name]
        _counts[(name, window)] = _count_frames(fo, name, pc.frames(name), W, H, window, pc.oracle_run(fo, name, 12, window, 3, record=True))
    return _counts[(name, window)]


@pytest.mark.parametrize("name,window", [(n, 16) for n in pc.FAR] + [("qcif_se40", 32)])
def test_far_sequences_reach_long_vectors(fo, name, window):
    """The conditions every far sequence must meet.  "Half of the partitions of every P picture": of all nmb * 4 partitions, those
    of P_Skip macroblocks counted with their derived vector; and of the partitions the oracle searched, half on their own."""
    cs, tot = _counts_of(fo, name, window)
    for t, c in enumerate(cs):
        assert 2 * (c["gt64"] + 4 * c["skip_gt64"]) >= c["parts"], (name, t + 1, "fewer than half of the partitions exceed 64 quarter samples", c)
        assert 2 * c["gt64"] >= c["parts"] - 4 * c["types"]["P_Skip"], (name, t + 1, "fewer than half of the searched partitions exceed 64", c)
    assert tot["max_level"] <= MAX_LEVEL
    assert tot["gt256"] >= 20, (name, "partitions above 256 quarter samples")
    assert tot["skip_gt64"] >= 1, (name, "no P_Skip macroblock with a vector above 64 quarter samples")
    if name in ("tall", "wide"):
        assert tot["maxv"] > 800, (name, "no component above 800 quarter samples")


# About one fifth of what the oracle reaches at QP 12, window 16 over the P pictures of each sequence (sums, and the maxima maxv,
# maxmvp, maxmvd); DESIGN.md holds the measured figures.  Conditions on the generator: change seeds or content, never a floor.
FLOORS = {
    "qcif_se40": {"gt64": 167, "gt256": 28, "hangs": 17, "mvd255": 18, "skip_nz": 12, "skip_gt64": 12, "hit": 4, "miss": 181, "maxv": 134, "maxmvp": 89, "maxmvd": 108, "P_L0_16x16": 10, "P_8x8": 35, "P_Skip": 12},
    "qcif_nw40": {"gt64": 103, "gt256": 36, "hangs": 3, "mvd255": 22, "skip_nz": 26, "skip_gt64": 26, "hit": 11, "miss": 121, "maxv": 125, "maxmvp": 123, "maxmvd": 132, "P_L0_16x16": 7, "P_8x8": 25, "P_Skip": 26},
    "qcif_ne90": {"gt64": 186, "gt256": 126, "hangs": 22, "mvd255": 36, "skip_nz": 6, "skip_gt64": 6, "hit": 4, "miss": 207, "maxv": 119, "maxmvp": 114, "maxmvd": 130, "P_L0_16x16": 10, "P_8x8": 42, "P_Skip": 6},
    "qcif_sw90": {"gt64": 149, "gt256": 87, "hangs": 21, "mvd255": 32, "skip_nz": 11, "skip_gt64": 11, "hit": 8, "miss": 183, "maxv": 138, "maxmvp": 116, "maxmvd": 138, "P_L0_16x16": 6, "P_8x8": 41, "P_Skip": 11},
    "tall": {"gt64": 235, "gt256": 180, "hangs": 48, "mvd255": 35, "skip_nz": 4, "skip_gt64": 4, "hit": 9, "miss": 261, "maxv": 220, "maxmvp": 218, "maxmvd": 297, "P_L0_16x16": 13, "P_8x8": 54, "P_Skip": 4},
    "wide": {"gt64": 243, "gt256": 201, "hangs": 49, "mvd255": 32, "skip_nz": 4, "skip_gt64": 4, "hit": 6, "miss": 265, "maxv": 211, "maxmvp": 197, "maxmvd": 296, "P_L0_16x16": 15, "P_8x8": 52, "P_Skip": 4},
    "qcif_near_in": {"gt64": 10, "gt256": 5, "hangs": 4, "mvd255": 7, "skip_nz": 28, "hit": 27, "miss": 16, "maxv": 105, "maxmvp": 102, "maxmvd": 110, "P_L0_16x16": 3, "P_8x8": 7, "P_Skip": 28},
    "qcif_near_out": {"gt64": 53, "gt256": 5, "hangs": 8, "mvd255": 4, "skip_nz": 25, "skip_gt64": 25, "hit": 1, "miss": 55, "maxv": 121, "maxmvp": 72, "maxmvd": 107, "P_L0_16x16": 9, "P_8x8": 5, "P_Skip": 25},
    "qcif_still_pan": {"gt64": 85, "gt256": 16, "hangs": 16, "mvd255": 15, "skip_nz": 13, "skip_gt64": 13, "hit": 20, "miss": 100, "maxv": 116, "maxmvp": 100, "maxmvd": 112, "P_L0_16x16": 12, "P_8x8": 18, "P_Skip": 49},
    "small": {"gt64": 1, "hangs": 2, "hit": 4, "miss": 2, "maxv": 24, "maxmvp": 20, "maxmvd": 20, "P_8x8": 1},
}


@pytest.mark.parametrize("name", pc.NAMED)
def test_sequences_reach_their_floors(fo, name):
    _, tot = _counts_of(fo, name, 16)
    assert tot["max_level"] <= MAX_LEVEL
    for k, floor in FLOORS[name].items():
        assert tot[k] >= floor, (name, k, tot[k], floor)
    if name == "qcif_still_pan":   # still, pan, pan, still: all P_Skip, long vectors, long vectors, and no vector left over
        cs = _counts_of(fo, name, 16)[0]
        assert cs[0]["types"]["P_Skip"] == 99 and cs[0]["skip_nz"] == 0
        assert cs[1]["gt64"] >= 45 and cs[2]["gt64"] >= 39 and cs[1]["skip_gt64"] >= 7 and cs[2]["skip_gt64"] >= 6   # of 229, 199, 36, 30
        assert cs[3]["types"]["P_Skip"] >= 16 and cs[3]["skip_nz"] == 0 and cs[3]["maxv"] == 0   # of 80


@pytest.mark.parametrize("case", pc.ENC_CASES, ids=pc.case_id)
def test_gpu_cases_stay_under_the_guards(fo, case):
    """every oracle run test_gpu_pan.py compares with: levels the CAVLC writer is pinned for, no sum-0 block in a reference picture"""
    names, qp, window, maxdiff = case
    for name in names:
        W, H, _, _ = pc.SEQS[name]
        run = pc.oracle_run(fo, name, qp, window, maxdiff)
        assert all(len(r["rbsp"]) > 0 for r in run)
        assert max(r["max_level"] for r in run) <= MAX_LEVEL, name
        for r in run:
            assert _block_sums(r["recon"][:W * H], W, H).min() > 0, name
    if names == pc.MANY:
        mv = [max(int(np.abs(r["mv"]).max()) for r in pc.oracle_run(fo, n, qp, window, maxdiff)[1:]) for n in names]
        print("pan many: largest component per stream", mv)
        assert mv[5] == 0 and mv[11] == 0 and sum(v > 64 for v in mv) >= 8


@pytest.mark.parametrize("name", pc.DEC_CASES)
def test_decoder_cases_decode_to_the_reconstruction(fo, name):
    run = pc.oracle_run(fo, name)
    for r in run[1:]:
        assert not ((r["mb_type"] != pc.P_SKIP) & (r["cbp"] == 0).all(1)).any(), "a coded macroblock of CBP 0: the reference decoder leaves the encoder's picture"
    n, dec, _ = fo.decode_stream_md5(pc.oracle_stream(fo, name))
    assert n == len(run)
    for d, r in zip(dec, run):
        assert np.array_equal(d, r["recon"])


@pytest.mark.parametrize("name,window", [("qcif_se40", 16), ("qcif_se40", 32), ("wide", 16)])
def test_model_lists_equal_the_oracle_at_far_centres(fo, name, window):
    """test_me_model_host.py's comparison on the pairs test_gpu_pan.py runs the list tests on: the list model is the reference of
    the GPU lists at guessed centres, so it must first give the oracle's own lists at the oracle's own, far, centres"""
    from me_model import oracle_pair
    from test_me_model_host import assert_list
    W, H = pc.SEQS[name][:2]
    f0, f1 = pc.frames(name)[:2]
    rec0, rec, mbt, mv, _ = oracle_pair(fo, f0, f1, W, H, window, 3)
    m = model_for(fo, rec0, f1, W, H, window)
    searched = np.flatnonzero(rec["searched"])
    assert searched.size >= 4 * 50
    far = 0
    for p in (int(v) for v in searched):
        mvpx, mvpy = (int(v) for v in rec["mvp"][p])
        far += max(abs(mvpx), abs(mvpy)) > 64
        assert m.sums(p) == rec["suma"][p].tolist(), (name, p)
        assert predict_8x8(mv.reshape(-1, 2), W // 16, p) == (mvpx, mvpy), (name, p)
        assert_list(m.stage3(p), rec, p, 2, "stage 3")
        assert_list(m.stage1(p, mvpx >> 2, mvpy >> 2), rec, p, 0, "stage 1")
        assert_list(m.stage2(p, mvpx >> 2, mvpy >> 2), rec, p, 1, "stage 2")
    print("pan", name, "window", window, "searched partitions", searched.size, "with a predictor above 64 quarter samples", far)
    assert 2 * far >= searched.size


def test_the_older_content_stays_short(fo, pkg):
    """the same counters on the pictures every other encoder parity test draws from: gen_frame() and the shifted mosaics"""
    import hard_content as hc
    W, H = 176, 144
    _, smooth = _count_frames(fo, "gen_frame", np.stack([pkg.gen_frame(W, H, t, 1234, 2) for t in range(4)]), W, H, 16)
    _, hard = _count_frames(fo, "mosaic", hc.sequence(W, H, 5), W, H, 16)
    assert smooth["maxv"] <= 64 and smooth["gt64"] == 0 and smooth["skip_gt64"] == 0
    assert hard["skip_gt64"] == 0
