"""The lists the four motion kernels hand each other, stage by stage, against the oracle's recording and the list model.

Set up like test_inter_decision_matches_oracle: reference = the oracle's reconstruction of picture 0, source = picture
1, one inter_encoding() call, status() == [0].  Every comparison is exact equality.

  k_me_pre      SUMA, ST3N and ST3[0, ST3N) == the oracle's recorded stage-3 list for every partition of a macroblock the
                oracle searched, == the model (me_model.py, itself pinned against the oracle on the host) for the others;
                V0 == the first entry of smallest SAD.  No partition is left out.
  k_me_spec     the guessed centre of EVERY partition == the predictor rules applied to the neighbours' V0, >> 2; where
                the header says lists were written, SPEC_L1 / SPEC_L2 == the model at that centre, and == the oracle's
                recording where the centre is the true one.  Partitions without lists (guessed P_Skip) are counted
                against the caps below.
  k_me_resolve  the final vector of every searched partition == the ordered first minimum of SAD + |mv - mvp| over the
                three GPU lists where the centre was a hit, == the oracle's vector where it was a miss; without
                speculation MV / MVD / types / ST3 are the same.

Caps on partitions without k_me_spec lists (the oracle's own P_Skip counts behind them are pinned on the host,
test_me_model_host.py), by content kind and at every window, 48 included: "textured", "patch" 5 %; "letterbox",
"flat-half" 50 %; "soft" 50 % at MAXDIFF 0.  The wide low picture ("thirds": two thirds of it flat, hence P_Skip) and
the tiny pictures are content kinds the caps do not name; they must have lists on at least one partition.

Routes.  Each predicate is computed from the MODEL (MeModel.route_predicates: sufficient conditions that do not depend on
which lane holds which candidate) and must hold on at least one compared partition of the named QCIF content:
  pruned wide search of k_me_pre                        every kind
  full evaluation by > 128 bound survivors              letterbox, patch
  selection refuses (> 64 survivors)                    flat-half, letterbox, patch
  tie at the list's end decided by arrival              every kind
  a speculation miss (guessed centre != mvp >> 2)       see MISS_KINDS
  a crowded partition (ST2N > 384) with lists           see CROWDED_KINDS
Not reached by THIS content: T0 >= 2^21 in select_topk_ex and the `fallback` bit of a crowded summary; the pairs of
route_content.py reach both, with predicates that need no lane layout (MeModel.stage2_routes, crowded_summary), and
test_gpu_me_routes.py compares them.  A metric >= 2^26 is out of reach while the centre is at most 1715 samples from the
block (test_route_content_host.py::test_metric_bounds; in larger pictures the guard stays live and unreached).  T infinite in k_me_pre (fewer than 33 lanes with a local candidate)
stays unreached: no legal picture gives it, by the lane argument of test_gpu_me_pre_paths.py.
"""
import numpy as np
import pytest
from me_model import KINDS, MAXDIFF, model_for, oracle_pair, predict_8x8, unpack_xy
from test_gpu_walk_dense import _content

pytestmark = pytest.mark.gpu

CAP = 384  # FER_ST2_CAP
NOLIST_CAP = {"textured": 0.05, "patch": 0.05, "letterbox": 0.5, "flat-half": 0.5, "soft": 0.5}
ROUTE_KINDS = {"pruned": KINDS, "full128": ["letterbox", "patch"], "refuse64": ["flat-half", "letterbox", "patch"], "tie_end": KINDS}
# where the model (guess from the model's own v0 against the oracle's predictor; walk count) finds the case on the CPU
MISS_KINDS = KINDS
CROWDED_KINDS = ["patch"]  # the crowded partitions of "letterbox" and "flat-half" lie in P_Skip macroblocks

READS = ("SUMA", "ST3", "ST3N", "V0", "SPEC_HDR", "SPEC_L1", "SPEC_L2", "MV", "MVD", "MBTYPE", "ST2N")
SHAPES = dict(SUMA=(4, 5), ST3=(4, 33, 3), ST3N=(4,), V0=(4,), SPEC_HDR=(4, 4), SPEC_L1=(4, 17, 2), SPEC_L2=(4, 33, 2), MV=(4, 2),
              MVD=(4, 2), MBTYPE=(), ST2N=(4,), ST2=(4, CAP, 2))


def frames_of(pkg, kind, W, H, seed=1234):
    """pictures 0 and 1 of a case; kind "pan:<name>": of that sequence of tests/pan_content.py"""
    if kind.startswith("pan:"):
        import pan_content
        assert (W, H) == pan_content.SEQS[kind[4:]][:2]
        return tuple(pan_content.frames(kind[4:])[:2])
    if (W, H) == (176, 144) and seed == 1234:
        return _content(pkg, kind, 0), _content(pkg, kind, 1)
    out = []
    for t in (0, 1):
        f = pkg.gen_frame(W, H, t, seed, 2).copy()
        y = f[: W * H].reshape(H, W)
        if kind == "thirds":  # two flat areas of different values around a textured one
            y[:, : W // 3] = 60
            y[:, 2 * W // 3:] = 200
        else:
            assert kind == "textured"
        out.append(f)
    return out


def gpu_state(pkg, W, H, window, maxdiff, rec0s, f1s, speculate=True, extra=()):
    """one inter_encoding() over len(f1s) streams -> per stream a dict of the read-backs (READS and `extra`), partitions
    flattened"""
    reads = READS + tuple(extra)
    S = len(f1s)
    g = pkg.FerHip(W, H, S, qp=12, window=window, maxdiff=maxdiff)
    if not speculate:
        g.tune(pkg.TUNE_SPECULATE, 0)
    nmb = (W // 16) * (H // 16)
    try:
        g.set_reference(np.stack(rec0s))
        g.set_frames(np.stack(f1s))
        g.inter_encoding()
        assert g.status() == [0] * S
        raw = {n: g.read(n).reshape((S, nmb) + SHAPES[n]) for n in reads}
    finally:
        g.close()
    out = []
    for s in range(S):
        st = {n: raw[n][s].astype(np.int64) for n in reads}
        for n in reads:
            if n != "MBTYPE":
                st[n] = st[n].reshape((nmb * 4,) + SHAPES[n][1:])
        out.append(st)
    return out


def first_min(lists, mvpx, mvpy):
    """eval_list over the lists in turn (F/moestimation.cpp:458-505): the first entry of smallest SAD + |mv - mvp|"""
    best, bx, by = 2000000000, 0, 0
    for vx, vy, sad in lists:
        for x, y, s in zip(vx, vy, sad):
            c = int(s) + abs(int(x) - mvpx) + abs(int(y) - mvpy)
            if c < best:
                best, bx, by = c, int(x), int(y)
    return bx, by


def check_stream(tag, st, rec, omv, m, W, H):
    """All list-level comparisons of one stream; -> counters (partitions, without lists, hits, misses, crowded with
    lists, and how many partitions each route predicate held on)."""
    mbw, mbh = W // 16, H // 16
    np4 = mbw * mbh * 4
    cnt = dict(parts=np4, nolist=0, hit=0, miss=0, crowded=0, pruned=0, full128=0, refuse64=0, tie_end=0)
    # ---- k_me_pre: every partition
    for p in range(np4):
        mod = m.stage3(p, routes=True)
        for r, on in mod["routes"].items():
            cnt[r] += on
        if rec["searched"][p]:
            n = int(rec["n"][p, 2])
            want = np.stack([rec["bx"][p, 2, :n], rec["by"][p, 2, :n], rec["sad"][p, 2, :n]], -1)
            assert st["SUMA"][p].tolist() == rec["suma"][p].tolist(), (tag, p, "suma")
        else:
            n = mod["n"]
            want = np.stack([mod["vx"], mod["vy"], mod["sad"]], -1)
            assert st["SUMA"][p].tolist() == m.sums(p), (tag, p, "suma")
        assert st["ST3N"][p] == n, (tag, p, "st3n", int(st["ST3N"][p]), n)
        got = st["ST3"][p, :n]
        assert np.array_equal(got, want), (tag, p, "st3", got.tolist(), want.tolist())
        v0 = (0, 0)
        if n:
            k = int(np.argmin(got[:, 2]))  # the first entry of smallest SAD
            v0 = (int(got[k, 0]), int(got[k, 1]))
        assert tuple(int(v) for v in unpack_xy(st["V0"][p])) == v0, (tag, p, "v0")
    # ---- k_me_spec
    v0f = np.stack(unpack_xy(st["V0"]), -1)
    hdr = st["SPEC_HDR"]
    for p in range(np4):
        gx, gy = (int(v) for v in unpack_xy(hdr[p, 0]))
        px, py = predict_8x8(v0f, mbw, p)
        assert (gx, gy) == (px >> 2, py >> 2), (tag, p, "guessed centre")
        flags = int(hdr[p, 1])
        if not (flags >> 16) & 1:
            cnt["nolist"] += 1
            continue
        c1, c2 = flags & 0xff, (flags >> 8) & 0xff
        searched = bool(rec["searched"][p])
        hit = searched and (gx, gy) == (int(rec["mvp"][p, 0]) >> 2, int(rec["mvp"][p, 1]) >> 2)
        cnt["crowded"] += int(st["ST2N"][p] > CAP)
        for name, got, cn, mod, li in (("l1", st["SPEC_L1"][p], c1, m.stage1(p, gx, gy), 0), ("l2", st["SPEC_L2"][p], c2, m.stage2(p, gx, gy), 1)):
            assert cn == mod["n"], (tag, p, name, cn, mod["n"])
            vx, vy = unpack_xy(got[:cn, 0])
            assert np.array_equal(vx, mod["vx"]) and np.array_equal(vy, mod["vy"]), (tag, p, name, "vectors", vx.tolist(), vy.tolist(), mod["vx"].tolist(), mod["vy"].tolist())
            assert np.array_equal(got[:cn, 1], mod["sad"]), (tag, p, name, "sad")
            if hit:
                assert cn == rec["n"][p, li], (tag, p, name, "count against the oracle")
                assert np.array_equal(vx, rec["bx"][p, li, :cn]) and np.array_equal(vy, rec["by"][p, li, :cn]) and \
                    np.array_equal(got[:cn, 1], rec["sad"][p, li, :cn]), (tag, p, name, "against the oracle")
        # ---- k_me_resolve: the final vector of a searched partition
        if searched:
            cnt["hit" if hit else "miss"] += 1
            fin = (int(st["MV"][p, 0]), int(st["MV"][p, 1]))
            if hit:
                n3 = int(st["ST3N"][p])
                lists = []
                for a, cn in ((st["SPEC_L1"][p], c1), (st["SPEC_L2"][p], c2)):
                    vx, vy = unpack_xy(a[:cn, 0])
                    lists.append((vx, vy, a[:cn, 1]))
                lists.append((st["ST3"][p, :n3, 0], st["ST3"][p, :n3, 1], st["ST3"][p, :n3, 2]))
                assert fin == first_min(lists, int(rec["mvp"][p, 0]), int(rec["mvp"][p, 1])), (tag, p, "resolve on a hit")
            else:
                assert fin == (int(omv[p, 0]), int(omv[p, 1])), (tag, p, "resolve on a miss")
    # searched partitions whose lists k_me_spec skipped: the chain searched them itself
    for p in np.nonzero(rec["searched"])[0]:
        if not (int(hdr[p, 1]) >> 16) & 1:
            assert (int(st["MV"][p, 0]), int(st["MV"][p, 1])) == (int(omv[p, 0]), int(omv[p, 1])), (tag, p, "resolve without lists")
    return cnt


def run_case(pkg, fo, kind, W, H, window, maxdiff, seeds=(1234,)):
    pairs = [frames_of(pkg, kind, W, H, s) for s in seeds]
    orc = [oracle_pair(fo, f0, f1, W, H, window, maxdiff) for f0, f1 in pairs]
    sts = gpu_state(pkg, W, H, window, maxdiff, [o[0] for o in orc], [f1 for _, f1 in pairs])
    total = None
    for s, (st, (rec0, rec, mbt, omv, _), (_, f1)) in enumerate(zip(sts, orc, pairs)):
        m = model_for(fo, rec0, f1, W, H, window)
        assert np.array_equal(st["MBTYPE"], mbt), (kind, s, "mb_type")
        c = check_stream((kind, W, H, window, s), st, rec, omv.reshape(-1, 2), m, W, H)
        print("me_lists", kind, W, H, window, "stream", s, c)
        total = c if total is None else {k: total[k] + c[k] for k in c}
    return total, sts, orc


@pytest.mark.parametrize("window", [16, 32])
@pytest.mark.parametrize("kind", KINDS)
def test_lists_qcif(pkg, fo, kind, window):
    c, _, _ = run_case(pkg, fo, kind, 176, 144, window, MAXDIFF.get(kind, 3))
    assert c["nolist"] <= NOLIST_CAP[kind] * c["parts"], (kind, c)
    for route, kinds in ROUTE_KINDS.items():
        if kind in kinds:
            assert c[route] > 0, (kind, route, "route not reached")
    if kind in MISS_KINDS:
        assert c["miss"] > 0, (kind, "no speculation miss among the compared partitions")
    if kind in CROWDED_KINDS:
        assert c["crowded"] > 0, (kind, "no crowded partition with lists")
    assert c["hit"] > 0, (kind, c)


@pytest.mark.parametrize("kind", ["textured", "flat-half"])
def test_lists_window_48(pkg, fo, kind):
    """WindowSize 48: the kernels' general code (feat_rec_direct, ordered insertion)"""
    c, _, _ = run_case(pkg, fo, kind, 176, 144, 48, 3)
    assert c["nolist"] <= NOLIST_CAP[kind] * c["parts"], (kind, c)
    assert c["hit"] > 0 and c["miss"] > 0, (kind, c)


def test_lists_wide_low_picture(pkg, fo):
    """1920 x 48 "thirds": the column range of the 280-diamond matters, flat areas overflow the candidate lists"""
    c, _, _ = run_case(pkg, fo, "thirds", 1920, 48, 32, 3)
    assert c["nolist"] < c["parts"] and c["hit"] > 0, c


@pytest.mark.parametrize("W,H", [(16, 16), (32, 16)])
def test_lists_tiny_pictures(pkg, fo, W, H):
    """every local search hangs over a picture edge"""
    c, _, _ = run_case(pkg, fo, "textured", W, H, 32, 0)
    assert c["nolist"] < c["parts"], c


def test_lists_three_streams(pkg, fo):
    """three streams of different seeds in one context: the per-stream indexing of the read-backs"""
    c, sts, _ = run_case(pkg, fo, "textured", 176, 144, 16, 3, seeds=(1234, 1235, 1236))
    assert c["parts"] == 3 * 396 and c["nolist"] <= 0.05 * c["parts"] and c["hit"] > 0, c
    assert not np.array_equal(sts[0]["ST3"], sts[1]["ST3"]) and not np.array_equal(sts[1]["ST3"], sts[2]["ST3"])


@pytest.mark.parametrize("kind,window", [("textured", 16), ("flat-half", 32)])
def test_without_speculation_nothing_changes(pkg, fo, kind, window):
    f0, f1 = frames_of(pkg, kind, 176, 144)
    rec0 = oracle_pair(fo, f0, f1, 176, 144, window, 3)[0]
    on = gpu_state(pkg, 176, 144, window, 3, [rec0], [f1])[0]
    off = gpu_state(pkg, 176, 144, window, 3, [rec0], [f1], speculate=False)[0]
    for n in ("MV", "MVD", "MBTYPE", "ST3N", "SUMA", "V0"):
        assert np.array_equal(on[n], off[n]), (kind, n)
    for p in range(on["ST3N"].size):
        k = int(on["ST3N"][p])
        assert np.array_equal(on["ST3"][p, :k], off["ST3"][p, :k]), (kind, p)
