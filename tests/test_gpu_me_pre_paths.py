"""The data-dependent routes of k_me_pre<16|32> at their boundaries, with the harness of test_gpu_me_lists.py: reference
= the oracle's reconstruction of picture 0, source = picture 1, one inter_encoding(); SUMA, ST3N, every entry of ST3 in
order and V0 against the oracle's recording / the list model, MBTYPE and the final vector of every searched partition
against the oracle (check_stream compares all of them, for every partition).  Every comparison is exact equality.

Which route a partition takes is decided here by a LANE model of the kernel's pruning (lane_route), written from the
layout the kernel documents: local candidate c = (ix * N1 + iy) * 16 + plane sits in lane c % 64; T = the 33rd smallest
per-lane minimum of the local metrics, absent when fewer than 33 lanes hold a candidate; a valid wide candidate
survives when 5 (|tx| + |ty| + 4) |s0 - k0| <= T; more than 128 survivors take the full evaluation.  The outputs cannot
tell 128 survivors from 129 (both routes must give the same list), so each test asserts the model's count before it
compares: a case cannot silently stop reaching its route.

The source blocks of the boundary cases were found by a search over this model on the host (the reference picture does
not depend on the source picture, so a block can be tuned without moving anything else); they are rebuilt here from
the textured QCIF picture by fixed recipes.

T absent.  A legal picture is at least 16 x 16 and a partition's local window reaches 8 samples of the block itself, so at
least 2 x 2 (WindowSize 16) or 3 x 3 (WindowSize 32) local positions lie inside every picture; consecutive positions
fall into different 16-lane groups, which leaves at least 48 lanes with a candidate: the kernel's "fewer than 33" branch
cannot be reached by any picture.  test_no_threshold_is_unreachable pins that with the lane model over the tiny and
flat pictures named for it (and runs them); the full evaluation itself is reached by the 129-survivor case and by the
letterbox picture (44 partitions with up to 528 survivors).
"""
import numpy as np
import pytest
from me_model import model_for, oracle_pair
from test_gpu_me_lists import check_stream, frames_of, gpu_state, run_case
from test_gpu_walk_dense import _content

pytestmark = pytest.mark.gpu

QW, QH = 176, 144


def lane_route(m, p):
    """(T or None, survivors of the pruned wide search, survivors whose bound equals T) of partition p"""
    su = [int(v) for v in m.sums(p)]
    sx, sy = m.origin(p)
    R, r2 = m.window // 2, m.window // 16
    n2 = 2 * r2 + 1
    ix, iy, fr = (a.reshape(-1) for a in np.meshgrid(np.arange(n2), np.arange(n2), np.arange(16), indexing="ij"))
    c = (ix * n2 + iy) * 16 + fr
    rx, ry = sx - r2 + ix, sy - r2 + iy
    ok = (rx >= 0) & (rx < m.W) & (ry >= 0) & (ry < m.H)
    met = (np.abs(ix - r2) + np.abs(iy - r2) + 4) * m._dist(su, fr, np.clip(ry, 0, m.H - 1), np.clip(rx, 0, m.W - 1))
    lmin = np.full(64, 1 << 40, np.int64)
    np.minimum.at(lmin, (c % 64)[ok], met[ok])
    have = np.sort(lmin[lmin < (1 << 21)])
    if have.size < 33:
        return None, 0, 0
    T = int(have[32])
    n = 2 * R + 1
    wx, wy = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    rx, ry = sx - R + wx, sy - R + wy
    okw = (rx >= 0) & (rx < m.W) & (ry >= 0) & (ry < m.H)
    k0 = m.kar[0, 0, np.clip(ry, 0, m.H - 1), np.clip(rx, 0, m.W - 1)]
    lb = 5 * (np.abs(wx - R) + np.abs(wy - R) + 4) * np.abs(su[0] - k0)
    return T, int((okw & (lb <= T)).sum()), int((okw & (lb == T)).sum())


# ---- the boundary picture: textured QCIF with three source blocks replaced (partition -> recipe)
P_EQ, P_128, P_129 = 13, 228, 31


def _origin(p):
    mb, part = p // 4, p % 4
    return (mb % (QW // 16)) * 16 + (part & 1) * 8, (mb // (QW // 16)) * 16 + (part >> 1) * 8


def boundary_pair(pkg):
    f0, f1 = _content(pkg, "textured", 0), _content(pkg, "textured", 1).copy()
    y = f1[: QW * QH].reshape(QH, QW)

    def block(p):
        sx, sy = _origin(p)
        return y[sy:sy + 8, sx:sx + 8]
    b = block(P_EQ)
    b[:] = np.clip(b[::-1, ::-1].astype(np.int64) + (36 - 128), 0, 255).astype(np.uint8)
    b = block(P_128)
    b[:4], b[4:] = 68, 128
    b = block(P_129)
    b[:] = np.clip(b.astype(np.int64) + 2, 0, 255).astype(np.uint8)
    b[2] = 241
    return f0, f1


def run_pairs(pkg, fo, pairs, window, maxdiff, tag):
    """run_case of test_gpu_me_lists for explicit (picture 0, picture 1) pairs, one stream each -> the models and counters"""
    orc = [oracle_pair(fo, f0, f1, QW, QH, window, maxdiff) for f0, f1 in pairs]
    sts = gpu_state(pkg, QW, QH, window, maxdiff, [o[0] for o in orc], [f1 for _, f1 in pairs])
    models, counts = [], []
    for s, (st, (rec0, rec, mbt, omv, _), (_, f1)) in enumerate(zip(sts, orc, pairs)):
        m = model_for(fo, rec0, f1, QW, QH, window)
        assert np.array_equal(st["MBTYPE"], mbt), (tag, s, "mb_type")
        counts.append(check_stream((tag, window, s), st, rec, omv.reshape(-1, 2), m, QW, QH))
        models.append(m)
    return models, counts


def test_prune_boundary(pkg, fo):
    """a bound equal to T, exactly 128 survivors (the pruned route's last count) and exactly 129 (the first of the fallback)"""
    (m,), (c,) = run_pairs(pkg, fo, [boundary_pair(pkg)], 32, 3, "boundary")
    T, ns, eq = lane_route(m, P_EQ)
    print("me_pre_paths boundary: eq", (T, ns, eq), "128", lane_route(m, P_128), "129", lane_route(m, P_129), c)
    assert T is not None and T > 0 and 0 < ns < 128 and eq >= 1, (T, ns, eq)
    assert lane_route(m, P_128)[1] == 128
    assert lane_route(m, P_129)[1] == 129


@pytest.mark.parametrize("W,H", [(16, 16), (32, 16), (16, 32), (48, 48), (1024, 16)])
def test_window_clipped_on_every_side(pkg, fo, W, H):
    """WindowSize 32 on pictures no wider or higher than the window: the wide window and the local patch of every
    partition leave the picture on two sides or more (row / column masks, the column n - 1); 1024 x 16: a single row of
    macroblocks, every wide row but 16 outside"""
    c, _, _ = run_case(pkg, fo, "textured", W, H, 32, 0)
    assert c["parts"] == (W // 16) * (H // 16) * 4, c


@pytest.mark.parametrize("W,H,kind", [(16, 16, "textured"), (32, 16, "textured"), (16, 16, "flat"), (176, 144, "flat")])
def test_no_threshold_is_unreachable(pkg, fo, W, H, kind):
    """T is present on every partition of the tiny and the flat pictures (see the module text); they are compared like the rest"""
    f0, f1 = (pkg.gen_frame(W, H, t, 1234, 2).copy() for t in (0, 1))
    if kind == "flat":
        f0[: W * H] = 100
        f1[: W * H] = 100
    for window in (16, 32):
        rec0, rec, mbt, omv, _ = oracle_pair(fo, f0, f1, W, H, window, 0)
        st = gpu_state(pkg, W, H, window, 0, [rec0], [f1])[0]
        m = model_for(fo, rec0, f1, W, H, window)
        assert np.array_equal(st["MBTYPE"], mbt), (kind, W, H, window, "mb_type")
        check_stream((kind, W, H, window), st, rec, omv.reshape(-1, 2), m, W, H)
        routes = [lane_route(m, p) for p in range((W // 16) * (H // 16) * 4)]
        assert all(r[0] is not None for r in routes), (kind, W, H, window)


@pytest.mark.parametrize("kind", ["textured", "letterbox"])
@pytest.mark.parametrize("window", [16, 48])
def test_other_windows(pkg, fo, kind, window):
    """k_me_pre<16> and the general k_me_pre<0>"""
    c, _, _ = run_case(pkg, fo, kind, QW, QH, window, 3)
    assert c["hit"] > 0, c


def test_three_routes_in_one_launch(pkg, fo):
    """three streams in one launch: plain textured (pruned route everywhere), the boundary picture (129 survivors: the
    fallback by the smallest overflow) and the letterbox picture (dozens of partitions with hundreds of survivors) --
    per-stream pointers, and both uses of the LDS inside one launch.  (The no-T fallback cannot be reached, see the
    module text.)"""
    pairs = [frames_of(pkg, "textured", QW, QH), boundary_pair(pkg), frames_of(pkg, "letterbox", QW, QH)]
    models, counts = run_pairs(pkg, fo, pairs, 32, 3, "three routes")
    r0 = [lane_route(models[0], p) for p in range(396)]
    assert all(t is not None and ns <= 128 for t, ns, _ in r0), "stream 0 leaves the pruned wide search"
    assert lane_route(models[1], P_129)[1] == 129
    assert sum(ns > 128 for _, ns, _ in (lane_route(models[2], p) for p in range(396))) >= 40
    assert counts[0]["hit"] > 0 and counts[1]["hit"] > 0
