"""A lane model of the routes select_topk_ex (fer_me.hip) takes at each of its call sites at WindowSize 16 / 32, on top of
the list model of me_model.py (which says WHAT the lists are; the route never changes that).

The selection looks for a bound T0 of the need-th smallest candidate among the 64 per-lane minima, gathers every
candidate <= T0 and ranks what it gathered.  Its first bound is coarse (fer_sel_thr.h: the largest value with the same
4 significant bits as the need-th smallest lane minimum); more than 64 candidates under it send it to the exact need-th
smallest lane minimum and a second gather; more than 64 under that leave the wide route (the ordered general route, or,
in k_me_pre's pruned search, the full evaluation).  Which lane holds which candidate decides all of it, so the model
lays the candidates out as the kernels do:

  stage 1          candidate c = (ix * n1 + iy) * 16 + frac of the (2 r + 1)^2 x 16 grid around the centre, -1 outside
                   the picture, in batch c // 64, lane c % 64 (local_metrics)
  stage 2          walk candidate number c in batch c // 64, lane c % 64; three batches when the list holds at most
                   192, six otherwise, more than 384 = crowded: no selection
  stage 3 pruned   T = the 33rd smallest per-lane minimum of the local grid (centre 0); the wide candidates with
                   5 w |s0 - k0| <= T in the order the kernel meets them -- row by row (iy, then ix) over the first
                   WindowSize columns, then column WindowSize by iy -- survivor number i in batch i // 64, lane i % 64,
                   the local grid behind them.  More than 128 survivors: no pruned selection
  stage 3 full     the whole wide grid c = ix * n + iy, -1 outside the picture, then the local grid from batch
                   ceil(n * n / 64) on: runs when the pruned route did not deliver, and starts with the exact bound
                   (the coarse one nearly always overflows where the pruned selection has refused)

ROUTES: "coarse_fits", "exact_fits" (coarse overflowed), "both_over", and "general" (fewer than `need` lanes below 2^21:
no wide route at all, not a matter of the bound).
"""
import numpy as np

LIMIT = 1 << 21
ROUTES = ("coarse_fits", "exact_fits", "both_over", "general")


def code_of(t):
    """fer_sel_thr.h sel_code_of, restated: t < 8 is its own code, else (floor(log2 t) - 2) << 3 | the 3 bits below the top one"""
    t = int(t)
    if t < 8:
        return t
    e = t.bit_length() - 1
    return ((e - 2) << 3) | ((t >> (e - 3)) & 7)


def thr(code):
    """fer_sel_thr.h sel_thr, restated: the largest value of the code, capped at 2^21 - 1"""
    E, mant = code >> 3, code & 7
    if E == 0:
        return mant
    return min(((9 + mant) << (E - 1)) - 1, LIMIT - 1)


def route(v, K, coarse_first=True):
    """v: metrics in register layout [batches][64], -1 = no candidate -> (route or None when there is no candidate,
    dict of the figures behind it).  coarse_first=False: a site that starts with the exact bound (only "exact_fits" /
    "both_over" / "general" there)"""
    v = np.asarray(v, np.int64).reshape(-1, 64)
    valid = v >= 0
    total = int(valid.sum())
    need = min(K, total)
    if need == 0:
        return None, dict(need=0)
    assert v.max() < (1 << 26), "beyond the selection's guard: not modelled"
    lmin = np.where(valid, v, 1 << 40).min(0)
    below = np.sort(lmin[lmin < LIMIT])
    if below.size < need:
        return "general", dict(need=need, total=total)
    exact = int(below[need - 1])
    coarse = thr(code_of(exact))
    assert exact <= coarse < LIMIT
    c1 = int((valid & (v <= coarse)).sum())
    c2 = int((valid & (v <= exact)).sum())
    r = "coarse_fits" if c1 <= 64 and coarse_first else ("exact_fits" if c2 <= 64 else "both_over")
    return r, dict(need=need, total=total, exact=exact, coarse=coarse, under_coarse=c1, under_exact=c2)


def _batches(x):
    x = np.asarray(x, np.int64)
    pad = (-x.size) % 64
    return np.concatenate([x, np.full(pad, -1, np.int64)]).reshape(-1, 64)


def local_grid(m, p, cx, cy):
    """metrics of the stage-1 shaped grid around (cx, cy) in the kernel's candidate order, -1 outside the picture"""
    r = m.window // 16
    n1 = 2 * r + 1
    sx, sy = m.origin(p)
    su = m.sums(p)
    ix, iy, fr = np.meshgrid(np.arange(n1), np.arange(n1), np.arange(16), indexing="ij")
    ix, iy, fr = ix.reshape(-1), iy.reshape(-1), fr.reshape(-1)
    rx, ry = sx + cx - r + ix, sy + cy - r + iy
    ok = (rx >= 0) & (rx < m.W) & (ry >= 0) & (ry < m.H)
    d = m._dist(su, fr, np.clip(ry, 0, m.H - 1), np.clip(rx, 0, m.W - 1))
    return np.where(ok, (np.abs(ix - r) + np.abs(iy - r) + 4) * d, -1)


def stage1_route(m, p, genx, geny):
    return route(_batches(local_grid(m, p, genx, geny)), 17)


def stage2_route(m, p, genx, geny):
    """-> (route, figures); route None for an empty list, "crowded" beyond 384 candidates (no selection runs)"""
    px, py, pd = m.stage2_candidates(p)
    n = int(px.size)
    if n > 384:
        return "crowded", dict(n2=n)
    met = (np.abs(px - genx) + np.abs(py - geny) + 4) * pd
    r, f = route(_batches(met), 33)
    f["n2"] = n
    f["last_arrival"] = n - 1
    return r, f


def wide_grid(m, p):
    """(metric, lower bound 5 w |s0 - k0|, valid) of the wide grid of stage 3, indexed [ix][iy]"""
    R = m.window // 2
    n = 2 * R + 1
    sx, sy = m.origin(p)
    su = m.sums(p)
    ix, iy = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rx, ry = sx - R + ix, sy - R + iy
    ok = (rx >= 0) & (rx < m.W) & (ry >= 0) & (ry < m.H)
    cx, cy = np.clip(rx, 0, m.W - 1), np.clip(ry, 0, m.H - 1)
    w = np.abs(ix - R) + np.abs(iy - R) + 4
    met = w * m._dist(su, 0, cy, cx)
    lb = 5 * w * np.abs(su[0] - m.kar[0, 0, cy, cx])
    return met, lb, ok


def stage3_routes(m, p):
    """-> dict(pruned=(route or None when the pruned selection does not run, figures), full=(route, figures) or None
    when the full evaluation does not run)"""
    assert m.window in (16, 32)
    loc = _batches(local_grid(m, p, 0, 0))
    lminl = np.where(loc >= 0, loc, 1 << 40).min(0)
    below = np.sort(lminl[lminl < LIMIT])
    met, lb, ok = wide_grid(m, p)
    n = met.shape[0]
    out = dict(pruned=(None, dict(T=None)), full=None)
    delivered = False
    if below.size >= 33:
        T = int(below[32])
        keep = ok & (lb <= T)
        body = keep[: n - 1].T  # [iy][ix] over the first WindowSize columns: the kernel's batches are rows of them
        order = [met[: n - 1].T[body], met[n - 1][keep[n - 1]]]
        surv = np.concatenate(order)
        fig = dict(T=T, survivors=int(surv.size))
        if surv.size <= 128:
            sb = np.full(128, -1, np.int64)
            sb[: surv.size] = surv
            r, f = route(np.concatenate([sb.reshape(2, 64), loc]), 33)
            f.update(fig)
            out["pruned"] = (r, f)
            delivered = r in ("coarse_fits", "exact_fits")
        else:
            out["pruned"] = (None, fig)
    if not delivered:
        wide = np.where(ok, met, -1).reshape(-1)  # c = ix * n + iy
        out["full"] = route(np.concatenate([_batches(wide), loc]), 33, coarse_first=False)
    return out


# ---------------------------------------------------------------- the inputs both selection test modules run
# The five content kinds of test_gpu_walk_dense._content, and three low-contrast ramps (the "soft" kind with another
# noise seed / amplitude), found by searching seeds on the CPU for what the kinds do not reach: many nearly equal metrics
# around the need-th smallest, so that the coarse bound admits more than 64 candidates and the exact one does not.
W, H = 176, 144
RAMPS = {"ramp21a2": (21, 2), "ramp21a3": (21, 3), "ramp31a2": (31, 2)}
INPUTS = ["textured", "letterbox", "flat-half", "soft", "patch"] + sorted(RAMPS)
_cache = {}


def frames(gen, name):
    """pictures 0 and 1 of an input; gen = anything with gen_frame (the package or the oracle module)"""
    from test_gpu_walk_dense import _content
    if name not in RAMPS:
        return _content(gen, name, 0), _content(gen, name, 1)
    seed, amp = RAMPS[name]
    out = []
    for t in (0, 1):
        f = gen.gen_frame(W, H, t, 1234, 2).copy()
        rng = np.random.default_rng(seed + t)
        yy, xx = np.mgrid[0:H, 0:W]
        f[: W * H].reshape(H, W)[:] = np.clip(90 + xx // 11 + yy // 9 + rng.integers(0, amp, size=(H, W)), 0, 255).astype(np.uint8)
        out.append(f)
    return tuple(out)


def maxdiff_of(name):
    return 0 if name == "soft" or name in RAMPS else 3  # the low-contrast inputs are all P_Skip at MAXDIFF 3


def analysis(fo, name, window):
    """oracle recording, list model and the routes of every selection the device must run: stage 3 of every partition,
    stages 1 and 2 of every partition the oracle searched, at the oracle's centre (k_me_spec runs them there when its
    guess is right, the chain when it is not or when speculation is off).  Computed once per (name, window); callers
    leave it unchanged."""
    from me_model import model_for, oracle_pair
    key = (name, window)
    if key not in _cache:
        f0, f1 = frames(fo, name)
        orc = oracle_pair(fo, f0, f1, W, H, window, maxdiff_of(name))
        rec0, rec = orc[0], orc[1]
        m = model_for(fo, rec0, f1, W, H, window)
        np4 = (W // 16) * (H // 16) * 4
        r = dict(st3=[], st3_full=[], st1=[], st2=[], n2=[], late=0)
        for p in range(np4):
            s3 = stage3_routes(m, p)
            r["st3"].append(s3["pruned"][0])
            if s3["full"] is not None:
                r["st3_full"].append(s3["full"][0])
            if rec["searched"][p]:
                gx, gy = int(rec["mvp"][p, 0]) >> 2, int(rec["mvp"][p, 1]) >> 2
                r["st1"].append(stage1_route(m, p, gx, gy)[0])
                r2, f2 = stage2_route(m, p, gx, gy)
                r["st2"].append(r2)
                r["n2"].append(f2["n2"])
                if r2 not in (None, "crowded") and f2["n2"] > 192:
                    px, py, pd = m.stage2_candidates(p)
                    win = np.argsort((np.abs(px - gx) + np.abs(py - gy) + 4) * pd, kind="stable")[:33]
                    r["late"] += int((win >= 192).any())  # a winner from the batches that are read on the count alone
        _cache[key] = dict(orc=orc, model=m, f1=f1, routes=r)
    return _cache[key]
