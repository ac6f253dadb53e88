"""A numpy model of how interEncoding (F/moestimation.cpp:392-585) builds its three candidate lists, for ANY search
centre.

The oracle (oracle/fo_inter.c) builds the stage-1 and stage-2 lists around the TRUE predictor; k_me_spec builds them
around a GUESSED integer centre, so the two can be compared directly only where the guess is right.  This model
restates MEstimation (F/moestimation.cpp:254-296) as what its insertion sort computes -- the first K candidates by
(metric, arrival index) -- from the oracle's own tables: Oracle.kar(k, f) (the five box features of the 16 quarter-sample
planes), Oracle.interp(f) (the planes, for the SADs with the clamping of sad8x8) and the bucket walk of WalkModel.  It is
checked against the oracle's recorded lists on the host (test_me_model_host.py) and then used as the reference of the
GPU lists at the centres the GPU guessed (test_gpu_me_lists.py).

Why "first K by (metric, arrival)" is exact: MEstimation keeps 65 entries, a candidate enters at slot 64 when its metric
is <= that slot's and moves up while it is STRICTLY smaller than the entry above.  Equal metrics therefore stay in
arrival order, and the only place where a later arrival displaces an equal earlier one is slot 64 itself, far below the
17 / 33 entries that are ever read.
"""
import numpy as np

# FER_ST2_CAP, FER_BIGS, FER_OUTL, FER_P2_CAP, FER_BIG_SLICE of fer_dev.h: what the crowded summary depends on
ST2_CAP, BIGS, OUTL, P2_CAP, BIG_SLICE = 384, 3, 512, 320, 1024


def box_sums(cur, sx, sy):
    """suma[5] of the 8x8 source block at (sx, sy), F/moestimation.cpp:440-451"""
    b = cur[sy:sy + 8, sx:sx + 8].astype(np.int64)
    return [int(b.sum()), int(b[:4].sum()), int(b[:, :4].sum()), int(b[[0, 1, 4, 5]].sum()), int(b[:, [0, 1, 4, 5]].sum())]


class WalkModel:
    """The walk of F/moestimation.cpp:470-496 over the sorted feature table of the reference (plane 0).
    kar = the five feature planes of plane 0, each [H][W]."""

    def __init__(self, kar):
        W = np.asarray(kar[0]).shape[1]
        self.k = [np.asarray(k, np.int64).reshape(-1) for k in kar]
        a = self.k[0]
        pos = np.arange(a.size)
        tx, ty = pos % W, pos // W
        order = np.lexsort((ty, tx, a))  # bucket, then tx, then ty
        self.a, self.tx, self.ty = a[order], tx[order], ty[order]
        self.q = [k[order] for k in self.k[1:]]
        self.start = np.searchsorted(self.a, np.arange(16385))
        self._walks = {}  # walk_arrays per partition, kept for the life of the model: small at QCIF, not meant for large pictures

    def walk_arrays(self, su, sx, sy):
        """-> (tmpx, tmpy, D) of the candidates in arrival order up to the stop, the stop step, and the records of
        every slice read (step, side, first index, count, indices passing the filter) up to the stop step.  Computed
        once per argument set; callers leave the result unchanged."""
        key = (tuple(su), sx, sy)
        if key not in self._walks:
            self._walks[key] = self._walk_arrays(su, sx, sy)
        return self._walks[key]

    def _walk_arrays(self, su, sx, sy):
        s0 = su[0]
        px, py, pd, slices = [], [], [], []
        count, jend = 0, 180
        for j in range(181):
            for side in (0, 1):
                a = s0 + j if side else s0 - j
                if a < 0 or a > 16383:
                    slices.append((j, side, 0, 0, np.zeros(0, np.int64)))
                    continue
                lo, hi = self.start[a], self.start[a + 1]
                tx, ty = self.tx[lo:hi], self.ty[lo:hi]
                q = [x[lo:hi] for x in self.q]
                ok = (np.abs(tx - sx) + np.abs(ty - sy) < 280) & (np.abs(q[0] - su[1]) < 100) & (np.abs(q[1] - su[2]) < 100)
                D = j + sum(np.abs(su[i + 1] - q[i]) for i in range(4)) + sum(np.abs((s0 - su[i + 1]) - (a - q[i])) for i in range(4))
                idx = np.nonzero(ok)[0]
                px.append(tx[idx] - sx)
                py.append(ty[idx] - sy)
                pd.append(D[idx])
                slices.append((j, side, lo, hi - lo, idx))
                count += idx.size
            if count > 128:
                jend = j
                break
        cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
        return cat(px), cat(py), cat(pd), jend, slices

    def walk(self, su, sx, sy):
        """-> list of (rel, D) in arrival order up to the stop, the stop step, and the records of every slice read
        (step, side, first index, count, indices passing the filter) up to the stop step's group end."""
        px, py, pd, jend, slices = self.walk_arrays(su, sx, sy)
        slices = list(slices)
        out = [((int(x) << 16) | (int(y) & 0xffff), int(d)) for x, y, d in zip(px, py, pd)]
        s0 = su[0]
        for j in range(jend + 1, min(jend - jend % 16 + 16, 181)):  # the rest of the group: in its batches, not read
            for side in (0, 1):
                a = s0 + j if side else s0 - j
                n = int(self.start[a + 1] - self.start[a]) if 0 <= a <= 16383 else 0
                slices.append((j, side, 0, n, np.zeros(0, np.int64)))
        return out, jend, slices


def first_k(metric, k):
    """indices of the first k candidates by (metric, arrival index)"""
    return np.argsort(np.asarray(metric), kind="stable")[:k]


class MeModel:
    """Lists of one (reference picture, current picture, WindowSize).  kar[k][f] = Oracle.kar(k, f), interp[f] =
    Oracle.interp(f) after fill_interpolated() on the reference; cur = the source luma [H][W]."""

    def __init__(self, kar, interp, cur, window):
        self.H, self.W = np.asarray(cur).shape
        self.cur = np.asarray(cur)
        self.window = window
        self.kar = np.stack([np.stack([np.asarray(kar[k][f], np.int64) for f in range(16)]) for k in range(5)])  # [5][16][H][W]
        # sad8x8 clamps the block origin into the picture and then every sample to the last row / column: an edge
        # padding of 7 gives the same samples without a clamp per sample
        self.ip = np.stack([np.pad(np.asarray(interp[f], np.int64), ((0, 7), (0, 7)), mode="edge") for f in range(16)])
        self.walkm = WalkModel([self.kar[k][0] for k in range(5)])

    @classmethod
    def from_oracle(cls, o, cur, window):
        """o: an Oracle whose dpb is the reference picture and whose fill_interpolated() has run"""
        return cls([[o.kar(k, f) for f in range(16)] for k in range(5)], [o.interp(f) for f in range(16)], cur, window)

    def origin(self, p):
        mbw = self.W // 16
        mb, part = p // 4, p % 4
        return (mb % mbw) * 16 + (part & 1) * 8, (mb // mbw) * 16 + (part >> 1) * 8

    def sums(self, p):
        sx, sy = self.origin(p)
        return box_sums(self.cur, sx, sy)

    def _dist(self, su, f, ry, rx):
        k = self.kar[:, f, ry, rx]
        s0 = su[0]
        d = np.abs(s0 - k[0])
        for i in range(1, 5):
            d = d + np.abs(su[i] - k[i]) + np.abs(s0 - su[i] - k[0] + k[i])
        return d

    def _square(self, p, su, r, cx, cy, fracs):
        """MEstimation over the square of half width r around (cx, cy), weights measured from the same point, `fracs`
        planes per position: (metric, vx, vy) of the valid candidates in arrival order (tmpx, then tmpy, then frac)"""
        sx, sy = self.origin(p)
        n = 2 * r + 1
        tx, ty, fr = np.meshgrid(np.arange(cx - r, cx + r + 1), np.arange(cy - r, cy + r + 1), np.arange(fracs), indexing="ij")
        tx, ty, fr = tx.reshape(-1), ty.reshape(-1), fr.reshape(-1)
        assert tx.size == n * n * fracs
        rx, ry = sx + tx, sy + ty
        ok = (ry >= 0) & (ry < self.H) & (rx >= 0) & (rx < self.W)
        tx, ty, fr, rx, ry = tx[ok], ty[ok], fr[ok], rx[ok], ry[ok]
        m = (np.abs(tx - cx) + np.abs(ty - cy) + 4) * self._dist(su, fr, ry, rx)
        return m, tx * 4 + (fr & 3), ty * 4 + (fr >> 2)

    def sad(self, p, vx, vy):
        """sad8x8 (F/moestimation.cpp:175-195) of vectors in quarter samples"""
        sx, sy = self.origin(p)
        src = self.cur[sy:sy + 8, sx:sx + 8].astype(np.int64)
        out = []
        for x, y in zip(np.asarray(vx).tolist(), np.asarray(vy).tolist()):
            xi = min(max(sx + (x >> 2), 0), self.W - 1)
            yi = min(max(sy + (y >> 2), 0), self.H - 1)
            out.append(int(np.abs(src - self.ip[(x & 3) + (y & 3) * 4, yi:yi + 8, xi:xi + 8]).sum()))
        return np.asarray(out, np.int64)

    def _list(self, p, m, vx, vy, k):
        i = first_k(m, k)
        return dict(vx=vx[i], vy=vy[i], metric=m[i], sad=self.sad(p, vx[i], vy[i]), n=int(i.size))

    def stage1(self, p, genx, geny):
        """the 17 candidates of MEstimation(+-window/16, 16 planes) around (genx, geny)"""
        m, vx, vy = self._square(p, self.sums(p), self.window // 16, genx, geny, 16)
        return self._list(p, m, vx, vy, 17)

    def stage2_candidates(self, p):
        """the bucket walk's candidates (tmpx, tmpy, D) in arrival order; they do not depend on the centre"""
        sx, sy = self.origin(p)
        px, py, pd, _, _ = self.walkm.walk_arrays(self.sums(p), sx, sy)
        return px, py, pd

    def stage2(self, p, genx, geny, cand=None):
        """the 33 walk candidates re-ranked by (|tmpx - genx| + |tmpy - geny| + 4) * D"""
        px, py, pd = cand if cand is not None else self.stage2_candidates(p)
        m = (np.abs(px - genx) + np.abs(py - geny) + 4) * pd
        return self._list(p, m, px * 4, py * 4, 33)

    def stage3(self, p, routes=False):
        """the 33 candidates of MEstimation(+-window/2, plane 0) followed by MEstimation(+-window/16, 16 planes), both
        around 0.  With routes=True also the route predicates of k_me_pre (see route_predicates)."""
        su = self.sums(p)
        mw, wx, wy = self._square(p, su, self.window // 2, 0, 0, 1)
        ml, lx, ly = self._square(p, su, self.window // 16, 0, 0, 16)
        m = np.concatenate([mw, ml])
        out = self._list(p, m, np.concatenate([wx, lx]), np.concatenate([wy, ly]), 33)
        if routes:
            out["routes"] = self.route_predicates(su, p, mw, wx, wy, ml, m)
        return out

    def route_predicates(self, su, p, mw, wx, wy, ml, m):
        """Sufficient conditions, independent of which lane holds which candidate, for the data-dependent routes of
        k_me_pre<16|32>.  T, the kernel's pruning threshold, is the 33rd smallest per-lane minimum of the local metrics
        when at least 33 lanes hold one, so min(local) <= T <= max(local) whenever T is finite.
          pruned:    valid wide candidates with 5 w |s0 - k0| <= max local metric number <= 128 (the pruned wide search
                     keeps them all, provided T is finite)
          full128:   valid wide candidates with 5 w |s0 - k0| <= min local metric number > 128 (more than 128 survive any T)
          refuse64:  more than 64 candidates have a metric <= the 33rd smallest (the unordered selection gives up, or
                     the ordered one takes its general route)
          tie_end:   the 33rd and the 34th smallest metrics are equal (the list's end is decided by arrival)"""
        sx, sy = self.origin(p)
        k0 = self.kar[0, 0, sy + wy // 4, sx + wx // 4]
        lb = 5 * (np.abs(wx // 4) + np.abs(wy // 4) + 4) * np.abs(su[0] - k0)
        srt = np.sort(m)
        return dict(pruned=bool(ml.size and (lb <= ml.max()).sum() <= 128),
                    full128=bool(ml.size and (lb <= ml.min()).sum() > 128),
                    refuse64=bool(srt.size >= 33 and (m <= srt[32]).sum() > 64),
                    tie_end=bool(srt.size >= 34 and srt[32] == srt[33]))

    def stage2_routes(self, p, genx, geny, cand=None):
        """Sufficient conditions, independent of which lane holds which candidate, for the routes of select_topk_ex
        under stage2_list at the centre (genx, geny).  The selection runs only on a partition that is not crowded, so
        every predicate also requires 1 <= n <= ST2_CAP candidates.
          general_t0:  every candidate's metric is >= 2^21: every lane minimum is, so T0 = 1 << 21 (or, with fewer
                       than `need` lanes in use, 2^31 - 1) and the general route is entered through T0, not through ties
          straddle:    at least 33 candidates below 2^21, at least one at or above it, and on each side one within one
                       weight step (its own D) of 2^21: the fast route's guard and its `hi` bound from below
          mixed_t0:    at most 64 candidates (each alone in its lane, so T0 is known), some of them below 2^21, and
                       the need-th smallest at or above it: T0 = 1 << 21 with metrics on both sides of it
        also max_metric, n, below = how many metrics are < 2^21, and nth = the need-th smallest metric (need = min(33,
        n)), which IS T0 when n <= 64, every candidate then being alone in its lane."""
        px, py, pd = cand if cand is not None else self.stage2_candidates(p)
        m = (np.abs(px - genx) + np.abs(py - geny) + 4) * pd
        n, lim = int(m.size), 1 << 21
        out = dict(general_t0=False, straddle=False, mixed_t0=False, max_metric=int(m.max()) if n else 0, n=n, below=int((m < lim).sum()), nth=0)
        if 1 <= n <= ST2_CAP:
            lo, hi = m < lim, m >= lim
            out["nth"] = int(np.sort(m)[min(33, n) - 1])
            out["general_t0"] = bool(hi.all())
            out["straddle"] = bool(lo.sum() >= 33 and hi.any() and (lo & (m + pd >= lim)).any() and (hi & (m - pd < lim)).any())
            out["mixed_t0"] = bool(n <= 64 and lo.any() and out["nth"] >= lim)
        return out

    def crowded_summary(self, p):
        """What k_me_walk writes into the summary of a crowded partition (more than ST2_CAP walk candidates), restated
        from the model's buckets; None for a partition that is not crowded.  Only for pictures at most 280 samples wide:
        the column-tile range bt_lo..bt_hi of k_me_walk is then the whole picture for every partition, and a "slice" is a
        whole bucket of the sorted feature table.

        With J the stop step, the buckets su[0] + dj, dj = -J..J, of more than BIG_SLICE positions are `raw_big`; the
        device leaves bucket su[0] out of them when the ranges of its four other sums all contain the source's (the
        bucket may hold distance 0 and is read whole), which gives `bigs`, in the device's order.  The three causes of
        the fallback bit:
          a  more than BIGS big buckets
          b  (not a) a described big bucket with more than OUTL positions outside its class
          c  (neither) more than P2_CAP listed candidates: everything with D > 0 in the other buckets of the steps
             0..J (bucket su[0] once), and the outliers of the described big buckets that pass the walk's tests with a
             distance other than 0 and the class's
        The device takes the features of the bucket's MIDDLE record (sorted order) as its class; the modal class is the
        most frequent (k1..k4).  Where the two differ the device's rule is not the modal one and the partition is
        `undecided`; so is one with 33 or more candidates of distance 0, whose listing stops inside a batch.  An
        undecided partition claims no cause and no value of slot 41.

        This mirrors the KERNEL's rule (skip0, the order of the big buckets, outliers listed only for the buckets in front
        of the one that sets b), not anything the reference computes: slot 41 is a device-side summary with no counterpart
        there.  It tells which route a partition takes and pins the summary's layout; the independent check of what the
        routes compute is the final vector, MVD and MBTYPE against the oracle."""
        assert self.W <= 280, "a slice is a whole bucket only while the 280-diamond spans every column tile"
        w, su = self.walkm, self.sums(p)
        sx, sy = self.origin(p)
        px, _, _, J, _ = w.walk_arrays(su, sx, sy)
        if px.size <= ST2_CAP:
            return None
        s0 = su[0]

        def bucket(dj):
            a = s0 + dj
            if a < 0 or a > 16383:
                return None
            lo, hi = int(w.start[a]), int(w.start[a + 1])
            q = np.stack([x[lo:hi] for x in w.q], -1)  # [n][4]
            ok = (np.abs(w.tx[lo:hi] - sx) + np.abs(w.ty[lo:hi] - sy) < 280) & (np.abs(q[:, 0] - su[1]) < 100) & (np.abs(q[:, 1] - su[2]) < 100)
            D = abs(dj) + sum(np.abs(su[i + 1] - q[:, i]) + np.abs((s0 - su[i + 1]) - (a - q[:, i])) for i in range(4))
            return q, ok, D

        raw_big, bigs, skip0 = 0, [], False
        for dj in range(-J, J + 1):
            b = bucket(dj)
            if b is None or len(b[0]) <= BIG_SLICE:
                continue
            raw_big += 1
            if dj == 0 and all(b[0][:, i].min() <= su[i + 1] <= b[0][:, i].max() for i in range(4)):
                continue
            skip0 |= dj == 0
            bigs.append(dj)
        out = dict(J=J, raw_big=raw_big, bigs=bigs, nbig=min(len(bigs), BIGS), a=len(bigs) > BIGS, b=False, c=False, np2=None,
                   classes=[], undecided=None)
        listed = 0
        for dj in bigs[:BIGS]:
            q, ok, D = bucket(dj)
            cls, cnt = np.unique(q, axis=0, return_counts=True)
            mid = q[len(q) // 2]
            nmid = int((q == mid).all(1).sum())
            out["classes"].append((dj, tuple(int(v) for v in cls[np.argmax(cnt)]), len(q) - int(cnt.max())))
            if out["a"] or out["b"]:  # the device reads no class any more
                continue
            if nmid != cnt.max():
                out["undecided"] = "the middle record of bucket %d is not of its modal class" % (s0 + dj)
                return out
            if len(q) - nmid > OUTL:
                out["b"] = True
                continue
            member = (q == mid).all(1)
            DM = int(D[member][0])
            listed += int((~member & ok & (D > 0) & (D != DM)).sum())
        zero = 0
        for j in range(J + 1):
            for dj in ((0,) if j == 0 else (-j, j)):
                b = bucket(dj)
                if b is None or (len(b[0]) > BIG_SLICE and (j > 0 or skip0)):
                    continue
                listed += int((b[1] & (b[2] > 0)).sum())
                if j == 0:
                    zero = int((b[1] & (b[2] == 0)).sum())
        out["zero"] = zero
        if zero >= 33 and not (out["a"] or out["b"]):
            out["undecided"] = "33 or more candidates of distance 0: the listing stops inside a batch"
            return out
        if zero < 33:
            out["np2"] = listed
            out["c"] = not (out["a"] or out["b"]) and listed > P2_CAP
        out["fallback"] = out["a"] or out["b"] or out["c"]
        return out


# ---------------------------------------------------------------- the predictor of an 8x8 partition
def _core(A, B, C):
    """the median rule of PredictMV_Luma (F/mode_pred.cpp:322-371) for reference index 0 everywhere; None = not
    available"""
    ra = rb = rc = 0
    if A is None and B is None:
        A, ra = (0, 0), 0
    if A is None and B is not None:
        A, ra = (0, 0), -1
    if B is None:
        B, rb = A, ra
    if C is None:
        C, rc = A, ra
    if ra == 0 and rb != 0 and rc != 0:
        return A
    if ra != 0 and rb == 0 and rc != 0:
        return B
    if ra != 0 and rb != 0 and rc == 0:
        return C
    med = lambda a, b, c: max(min(a, b), min(c, max(a, b)))
    return med(A[0], B[0], C[0]), med(A[1], B[1], C[1])


def predict_8x8(field, mbw, p):
    """The predicted vector of 8x8 partition p from a field of one vector per partition, field[nmb * 4][2] laid out
    [macroblock][quadrant]: neighbours A (left), B (above), C (above right; not yet coded for quadrant 3, the next
    macroblock's for quadrant 1) with D (above left) in place of an unavailable C -- the rules of fer_mvpred.h /
    F/mode_pred.cpp for a P_8x8 macroblock whose neighbours are all inter."""
    mb, part = p // 4, p % 4
    gx, gy = (mb % mbw) * 2 + (part & 1), (mb // mbw) * 2 + (part >> 1)
    gw = mbw * 2

    def at(xa, ya):
        return tuple(int(v) for v in field[(((ya >> 1) * mbw + (xa >> 1)) << 2) + ((ya & 1) << 1) + (xa & 1)])

    A = at(gx - 1, gy) if gx > 0 else None
    B = at(gx, gy - 1) if gy > 0 else None
    vC = False if part == 3 else (True if part == 2 else ((gy > 0 and gx + 1 < gw) if part == 1 else gy > 0))
    if vC:
        C = at(gx + 1, gy - 1)
    else:
        C = at(gx - 1, gy - 1) if (gy > 0 and gx > 0) else None
    return _core(A, B, C)


def unpack_xy(w):
    """packed vector (x & 0xffff | y << 16) -> (x, y), arrays or scalars"""
    w = np.asarray(w).astype(np.int64)
    x = ((w & 0xffff) ^ 0x8000) - 0x8000
    y = (((w >> 16) & 0xffff) ^ 0x8000) - 0x8000
    return x, y


# ---------------------------------------------------------------- the cases both list test modules run
KINDS = ["textured", "letterbox", "flat-half", "soft", "patch"]  # the content kinds of test_gpu_walk_dense._content
# "soft" is all P_Skip at MAXDIFF 3 (pinned in test_me_model_host.py): it runs with MAXDIFF 0 so that its macroblocks search
MAXDIFF = {"soft": 0}


def oracle_pair(fo, f0, f1, W, H, window, maxdiff, qp=12):
    """I picture f0, then P picture f1 with recording -> (reconstruction of picture 0, lists, mb_type, mv, P_Skip count)"""
    o = fo.Oracle(W, H, qp=qp, window=window, maxdiff=maxdiff)
    o.set_frame(f0)
    o.encode_slice(5)
    rec0 = o.frame()
    o.record_me()
    o.set_frame(f1)
    o.encode_slice(1)
    rec = o.me_lists()
    out = rec0, rec, o.mb_type(), o.mv(), int(o.stats()[0])
    o.close()
    return out


def oracle_pair_ref(fo, ref, f1, W, H, window, maxdiff, qp=12):
    """oracle_pair with the reference picture given as it is (no I picture is coded): P picture f1 searched in `ref` with
    recording -> (ref, lists, mb_type, mv, P_Skip count)"""
    o = fo.Oracle(W, H, qp=qp, window=window, maxdiff=maxdiff)
    o.set_dpb(ref)
    o.fill_interpolated()
    o.record_me()
    o.set_frame(f1)
    o.encode_slice(1)
    out = ref, o.me_lists(), o.mb_type(), o.mv(), int(o.stats()[0])
    o.close()
    return out


def model_for(fo, rec0, f1, W, H, window):
    """the list model of (reference picture rec0, source picture f1)"""
    r = fo.Oracle(W, H, qp=12, window=window)
    r.set_dpb(rec0)
    r.fill_interpolated()
    m = MeModel.from_oracle(r, f1[: W * H].reshape(H, W), window)
    r.close()
    return m
