"""The two forms of the dense step of the stage-2 bucket walk (walk_buckets_q), at the batches where they meet.

A dense 64-record batch that leaves the count at or below min(128, halt_cnt) cannot end the walk and takes a short form
without stop tests; every other batch evaluates them per lane.  The candidate list (FERHIP_BUF_ST2) and count
(FERHIP_BUF_ST2N) of every partition must be those of the CPU model of the walk (me_model.WalkModel), and the batches
the model predicts must include the ones where a wrong choice of form, or a wrong stop test, would show:

  1. a batch that leaves the count at exactly 128 (the last count of the short form): the walk goes on;
  2. a batch that takes the count past 128 with no step closing at or behind the crossing lane: the walk goes on, and
     the next batch takes the full form;
  3. a crossing batch in which a step closes in front of the crossing lane: that close does not end the walk;
  4. a crossing batch in which the walk ends, with records of later slices behind the end: those are not candidates;
  5. a dense batch in which the count passes FER_ST2_CAP (the halt_cnt side of the limit).

At QCIF every column tile is in reach of every partition, so a slice is a whole bucket of the reference's sorted feature
table and the model knows each batch exactly.
"""
import numpy as np
import pytest
from me_model import WalkModel, box_sums

W, H = 176, 144
WINDOW = 32
CAP = 384  # FER_ST2_CAP
KINDS = ["textured", "flat-half", "patch"]


def _content(pkg, kind, t):
    f = pkg.gen_frame(W, H, t, 1234, 2).copy()
    y = f[: W * H].reshape(H, W)
    if kind == "flat-half":
        y[:, : W // 2] = 100
    elif kind == "patch":
        # a flat 30 x 30 square: one bucket of ~530 positions, so a count passes CAP inside a dense group
        y[40:70, 60:90] = 100
    return f


def _batch_cases(slices, jend):
    """Follows the walk through its dense batches as the kernel cuts them (groups of 16 steps, the records of a group's
    slices concatenated and cut 64 to a batch; groups of more than 62 x 64 records go slice by slice and have no dense
    batches).  -> the cases of the module docstring that occur (a set of 1 .. 5), and the step the dense walk ends in
    (None when it ends outside a dense batch)."""
    cases = set()
    tren = 0
    for j0 in range(0, 181, 16):
        grp = [s for s in slices if j0 <= s[0] < j0 + 16]
        if not grp:
            break
        T = sum(s[3] for s in grp)
        if T == 0:
            continue
        if T > 62 * 64:
            if j0 <= jend < j0 + 16:
                return cases, None
            tren += sum(len(s[4]) for s in grp)
            continue
        n_hi = {s[0]: s[3] for s in grp if s[1] == 1}
        # per place of the concatenation: passes the filter, step, last record of a slice that closes its step
        ok = np.zeros(T, bool)
        step = np.zeros(T, np.int64)
        close = np.zeros(T, bool)
        place = 0
        for (j, side, lo, n, idx) in grp:
            if n == 0:
                continue
            ok[place + np.asarray(idx, np.int64)] = True
            step[place:place + n] = j
            close[place + n - 1] = side == 1 or n_hi.get(j, 0) == 0
            place += n
        for b0 in range(0, T, 64):
            o, st, cl = ok[b0:b0 + 64], step[b0:b0 + 64], close[b0:b0 + 64]
            nmk = int(o.sum())
            if tren + nmk <= min(128, CAP):  # the short form
                tren += nmk
                if tren == 128:
                    cases.add(1)
                continue
            incl = tren + np.cumsum(o)
            crossing = tren <= 128
            cross_lane = int(np.argmax(incl > 128))
            s1 = np.nonzero(cl & (incl > 128))[0]
            s2 = np.nonzero(incl > CAP)[0]
            if s2.size:
                cases.add(5)
            if crossing and cl[:cross_lane].any():
                cases.add(3)
            if s1.size == 0 and s2.size == 0:
                if crossing:
                    assert b0 + 64 < T  # (the group's last record closes a step)
                    cases.add(2)
                tren += nmk
                continue
            live = np.ones(o.size, bool)
            if s1.size:
                live[s1[0] + 1:] = False
            if s2.size:
                live &= st <= st[s2[0]]
            end = int(np.nonzero(live)[0][-1])
            if crossing and s1.size and end + 1 < o.size:
                cases.add(4)
            return cases, int(st[end])
    return cases, None


_runs = {}


def _run(pkg, fo, kind):
    """One P picture of the content on the GPU and the model's walk of every partition (computed once per content)."""
    if kind in _runs:
        return _runs[kind]
    f0, f1 = _content(pkg, kind, 0), _content(pkg, kind, 1)
    o = fo.Oracle(W, H, qp=12, window=WINDOW)
    o.set_frame(f0)
    o.encode_slice(5)
    rec0 = o.frame()
    o.close()
    r = fo.Oracle(W, H, qp=12, window=WINDOW)
    r.set_dpb(rec0)
    r.fill_interpolated()
    m = WalkModel([r.kar(k, 0) for k in range(5)])
    r.close()
    assert m.a.min() > 0, "a sum-0 position would put the stream on the mis-filed bucket layout"
    g = pkg.FerHip(W, H, 1, qp=12, window=WINDOW)
    g.set_reference(rec0[None])
    g.set_frames(f1[None])
    g.inter_encoding()
    assert g.status() == [0]
    n2 = g.read("ST2N").copy()
    st2 = g.read("ST2").reshape(-1, CAP, 2).copy()
    g.close()
    cur = f1[: W * H].reshape(H, W)
    mbw = W // 16
    walks = []
    for p in range(n2.size):
        mb, part = p // 4, p % 4
        sx, sy = (mb % mbw) * 16 + (part & 1) * 8, (mb // mbw) * 16 + (part >> 1) * 8
        walks.append(m.walk(box_sums(cur, sx, sy), sx, sy))
    _runs[kind] = (n2, st2, walks)
    return _runs[kind]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_lists_match_model(pkg, fo, kind):
    n2, st2, walks = _run(pkg, fo, kind)
    for p, (ref, jend, slices) in enumerate(walks):
        if len(ref) > CAP:
            assert n2[p] > CAP, (kind, p, n2[p], len(ref))
            # the summary of a crowded partition starts with the step the walk stopped in
            assert st2[p, 40, 0] == jend, (kind, p)
            continue
        assert n2[p] == len(ref), (kind, p, n2[p], len(ref))
        got = [(int(x), int(y)) for x, y in st2[p, : len(ref)]]
        assert got == [(int(np.uint32(rel & 0xffffffff).view(np.int32)), D) for rel, D in ref], (kind, p)


@pytest.mark.gpu
def test_stop_cases_occur(pkg, fo):
    """The contents do produce the batches this file is about (the lists of the same runs are checked above)."""
    seen = {c: 0 for c in range(1, 6)}
    for kind in KINDS:
        _, _, walks = _run(pkg, fo, kind)
        for ref, jend, slices in walks:
            cases, jdense = _batch_cases(slices, jend)
            if len(ref) > CAP:
                cases &= {5}  # (cases 1 - 4 are about partitions whose whole list is compared)
            elif jdense is not None:
                assert jdense == jend, (kind, jdense, jend)  # the batches above end where the model's walk ends
            for c in cases:
                seen[c] += 1
        print(kind, dict(seen))
    assert seen[1] > 0, "no batch leaves the count at exactly 128"
    assert seen[2] > 0, "no batch takes the count past 128 without a step closing behind the crossing lane"
    assert seen[3] > 0, "no crossing batch with a step closing in front of the crossing lane"
    assert seen[4] > 0, "no crossing batch that ends the walk in front of records of later slices"
    assert seen[5] > 0, "no dense batch in which the count passes FER_ST2_CAP"
