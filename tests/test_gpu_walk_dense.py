"""The stage-2 bucket walk (k_me_walk) against a model of it on the CPU, on pictures where its batches span slices.

The walk cuts the records of the 32 slices of a 16-step group into dense 64-record batches, so a batch may hold the
tail of one slice and the heads of the next ones, and its stop tests fall on lanes.  At QCIF every column tile is in
reach of every partition, so a slice is a whole bucket of the reference's sorted feature table and the model below
knows each batch exactly.  The candidate list (FERHIP_BUF_ST2) and its count (FERHIP_BUF_ST2N) of every partition must
be the model's; the pictures are chosen so that the cases the lane-level stop tests exist for do occur, and the test
asserts that they do.
"""
import numpy as np
import pytest
from me_model import WalkModel as Model

W, H = 176, 144
CAP = 384  # FER_ST2_CAP


def _content(pkg, kind, t):
    f = pkg.gen_frame(W, H, t, 1234, 2).copy()
    y = f[: W * H].reshape(H, W)
    if kind == "letterbox":
        y[:16] = 16
        y[-16:] = 16
    elif kind == "flat-half":
        y[:, : W // 2] = 100
    elif kind == "patch":
        # a flat 30 x 30 square: one bucket of ~530 positions, so a count passes CAP inside a dense group
        y[40:70, 60:90] = 100
    elif kind == "soft":
        # a low-contrast ramp with a little noise: buckets of a few dozen positions, counts that pass 128 and 384
        # inside one step
        rng = np.random.default_rng(7 + t)
        yy, xx = np.mgrid[0:H, 0:W]
        y[:] = np.clip(90 + xx // 11 + yy // 9 + rng.integers(0, 2, size=(H, W)), 0, 255).astype(np.uint8)
    return f


def _sums(cur, sx, sy):
    b = cur[sy:sy + 8, sx:sx + 8].astype(np.int64)
    return [int(b.sum()), int(b[:4].sum()), int(b[:, :4].sum()), int(b[[0, 1, 4, 5]].sum()), int(b[:, [0, 1, 4, 5]].sum())]


def _cases(slices, jend, crowded):
    """Lane-level cases in the dense batches of the stop step's group: (the step closes mid-batch, with records of
    later slices behind it in the batch, after a slice of the group crossed a batch boundary; the count passes CAP
    at a lane that is not the last of its batch)."""
    j0 = jend - jend % 16
    grp = [s for s in slices if j0 <= s[0] < j0 + 16]
    T = sum(s[3] for s in grp)
    if T == 0 or T > 62 * 64:
        return False, False
    before = sum(len(s[4]) for s in slices if s[0] < j0)
    place, crossed, close_place, cap_place, c = 0, False, None, None, before
    for (j, side, lo, n, idx) in grp:
        if cap_place is None and c + len(idx) > CAP:
            cap_place = place + int(idx[CAP - c])
        c += len(idx)
        if n and close_place is None:
            crossed |= place // 64 != (place + n - 1) // 64
        if n and j == jend:
            close_place = place + n - 1
        place += n
    mid = not crowded and crossed and close_place is not None and close_place % 64 != 63 and close_place + 1 < T
    cap = crowded and cap_place is not None and cap_place % 64 != 63 and cap_place + 1 < T
    return mid, cap


@pytest.mark.gpu
@pytest.mark.parametrize("window", [32, 48])
@pytest.mark.parametrize("kind", ["textured", "letterbox", "flat-half", "soft", "patch"])
def test_walk_matches_model(pkg, fo, kind, window):
    seen_mid, seen_cap = walk_check(pkg, fo, kind, _content(pkg, kind, 0), _content(pkg, kind, 1), window)
    if kind in ("soft", "patch"):
        assert seen_mid > 0, "no partition whose step closes inside a batch that spans slices"
    if kind == "patch":
        assert seen_cap > 0, "no partition whose count passes CAP inside a dense batch"


def walk_check(pkg, fo, kind, f0, f1, window):
    """ST2N and ST2 of every partition of QCIF picture f1 searched in the oracle's reconstruction of f0 against the model ->
    how many partitions showed each of the two lane-level cases of _cases()"""
    o = fo.Oracle(W, H, qp=12, window=window)
    o.set_frame(f0)
    o.encode_slice(5)
    rec0 = o.frame()
    o.close()
    r = fo.Oracle(W, H, qp=12, window=window)
    r.set_dpb(rec0)
    r.fill_interpolated()
    m = Model([r.kar(k, 0) for k in range(5)])
    r.close()
    g = pkg.FerHip(W, H, 1, qp=12, window=window)
    g.set_reference(rec0[None])
    g.set_frames(f1[None])
    g.inter_encoding()
    assert g.status() == [0]
    n2 = g.read("ST2N")
    st2 = g.read("ST2").reshape(-1, CAP, 2)
    g.close()
    return walk_compare(kind, m, f1[: W * H].reshape(H, W), n2, st2)


def walk_compare(kind, m, cur, n2, st2):
    """the read-backs n2 = ST2N [partitions] and st2 = ST2 [partitions][CAP][2] of source luma `cur` (every column tile
    in reach of every partition: at most 280 samples wide) against the walk model m of its reference"""
    assert m.a.min() > 0, "a sum-0 position would put the stream on the mis-filed bucket layout"
    assert cur.shape[1] <= 280
    mbw = cur.shape[1] // 16
    seen_mid = seen_cap = 0
    for p in range(n2.size):
        mb, part = p // 4, p % 4
        sx, sy = (mb % mbw) * 16 + (part & 1) * 8, (mb // mbw) * 16 + (part >> 1) * 8
        su = _sums(cur, sx, sy)
        ref, jend, slices = m.walk(su, sx, sy)
        mid, cap = _cases(slices, jend, len(ref) > CAP)
        seen_mid += mid
        seen_cap += cap
        if len(ref) > CAP:
            assert n2[p] > CAP, (kind, p, n2[p], len(ref))
            # the summary of a crowded partition starts with the step the walk stopped in
            assert st2[p, 40, 0] == jend, (kind, p)
            continue
        assert n2[p] == len(ref), (kind, p)
        got = [(int(x), int(y)) for x, y in st2[p, : len(ref)]]
        assert got == [(int(np.uint32(rel & 0xffffffff).view(np.int32)), D) for rel, D in ref], (kind, p)
    return seen_mid, seen_cap
