"""SPEC_STAT is kept in one slot per workgroup of the motion chain and summed on read-back.

176x144 x 17 streams (the eight ticket queues), three pictures: the four totals must not depend on the chain's grid -- 1, 7,
64 and 3072 workgroups (the last is capped at the 306 rows of the picture set) -- nor on a change of the grid between two
pictures, where a smaller grid must not lose what the larger one's workgroups had counted.  `partitions the chain decided`
is the number of partitions the oracle searched in the same pictures.  Every fifth stream is a still sequence, so P_Skip
verdicts and skipped partitions occur.  Every comparison is exact equality.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, S, T = 176, 144, 17, 3
NMB = (W // 16) * (H // 16)
_CACHE = {}


def _frames(pkg):
    if "frames" not in _CACHE:
        _CACHE["frames"] = np.stack([np.stack([pkg.gen_frame(W, H, 0 if s % 5 == 4 else t, 1234 + s, 0 if s % 5 == 4 else 2)
                                               for s in range(S)]) for t in range(T)])
    return _CACHE["frames"]


def _oracle_searched(pkg, fo):
    """partitions the oracle searched over the P pictures of all streams, and its RBSPs [t][s]"""
    if "searched" not in _CACHE:
        frames = _frames(pkg)
        total, rbsp = 0, [[None] * S for _ in range(T)]
        for s in range(S):
            o = fo.Oracle(W, H, qp=12, window=16, maxdiff=3, intra_every=30)
            o.record_me(True)
            for t in range(T):
                o.set_frame(frames[t, s])
                nal = int(o.L.fo_select_nal_type(o.c))
                assert nal == (5 if t == 0 else 1)
                rbsp[t][s] = o.encode_slice(nal)
                if t > 0:
                    total += int(o.me_lists()["searched"].sum())
            o.close()
        _CACHE["searched"], _CACHE["rbsp"] = total, rbsp
    return _CACHE["searched"], _CACHE["rbsp"]


def _spec_stat(pkg, fo, grids):
    """grids[t] = workgroups of the chain for picture t"""
    frames = _frames(pkg)
    _, want = _oracle_searched(pkg, fo)
    g = pkg.FerHip(W, H, S, qp=12, window=16, maxdiff=3, intra_every=30)
    try:
        for t in range(T):
            g.tune(pkg.TUNE_RESOLVE_WGS, grids[t])
            g.set_frames(frames[t])
            rbsp, _ = g.encode_picture()
            assert rbsp == want[t], f"picture {t}"
        assert g.status() == [0] * S
        st = g.read("SPEC_STAT")
    finally:
        g.close()
    assert st.shape == (8,) and not st[4:].any()
    return [int(v) for v in st[:4]]


def _reference_totals(pkg, fo):
    if "totals" not in _CACHE:
        _CACHE["totals"] = _spec_stat(pkg, fo, [64] * T)
    return _CACHE["totals"]


@pytest.mark.parametrize("grid", [1, 7, 64, 3072])
def test_totals_do_not_depend_on_the_grid(pkg, fo, grid):
    st = _spec_stat(pkg, fo, [grid] * T)
    searched, _ = _oracle_searched(pkg, fo)
    parts, hits, skq, skh = st
    assert parts == searched, "partitions decided by the chain == partitions the oracle searched"
    assert skq == S * (T - 1) * NMB and 0 < skh <= skq and 0 < hits <= parts
    assert parts < 4 * skq, "the still streams are meant to leave skipped partitions out"
    assert st == _reference_totals(pkg, fo)


@pytest.mark.parametrize("grids", [[64, 3072, 7], [64, 7, 3072], [1, 64, 1]])
def test_grid_changed_between_pictures_loses_nothing(pkg, fo, grids):
    assert _spec_stat(pkg, fo, grids) == _reference_totals(pkg, fo)
