"""Argument checks of the neighbourhood seam (ferhip_intra_mbs, ferhip_mv_mbs; fer_seam_check_intra_mbs / _mv_mbs of
h264-fer_amd/csrc/fer_seam_host.h): one negative case per checked field per entry point, each refused with FERHIP_E_ARG
before the first HIP call -- so on a machine without a GPU too, where the same call with good arguments gets as far as the
first allocation and returns FERHIP_E_HIP (the scheme of test_seam_args_host.py)."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
E_ARG, E_HIP = -1, -2
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib(pkg):
    L = pkg.load_library()
    L.ferhip_intra_mbs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.ferhip_mv_mbs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def good(lib):
    """what a call with good arguments returns here: 0 with a GPU, FERHIP_E_HIP without one"""
    p = lib.ferhip_mem_alloc(16, 0)
    if p:
        lib.ferhip_mem_free(p, 0)
    return 0 if p else E_HIP


def _nb(mb_type, **kw):
    d = dict(mb_type=mb_type, cbp_luma=15, cbp_chroma=2, tc_luma=np.full(16, 16), tc_chroma=np.full(8, 16), i4mode=np.full(16, 8),
             mv=np.tile(np.array([32767, -32768]), 4))
    d.update(kw)
    return d


def _sweep(call, st, name, lo, hi, index=None):
    """every value outside [lo, hi] is refused, both ends are taken"""
    arr = st if index is None else getattr(st, name)
    key = name if index is None else index

    def put(v):
        if index is None:
            setattr(st, name, v)
        else:
            arr[key] = v

    keep = getattr(st, name) if index is None else arr[key]
    for v in (lo - 1, hi + 1, INT_MIN, INT_MAX):
        put(v)
        assert call() == E_ARG, (name, index, v)
    put(keep)


def test_intra_mbs_refuses_bad_jobs(pkg, lib, good):
    F = pkg.ferhip
    pic = dict(Y=np.zeros((32, 48), np.uint8), Cb=np.zeros((16, 24), np.uint8), Cr=np.zeros((16, 24), np.uint8))
    garbage = dict(mb_type=99, cbp_luma=-1, tc_luma=np.full(16, 99), i4mode=np.full(16, -3), mv=np.full(8, 2 ** 20))
    jobs = [
        # ENCODE at pos 0: no entry but the stale type at pos is looked at
        dict(op=F.INTRA_ENCODE, pos=0, slice_type=2, qp=0, mb=[dict(mb_type=31)] + [garbage] * 5, **pic),
        # ENCODE at the top of every range; the entry behind pos is not looked at
        dict(op=F.INTRA_ENCODE, pos=4, slice_type=2, qp=51, chroma_qp_offset=12, constrained_intra=1, mb=[_nb(24), _nb(0), _nb(31), _nb(1), dict(mb_type=24), garbage], **pic),
        # DECODE, P slice, Intra4x4 among every kind of neighbour, levels at the ends of 16 bits
        dict(op=F.INTRA_DECODE, pos=5, slice_type=0, qp=51, chroma_qp_offset=-12, constrained_intra=0, chroma_mode=3, prev_flag=np.ones(16), rem_mode=np.full(16, 7),
             mb=[_nb(4), _nb(5), _nb(29), _nb(31), _nb(0), dict(mb_type=5)], lumaLevel=np.full(256, 32767), cac=np.full(128, -32768), **pic),
        # DECODE, I slice, Intra16x16 plane prediction at pos 4
        dict(op=F.INTRA_DECODE, pos=4, slice_type=2, qp=30, chroma_mode=1, mb=[_nb(0), _nb(1), _nb(24), _nb(31), dict(mb_type=24), garbage], dc16=np.full(16, -32768), **pic),
    ]
    n = len(jobs)
    J, R = F.nbhd_jobs(jobs), (F.IntraResult * n)()

    def call():
        return lib.ferhip_intra_mbs(J, R, n)

    assert call() == good
    assert lib.ferhip_intra_mbs(None, R, n) == E_ARG
    assert lib.ferhip_intra_mbs(J, None, n) == E_ARG
    assert lib.ferhip_intra_mbs(J, R, 0) == E_ARG
    assert lib.ferhip_intra_mbs(J, R, (1 << 20) + 1) == E_ARG     # (refused before any job is read)
    for name, lo, hi in (("op", 0, 1), ("pos", 0, 5), ("qp", 0, 51), ("chroma_qp_offset", -12, 12), ("constrained_intra", 0, 1)):
        _sweep(call, J[1], name, lo, hi)
    for v in (1, 3, 5, 7, -1, INT_MAX):                           # slice_type: 0 (P) or 2 (I)
        J[2].slice_type = v
        assert call() == E_ARG, v
    J[2].slice_type = 0
    J[1].slice_type = 0                                           # ENCODE is for I slices
    assert call() == E_ARG
    J[1].slice_type = 2
    for v in (25, 30, 32, -1, INT_MAX):                           # the stale entry: a type of an I slice or P_Skip, no I_PCM
        J[1].mb[4].mb_type = v
        assert call() == E_ARG, v
    J[1].mb[4].mb_type = 31
    assert call() == good
    N = J[2].mb[1]                                                # a neighbour in front of pos, P slice
    for v in (30, 32, -1, INT_MIN, INT_MAX):
        N.mb_type = v
        assert call() == E_ARG, v
    N.mb_type = 5
    J[3].mb[2].mb_type = 25                                       # ... I slice: 0..24 or 31
    assert call() == E_ARG
    J[3].mb[2].mb_type = 24
    _sweep(call, N, "cbp_luma", 0, 15)
    _sweep(call, N, "cbp_chroma", 0, 2)
    for arr, hi in (("tc_luma", 16), ("tc_chroma", 16), ("i4mode", 8)):
        for i in (0, len(getattr(N, arr)) - 1):
            _sweep(call, N, arr, 0, hi, index=i)
    for i in (0, 7):
        _sweep(call, N, "mv", -32768, 32767, index=i)
    D = J[2]
    for v in (0, 4, 30, 31, -1):                                  # DECODE: the macroblock is intra
        D.mb[5].mb_type = v
        assert call() == E_ARG, v
    D.mb[5].mb_type = 5
    J[3].mb[4].mb_type = 31
    assert call() == E_ARG
    J[3].mb[4].mb_type = 24
    _sweep(call, D, "chroma_mode", 0, 3)
    for i in (0, 15):
        _sweep(call, D, "prev_flag", 0, 1, index=i)
        _sweep(call, D, "rem_mode", 0, 7, index=i)
    for arr in ("lumaLevel", "dc16", "ac16", "cdc", "cac"):
        for i in (0, len(getattr(D, arr)) - 1):
            _sweep(call, D, arr, -32768, 32767, index=i)
    assert call() == good
    # jobs that are not legal: a mode that reads a neighbour pos does not provide
    for pos, cm in ((0, 1), (0, 2), (0, 3), (1, 2), (2, 3), (3, 1), (3, 3)):
        keep = (J[3].pos, J[3].chroma_mode, J[3].mb[J[3].pos].mb_type)
        J[3].pos, J[3].chroma_mode = pos, cm
        J[3].mb[pos].mb_type = 3                                  # Intra16x16 DC
        assert call() == E_ARG, (pos, cm)
        J[3].chroma_mode = 0
        assert call() == good, pos
        J[3].pos, J[3].chroma_mode = keep[0], keep[1]
        J[3].mb[pos].mb_type = 1 if pos else 31
        J[3].mb[keep[0]].mb_type = keep[2]
    for pos, t in ((0, 1), (0, 2), (0, 4), (1, 1), (2, 4), (3, 2), (3, 4)):   # Intra16x16 vertical, horizontal, plane
        keep = (J[3].pos, J[3].chroma_mode)
        J[3].pos, J[3].chroma_mode, J[3].mb[pos].mb_type = pos, 0, t
        assert call() == E_ARG, (pos, t)
        J[3].pos, J[3].chroma_mode = keep
        J[3].mb[pos].mb_type = 1
    J[3].mb[4].mb_type = 24
    assert call() == good
    # Intra4x4 at pos 0: every block predicts DC; rem_mode 0 below it = vertical, which reads the missing row above
    D.pos, D.chroma_mode = 0, 0
    D.mb[0].mb_type = 5
    assert call() == good
    D.prev_flag[0], D.rem_mode[0] = 0, 0
    assert call() == E_ARG
    D.rem_mode[0] = 1                                             # horizontal: the missing column
    assert call() == E_ARG
    D.rem_mode[0] = 2                                             # at the prediction: mode 3, up-left diagonal down: the row above again
    assert call() == E_ARG
    D.prev_flag[0] = 1
    D.prev_flag[3], D.rem_mode[3] = 0, 3                          # block 3 lies inside: every mode has its samples
    assert call() == good


def test_mv_mbs_refuses_bad_jobs(pkg, lib, good):
    F = pkg.ferhip
    flat = np.tile(np.array([32767, -32768]), 4)
    jobs = [
        dict(op=F.MV_DERIVE, pos=0, mb_type=31, sub_mb_type=np.full(4, 0), mb=[dict(mb_type=99, mv=np.full(8, 2 ** 20))] * 6),
        dict(op=F.MV_DERIVE, pos=5, mb_type=4, sub_mb_type=np.full(4, 3), mvd=np.array([65536, -65536] * 4),
             mb=[_nb(0), _nb(29), _nb(31), _nb(3, mv=np.arange(8)), _nb(1, mv=np.array([1, 2, 1, 2, 3, 4, 3, 4])), dict(mb_type=99)]),
        dict(op=F.MV_PREDICT, pos=4, mb_type=2, sub_mb_type=np.zeros(4), mv=np.array([5, 6, 7, 8, 5, 6, 7, 8]), mvd=np.full(8, 2 ** 30),
             mb=[_nb(0), _nb(2, mv=np.array([1, 2, 3, 4, 1, 2, 3, 4])), _nb(31), _nb(4, mv=np.arange(8)), dict(mb_type=99), dict(mb_type=99)]),
    ]
    n = len(jobs)
    J, R = F.nbhd_jobs(jobs, mv=True), (F.MvResult * n)()

    def call():
        return lib.ferhip_mv_mbs(J, R, n)

    assert call() == good
    assert lib.ferhip_mv_mbs(None, R, n) == E_ARG
    assert lib.ferhip_mv_mbs(J, None, n) == E_ARG
    assert lib.ferhip_mv_mbs(J, R, 0) == E_ARG
    _sweep(call, J[1], "op", 0, 1)
    _sweep(call, J[1], "pos", 0, 5)
    for v in (5, 29, 30, 32, -1, INT_MAX):                        # DERIVE: 0..4 or P_Skip
        J[1].mb_type = v
        assert call() == E_ARG, v
    J[1].mb_type = 4
    for v in (5, 31, -1):                                         # PREDICT: 0..4 (k_p_resid writes no difference for P_Skip)
        J[2].mb_type = v
        assert call() == E_ARG, v
    J[2].mb_type = 2
    for i in (0, 3):
        _sweep(call, J[1], "sub_mb_type", 0, 3, index=i)
        _sweep(call, J[2], "sub_mb_type", 0, 0, index=i)
    for i in (0, 7):
        _sweep(call, J[1], "mvd", -65536, 65536, index=i)
        _sweep(call, J[2], "mv", -32768, 32767, index=i)
        _sweep(call, J[1].mb[1], "mv", -32768, 32767, index=i)
    for v in (30, 32, -1, INT_MAX):
        J[1].mb[2].mb_type = v
        assert call() == E_ARG, v
    J[1].mb[2].mb_type = 31
    # the quadrants of one partition carry one vector: neighbours, and the macroblock of a PREDICT job
    for m, i in ((0, 7), (2, 3), (4, 2), (4, 7)):                 # 16x16, P_Skip, 16x8 upper, 16x8 lower
        J[1].mb[m].mv[i] += 1
        assert call() == E_ARG, (m, i)
        J[1].mb[m].mv[i] -= 1
    J[2].mb[1].mv[4] += 1                                         # 8x16, left
    assert call() == E_ARG
    J[2].mb[1].mv[4] -= 1
    J[2].mv[5] += 1
    assert call() == E_ARG
    J[2].mv[5] -= 1
    J[2].mb[0].mb_type = 7                                        # PREDICT: every neighbour is inter, as in the encoder's P pictures
    assert call() == E_ARG
    J[2].mb[0].mb_type = 0
    assert call() == good


def test_seam_nbhd_host_check_program(tmp_path):
    """tools/seam_nbhd_host_check.cpp, the same checks as a stand-alone program over heap arrays of the exact sizes (its place
    under AddressSanitizer + UBSan is a developer's run, see the file): built plainly here, it must exit 0."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        return
    exe = tmp_path / "seam_nbhd_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "seam_nbhd_host_check.cpp"), "-o", str(exe)], check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
