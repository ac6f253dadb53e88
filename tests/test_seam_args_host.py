"""Argument checks of the per-macroblock entry points (ferhip_mb_unit, ferhip_cavlc_blocks, ferhip_cavlc_parse_blocks,
ferhip_residual_mbs, ferhip_mc_sub_mb_parts; h264-fer_amd/csrc/fer_seam_host.h).  The kernels behind them index device
tables with what the caller states, so a bad argument must be refused with FERHIP_E_ARG before the first HIP call: it is,
then, refused on a machine without a GPU too, where the same call with good arguments gets as far as the first
allocation and returns FERHIP_E_HIP."""
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
    vp, sz = C.c_void_p, C.c_size_t
    L.ferhip_mb_unit.argtypes = [vp, vp, sz]
    L.ferhip_cavlc_blocks.argtypes = [vp] * 3 + [sz] + [vp] * 3
    L.ferhip_cavlc_parse_blocks.argtypes = [vp, sz] + [vp] * 3 + [sz] + [vp] * 3
    L.ferhip_residual_mbs.argtypes = [vp, vp, sz]
    L.ferhip_mc_sub_mb_parts.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def good(lib):
    """what a call with good arguments returns here: 0 with a GPU, FERHIP_E_HIP without one"""
    p = lib.ferhip_mem_alloc(16, 0)
    if p:
        lib.ferhip_mem_free(p, 0)
    return 0 if p else E_HIP


def _ptr(a):
    return a.ctypes.data if a is not None else None


def test_mb_unit_refuses_bad_jobs(pkg, lib, good):
    n = 2
    J, R = (pkg.ferhip.MbJob * n)(), (pkg.ferhip.MbResult * n)()
    J[1].op, J[1].cls, J[1].qp, J[1].qpc, J[1].blk = 4, 2, 51, 51, 15
    assert lib.ferhip_mb_unit(J, R, n) == good
    assert lib.ferhip_mb_unit(None, R, n) == E_ARG
    assert lib.ferhip_mb_unit(J, None, n) == E_ARG
    assert lib.ferhip_mb_unit(J, R, 0) == E_ARG
    for name, hi in (("op", 4), ("cls", 2), ("qp", 51), ("qpc", 51), ("blk", 15)):
        keep = getattr(J[1], name)
        for v in (-1, hi + 1, INT_MIN, INT_MAX):
            setattr(J[1], name, v)
            assert lib.ferhip_mb_unit(J, R, n) == E_ARG, (name, v)
        setattr(J[1], name, keep)
    assert lib.ferhip_mb_unit(J, R, n) == good


def _block_args(n=4):
    return dict(coef=np.ones((n, 16), np.int32), nC=np.array([0, 5, 16, -1], np.int32), mx=np.array([16, 15, 16, 4], np.int32),
                bits=np.zeros((n, 64), np.uint8), nb=np.zeros(n, np.uint32), tc=np.zeros(n, np.int32))


BAD_BLOCKS = [(1, "mx", m) for m in (0, 3, 5, 14, 17, -1, INT_MAX)] + [(1, "nC", -2), (1, "nC", INT_MIN), (1, "nC", -1), (2, "nC", -1)]


def test_cavlc_blocks_refuses_bad_blocks(lib, good):
    a = _block_args()
    order = ("coef", "nC", "mx", None, "bits", "nb", "tc")

    def call(n=4, null=None):
        return lib.ferhip_cavlc_blocks(*[n if k is None else (None if k == null else _ptr(a[k])) for k in order])

    assert call() == good
    assert call(n=0) == E_ARG
    for k in order:
        if k:
            assert call(null=k) == E_ARG, k
    for i, k, v in BAD_BLOCKS:   # maxNumCoeff outside {4, 15, 16}; nC < -1; nC == -1 (chroma DC) with maxNumCoeff 15 / 16
        keep = a[k][i]
        a[k][i] = v
        assert call() == E_ARG, (i, k, v)
        a[k][i] = keep
    assert call() == good


def test_cavlc_parse_blocks_refuses_bad_blocks_and_positions(lib, good):
    a = _block_args()
    a.update(stream=np.zeros(7, np.uint8), pos=np.array([0, 8, 31, 55], np.uint64), used=np.zeros(4, np.uint32))
    order = ("stream", "nbytes", "pos", "nC", "mx", None, "coef", "tc", "used")

    def call(n=4, nbytes=7, null=None):
        return lib.ferhip_cavlc_parse_blocks(*[n if k is None else nbytes if k == "nbytes" else (None if k == null else _ptr(a[k])) for k in order])

    assert call() == good
    assert call(n=0) == E_ARG
    assert call(nbytes=0) == E_ARG
    assert call(nbytes=6) == E_ARG            # position 55 lies behind 48 bits
    assert call(nbytes=2 ** 28 + 1) == E_ARG  # the device reader keeps positions in 32 bits
    for k in order:
        if k and k != "nbytes":
            assert call(null=k) == E_ARG, k
    for v in (56, 2 ** 32, 2 ** 32 + 8, 2 ** 64 - 1):   # at or behind 8 * nbytes, values that wrap in 32 bits included
        a["pos"][3] = v
        assert call() == E_ARG, v
    a["pos"][3] = 55
    for i, k, v in BAD_BLOCKS:
        keep = a[k][i]
        a[k][i] = v
        assert call() == E_ARG, (i, k, v)
        a[k][i] = keep
    assert call() == good


def test_mc_sub_mb_parts_refuses_bad_indices(lib, good):
    W, H = 48, 32
    ref = np.zeros(W * H * 3 // 2, np.uint8)
    desc = np.array([[0, 0, 0, 0, 0], [5, 3, 3, 2 ** 30, -2 ** 30]], np.int32)   # (vectors are clamped, not checked)
    pl, pb, pr = np.zeros(32, np.int32), np.zeros(8, np.int32), np.zeros(8, np.int32)

    def call(w=W, h=H, n=2, null=None):
        p = {k: (None if k == null else _ptr(v)) for k, v in dict(ref=ref, desc=desc, pl=pl, pb=pb, pr=pr).items()}
        return lib.ferhip_mc_sub_mb_parts(p["ref"], w, h, p["desc"], n, p["pl"], p["pb"], p["pr"])

    assert call() == good
    assert call(h=16) == E_ARG   # macroblock 5 is not in a 3 x 1 picture
    assert call(w=0) == E_ARG and call(h=-16) == E_ARG and call(w=W + 8) == E_ARG and call(n=0) == E_ARG
    for k in ("ref", "desc", "pl", "pb", "pr"):
        assert call(null=k) == E_ARG, k
    for col, hi in ((0, 5), (1, 3), (2, 3)):
        keep = desc[1, col]
        for v in (-1, hi + 1, INT_MIN, INT_MAX):
            desc[1, col] = v
            assert call() == E_ARG, (col, v)
        desc[1, col] = keep
    assert call() == good


def test_residual_mbs_refuses_bad_jobs(pkg, lib, good):
    F = pkg.ferhip
    full = dict(p_skip=1, cbp_luma=15, cbp_chroma=2, tc_luma=np.full(16, 16), tc_chroma=np.full(8, 16))
    jobs = [
        # WRITE without neighbours: their records are not looked at
        dict(op=F.RES_WRITE, cls=0, avail=0, nb=(dict(p_skip=7, cbp_luma=-1), dict(tc_luma=np.full(16, 99)))),
        # WRITE at the top of every range
        dict(op=F.RES_WRITE, cls=1, cbp_luma=15, cbp_chroma=2, avail=3, nb=(full, full), lumaLevel=np.full(256, 32767), cac=np.full(128, -32768)),
        # PARSE of a full buffer at its last bit; levels are an input of WRITE only
        dict(op=F.RES_PARSE, cls=2, avail=1, nb=(full, None), bits=np.zeros(F.RES_BITS_MAX, np.uint8), bit_pos=F.RES_BITS_MAX * 8 - 1, dc16=np.full(16, 2 ** 20)),
    ]
    n = len(jobs)
    J, R = F.residual_jobs(jobs), (F.ResResult * n)()

    def call():
        return lib.ferhip_residual_mbs(J, R, n)

    assert call() == good
    assert lib.ferhip_residual_mbs(None, R, n) == E_ARG
    assert lib.ferhip_residual_mbs(J, None, n) == E_ARG
    assert lib.ferhip_residual_mbs(J, R, 0) == E_ARG
    for name, hi in (("op", 1), ("cls", 2), ("cbp_luma", 15), ("cbp_chroma", 2), ("avail", 3)):
        keep = getattr(J[2], name)
        for v in (-1, hi + 1, INT_MIN, INT_MAX):
            setattr(J[2], name, v)
            assert call() == E_ARG, (name, v)
        setattr(J[2], name, keep)
    J[1].cbp_luma = 7            # Intra16x16 codes all of its AC blocks or none
    assert call() == E_ARG
    J[1].cbp_luma = 15
    for k in range(2):           # the records of neighbours that exist
        N = J[1].nb[k]
        for name, hi in (("p_skip", 1), ("cbp_luma", 15), ("cbp_chroma", 2)):
            keep = getattr(N, name)
            for v in (-1, hi + 1, INT_MIN, INT_MAX):
                setattr(N, name, v)
                assert call() == E_ARG, (k, name, v)
            setattr(N, name, keep)
        for arr, i in ((N.tc_luma, 0), (N.tc_luma, 15), (N.tc_chroma, 0), (N.tc_chroma, 7)):
            for v in (-1, 17, INT_MAX):
                arr[i] = v
                assert call() == E_ARG, (k, i, v)
            arr[i] = 16
    for pos, nbytes in ((F.RES_BITS_MAX * 8, F.RES_BITS_MAX), (2 ** 32 - 1, F.RES_BITS_MAX), (0, F.RES_BITS_MAX + 1), (0, 2 ** 32 - 1),
                        (0, 2 ** 29), (0, 0), (8, 1)):   # a bit_pos at or behind 8 * nbytes; nbytes 0, above the buffer, wrapping
        J[2].bit_pos, J[2].nbytes = pos, nbytes
        assert call() == E_ARG, (pos, nbytes)
    J[2].bit_pos, J[2].nbytes = 7, 1
    assert call() == good
    for v in (32768, -32769):    # WRITE: levels the device's 16 bits cannot hold
        J[1].dc16[5] = v
        assert call() == E_ARG, v
    J[1].dc16[5] = 0
    assert call() == good


def test_seam_host_check_program(tmp_path):
    """tools/seam_host_check.cpp, the same checks as a stand-alone program over heap arrays of the exact sizes (its place under
    AddressSanitizer + UBSan is a developer's run, see the file): built plainly here, it must exit 0."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        return
    exe = tmp_path / "seam_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "seam_host_check.cpp"), "-o", str(exe)], check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
