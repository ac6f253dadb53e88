"""The refusals of the SRTP entry points that need no device (include/ferhip.h; the checks stand in
h264-fer_amd/csrc/fer_srtp_host.h): a bad argument is refused with FERHIP_E_ARG, and a stream without a key with
FERHIP_E_STATE, before the first HIP call -- so on a machine without a GPU too, where the same call with good arguments gets
as far as the first allocation and returns FERHIP_E_HIP.  ferhip_srtp_derive is host code altogether."""
import ctypes as C

import numpy as np
import pytest

import srtp_model as sm

E_ARG, E_HIP, E_STATE = -1, -2, -3
MASTERS = [(bytes(range(s, s + 16)), bytes(range(50 + s, 64 + s))) for s in range(3)]


@pytest.fixture(scope="module")
def good(pkg):
    """what a call with good arguments returns here: 0 with a GPU, FERHIP_E_HIP without one"""
    lib = pkg.load_library()
    p = lib.ferhip_mem_alloc(16, 0)
    if p:
        lib.ferhip_mem_free(p, 0)
    return 0 if p else E_HIP


def _case(pkg):
    packets = [sm.rtp_packet(b"abc", 1), sm.rtp_packet(b"defgh", 2, cc=1)]
    base = b"".join(packets)
    t = np.zeros(2, pkg.RTP_PKT)
    t[0], t[1] = (0, len(packets[0]), 0), (len(packets[0]), len(packets[1]), 2)
    return base, t


def test_derive_is_the_models_and_rfc_3711_b3(pkg):
    k_e, k_a, k_s = pkg.srtp_derive(bytes.fromhex("E1F97A0D3E018BE0D64FA32C06DE4139"), bytes.fromhex("0EC675AD498AFEEBB6960B3AABE6"))
    assert k_e.hex().upper() == "C61E7A93744F39EE10734AFE3FF7A087" and k_s.hex().upper() == "30CBBC08863D8C85D49DB34A9AE1"
    assert k_a.hex().upper() == "CEBE321F6FF7716B6FD4AB49AF256A156D38BAA4"
    for m in MASTERS:
        assert pkg.srtp_derive(*m) == sm.derive(*m)
    lib = pkg.load_library()
    buf = np.zeros(50, np.uint8)
    assert lib.ferhip_srtp_derive(None, buf.ctypes.data, buf.ctypes.data) == E_ARG and lib.ferhip_srtp_derive(buf.ctypes.data, None, buf.ctypes.data) == E_ARG
    assert lib.ferhip_srtp_derive(buf.ctypes.data, buf.ctypes.data, None) == E_ARG


def test_blocks_refusals_come_before_the_device(pkg, good):
    base, t = _case(pkg)
    st = [(0, 0, 0)] * 3
    assert pkg.srtp_blocks_raw(0, MASTERS, st, base, t)[0] == good and pkg.srtp_blocks_raw(1, MASTERS, st, base, t)[0] == good
    for op in (2, -1, 256):
        assert pkg.srtp_blocks_raw(op, MASTERS, st, base, t)[0] == E_ARG
    assert pkg.srtp_blocks_raw(0, MASTERS[:2], st[:2], base, t)[0] == E_ARG, "stream >= S"
    assert pkg.srtp_blocks_raw(0, MASTERS[:2] + [None], st, base, t)[0] == E_STATE, "a stream whose key was never set"
    assert pkg.srtp_blocks_raw(0, MASTERS[:2] + [None], st, base, t[:1])[0] == good
    assert pkg.srtp_blocks_raw(0, MASTERS, st, base[:-1], t)[0] == E_ARG, "a row that leaves base"
    far = t.copy()
    far["offset"][1] = 2 ** 64 - 2
    assert pkg.srtp_blocks_raw(0, MASTERS, st, base, far)[0] == E_ARG
    for m in (-1, 16):
        assert pkg.srtp_blocks_raw(0, MASTERS, st, base, t, misalign=m)[0] == E_ARG
    keys = pkg.srtp_keys(MASTERS)
    keys["reserved"][1] = 1
    assert pkg.srtp_blocks_raw(0, keys, st, base, t)[0] == E_ARG
    assert pkg.srtp_blocks_raw(0, MASTERS, [(0, 0, 2)] * 3, base, t)[0] == E_ARG
    # null pointers, and a null buffer with a cap
    lib = pkg.load_library()
    keys, s0, s1 = pkg.srtp_keys(MASTERS), np.zeros(3, pkg.SRTP_INDEX), np.zeros(3, pkg.SRTP_INDEX)
    b, out, tab, stat = np.frombuffer(base, np.uint8), np.zeros(256, np.uint8), np.zeros(3, pkg.RTP_PKT), np.zeros(2, np.int32)

    def call(op=0, k=keys.ctypes.data, a=s0.ctypes.data, n=3, bp=b.ctypes.data, rows=t.ctypes.data, o=out.ctypes.data, cap=256, tp=tab.ctypes.data,
             sp=stat.ctypes.data, z=s1.ctypes.data):
        return lib.ferhip_srtp_blocks(op, k, a, n, bp, b.size, rows, 2, 0, o, cap, tp, sp, z)

    assert call() == good and call(op=1) == good and call(sp=None) == good and call(o=None, cap=0) == good
    for kw in (dict(k=None), dict(a=None), dict(n=0), dict(n=65536), dict(bp=None), dict(rows=None), dict(o=None), dict(tp=None), dict(z=None),
               dict(op=1, sp=None)):
        assert call(**kw) == E_ARG, kw


def test_session_calls_refuse_null_handles(pkg):
    lib = pkg.load_library()
    vp = C.c_void_p
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    assert lib.ferhip_srtp_create(None, 3) == E_ARG
    h = vp()
    for n in (0, -1, 65536):
        assert lib.ferhip_srtp_create(C.byref(h), n) == E_ARG and not h.value
    assert lib.ferhip_srtp_set_key(None, 0, p, p) == E_ARG and lib.ferhip_srtp_set_index(None, 0, 0, 0, 0) == E_ARG
    assert lib.ferhip_srtp_get_index(None, 0, C.byref(C.c_uint32()), C.byref(C.c_uint32()), C.byref(C.c_int())) == E_ARG
    assert lib.ferhip_srtp_protect(None, None, vp(p), vp(p), 1, vp(p), 16, vp(p)) == E_ARG
    assert lib.ferhip_srtp_protect_dev(None, None, vp(p), vp(p), 1, vp(p), 16, vp(p)) == E_ARG
    assert lib.ferhip_srtp_unprotect(None, None, vp(p), 0, vp(p), 1, vp(p), 16, vp(p), vp(p)) == E_ARG
    lib.ferhip_srtp_destroy(None)
