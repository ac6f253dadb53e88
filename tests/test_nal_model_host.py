"""The closed form of NAL framing in tests/nal_model.py against the two byte loops it has to equal: the oracle's fo_write_nal and
the library's host ferhip_write_nal (both restate writeNAL, F/nal.cpp:261-299).  This pins the model that the device kernels
of ferhip_pack_nal are checked against (tests/test_gpu_nal_pack.py); it needs no GPU and passes without those kernels."""
import ctypes as C

import numpy as np

import nal_model


def _byte_loop(fn, nal_type, payload):
    p = np.ascontiguousarray(payload, np.uint8)
    out = np.empty(p.size * 3 // 2 + 16, np.uint8)
    n = fn(1, nal_type, C.c_void_p(p.ctypes.data), C.c_size_t(p.size), C.c_void_p(out.ctypes.data))
    return out[:n].tobytes()


def test_closed_form_small_cases():
    f = nal_model.frame_nal
    assert f(5, b"") == b"\0\0\0\1\x25"
    assert f(1, [0, 0, 0]) == b"\0\0\0\1\x21\0\0\3\0"
    assert f(1, [0, 0, 1]) == b"\0\0\0\1\x21\0\0\3\1"
    assert f(1, [0, 0, 4]) == b"\0\0\0\1\x21\0\0\4"
    assert f(1, [0, 0, 0, 0, 0]) == b"\0\0\0\1\x21\0\0\3\0\0\3\0"   # before z2 and z4
    assert f(1, [0, 0, 0, 1]) == b"\0\0\0\1\x21\0\0\3\0\1"          # L = 3 is odd: nothing before the 01
    assert f(1, [0, 0, 0, 0, 3]) == b"\0\0\0\1\x21\0\0\3\0\0\3\3"   # L = 4 is even


def test_model_equals_both_byte_loops(pkg, fo):
    lib = pkg.load_library()
    fo_fn = fo.lib().fo_write_nal
    fo_fn.restype = C.c_size_t
    hip_fn = lib.ferhip_write_nal
    corpus = nal_model.corpus()
    assert len(corpus) >= 800
    inserted = 0
    for k, (p, t) in enumerate(corpus):
        want = nal_model.frame_nal(t, p)
        inserted += len(want) - 5 - p.size
        assert _byte_loop(fo_fn, t, p) == want, f"payload {k} ({p.size} bytes): model differs from fo_write_nal"
        assert _byte_loop(hip_fn, t, p) == want, f"payload {k} ({p.size} bytes): model differs from ferhip_write_nal"
    assert inserted > 100000  # the corpus is about escaping
