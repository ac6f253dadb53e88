"""The picture-by-picture oracle comparison of streams whose QP changes between pictures, shared by test_gpu_rate_control.py,
test_gpu_quality.py and test_gpu_qp_sweep.py.

A picture coded at QP q depends only on q and its inputs, so the oracle is driven picture by picture: set_frame,
fo_select_nal_type, fo_set_params(q) + a discarded fo_write_pps (which moves the oracle's QPy), encode_slice, frame().
Its slice headers always carry slice_qp_delta = -14; the library's carry q - base - 14, so slice data are compared
bit for bit after the header and the header's slice_qp_delta is checked as a value."""
import ctypes as C

import numpy as np
from rate_model import CQP

IDR, SLICE = 5, 1


def frames(pkg, W, H, T, S, seed=1234, cut=None):
    """[T][S][fsz]; from picture `cut` on every stream shows the negative (a scene cut)"""
    def f(t, s):
        x = pkg.gen_frame(W, H, t, seed + s, 2)
        return 255 - x if cut is not None and t >= cut else x
    return np.stack([np.stack([f(t, s) for s in range(S)]) for t in range(T)])


class Bits:
    def __init__(self, b):
        self.s = "".join(format(x, "08b") for x in b)
        self.p = 0

    def u(self, n):
        v = int(self.s[self.p:self.p + n], 2) if n else 0
        self.p += n
        return v

    def ue(self):
        z = 0
        while self.s[self.p] == "0":
            z += 1
            self.p += 1
        self.p += 1
        return (1 << z) - 1 + self.u(z)

    def se(self):
        v = self.ue()
        return (v + 1) // 2 if v & 1 else -(v // 2)


def split_slice(rbsp, nal_type):
    """-> (header bits before slice_qp_delta, slice_qp_delta, slice data bits up to the stop bit)"""
    r = Bits(rbsp)
    r.ue()
    st = r.ue()
    r.ue()
    r.u(9)
    if nal_type == IDR:
        r.ue()
    r.u(10)
    r.u(3 if st == 0 else 2)
    head = r.s[:r.p]
    dq = r.se()
    return head, dq, r.s[r.p:].rstrip("0")


def oracle_lib(fo):
    L = fo.lib()
    L.fo_write_pps.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.fo_write_pps.restype = C.c_size_t
    L.fo_select_nal_type.argtypes = [C.c_void_p]
    return L


def oracle_pictures(fo, frames, qps, W, H, window=16, intra_every=30, types=None):
    """one stream, picture by picture at the QPs given -> list of (nal type, rbsp, recon), brojTipova"""
    L = oracle_lib(fo)
    o = fo.Oracle(W, H, qp=qps[0], window=window, maxdiff=3, intra_every=intra_every)
    buf = np.empty(4096, np.uint8)
    out = []
    for t, q in enumerate(qps):
        o.set_frame(frames[t])
        nt = L.fo_select_nal_type(o.c) if types is None else types[t]
        L.fo_set_params(o.c, int(q), 0, window, 3, intra_every)
        L.fo_write_pps(o.c, buf.ctypes.data, buf.size)
        out.append((nt, o.encode_slice(nt), o.frame()))
    stats = list(o.stats())
    o.close()
    return out, stats


def check_pictures(gpu, base, ora, what):
    """gpu: list of (nal type, rbsp, recon, qp) of one stream; ora: oracle_pictures' list"""
    assert len(gpu) == len(ora)
    for t, ((nt, rb, rec, q), (ont, orb, orec)) in enumerate(zip(gpu, ora)):
        assert nt == ont, f"{what} picture {t}: type"
        assert np.array_equal(rec, orec), f"{what} picture {t}: recon at qp {q}"
        gh, gdq, gdata = split_slice(rb, nt)
        oh, odq, odata = split_slice(orb, ont)
        assert odq == -14 and gdq == q - base - 14, f"{what} picture {t}: slice_qp_delta {gdq} at qp {q}, base {base}"
        assert gh == oh, f"{what} picture {t}: slice header"
        assert gdata == odata, f"{what} picture {t}: slice data at qp {q}"


def encode_by_picture(g, frames, qp_sched=None, types=None):
    """host path picture by picture; qp_sched[t][s]: CQP QPs set before picture t (None: leave that stream's rate as it is)
    -> per stream list of (nal type, rbsp, recon, qp)"""
    T, S = frames.shape[0], frames.shape[1]
    res = [[] for _ in range(S)]
    for t in range(T):
        if qp_sched is not None:
            for s in range(S):
                if qp_sched[t][s] is not None:
                    g.set_rate(s, CQP, qp=int(qp_sched[t][s]))
        g.set_frames(frames[t])
        rbsp, nt = g.encode_picture(None if types is None else types[t])
        rec = g.get_recon()
        qps = g.last_qp()
        for s in range(S):
            res[s].append((nt[s], rbsp[s], rec[s], qps[s]))
    return res
