"""Every QP 0..51 on whole pictures: the inputs and the oracle's side, shared by test_qp_sweep_host.py and test_gpu_qp_sweep.py.

Five streams of four 64x48 pictures (12 macroblocks, the interior ones with neighbours A, B, C and D), coded IDR, P, P, P
(hard_content.NAL_TYPES) with window 16 and maxdiff 3 at each of the 52 QPs:

  "mild"       synth.gen_frame(64, 48, t, 77, 4), t = 0..3: small levels, under the level guard at every QP
  20, 21, 22   hard_content.sequence(64, 48, seed): saturated mosaics that keep coding luma and chroma residuals up to QP 51;
               under the guard from QP 9, 3 and 5 on
  "noisy"      synth.gen_frame(64, 48, t, 80, 24): the second stream under the guard at QP 0..2, where no mosaic is; its +-24
               texture makes Intra4x4 macroblocks and P macroblocks with chroma AC there

run() is hard_content.oracle_run's record of a stream at a QP, with the oracle's Annex-B stream (its own SPS and PPS) and what
the oracle decoder makes of it.  The level guard (|level| <= 2063, the largest a 12-bit escape suffix carries; R3 of DESIGN.md)
is computed from the run, never tabulated: below it the reference's CAVLC writer is pinned, above it the oracle writes the low
12 bits of the suffix and the comparison pins the device against the oracle alone.
"""
import ctypes as C

import numpy as np

import hard_content as hc
from conftest import load_pkg
from nal_model import frame_nal

W, H = 64, 48
WINDOW = 16
STREAMS = ("mild", 20, 21, 22, "noisy")
SMOOTH = {"mild": (77, 4), "noisy": (80, 24)}   # (seed, noise amplitude) of synth.gen_frame
QPS = range(52)
NAL_TYPES = hc.NAL_TYPES
MAX_LEVEL = 2063
_frames, _runs = {}, {}


def frames(stream):
    """[4][W*H*3/2] uint8, read-only"""
    if stream not in _frames:
        f = np.stack([load_pkg().gen_frame(W, H, t, *SMOOTH[stream]) for t in range(4)]) if stream in SMOOTH else hc.sequence(W, H, stream)
        f.setflags(write=False)
        _frames[stream] = f
    return _frames[stream]


def parameter_sets(fo, qp):
    L = fo.lib()
    L.fo_write_sps.argtypes = L.fo_write_pps.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.fo_write_sps.restype = L.fo_write_pps.restype = C.c_size_t
    o = fo.Oracle(W, H, qp=qp, window=WINDOW, maxdiff=3, intra_every=1000)
    buf = np.empty(256, np.uint8)
    sps = bytes(buf[:L.fo_write_sps(o.c, buf.ctypes.data, buf.size)])
    pps = bytes(buf[:L.fo_write_pps(o.c, buf.ctypes.data, buf.size)])
    o.close()
    return frame_nal(7, np.frombuffer(sps, np.uint8)) + frame_nal(8, np.frombuffer(pps, np.uint8))


def run(fo, stream, qp):
    """-> dict: pics (hard_content.oracle_run's four dicts), stream (Annex-B), decoded ([4][fsz], the oracle decoder's
    pictures of that stream), max_level (over the four pictures).  Computed once and shared; callers leave it unchanged."""
    key = (stream, qp)
    if key not in _runs:
        pics = hc.oracle_run_frames(fo, W, H, frames(stream), qp, WINDOW) if stream in SMOOTH else hc.oracle_run(fo, W, H, stream, qp, WINDOW)
        annexb = parameter_sets(fo, qp) + b"".join(frame_nal(nt, np.frombuffer(p["rbsp"], np.uint8)) for nt, p in zip(NAL_TYPES, pics))
        n, dec, _ = fo.decode_stream_md5(annexb)
        assert n == len(pics), (stream, qp, n)
        _runs[key] = dict(pics=pics, stream=annexb, decoded=np.stack(dec), max_level=max(p["max_level"] for p in pics))
    return _runs[key]


def under_guard(fo, stream, qp):
    return run(fo, stream, qp)["max_level"] <= MAX_LEVEL


def luma_pictures(fo, stream, qp):
    """How many leading pictures of the stream a decoder must give back with the encoder's luma: all of them under the level
    guard, up to the first P picture whose last macroblock is P_Skip.  The reference decoder's more_rbsp_data heuristic
    (F/rbsp_IO.cpp:193) can stop in front of a skip run that ends the slice, so such a picture, and those predicted from it, are
    held by the md5 record of the reference decoder instead.  Above the guard: 0."""
    if not under_guard(fo, stream, qp):
        return 0
    k = 1
    for p in run(fo, stream, qp)["pics"][1:]:
        if p["mb_type"][-1] == 31:
            break
        k += 1
    return k


def y4m_md5(pictures):
    from slice_synth import y4m_md5 as f
    return f(pictures, W, H)
