"""Cost of the fragmented MP4 framing (include/ferhip.h): S 1920x1072 streams in ONE context, bench.py's content, qp 12,
window 32; a GOP of `--gop` pictures (an I picture, then P pictures), one media segment per stream and GOP.
Way out, two routes that end with every stream's moof + mdat in host memory:
  (a) per picture, the only way there was: ferhip_fetch_nal(FERHIP_AU_AVCC | FERHIP_AU_PARAM_SETS) into pinned memory -- a
      wait and a read of the index for every picture -- then a plain C++ muxer of the same definition on one host thread
      that appends the samples to every stream's segment and writes the boxes at the end -- the one below, compiled here;
  (b) per segment: ferhip_mp4_append behind every picture (asynchronous; timed with the wait for the context's stream, which a
      caller would not make, and without it), then one ferhip_mp4_fetch per GOP.
Every figure is wall time; the GOP is coded `--reps` + 1 times and the first is dropped as warm-up: medians.
Usage: python tools/mp4_pack_rate.py [--streams 256] [--gop 30] [--reps 3]
Not a test; reads nothing outside the repository.  The measured values stand in DESIGN.md section 6."""
import argparse
import ctypes as C
import json
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(ROOT / "tests"))
from conftest import load_pkg  # noqa: E402
from quality_rate import make_frames  # noqa: E402

MUXER = r"""
#include "fer_mp4_host.h"
struct au { uint64_t offset; uint32_t bytes; int32_t nal_type; };
struct seg { uint64_t offset; uint32_t bytes, nsamples; int32_t first; uint32_t fault; };
static void put32(uint8_t *p, uint32_t x) { p[0] = (uint8_t)(x >> 24), p[1] = (uint8_t)(x >> 16), p[2] = (uint8_t)(x >> 8), p[3] = (uint8_t)x; }
// one picture's length-prefixed entries (ferhip_fetch_nal) -> sample n of every stream's region, and its trun entry
extern "C" void mp4_add(const uint8_t *in, const au *index, int S, uint32_t K, uint32_t duration, uint8_t *out, size_t stride, seg *st)
{
    const uint32_t D = fer_mp4_data_offset(K);
    for (int s = 0; s < S; s++) {
        if (!index[s].bytes) continue;
        uint8_t *r = out + (size_t)s * stride;
        memcpy(r + D + st[s].bytes, in + index[s].offset, index[s].bytes);
        uint8_t *t = r + 88 + 12 * st[s].nsamples;
        put32(t, duration), put32(t + 4, index[s].bytes), put32(t + 8, fer_mp4_sample_flags(index[s].nal_type == 5));
        st[s].bytes += index[s].bytes;
        st[s].nsamples++;
    }
}
// the boxes in front of every stream's samples, then the segments back to back in `packed`; returns the total
extern "C" uint64_t mp4_end(int S, uint32_t K, uint64_t decode_time, uint32_t sequence, uint8_t *out, size_t stride, seg *st, uint8_t *packed)
{
    const uint32_t D = fer_mp4_data_offset(K);
    uint64_t total = 0;
    for (int s = 0; s < S; s++) {
        if (!st[s].nsamples) continue;
        uint8_t *r = out + (size_t)s * stride;
        for (uint32_t w = 0; w < D / 4; w++) {
            bool keep;
            const uint32_t x = fer_mp4_front_word(w, st[s].nsamples, D, st[s].bytes, decode_time, sequence, &keep);
            if (!keep) put32(r + 4 * w, x);
        }
        memcpy(packed + total, r, D + st[s].bytes);
        total += D + st[s].bytes;
    }
    return total;
}
"""


def build_muxer(tmp):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    src, so = Path(tmp) / "mux.cpp", Path(tmp) / "libmux.so"
    src.write_text(MUXER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-shared", "-fPIC", "-I", str(ROOT / "h264-fer_amd" / "csrc"), str(src), "-o", str(so)], check=True,
                   timeout=120)
    lib = C.CDLL(str(so))
    lib.mp4_add.restype = None
    lib.mp4_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mp4_end.restype = C.c_uint64
    lib.mp4_end.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return lib


def med(t):
    return round(statistics.median(t) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--gop", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mib-per-picture", type=float, default=1.0, help="room per stream and picture; checked against the index")
    args = ap.parse_args()
    W, H_IN, H, S, R, K = 1920, 1080, 1072, args.streams, args.reps, args.gop
    pkg = load_pkg()
    frames = make_frames(S, 2, W, H_IN, H)
    lib = pkg.load_library()
    stride = (int(args.mib_per_picture * (1 << 20)) * K + pkg.mp4_data_offset(K) + 15) & ~15
    cap_nal = S << 21
    flags = pkg.AU_PARAM_SETS
    assert stride < 1 << 31

    def view(buf, n, dtype=np.uint8):
        return np.ctypeslib.as_array(C.cast(C.c_void_p(buf.ptr), C.POINTER(C.c_uint8)), shape=(n,)).view(dtype)

    with tempfile.TemporaryDirectory() as tmp:
        host = build_muxer(tmp)
        e = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=K)
        pin_nal = pkg.DeviceBuffer(cap_nal, pinned=True)
        dev, didx = pkg.DeviceBuffer(S * stride), pkg.DeviceBuffer(24 * (S + 1))
        regions_a, packed_a, packed_b = np.zeros(S * stride, np.uint8), np.zeros(S * stride, np.uint8), np.zeros(S * stride, np.uint8)
        idx_nal, idx_b = np.zeros(S + 1, pkg.AU), np.zeros(S + 1, pkg.MP4_SEG)
        t_host, t_dev, t_dev_async, t_fetch, t_end = [], [], [], [], []
        for rep in range(R + 1):
            st = np.zeros(S, pkg.MP4_SEG)
            hdr = pkg.mp4_hdr(S, decode_time=3000 * K * rep, sequence=1 + rep, duration=3000)
            e.mp4_open(hdr, K, dev.ptr, stride, flags)
            th = td = ta = 0.0
            for k in range(K):
                e.set_frames_device(frames[k & 1].data_ptr())
                e.encode_picture_device([pkg.NAL_IDR if k == 0 else pkg.NAL_SLICE] * S)
                e.sync()
                t0 = time.perf_counter()
                assert lib.ferhip_fetch_nal(e.ctx, flags | pkg.AU_AVCC, C.c_void_p(pin_nal.ptr), cap_nal, idx_nal.ctypes.data) == 0
                host.mp4_add(C.c_void_p(pin_nal.ptr), idx_nal.ctypes.data, S, K, 3000, regions_a.ctypes.data, stride, st.ctypes.data)
                th += time.perf_counter() - t0
                t0 = time.perf_counter()
                e.mp4_append()
                ta += time.perf_counter() - t0
                e.sync()
                td += time.perf_counter() - t0
            t0 = time.perf_counter()
            total_a = host.mp4_end(S, K, 3000 * K * rep, 1 + rep, regions_a.ctypes.data, stride, st.ctypes.data, packed_a.ctypes.data)
            t_end.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            assert lib.ferhip_mp4_fetch(e.ctx, packed_b.ctypes.data, packed_b.size, idx_b.ctypes.data) == 0
            t_fetch.append(time.perf_counter() - t0)
            t_host.append(th)
            t_dev.append(td)
            t_dev_async.append(ta)
            assert int(idx_b[S]["fault"]) == 0 and int(idx_b[S]["nsamples"]) == S * K, "a region was too small: raise --mib-per-picture"
        total_b = int(idx_b["bytes"][:S].astype(np.int64).sum())
        same = int(total_a) == total_b and np.array_equal(packed_a[:total_b], packed_b[:total_b])
        a = med([x + y for x, y in zip(t_host[1:], t_end[1:])])
        b = med([x + y for x, y in zip(t_dev[1:], t_fetch[1:])])
        out = {"streams": S, "coded_size": f"{W}x{H}", "gop": K, "reps": R, "segment_bytes": total_b, "identical": bool(same),
               "per_picture_route_ms": a, "fetch_nal_and_mux_ms": med(t_host[1:]), "host_boxes_and_pack_ms": med(t_end[1:]),
               "segment_route_ms": b, "appends_with_wait_ms": med(t_dev[1:]), "appends_enqueue_only_ms": med(t_dev_async[1:]),
               "mp4_fetch_ms": med(t_fetch[1:]), "per_picture_over_segment": round(a / b, 2)}
        assert e.status() == [0] * S
        e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
