"""Cost of the transport stream framing (ISO/IEC 13818-1; include/ferhip.h): S 1920x1072 streams in ONE context, bench.py's
content, qp 12, window 32; an I picture and the P picture behind it, each framed `--reps` times after it was coded (packing
may be repeated).
Way out, two routes that end with every 188-byte packet in host memory:
  (a) the host route, the only one there was: ferhip_fetch_nal (with the parameter sets) into pinned memory, then a plain
      C++ multiplexer of the same definition on one host thread -- the one below, compiled here;
  (b) the device route: ferhip_pack_ts into a device buffer, the index read back, then one copy of index[S].offset bytes.
Also ferhip_pack_ts against ferhip_pack_nal on the same picture, from the call to the end of the context's stream (device to
device, nothing copied): the kernels and their launches.
Way in, on the I picture's packets, every stream one run:
  (c) packets in host memory: ferhip_decs_decode_ts(base_on_device = 0), whose demultiplexer is split_ts on the host;
  (d) packets where ferhip_pack_ts left them: ferhip_decs_decode_ts(base_on_device = 1): k_unts_* and the device splitter.
Both decode the same pictures, so the difference of the two calls is the difference of the two ways in.
Every figure is wall time around the call and the wait for the context's stream -- the packers run on the context's own
stream, on which a caller cannot record events --, the first repetition dropped as warm-up: median, minimum and maximum.
Usage: python tools/ts_pack_rate.py [--streams 256] [--reps 9] [--no-decode]
Not a test; reads nothing outside the repository.

Measured once (2026-10-20, one MI355X, ROCm 7.2, 256 streams, 9 repetitions), medians:
  I picture, 1 590 621 packets, 299.0 MB: host route 33.01 ms, device route 6.10 ms (x 5.41); pack_ts 0.727 ms, pack_nal 0.636 ms (x 1.14)
  P picture,   931 593 packets, 175.1 MB: host route 18.86 ms, device route 3.64 ms (x 5.18); pack_ts 0.474 ms, pack_nal 0.410 ms (x 1.16)
  decode of the I picture's packets: from host memory 1229.1 ms, from device memory 1171.9 ms (the whole decode call)
and the two routes' packets were identical."""
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

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from conftest import load_pkg  # noqa: E402
from quality_rate import make_frames  # noqa: E402

MUXER = r"""
#include <stdint.h>
#include <string.h>
struct au { uint64_t offset; uint32_t bytes; int32_t nal_type; };
struct hdr { uint64_t pts, pcr; uint16_t pid, pmt_pid; uint8_t cc, psi_cc; uint16_t reserved; };
// Annex-B entries (ferhip_fetch_nal) -> every stream's packets at the next multiple of 16 (no PSI); returns the total
extern "C" uint64_t mux(const uint8_t *in, const au *index, int S, const hdr *h, uint8_t *out, uint8_t *pes)
{
    uint64_t off = 0;
    for (int s = 0; s < S; s++) {
        if (!index[s].bytes) continue;
        const bool idr = index[s].nal_type == 5;
        const uint64_t pts = h[s].pts, pcr = h[s].pcr;
        const uint8_t head[20] = {0, 0, 1, 0xE0, 0, 0, 0x84, 0x80, 5, (uint8_t)(0x21 | ((pts >> 29) & 0x0E)), (uint8_t)(pts >> 22),
                                  (uint8_t)(1 | ((pts >> 14) & 0xFE)), (uint8_t)(pts >> 7), (uint8_t)(1 | ((pts << 1) & 0xFE)),
                                  0, 0, 0, 1, 9, (uint8_t)(idr ? 0x10 : 0x30)};
        memcpy(pes, head, 20);
        memcpy(pes + 20, in + index[s].offset, index[s].bytes);
        const size_t L = 20 + (size_t)index[s].bytes;
        uint8_t *w = out + off;
        size_t x = 0;
        for (unsigned k = 0; x < L; k++, w += 188) {
            const size_t left = L - x, room = k ? 184 : 176, c = left < room ? left : room;
            w[0] = 0x47, w[1] = (uint8_t)((k ? 0 : 0x40) | h[s].pid >> 8), w[2] = (uint8_t)h[s].pid;
            w[3] = (uint8_t)(((k == 0 || c < 184) ? 0x30 : 0x10) | ((h[s].cc + k) & 15));
            if (k == 0) {
                w[4] = (uint8_t)(183 - c), w[5] = (uint8_t)(0x10 | (idr ? 0x40 : 0));
                w[6] = (uint8_t)(pcr >> 25), w[7] = (uint8_t)(pcr >> 17), w[8] = (uint8_t)(pcr >> 9), w[9] = (uint8_t)(pcr >> 1);
                w[10] = (uint8_t)(((pcr & 1) << 7) | 0x7E), w[11] = 0;
                memset(w + 12, 0xFF, 176 - c);
            } else if (c < 184) {
                w[4] = (uint8_t)(183 - c);
                if (c < 183) w[5] = 0, memset(w + 6, 0xFF, 182 - c);
            }
            memcpy(w + 188 - c, pes + x, c);
            x += c;
        }
        off += ((uint64_t)(w - (out + off)) + 15) & ~(uint64_t)15;
    }
    return off;
}
"""


def build_muxer(tmp):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    src, so = Path(tmp) / "mux.cpp", Path(tmp) / "libmux.so"
    src.write_text(MUXER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-shared", "-fPIC", str(src), "-o", str(so)], check=True, timeout=120)
    lib = C.CDLL(str(so))
    lib.mux.restype = C.c_uint64
    lib.mux.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 3
    return lib


def stats(t):
    t = [x * 1e3 for x in t[1:]]
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-decode", action="store_true")
    args = ap.parse_args()
    W, H_IN, H, S, R = 1920, 1080, 1072, args.streams, args.reps
    pkg = load_pkg()
    frames = make_frames(S, 2, W, H_IN, H)
    lib = pkg.load_library()
    cap = S << 21  # 2 MiB per stream: three times what a 1080p I picture takes at qp 12; checked against the index below
    flags = pkg.AU_PARAM_SETS

    def view(buf, n, dtype=np.uint8):
        return np.ctypeslib.as_array(C.cast(C.c_void_p(buf.ptr), C.POINTER(C.c_uint8)), shape=(n,)).view(dtype)

    with tempfile.TemporaryDirectory() as tmp:
        host = build_muxer(tmp)
        e = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=30)
        pin_nal, pin_out, pin_idx = pkg.DeviceBuffer(cap, pinned=True), pkg.DeviceBuffer(cap, pinned=True), pkg.DeviceBuffer(24 * (S + 1), pinned=True)
        dev, didx = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(24 * (S + 1))
        out_a, pes = np.zeros(cap, np.uint8), np.zeros(1 << 22, np.uint8)
        idx_nal = np.zeros(S + 1, pkg.AU)
        hdr = pkg.ts_hdr(S, pts=90000, pcr=89000, pid=0x100 + np.arange(S), pmt_pid=0x1000, cc=5)
        out = {"streams": S, "coded_size": f"{W}x{H}", "reps": R}
        for k, name in enumerate(("I", "P")):
            e.set_frames_device(frames[k].data_ptr())
            e.encode_picture_device(None)
            e.sync()
            ta, tb, tt, tn = [], [], [], []
            for _ in range(R + 1):  # the first repetition allocates: dropped
                t0 = time.perf_counter()
                assert lib.ferhip_fetch_nal(e.ctx, flags, C.c_void_p(pin_nal.ptr), cap, idx_nal.ctypes.data) == 0
                total_a = host.mux(C.c_void_p(pin_nal.ptr), idx_nal.ctypes.data, S, hdr.ctypes.data, out_a.ctypes.data, pes.ctypes.data)
                ta.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                e.pack_ts_device(hdr, dev.ptr, cap, didx.ptr, flags)
                e.sync()
                lib.ferhip_mem_copy(C.c_void_p(pin_idx.ptr), C.c_void_p(didx.ptr), 24 * (S + 1))
                idx = view(pin_idx, 24 * (S + 1), pkg.TS_AU)
                total = int(idx["offset"][S])
                assert total <= cap and int(idx["bytes"][S]) == S
                lib.ferhip_mem_copy(C.c_void_p(pin_out.ptr), C.c_void_p(dev.ptr), total)
                tb.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                e.pack_ts_device(hdr, dev.ptr, cap, didx.ptr, flags)
                e.sync()
                tt.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                e.pack_nal_device(dev.ptr, didx.ptr, cap, flags)
                e.sync()
                tn.append(time.perf_counter() - t0)
            out_b = view(pin_out, total)
            same = int(total_a) == total and all(
                np.array_equal(out_a[int(o): int(o) + int(n)], out_b[int(o): int(o) + int(n)]) for o, n in zip(idx["offset"][:S], idx["bytes"][:S]))
            a, b, t, n = stats(ta), stats(tb), stats(tt), stats(tn)
            out[name] = {"packets": int(idx["npkts"][S]), "bytes": total, "host_route": a, "device_route": b,
                         "host_over_device": round(a["median_ms"] / b["median_ms"], 2), "pack_ts": t, "pack_nal": n,
                         "ts_over_nal": round(t["median_ms"] / n["median_ms"], 2), "identical": bool(same)}
            if name == "I" and not args.no_decode:
                # the way in: the packets ferhip_pack_ts just left in `dev` (written again, since pack_nal used the buffer)
                e.pack_ts_device(hdr, dev.ptr, cap, didx.ptr, flags)
                e.sync()
                lib.ferhip_mem_copy(C.c_void_p(pin_out.ptr), C.c_void_p(dev.ptr), total)
                runs = np.array([(int(idx["offset"][s]), int(idx["bytes"][s]), s) for s in range(S)], pkg.TS_RUN)
                pids = np.ascontiguousarray(hdr["pid"], np.uint16)
                pics, st = (C.c_int * S)(), (C.c_int * S)()
                res = {}
                for route, base, on_dev in (("host_packets", pin_out.ptr, 0), ("device_packets", dev.ptr, 1)):
                    d = pkg.LiveDecoder(S, W, H, 1)
                    picture = pkg.DeviceBuffer(S * d.fsz)
                    td = []
                    for _ in range(R + 1):
                        for s in range(S):
                            d.reset_stream(s)
                        t0 = time.perf_counter()
                        rc = lib.ferhip_decs_decode_ts(d.h, C.c_void_p(base), on_dev, runs.ctypes.data, S, pids.ctypes.data, C.c_void_p(picture.ptr), 1,
                                                       pics, st)
                        td.append(time.perf_counter() - t0)
                        assert rc == 0 and list(pics) == [1] * S and list(st) == [0] * S
                    res[route] = stats(td)
                    d.close()
                    picture.free()
                res["host_over_device"] = round(res["host_packets"]["median_ms"] / res["device_packets"]["median_ms"], 2)
                out["decode_I"] = res
        assert e.status() == [0] * S
        e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
