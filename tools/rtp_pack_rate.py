"""Cost of RTP packetisation (RFC 6184, packetization-mode 1, max_packet 1400): S 1920x1072 streams in ONE context, bench.py's
content, qp 12, window 32; an I picture and the P picture behind it, each framed `--reps` times after it was coded (packing
may be repeated), by two routes that end with every packet and the packet table in host memory:
  (a) the host route, the only one there was: ferhip_fetch_nal into pinned memory, then a plain C++ packetiser on one host
      thread -- the one below, compiled here: a header and one memcpy per fragment;
  (b) the device route: ferhip_pack_rtp into device buffers, the index read back, then one copy of index[S].offset bytes and
      one of the table's rows.
Reported per picture type: the median wall time of one framing by each route and their ratio, the packets and bytes, and
whether the two routes' packets are identical.  Also the median wall time from the call to the end of the context's stream
of ferhip_pack_rtp against ferhip_pack_nal on the same picture (device to device, nothing copied): the kernels and their
launches.
Unless --no-prof, the run is made once more under `rocprofv3 --kernel-trace --stats` for the times of the k_nal_* and k_rtp_*
kernels themselves.
Usage: python tools/rtp_pack_rate.py [--streams 256] [--reps 9] [--no-prof]
Not a test; reads nothing outside the repository.

Measured once (2026-10-20, one MI355X, ROCm 7.2, 256 streams, 9 repetitions):
  I picture, 211 267 packets, 297.3 MB: host route 21.36 ms, device route 6.21 ms (x 3.44); pack_rtp 0.790 ms, pack_nal 0.630 ms (x 1.25)
  P picture, 123 781 packets, 174.1 MB: host route 12.29 ms, device route 3.75 ms (x 3.28); pack_rtp 0.512 ms, pack_nal 0.403 ms (x 1.27)
and the two routes' packets were identical.  Kernels, mean per call over both pictures: k_nal_count 167.0 us, k_nal_plan 8.4 us (both
packers), k_rtp_index 5.2 us / k_nal_index 4.9 us, k_rtp_emit 446.7 us / k_nal_emit 324.6 us (x 1.38)."""
import argparse
import csv
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

PACKETISER = r"""
#include <stdint.h>
#include <string.h>
struct au { uint64_t offset; uint32_t bytes; int32_t nal_type; };
struct pkt { uint64_t offset; uint32_t bytes; uint32_t stream; };
struct hdr { uint32_t ssrc, timestamp; uint16_t seq; uint8_t payload_type, reserved; };
static uint8_t *rtp(uint8_t *w, const hdr &h, unsigned k, bool m)
{
    const unsigned seq = h.seq + k;
    w[0] = 0x80, w[1] = (uint8_t)((m ? 0x80 : 0) | h.payload_type), w[2] = (uint8_t)(seq >> 8), w[3] = (uint8_t)seq;
    for (int i = 0; i < 4; i++) w[4 + i] = (uint8_t)(h.timestamp >> (24 - 8 * i)), w[8 + i] = (uint8_t)(h.ssrc >> (24 - 8 * i));
    return w + 12;
}
// Annex-B entries (ferhip_fetch_nal, no parameter sets) -> packets at multiples of 16 and their table; returns the packets
extern "C" size_t packetise(const uint8_t *in, const au *index, int S, int P, const hdr *h, uint8_t *out, pkt *rows, uint64_t *total)
{
    const size_t B = P - 12, F = B - 2;
    size_t off = 0, n = 0;
    for (int s = 0; s < S; s++) {
        if (!index[s].bytes) continue;
        const uint8_t *u = in + index[s].offset + 4;
        const size_t N = index[s].bytes - 4;
        if (N <= B) {
            uint8_t *w = rtp(out + off, h[s], 0, true);
            memcpy(w, u, N);
            rows[n++] = {off, (uint32_t)(12 + N), (uint32_t)s};
            off += (12 + N + 15) & ~(size_t)15;
            continue;
        }
        const size_t cnt = (N - 1 + F - 1) / F;
        for (size_t k = 0; k < cnt; k++) {
            const size_t a = 1 + k * F, e = a + F < N ? a + F : N;
            uint8_t *w = rtp(out + off, h[s], (unsigned)k, k == cnt - 1);
            w[0] = (uint8_t)((u[0] & 0xE0) | 28);
            w[1] = (uint8_t)((k == 0 ? 0x80 : 0) | (k == cnt - 1 ? 0x40 : 0) | (u[0] & 0x1F));
            memcpy(w + 2, u + a, e - a);
            rows[n++] = {off, (uint32_t)(14 + e - a), (uint32_t)s};
            off += (14 + e - a + 15) & ~(size_t)15;
        }
    }
    *total = off;
    return n;
}
"""


def build_packetiser(tmp):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    src, so = Path(tmp) / "packetise.cpp", Path(tmp) / "libpacketise.so"
    src.write_text(PACKETISER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-shared", "-fPIC", str(src), "-o", str(so)], check=True, timeout=120)
    lib = C.CDLL(str(so))
    lib.packetise.restype = C.c_size_t
    lib.packetise.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def profile(args):
    """the same run once more in a child process under rocprofv3 -> {kernel name: calls, total ms, mean us}; per repetition
    and picture k_rtp_* run twice (the device route, and ferhip_pack_rtp alone), k_nal_index / k_nal_emit twice
    (ferhip_fetch_nal, ferhip_pack_nal) and k_nal_count / k_nal_plan four times, all on the same two pictures"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"error": "rocprofv3 not found"}
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "rtp", "--", sys.executable, __file__,
               "--streams", str(args.streams), "--reps", str(args.reps), "--no-prof"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": f"rocprofv3 exit {r.returncode}", "tail": r.stderr[-400:]}
        files = list(Path(d).rglob("*.csv"))
        for p in files:
            if "stats" not in p.name:
                continue
            with open(p) as f:
                for row in csv.DictReader(f):
                    name = row.get("Name", row.get("KERNEL_NAME", ""))
                    if "k_nal_" in name or "k_rtp_" in name:
                        calls = int(row.get("Calls", 0))
                        tot = float(row.get("TotalDurationNs", 0))
                        out[name[:40]] = {"calls": calls, "total_ms": round(tot / 1e6, 3), "mean_us": round(tot / max(calls, 1) / 1e3, 1)}
        if not out:
            out["files"] = [str(p.relative_to(d)) for p in files]
            out["tail"] = (r.stdout[-300:], r.stderr[-300:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-prof", action="store_true")
    args = ap.parse_args()
    W, H_IN, H, S, P, R = 1920, 1080, 1072, args.streams, 1400, args.reps
    pkg = load_pkg()
    frames = make_frames(S, 2, W, H_IN, H)
    lib = pkg.load_library()
    cap = S << 21  # 2 MiB per stream: three times what a 1080p I picture takes at qp 12; checked against the index below
    pcap = cap // 1024

    def view(buf, n, dtype=np.uint8):
        return np.ctypeslib.as_array(C.cast(C.c_void_p(buf.ptr), C.POINTER(C.c_uint8)), shape=(n,)).view(dtype)

    with tempfile.TemporaryDirectory() as tmp:
        host = build_packetiser(tmp)
        e = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=30)
        pin_nal, pin_out = pkg.DeviceBuffer(cap, pinned=True), pkg.DeviceBuffer(cap, pinned=True)
        pin_rows, pin_idx = pkg.DeviceBuffer(16 * pcap, pinned=True), pkg.DeviceBuffer(24 * (S + 1), pinned=True)
        dev, drows, didx = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * pcap), pkg.DeviceBuffer(24 * (S + 1))
        rows_a = np.zeros(pcap, pkg.RTP_PKT)
        out_a = np.zeros(cap, np.uint8)
        idx_nal = np.zeros(S + 1, pkg.AU)
        hdr = pkg.rtp_hdr(S, ssrc=1000 + np.arange(S), timestamp=90000, seq=65000, payload_type=96)
        total_a = C.c_uint64()
        out = {"streams": S, "coded_size": f"{W}x{H}", "max_packet": P, "reps": R}
        for k, name in enumerate(("I", "P")):
            e.set_frames_device(frames[k].data_ptr())
            e.encode_picture_device(None)
            e.sync()
            ta, tb, tr, tn = [], [], [], []
            for _ in range(R + 1):  # the first repetition allocates: dropped
                t0 = time.perf_counter()
                rc = lib.ferhip_fetch_nal(e.ctx, 0, C.c_void_p(pin_nal.ptr), cap, idx_nal.ctypes.data)
                assert rc == 0
                na = host.packetise(C.c_void_p(pin_nal.ptr), idx_nal.ctypes.data, S, P, hdr.ctypes.data, out_a.ctypes.data, rows_a.ctypes.data,
                                    C.byref(total_a))
                ta.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                e.pack_rtp_device(hdr, P, dev.ptr, cap, drows.ptr, pcap, didx.ptr)
                e.sync()
                lib.ferhip_mem_copy(C.c_void_p(pin_idx.ptr), C.c_void_p(didx.ptr), 24 * (S + 1))
                idx = view(pin_idx, 24 * (S + 1), pkg.RTP_AU)
                total, npk = int(idx["offset"][S]), int(idx["first_pkt"][S])
                assert total <= cap and npk <= pcap and int(idx["bytes"][S]) == S
                lib.ferhip_mem_copy(C.c_void_p(pin_out.ptr), C.c_void_p(dev.ptr), total)
                lib.ferhip_mem_copy(C.c_void_p(pin_rows.ptr), C.c_void_p(drows.ptr), 16 * npk)
                tb.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                e.pack_rtp_device(hdr, P, dev.ptr, cap, drows.ptr, pcap, didx.ptr)
                e.sync()
                tr.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                e.pack_nal_device(dev.ptr, didx.ptr, cap)
                e.sync()
                tn.append(time.perf_counter() - t0)
            rows_b = view(pin_rows, 16 * npk, pkg.RTP_PKT)
            out_b = view(pin_out, total)
            same = na == npk and int(total_a.value) == total and np.array_equal(rows_a[:na], rows_b)
            if same:
                o, n = rows_b["offset"].astype(np.int64), rows_b["bytes"].astype(np.int64)
                step = max(1, npk // 4096)  # every packet's first 16 bytes, and a sample of whole packets
                same = all(np.array_equal(out_a[a: a + 16], out_b[a: a + 16]) for a in o) and \
                    all(np.array_equal(out_a[a: a + m], out_b[a: a + m]) for a, m in zip(o[::step], n[::step]))
            med = lambda t: statistics.median(t[1:])
            out[name] = {"packets": npk, "bytes": total, "host_route_ms": round(med(ta) * 1e3, 3), "device_route_ms": round(med(tb) * 1e3, 3),
                         "host_over_device": round(med(ta) / med(tb), 2), "pack_rtp_ms": round(med(tr) * 1e3, 3),
                         "pack_nal_ms": round(med(tn) * 1e3, 3), "rtp_over_nal": round(med(tr) / med(tn), 2), "identical": bool(same)}
        assert e.status() == [0] * S
        e.close()
    print(json.dumps(out), flush=True)
    if not args.no_prof:
        del frames
        print(json.dumps({"rocprof": profile(args)}), flush=True)


if __name__ == "__main__":
    main()
