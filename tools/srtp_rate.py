"""Cost of SRTP (RFC 3711: AES-128 counter mode, HMAC-SHA1-80) on the RTP packets of a picture: S 1920x1072 streams in ONE
context, bench.py's content, qp 12, window 32, max_packet 1400; an I picture and the P picture behind it, each protected
`--reps` times after it was coded, by two routes that end with every SRTP packet and the packet table in host memory:
  (a) the host route: ferhip_fetch_rtp into pinned memory (measured), then a host protect.  The host protect is the plain
      C++ of tools/srtp_host_check.cpp, built -O2 here and run on ONE core over 1400-byte packets (`srtp_host_check rate`);
      its time is scaled to the picture's bytes and divided by the 16 cores a sender may have: that scaling is arithmetic,
      not a run, and table-driven C++ is not what a host with AES and SHA instructions and an optimised library reaches.
  (b) the device route: ferhip_pack_rtp, the index read back (the caller needs npkts and advances seq by it anyway),
      ferhip_srtp_protect_dev on the table where it lies, then one copy of the packets and one of the table's rows.
Also, device to device with nothing copied: ferhip_srtp_protect_dev from the call to the end of the context's stream, and
ferhip_srtp_unprotect of the same packets from device memory and from pinned host memory (one staging copy), each with its
one synchronisation.  The decoder handed to ferhip_srtp_unprotect only lends its stream: a small one is made for that.
Reported per picture type: medians over the repetitions (the first, which allocates, is dropped), packets and bytes, and
whether unprotect gave back the packets ferhip_pack_rtp wrote, every status 0.
Unless --no-prof, the run is made once more under `rocprofv3 --kernel-trace --stats` for the times of the k_srtp_* kernels.
Usage: python tools/srtp_rate.py [--streams 256] [--reps 9] [--no-prof]
Not a test; reads nothing outside the repository.  The figures measured with it stand in DESIGN.md."""
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

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(ROOT / "tests"))
from conftest import load_pkg  # noqa: E402
from quality_rate import make_frames  # noqa: E402


def host_protect_rate(tmp, npackets=20000, nbytes=1400):
    """seconds per byte of the stand-alone host protect on one core"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    exe = Path(tmp) / "srtp_host_check"
    subprocess.run([cxx, "-std=c++17", "-O2", str(ROOT / "tools" / "srtp_host_check.cpp"), "-o", str(exe)], check=True, timeout=180)
    t = []
    for _ in range(3):
        r = subprocess.run([str(exe), "rate", str(npackets), str(nbytes)], capture_output=True, text=True, timeout=300, check=True)
        t.append(float(r.stdout.split()[0]))
    return statistics.median(t) / (npackets * nbytes)


def profile(args):
    """the same run once more in a child process under rocprofv3 -> {kernel name: calls, total ms, mean us}"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"error": "rocprofv3 not found"}
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "srtp", "--", sys.executable, __file__,
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
                    if "k_srtp_" in name or "k_rtp_" in name:
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
    cap = S << 21  # 2 MiB per stream: three times what a 1080p I picture takes at qp 12; checked against the tables below
    pcap = cap // 1024

    def view(buf, n, dtype=np.uint8):
        return np.ctypeslib.as_array(C.cast(C.c_void_p(buf.ptr), C.POINTER(C.c_uint8)), shape=(n,)).view(dtype)

    def copy(dst, src, n):
        rc = lib.ferhip_mem_copy(C.c_void_p(dst), C.c_void_p(src), n)
        assert rc == 0

    med = lambda t: statistics.median(t[1:])  # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        per_byte = host_protect_rate(tmp)
        e = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=30)
        dec = pkg.LiveDecoder(1, 176, 144, 1)
        tx, rx = pkg.Srtp(S), pkg.Srtp(S)
        for s in range(S):
            key, salt = bytes((s + 3 * k) & 255 for k in range(16)), bytes((s + 5 * k) & 255 for k in range(14))
            tx.set_key(s, key, salt)
            rx.set_key(s, key, salt)
        pin_out, pin_rows = pkg.DeviceBuffer(cap, pinned=True), pkg.DeviceBuffer(16 * (pcap + 1), pinned=True)
        pin_idx, pin_rtp = pkg.DeviceBuffer(24 * (S + 1), pinned=True), pkg.DeviceBuffer(cap, pinned=True)
        dev, drows, didx = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * pcap), pkg.DeviceBuffer(24 * (S + 1))
        sdev, srows, plain = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * (pcap + 1)), pkg.DeviceBuffer(cap)
        rows_a, idx_a = np.zeros(pcap, pkg.RTP_PKT), np.zeros(S + 1, pkg.RTP_AU)
        hdr = pkg.rtp_hdr(S, ssrc=1000 + np.arange(S), timestamp=90000, seq=65000, payload_type=96)
        out = {"streams": S, "coded_size": f"{W}x{H}", "max_packet": P, "reps": R, "host_protect_MBps_one_core": round(1e-6 / per_byte, 1)}
        for k, name in enumerate(("I", "P")):
            e.set_frames_device(frames[k].data_ptr())
            e.encode_picture_device(None)
            e.sync()
            tf, tb, tp, tud, tuh = [], [], [], [], []
            for _ in range(R + 1):  # the first repetition allocates: dropped.  The same packets every time: a replay is authentic
                t0 = time.perf_counter()
                rc = lib.ferhip_fetch_rtp(e.ctx, 0, P, hdr.ctypes.data, C.c_void_p(pin_rtp.ptr), cap, rows_a.ctypes.data, pcap, idx_a.ctypes.data)
                assert rc == 0
                tf.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                e.pack_rtp_device(hdr, P, dev.ptr, cap, drows.ptr, pcap, didx.ptr)
                e.sync()
                copy(pin_idx.ptr, didx.ptr, 24 * (S + 1))
                idx = view(pin_idx, 24 * (S + 1), pkg.RTP_AU)
                total, npk = int(idx["offset"][S]), int(idx["first_pkt"][S])
                assert total <= cap and npk <= pcap and int(idx["bytes"][S]) == S
                tx.protect(e, dev.ptr, drows.ptr, npk, sdev.ptr, cap, srows.ptr)
                e.sync()
                copy(pin_rows.ptr, srows.ptr, 16 * (npk + 1))
                stab = view(pin_rows, 16 * (npk + 1), pkg.RTP_PKT)
                stotal = int(stab["offset"][npk])
                assert stotal <= cap and int(stab["bytes"][npk]) == npk
                copy(pin_out.ptr, sdev.ptr, stotal)
                tb.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                tx.protect(e, dev.ptr, drows.ptr, npk, sdev.ptr, cap, srows.ptr)
                e.sync()
                tp.append(time.perf_counter() - t0)
                rows_s = stab[:npk].copy()
                t0 = time.perf_counter()
                table, status = rx.unprotect(dec, sdev.ptr, rows_s, plain.ptr, cap, base_on_device=True)
                tud.append(time.perf_counter() - t0)
                ok = not status.any() and int(table["bytes"][npk]) == npk
                t0 = time.perf_counter()
                table_h, status_h = rx.unprotect(dec, view(pin_out, stotal), rows_s, plain.ptr, cap)
                tuh.append(time.perf_counter() - t0)
                ok = ok and not status_h.any() and np.array_equal(table, table_h)
            # unprotect gave back what ferhip_pack_rtp wrote: the tables agree, and a sample of whole packets
            copy(pin_out.ptr, plain.ptr, int(table["offset"][npk]))
            copy(pin_rtp.ptr, dev.ptr, total)
            copy(pin_rows.ptr, drows.ptr, 16 * npk)
            a, b, rows_p = view(pin_out, int(table["offset"][npk])), view(pin_rtp, total), view(pin_rows, 16 * npk, pkg.RTP_PKT)
            ok = ok and np.array_equal(table["bytes"][:npk], rows_p["bytes"])
            step = max(1, npk // 4096)
            ok = ok and all(np.array_equal(a[int(r["offset"]):][: int(r["bytes"])], b[int(q["offset"]):][: int(q["bytes"])])
                            for r, q in zip(table[:npk:step], rows_p[::step]))
            host_protect = per_byte * float(rows_p["bytes"].sum())
            route_a = med(tf) + host_protect / 16
            out[name] = {"packets": npk, "rtp_bytes": int(rows_p["bytes"].sum()), "srtp_buffer_bytes": stotal,
                         "fetch_rtp_ms": round(med(tf) * 1e3, 3), "host_protect_one_core_ms": round(host_protect * 1e3, 3),
                         "host_route_16_cores_ms": round(route_a * 1e3, 3), "device_route_ms": round(med(tb) * 1e3, 3),
                         "host_over_device": round(route_a / med(tb), 2), "protect_ms": round(med(tp) * 1e3, 3),
                         "unprotect_from_device_ms": round(med(tud) * 1e3, 3), "unprotect_from_host_ms": round(med(tuh) * 1e3, 3),
                         "round_trip_identical": bool(ok)}
        assert e.status() == [0] * S
        for x in (tx, rx, dec, e):
            x.close()
    print(json.dumps(out), flush=True)
    if not args.no_prof:
        del frames
        print(json.dumps({"rocprof": profile(args)}), flush=True)


if __name__ == "__main__":
    main()
