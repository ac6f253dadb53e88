"""Cost of NAL framing: S 1920x1072 streams in ONE context, bench.py's content (generated at 1920x1080, cropped to 1072
rows), window 32, IntraEvery 30, pictures in device memory, ferhip_encode_picture_dev with AUTO picture types; one warm-up
GOP and one timed GOP, every picture leaving as Annex-B NAL units in host memory, by two paths:
  (a) the host path: ferhip_copy_rbsp of every stream at the longest stream's length (read back first, rounded up to 4 KiB)
      into pinned host memory, then ferhip_write_nal per stream on one host thread;
  (b) the device path: ferhip_pack_nal into a device buffer, its index read back, one device-to-host copy of `total` bytes.
Reported per path: macroblocks/s, bytes over PCIe per picture (all streams) and the host CPU seconds spent framing; the two
paths' bytes are compared stream by stream on the last picture.
Unless --no-prof, (b) runs once more under `rocprofv3 --kernel-trace --stats` for the times of the four k_nal_* kernels.
Usage: python tools/nal_pack_rate.py [--streams 256] [--configs ab] [--no-prof]"""
import argparse
import csv
import ctypes as C
import json
import os
import shutil
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


def profile(args):
    """(b) once more in a child process under rocprofv3 -> {kernel name: calls, total ms, mean us}"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"error": "rocprofv3 not found"}
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "nal", "--", sys.executable, __file__,
               "--streams", str(args.streams), "--configs", "b", "--no-prof"]
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
                    if any(k in name for k in ("k_nal_", "k_cavlc", "k_me_resolve", "k_me_pre", "k_intra_mb")):
                        calls = int(row.get("Calls", 0))
                        tot = float(row.get("TotalDurationNs", 0))
                        out[name[:60]] = {"calls": calls, "total_ms": round(tot / 1e6, 3),
                                          "mean_us": round(tot / max(calls, 1) / 1e3, 1)}
        if not out:
            out["files"] = [str(p.relative_to(d)) for p in files]
            out["tail"] = (r.stdout[-300:], r.stderr[-300:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--configs", default="ab")
    ap.add_argument("--no-prof", action="store_true")
    args = ap.parse_args()
    W, H_IN, H, GOP, S = 1920, 1080, 1072, 30, args.streams
    pkg = load_pkg()
    frames = make_frames(S, GOP, W, H_IN, H)
    lib = pkg.load_library()  # after torch has initialised the GPU, as in the other tools (the first FerHip loads it there)
    nmb = (W // 16) * (H // 16)
    stride = nmb * 1024 + 4096

    def view(buf, n):
        return np.ctypeslib.as_array(C.cast(C.c_void_p(buf.ptr), C.POINTER(C.c_uint8)), shape=(n,))

    def run(cfg):
        e = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=GOP)
        pin = pkg.DeviceBuffer(S * stride, pinned=True)       # (a) RBSP rows / (b) the packed units
        pin_small = pkg.DeviceBuffer(16 * (S + 1), pinned=True)  # (a) lengths / (b) the index
        host, small = view(pin, S * stride), view(pin_small, 16 * (S + 1))
        if cfg == "b":
            dev = pkg.DeviceBuffer(S * stride)
            dindex = pkg.DeviceBuffer(16 * (S + 1))
        nal = np.empty(stride * 3 // 2 + 16, np.uint8)
        last = None
        for _ in range(2):  # warm-up GOP, timed GOP
            pcie = 0
            cpu = 0.0
            e.sync()
            t0 = time.perf_counter()
            for k in range(GOP):
                e.set_frames_device(frames[k].data_ptr())
                _, _, plen, nt = e.encode_picture_device(None)
                if cfg == "a":
                    e.sync()  # the lengths decide how much of every row crosses the bus
                    lib.ferhip_mem_copy(C.c_void_p(pin_small.ptr), C.c_void_p(plen), 4 * S)
                    lens = small[: 4 * S].view(np.uint32)
                    width = min((int(lens.max()) + 4095) & ~4095, stride)
                    rc = lib.ferhip_copy_rbsp(e.ctx, C.c_void_p(pin.ptr), stride, width, C.c_void_p(pin_small.ptr), 1)
                    assert rc == 0
                    e.sync()
                    pcie += width * S + 8 * S
                    c0 = time.process_time()
                    units = []
                    for s in range(S):
                        m = lib.ferhip_write_nal(1, nt[s], C.c_void_p(pin.ptr + s * stride), int(lens[s]), nal.ctypes.data)
                        units.append(nal[:m].tobytes() if k == GOP - 1 else m)
                    cpu += time.process_time() - c0
                else:
                    e.pack_nal_device(dev.ptr, dindex.ptr, S * stride)
                    e.sync()
                    lib.ferhip_mem_copy(C.c_void_p(pin_small.ptr), C.c_void_p(dindex.ptr), 16 * (S + 1))
                    idx = small.view(pkg.AU)
                    total = int(idx["offset"][S])
                    assert total <= S * stride and int(idx["bytes"][S]) == S
                    lib.ferhip_mem_copy(C.c_void_p(pin.ptr), C.c_void_p(dev.ptr), total)
                    pcie += total + 16 * (S + 1)
                    if k == GOP - 1:
                        units = [host[int(a["offset"]): int(a["offset"]) + int(a["bytes"])].tobytes() for a in idx[:S]]
            e.sync()
            dt = time.perf_counter() - t0
            last = units
        assert e.status() == [0] * S
        e.close()
        return last, {"seconds": round(dt, 4), "mbps": S * GOP * nmb / dt, "pcie_bytes_per_picture": pcie // GOP,
                      "host_framing_cpu_seconds": round(cpu, 4)}

    out = {"streams": S, "coded_size": f"{W}x{H}", "intra_every": GOP}
    units = {}
    for cfg in "ab":
        if cfg in args.configs:
            units[cfg], out[cfg] = run(cfg)
    if len(units) == 2:
        out["last_picture_identical"] = units["a"] == units["b"]
    print(json.dumps(out), flush=True)
    if not args.no_prof and "b" in args.configs:
        del frames
        print(json.dumps({"rocprof_b": profile(args)}), flush=True)


if __name__ == "__main__":
    os.environ.setdefault("PYTHONUNBUFFERED", "1")
    main()
