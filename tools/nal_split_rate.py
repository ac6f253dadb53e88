"""Cost of splitting Annex-B input: S 1920x1072 streams of the library's own encoder (bench.py's content, QP 12, window 32,
one I picture and T - 1 P pictures each, SPS + PPS in front of the I picture) decoded by one live decoder, one picture of
every stream per call, device output, by two paths in one process:
  (a) ferhip_decs_decode on the chunks in host memory: the host splitter, then the slices gathered into pinned memory and
      copied to the device;
  (b) ferhip_decs_decode_dev on the same bytes resident in device memory: the device splitter, nothing staged.
Each path decodes the sequence twice on its own decoder (reset in between), the second pass is timed.  Reported per path:
seconds per call, and from ferhip_decs_timing the seconds in the host splitter and in pack + H2D (a) and in the device
splitter's launches, by HIP events (b), with the splitter's bytes per second; the pictures of the two paths are compared.
Every stream count runs in a process of its own under `timeout`; the first one that fails ends the run.
Usage: python tools/nal_split_rate.py [--streams 8,64,128] [--pictures 4] [--limit 420]"""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))


def child(S, T):
    from conftest import load_pkg
    from quality_rate import make_frames
    W, H_IN, H = 1920, 1080, 1072
    pkg = load_pkg()
    frames = make_frames(S, T, W, H_IN, H)
    e = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=30)
    chunks = []
    for k in range(T):
        e.set_frames_device(frames[k].data_ptr())
        e.encode_picture_device([5 if k == 0 else 1] * S)
        units, _ = e.fetch_nal(pkg.AU_PARAM_SETS)
        chunks.append(units)
    assert e.status() == [0] * S
    e.close()
    del frames
    fsz = W * H * 3 // 2
    out = pkg.DeviceBuffer(S * fsz)
    # (b)'s input: every picture's chunks in one device buffer, each chunk at the next multiple of 16 plus one
    offs, total = [], 0
    for k in range(T):
        row = []
        for s in range(S):
            row.append(total + 1)
            total += (len(chunks[k][s]) + 1 + 15) & ~15
        offs.append(row)
    src = pkg.DeviceBuffer(total + 16)
    for k in range(T):
        for s in range(S):
            src.upload(np.frombuffer(chunks[k][s], np.uint8), offs[k][s])
    nbytes = sum(len(c) for row in chunks for c in row)
    res = {"streams": S, "pictures": T, "coded_size": f"{W}x{H}", "annexb_bytes_per_call": nbytes // T}
    sums = {}
    for path in "ab":
        dec = pkg.LiveDecoder(S, W, H, 1)
        for rep in range(2):
            for s in range(S):
                dec.reset_stream(s)
            dec.timing(reset=True)
            t0 = time.perf_counter()
            for k in range(T):
                if path == "a":
                    _, pics, st = dec.decode(chunks[k], out)
                else:
                    _, pics, st = dec.decode_dev([src.ptr + o for o in offs[k]], [len(c) for c in chunks[k]], out)
                assert pics == [1] * S and st == [0] * S, (path, k, pics, st)
            dt = time.perf_counter() - t0
        t = dec.timing()
        sums[path] = int(out.download().astype(np.uint64).sum())  # the last picture of every stream
        r = {"seconds_per_call": round(dt / T, 5), "parse_s_per_call": round(t["parse"] / T, 5), "recon_s_per_call": round(t["recon"] / T, 5)}
        if path == "a":
            r["host_split_s_per_call"] = round(t["host_split"] / T, 6)
            r["pack_h2d_s_per_call"] = round(t["pack_h2d"] / T, 6)
            r["split_pack_h2d_s_per_call"] = round((t["host_split"] + t["pack_h2d"]) / T, 6)
        else:
            r["dev_split_s_per_call"] = round(t["dev_split"] / T, 6)
            r["header_prep_s_per_call"] = round(t["pack_h2d"] / T, 6)  # slice headers and their copies: what is left of (a)'s pack
            r["dev_split_bytes_per_s"] = round(t["dev_split_bytes"] / max(t["dev_split"], 1e-12))
        res[path] = r
        dec.close()
    res["last_pictures_identical"] = sums["a"] == sums["b"]
    res["dev_split_faster_than_host_split_pack_h2d"] = res["b"]["dev_split_s_per_call"] < res["a"]["split_pack_h2d_s_per_call"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="8,64,128")
    ap.add_argument("--pictures", type=int, default=4)
    ap.add_argument("--limit", type=int, default=420, help="seconds a stream count may take")
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.pictures)
        return
    for S in [int(x) for x in a.streams.split(",")]:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, __file__, "--child", str(S), "--pictures", str(a.pictures)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"streams": S, "error": f"exit {rc}"}), flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    os.environ.setdefault("PYTHONUNBUFFERED", "1")
    main()
