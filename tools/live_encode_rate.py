"""Live encoder rate: S 1920x1072 streams in ONE context, bench.py's content (generated at 1920x1080, cropped to 1072 rows),
window 32, IntraEvery 30, the device path (pictures in device memory, ferhip_encode_picture_dev, AUTO picture types), at
four presence patterns.  The figure is macroblocks/s OF PICTURES ACTUALLY CODED:
  (a) every stream present, through the lockstep call (ferhip_set_frames + NULL types: what bench.py runs);
  (b) every stream present, through the live calls (ferhip_set_frames_live with a full mask, explicit AUTO types);
  (c) every stream absent on every other call, in two phases of S / 2 (even calls: the first half, odd calls: the second);
  (d) one seeded random quarter of the streams absent per call.
In call k every present stream is given picture k % 30 of its content (a feed that drops pictures drops them from its
content too).  One warm-up pass and one timed pass of 30 calls (a, b), 60 calls (c: 30 pictures per stream) or 40 calls (d).
Unless --no-prof, (c) runs once more under `rocprofv3 --kernel-trace --stats` for the time of k_carry_ref and of the
masked k_repack.
Usage: python tools/live_encode_rate.py [--streams 256] [--configs abcd] [--no-prof]"""
import argparse
import csv
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
    """(c) once more in a child process under rocprofv3 -> {kernel name: calls, total ms, mean us} of the rows that matter"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"error": "rocprofv3 not found"}
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "live", "--", sys.executable, __file__,
               "--streams", str(args.streams), "--configs", "c", "--no-prof"]
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
                    if any(k in name for k in ("k_carry_ref", "k_repack", "k_frame_sad", "k_rc_plan", "k_me_resolve", "k_me_pre",
                                               "k_me_spec", "k_p_resid", "k_intra_mb")):
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
    ap.add_argument("--configs", default="abcd")
    ap.add_argument("--no-prof", action="store_true")
    args = ap.parse_args()
    W, H_IN, H, GOP, S = 1920, 1080, 1072, 30, args.streams
    pkg = load_pkg()
    NONE, AUTO = pkg.NAL_NONE, pkg.NAL_AUTO
    frames = make_frames(S, GOP, W, H_IN, H)
    nmb = (W // 16) * (H // 16)
    rng = np.random.default_rng(1234)

    def masks(cfg):
        if cfg in "ab":
            return [np.ones(S, np.uint8)] * GOP
        if cfg == "c":
            half = (np.arange(S) < S // 2).astype(np.uint8)
            return [half if k % 2 == 0 else 1 - half for k in range(2 * GOP)]
        out = []
        for _ in range(GOP * 4 // 3):
            m = np.ones(S, np.uint8)
            m[rng.permutation(S)[: S // 4]] = 0
            out.append(m)
        return out

    def run(cfg):
        e = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=GOP)
        plan = masks(cfg)
        types = [[AUTO if m[s] else NONE for s in range(S)] for m in plan]
        coded = int(sum(int(m.sum()) for m in plan))
        for _ in range(2):  # warm-up pass, timed pass
            e.sync()
            t0 = time.perf_counter()
            for k, m in enumerate(plan):
                ptr = frames[k % GOP].data_ptr()
                if cfg == "a":
                    e.set_frames_device(ptr)
                    e.encode_picture_device(None)
                else:
                    e.set_frames_live(ptr, m)
                    e.encode_picture_device(types[k])
            e.sync()
            dt = time.perf_counter() - t0
        assert e.status() == [0] * S
        e.close()
        return {"calls": len(plan), "pictures_coded": coded, "seconds": round(dt, 4), "mbps": coded * nmb / dt}

    out = {"streams": S, "coded_size": f"{W}x{H}", "intra_every": GOP}
    for cfg in "abcd":
        if cfg in args.configs:
            out[cfg] = run(cfg)
    print(json.dumps(out), flush=True)
    if not args.no_prof and "c" in args.configs:
        del frames
        print(json.dumps({"rocprof_c": profile(args)}), flush=True)


if __name__ == "__main__":
    os.environ.setdefault("PYTHONUNBUFFERED", "1")
    main()
