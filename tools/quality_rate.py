"""Encoder rate with quality measurement and the QUALITY rate mode: S 1920x1072 streams in ONE context, bench.py's content
(gen_frames_torch, generated at 1920x1080 and cropped to 1072 rows), window 32, GOP 30, the device path
(ferhip_encode_picture_dev, AUTO picture types) that bench.py times, three configurations:
  (a) measurement off (what bench.py runs);
  (b) FERHIP_QM_SSE | FERHIP_QM_SSIM on every picture, the ring read once per GOP;
  (c) FERHIP_RC_QUALITY on every stream: target = the mean luma SSE of that stream's P pictures in a CQP run with the QPs
      12..37 cycled over the streams (tools/rate_control_rate.py's (b)), first QP 24.
Prints macroblocks/s of each (one timed GOP after a warm-up GOP), the mean PSNR / SSIM of (b), for (c) the achieved SSE
against the target per QP class, and -- unless --no-prof -- the time of k_quality and of the source snapshot (a device
copy) from a separate run of (b) under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/quality_rate.py [--streams 256] [--configs abc] [--no-prof]"""
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

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from conftest import load_pkg  # noqa: E402


def make_frames(S, GOP, W, H_IN, H):
    import torch
    from h264_fer_amd.synth import gen_frames_torch
    dev = torch.device("cuda", 0)
    fr = gen_frames_torch(W, H_IN, GOP, S, dev, seed=1234, noise=2)
    ys, ct = W * H_IN, (H_IN - H) // 2
    Y = fr[:, :, :ys].view(GOP, S, H_IN, W)[:, :, ct:ct + H, :]
    U = fr[:, :, ys:ys + ys // 4].view(GOP, S, H_IN // 2, W // 2)[:, :, ct // 2:ct // 2 + H // 2, :]
    V = fr[:, :, ys + ys // 4:].view(GOP, S, H_IN // 2, W // 2)[:, :, ct // 2:ct // 2 + H // 2, :]
    frames = torch.cat([Y.reshape(GOP, S, -1), U.reshape(GOP, S, -1), V.reshape(GOP, S, -1)], dim=2).contiguous()
    del fr, Y, U, V
    torch.cuda.synchronize()
    return frames


def profile(args):
    """(b) once more in a child process under rocprofv3; -> {kernel name: (calls, total ms, mean us)} of the rows that
    matter here"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"error": "rocprofv3 not found"}
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "q", "--", sys.executable, __file__,
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
                    if any(k in name for k in ("k_quality", "copyBuffer", "k_rc_plan", "k_cavlc")):
                        calls = int(row.get("Calls", 0))
                        tot = float(row.get("TotalDurationNs", 0))
                        out[name[:60]] = {"calls": calls, "total_ms": round(tot / 1e6, 3),
                                          "mean_us": round(tot / max(calls, 1) / 1e3, 1)}
        if not out:  # say what rocprofv3 wrote instead
            out["files"] = [str(p.relative_to(d)) for p in files]
            out["headers"] = [open(p).readline().strip()[:200] for p in files if "stats" in p.name]
            out["tail"] = (r.stdout[-300:], r.stderr[-300:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--configs", default="abc")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--prof-only", action="store_true", help="only the rocprofv3 run of (b)")
    args = ap.parse_args()
    if args.prof_only:
        print(json.dumps({"rocprof_b": profile(args)}), flush=True)
        return
    W, H_IN, H, GOP, S = 1920, 1080, 1072, 30, args.streams
    pkg = load_pkg()
    frames = make_frames(S, GOP, W, H_IN, H)
    nmb = (W // 16) * (H // 16)
    cqp = [12 + s % 26 for s in range(S)]

    def run(setup, read_ring=False):
        e = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=GOP)
        setup(e)
        q = None
        for _ in range(2):  # warm-up GOP, timed GOP
            e.sync()
            t0 = time.perf_counter()
            for t in range(GOP):
                e.set_frames_device(frames[t].data_ptr())
                e.encode_picture_device(None)
            if read_ring:
                q = e.quality(GOP)  # once per GOP (waits for the last picture)
            e.sync()
            dt = time.perf_counter() - t0
        assert e.status() == [0] * S
        e.close()
        return S * GOP * nmb / dt, q

    out = {"streams": S, "coded_size": f"{W}x{H}", "gop": GOP}
    if "a" in args.configs:
        out["a_off_mbps"] = run(lambda e: None)[0]
    if "b" in args.configs:
        rate, q = run(lambda e: e.set_quality(pkg.QM_SSE | pkg.QM_SSIM), read_ring=True)
        out["b_sse_ssim_mbps"] = rate
        out["b_mean_psnr_y"] = round(float(q.psnr[:, :, 0].mean()), 3)
        out["b_mean_ssim"] = round(float(q.ssim.mean()), 5)
    if "c" in args.configs:
        def setb(e):
            e.set_quality(pkg.QM_SSE)
            for s in range(S):
                e.set_rate(s, pkg.RC_CQP, qp=cqp[s])
        _, qb = run(setb, read_ring=True)
        isP = qb.nal_type[:, 0] == pkg.ferhip.NAL_SLICE
        targets = qb.sse[isP, :, 0].mean(axis=0).astype(np.int64)

        def setc(e):
            for s in range(S):
                e.set_rate(s, pkg.RC_QUALITY, qp=24, qp_min=0, qp_max=51, max_step=2, ip_offset=3,
                           target_sse=int(targets[s]))
        rate, qc = run(lambda e: (setc(e), e.set_quality(pkg.QM_SSE)), read_ring=True)
        out["c_quality_mbps"] = rate
        rows = []
        isPc = qc.nal_type[:, 0] == pkg.ferhip.NAL_SLICE
        for qq in sorted(set(cqp)):
            ss = [s for s in range(S) if cqp[s] == qq]
            tgt = float(targets[ss].mean())
            ach = float(qc.sse[isPc][:, ss, 0].mean())
            rows.append({"cqp": qq, "streams": len(ss), "target_sse": round(tgt), "achieved_sse": round(ach),
                         "ratio": round(ach / tgt, 3), "mean_qp": round(float(qc.qp[isPc][:, ss].mean()), 2)})
        out["c_table"] = rows
    print(json.dumps(out), flush=True)
    if not args.no_prof and "b" in args.configs:
        del frames
        print(json.dumps({"rocprof_b": profile(args)}), flush=True)


if __name__ == "__main__":
    os.environ.setdefault("PYTHONUNBUFFERED", "1")
    main()
