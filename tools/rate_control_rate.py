"""Encoder rate with per-stream QP and the device rate controller: S 1920x1072 streams in ONE context, bench.py's content
(gen_frames_torch, generated at 1920x1080 and cropped to 1072 rows), window 32, GOP 30, the device path
(ferhip_encode_picture_dev, AUTO picture types) that bench.py times, three configurations:
  (a) default: every stream at params.qp = 12 (what bench.py runs);
  (b) CQP with a different QP per stream, 12..37 cycled;
  (c) ABR on every stream: target = the mean RBSP bits per picture of that stream in (b), first QP 24.
Prints macroblocks/s of each (one timed GOP after a warm-up GOP), and for (c) the target against the achieved mean over
the timed GOP per QP class of (b).  Run it under `rocprofv3 --kernel-trace --stats -- python ...` for k_rc_plan's time.
Usage: python tools/rate_control_rate.py [--streams 256] [--configs abc]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from conftest import load_pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--configs", default="abc")
    args = ap.parse_args()
    import torch
    W, H_IN, H, GOP, S = 1920, 1080, 1072, 30, args.streams
    pkg = load_pkg()
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
    nmb = (W // 16) * (H // 16)
    cqp = [12 + s % 26 for s in range(S)]

    def run(setup):
        e = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=GOP)
        setup(e)
        for _ in range(2):  # warm-up GOP, timed GOP
            e.sync()
            t0 = time.perf_counter()
            for t in range(GOP):
                e.set_frames_device(frames[t].data_ptr())
                e.encode_picture_device(None)
            e.sync()
            dt = time.perf_counter() - t0
        assert e.status() == [0] * S
        e.close()
        return S * GOP * nmb / dt

    def run_lens(setup):
        """one GOP, RBSP lengths and QPs of every picture (host path: the lengths come back with each picture)"""
        e = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=GOP)
        setup(e)
        stride = nmb * 1024 + 4096
        lens, qps = np.zeros((GOP, S), np.int64), np.zeros((GOP, S), np.int64)
        keep = pkg.DeviceBuffer(S * 64)
        ln = pkg.DeviceBuffer(S * 4)
        for t in range(GOP):
            e.set_frames_device(frames[t].data_ptr())
            e.encode_picture_device(None)
            e.copy_rbsp_device(keep.ptr, ln.ptr, stride=64, nbytes=64)
            qps[t] = e.last_qp()  # (waits for the picture and the copy)
            lens[t] = ln.download(dtype=np.uint32)
        assert e.status() == [0] * S
        e.close()
        keep.free()
        ln.free()
        return lens, qps

    out = {"streams": S, "coded_size": f"{W}x{H}", "gop": GOP}
    if "a" in args.configs:
        out["a_default_mbps"] = run(lambda e: None)
    if "b" in args.configs or "c" in args.configs:
        def setb(e):
            for s in range(S):
                e.set_rate(s, pkg.RC_CQP, qp=cqp[s])
        if "b" in args.configs:
            out["b_cqp_mbps"] = run(setb)
        lb, _ = run_lens(setb)
        targets = (8 * lb).mean(axis=0).astype(np.int64)
    if "c" in args.configs:
        def setc(e):
            for s in range(S):
                e.set_rate(s, pkg.RC_ABR, qp=24, qp_min=0, qp_max=51, max_step=2, ip_offset=3, window=0,
                           target_bits=int(targets[s]))
        out["c_abr_mbps"] = run(setc)
        lc, qc = run_lens(setc)
        rows = []
        for q in sorted(set(cqp)):
            ss = [s for s in range(S) if cqp[s] == q]
            tgt = float(targets[ss].mean())
            ach = float((8 * lc[:, ss]).mean())
            rows.append({"cqp": q, "streams": len(ss), "target_bits": round(tgt), "achieved_bits": round(ach),
                         "ratio": round(ach / tgt, 3), "mean_qp": round(float(qc[:, ss].mean()), 2)})
        out["c_table"] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
