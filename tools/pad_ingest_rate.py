#!/usr/bin/env python3
"""Rate of the display-size ingest (ferhip_set_frames_display, k_pad_ingest of fer_pic.hip) against the coded-size ingest
of the same context (ferhip_set_frames, k_repack), both from device memory.

  S 1920x1080 streams in a 1920x1088 context, and S 1366x768 streams in a 1376x768 context.

k_repack is the yardstick: it writes exactly the same destination bytes and reads slightly more (coded-size pictures).
Every figure is HIP-event time over `reps` back-to-back calls after `warmup` calls, on the library's own stream (the calls
are asynchronous, so the events bracket the kernels, not the Python loop); the two kernels are timed alternately, `rounds`
times, and the median round is reported with the spread.  One JSON line per size.

    python tools/pad_ingest_rate.py --streams 64 --reps 20 --rounds 5
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
from conftest import load_pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    dev = torch.device("cuda:0")
    for W, H, dw, dh in ((1920, 1088, 1920, 1080), (1376, 768, 1366, 768)):
        S = a.streams
        enc = pkg.FerHip(W, H, S, qp=20, window=16)
        enc.set_display_size(dw, dh)
        g = torch.Generator(device=dev).manual_seed(1)
        coded = torch.randint(0, 256, (S, W * H * 3 // 2), dtype=torch.uint8, device=dev, generator=g)
        disp = torch.randint(0, 256, (S, dw * dh * 3 // 2), dtype=torch.uint8, device=dev, generator=g)
        torch.cuda.synchronize()

        def timed(call):
            for _ in range(a.warmup):
                call()
            enc.sync()
            # the library launches on a stream of its own: events on that stream are not reachable from here, so the
            # stream is idle at `t0` (sync above), the calls are enqueued without waiting, and `t1` follows the last sync
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            torch.cuda.synchronize()
            for _ in range(a.reps):
                call()
            enc.sync()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / a.reps

        pad, rep = [], []
        for _ in range(a.rounds):
            rep.append(timed(lambda: enc.set_frames_device(coded.data_ptr())))
            pad.append(timed(lambda: enc.set_frames_display(disp.data_ptr())))
        mp, mr = statistics.median(pad), statistics.median(rep)
        moved = S * (dw * dh + W * H) * 3 // 2
        print(json.dumps(dict(coded=f"{W}x{H}", display=f"{dw}x{dh}", streams=S, reps=a.reps, rounds=a.rounds,
                              pad_ms=round(mp, 4), pad_ms_min_max=[round(min(pad), 4), round(max(pad), 4)],
                              repack_ms=round(mr, 4), repack_ms_min_max=[round(min(rep), 4), round(max(rep), 4)],
                              ratio=round(mp / mr, 3), pad_GBps=round(moved / mp / 1e6, 1),
                              repack_GBps=round(S * W * H * 3 / mr / 1e6, 1))), flush=True)
        enc.close()
        del coded, disp


if __name__ == "__main__":
    main()
