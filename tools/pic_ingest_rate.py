#!/usr/bin/env python3
"""Rate of the descriptor ingest (ferhip_set_pictures, k_pic_ingest of fer_pic.hip) against the packed ingests and against
the route a caller had before it, all from device memory, in one process.

  (a) k_repack       ferhip_set_frames(host = 0) from a packed [S][W*H*3/2] array, S streams of 1920x1072
  (b) k_pad_ingest   ferhip_set_frames_display(host = 0), 1920x1080 pictures into a 1920x1088 context
  (c) k_pic_ingest   I420 at pitch 2048 (chroma 1024), one region per stream, 1920x1072
  (d) k_pic_ingest   NV12 at pitch 2048, 1920x1072
  (e) the route without descriptors for (d): torch de-interleaves and packs the pitched NV12 pool into [S][W*H*3/2]
      (three strided copies over the whole pool -- the best case: a pool that is one tensor), a synchronise of torch's stream
      (the library launches on its own), then ferhip_set_frames(host = 0); (e_streams) the same with the copies made stream
      by stream, as for a pool of separate allocations

The yardstick for (c) and (d) is (a) / (b) of the same run plus 25 %: all move about twice the picture's bytes.  Every
figure is HIP-event time over `reps` back-to-back calls after `warmup` calls (the calls only enqueue on the library's own
stream, which is idle at the first event and synchronised before the second); the arms alternate, `rounds` times, and the
median round is reported with the spread.  One JSON line.  The events lie on torch's stream and the work on the library's,
so a figure is the host's time between two synchronised points, not the kernels' device time; and arms (c) and (d) time
ferhip_set_pictures, which (a) has no counterpart of: a 10 KB copy of the descriptor table from pinned memory and an event
record in front of every kernel, and every eighth call may wait in the pinned ring for the copy eight calls back.  The
kernels alone are read from `rocprofv3 --kernel-trace` over the same command.

  --emit   instead: S 1920x1088 streams of --pictures pictures are encoded, then decoded picture by picture by the live
           decoder into device slots with the window (0, 0, 1920, 1080), in the default layout (tight slots) and as NV12 and
           I420 at pitch 2048: one launch of k_pic_emit per picture in all three.  The mode times nothing itself (a decode
           call is dominated by the parse): run it under `rocprofv3 --kernel-trace` and read the launches' device times
           there, leaving out the first few of each layout as warm-up.
  --emit --full --out-offset 1   the default layout only, whole 1920x1088 pictures into a buffer that starts one byte past a
           16-byte boundary (k_pic_emit; at offset 0 the same pictures go through k_dec_out).

    python tools/pic_ingest_rate.py --streams 256 --reps 50 --rounds 5
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
from conftest import load_pkg  # noqa: E402

PITCH = 2048


def emit(a, pkg, torch):
    import numpy as np
    W, H, dh, S, T = 1920, 1088, 1080, a.streams, a.pictures
    enc = pkg.FerHip(W, H, S, qp=28, window=16)
    four = [pkg.gen_frame(W, H, 0, 40 + k, 2) for k in range(4)]
    streams = [b"".join(enc.sps_pps(s)) for s in range(S)]
    for t in range(T):  # the content only has to decode: four pictures, shifted by two columns per picture
        moved = [np.concatenate([np.roll(p.reshape(-1, W), 2 * t, 1).ravel() for p in (f[:W * H], f[W * H:])]) for f in four]
        enc.set_frames(np.stack([moved[s % 4] for s in range(S)]))
        rbsp, nt = enc.encode_picture()
        for s in range(S):
            streams[s] += enc.write_nal(nt[s], rbsp[s])
    enc.close()
    aus = [pkg.access_units(s) for s in streams]
    layouts = (("default", None), ("nv12", (pkg.FMT_NV12, PITCH, PITCH)), ("i420", (pkg.FMT_I420, PITCH, PITCH // 2)))
    for name, layout in layouts[:1] if a.full else layouts:
        dec = pkg.LiveDecoder(S, W, H, 1)
        dec.set_display(0, 0, W, H if a.full else dh)
        if layout:
            dec.set_layout(*layout)
        out = pkg.DeviceBuffer(S * dec.fsz + 32)
        assert out.ptr % 16 == 0
        for t in range(T):
            _, pics, st = dec.decode([x[t] for x in aus], out.ptr + a.out_offset if a.out_offset else out)
            assert pics == [1] * S and st == [0] * S
        print(json.dumps(dict(emit=name, streams=S, slot=dec.fsz, pictures=T, full=a.full, out_offset=a.out_offset)), flush=True)
        dec.close()
        out.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--emit", action="store_true")
    ap.add_argument("--pictures", type=int, default=55, help="--emit: pictures per stream")
    ap.add_argument("--full", action="store_true", help="--emit: whole coded pictures in the default layout only")
    ap.add_argument("--out-offset", type=int, default=0, help="--emit: bytes from a 16-byte boundary to the output buffer")
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    if a.emit:
        return emit(a, pkg, torch)
    dev = torch.device("cuda:0")
    S = a.streams
    g = torch.Generator(device=dev).manual_seed(1)

    def timed(enc, call):
        for _ in range(a.warmup):
            call()
        enc.sync()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            call()
        enc.sync()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.reps

    res = {}
    # (b): 1920x1080 -> 1088
    W, H, dh = 1920, 1088, 1080
    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    enc.set_display_size(W, dh)
    disp = torch.randint(0, 256, (S, W * dh * 3 // 2), dtype=torch.uint8, device=dev, generator=g)
    torch.cuda.synchronize()
    res["b_pad"] = [timed(enc, lambda: enc.set_frames_display(disp.data_ptr())) for _ in range(a.rounds)]
    moved_b = S * (W * dh + W * H) * 3 // 2
    enc.close()
    del disp

    # (a), (c), (d), (e): 1920x1072
    H = 1072
    fsz = W * H * 3 // 2
    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    packed = torch.randint(0, 256, (S, fsz), dtype=torch.uint8, device=dev, generator=g)
    pool = torch.randint(0, 256, (S, H * 3 // 2, PITCH), dtype=torch.uint8, device=dev, generator=g)  # one region per stream
    staged = torch.empty((S, fsz), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    base = [pool[s].data_ptr() for s in range(S)]
    i420 = pkg.pic_table([([b, b + PITCH * H, b + PITCH * H + PITCH // 2 * (H // 2)], [PITCH, PITCH // 2, PITCH // 2]) for b in base])
    nv12 = pkg.pic_table([([b, b + PITCH * H], [PITCH, PITCH]) for b in base])
    sy, sc = staged[:, :W * H].view(S, H, W), staged[:, W * H:].view(S, 2, H // 2, W // 2)

    def torch_route(per_stream):
        if per_stream:
            for s in range(S):
                sy[s].copy_(pool[s, :H, :W])
                uv = pool[s, H:, :W].unflatten(-1, (W // 2, 2))
                sc[s, 0].copy_(uv[..., 0])
                sc[s, 1].copy_(uv[..., 1])
        else:
            sy.copy_(pool[:, :H, :W])
            uv = pool[:, H:, :W].unflatten(-1, (W // 2, 2))
            sc[:, 0].copy_(uv[..., 0])
            sc[:, 1].copy_(uv[..., 1])
        torch.cuda.current_stream().synchronize()
        enc.set_frames_device(staged.data_ptr())

    arms = dict(a_repack=lambda: enc.set_frames_device(packed.data_ptr()),
                c_pic_i420=lambda: enc.lib.ferhip_set_pictures(enc.ctx, i420, pkg.FMT_I420),
                d_pic_nv12=lambda: enc.lib.ferhip_set_pictures(enc.ctx, nv12, pkg.FMT_NV12),
                e_torch=lambda: torch_route(False), e_torch_streams=lambda: torch_route(True))
    for k in arms:
        res[k] = []
    for _ in range(a.rounds):
        for k, f in arms.items():
            res[k].append(timed(enc, f))
    # (d) and (e) must fill the same pictures
    arms["d_pic_nv12"]()
    enc.sync()
    want = enc.read("CUR")
    arms["e_torch"]()
    enc.sync()
    same = bool((enc.read("CUR") == want).all())
    enc.close()

    med = {k: statistics.median(v) for k, v in res.items()}
    moved = 2 * S * fsz
    yard = {"a": 1.25 * med["a_repack"], "b": 1.25 * med["b_pad"] * moved / moved_b}  # (b) moves slightly more: scaled to this size
    out = dict(streams=S, reps=a.reps, rounds=a.rounds, coded=f"{W}x{H}", pitch=PITCH,
               ms={k: round(v, 4) for k, v in med.items()}, ms_min_max={k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
               TBps={k: round((moved_b if k == "b_pad" else moved) / med[k] / 1e9, 2) for k in ("a_repack", "b_pad", "c_pic_i420", "d_pic_nv12")},
               margin_ms={k: round(v, 4) for k, v in yard.items()}, c_within_margin={k: med["c_pic_i420"] <= v for k, v in yard.items()},
               d_within_margin={k: med["d_pic_nv12"] <= v for k, v in yard.items()},
               d_over_e=round(med["d_pic_nv12"] / med["e_torch"], 3), d_over_e_streams=round(med["d_pic_nv12"] / med["e_torch_streams"], 3),
               d_equals_e=same)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
