#!/usr/bin/env python3
"""Rate of the converting ingest (ferhip_set_pictures in FERHIP_FMT_YUY2 / FERHIP_FMT_BGRA, k_pic_ingest_packed of
fer_pic.hip) against the NV12 descriptor ingest and against the route a caller had before it, all from device memory, in
one process.  S streams of 1920x1072, one region of a pool per stream:

  (d)           k_pic_ingest          NV12 at pitch 2048: the yardstick (arm (d) of tools/pic_ingest_rate.py)
  yuy2_p4096    k_pic_ingest_packed   YUY2 at pitch 4096        yuy2_tight   at the row's 3840 bytes
  bgra_p8192    k_pic_ingest_packed   BGRA at pitch 8192        bgra_tight   at the row's 7680 bytes
  bgra_torch    the route without the format: torch integer ops with the formulas of include/ferhip.h (BT.601) from the pitched
                BGRA pool into a packed [S][W*H*3/2] array, a synchronise of torch's stream (the library launches on its
                own), then ferhip_set_frames(host = 0)

Every arm's time is divided by the bytes it moves (source bytes + coded bytes); the expectation is that a converting arm's
time per byte is within 25 % of (d)'s in the same run and its time below bgra_torch's.  Every figure is HIP-event time over
`reps` back-to-back calls after `warmup` calls, the arms alternate, `rounds` times, and the median round is reported with the
spread; see tools/pic_ingest_rate.py for what such a figure contains besides the kernel.  The tool also checks that
bgra_p8192 and bgra_torch leave identical pictures in the context.  One JSON line.

  --emit   instead: S 1920x1088 streams of --pictures pictures are encoded, then decoded picture by picture by the live
           decoder into device slots with the window (0, 0, 1920, 1080), as NV12 at pitch 2048 (k_pic_emit), YUY2 at pitch 4096
           and BGRA at pitch 8192 (k_pic_emit_packed): one launch of the output kernel per picture.  The mode times nothing
           itself: run it under `rocprofv3 --kernel-trace` and read the launches' device times there, leaving out the first
           few of each layout as warm-up, and scale by the bytes written that each line reports.

    python tools/pic_convert_rate.py --streams 256 --reps 50 --rounds 5
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
from conftest import load_pkg  # noqa: E402


def emit(a, pkg):
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
    layouts = (("nv12", pkg.FMT_NV12, 2048, 2048, W * dh * 3 // 2), ("yuy2", pkg.FMT_YUY2, 4096, 0, 2 * W * dh),
               ("bgra", pkg.FMT_BGRA, 8192, 0, 4 * W * dh))
    for name, fmt, py, pc, written in layouts:
        dec = pkg.LiveDecoder(S, W, H, 1)
        dec.set_display(0, 0, W, dh)
        dec.set_layout(fmt, py, pc)
        out = pkg.DeviceBuffer(S * dec.fsz + 16)
        for t in range(T):
            _, pics, st = dec.decode([x[t] for x in aus], out)
            assert pics == [1] * S and st == [0] * S
        print(json.dumps(dict(emit=name, streams=S, slot=dec.fsz, pictures=T, bytes_written_per_launch=S * written,
                              bytes_read_per_launch=S * W * dh * 3 // 2)), flush=True)
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
    a = ap.parse_args()
    pkg = load_pkg()
    if a.emit:
        return emit(a, pkg)
    import torch
    dev = torch.device("cuda:0")
    S, W, H = a.streams, 1920, 1072
    fsz = W * H * 3 // 2
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

    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    nv12_pool = torch.randint(0, 256, (S, H * 3 // 2, 2048), dtype=torch.uint8, device=dev, generator=g)
    bgra_pool = torch.randint(0, 256, (S, H, 8192), dtype=torch.uint8, device=dev, generator=g)  # YUY2 at pitch 4096 lies in it too
    staged = torch.empty((S, fsz), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    nv12 = pkg.pic_table([([nv12_pool[s].data_ptr(), nv12_pool[s].data_ptr() + 2048 * H], [2048, 2048]) for s in range(S)])

    def table(pitch):
        return pkg.pic_table([([bgra_pool[s].data_ptr()], [pitch]) for s in range(S)])
    tabs = {k: table(p) for k, p in (("yuy2_p4096", 4096), ("yuy2_tight", 3840), ("bgra_p8192", 8192), ("bgra_tight", 7680))}
    sy, sc = staged[:, :W * H].view(S, H, W), staged[:, W * H:].view(S, 2, H // 2, W // 2)

    def torch_route():
        px = bgra_pool[:, :, :4 * W].view(S, H, W, 4)
        B, G, R = (px[..., k].to(torch.int32) for k in range(3))
        sy.copy_(16 + ((66 * R + 129 * G + 25 * B + 128) >> 8))
        Bs, Gs, Rs = (c.view(S, H // 2, 2, W // 2, 2).sum((2, 4)) for c in (B, G, R))
        sc[:, 0].copy_(128 + ((-38 * Rs - 74 * Gs + 112 * Bs + 512) >> 10))
        sc[:, 1].copy_(128 + ((112 * Rs - 94 * Gs - 18 * Bs + 512) >> 10))
        torch.cuda.current_stream().synchronize()
        enc.set_frames_device(staged.data_ptr())

    def pic_arm(tab, fmt):
        return lambda: enc.lib.ferhip_set_pictures(enc.ctx, tab, fmt)
    arms = dict(d_pic_nv12=pic_arm(nv12, pkg.FMT_NV12), yuy2_p4096=pic_arm(tabs["yuy2_p4096"], pkg.FMT_YUY2),
                yuy2_tight=pic_arm(tabs["yuy2_tight"], pkg.FMT_YUY2), bgra_p8192=pic_arm(tabs["bgra_p8192"], pkg.FMT_BGRA),
                bgra_tight=pic_arm(tabs["bgra_tight"], pkg.FMT_BGRA), bgra_torch=torch_route)
    moved = dict(d_pic_nv12=2 * S * fsz, yuy2_p4096=S * (2 * W * H + fsz), yuy2_tight=S * (2 * W * H + fsz),
                 bgra_p8192=S * (4 * W * H + fsz), bgra_tight=S * (4 * W * H + fsz), bgra_torch=S * (4 * W * H + fsz))
    res = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, f in arms.items():
            res[k].append(timed(enc, f))
    # both BGRA routes must fill the same pictures
    assert arms["bgra_p8192"]() == 0
    enc.sync()
    want = enc.read("CUR")
    arms["bgra_torch"]()
    enc.sync()
    same = bool((enc.read("CUR") == want).all())
    enc.close()

    med = {k: statistics.median(v) for k, v in res.items()}
    ps_per_byte = {k: med[k] * 1e9 / moved[k] for k in arms}
    new = ("yuy2_p4096", "yuy2_tight", "bgra_p8192", "bgra_tight")
    out = dict(streams=S, reps=a.reps, rounds=a.rounds, coded=f"{W}x{H}",
               ms={k: round(v, 4) for k, v in med.items()}, ms_min_max={k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
               TBps={k: round(moved[k] / med[k] / 1e9, 2) for k in arms}, ps_per_byte={k: round(v, 4) for k, v in ps_per_byte.items()},
               per_byte_over_d={k: round(ps_per_byte[k] / ps_per_byte["d_pic_nv12"], 3) for k in new},
               within_margin={k: ps_per_byte[k] <= 1.25 * ps_per_byte["d_pic_nv12"] for k in new},
               over_torch={k: round(med[k] / med["bgra_torch"], 4) for k in ("bgra_p8192", "bgra_tight")},
               bgra_equals_torch=same)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
