"""Live-decoder throughput: S 1920x1072 IPPP streams produced by the GPU encoder (qp 12 and qp 28) are decoded three ways:
  (a) ferhip_decode_streams: every stream complete, windows of many pictures per stream parsed by one launch;
  (b) LiveDecoder, one picture of every stream per call (decoded pictures go to device memory);
  (c) S separate streaming Decoder objects (ferhip_dec_nal), fed NAL unit by NAL unit in round-robin (each picture is
      copied to the host, as Decoder.nal does).  Its decoders run one after the other, so its rate does not depend on S:
      it is measured once per qp on --cap-c streams (one 1080p picture takes a few hundred ms to parse on its own).
Prints macroblocks/s of each and the median / p99 call latency of (b), one JSON line per (qp, S).
Usage: python tools/live_decode_rate.py [--streams 8,64,128] [--pictures 30] [--cap-c 8]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from conftest import load_pkg  # noqa: E402

pkg = load_pkg()
W, H = 1920, 1072
NMB = (W // 16) * (H // 16)
DISTINCT = 4  # distinct encoded streams, repeated up to S (the decoder's work depends on the content, not on identity)


def encode(qp, T):
    frames = np.stack([np.stack([pkg.gen_frame(W, H, t, 1234 + s, 2) for s in range(DISTINCT)]) for t in range(T)])
    g = pkg.FerHip(W, H, DISTINCT, qp=qp, window=32, maxdiff=3, intra_every=30)
    streams, _ = g.encode_streams(frames)
    g.close()
    return streams


def rate_a(streams, T):
    pkg.decode_streams(streams, T, want_pictures=False)  # warm-up: window buffers, tables
    t0 = time.perf_counter()
    _, pics, _, _ = pkg.decode_streams(streams, T, want_pictures=False)
    dt = time.perf_counter() - t0
    assert pics == [T] * len(streams)
    return len(streams) * T * NMB / dt


def rate_b(streams, T):
    S = len(streams)
    aus = [pkg.access_units(s) for s in streams]
    assert all(len(a) == T for a in aus)
    dec = pkg.LiveDecoder(S, W, H, 1)
    buf = pkg.DeviceBuffer(S * W * H * 3 // 2)
    dec.decode([a[0] for a in aus], buf)  # warm-up call (staging, hold buffer, tables), then a fresh decoder state
    for s in range(S):
        dec.reset_stream(s)
    lat = []
    t0 = time.perf_counter()
    for t in range(T):
        c0 = time.perf_counter()
        _, pics, status = dec.decode([a[t] for a in aus], buf)
        lat.append(time.perf_counter() - c0)
        assert pics == [1] * S and status == [0] * S, (pics, status)
    dt = time.perf_counter() - t0
    dec.close()
    buf.free()
    lat = np.array(lat) * 1e3
    return S * T * NMB / dt, float(np.median(lat)), float(np.percentile(lat, 99))


def rate_c(streams, T):
    S = len(streams)
    nals = [[pkg.unescape_nal(n) for n in pkg.split_nals(s)] for s in streams]
    decs = [pkg.Decoder() for _ in range(S)]
    for s in range(S):  # parameter sets and the first picture: warm-up
        for k in range(3):
            decs[s].nal(*nals[s][k])
    t0 = time.perf_counter()
    n = 0
    for k in range(3, len(nals[0])):
        for s in range(S):
            if decs[s].nal(*nals[s][k]) is not None:
                n += 1
    dt = time.perf_counter() - t0
    for d in decs:
        d.close()
    return n * NMB / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="8,64,128")
    ap.add_argument("--pictures", type=int, default=30)
    ap.add_argument("--cap-c", type=int, default=8)
    ap.add_argument("--qps", default="12,28")
    a = ap.parse_args()
    T = a.pictures
    for qp in [int(q) for q in a.qps.split(",")]:
        base = encode(qp, T)
        sc = a.cap_c
        rc = rate_c([base[s % DISTINCT] for s in range(sc)], T)
        for S in [int(x) for x in a.streams.split(",")]:
            streams = [base[s % DISTINCT] for s in range(S)]
            ra = rate_a(streams, T)
            rb, med, p99 = rate_b(streams, T)
            print(json.dumps(dict(qp=qp, streams=S, pictures=T, a_decode_streams_mb_s=round(ra), b_live_mb_s=round(rb),
                                  b_call_ms_median=round(med, 3), b_call_ms_p99=round(p99, 3), c_streams=sc, c_separate_mb_s=round(rc),
                                  b_over_c=round(rb / rc, 2), b_over_a=round(rb / ra, 3))), flush=True)


if __name__ == "__main__":
    main()
