"""Per-stream QP and the device rate controller (ferhip_set_rate, k_rc_plan), through the C ABI against the oracle.

The picture-by-picture oracle comparison is tests/picture_oracle.py."""
import numpy as np
import pytest
from rate_model import ABR, CQP, I, P, RateModel

from picture_oracle import check_pictures as _check_pictures
from picture_oracle import encode_by_picture as _encode_by_picture
from picture_oracle import frames as _frames
from picture_oracle import oracle_pictures as _oracle_pictures
from picture_oracle import split_slice as _split_slice

pytestmark = pytest.mark.gpu
IDR, SLICE = 5, 1


def _annexb(g, s, pics):
    sps, pps = g.sps_pps(s)
    return sps + pps + b"".join(g.write_nal(nt, rb) for nt, rb, _, _ in pics)


@pytest.mark.parametrize("W,H", [(176, 144), (352, 288)])
def test_per_stream_constant_qp_matches_oracle(pkg, fo, W, H):
    qps = [10, 12, 20, 28, 33, 37]
    S, T = len(qps), 8
    frames = _frames(pkg, W, H, T, S, cut=5)
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=30)
    for s, q in enumerate(qps):
        g.set_rate(s, CQP, qp=q)
    streams, rec, used = g.encode_streams(frames, want_recon=True, want_qp=True)
    assert g.status() == [0] * S
    assert (used == np.array(qps)[None, :]).all()
    # the C entry point writes the same per-stream PPS (a second context, same settings)
    g2 = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=30)
    for s, q in enumerate(qps):
        g2.set_rate(s, CQP, qp=q)
    streams2, _ = g2.encode_streams(frames)
    assert streams2 == streams
    g2.close()
    counts = g.stats()
    for s, q in enumerate(qps):
        o = fo.Oracle(W, H, qp=q, window=16, maxdiff=3, intra_every=30)
        ref, ref_rec = o.encode_stream(frames[:, s])
        ref_counts = list(o.stats())
        o.close()
        assert streams[s] == ref, f"stream {s} (qp {q}): bitstream"
        assert np.array_equal(rec[:, s], ref_rec), f"stream {s}: recon"
        assert list(counts[s]) == ref_counts, f"stream {s}: brojTipova"
    assert sum(1 for b in streams[0].split(b"\x00\x00\x00\x01") if b and (b[0] & 31) == 5) == 2, "the scene cut makes an IDR"
    g.close()


def test_per_stream_qp_at_1080p_across_ticket_queues(pkg, fo):
    W, H, T, S = 1920, 1072, 2, 16
    qps = [12 + (s * 5) % 26 for s in range(S)]
    assert len(set(qps)) == S
    frames = _frames(pkg, W, H, T, S, seed=99)
    g = pkg.FerHip(W, H, S, qp=12, window=16, maxdiff=3, intra_every=30)
    for s, q in enumerate(qps):
        g.set_rate(s, CQP, qp=q)
    streams, rec = g.encode_streams(frames, want_recon=True)
    assert g.status() == [0] * S
    assert g.last_qp() == qps
    for s in (0, 7, 8, 15):
        o = fo.Oracle(W, H, qp=qps[s], window=16, maxdiff=3, intra_every=30)
        ref, ref_rec = o.encode_stream(frames[:, s])
        o.close()
        assert np.array_equal(rec[:, s], ref_rec), f"stream {s} (qp {qps[s]}): recon"
        assert streams[s] == ref, f"stream {s} (qp {qps[s]}): bitstream"
    g.close()


# QP of every picture per stream: 0 and 51, jumps of more than 6, IDR pictures at 0 and 4 (intra_every 4)
SCHED = [[20, 0, 51, 10, 30, 5, 45, 12, 37],
         [37, 12, 25, 51, 0, 40, 20, 33, 8],
         [12, 30, 14, 28, 13, 40, 26, 12, 51]]


def test_qp_changing_every_picture_matches_oracle(pkg, fo):
    W, H, T, S = 176, 144, len(SCHED[0]), len(SCHED)
    frames = _frames(pkg, W, H, T, S, seed=321)
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=4)
    sched = np.array(SCHED).T  # [T][S]
    res = _encode_by_picture(g, frames, sched)
    assert g.status() == [0] * S
    counts = g.stats()
    for s in range(S):
        assert [p[3] for p in res[s]] == SCHED[s]
        assert sum(p[0] == IDR for p in res[s]) == 3
        ora, ocnt = _oracle_pictures(fo, frames[:, s], SCHED[s], W, H, intra_every=4)
        _check_pictures(res[s], SCHED[s][0], ora, f"stream {s}")
        assert list(counts[s]) == ocnt, f"stream {s}: brojTipova"
    # decoders: the GPU decoder and the oracle decoder give back the encoder's luma (streams whose QPs are all >= 12)
    ys = W * H
    for s in range(S):
        if min(SCHED[s]) < 12:
            continue
        pics = res[s]
        stream = _annexb(g, s, pics)
        out, npics, _, _ = pkg.decode_streams([stream], len(pics))
        assert npics == [len(pics)]
        n, dec, _ = fo.decode_stream_md5(stream)
        assert n == len(pics)
        for t, p in enumerate(pics):
            assert np.array_equal(out[t, 0][:ys], p[2][:ys]), f"GPU decoder, stream {s} picture {t}"
            assert np.array_equal(dec[t][:ys], p[2][:ys]), f"oracle decoder, stream {s} picture {t}"
    g.close()


# ABR settings per stream: target bits, window, ip_offset, max_step, qp_min, qp_max, first qp
ABR_SET = [(6000, 0, 3, 2, 0, 51, 26), (12000, 5, 2, 1, 10, 40, 20), (25000, 0, 4, 3, 0, 51, 30), (50000, 15, 0, 2, 5, 45, 18),
           (3000, 8, 6, 4, 20, 51, 34), (100000, 0, 3, 2, 0, 30, 12), (18000, 30, 1, 5, 0, 51, 37), (9000, 3, 3, 2, 12, 36, 24)]


def _set_abr(g, s, k):
    tgt, win, ipo, step, lo, hi, q0 = ABR_SET[k]
    g.set_rate(s, ABR, qp=q0, qp_min=lo, qp_max=hi, max_step=step, ip_offset=ipo, window=win, target_bits=tgt)


def _model(k, intra_every):
    tgt, win, ipo, step, lo, hi, q0 = ABR_SET[k]
    m = RateModel(26, intra_every)
    m.set_rate(ABR, q0, qp_min=lo, qp_max=hi, max_step=step, ip_offset=ipo, window=win, target_bits=tgt)
    return m


def _abr_run(pkg, frames, streams, intra_every, switch=None):
    """streams: ABR_SET index of every stream of the context; switch = (stream, t_cqp, t_abr): that stream goes to CQP
    at picture t_cqp and back to ABR at t_abr"""
    T, S = frames.shape[0], len(streams)
    W, H = 176, 144
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=intra_every)
    for s, k in enumerate(streams):
        _set_abr(g, s, k)
    res = [[] for _ in range(S)]
    for t in range(T):
        if switch and t == switch[1]:
            g.set_rate(switch[0], CQP, qp=22)
        if switch and t == switch[2]:
            _set_abr(g, switch[0], streams[switch[0]])
        g.set_frames(frames[t][:S])
        rbsp, nt = g.encode_picture()
        rec = g.get_recon()
        qps = g.last_qp()
        for s in range(S):
            res[s].append((nt[s], rbsp[s], rec[s], qps[s]))
    assert g.status() == [0] * S
    return g, res


def test_device_controller_follows_the_model(pkg, fo):
    W, H, IE = 176, 144, 10
    T, S = 3 * IE, len(ABR_SET)
    frames = _frames(pkg, W, H, T, S, seed=555, cut=17)
    sw = (7, 12, 16)
    g, res = _abr_run(pkg, frames, list(range(S)), IE, switch=sw)
    for s in range(S):
        m = _model(s, IE)
        want = []
        for t, (nt, rb, _, q) in enumerate(res[s]):
            if s == sw[0] and t == sw[1]:
                m.set_rate(CQP, 22)
            if s == sw[0] and t == sw[2]:
                tgt, win, ipo, step, lo, hi, q0 = ABR_SET[s]
                m.set_rate(ABR, q0, qp_min=lo, qp_max=hi, max_step=step, ip_offset=ipo, window=win, target_bits=tgt)
            want.append(m.pick(I if nt == IDR else P))
            m.coded(len(rb))
        got = [p[3] for p in res[s]]
        assert got == want, f"stream {s}: device QPs {got} != model {want}"
        assert len(set(got)) > 1, f"stream {s}: the controller never moved"
        ora, _ = _oracle_pictures(fo, frames[:, s], got, W, H, intra_every=IE)
        _check_pictures(res[s], ABR_SET[s][6], ora, f"stream {s}")
    g.close()


def test_abr_streams_are_isolated(pkg):
    W, H, IE = 176, 144, 10
    T = 2 * IE
    frames = _frames(pkg, W, H, T, 8, seed=777)
    g, batch = _abr_run(pkg, frames, list(range(8)), IE)
    g.close()
    for s in (3, 6):
        g1, alone = _abr_run(pkg, frames[:, s:s + 1], [s], IE)
        g1.close()
        assert [p[3] for p in alone[0]] == [p[3] for p in batch[s]], f"stream {s}: QPs"
        assert [p[1] for p in alone[0]] == [p[1] for p in batch[s]], f"stream {s}: bytes"


def test_device_path_back_to_back_in_abr(pkg):
    W, H, T, S = 176, 144, 12, 4
    frames = _frames(pkg, W, H, T, S, seed=888)
    types = [[IDR if t % 6 == 0 else SLICE] * S for t in range(T)]
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=1000)
    for s in range(S):
        _set_abr(g, s, s)
    host = _encode_by_picture(g, frames, types=types)
    g.close()
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=1000)
    for s in range(S):
        _set_abr(g, s, s)
    fsz, stride = g.fsz, g.nmb * 1024 + 4096
    dev = pkg.DeviceBuffer(T * S * fsz)
    dev.upload(frames)
    keep = pkg.DeviceBuffer(T * S * stride)
    lens = pkg.DeviceBuffer(T * S * 4)
    for t in range(T):
        g.set_frames_device(dev.ptr + t * S * fsz)
        _, _, _, nt = g.encode_picture_device(types[t])
        g.copy_rbsp_device(keep.ptr + t * S * stride, lens.ptr + t * S * 4)
    assert g.status() == [0] * S
    kb = keep.download().reshape(T, S, stride)
    ln = lens.download(dtype=np.uint32).reshape(T, S)
    assert g.last_qp() == [host[s][-1][3] for s in range(S)]
    for s in range(S):
        base = ABR_SET[s][6]
        for t in range(T):
            rb = bytes(kb[t, s, :ln[t, s]])
            assert rb == host[s][t][1], f"stream {s} picture {t}: bytes"
            assert _split_slice(rb, types[t][s])[1] + base + 14 == host[s][t][3], f"stream {s} picture {t}: qp"
    for b_ in (dev, keep, lens):
        b_.free()
    g.close()


@pytest.mark.parametrize("W,H", [(352, 288), (1280, 720)])
def test_abr_accuracy(pkg, W, H):
    """Targets = the mean RBSP bits per picture of constant-QP runs at 16, 24 and 32; ABR from QP 26.  Over the pictures
    after the first GOP the mean is within 15 % of the target, and a higher target never gets a higher mean QP."""
    IE = 10
    T, S = 3 * IE, 3
    frames = np.stack([np.stack([pkg.gen_frame(W, H, t, 4242, 2)] * S) for t in range(T)])
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=IE)
    for s, q in enumerate((16, 24, 32)):
        g.set_rate(s, CQP, qp=q)
    cq = _encode_by_picture(g, frames)
    g.close()
    targets = [int(np.mean([8 * len(p[1]) for p in cq[s]])) for s in range(S)]
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=IE)
    for s in range(S):
        g.set_rate(s, ABR, qp=26, qp_min=0, qp_max=51, max_step=2, ip_offset=3, window=0, target_bits=targets[s])
    ab = _encode_by_picture(g, frames)
    assert g.status() == [0] * S
    g.close()
    rows = []
    for s in range(S):
        mean = float(np.mean([8 * len(p[1]) for p in ab[s][IE:]]))
        mq = float(np.mean([p[3] for p in ab[s][IE:]]))
        rows.append((targets[s], mean, mq, [p[3] for p in ab[s]]))
    print("\nABR accuracy %dx%d:" % (W, H), *["target %d achieved %.0f (%.3f) mean qp %.2f qps %s" % (t, m, m / t, q, qs)
                                            for t, m, q, qs in rows], sep="\n  ")
    for t, m, _, _ in rows:
        assert abs(m / t - 1) <= 0.15, rows
    mqs = [r[2] for r in sorted(rows)]
    assert all(a >= b for a, b in zip(mqs, mqs[1:])), rows


def test_set_rate_arguments(pkg):
    W, H, S = 176, 144, 2
    g = pkg.FerHip(W, H, S, qp=20, window=16, maxdiff=3, intra_every=30)
    bad = [dict(stream=2), dict(stream=-2), dict(qp=-1), dict(qp=52), dict(qp=38),
           dict(mode=ABR, qp=20, qp_min=30, qp_max=20, target_bits=1000), dict(mode=ABR, qp=20, target_bits=0),
           dict(mode=ABR, qp=20, target_bits=-5), dict(mode=ABR, qp=20, qp_min=-1, target_bits=1000),
           dict(mode=ABR, qp=20, qp_max=52, target_bits=1000), dict(mode=ABR, qp=20, max_step=0, target_bits=1000),
           dict(mode=ABR, qp=20, window=-1, target_bits=1000), dict(mode=2, qp=20)]
    for kw in bad:
        with pytest.raises(pkg.FerHipError):
            g.set_rate(**kw)
    pps0 = g.sps_pps(0)[1]
    assert pps0 == g.sps_pps()[1]       # base = params.qp until set_rate
    g.set_rate(0, CQP, qp=37)           # 37 is the largest base
    g.set_rate(1, CQP, qp=14)
    assert g.sps_pps(0)[1] != pps0
    pps = [g.sps_pps(s)[1] for s in range(S)]
    assert g.sps_pps()[1] == pps0       # ferhip_write_pps keeps params.qp
    frames = _frames(pkg, W, H, 2, S)
    g.set_frames(frames[0])
    g.encode_picture()
    assert g.last_qp() == [37, 14]
    # after the first picture the base is frozen: larger QPs are fine, the PPS does not change
    g.set_rate(-1, CQP, qp=45)
    assert [g.sps_pps(s)[1] for s in range(S)] == pps
    g.set_frames(frames[1])
    rbsp, nt = g.encode_picture()
    assert g.last_qp() == [45, 45]
    assert [_split_slice(rbsp[s], nt[s])[1] for s in range(S)] == [45 - 37 - 14, 45 - 14 - 14]
    with pytest.raises(pkg.FerHipError):
        g.sps_pps(S)
    g.close()
