"""Quality measurement on the device (ferhip_set_quality / ferhip_get_quality, k_quality) and the FERHIP_RC_QUALITY rate
mode (k_rc_plan), through the C ABI: SSE and SSIM against numpy models of the definitions in include/ferhip.h, the ring,
that measuring changes no byte, and the QUALITY controller against tests/quality_model.py and the oracle."""
import numpy as np
import pytest
from quality_model import CQP, I, P, QUALITY, QualityModel, plane_sse, ssim_windows

from picture_oracle import check_pictures as _check_pictures
from picture_oracle import encode_by_picture as _encode_by_picture
from picture_oracle import frames as _frames
from picture_oracle import oracle_pictures as _oracle_pictures

pytestmark = pytest.mark.gpu
IDR, SLICE = 5, 1
SSE, SSIM = 1, 2


# ---- measurement
def _check_measured(q, src, rec, W, H, ssim):
    """q: Quality of one picture ([1][S]); src, rec: [S][fsz]"""
    S = src.shape[0]
    for s in range(S):
        want = plane_sse(src[s], rec[s], W, H)
        assert list(q.sse[0, s]) == list(want), f"stream {s}: sse {list(q.sse[0, s])} != numpy {list(want)}"
        with np.errstate(divide="ignore"):
            n = np.array([W * H, W * H // 4, W * H // 4], np.float64)
            assert np.array_equal(q.psnr[0, s], 10 * np.log10(255.0 ** 2 * n / want))
        if ssim:
            v = ssim_windows(src[s], rec[s], W, H)
            assert q.ssim_windows[0, s] == (W // 4 - 1) * (H // 4 - 1) == v.size
            assert abs(q.ssim[0, s] - v.mean()) <= 1e-12, f"stream {s}: ssim {q.ssim[0, s]!r} != numpy {v.mean()!r}"
        else:
            assert q.ssim_windows[0, s] == 0 and q.ssim_sum[0, s] == 0.0


@pytest.mark.parametrize("W,H,S", [(16, 16, 2), (208, 112, 2), (352, 288, 2), (1920, 1072, 3)])
def test_sse_and_ssim_match_numpy(pkg, W, H, S):
    T = 3
    frames = _frames(pkg, W, H, T, S, seed=31)
    g = pkg.FerHip(W, H, S, qp=28, window=16, maxdiff=3, intra_every=30)
    g.set_quality(SSE | SSIM)
    types = []
    for t in range(T):
        g.set_frames(frames[t])
        _, nt = g.encode_picture()
        types.append(nt)
        rec = g.get_recon()
        q = g.quality(1)
        _check_measured(q, frames[t], rec, W, H, ssim=True)
        assert list(q.nal_type[0]) == nt
    assert types[0] == [IDR] * S and types[1] == [SLICE] * S, "I and P pictures are both covered"
    assert g.status() == [0] * S
    g.close()


@pytest.mark.parametrize("path", ["host", "device", "upload"])
def test_sse_on_every_ingest_path(pkg, path):
    W, H, S, T = 208, 112, 2, 3
    frames = _frames(pkg, W, H, T, S, seed=47)
    g = pkg.FerHip(W, H, S, qp=30, window=16, maxdiff=3, intra_every=30)
    g.set_quality(SSE)
    fsz = g.fsz
    dev = pin = None
    if path == "device":
        dev = pkg.DeviceBuffer(T * S * fsz)
        dev.upload(frames)
    if path == "upload":
        pin = pkg.DeviceBuffer(T * S * fsz, pinned=True)
        pin.upload(frames)
    for t in range(T):
        if path == "host":
            g.set_frames(frames[t])
        elif path == "device":
            g.set_frames_device(dev.ptr + t * S * fsz)
        else:
            g.upload_frames(pin.ptr + t * S * fsz)
            g.set_frames_uploaded()
        g.encode_picture()
        _check_measured(g.quality(1), frames[t], g.get_recon(), W, H, ssim=False)
    for b in (dev, pin):
        if b is not None:
            b.free()
    g.close()


def test_ssim_sum_is_bit_identical_run_to_run(pkg):
    W, H, S, T = 352, 288, 3, 3
    frames = _frames(pkg, W, H, T, S, seed=5)
    runs = []
    for _ in range(2):
        g = pkg.FerHip(W, H, S, qp=34, window=16, maxdiff=3, intra_every=30)
        g.set_quality(SSE | SSIM)
        for t in range(T):
            g.set_frames(frames[t])
            g.encode_picture()
        q = g.quality(T)
        runs.append((q.ssim_sum.view(np.uint64).copy(), q.sse.copy()))
        g.close()
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1], runs[1][1])


def test_measuring_changes_no_byte(pkg):
    """17 streams: every ticket queue of the motion chain; off, SSE and SSE | SSIM give the same RBSP, recon and stats."""
    W, H, S, T = 176, 144, 17, 4
    frames = _frames(pkg, W, H, T, S, seed=77, cut=3)
    outs = []
    for flags in (0, SSE, SSE | SSIM):
        g = pkg.FerHip(W, H, S, qp=24, window=16, maxdiff=3, intra_every=30)
        if flags:
            g.set_quality(flags)
        res = _encode_by_picture(g, frames)
        assert g.status() == [0] * S
        outs.append((res, g.stats().copy()))
        if flags:
            assert g.quality(T).sse.shape == (T, S, 3)
        g.close()
    for res, st in outs[1:]:
        assert np.array_equal(st, outs[0][1])
        for s in range(S):
            for t in range(T):
                a, b = res[s][t], outs[0][0][s][t]
                assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3], f"stream {s} picture {t}: bytes"
                assert np.array_equal(a[2], b[2]), f"stream {s} picture {t}: recon"


def test_quality_arguments_and_state(pkg):
    W, H, S = 32, 32, 2
    g = pkg.FerHip(W, H, S, qp=20, window=16, maxdiff=3, intra_every=30)
    frames = _frames(pkg, W, H, 1, S)
    g.set_frames(frames[0])
    g.encode_picture()
    with pytest.raises(pkg.FerHipError, match="code -3"):  # FERHIP_E_STATE: never measured
        g.quality(1)
    for bad in (4, -1, 8):
        with pytest.raises(pkg.FerHipError):
            g.set_quality(bad)
    with pytest.raises(pkg.FerHipError, match="code -1"):
        g.quality(0)
    bad = [dict(mode=QUALITY, qp=20, target_sse=0), dict(mode=QUALITY, qp=20, target_sse=-3),
           dict(mode=QUALITY, qp=20, qp_min=30, qp_max=20, target_sse=1000), dict(mode=QUALITY, qp=20, qp_min=-1, target_sse=1000),
           dict(mode=QUALITY, qp=20, qp_max=52, target_sse=1000), dict(mode=QUALITY, qp=20, max_step=0, target_sse=1000),
           dict(mode=QUALITY, qp=20, ip_offset=52, target_sse=1000), dict(mode=QUALITY, qp=52, target_sse=1000),
           dict(mode=3, qp=20, target_sse=1000)]
    for kw in bad:
        with pytest.raises(pkg.FerHipError):
            g.set_rate(**kw)
    g.set_rate(0, QUALITY, qp=20, window=-1, target_sse=1000)  # window is ignored
    assert g.sse_of_psnr(40.0) == int(255 ** 2 * W * H / 10 ** 4.0)
    g.set_rate(1, QUALITY, qp=20, target_psnr=40.0)
    g.close()


def test_ring_keeps_the_last_64_measured_pictures(pkg):
    W, H, S = 32, 32, 3
    T_off, T_on = 3, 70
    T = T_off + T_on + 2
    frames = _frames(pkg, W, H, T, S, seed=9, cut=40)
    g = pkg.FerHip(W, H, S, qp=20, window=16, maxdiff=3, intra_every=12)
    seen = []
    for t in range(T):
        on = T_off <= t < T_off + T_on
        g.set_quality(SSE if on else 0)
        for s in range(S):
            g.set_rate(s, CQP, qp=14 + (3 * t + 5 * s) % 30)
        g.set_frames(frames[t])
        rbsp, nt = g.encode_picture()
        qp = g.last_qp()
        if on:
            q = g.quality(1)
            assert list(q.picture[0]) == [t] * S
            assert list(q.qp[0]) == qp
            assert list(q.nal_type[0]) == nt
            assert list(q.rbsp_bytes[0]) == [len(b) for b in rbsp]
            seen.append(q)
            if t == T_off + 4:
                assert list(g.quality(64).picture[:, 0]) == list(range(T_off, t + 1)), "only measured pictures"
    assert {I_ for q in seen for I_ in q.nal_type[0]} == {IDR, SLICE}
    q = g.quality(64)
    assert q.sse.shape == (64, S, 3)
    assert list(q.picture[:, 0]) == list(range(T_off + T_on - 64, T_off + T_on))
    for k in range(64):
        one = seen[T_on - 64 + k]
        for f in ("sse", "qp", "nal_type", "rbsp_bytes", "picture"):
            assert np.array_equal(getattr(q, f)[k], getattr(one, f)[0]), (k, f)
    assert g.quality(1000).sse.shape == (64, S, 3)
    g.close()


# ---- the QUALITY rate mode
# per stream: target luma SSE, ip_offset, max_step, qp_min, qp_max, first qp
QSET = [(60000, 3, 2, 0, 51, 26), (20000, 2, 1, 10, 40, 20), (150000, 4, 3, 0, 51, 30), (8000, 0, 4, 5, 45, 34)]


def _set_quality_rate(g, s, k):
    tgt, ipo, step, lo, hi, q0 = QSET[k]
    g.set_rate(s, QUALITY, qp=q0, qp_min=lo, qp_max=hi, max_step=step, ip_offset=ipo, target_sse=tgt)


def test_quality_mode_follows_the_model_and_the_oracle(pkg, fo):
    W, H, IE = 176, 144, 10
    T, S = 2 * IE, len(QSET)
    frames = _frames(pkg, W, H, T, S, seed=2024, cut=13)
    sw = (3, 6, 9)  # stream 3: CQP 22 at picture 6, QUALITY again at picture 9
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=IE)
    for s in range(S):
        _set_quality_rate(g, s, s)
    res = [[] for _ in range(S)]
    for t in range(T):
        if t == sw[1]:
            g.set_rate(sw[0], CQP, qp=22)
        if t == sw[2]:
            _set_quality_rate(g, sw[0], sw[0])
        g.set_frames(frames[t])
        rbsp, nt = g.encode_picture()
        rec = g.get_recon()
        qps = g.last_qp()
        for s in range(S):
            res[s].append((nt[s], rbsp[s], rec[s], qps[s]))
    assert g.status() == [0] * S
    q = g.quality(T)  # QUALITY turns the measurement on by itself
    assert q.sse.shape == (T, S, 3)
    for s in range(S):
        tgt, ipo, step, lo, hi, q0 = QSET[s]
        m = QualityModel(26)
        m.set_rate(QUALITY, q0, qp_min=lo, qp_max=hi, max_step=step, ip_offset=ipo, target_sse=tgt)
        want = []
        for t, (nt, rb, rec, _) in enumerate(res[s]):
            if s == sw[0] and t == sw[1]:
                m.set_rate(CQP, 22)
            if s == sw[0] and t == sw[2]:
                m.set_rate(QUALITY, q0, qp_min=lo, qp_max=hi, max_step=step, ip_offset=ipo, target_sse=tgt)
            want.append(m.pick(I if nt == IDR else P))
            assert q.sse[t, s, 0] == plane_sse(frames[t, s], rec, W, H)[0], f"stream {s} picture {t}: luma sse"
            m.coded(q.sse[t, s, 0])
        got = [p[3] for p in res[s]]
        assert got == want, f"stream {s}: device QPs {got} != model {want}"
        assert list(q.qp[:, s]) == got
        assert len(set(got)) > 1, f"stream {s}: the controller never moved"
        ora, _ = _oracle_pictures(fo, frames[:, s], got, W, H, intra_every=IE)
        _check_pictures(res[s], QSET[s][5], ora, f"stream {s}")
    g.close()


@pytest.mark.parametrize("W,H", [(352, 288), (1280, 720)])
def test_quality_accuracy(pkg, W, H):
    """Targets = the mean luma SSE of the P pictures of constant-QP runs at 16, 24 and 32; QUALITY from QP 26.  Over the
    P pictures after the first GOP the mean achieved SSE / target lies in [0.7, 1.4], the mean QP is at least the constant
    QP - 2 and at most the constant QP + 8, and a larger target never gets a smaller mean QP.  (The upper bound is not 2:
    at QP 32 the P pictures' distortion follows their reference, and QUALITY codes the IDR pictures finer than CQP does, so
    it holds the same SSE at P QPs up to 8 higher -- DESIGN.md section 6.)"""
    IE = 10
    T, S = 3 * IE, 3
    cqp = (16, 24, 32)
    frames = np.stack([np.stack([pkg.gen_frame(W, H, t, 4242, 2)] * S) for t in range(T)])
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=IE)
    g.set_quality(SSE)
    for s, qc in enumerate(cqp):
        g.set_rate(s, CQP, qp=qc)
    cq = _encode_by_picture(g, frames)
    qc = g.quality(T)
    g.close()
    isP = np.array([p[0] == SLICE for p in cq[0]])
    targets = [int(qc.sse[isP, s, 0].mean()) for s in range(S)]
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=IE)
    for s in range(S):
        g.set_rate(s, QUALITY, qp=26, qp_min=0, qp_max=51, max_step=2, ip_offset=3, target_sse=targets[s])
    qa = _encode_by_picture(g, frames)
    assert g.status() == [0] * S
    q = g.quality(T)
    g.close()
    rows = []
    for s in range(S):
        sel = [t for t in range(IE, T) if qa[s][t][0] == SLICE]
        ratio = float(q.sse[sel, s, 0].mean()) / targets[s]
        mq = float(np.mean([qa[s][t][3] for t in sel]))
        rows.append((cqp[s], targets[s], ratio, mq, [p[3] for p in qa[s]]))
    print("\nQUALITY accuracy %dx%d:" % (W, H), *["cqp %d target %d achieved/target %.3f mean qp %.2f qps %s" % r
                                                 for r in rows], sep="\n  ")
    for c, _, ratio, mq, _ in rows:
        assert 0.7 <= ratio <= 1.4, rows
        assert c - 2 <= mq <= c + 8, rows
    mqs = [r[3] for r in sorted(rows, key=lambda r: r[1])]
    assert all(a <= b for a, b in zip(mqs, mqs[1:])), rows
