"""The integer QUALITY rule of include/ferhip.h (tests/quality_model.py, the model the GPU tests hold the device controller
k_rc_plan to) and the numpy SSIM definition, on the CPU."""
import numpy as np
from quality_model import CQP, I, P, QUALITY, QualityModel, est, plane_sse, ssim_windows
from rate_model import pow2q16


def _quality(m, target, qp=26, **kw):
    args = dict(qp_min=0, qp_max=51, max_step=2, ip_offset=3)
    args.update(kw)
    m.set_rate(QUALITY, qp, target_sse=target, **args)


def test_first_pictures_and_type_changes():
    m = QualityModel(20)
    _quality(m, 10 ** 6, qp=26, ip_offset=4)
    assert m.pick(I) == 26                 # nothing known: r->qp
    m.coded(2 * 10 ** 6)
    assert m.pick(P) == 30                 # P after I, no P known: last I QP + ip_offset
    m.coded(10 ** 6)
    assert m.pick(I) == 24                 # I after P: the first I's history (2e6 at 26 -> 23 fits), clamped to 26 - 2
    m = QualityModel(20)
    _quality(m, 10 ** 6, qp=24, ip_offset=4)
    assert m.pick(P) == 24
    m.coded(5 * 10 ** 5)
    assert m.pick(I) == 20                 # I after P, no I known: last P QP - ip_offset


def test_sse_zero_goes_to_the_top_within_the_step():
    m = QualityModel(20)
    _quality(m, 1000, qp=20, max_step=3)
    qs = []
    for _ in range(12):
        qs.append(m.pick(P))
        m.coded(0)
    assert qs == [20, 23, 26, 29, 32, 35, 38, 41, 44, 47, 50, 51]


def test_unreachable_target_gives_qp_min_and_the_clamp_limits_the_fall():
    m = QualityModel(30)
    _quality(m, 10, qp=30, qp_min=12, qp_max=45, max_step=4)
    qs = []
    for _ in range(8):
        qs.append(m.pick(P))
        m.coded(10 ** 9)
    assert qs == [30, 26, 22, 18, 14, 12, 12, 12]


def test_estimate_steers_to_the_target_exactly():
    """A stream whose SSE follows the model exactly (SSE ~ Qstep^2) lands on the largest QP that meets the target."""
    e0, q0 = 3 * 10 ** 7, 22

    def sse_at(q):
        return est(e0, q0, q)

    target = sse_at(29)
    m = QualityModel(q0)
    _quality(m, target, qp=q0, max_step=51)
    q = m.pick(P)
    m.coded(sse_at(q))
    q = m.pick(P)
    assert q == 29
    assert est(e0, q0, 30) > target


def test_max_step_clamp_both_ways():
    m = QualityModel(26)
    _quality(m, 10 ** 12, qp=26, max_step=1)  # any q meets the target: upward by one per picture
    assert m.pick(P) == 26
    m.coded(10 ** 6)
    assert m.pick(P) == 27
    m.coded(10 ** 6)
    assert m.pick(P) == 28


def test_i_and_p_keep_separate_histories():
    m = QualityModel(26)
    _quality(m, 4 * 10 ** 6, qp=26, max_step=51, ip_offset=3)
    seq = []
    for y, e in ((I, 8 * 10 ** 6), (P, 2 * 10 ** 6), (P, 2 * 10 ** 6), (I, 4 * 10 ** 6), (P, 10 ** 6)):
        seq.append(m.pick(y))
        m.coded(e)
    # I: 26 -> (I known: 8e6 at 26) largest q with 8e6 * 2^(2(q-26)/6) <= 4e6 -> q = 23
    # P after I: 26 + 3 = 29; then P known (2e6 at 29): largest q with 2e6 * 2^((q-29)/3) <= 4e6 -> 32
    assert seq[:4] == [26, 29, 32, 23]
    assert est(8 * 10 ** 6, 26, 23) <= 4 * 10 ** 6 < est(8 * 10 ** 6, 26, 24)


def test_switch_to_cqp_and_back_clears_the_history():
    m = QualityModel(26)
    _quality(m, 10 ** 6, qp=30)
    assert m.pick(P) == 30
    m.coded(10)
    m.set_rate(CQP, 18)
    assert m.pick(P) == 18
    m.coded(10 ** 9)
    _quality(m, 10 ** 6, qp=33)
    assert m.pick(P) == 33                 # have[] cleared on entering: r->qp again
    m.coded(10)
    assert m.pick(P) == 35


def test_estimate_is_exact_at_4k_over_51_qp():
    """4K luma SSE at its largest (255^2 per sample) times 2^(102/6): far beyond 64 bits, kept exact."""
    W, H = 3840, 2160
    e = 255 ** 2 * W * H
    assert est(e, 0, 51) == (e * pow2q16(102)) >> 16 == (e * (65536 << 17)) >> 16
    assert e * pow2q16(102) >= 1 << 64
    assert est(e, 51, 0) == 0 and est(e, 51, 50) == (e * pow2q16(-2)) >> 16
    # a target that only the top QP span can meet: the rule picks on the exact value, not a wrapped one
    m = QualityModel(0)
    _quality(m, est(e, 0, 51), qp=0, max_step=51)
    m.pick(P)
    m.coded(e)
    assert m.pick(P) == 51
    m = QualityModel(0)
    _quality(m, est(e, 0, 51) - 1, qp=0, max_step=51)
    m.pick(P)
    m.coded(e)
    assert m.pick(P) == 50


def test_numpy_ssim_model_on_identical_and_known_pictures():
    W, H = 32, 16
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    v = ssim_windows(a, a, W, H)
    assert v.shape == (H // 4 - 1, W // 4 - 1)
    assert np.all(v == 1.0)                # num == den for identical windows
    b = a.copy()
    b[:W * H] = 255 - b[:W * H]
    assert np.all(ssim_windows(a, b, W, H) < 1)
    assert list(plane_sse(a, a, W, H)) == [0, 0, 0]
    c = a.copy()
    c[W * H] ^= 3
    assert list(plane_sse(a, c, W, H)) == [0, (int(a[W * H]) - int(c[W * H])) ** 2, 0]
