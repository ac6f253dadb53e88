"""The integer rate-control rule of include/ferhip.h (tests/rate_model.py, the model the GPU tests hold the device
controller k_rc_plan to), on the CPU."""
import math

import pytest
from rate_model import ABR, CQP, I, P, P6, RateModel, pow2q16, target_clamp, tdiv


def test_pow2q16_table_and_floor_semantics():
    for k in range(6):
        assert P6[k] == round(65536 * 2 ** (k / 6))
    for d in range(-60, 61):
        e, m = math.floor(d / 6), d - 6 * math.floor(d / 6)
        want = P6[m] << e if e >= 0 else P6[m] >> -e
        assert pow2q16(d) == want, d
        assert abs(pow2q16(d) / 65536 - 2 ** (d / 6)) <= 2 ** (d / 6) * 1e-4 + 2 / 65536, d
    assert pow2q16(-1) == 58386 and pow2q16(-6) == 32768 and pow2q16(-7) == 29193 and pow2q16(6) == 131072


def test_target_clamp():
    assert tdiv(-7, 2) == -3 and tdiv(7, -2) == -3 and tdiv(7, 2) == 3
    assert target_clamp(8000, 0, 30) == 8000
    assert target_clamp(8000, 3000, 30) == 7900
    assert target_clamp(8000, -3001, 30) == 8100           # truncation toward zero: -3001 / 30 = -100
    assert target_clamp(8000, 10 ** 9, 30) == 1000         # target / 8
    assert target_clamp(8000, -10 ** 9, 30) == 64000       # 8 * target
    assert target_clamp(5, 10 ** 6, 10) == 1               # at least one bit


def test_stream_that_follows_the_estimate_converges():
    """Bits that scale exactly like the model's estimate: the controller settles on the QP whose estimate meets the target."""
    b0, q0 = 400000, 20
    def bits_at(q):
        return (b0 * pow2q16(q0 - q)) >> 16
    target = bits_at(27) + 1
    m = RateModel(q0, 1000)
    m.set_rate(ABR, q0, qp_min=0, qp_max=51, max_step=2, ip_offset=3, window=8, target_bits=target)
    q = m.pick(I)
    m.coded(bits_at(q) // 8)
    seen = []
    for _ in range(40):
        q = m.pick(P)
        m.coded(bits_at(q) // 8)
        seen.append(q)
    assert seen[-10:] == [27] * 10, seen
    # the first P picture only knows the I picture: I QP + ip_offset
    assert seen[0] == q0 + 3


def test_max_step_limits_consecutive_p_pictures():
    m = RateModel(10, 1000)
    m.set_rate(ABR, 10, max_step=2, ip_offset=0, window=4, target_bits=1000)
    m.pick(P)
    m.coded(10 ** 6)  # far over: the estimate asks for a much higher QP
    qs = []
    for _ in range(5):
        qs.append(m.pick(P))
        m.coded(10 ** 6)
    assert qs == [12, 14, 16, 18, 20]
    m2 = RateModel(10, 1000)
    m2.set_rate(ABR, 10, max_step=5, ip_offset=0, window=4, target_bits=1000)
    m2.pick(P)
    m2.coded(10 ** 6)
    assert m2.pick(P) == 15


def test_i_picture_handling_and_entering_abr():
    m = RateModel(30, 10)
    m.set_rate(ABR, 24, qp_min=4, qp_max=40, max_step=3, ip_offset=5, window=0, target_bits=50000)
    assert m.window == 10
    assert m.pick(I) == 24             # nothing known: r.qp
    m.coded(20000)
    assert m.pick(I) == 24             # only an I picture known: its QP
    m.coded(20000)
    q = m.pick(P)
    assert q == 29                     # I QP + ip_offset
    m.coded(4000)
    qp_p = m.pick(P)
    m.coded(4000)
    assert m.pick(I) == max(qp_p - 5, 4)  # last P QP - ip_offset
    # the I picture's excess lands in err, which later P pictures pay back
    m.coded(200000)
    err_before = m.err
    m.pick(P)
    assert m.err == err_before + 8 * 200000 - 50000
    # qp_min / qp_max clamp everything
    m2 = RateModel(30, 10)
    m2.set_rate(ABR, 50, qp_min=10, qp_max=20, target_bits=1000)
    assert m2.pick(I) == 20
    # leaving for CQP and coming back clears err and have[]
    m.set_rate(CQP, 33)
    m.coded(1000)
    assert m.pick(P) == 33
    m.coded(1000)
    m.set_rate(ABR, 22, target_bits=50000)
    assert m.err == 0 and m.have == [0, 0]
    assert m.pick(P) == 22
    # ABR -> ABR keeps the state
    m.coded(500)
    m.pick(P)
    have = list(m.have)
    m.set_rate(ABR, 22, target_bits=60000)
    assert m.have == have


@pytest.mark.parametrize("target", [20000, 50000, 150000])
def test_err_is_bounded_for_a_well_behaved_stream(target):
    """Bits proportional to 2^(-q/6) with I pictures 4x dearer, first QP 3 off the QP that meets the target on P pictures:
    the mean over the later GOPs is near the target."""
    def bits(q, y):
        return int(3.0e6 * 2 ** (-q / 6) * (4 if y == I else 1))
    q0 = round(6 * math.log2(3.0e6 / target)) - 3
    m = RateModel(q0, 10)
    m.set_rate(ABR, q0, qp_min=0, qp_max=51, max_step=2, ip_offset=3, window=0, target_bits=target)
    got = []
    for t in range(60):
        y = I if t % 10 == 0 else P
        q = m.pick(y)
        b = bits(q, y) // 8
        m.coded(b)
        if t >= 10:
            got.append(8 * b)
    mean = sum(got) / len(got)
    assert 0.8 * target <= mean <= 1.25 * target, (mean, target)
