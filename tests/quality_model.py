"""Integer model of the QUALITY mode of the device rate controller k_rc_plan (h264-fer_amd/csrc/fer_rate.hip, rule in
include/ferhip.h), and numpy models of the quality measurement of k_quality (fer_quality.hip).  Test helpers: fed with a
stream's picture types and the luma SSE the library reported, QualityModel must give the QPs the device chose, exactly."""
import numpy as np
from rate_model import pow2q16

CQP, ABR, QUALITY = 0, 1, 2
P, I = 0, 1


def est(last_sse, last_qp, q):
    """(last_sse * pow2q16(2 * (q - last_qp))) >> 16 -- Python integers are exact at any width"""
    return (last_sse * pow2q16(2 * (q - last_qp))) >> 16


class QualityModel:
    """One stream.  set_rate() mirrors ferhip_set_rate (CQP and QUALITY), pick(type) the choice for the next picture,
    coded(luma_sse) feeds back the luma SSE of the picture just picked."""

    def __init__(self, qp):
        self.mode, self.qp = CQP, qp
        self.qp_min, self.qp_max, self.max_step, self.ip_offset, self.target = 0, 51, 1, 0, 0
        self.last_sse, self.last_qp, self.have = [0, 0], [0, 0], [0, 0]
        self.cur_qp = qp
        self.prev_type = P
        self.pending = False
        self.pending_sse = None

    def set_rate(self, mode, qp, qp_min=0, qp_max=51, max_step=2, ip_offset=3, target_sse=0):
        assert mode in (CQP, QUALITY)
        if mode == QUALITY and self.mode != QUALITY:  # entering QUALITY
            self.have = [0, 0]
            self.pending = False
        self.mode, self.qp = mode, qp
        if mode == QUALITY:
            self.qp_min, self.qp_max, self.max_step, self.ip_offset = qp_min, qp_max, max_step, ip_offset
            self.target = target_sse

    def pick(self, y):
        """QP of the next picture of type y (P = 0, I = 1)"""
        if self.pending:
            assert self.pending_sse is not None, "coded() was not called for the last picture"
            self.last_sse[self.prev_type] = self.pending_sse
            self.last_qp[self.prev_type] = self.cur_qp
            self.have[self.prev_type] = 1
        q = self.qp
        if self.mode == QUALITY:
            if self.have[y]:
                q = next((k for k in range(self.qp_max, self.qp_min - 1, -1)
                          if est(self.last_sse[y], self.last_qp[y], k) <= self.target), self.qp_min)
                q = min(max(q, self.last_qp[y] - self.max_step), self.last_qp[y] + self.max_step)
            elif self.have[1 - y]:
                q = self.last_qp[1 - y] + (self.ip_offset if y == P else -self.ip_offset)
            q = min(max(q, self.qp_min), self.qp_max)
        self.pending = self.mode == QUALITY
        self.pending_sse = None
        self.prev_type = y
        self.cur_qp = q
        return q

    def coded(self, luma_sse):
        self.pending_sse = int(luma_sse)


def plane_sse(src, rec, W, H):
    """[3] int64 sums of squared differences of one I420 picture pair (Y, Cb, Cr)"""
    a, b = src.astype(np.int64), rec.astype(np.int64)
    ys, cs = W * H, W * H // 4
    cuts = ((0, ys), (ys, ys + cs), (ys + cs, ys + 2 * cs))
    return np.array([int(((a[x:y] - b[x:y]) ** 2).sum()) for x, y in cuts], np.int64)


def ssim_windows(src, rec, W, H):
    """the per-window SSIM values of include/ferhip.h, from int64 window sums -> float64 [(H/4 - 1), (W/4 - 1)]"""
    a = src[:W * H].reshape(H, W).astype(np.int64)
    b = rec[:W * H].reshape(H, W).astype(np.int64)

    def blk(x):  # 4x4 block sums
        return x.reshape(H // 4, 4, W // 4, 4).sum(axis=(1, 3))

    def win(x):  # 2x2 blocks -> 8x8 windows at a 4-sample step
        return x[:-1, :-1] + x[1:, :-1] + x[:-1, 1:] + x[1:, 1:]

    s1, s2 = win(blk(a)), win(blk(b))
    ss, s12 = win(blk(a * a) + blk(b * b)), win(blk(a * b))
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    num = (2 * s1 * s2 + 416) * (2 * covar + 235963)
    den = (s1 * s1 + s2 * s2 + 416) * (vars_ + 235963)
    return num.astype(np.float64) / den.astype(np.float64)
