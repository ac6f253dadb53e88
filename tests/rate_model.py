"""Integer model of the device rate controller k_rc_plan (h264-fer_amd/csrc/fer_rate.hip, rule in include/ferhip.h).
A test helper: fed with a stream's picture types and the RBSP lengths the library reported, it must give the QPs the
device chose, exactly."""

P6 = [65536, 73562, 82570, 92682, 104032, 116772]  # round(2^16 * 2^(k/6))
CQP, ABR = 0, 1
P, I = 0, 1


def pow2q16(d):
    e, m = d // 6, d % 6  # floor semantics
    return P6[m] << e if e >= 0 else P6[m] >> -e


def tdiv(a, b):
    """C integer division (truncates toward zero)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def target_clamp(target, err, window):
    return min(max(target - tdiv(err, window), max(target // 8, 1)), 8 * target)


class RateModel:
    """One stream.  set_rate() mirrors ferhip_set_rate, pick(type) the choice for the next picture, coded(nbytes) feeds
    back the RBSP length of the picture just picked."""

    def __init__(self, qp, intra_every):
        self.intra_every = intra_every
        self.mode, self.qp = CQP, qp
        self.qp_min, self.qp_max, self.max_step, self.ip_offset, self.window, self.target = 0, 51, 1, 0, intra_every, 0
        self.err = 0
        self.last_bits, self.last_qp, self.have = [0, 0], [0, 0], [0, 0]
        self.cur_qp = qp
        self.prev_type = P
        self.pending = False
        self.pending_bits = None

    def set_rate(self, mode, qp, qp_min=0, qp_max=51, max_step=2, ip_offset=3, window=0, target_bits=0):
        if mode == ABR and self.mode != ABR:  # entering ABR
            self.err = 0
            self.have = [0, 0]
            self.pending = False
        self.mode, self.qp = mode, qp
        if mode == ABR:
            self.qp_min, self.qp_max, self.max_step, self.ip_offset = qp_min, qp_max, max_step, ip_offset
            self.window = window if window > 0 else self.intra_every
            self.target = target_bits

    def est(self, y, q):
        return (self.last_bits[y] * pow2q16(self.last_qp[y] - q)) >> 16

    def pick(self, y):
        """QP of the next picture of type y (P = 0, I = 1)"""
        if self.pending:
            assert self.pending_bits is not None, "coded() was not called for the last picture"
            b = self.pending_bits
            self.err += b - self.target
            self.last_bits[self.prev_type] = b
            self.last_qp[self.prev_type] = self.cur_qp
            self.have[self.prev_type] = 1
        q = self.qp
        if self.mode == ABR:
            T = target_clamp(self.target, self.err, self.window)
            if y == P:
                if self.have[P]:
                    q = next((k for k in range(self.qp_min, self.qp_max + 1) if self.est(P, k) <= T), self.qp_max)
                    q = min(max(q, self.last_qp[P] - self.max_step), self.last_qp[P] + self.max_step)
                elif self.have[I]:
                    q = self.last_qp[I] + self.ip_offset
            else:
                if self.have[P]:
                    q = self.last_qp[P] - self.ip_offset
                elif self.have[I]:
                    q = self.last_qp[I]
            q = min(max(q, self.qp_min), self.qp_max)
        self.pending = self.mode == ABR
        self.pending_bits = None
        self.prev_type = y
        self.cur_qp = q
        return q

    def coded(self, nbytes):
        self.pending_bits = 8 * int(nbytes)
