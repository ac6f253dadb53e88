"""The encoder's block arithmetic in 64 bits: a numpy int64 model of the forward core, quantisationResidualBlock, the luma DC and
chroma DC quantisers and the four inverses (oracle/fo_transform.c, F/quantizationTransform.cpp, F/scaleTransform.cpp), written to
answer one question the 32-bit code cannot answer about itself: does any intermediate leave int32?

Every function takes [n][16] (raster 4x4; the chroma DC functions use slots 0..3 as a raster 2x2) and returns the result in
int64.  With a Track given, every intermediate is reported to it: Track.peak is the largest magnitude seen, Track.product the
largest quantiser / dequantiser product (value * LevelQuantize or value * LevelScale, before the rounding shift).  Shifts are
arithmetic and products are exact in int64, so wherever Track.peak < 2^31 the model IS the int32 computation.
"""
import numpy as np

V = ((10, 16, 13), (11, 18, 14), (13, 20, 16), (14, 23, 18), (16, 25, 20), (18, 29, 23))   # normAdjust4x4 v[m][class]
INT32 = (1 << 31) - 1
INT16 = (1 << 15) - 1
DC_MIN, DC_MAX = -255 * 64 - 32, 255 * 64 - 32   # the unquantised DC of a flat residual block of -255 / +255


def level_scale(m):
    """[16] raster: 16 * v[m][class of (i, j)]"""
    i, j = np.divmod(np.arange(16), 4)
    cls = np.where((i % 2 == 0) & (j % 2 == 0), 0, np.where((i % 2 == 1) & (j % 2 == 1), 1, 2))
    return 16 * np.array(V[m], np.int64)[cls]


def level_quantize(m):
    """round(32768 / LevelScale)"""
    ls = level_scale(m)
    return (2 * 32768 + ls) // (2 * ls)


class Track:
    def __init__(self):
        self.peak = 0
        self.product = 0

    def see(self, *arrays):
        for a in arrays:
            if a.size:
                self.peak = max(self.peak, int(np.abs(a).max()))

    def prod(self, a):
        self.see(a)
        if a.size:
            self.product = max(self.product, int(np.abs(a).max()))
        return a


class _NoTrack(Track):
    def see(self, *arrays):
        pass

    def prod(self, a):
        return a


def _blocks(a):
    return np.asarray(a, np.int64).reshape(-1, 4, 4)


_K = np.array([[256, 256, 256, 256], [416, 208, -208, -416], [256, -256, -256, 256], [208, -416, 416, -208]], np.int64)


def forward_core(r, tr=None):
    tr = tr or _NoTrack()
    r = _blocks(r)
    h = np.where(r == 0, 0, r * 64 - 32)
    s = np.einsum("ki,nij->nkj", _K, h)          # vertical: f[k][j] = sum_i K[k][i] h[i][j]
    tr.see(h, s, s + 512)
    f = (s + 512) >> 10
    s = np.einsum("nij,kj->nik", f, _K)          # horizontal: d[i][k] = sum_j K[k][j] f[i][j]
    tr.see(f, s, s + 512)
    return ((s + 512) >> 10).reshape(-1, 16)


def quant_residual(d, qp, keep_dc=False, tr=None):
    tr = tr or _NoTrack()
    d = np.asarray(d, np.int64).reshape(-1, 16)
    q6, lq = qp // 6, level_quantize(qp % 6)
    if qp < 24:
        s = d * (1 << (4 - q6)) - (1 << (3 - q6))
    else:
        s = d >> (q6 - 4)
    t = tr.prod(s * lq)
    tr.see(s, t + 16384)
    c = (t + 16384) >> 15
    if keep_dc:
        c[:, 0] = d[:, 0]
    return c


def forward_residual(r, qp, keep_dc=False, tr=None):
    return quant_residual(forward_core(r, tr), qp, keep_dc, tr)


def forward_dc_luma(f, qp, tr=None):
    tr = tr or _NoTrack()
    f = _blocks(f)
    g = np.stack([f[:, 0] + f[:, 3], f[:, 1] + f[:, 2], f[:, 1] - f[:, 2], f[:, 0] - f[:, 3]], 1)
    e = np.stack([g[:, 0] + g[:, 1], g[:, 3] + g[:, 2], g[:, 0] - g[:, 1], g[:, 3] - g[:, 2]], 1)
    d = np.stack([e[:, :, 0] + e[:, :, 3], e[:, :, 1] + e[:, :, 2], e[:, :, 1] - e[:, :, 2], e[:, :, 0] - e[:, :, 3]], 2)
    u = np.stack([d[:, :, 0] + d[:, :, 1], d[:, :, 3] + d[:, :, 2], d[:, :, 0] - d[:, :, 1], d[:, :, 3] - d[:, :, 2]], 2)
    tr.see(g, e, d, u, u + 8)
    t = ((u + 8) >> 4).reshape(-1, 16)
    q6, ql = qp // 6, int(level_quantize(qp % 6)[0])
    s = t >> (q6 - 6) if qp >= 36 else t * (1 << (6 - q6)) - (1 << (5 - q6))
    v = tr.prod(s * ql)
    tr.see(s, v + 16384)
    return (v + 16384) >> 15


def forward_dc_chroma(f, qp, tr=None):
    tr = tr or _NoTrack()
    f = np.asarray(f, np.int64).reshape(-1, 16)
    d00, d01, d10, d11 = f[:, 0] + f[:, 1], f[:, 0] - f[:, 1], f[:, 2] + f[:, 3], f[:, 2] - f[:, 3]
    u = np.stack([d00 + d10, d01 + d11, d00 - d10, d01 - d11], 1)
    tr.see(u, u + 2)
    t = (u + 2) >> 2
    q6, ql = qp // 6, int(level_quantize(qp % 6)[0])
    v = tr.prod(((t * 32) >> q6) * ql)
    tr.see(t * 32, v + 16384)
    out = np.zeros_like(f)
    out[:, :4] = (v + 16384) >> 15
    return out


def inverse_residual(c, qp, keep_dc=False, tr=None):
    tr = tr or _NoTrack()
    c = np.asarray(c, np.int64).reshape(-1, 16)
    q6, ls = qp // 6, level_scale(qp % 6)
    p = tr.prod(c * ls)
    if qp >= 24:
        d = p * (1 << (q6 - 4))
    else:
        tr.see(p + (1 << (3 - q6)))
        d = (p + (1 << (3 - q6))) >> (4 - q6)
    if keep_dc:
        d[:, 0] = c[:, 0]
    d = d.reshape(-1, 4, 4)
    e = np.stack([d[:, :, 0] + d[:, :, 2], d[:, :, 0] - d[:, :, 2], (d[:, :, 1] >> 1) - d[:, :, 3], d[:, :, 1] + (d[:, :, 3] >> 1)], 2)
    f = np.stack([e[:, :, 0] + e[:, :, 3], e[:, :, 1] + e[:, :, 2], e[:, :, 1] - e[:, :, 2], e[:, :, 0] - e[:, :, 3]], 2)
    g = np.stack([f[:, 0] + f[:, 2], f[:, 0] - f[:, 2], (f[:, 1] >> 1) - f[:, 3], f[:, 1] + (f[:, 3] >> 1)], 1)
    h = np.stack([g[:, 0] + g[:, 3], g[:, 1] + g[:, 2], g[:, 1] - g[:, 2], g[:, 0] - g[:, 3]], 1)
    tr.see(d, e, f, g, h, h + 32)
    return ((h + 32) >> 6).reshape(-1, 16)


def inverse_dc_luma(c, qp, tr=None):
    tr = tr or _NoTrack()
    c = _blocks(c)
    d = np.stack([c[:, :, 0] + c[:, :, 2], c[:, :, 0] - c[:, :, 2], c[:, :, 1] - c[:, :, 3], c[:, :, 1] + c[:, :, 3]], 2)
    e = np.stack([d[:, :, 0] + d[:, :, 3], d[:, :, 1] + d[:, :, 2], d[:, :, 1] - d[:, :, 2], d[:, :, 0] - d[:, :, 3]], 2)
    g = np.stack([e[:, 0] + e[:, 2], e[:, 0] - e[:, 2], e[:, 1] - e[:, 3], e[:, 1] + e[:, 3]], 1)
    f = np.stack([g[:, 0] + g[:, 3], g[:, 1] + g[:, 2], g[:, 1] - g[:, 2], g[:, 0] - g[:, 3]], 1).reshape(-1, 16)
    tr.see(d, e, g, f)
    q6, ls = qp // 6, int(level_scale(qp % 6)[0])
    p = tr.prod(f * ls)
    if qp >= 36:
        out = p * (1 << (q6 - 6))
    else:
        tr.see(p + (1 << (5 - q6)))
        out = (p + (1 << (5 - q6))) >> (6 - q6)
    tr.see(out)
    return out


def inverse_dc_chroma(c, qp, tr=None):
    tr = tr or _NoTrack()
    c = np.asarray(c, np.int64).reshape(-1, 16)
    d00, d01, d10, d11 = c[:, 0] + c[:, 2], c[:, 1] + c[:, 3], c[:, 0] - c[:, 2], c[:, 1] - c[:, 3]
    f = np.stack([d00 + d01, d00 - d01, d10 + d11, d10 - d11], 1)
    p = tr.prod(f * int(level_scale(qp % 6)[0]))
    s = p * (1 << (qp // 6))
    tr.see(f, s)
    out = np.zeros_like(c)
    out[:, :4] = s >> 5
    return out


# ---------------------------------------------------------------- the block KAT inputs (shared with test_gpu_qp_sweep.py)
def extreme_sign_patterns():
    """[32][16]: for each of the 16 coefficients the +-255 block that maximises it, and its negative.  The forward core is two
    separable passes with the rows of _K, so coefficient (k, l) is largest where sample (i, j) has the sign of K[k][i] * K[l][j]."""
    out = []
    for k in range(4):
        for l in range(4):
            s = np.sign(np.outer(_K[k], _K[l])).astype(np.int64) * 255
            out += [s.ravel(), -s.ravel()]
    return np.stack(out)


def forward_inputs():
    """the forward KAT blocks [n][16] int32: the 32 extreme sign patterns, impulses +-1 and +-255 at each position, flat blocks
    0, +-1, +-2, +-255, and 256 random full-range blocks"""
    imp = np.concatenate([np.eye(16, dtype=np.int64) * v for v in (1, -1, 255, -255)])
    flat = np.stack([np.full(16, v, np.int64) for v in (0, 1, -1, 2, -2, 255, -255)])
    rnd = np.random.default_rng(52).integers(-255, 256, (256, 16))
    return np.concatenate([extreme_sign_patterns(), imp, flat, rnd]).astype(np.int32)


def dc_inputs(qp, keep_dc_out):
    """DC blocks for the luma / chroma DC quantisers [n][16] int32, built from the forward outputs with keep_dc (whose slot 0 is
    the unquantised DC): sixteen DCs of consecutive blocks per record, plus the all-equal extremes.  The forward core maps a
    flat residual r != 0 to the DC 64 r - 32, so 8-bit input gives DCs in [-16352, 16288]; +-16320 = 64 * 255 is there as well."""
    dc = np.asarray(keep_dc_out)[:, 0]
    dc = dc[:dc.size // 16 * 16].reshape(-1, 16)
    ext = np.stack([np.full(16, v) for v in (DC_MIN, DC_MAX, 16320, -16320, 0, 1, -1)])
    alt = np.stack([np.where(np.arange(16) % 2 == 0, 16320, -16320), np.where(np.arange(16) // 4 % 2 == 0, 16320, -16320)])
    return np.concatenate([dc, ext, alt]).astype(np.int32)


MODEL = dict(forward_residual=forward_residual, inverse_residual=inverse_residual, forward_dc_luma_intra=forward_dc_luma,
             inverse_dc_luma_intra=inverse_dc_luma, forward_dc_chroma=forward_dc_chroma, inverse_dc_chroma=inverse_dc_chroma)


def kat_cases(qp):
    """The block known-answer inputs of one QP -> list of (operation, keep_dc or None, blocks [n][16] int32), operation a key
    of MODEL (the DC operations carry the names block_op() knows).  Inverse inputs are the model's forward outputs of the same
    blocks plus random levels within the largest level the model reaches at this QP; for keep_dc also blocks whose slot 0 is a
    dequantised luma DC.  The DC operations get DC blocks built from the forward outputs, plus the all-equal extremes."""
    rng = np.random.default_rng(1000 + qp)
    blocks = forward_inputs()
    out = []
    fwd = {}
    for keep in (False, True):
        out.append(("forward_residual", keep, blocks))
        fwd[keep] = forward_residual(blocks, qp, keep)
    dcs = dc_inputs(qp, fwd[True])
    ldc, cdc = forward_dc_luma(dcs, qp), forward_dc_chroma(dcs, qp)
    lmax, cmax = int(np.abs(ldc).max()), int(np.abs(cdc).max())
    inv_l = np.concatenate([ldc, np.full((1, 16), lmax), np.full((1, 16), -lmax), rng.integers(-lmax, lmax + 1, (16, 16))]).astype(np.int32)
    inv_c = np.concatenate([cdc, np.full((1, 16), cmax), np.full((1, 16), -cmax), rng.integers(-cmax, cmax + 1, (16, 16))]).astype(np.int32)
    inv_c[:, 4:] = 0
    out += [("forward_dc_luma_intra", None, dcs), ("forward_dc_chroma", None, dcs), ("inverse_dc_luma_intra", None, inv_l),
            ("inverse_dc_chroma", None, inv_c)]
    m = int(np.abs(fwd[False]).max())
    for keep in (False, True):
        lv = np.concatenate([fwd[keep], rng.integers(-m, m + 1, (128, 16))])
        if keep:
            dq = lv[:min(lv.shape[0], inv_l.size)].copy()
            dq[:, 0] = inverse_dc_luma(inv_l, qp).ravel()[:dq.shape[0]]
            lv = np.concatenate([lv, dq])
        out.append(("inverse_residual", keep, lv.astype(np.int32)))
    return out


def max_levels():
    """per QP (largest |residual level|, largest |luma DC level|, largest |chroma DC level|, largest quantiser product, largest
    intermediate) the model reaches on forward_inputs() and dc_inputs(): [52][5] int64"""
    out = np.zeros((52, 5), np.int64)
    blocks = forward_inputs()
    for qp in range(52):
        tr = Track()
        lv = forward_residual(blocks, qp, False, tr)
        kd = forward_residual(blocks, qp, True, tr)
        dcs = dc_inputs(qp, kd)
        l = forward_dc_luma(dcs, qp, tr)
        c = forward_dc_chroma(dcs, qp, tr)
        out[qp] = (np.abs(lv).max(), np.abs(l).max(), np.abs(c).max(), tr.product, tr.peak)
    return out
