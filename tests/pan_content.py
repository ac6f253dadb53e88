"""Deterministic PANNED 4:2:0 source pictures: one endless textured plane seen through a moving window (integer-only numpy).

synth.gen_frame() moves by (2, 1) samples a picture and hard_content.mosaic() by (6, 2) at the most, so no encoder parity test ever
saw a vector longer than a few samples.  Here the camera pans by tens to hundreds of samples a picture over a texture that has
detail at every scale, so stage 2 of interEncoding finds the moved block far away and the vectors, the predictors and the vector
differences are hundreds of quarter samples long.

Numbers.  Everything is drawn from the project's LCG (synth._lcg) through the mix of hard_content.py, never from numpy.random:

  lcg(s)       = s*6364136223846793005 + 1442695040888963407 (mod 2^64)
  mix(z)       = z = lcg(z); z ^= z >> 29; z = lcg(z); return z >> 33
  s0           = lcg(seed ^ 0x9E3779B97F4A7C15)
  key(p, k)    = lcg(s0 + 8*p + k)                       plane p = 0, 1, 2 for Y, Cb, Cr; scale k = 0..3       (all mod 2^64)
  cell(a, b)   = ((b mod 2^20) << 20) | (a mod 2^20)     a, b: column and row of a cell, possibly negative (two's complement)
  f(p, k, X, Y) = mix(key(p, k) + cell(floor(X / B), floor(Y / B))) % A - (A - 1)/2       with B = BLOCK[p][k], A = AMP[p][k]

Masters.  All three masters live on ONE endless grid at twice the luma resolution in each direction, X to the right, Y down, any
integer, negative included.  Master p at (X, Y) is the clipped sum of four block-constant fields:

  M(p, X, Y)   = clip(1, 255, 128 + f(p, 0, X, Y) + f(p, 1, X, Y) + f(p, 2, X, Y) + f(p, 3, X, Y))

  luma    BLOCK 32, 8, 2, 1 master samples,  AMP 161, 81, 41, 9   (+-80, +-40, +-20, +-4)
  chroma  BLOCK 64, 16, 4, 1 master samples, AMP 97, 49, 25, 9    (+-48, +-24, +-12, +-4): the same detail per chroma sample

Pictures.  The window of a picture sits at the offset (ox, oy), given in master samples = HALF luma samples; odd offsets are
half-sample pans.  A luma sample is the rounded mean of its 2x2 master samples, a chroma sample (which covers 2x2 luma samples) the
rounded mean of its 4x4 master samples, so luma and chroma show the same pan, whatever its parity:

  Y[r][c]      = (sum of M(0, ox + 2c + i, oy + 2r + j) over i, j in 0..1  +  2) >> 2        r < H,   c < W
  Cb[r][c]     = (sum of M(1, ox + 4c + i, oy + 4r + j) over i, j in 0..3  +  8) >> 4        r < H/2, c < W/2      Cr: M(2, ..)

Every master sample lies in 1..255, hence every picture sample too, and no 8x8 luma block can sum to 0.  A window that moves by
(dx, dy) master samples shows content that moves by (-dx/2, -dy/2) luma samples, so a block of the new picture is found in the old
one at the vector (+2dx, +2dy) quarter samples: an odd dx is a half-sample luma vector, and its chroma vector (the same number in
eighth chroma samples) has the phase 2 or 6.

sequence(W, H, seed, offsets) is one picture per offset; the sequences are meant to be coded IDR, P, P, .. with EXPLICIT picture
types, since a pan may exceed the scene-cut threshold of selectNALUnitType.  SEQS names the sequences the tests share; oracle_run()
codes one of them on the oracle, once per argument set.

The module also restates the vector prediction of a P macroblock (fer_mvpred.h, F/mode_pred.cpp:252-371, :381-482) for the
encoder's case -- every macroblock inter, reference index 0, one vector per 8x8 quadrant -- so that the vector differences of a
picture can be derived from the oracle's vectors and types: the oracle keeps mvd for the current macroblock only.
"""
import numpy as np
from conftest import load_pkg

from hard_content import _G, _mix, _u64
from me_model import _core

_lcg = load_pkg().synth._lcg
BLOCK = ((32, 8, 2, 1), (64, 16, 4, 1), (64, 16, 4, 1))
AMP = ((161, 81, 41, 9), (97, 49, 25, 9), (97, 49, 25, 9))


def _key(seed, plane, k):
    with np.errstate(over="ignore"):
        s0 = _lcg(_u64(seed) ^ _G)
        return _lcg(s0 + np.uint64(8 * plane + k))


def master(plane, seed, X0, Y0, w, h):
    """M(plane, X, Y) for X in [X0, X0 + w), Y in [Y0, Y0 + h) -> int64 [h][w]"""
    Y, X = np.mgrid[Y0:Y0 + h, X0:X0 + w].astype(np.int64)
    v = np.full((h, w), 128, np.int64)
    for k, (B, A) in enumerate(zip(BLOCK[plane], AMP[plane])):
        cell = (((Y // B) & 0xFFFFF) << 20) | ((X // B) & 0xFFFFF)
        with np.errstate(over="ignore"):
            z = _key(seed, plane, k) + cell.astype(np.uint64)
        v += (_mix(z) % np.uint64(A)).astype(np.int64) - (A - 1) // 2
    return np.clip(v, 1, 255)


def picture(W, H, seed, offset):
    """One I420 picture (W*H*3/2 bytes) of the window at offset = (ox, oy) in master samples (half luma samples)."""
    ox, oy = offset
    assert W % 2 == 0 and H % 2 == 0
    planes = []
    for plane, n in ((0, 2), (1, 4), (2, 4)):
        m = master(plane, seed, ox, oy, 2 * W, 2 * H)
        pw, ph = 2 * W // n, 2 * H // n
        s = m.reshape(ph, n, pw, n).sum((1, 3))
        planes.append(((s + n * n // 2) // (n * n)).astype(np.uint8).ravel())
    return np.concatenate(planes)


_seq_cache = {}


def sequence(W, H, seed, offsets):
    """[len(offsets)][W*H*3/2]: the pictures to be coded IDR, P, P, ..; computed once and shared, callers leave it unchanged"""
    key = (W, H, seed, tuple(tuple(o) for o in offsets))
    if key not in _seq_cache:
        _seq_cache[key] = np.stack([picture(W, H, seed, o) for o in key[3]])
    return _seq_cache[key]


def pan(*steps):
    """offsets of the pictures of a pan: (0, 0), then one more picture per step = (dx, dy) master samples"""
    out = [(0, 0)]
    for dx, dy in steps:
        out.append((out[-1][0] + dx, out[-1][1] + dy))
    return tuple(out)


# name -> (W, H, seed, offsets in master samples).  "far": every P picture is a long pan.
SEQS = {
    # QCIF, one direction per quadrant: about 40 and 90 luma samples a picture.  Two start with an odd (half-sample) step; every
    # one ends with whole-sample steps, where the predicted vector of a macroblock amid an exact pan is exact too (P_Skip).
    "qcif_se40": (176, 144, 11, pan((81, 47), (80, 48), (80, 48))),
    "qcif_nw40": (176, 144, 12, pan((-80, -56), (-80, -56), (-80, -56))),
    "qcif_ne90": (176, 144, 13, pan((181, -61), (180, -60), (180, -60))),
    "qcif_sw90": (176, 144, 14, pan((-180, 84), (-180, 84), (-180, 84))),
    # near the reach of stage 3 (+-WindowSize/2 = 8 samples at window 16): (7, -5) inside, (17, 0) just outside
    "qcif_near_in": (176, 144, 15, pan((14, -10), (14, -10))),
    "qcif_near_out": (176, 144, 16, pan((34, 0), (34, 0))),
    # still, pan, pan, still: P_Skip runs around long vectors
    "qcif_still_pan": (176, 144, 17, ((0, 0), (0, 0), (100, 60), (200, 120), (200, 120))),
    # larger than the 280-diamond along one axis, pans of 150, 280 and 220 samples along it: a half-sample step, one whose true
    # vector (5 + 280 samples) lies just outside the diamond, a whole-sample step
    "tall": (48, 640, 18, pan((7, 301), (-10, 560), (6, 440))),
    "wide": (640, 48, 19, pan((301, 7), (560, -10), (440, 6))),
    # a pan larger than the picture
    "small": (32, 32, 20, pan((90, 70), (90, 70))),
}
FAR = ("qcif_se40", "qcif_nw40", "qcif_ne90", "qcif_sw90", "tall", "wide")
QUAD = FAR[:4]
NAMED = tuple(SEQS)
# seventeen QCIF streams for one context (the eight ticket queues of k_me_resolve): every stream another pan, up to 83 master samples
# (41 luma samples) a picture in either direction, odd and even steps; streams 5 and 11 stand still
MANY = tuple("many_%02d" % s for s in range(17))
for _s, _n in enumerate(MANY):
    _step = (0, 0) if _s in (5, 11) else ((_s * 59) % 167 - 83, (_s * 101) % 131 - 65)
    SEQS[_n] = (176, 144, 30 + _s, pan(_step, _step))
# the encoder cases of test_gpu_pan.py: (streams of one context, qp, window, maxdiff); test_pan_content_host.py holds the oracle's
# side of every one of them under the level guard and off the sum-0 layout
ENC_CASES = ([(QUAD, 12, w, 3) for w in (16, 32, 48)] + [(QUAD, 12, 16, -1), (QUAD, 28, 16, 3), (QUAD, 28, 32, -1)]
             + [(("qcif_near_in", "qcif_near_out"), 12, w, 3) for w in (16, 32)] + [(("qcif_still_pan",), 12, w, 3) for w in (16, 32)]
             + [((n,), 12, w, 3) for n in ("tall", "wide", "small") for w in (16, 32)] + [(MANY, 12, 16, 3)])
def case_id(case):
    names, qp, window, maxdiff = case
    return "%s_S%d_qp%d_w%d_md%d" % (names[0], len(names), qp, window, maxdiff)


# streams whose non-skip macroblocks all code something: on a macroblock of CBP 0 the reference DECODER re-applies stale chroma AC
# levels (F/residual.cpp:28-49), so only on these does a decoder also give the encoder's reconstruction
DEC_CASES = ("qcif_se40", "qcif_ne90", "tall")


def frames(name):
    W, H, seed, offsets = SEQS[name]
    return sequence(W, H, seed, offsets)


def nal_types(n):
    return (5,) + (1,) * (n - 1)


_run_cache = {}


def oracle_frames(fo, W, H, pics, qp, window, maxdiff=3, record=False):
    """The oracle over the pictures, one by one with explicit types IDR, P, P, .. -> list of dicts: rbsp, recon, mb_type, cbp
    [nmb][2], tc [nmb][24], mv [nmb][4][2], max_level, stats (brojTipova so far); record: on P pictures also me = me_lists()."""
    o = fo.Oracle(W, H, qp=qp, window=window, maxdiff=maxdiff, intra_every=1000)
    if record:
        o.record_me()
    out = []
    for f, nt in zip(pics, nal_types(len(pics))):
        o.set_frame(f)
        r = dict(rbsp=o.encode_slice(nt))
        r.update(recon=o.frame(), mb_type=o.mb_type(), cbp=o.cbp(), tc=o.tc(), mv=o.mv(), max_level=o.max_level(), stats=o.stats())
        if record and nt == 1:
            r["me"] = o.me_lists()
        out.append(r)
    o.close()
    return out


def oracle_run(fo, name, qp=12, window=16, maxdiff=3, record=False):
    """oracle_frames over the named sequence; computed once per argument set and shared, callers leave it unchanged"""
    key = (name, qp, window, maxdiff)
    if key not in _run_cache or (record and not any("me" in r for r in _run_cache[key])):
        W, H, _, _ = SEQS[name]
        _run_cache[key] = oracle_frames(fo, W, H, frames(name), qp, window, maxdiff, record)
    return _run_cache[key]


def oracle_stream(fo, name, qp=12, window=16):
    """the Annex-B stream of oracle_run(name): the oracle's own SPS and PPS, then one slice NAL unit per picture"""
    from nal_model import frame_nal
    W, H, _, _ = SEQS[name]
    o = fo.Oracle(W, H, qp=qp, window=window, maxdiff=3, intra_every=1000)
    head, _ = o.encode_stream(frames(name)[:1])
    o.close()
    sets = b"".join(n for n in load_pkg().split_nals(head) if n[4] & 31 in (7, 8))
    run = oracle_run(fo, name, qp, window)
    return sets + b"".join(frame_nal(nt, r["rbsp"]) for nt, r in zip(nal_types(len(run)), run))


# ---------------------------------------------------------------- vector prediction of a P macroblock (encoder's case)
P_SKIP = 31
# partitions of the inter types: (x, y, w, h, quadrant that carries the vector)
PARTS = {0: ((0, 0, 16, 16, 0),), 1: ((0, 0, 16, 8, 0), (0, 8, 16, 8, 2)), 2: ((0, 0, 8, 16, 0), (8, 0, 8, 16, 1)),
         3: ((0, 0, 8, 8, 0), (8, 0, 8, 8, 1), (0, 8, 8, 8, 2), (8, 8, 8, 8, 3))}
PARTS[4] = PARTS[3]
PARTS[P_SKIP] = PARTS[0]


def _neighbour(mv, mbw, mb, xN, yN):
    """the vector of the quadrant that holds sample (xN, yN) relative to macroblock mb, or None where that sample is outside the
    picture or not coded yet (nbr_locate of fer_mvpred.h)"""
    mbx, mby = mb % mbw, mb // mbw
    if (xN > 15 and yN >= 0) or yN > 15:
        return None
    if xN < 0:
        mbx, xN = mbx - 1, xN + 16
    elif xN > 15:
        mbx, xN = mbx + 1, xN - 16
    if yN < 0:
        mby, yN = mby - 1, yN + 16
    if mbx < 0 or mbx >= mbw or mby < 0:
        return None
    return tuple(int(v) for v in mv[mby * mbw + mbx, (yN >> 3) * 2 + (xN >> 3)])


def predict(mv, mbw, mb, mtype, part):
    """PredictMV_Luma of partition `part` of macroblock mb of type mtype (0 16x16, 1 16x8, 2 8x16, 3 / 4 8x8, 31 the 16x16
    prediction of P_Skip) from mv [nmb][4][2], which holds the final vectors of everything coded before the partition"""
    x, y, w, _, _ = PARTS[mtype][part]
    A, B = _neighbour(mv, mbw, mb, x - 1, y), _neighbour(mv, mbw, mb, x, y - 1)
    C = _neighbour(mv, mbw, mb, x + w, y - 1)
    if C is None:
        C = _neighbour(mv, mbw, mb, x - 1, y - 1)
    if mtype == 1 and part == 0 and B is not None:
        return B
    if ((mtype == 1 and part == 1) or (mtype == 2 and part == 0)) and A is not None:
        return A
    if mtype == 2 and part == 1 and C is not None:
        return C
    return _core(A, B, C)


def skip_vector(mv, mbw, mb):
    """the derived vector of a P_Skip macroblock (F/mode_pred.cpp:381-420)"""
    if mb < mbw or mb % mbw == 0:
        return (0, 0)
    if not mv[mb - mbw, 2].any() or not mv[mb - 1, 1].any():
        return (0, 0)
    return predict(mv, mbw, mb, P_SKIP, 0)


def mvd_of(mv, mb_type, mbw):
    """The vector differences of a P picture from its final vectors and types -> int [nmb][4][2] in the layout of
    FERHIP_BUF_MVD: slot i = partition i of the macroblock's type, the other slots 0; a P_Skip macroblock has none (left 0).
    A partition's neighbours inside its own macroblock are earlier partitions of the same type, whose vectors the quadrant
    storage already holds."""
    out = np.zeros((mb_type.size, 4, 2), np.int64)
    for mb, t in enumerate(int(v) for v in mb_type):
        if t == P_SKIP:
            continue
        for i, (_, _, _, _, q) in enumerate(PARTS[t]):
            px, py = predict(mv, mbw, mb, t, i)
            out[mb, i] = (int(mv[mb, q, 0]) - px, int(mv[mb, q, 1]) - py)
    return out
