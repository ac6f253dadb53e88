"""Deterministic HARD 4:2:0 source pictures: saturated, directional and chroma-rich (integer-only numpy).

synth.gen_frame() is smooth: ramps, a +-12 texture, chroma ramps.  On it the encoder hardly ever chooses Intra4x4, never a
directional Intra16x16 mode, never codes a chroma residual in a P macroblock and never clips.  mosaic() is the opposite: a
patchwork of tiles, every one built so that one prediction mode, one CBP pattern or one clip wins.

Numbers.  Everything is drawn from the project's LCG (synth._lcg), never from numpy.random:

  lcg(s)   = s*6364136223846793005 + 1442695040888963407 (mod 2^64)
  mix(z)   = z = lcg(z); z ^= z >> 29; z = lcg(z); return z >> 33          (the noise hash of synth.gen_frame)
  chain    : state s0 = lcg(seed ^ 0x9E3779B97F4A7C15); every tile takes one key: s = lcg(s), key = s
  u(key, i, m) = mix(key + i) % m                                           (draw i of a tile, uniform in [0, m))

Planes.  Luma is tiled by 16x16 tiles in raster order, then Cb by 8x8 tiles, then Cr by 8x8 tiles; the three planes share the
one chain, so chroma tiles are chosen independently of luma.  A tile of side T at key k has kind KINDS[u(k, 0, len(KINDS))]
and, with x, y in [0, T):

  cols     v[y][x] = u(k, 1 + x, 256)                                  columns constant: vertical prediction wins
  rows     v[y][x] = u(k, 1 + y, 256)                                  rows constant: horizontal prediction wins
  diag_dl  v[y][x] = u(k, 1 + x + y, 256)                              constant along down-left diagonals
  diag_dr  v[y][x] = u(k, 1 + x - y + T - 1, 256)                      constant along down-right diagonals
  sat      v[y][x] = clip(0, 255, (0, 3, 252, 255)[u(k, 1, 4)] + u(k, 2 + y*T + x, 13) - 6)
  noise    v[y][x] = u(k, 1 + y*T + x, 256)
  patch    every 4x4 block b (raster, b in [0, (T/4)^2)) is a tile of side 4 of its own with key k + 64*(b + 1) and kind
           (cols, rows, diag_dl, diag_dr, const)[u(key, 0, 5)]
  ramp     v[y][x] = clip(0, 255, u(k, 1, 256) + (u(k, 2, 17) - 8) * x + (u(k, 3, 17) - 8) * y)
  const    v[y][x] = u(s0, 1 + plane, 256), plane = 0, 1, 2 for Y, Cb, Cr: one value per plane for all its const tiles

KINDS lists `const` three times, all const tiles of a plane share their value, and a Cr tile is const wherever the Cb tile at
its place is (it still takes its key from the chain; elsewhere its kind is drawn like any other).  The encoder derives the
chroma prediction mode from the best Intra16x16 luma mode, so a macroblock codes no chroma at all (cbpC 0) only where both its
chroma tiles AND those of the neighbours that mode reads are constant and equal; with other neighbours it codes a DC only
(cbpC 1); the other kinds nearly always give cbpC 2.

shift = (dx, dy), both even: the finished luma plane is rolled by dx samples to the right and dy down (numpy.roll, wrapping),
the chroma planes by dx/2 and dy/2.  sequence() is the four-picture test sequence: the base picture, two shifted ones and the
last of them again (P_Skip runs, also at the end of the slice); it is meant to be coded IDR, P, P, P with EXPLICIT picture
types, since every shifted mosaic exceeds the scene-cut threshold of selectNALUnitType.
"""
import numpy as np
from conftest import load_pkg

_lcg = load_pkg().synth._lcg
_G = np.uint64(0x9E3779B97F4A7C15)
KINDS = ("cols", "rows", "diag_dl", "diag_dr", "sat", "noise", "patch", "ramp", "const", "const", "const")
PATCH_KINDS = ("cols", "rows", "diag_dl", "diag_dr", "const")
SHIFTS = ((0, 0), (2, -2), (6, 2), (6, 2))


def _u64(v):
    return np.uint64(int(v) & ((1 << 64) - 1))


def _mix(z):
    with np.errstate(over="ignore"):
        z = _lcg(z)
        z = z ^ (z >> np.uint64(29))
        z = _lcg(z)
    return z >> np.uint64(33)


def _u(key, i, m):
    """draws i (an integer array or scalar) of the tile with this key, uniform in [0, m) -> int64"""
    with np.errstate(over="ignore"):
        z = key + np.asarray(i, np.int64).astype(np.uint64)
    return (_mix(z) % np.uint64(m)).astype(np.int64)


def _kind(key, kinds=KINDS):
    return kinds[int(_u(key, 0, len(kinds)))]


def _tile(key, T, flat, kind):
    y, x = np.mgrid[0:T, 0:T].astype(np.int64)
    if kind == "cols":
        return _u(key, 1 + x, 256)
    if kind == "rows":
        return _u(key, 1 + y, 256)
    if kind == "diag_dl":
        return _u(key, 1 + x + y, 256)
    if kind == "diag_dr":
        return _u(key, 1 + x - y + T - 1, 256)
    if kind == "sat":
        return np.clip((0, 3, 252, 255)[int(_u(key, 1, 4))] + _u(key, 2 + y * T + x, 13) - 6, 0, 255)
    if kind == "noise":
        return _u(key, 1 + y * T + x, 256)
    if kind == "patch":
        v = np.empty((T, T), np.int64)
        n = T // 4
        for b in range(n * n):
            with np.errstate(over="ignore"):
                kb = key + np.uint64(64 * (b + 1))
            v[(b // n) * 4:(b // n) * 4 + 4, (b % n) * 4:(b % n) * 4 + 4] = _tile(kb, 4, flat, _kind(kb, PATCH_KINDS))
        return v
    if kind == "ramp":
        return np.clip(_u(key, 1, 256) + (_u(key, 2, 17) - 8) * x + (_u(key, 3, 17) - 8) * y, 0, 255)
    return np.full((T, T), flat, np.int64)


_base_cache = {}


def _base(W, H, seed):
    if (W, H, seed) not in _base_cache:
        with np.errstate(over="ignore"):
            s = _lcg(_u64(seed) ^ _G)
        s0 = s
        planes, cb_const = [], set()
        for plane, (pw, ph, T) in enumerate(((W, H, 16), (W // 2, H // 2, 8), (W // 2, H // 2, 8))):
            flat = int(_u(s0, 1 + plane, 256))
            p = np.empty((ph, pw), np.uint8)
            for ty in range(ph // T):
                for tx in range(pw // T):
                    with np.errstate(over="ignore"):
                        s = _lcg(s)
                    kind = "const" if plane == 2 and (tx, ty) in cb_const else _kind(s)
                    if plane == 1 and kind == "const":
                        cb_const.add((tx, ty))
                    p[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T] = _tile(s, T, flat, kind)
            planes.append(p)
        _base_cache[(W, H, seed)] = planes
    return _base_cache[(W, H, seed)]


def mosaic(W, H, seed, shift=(0, 0)):
    """One I420 picture (W*H*3/2 bytes); W and H multiples of 16, shift = (dx, dy) in luma samples, both even."""
    dx, dy = shift
    assert W % 16 == 0 and H % 16 == 0 and dx % 2 == 0 and dy % 2 == 0
    Y, U, V = _base(W, H, seed)
    return np.concatenate([np.roll(Y, (dy, dx), (0, 1)).ravel(), np.roll(U, (dy // 2, dx // 2), (0, 1)).ravel(),
                           np.roll(V, (dy // 2, dx // 2), (0, 1)).ravel()])


def sequence(W, H, seed):
    """[4][W*H*3/2]: the pictures to be coded IDR, P, P, P"""
    return np.stack([mosaic(W, H, seed, sh) for sh in SHIFTS])


NAL_TYPES = (5, 1, 1, 1)
_run_cache = {}


def oracle_run(fo, W, H, seed, qp, window, planes=False):
    """The oracle over sequence(W, H, seed), picture by picture with explicit types (maxdiff 3) -> list of four dicts:
    rbsp, recon, mb_type, cbp [nmb][2], tc [nmb][24], mv [nmb][4][2], max_level, stats (brojTipova so far), on the I picture
    i4mode [nmb][16] and mbsize [nmb][2]; planes: also interp_sat = (samples at 0, samples at 255) of the 15 fractional planes
    made from this picture's reconstruction.  Computed once per argument set and shared; callers leave it unchanged."""
    key = (W, H, seed, qp, window)
    if key not in _run_cache or (planes and "interp_sat" not in _run_cache[key][0]):
        _run_cache[key] = oracle_run_frames(fo, W, H, sequence(W, H, seed), qp, window, planes)
    return _run_cache[key]


def oracle_run_frames(fo, W, H, frames, qp, window, planes=False):
    """oracle_run's four dicts for any four pictures (coded IDR, P, P, P), not cached"""
    o = fo.Oracle(W, H, qp=qp, window=window, maxdiff=3, intra_every=1000)
    out = []
    for f, nt in zip(frames, NAL_TYPES):
        o.set_frame(f)
        r = dict(rbsp=o.encode_slice(nt))
        r.update(recon=o.frame(), mb_type=o.mb_type(), cbp=o.cbp(), tc=o.tc(), mv=o.mv(), max_level=o.max_level(), stats=o.stats())
        if nt == 5:
            r.update(i4mode=o.i4mode(), mbsize=o.mbsize())
        if planes:
            p = np.stack([o.interp(k) for k in range(1, 16)])
            r["interp_sat"] = (int((p == 0).sum()), int((p == 255).sum()))
        out.append(r)
    o.close()
    return out
