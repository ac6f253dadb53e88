"""tests/csc_model.py, the numpy yardstick of the packed picture formats (tests/test_gpu_csc.py), pinned against a
pixel-serial transcription of the definition in include/ferhip.h, against known answers and against itself.  No GPU."""
import itertools

import numpy as np
import pytest

import csc_model as csc

FMT_ID = {csc.YUY2: "yuy2", csc.UYVY: "uyvy", csc.BGRA: "bgra", csc.RGBA: "rgba"}
MAT_ID = {csc.BT601: "bt601", csc.BT709: "bt709"}


# ---------------------------------------------------------------- the definition, one pixel at a time
def _byte_pos(fmt):
    """positions in a pixel pair's (4:2:2) or a pixel's (RGB) four bytes"""
    return {csc.YUY2: dict(y0=0, cb=1, y1=2, cr=3), csc.UYVY: dict(cb=0, y0=1, cr=2, y1=3),
            csc.BGRA: dict(b=0, g=1, r=2, a=3), csc.RGBA: dict(r=0, g=1, b=2, a=3)}[fmt]


def serial_in(buf, off, pitch, fmt, matrix, dw, dh):
    buf = [int(v) for v in buf]
    pos = _byte_pos(fmt)
    Y = [[0] * dw for _ in range(dh)]
    Cb = [[0] * (dw // 2) for _ in range(dh // 2)]
    Cr = [[0] * (dw // 2) for _ in range(dh // 2)]
    if fmt in (csc.YUY2, csc.UYVY):
        def at(p, y, name):
            return buf[off + y * pitch + 4 * p + pos[name]]
        for y in range(dh):
            for x in range(dw):
                Y[y][x] = at(x // 2, y, "y1" if x & 1 else "y0")
        for q in range(dh // 2):
            for p in range(dw // 2):
                Cb[q][p] = (at(p, 2 * q, "cb") + at(p, 2 * q + 1, "cb") + 1) >> 1
                Cr[q][p] = (at(p, 2 * q, "cr") + at(p, 2 * q + 1, "cr") + 1) >> 1
    else:
        yr, yg, yb, br, bg, bb, rr, rg, rb = csc.FWD[matrix]

        def at(x, y, name):
            return buf[off + y * pitch + 4 * x + pos[name]]
        for y in range(dh):
            for x in range(dw):
                Y[y][x] = 16 + ((yr * at(x, y, "r") + yg * at(x, y, "g") + yb * at(x, y, "b") + 128) >> 8)
        for q in range(dh // 2):
            for p in range(dw // 2):
                Rs, Gs, Bs = (sum(at(2 * p + i, 2 * q + k, n) for i in (0, 1) for k in (0, 1)) for n in "rgb")
                Cb[q][p] = 128 + ((br * Rs + bg * Gs + bb * Bs + 512) >> 10)
                Cr[q][p] = 128 + ((rr * Rs + rg * Gs + rb * Bs + 512) >> 10)
    return [v for rows in (Y, Cb, Cr) for row in rows for v in row]


def serial_out(buf, off, pitch, fmt, matrix, frame, dw, dh):
    out = [int(v) for v in buf]
    f = [int(v) for v in frame]
    pos = _byte_pos(fmt)

    def Y(x, y):
        return f[y * dw + x]

    def Cb(p, q):
        return f[dw * dh + q * (dw // 2) + p]

    def Cr(p, q):
        return f[dw * dh * 5 // 4 + q * (dw // 2) + p]

    def clip(v):
        return 0 if v < 0 else 255 if v > 255 else v
    for y in range(dh):
        for x in range(dw):
            if fmt in (csc.YUY2, csc.UYVY):
                o = off + y * pitch + 4 * (x // 2)
                out[o + pos["y1" if x & 1 else "y0"]] = Y(x, y)
                out[o + pos["cb"]] = Cb(x // 2, y // 2)
                out[o + pos["cr"]] = Cr(x // 2, y // 2)
            else:
                rv, gu, gv, bu = csc.INV[matrix]
                c, d, e = Y(x, y) - 16, Cb(x >> 1, y >> 1) - 128, Cr(x >> 1, y >> 1) - 128
                o = off + y * pitch + 4 * x
                out[o + pos["r"]] = clip((298 * c + rv * e + 128) >> 8)
                out[o + pos["g"]] = clip((298 * c + gu * d + gv * e + 128) >> 8)
                out[o + pos["b"]] = clip((298 * c + bu * d + 128) >> 8)
                out[o + pos["a"]] = 255
    return out


@pytest.mark.parametrize("matrix", [csc.BT601, csc.BT709], ids=MAT_ID.get)
@pytest.mark.parametrize("fmt", csc.FMTS, ids=FMT_ID.get)
@pytest.mark.parametrize("dw,dh", [(6, 4), (16, 6)])
def test_model_is_the_definition(dw, dh, fmt, matrix):
    rng = np.random.default_rng(dw * 31 + fmt * 3 + matrix)
    rowb = csc.row_bytes(fmt, dw)
    pitch, off = rowb + 8, 12
    n = off + pitch * dh + 5
    buf = rng.integers(0, 256, n, dtype=np.uint8)
    pics = [None, [(0, off, pitch)]]
    got = csc.to_i420([buf], pics, fmt, matrix, dw, dh)
    assert got[0] is None
    assert got[1].tolist() == serial_in(buf, off, pitch, fmt, matrix, dw, dh)
    frame = rng.integers(0, 256, dw * dh * 3 // 2, dtype=np.uint8)  # any bytes: the way out clips
    out = csc.from_i420([buf], pics, fmt, matrix, [None, frame], dw, dh)
    assert out[0].tolist() == serial_out(buf, off, pitch, fmt, matrix, frame, dw, dh)
    touched = np.zeros(n, bool)
    for y in range(dh):
        touched[off + y * pitch:off + y * pitch + rowb] = True
    assert np.array_equal(out[0][~touched], buf[~touched])  # rows are written, everything else is as it was


# ---------------------------------------------------------------- known answers and ranges
KNOWN = {csc.BT601: {(255, 255, 255): (235, 128, 128), (0, 0, 0): (16, 128, 128), (255, 0, 0): (82, 90, 240),
                     (0, 255, 0): (144, 54, 34), (0, 0, 255): (41, 240, 110)},
         csc.BT709: {(255, 0, 0): (63, 102, 240), (0, 255, 0): (172, 42, 26), (0, 0, 255): (32, 240, 118)}}


@pytest.mark.parametrize("fmt", [csc.BGRA, csc.RGBA], ids=FMT_ID.get)
@pytest.mark.parametrize("matrix", [csc.BT601, csc.BT709], ids=MAT_ID.get)
def test_known_answers(matrix, fmt):
    for (r, g, b), want in KNOWN[matrix].items():
        px = [b, g, r, 7] if fmt == csc.BGRA else [r, g, b, 7]  # A is ignored
        buf = np.array(px * 4, np.uint8)  # 2 x 2 pixels of the colour
        got = csc.to_i420([buf], [[(0, 0, 8)]], fmt, matrix, 2, 2)[0]
        assert got.tolist() == [want[0]] * 4 + [want[1], want[2]], (r, g, b)


@pytest.mark.parametrize("matrix", [csc.BT601, csc.BT709], ids=MAT_ID.get)
def test_ranges_need_no_clamp(matrix):
    yr, yg, yb, br, bg, bb, rr, rg, rb = csc.FWD[matrix]
    v = np.arange(256, dtype=np.int32)
    Y = 16 + ((yr * v[:, None, None] + yg * v[None, :, None] + yb * v[None, None, :] + 128) >> 8)  # all 2^24 colours
    assert Y.min() == 16 and Y.max() == 235
    # chroma is monotone in each sum, so the corners of the cube of sums (0 or 4 * 255 each) bound it
    corners = np.array(list(itertools.product((0, 1020), repeat=3)), np.int64)
    rng = np.random.default_rng(5)
    sums = np.concatenate([corners, rng.integers(0, 1021, (200000, 3))])
    Cb = 128 + ((br * sums[:, 0] + bg * sums[:, 1] + bb * sums[:, 2] + 512) >> 10)
    Cr = 128 + ((rr * sums[:, 0] + rg * sums[:, 1] + rb * sums[:, 2] + 512) >> 10)
    assert Cb[:8].min() == 16 and Cb[:8].max() == 240 and Cr[:8].min() == 16 and Cr[:8].max() == 240
    assert Cb.min() == 16 and Cb.max() == 240 and Cr.min() == 16 and Cr.max() == 240
    # the model's own function over whole pictures of random colours
    R, G, B = rng.integers(0, 256, (3, 64, 64))
    y, cb, cr = csc.rgb_to_yuv(R, G, B, matrix)
    assert 16 <= y.min() and y.max() <= 235 and 16 <= min(cb.min(), cr.min()) and max(cb.max(), cr.max()) <= 240


# ---------------------------------------------------------------- 4:2:2 out, then in, is the identity
@pytest.mark.parametrize("fmt", [csc.YUY2, csc.UYVY], ids=FMT_ID.get)
@pytest.mark.parametrize("dw,dh", [(6, 4), (46, 18)])
def test_422_round_trip(dw, dh, fmt):
    rng = np.random.default_rng(dw + fmt)
    frames = rng.integers(0, 256, (2, dw * dh * 3 // 2), dtype=np.uint8)
    pitch = 2 * dw + 4
    bufs = [np.full(2 * pitch * dh + 64, 0xEE, np.uint8)]
    pics = [csc.slot_pic(fmt, pitch, dh, base=16), csc.slot_pic(fmt, pitch, dh, base=16 + csc.slot_bytes(fmt, pitch, dh))]
    out = csc.from_i420(bufs, pics, fmt, csc.BT601, frames, dw, dh)
    back = csc.to_i420(out, pics, fmt, csc.BT709, dw, dh)  # the matrix has no effect on 4:2:2
    for s in range(2):
        assert np.array_equal(back[s], frames[s])


def test_check_refuses():
    dw = 16
    for fmt in csc.FMTS:
        rowb = csc.row_bytes(fmt, dw)
        csc.check([None, [(0, 8, rowb)], [(0, 4, rowb + 4), "ignored", "ignored"]], fmt, dw)
        for bad in [(0, 1, rowb), (0, 2, rowb), (0, 3, rowb), (0, 0, rowb + 1), (0, 0, rowb + 2), (0, 0, rowb - 4)]:
            with pytest.raises(AssertionError):
                csc.check([[bad]], fmt, dw)
    for fmt in (0, 1, 2, 3, 6, 7, 10, -1):  # the planar formats have their own model; the rest are no formats
        with pytest.raises(AssertionError):
            csc.check([None], fmt, dw)
