"""Model of the packed picture formats (FERHIP_FMT_YUY2, UYVY, BGRA, RGBA of ferhip_set_pictures, ferhip_get_recon_pictures
and ferhip_decs_set_layout), in plain numpy: the integer definition of include/ferhip.h.  Test infrastructure.

A descriptor of the model is None (the stream is absent) or a list whose first entry is (buffer, offset, pitch): row r of
the one plane starts at byte offset + r * pitch of buffers[buffer], a flat uint8 array.  Offsets are taken from the
buffer's start; a test places its buffers at 16-byte boundaries.

  to_i420     descriptors -> the converted tight I420 picture [dw*dh*3/2] of every present stream (what the padding of
              pad_model.pad_picture is then applied to)
  from_i420   tight I420 pictures -> the bytes the buffers must hold afterwards: rows written, everything else as it was
  check       what the library refuses with FERHIP_E_ARG
  slot_bytes  bytes of one output slot of the live decoder in a packed layout
  slot_pic    the descriptor of the slot that starts at `base` of a buffer
"""
import numpy as np

YUY2, UYVY, BGRA, RGBA = 4, 5, 8, 9
BT601, BT709 = 0, 1
FMTS = (YUY2, UYVY, BGRA, RGBA)

# (yr, yg, yb | br, bg, bb | rr, rg, rb) and (rv, gu, gv, bu)
FWD = {BT601: (66, 129, 25, -38, -74, 112, 112, -94, -18), BT709: (47, 157, 16, -26, -86, 112, 112, -102, -10)}
INV = {BT601: (409, -100, -208, 516), BT709: (459, -55, -136, 541)}


def bpp(fmt):
    return 2 if fmt in (YUY2, UYVY) else 4


def row_bytes(fmt, dw):
    return bpp(fmt) * dw


def check(pics, fmt, dw):
    """what ferhip_set_pictures refuses with FERHIP_E_ARG; only the first plane of a descriptor is looked at"""
    assert fmt in FMTS
    for p in pics:
        if p is None:
            continue
        _, off, pitch = p[0]
        assert off % 4 == 0 and pitch % 4 == 0 and pitch >= row_bytes(fmt, dw)


def _rows(buffers, pic, fmt, dw, dh):
    """-> (buffer number, flat indices [dh][row bytes])"""
    buf, off, pitch = pic[0]
    return buf, off + np.arange(dh)[:, None] * pitch + np.arange(row_bytes(fmt, dw))[None, :]


def rgb_to_yuv(R, G, B, matrix):
    """R, G, B: int arrays [dh][dw] -> Y [dh][dw], Cb, Cr [dh/2][dw/2]"""
    yr, yg, yb, br, bg, bb, rr, rg, rb = FWD[matrix]
    R, G, B = (np.asarray(a, np.int64) for a in (R, G, B))
    Y = 16 + ((yr * R + yg * G + yb * B + 128) >> 8)
    Rs, Gs, Bs = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] for a in (R, G, B))
    Cb = 128 + ((br * Rs + bg * Gs + bb * Bs + 512) >> 10)
    Cr = 128 + ((rr * Rs + rg * Gs + rb * Bs + 512) >> 10)
    return Y, Cb, Cr


def yuv_to_rgb(Y, Cb, Cr, matrix):
    """Y [dh][dw], Cb, Cr [dh/2][dw/2] -> R, G, B [dh][dw]; chroma is nearest"""
    rv, gu, gv, bu = INV[matrix]
    c = np.asarray(Y, np.int64) - 16
    d = np.repeat(np.repeat(np.asarray(Cb, np.int64), 2, 0), 2, 1) - 128
    e = np.repeat(np.repeat(np.asarray(Cr, np.int64), 2, 0), 2, 1) - 128
    R = np.clip((298 * c + rv * e + 128) >> 8, 0, 255)
    G = np.clip((298 * c + gu * d + gv * e + 128) >> 8, 0, 255)
    B = np.clip((298 * c + bu * d + 128) >> 8, 0, 255)
    return R, G, B


def to_i420(buffers, pics, fmt, matrix, dw, dh):
    """-> list over streams: the converted tight I420 picture [dw*dh*3/2] of a present stream, None for an absent one"""
    check(pics, fmt, dw)
    out = []
    for pic in pics:
        if pic is None:
            out.append(None)
            continue
        buf, idx = _rows(buffers, pic, fmt, dw, dh)
        px = np.asarray(buffers[buf], np.uint8)[idx].astype(np.int64).reshape(dh, dw * bpp(fmt) // 4, 4)
        if fmt in (YUY2, UYVY):
            yo, co = (0, 1) if fmt == YUY2 else (1, 0)
            Y = px[:, :, [yo, yo + 2]].reshape(dh, dw)
            cb, cr = px[:, :, co], px[:, :, co + 2]  # [dh][dw/2]
            Cb = (cb[0::2] + cb[1::2] + 1) >> 1
            Cr = (cr[0::2] + cr[1::2] + 1) >> 1
        else:
            r, b = (2, 0) if fmt == BGRA else (0, 2)
            Y, Cb, Cr = rgb_to_yuv(px[:, :, r], px[:, :, 1], px[:, :, b], matrix)
        assert Y.min() >= 0 and Y.max() <= 255 and min(Cb.min(), Cr.min()) >= 0 and max(Cb.max(), Cr.max()) <= 255
        out.append(np.concatenate([Y.ravel(), Cb.ravel(), Cr.ravel()]).astype(np.uint8))
    return out


def from_i420(buffers, pics, fmt, matrix, frames, dw, dh):
    """frames[s] = tight I420 of dw x dh (ignored for an absent stream) -> copies of `buffers` with every picture written
    through its descriptor"""
    check(pics, fmt, dw)
    out = [np.array(b, np.uint8, copy=True) for b in buffers]
    for pic, f in zip(pics, frames):
        if pic is None:
            continue
        f = np.asarray(f, np.uint8).reshape(-1)
        assert f.size == dw * dh * 3 // 2
        Y = f[:dw * dh].reshape(dh, dw)
        Cb = f[dw * dh:dw * dh * 5 // 4].reshape(dh // 2, dw // 2)
        Cr = f[dw * dh * 5 // 4:].reshape(dh // 2, dw // 2)
        px = np.empty((dh, dw * bpp(fmt) // 4, 4), np.uint8)
        if fmt in (YUY2, UYVY):
            yo, co = (0, 1) if fmt == YUY2 else (1, 0)
            px[:, :, yo] = Y[:, 0::2]
            px[:, :, yo + 2] = Y[:, 1::2]
            px[:, :, co] = np.repeat(Cb, 2, 0)
            px[:, :, co + 2] = np.repeat(Cr, 2, 0)
        else:
            R, G, B = yuv_to_rgb(Y, Cb, Cr, matrix)
            r, b = (2, 0) if fmt == BGRA else (0, 2)
            px[:, :, r], px[:, :, 1], px[:, :, b], px[:, :, 3] = R, G, B, 255
        buf, idx = _rows(buffers, pic, fmt, dw, dh)
        out[buf][idx] = px.reshape(dh, -1)
    return out


def slot_bytes(fmt, pitch_y, dh):
    assert fmt in FMTS
    return pitch_y * dh


def slot_pic(fmt, pitch_y, dh, base=0, buf=0):
    assert fmt in FMTS
    return [(buf, base, pitch_y)]
