"""Model of pictures by descriptor (ferhip_set_pictures, ferhip_get_recon_pictures, ferhip_decs_set_layout), in plain numpy.
Test infrastructure.

A descriptor of the model is None (the stream is absent) or a list of (buffer, offset, pitch) per plane: row r of the plane
starts at byte offset + r * pitch of buffers[buffer], a flat uint8 array.  I420 has the planes Y, Cb, Cr; NV12 has Y and
the plane of interleaved CbCr pairs.

  gather      descriptors -> coded I420 pictures of W x H: ferhip_set_pictures, i.e. per plane of display size (pw, ph)
              coded sample (x, y) = source sample (min(x, pw - 1), min(y, ph - 1))
  scatter     tight I420 pictures of dw x dh -> the bytes the pitched destinations must hold afterwards: rows written,
              every other byte (pitch gaps, surroundings) as it was
  slot_bytes  bytes of one output slot of the live decoder in a pitched layout
  slot_pic    the descriptor of the slot that starts at `base` of a buffer
"""
import numpy as np

I420, NV12 = 0, 1


def _plane_dims(dw, dh):
    return [(dw, dh), (dw // 2, dh // 2), (dw // 2, dh // 2)]


def _sample_index(fmt, k, pic, x, y):
    """flat indices into the plane's buffer of samples (x[None, :], y[:, None]) of plane k (0 Y, 1 Cb, 2 Cr)"""
    if fmt == NV12 and k > 0:
        buf, off, pitch = pic[1]
        return buf, off + y[:, None] * pitch + 2 * x[None, :] + (k - 1)
    buf, off, pitch = pic[k]
    return buf, off + y[:, None] * pitch + x[None, :]


def check(pics, fmt, dw):
    """what ferhip_set_pictures refuses with FERHIP_E_ARG"""
    assert fmt in (I420, NV12)
    for p in pics:
        if p is None:
            continue
        assert p[0][2] >= dw
        for k in range(1, 3 if fmt == I420 else 2):
            assert p[k][2] >= (dw // 2 if fmt == I420 else dw)


def gather(buffers, pics, fmt, dw, dh, W, H):
    """-> list over streams: the coded I420 picture [W*H*3/2] of a present stream, None for an absent one"""
    check(pics, fmt, dw)
    out = []
    for pic in pics:
        if pic is None:
            out.append(None)
            continue
        planes = []
        for k, ((pw, ph), (PW, PH)) in enumerate(zip(_plane_dims(dw, dh), _plane_dims(W, H))):
            y = np.minimum(np.arange(PH), ph - 1)
            x = np.minimum(np.arange(PW), pw - 1)
            buf, idx = _sample_index(fmt, k, pic, x, y)
            planes.append(np.asarray(buffers[buf], np.uint8)[idx].ravel())
        out.append(np.concatenate(planes))
    return out


def scatter(buffers, pics, fmt, frames, dw, dh):
    """frames[s] = tight I420 of dw x dh (ignored for an absent stream) -> copies of `buffers` with every picture written
    through its descriptor"""
    check(pics, fmt, dw)
    out = [np.array(b, np.uint8, copy=True) for b in buffers]
    for pic, f in zip(pics, frames):
        if pic is None:
            continue
        f = np.asarray(f, np.uint8).reshape(-1)
        assert f.size == dw * dh * 3 // 2
        o = 0
        for k, (pw, ph) in enumerate(_plane_dims(dw, dh)):
            buf, idx = _sample_index(fmt, k, pic, np.arange(pw), np.arange(ph))
            out[buf][idx] = f[o:o + pw * ph].reshape(ph, pw)
            o += pw * ph
    return out


def slot_bytes(fmt, pitch_y, pitch_c, dh):
    return pitch_y * dh + (1 if fmt == NV12 else 2) * pitch_c * (dh // 2)


def slot_pic(fmt, pitch_y, pitch_c, dh, base=0, buf=0):
    """Y at base, then Cb and Cr (I420) or CbCr (NV12): the Y plane takes pitch_y * dh bytes, a chroma plane pitch_c * dh/2"""
    pic = [(buf, base, pitch_y), (buf, base + pitch_y * dh, pitch_c)]
    if fmt == I420:
        pic.append((buf, base + pitch_y * dh + pitch_c * (dh // 2), pitch_c))
    return pic


def tight_pic(fmt, dw, dh, base=0, buf=0):
    """a picture packed tight: pitches equal to the row bytes"""
    return slot_pic(fmt, dw, dw // 2 if fmt == I420 else dw, dh, base, buf)
