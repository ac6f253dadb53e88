"""Model of the display-size feature (ferhip_set_display_size and friends), in numpy and plain Python.  Test infrastructure.

  pad_picture   the padding rule of ferhip_set_frames_display: per plane of display size (pw, ph),
                coded sample (x, y) = source sample (min(x, pw - 1), min(y, ph - 1))
  window        the (x0, y0, dw, dh) window of an I420 picture (ferhip_get_recon_display, ferhip_decs_set_display)
  sps_rbsp      the SPS the encoder writes (ferhip_write_sps), with the frame cropping of a display size or of any four offsets
  swap_sps      an Annex-B stream with its SPS replaced
"""
import numpy as np
from pslice_synth import Bits, nal_unit


def planes(frame, w, h):
    f = np.asarray(frame, np.uint8).reshape(-1)
    ys, cs = w * h, (w // 2) * (h // 2)
    assert f.size == ys + 2 * cs
    return [f[:ys].reshape(h, w), f[ys:ys + cs].reshape(h // 2, w // 2), f[ys + cs:].reshape(h // 2, w // 2)]


def pad_picture(frame, dw, dh, W, H):
    """I420 dw x dh -> I420 W x H by the rule above, written as the rule: one gather per plane"""
    out = []
    for p, (PW, PH) in zip(planes(frame, dw, dh), ((W, H), (W // 2, H // 2), (W // 2, H // 2))):
        ph, pw = p.shape
        y = np.minimum(np.arange(PH), ph - 1)
        x = np.minimum(np.arange(PW), pw - 1)
        out.append(p[y[:, None], x[None, :]].ravel())
    return np.concatenate(out)


def window(frame, W, H, x0, y0, dw, dh):
    """the window (x0, y0, dw, dh) (all even) of an I420 picture of W x H, as I420 of dw x dh"""
    y, u, v = planes(frame, W, H)
    return np.concatenate([y[y0:y0 + dh, x0:x0 + dw].ravel(), u[y0 // 2:(y0 + dh) // 2, x0 // 2:(x0 + dw) // 2].ravel(),
                           v[y0 // 2:(y0 + dh) // 2, x0 // 2:(x0 + dw) // 2].ravel()])


def sps_bits(W, H, crop=None):
    """-> (Bits of the SPS up to and including vui_parameters_present_flag, number of bits in front of frame_cropping_flag).
    crop = (left, right, top, bottom) in luma samples (even), or None = no cropping."""
    w = Bits()
    w.put(8, 66)   # profile_idc
    w.put(1, 1)    # constraint_set0_flag
    w.put(1, 1)    # constraint_set1_flag
    w.put(1, 0)
    w.put(5, 0)
    w.put(8, 41)   # level_idc
    w.ue(0)        # seq_parameter_set_id
    w.ue(5)        # log2_max_frame_num_minus4
    w.ue(0)        # pic_order_cnt_type
    w.ue(6)        # log2_max_pic_order_cnt_lsb_minus4
    w.ue(1)        # max_num_ref_frames
    w.put(1, 0)    # gaps_in_frame_num_value_allowed_flag
    w.ue(W // 16 - 1)
    w.ue(H // 16 - 1)
    w.put(1, 1)    # frame_mbs_only_flag
    w.put(1, 1)    # direct_8x8_inference_flag
    before = len(w.b)
    if crop is None:
        w.put(1, 0)
    else:
        w.put(1, 1)
        for c in crop:
            assert c % 2 == 0
            w.ue(c // 2)
    w.put(1, 0)    # vui_parameters_present_flag
    return w, before


def sps_rbsp(W, H, dw=None, dh=None, crop=None):
    """The SPS RBSP of a W x H context: display size (dw, dh) -> cropping (0, W - dw, 0, H - dh) when that is not all zero;
    crop = the four offsets given directly (decoder tests)."""
    if crop is None and dw is not None and (dw < W or dh < H):
        crop = (0, W - dw, 0, H - dh)
    return sps_bits(W, H, crop)[0].rbsp(0)


def sps_nal(W, H, dw=None, dh=None, crop=None):
    return nal_unit(7, 1, sps_rbsp(W, H, dw, dh, crop))


def split_nals(stream):
    out, starts, i = [], [], 0
    while True:
        j = stream.find(b"\x00\x00\x00\x01", i)
        if j < 0:
            break
        starts.append(j)
        i = j + 4
    for k, s in enumerate(starts):
        out.append(stream[s:starts[k + 1] if k + 1 < len(starts) else len(stream)])
    return out


def swap_sps(stream, sps):
    """every SPS NAL unit of an Annex-B stream replaced by `sps` (a whole NAL unit with its start code)"""
    return b"".join(sps if (n[4] & 31) == 7 else n for n in split_nals(stream))
