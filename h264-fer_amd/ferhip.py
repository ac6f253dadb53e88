"""ctypes binding of include/ferhip.h (no torch types cross the C ABI)."""
import ctypes as C
import math
import os
from pathlib import Path

import numpy as np

NAL_SLICE, NAL_IDR, NAL_AUTO = 1, 5, 0
NAL_NONE = -1  # live contexts: the stream has no picture in this call

BUF = dict(INTERP=1, FEAT=2, SORTPOS=3, KOLIKO=4, MBTYPE=5, MV=6, MVD=7, LEVELS=8, CBP=9, TC=10, I4MODE=11,
           CUR=12, REF=13, TIMING=14, ST2N=15, ST2=16, SPEC_STAT=17, MBSIZE=18,
           SUMA=19, ST3=20, ST3N=21, V0=22, SPEC_HDR=23, SPEC_L1=24, SPEC_L2=25)
TUNE_RESOLVE_WGS, TUNE_RESOLVE_GROUP, TUNE_SPECULATE, TUNE_OVERLAP_SORT = 1, 2, 3, 4
RC_CQP, RC_ABR, RC_QUALITY = 0, 1, 2
QM_SSE, QM_SSIM, QUALITY_RING = 1, 2, 64
AU_PARAM_SETS = 1  # pack_nal / fetch_nal: SPS and the stream's own PPS in front of every IDR slice
AU_AVCC = 4        # ... every NAL unit behind its 4-byte big-endian length instead of the start code (FERHIP_AU_AVCC)
IN_ANNEXB, IN_AVCC = 0, 1  # LiveDecoder.set_input
_BUF_DTYPE = {1: np.uint8, 2: np.uint16, 3: np.uint32, 4: np.int32, 5: np.int32, 6: np.int16, 7: np.int16,
              8: np.int16, 9: np.uint8, 10: np.uint8, 11: np.uint8, 12: np.uint8, 13: np.uint8, 14: np.int64, 15: np.int32, 16: np.int32,
              17: np.uint64, 18: np.int32, 19: np.int32, 20: np.int32, 21: np.int32, 22: np.int32, 23: np.int32, 24: np.int32,
              25: np.int32}


class FerHipError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [("qp", C.c_int), ("basic", C.c_int), ("window", C.c_int), ("maxdiff", C.c_int),
                ("intra_every", C.c_int)]


class Rate(C.Structure):
    """ferhip_rate of include/ferhip.h"""
    _fields_ = [("mode", C.c_int), ("qp", C.c_int), ("qp_min", C.c_int), ("qp_max", C.c_int), ("max_step", C.c_int),
                ("ip_offset", C.c_int), ("window", C.c_int), ("target_bits", C.c_longlong), ("target_sse", C.c_longlong)]


class QualityRec(C.Structure):
    """ferhip_quality of include/ferhip.h"""
    _fields_ = [("sse", C.c_uint64 * 3), ("ssim_sum", C.c_double), ("ssim_windows", C.c_uint32), ("qp", C.c_int32),
                ("nal_type", C.c_int32), ("rbsp_bytes", C.c_uint32), ("picture", C.c_uint32)]


_QREC = np.dtype([("sse", np.uint64, 3), ("ssim_sum", np.float64), ("ssim_windows", np.uint32), ("qp", np.int32),
                  ("nal_type", np.int32), ("rbsp_bytes", np.uint32), ("picture", np.uint32)], align=True)
assert _QREC.itemsize == C.sizeof(QualityRec)

# ferhip_au of include/ferhip.h: one entry of the index of ferhip_pack_nal / ferhip_fetch_nal / ferhip_frame_nal_blocks
AU = np.dtype([("offset", np.uint64), ("bytes", np.uint32), ("nal_type", np.int32)])
# ferhip_nal_unit: one entry of the table of ferhip_split_nal_blocks
NAL_UNIT = np.dtype([("range", np.uint32), ("nal_type", np.int32), ("ref_idc", np.int32), ("bytes", np.uint32), ("offset", np.uint64)])
SPLIT_PREFIX = 64  # FERHIP_SPLIT_PREFIX: bytes of every unit's RBSP that decode_dev parses headers from
assert AU.itemsize == 16
# ferhip_rtp_hdr, ferhip_rtp_pkt, ferhip_rtp_au: the caller's RTP header fields per stream, one row of the packet table, one
# entry of the index of ferhip_pack_rtp / ferhip_fetch_rtp / ferhip_rtp_blocks
RTP_HDR = np.dtype([("ssrc", np.uint32), ("timestamp", np.uint32), ("seq", np.uint16), ("payload_type", np.uint8), ("reserved", np.uint8)])
RTP_PKT = np.dtype([("offset", np.uint64), ("bytes", np.uint32), ("stream", np.uint32)])
RTP_AU = np.dtype([("offset", np.uint64), ("bytes", np.uint32), ("nal_type", np.int32), ("first_pkt", np.uint32), ("npkts", np.uint32)])
assert (RTP_HDR.itemsize, RTP_PKT.itemsize, RTP_AU.itemsize) == (12, 16, 24)
# ferhip_ts_hdr, ferhip_ts_au: the caller's transport stream fields per stream and one entry of the index of ferhip_pack_ts /
# ferhip_fetch_ts / ferhip_ts_blocks; a row of ferhip_decs_decode_ts's table of runs has dtype RTP_PKT
TS_HDR = np.dtype([("pts", np.uint64), ("pcr", np.uint64), ("pid", np.uint16), ("pmt_pid", np.uint16), ("cc", np.uint8), ("psi_cc", np.uint8),
                   ("reserved", np.uint16)])
TS_AU = np.dtype([("offset", np.uint64), ("bytes", np.uint32), ("nal_type", np.int32), ("npkts", np.uint32), ("reserved", np.uint32)])
TS_RUN = RTP_PKT
TS_PSI = 8  # FERHIP_TS_PSI
assert (TS_HDR.itemsize, TS_AU.itemsize) == (24, 24)
# ferhip_mp4_hdr, ferhip_mp4_seg: the caller's fields of a stream's segment and one entry of the index of ferhip_mp4_close /
# ferhip_mp4_fetch / ferhip_mp4_blocks
MP4_HDR = np.dtype([("decode_time", np.uint64), ("sequence", np.uint32), ("duration", np.uint32)])
MP4_SEG = np.dtype([("offset", np.uint64), ("bytes", np.uint32), ("nsamples", np.uint32), ("first_nal_type", np.int32), ("fault", np.uint32)])
MP4_RUN = RTP_PKT
assert (MP4_HDR.itemsize, MP4_SEG.itemsize) == (16, 24)


# ferhip_srtp_key, ferhip_srtp_index: a stream's master key and salt, and its packet index state (roc, s_l, set)
SRTP_KEY = np.dtype([("master_key", np.uint8, 16), ("master_salt", np.uint8, 14), ("set", np.uint8), ("reserved", np.uint8)])
SRTP_INDEX = np.dtype([("roc", np.uint32), ("s_l", np.uint16), ("set", np.uint16)])
SRTP_PROTECT, SRTP_UNPROTECT = 0, 1
assert (SRTP_KEY.itemsize, SRTP_INDEX.itemsize) == (32, 8)


def rtp_hdr(n, ssrc=0, timestamp=0, seq=0, payload_type=96):
    """n entries of dtype RTP_HDR; every argument a scalar or a sequence of n"""
    h = np.zeros(n, RTP_HDR)
    h["ssrc"], h["timestamp"], h["seq"], h["payload_type"] = ssrc, timestamp, seq, payload_type
    return h


def ts_hdr(n, pts=0, pcr=0, pid=0x100, pmt_pid=0x1000, cc=0, psi_cc=0):
    """n entries of dtype TS_HDR; every argument a scalar or a sequence of n"""
    h = np.zeros(n, TS_HDR)
    h["pts"], h["pcr"], h["pid"], h["pmt_pid"], h["cc"], h["psi_cc"] = pts, pcr, pid, pmt_pid, cc, psi_cc
    return h


def mp4_hdr(n, decode_time=0, sequence=1, duration=1):
    """n entries of dtype MP4_HDR; every argument a scalar or a sequence of n"""
    h = np.zeros(n, MP4_HDR)
    h["decode_time"], h["sequence"], h["duration"] = decode_time, sequence, duration
    return h


def mp4_data_offset(max_samples):
    """D of include/ferhip.h: where the samples of a region begin"""
    return (104 + 12 * int(max_samples) + 15) & ~15


class Quality:
    """FerHip.quality(): arrays over [n pictures, oldest first][S streams] (sse, psnr: [..][3] for Y, Cb, Cr)"""

    def __init__(self, rec, W, H):
        self.sse = rec["sse"].astype(np.int64)
        n = np.array([W * H, W * H // 4, W * H // 4], np.float64)
        with np.errstate(divide="ignore"):
            self.psnr = 10 * np.log10(255.0 ** 2 * n / self.sse)  # +inf where sse == 0
        self.ssim_sum = rec["ssim_sum"].copy()
        self.ssim_windows = rec["ssim_windows"].astype(np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.ssim = np.where(self.ssim_windows > 0, self.ssim_sum / np.maximum(self.ssim_windows, 1), np.nan)
        self.qp = rec["qp"].copy()
        self.nal_type = rec["nal_type"].copy()
        self.rbsp_bytes = rec["rbsp_bytes"].copy()
        self.picture = rec["picture"].copy()


def lib_path():
    return Path(__file__).resolve().parent / "libferhip.so"


_lib = None


def load_library():
    """Load libferhip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not p.exists():
        raise FerHipError(f"{p} missing: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    lib = C.CDLL(str(p))
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.ferhip_version.restype = C.c_char_p
    lib.ferhip_create.argtypes = [C.POINTER(vp), i, i, i, C.POINTER(Params)]
    lib.ferhip_destroy.argtypes = [vp]
    lib.ferhip_destroy.restype = None
    lib.ferhip_set_frames.argtypes = [vp, vp, i]
    lib.ferhip_mem_alloc.argtypes = [sz, i]
    lib.ferhip_mem_alloc.restype = vp
    lib.ferhip_mem_free.argtypes = [vp, i]
    lib.ferhip_mem_free.restype = None
    lib.ferhip_mem_copy.argtypes = [vp, vp, sz]
    lib.ferhip_set_reference.argtypes = [vp, vp]
    lib.ferhip_upload_frames.argtypes = [vp, vp]
    lib.ferhip_set_frames_uploaded.argtypes = [vp]
    lib.ferhip_set_frames_live.argtypes = [vp, vp, i, vp]
    lib.ferhip_upload_frames_live.argtypes = [vp, vp, vp]
    lib.ferhip_reset_stream.argtypes = [vp, i]
    lib.ferhip_set_display_size.argtypes = [vp, i, i]
    lib.ferhip_set_frames_display.argtypes = [vp, vp, i, vp]
    lib.ferhip_upload_frames_display.argtypes = [vp, vp, vp]
    lib.ferhip_get_recon_display.argtypes = [vp, vp, i]
    lib.ferhip_set_pictures.argtypes = [vp, vp, i]
    lib.ferhip_get_recon_pictures.argtypes = [vp, vp, i]
    lib.ferhip_set_csc.argtypes = [vp, i]
    lib.ferhip_encode_picture.argtypes = [vp, C.POINTER(i), vp, sz, C.POINTER(C.c_uint32)]
    lib.ferhip_encode_picture_dev.argtypes = [vp, C.POINTER(i), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp)]
    lib.ferhip_select_nal_type.argtypes = [vp, C.POINTER(i)]
    lib.ferhip_copy_rbsp.argtypes = [vp, vp, sz, sz, vp, i]
    lib.ferhip_sync.argtypes = [vp]
    lib.ferhip_get_recon.argtypes = [vp, vp, i]
    lib.ferhip_write_sps.argtypes = [vp, vp, sz]
    lib.ferhip_write_sps.restype = sz
    lib.ferhip_write_pps.argtypes = [vp, vp, sz]
    lib.ferhip_write_pps.restype = sz
    lib.ferhip_write_pps_stream.argtypes = [vp, i, vp, sz]
    lib.ferhip_write_pps_stream.restype = sz
    lib.ferhip_set_rate.argtypes = [vp, i, C.POINTER(Rate)]
    lib.ferhip_get_qp.argtypes = [vp, C.POINTER(i)]
    lib.ferhip_set_quality.argtypes = [vp, i]
    lib.ferhip_get_quality.argtypes = [vp, i, vp]
    lib.ferhip_write_nal.argtypes = [i, i, vp, sz, vp]
    lib.ferhip_write_nal.restype = sz
    lib.ferhip_encode_streams.argtypes = [vp, vp, i, vp, sz, C.POINTER(sz), vp]
    lib.ferhip_pack_nal.argtypes = [vp, i, vp, sz, vp]
    lib.ferhip_fetch_nal.argtypes = [vp, i, vp, sz, vp]
    lib.ferhip_frame_nal_blocks.argtypes = [vp, sz, vp, vp, sz, vp, sz, vp]
    lib.ferhip_frame_nal_blocks_fmt.argtypes = [vp, sz, vp, vp, sz, i, vp, sz, vp]
    lib.ferhip_write_avcc_config.argtypes = [vp, i, vp, sz]
    lib.ferhip_write_avcc_config.restype = sz
    lib.ferhip_pack_rtp.argtypes = [vp, i, i, vp, vp, sz, vp, sz, vp]
    lib.ferhip_fetch_rtp.argtypes = [vp, i, i, vp, vp, sz, vp, sz, vp]
    lib.ferhip_rtp_blocks.argtypes = [vp, sz, vp, vp, sz, i, vp, vp, sz, vp, sz, vp]
    lib.ferhip_write_sdp_fmtp.argtypes = [vp, i, vp, sz]
    lib.ferhip_write_sdp_fmtp.restype = sz
    lib.ferhip_get_stats.argtypes = [vp, C.POINTER(i)]
    lib.ferhip_status.argtypes = [vp, C.POINTER(i)]
    lib.ferhip_fill_interpolated.argtypes = [vp]
    lib.ferhip_inter_encoding.argtypes = [vp]
    lib.ferhip_read_buffer.argtypes = [vp, i, vp, sz]
    lib.ferhip_read_buffer.restype = sz
    lib.ferhip_profile.argtypes = [vp, i]
    lib.ferhip_tune.argtypes = [vp, i, i]
    lib.ferhip_get_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long), i]
    lib.ferhip_decode_streams.argtypes = [C.POINTER(C.c_char_p), C.POINTER(sz), i, vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    lib.ferhip_decode_release.argtypes = []
    lib.ferhip_dec_create.argtypes = [C.POINTER(vp)]
    lib.ferhip_dec_destroy.argtypes = [vp]
    lib.ferhip_dec_destroy.restype = None
    lib.ferhip_dec_nal.argtypes = [vp, i, i, vp, sz, vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    lib.ferhip_decs_create.argtypes = [C.POINTER(vp), i, i, i, i]
    lib.ferhip_decs_decode.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), vp, i, C.POINTER(i), C.POINTER(i)]
    lib.ferhip_decs_reset_stream.argtypes = [vp, i]
    lib.ferhip_decs_get_crop.argtypes = [vp, i, C.POINTER(i)]
    lib.ferhip_decs_set_display.argtypes = [vp, i, i, i, i]
    lib.ferhip_decs_set_layout.argtypes = [vp, i, C.c_uint32, C.c_uint32]
    lib.ferhip_decs_set_csc.argtypes = [vp, i]
    lib.ferhip_decs_decode_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), vp, i, C.POINTER(i), C.POINTER(i)]
    lib.ferhip_pack_ts.argtypes = [vp, i, vp, vp, sz, vp]
    lib.ferhip_fetch_ts.argtypes = [vp, i, vp, vp, sz, vp]
    lib.ferhip_ts_blocks.argtypes = [vp, sz, vp, vp, sz, vp, vp, sz, vp]
    lib.ferhip_write_ts_psi.argtypes = [i, i, i, vp, sz]
    lib.ferhip_write_ts_psi.restype = sz
    lib.ferhip_mp4_open.argtypes = [vp, i, i, vp, vp, sz]
    lib.ferhip_mp4_append.argtypes = [vp]
    lib.ferhip_mp4_close.argtypes = [vp, vp]
    lib.ferhip_mp4_fetch.argtypes = [vp, vp, sz, vp]
    lib.ferhip_write_mp4_init.argtypes = [vp, i, C.c_uint32, vp, sz]
    lib.ferhip_write_mp4_init.restype = sz
    lib.ferhip_mp4_blocks.argtypes = [vp, sz, vp, vp, sz, sz, i, vp, vp, sz, vp]
    lib.ferhip_decs_decode_mp4.argtypes = [vp, vp, i, vp, sz, i, vp, i, C.POINTER(i), C.POINTER(i)]
    lib.ferhip_mp4_find_avcc.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(sz)]
    lib.ferhip_decs_decode_ts.argtypes = [vp, vp, i, vp, sz, vp, vp, i, C.POINTER(i), C.POINTER(i)]
    lib.ferhip_unts_blocks.argtypes = [vp, sz, vp, sz, i, i, vp, vp, vp, sz, vp, sz, C.POINTER(sz), vp, vp]
    lib.ferhip_decs_decode_rtp.argtypes = [vp, vp, i, vp, sz, vp, i, C.POINTER(i), C.POINTER(i)]
    lib.ferhip_unrtp_blocks.argtypes = [vp, sz, vp, sz, i, i, vp, vp, sz, vp, sz, C.POINTER(sz), vp, vp]
    lib.ferhip_srtp_create.argtypes = [C.POINTER(vp), i]
    lib.ferhip_srtp_destroy.argtypes = [vp]
    lib.ferhip_srtp_destroy.restype = None
    lib.ferhip_srtp_set_key.argtypes = [vp, i, vp, vp]
    lib.ferhip_srtp_derive.argtypes = [vp, vp, vp]
    lib.ferhip_srtp_get_index.argtypes = [vp, i, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(i)]
    lib.ferhip_srtp_set_index.argtypes = [vp, i, C.c_uint32, C.c_uint32, i]
    lib.ferhip_srtp_protect.argtypes = [vp, vp, vp, vp, sz, vp, sz, vp]
    lib.ferhip_srtp_protect_dev.argtypes = [vp, vp, vp, vp, sz, vp, sz, vp]
    lib.ferhip_srtp_unprotect.argtypes = [vp, vp, vp, i, vp, sz, vp, sz, vp, vp]
    lib.ferhip_srtp_blocks.argtypes = [i, vp, vp, i, vp, sz, vp, sz, i, vp, sz, vp, vp, vp]
    lib.ferhip_decs_timing.argtypes = [vp, C.POINTER(C.c_double), i]
    lib.ferhip_split_nal_blocks.argtypes = [vp, sz, vp, sz, i, vp, sz, vp, sz, C.POINTER(sz)]
    lib.ferhip_split_avcc_blocks.argtypes = [vp, sz, vp, sz, i, i, vp, sz, vp, sz, C.POINTER(sz), vp]
    lib.ferhip_decs_set_input.argtypes = [vp, i, i]
    lib.ferhip_decs_set_config.argtypes = [vp, i, vp, sz]
    lib.ferhip_decs_destroy.argtypes = [vp]
    lib.ferhip_decs_destroy.restype = None
    lib.ferhip_y4m_open.argtypes = [C.POINTER(vp), C.c_char_p, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    lib.ferhip_y4m_read.argtypes = [vp, vp]
    lib.ferhip_y4m_close.argtypes = [vp]
    lib.ferhip_y4m_close.restype = None
    lib.ferhip_y4m_write_header.argtypes = [vp, i, i]
    lib.ferhip_y4m_write_frame.argtypes = [vp, vp, i, i, i]
    lib.ferhip_forward_residual.argtypes = [i, vp, vp, i, sz]
    lib.ferhip_inverse_residual.argtypes = [i, vp, vp, i, sz]
    for n_ in ("forward_dc_luma_intra", "inverse_dc_luma_intra", "forward_dc_chroma", "inverse_dc_chroma"):
        getattr(lib, "ferhip_" + n_).argtypes = [i, vp, vp, sz]
    lib.ferhip_transform_scan.argtypes = [vp, vp, i, sz]
    lib.ferhip_transform_inverse_scan.argtypes = [vp, vp, sz]
    _lib = lib
    return lib


FMT_I420, FMT_NV12 = 0, 1
FMT_YUY2, FMT_UYVY, FMT_BGRA, FMT_RGBA = 4, 5, 8, 9  # packed: one plane, converted on the device (see ferhip.h)
CSC_BT601, CSC_BT709 = 0, 1


class Pic(C.Structure):
    """ferhip_pic: one picture where it lies in device memory -- a pointer and a row pitch per plane"""
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_uint32 * 3), ("reserved", C.c_uint32)]


def pic_table(pics):
    """a list of Pic, None (an absent stream) or (planes, pitches) tuples of up to three entries each -> a ferhip_pic array"""
    t = (Pic * len(pics))()
    for k, p in enumerate(pics):
        if p is None:
            continue
        if isinstance(p, Pic):
            t[k] = p
            continue
        planes, pitches = p
        for n, (a, b) in enumerate(zip(planes, pitches)):
            t[k].plane[n] = int(a) if a else None
            t[k].pitch[n] = int(b)
    return t


def _chk(rc, what):
    if rc != 0:
        raise FerHipError(f"{what} failed with code {rc}")


class DeviceBuffer:
    """HBM (or pinned host) memory through the library's own runtime (ferhip_mem_*), for callers without torch."""

    def __init__(self, nbytes, pinned=False):
        self.lib = load_library()
        self.nbytes, self.kind = nbytes, int(pinned)
        self.ptr = self.lib.ferhip_mem_alloc(nbytes, self.kind)
        if not self.ptr:
            raise FerHipError(f"ferhip_mem_alloc({nbytes}) failed")

    def upload(self, arr, offset=0):
        a = np.ascontiguousarray(arr)
        _chk(self.lib.ferhip_mem_copy(C.c_void_p(self.ptr + offset), a.ctypes.data, a.nbytes), "ferhip_mem_copy")

    def download(self, nbytes=None, offset=0, dtype=np.uint8):
        out = np.empty((nbytes or self.nbytes) // np.dtype(dtype).itemsize, dtype)
        _chk(self.lib.ferhip_mem_copy(out.ctypes.data, C.c_void_p(self.ptr + offset), out.nbytes), "ferhip_mem_copy")
        return out

    def free(self):
        if self.ptr:
            self.lib.ferhip_mem_free(C.c_void_p(self.ptr), self.kind)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class FerHip:
    """One encoder context = S independent streams of W x H pictures on one GPU.

    Mirrors Starter::PostaviParametre / PokreniKoder / NastaviKoder / DohvatiStatistiku.
    """

    def __init__(self, width, height, nstreams=1, qp=12, window=16, maxdiff=3, intra_every=30, basic=0):
        self.lib = load_library()
        self.W, self.H, self.S = width, height, nstreams
        self.nmb = (width // 16) * (height // 16)
        self.fsz = width * height * 3 // 2
        self.dw, self.dh, self.dfsz = width, height, self.fsz  # display size (set_display_size)
        self.params = Params(qp, basic, window, maxdiff, intra_every)
        self.ctx = C.c_void_p()
        _chk(self.lib.ferhip_create(C.byref(self.ctx), width, height, nstreams, C.byref(self.params)), "ferhip_create")

    def close(self):
        if self.ctx:
            self.lib.ferhip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- pictures
    def set_frames(self, frames):
        a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(self.S, self.fsz)
        _chk(self.lib.ferhip_set_frames(self.ctx, a.ctypes.data, 1), "ferhip_set_frames")

    def set_frames_device(self, dptr):
        _chk(self.lib.ferhip_set_frames(self.ctx, C.c_void_p(int(dptr)), 0), "ferhip_set_frames(dev)")

    def upload_frames(self, host_ptr):
        """start the asynchronous H2D copy of the next pictures (pinned host memory, [S][fsz])"""
        _chk(self.lib.ferhip_upload_frames(self.ctx, C.c_void_p(int(host_ptr))), "ferhip_upload_frames")

    def set_frames_uploaded(self):
        _chk(self.lib.ferhip_set_frames_uploaded(self.ctx), "ferhip_set_frames_uploaded")

    # --- live contexts: streams that sit out a picture, slots that change feeds
    def _mask(self, present):
        m = np.ascontiguousarray(np.asarray(present) != 0, dtype=np.uint8).reshape(-1)
        if m.size != self.S:
            raise ValueError(f"present has {m.size} entries, the context {self.S} streams")
        return m

    def set_frames_live(self, frames, present):
        """ferhip_set_frames_live: the pictures of the streams with present[s] != 0; the other slots are never read.
        frames: an [S][fsz] uint8 array (host), or an integer = a device pointer to that layout."""
        m = self._mask(present)
        if isinstance(frames, (int, np.integer)):
            rc = self.lib.ferhip_set_frames_live(self.ctx, C.c_void_p(int(frames)), 0, m.ctypes.data)
        else:
            a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(self.S, self.fsz)
            rc = self.lib.ferhip_set_frames_live(self.ctx, a.ctypes.data, 1, m.ctypes.data)
        _chk(rc, "ferhip_set_frames_live")

    def upload_frames_live(self, host_ptr, present):
        """upload_frames for the present streams only (pinned host memory, [S][fsz]); set_frames_uploaded() follows"""
        m = self._mask(present)
        _chk(self.lib.ferhip_upload_frames_live(self.ctx, C.c_void_p(int(host_ptr)), m.ctypes.data), "ferhip_upload_frames_live")

    def reset_stream(self, s):
        """ferhip_reset_stream: slot s as in a freshly created context (a new feed takes the slot)"""
        _chk(self.lib.ferhip_reset_stream(self.ctx, int(s)), "ferhip_reset_stream")

    def encode_live(self, pictures, nal_types=None):
        """One call of a live context.  pictures: length-S list, pictures[s] = the I420 picture of stream s (fsz bytes) or
        None when stream s has none now.  -> (list of rbsp bytes, b"" for absent streams; nal types, NAL_NONE for them).
        nal_types (optional) requests NAL_IDR / NAL_SLICE / NAL_AUTO for the present streams."""
        if len(pictures) != self.S:
            raise ValueError(f"{len(pictures)} pictures for {self.S} streams")
        present = np.array([p is not None for p in pictures], np.uint8)
        buf = np.empty((self.S, self.fsz), np.uint8)
        for s, p in enumerate(pictures):
            if p is not None:
                buf[s] = np.asarray(p, np.uint8).reshape(self.fsz)
        if present.any():
            self.set_frames_live(buf, present)
        nt = [NAL_NONE if not present[s] else (NAL_AUTO if nal_types is None else nal_types[s]) for s in range(self.S)]
        return self.encode_picture(nt)

    # --- display size: pictures of any even size, padded to the coded size on the device and cropped by the SPS
    def set_display_size(self, dw, dh):
        """ferhip_set_display_size: W - 16 < dw <= W, H - 16 < dh <= H, both even; before the first picture"""
        _chk(self.lib.ferhip_set_display_size(self.ctx, int(dw), int(dh)), "ferhip_set_display_size")
        self.dw, self.dh, self.dfsz = int(dw), int(dh), int(dw) * int(dh) * 3 // 2

    def set_frames_display(self, frames, present=None):
        """ferhip_set_frames_display: [S][dw*dh*3/2] display-size pictures, padded by edge replication on the device.
        frames: a uint8 array (host), or an integer = a device pointer of any alignment.  present (optional): as in
        set_frames_live."""
        m = None if present is None else self._mask(present)
        mp = None if m is None else m.ctypes.data
        if isinstance(frames, (int, np.integer)):
            rc = self.lib.ferhip_set_frames_display(self.ctx, C.c_void_p(int(frames)), 0, mp)
        else:
            a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(self.S, self.dfsz)
            rc = self.lib.ferhip_set_frames_display(self.ctx, a.ctypes.data, 1, mp)
        _chk(rc, "ferhip_set_frames_display")

    def upload_frames_display(self, host_ptr, present=None):
        """upload_frames for display-size pictures (pinned host memory, [S][dw*dh*3/2]); set_frames_uploaded() pads them"""
        m = None if present is None else self._mask(present)
        _chk(self.lib.ferhip_upload_frames_display(self.ctx, C.c_void_p(int(host_ptr)), None if m is None else m.ctypes.data),
             "ferhip_upload_frames_display")

    def get_recon_display(self):
        """the top-left dw x dh window of the last reconstruction, [S][dw*dh*3/2]"""
        out = np.empty((self.S, self.dfsz), np.uint8)
        _chk(self.lib.ferhip_get_recon_display(self.ctx, out.ctypes.data, 1), "ferhip_get_recon_display")
        return out

    # --- pictures by descriptor: one pointer and row pitch per stream and plane, I420 or NV12, in device memory
    def set_pictures(self, pics, fmt=FMT_I420):
        """ferhip_set_pictures: pics[s] = Pic, (planes, pitches) or None for an absent stream (see pic_table); pictures of the
        display size, padded by edge replication on the device"""
        if len(pics) != self.S:
            raise ValueError(f"{len(pics)} descriptors for {self.S} streams")
        _chk(self.lib.ferhip_set_pictures(self.ctx, pic_table(pics), int(fmt)), "ferhip_set_pictures")

    def set_csc(self, matrix):
        """ferhip_set_csc: CSC_BT601 (the default) or CSC_BT709 for set_pictures / get_recon_pictures in FMT_BGRA / FMT_RGBA"""
        _chk(self.lib.ferhip_set_csc(self.ctx, int(matrix)), "ferhip_set_csc")

    def get_recon_pictures(self, pics, fmt=FMT_I420):
        """ferhip_get_recon_pictures: the dw x dh window of the last reconstruction, written through the descriptors"""
        if len(pics) != self.S:
            raise ValueError(f"{len(pics)} descriptors for {self.S} streams")
        _chk(self.lib.ferhip_get_recon_pictures(self.ctx, pic_table(pics), int(fmt)), "ferhip_get_recon_pictures")

    def set_reference(self, frames):
        a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(self.S, self.fsz)
        _chk(self.lib.ferhip_set_reference(self.ctx, a.ctypes.data), "ferhip_set_reference")

    def encode_picture(self, nal_types=None):
        """RBSP_encode for one picture of every stream -> (list of rbsp bytes, nal types).  A stream whose entry of
        nal_types is NAL_NONE has no picture in this call: b"" and NAL_NONE come back for it."""
        nt = (C.c_int * self.S)(*([NAL_AUTO] * self.S if nal_types is None else nal_types))
        stride = self.nmb * 1024 + 4096
        buf = np.empty((self.S, stride), np.uint8)
        ln = (C.c_uint32 * self.S)()
        _chk(self.lib.ferhip_encode_picture(self.ctx, nt, buf.ctypes.data, stride, ln), "ferhip_encode_picture")
        return [bytes(buf[s, : ln[s]]) for s in range(self.S)], list(nt)

    def encode_picture_device(self, nal_types=None):
        nt = (C.c_int * self.S)(*([NAL_AUTO] * self.S if nal_types is None else nal_types))
        p, st, pl = C.c_void_p(), C.c_size_t(), C.c_void_p()
        _chk(self.lib.ferhip_encode_picture_dev(self.ctx, nt, C.byref(p), C.byref(st), C.byref(pl)),
             "ferhip_encode_picture_dev")
        return p.value, st.value, pl.value, list(nt)

    def copy_rbsp_device(self, dst_ptr, len_ptr, stride=None, nbytes=None):
        """RBSP + lengths of the last picture -> device buffers, on the library's stream (asynchronous)."""
        stride = stride or (self.nmb * 1024 + 4096)
        _chk(self.lib.ferhip_copy_rbsp(self.ctx, C.c_void_p(int(dst_ptr)), stride, nbytes or stride, C.c_void_p(int(len_ptr)), 0),
             "ferhip_copy_rbsp")

    def copy_rbsp_host(self, dst, lens, nbytes):
        """... -> host arrays dst [S][stride] uint8 (pinned for asynchrony), lens [S] uint32; sync() before reading"""
        _chk(self.lib.ferhip_copy_rbsp(self.ctx, C.c_void_p(int(dst.ctypes.data if hasattr(dst, "ctypes") else dst.data_ptr())),
                                       int(dst.strides[0] if hasattr(dst, "strides") else dst.stride(0)), nbytes,
                                       C.c_void_p(int(lens.ctypes.data if hasattr(lens, "ctypes") else lens.data_ptr())), 1),
             "ferhip_copy_rbsp")

    def sync(self):
        _chk(self.lib.ferhip_sync(self.ctx), "ferhip_sync")

    def get_recon(self):
        out = np.empty((self.S, self.fsz), np.uint8)
        _chk(self.lib.ferhip_get_recon(self.ctx, out.ctypes.data, 1), "ferhip_get_recon")
        return out

    def encode_streams(self, frames, want_recon=False, want_qp=False):
        """frames: [T][S][fsz] uint8 -> (list of Annex-B byte strings, recon or None); want_qp: also the [T][S] QPs used."""
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        T = a.size // (self.S * self.fsz)
        a = a.reshape(T, self.S, self.fsz)
        if want_qp:
            # ferhip_encode_streams picture by picture, with the QP of every picture read back
            out = [b"".join(self.sps_pps(s)) for s in range(self.S)]
            rec = np.empty((T, self.S, self.fsz), np.uint8) if want_recon else None
            qps = np.empty((T, self.S), np.int32)
            for t in range(T):
                self.set_frames(a[t])
                rbsp, nt = self.encode_picture()
                for s in range(self.S):
                    out[s] += self.write_nal(nt[s], rbsp[s])
                qps[t] = self.last_qp()
                if want_recon:
                    rec[t] = self.get_recon()
            return out, rec, qps
        stride = 64 + T * (self.nmb * 1024 + 4096) * 3 // 2
        out = np.empty((self.S, stride), np.uint8)
        ln = (C.c_size_t * self.S)()
        rec = np.empty((T, self.S, self.fsz), np.uint8) if want_recon else None
        _chk(self.lib.ferhip_encode_streams(self.ctx, a.ctypes.data, T, out.ctypes.data, stride, ln,
                                            rec.ctypes.data if want_recon else None), "ferhip_encode_streams")
        return [bytes(out[s, : ln[s]]) for s in range(self.S)], rec

    def sps_pps(self, stream=None):
        """Annex-B SPS and PPS; stream = s: the PPS of stream s (pic_init_qp = 14 + its base QP), None: of params.qp"""
        b = np.empty(64, np.uint8)
        o = np.empty(128, np.uint8)
        n = self.lib.ferhip_write_sps(self.ctx, b.ctypes.data, 64)
        m = self.lib.ferhip_write_nal(1, 7, b.ctypes.data, n, o.ctypes.data)
        sps = bytes(o[:m])
        if stream is None:
            n = self.lib.ferhip_write_pps(self.ctx, b.ctypes.data, 64)
        else:
            n = self.lib.ferhip_write_pps_stream(self.ctx, stream, b.ctypes.data, 64)
            if n == 0:
                raise FerHipError(f"ferhip_write_pps_stream({stream}) failed")
        m = self.lib.ferhip_write_nal(1, 8, b.ctypes.data, n, o.ctypes.data)
        return sps, bytes(o[:m])

    def avcc_config(self, stream):
        """ferhip_write_avcc_config: the AVCDecoderConfigurationRecord of a stream (the payload of an avcC box): its SPS and
        its own PPS, 4-byte NAL lengths"""
        o = np.empty(256, np.uint8)
        n = self.lib.ferhip_write_avcc_config(self.ctx, int(stream), o.ctypes.data, o.size)
        if n == 0:
            raise FerHipError(f"ferhip_write_avcc_config({stream}) failed")
        return bytes(o[:n])

    def write_nal(self, nal_type, rbsp):
        r = np.frombuffer(rbsp, np.uint8)
        o = np.empty(len(rbsp) * 3 // 2 + 16, np.uint8)
        m = self.lib.ferhip_write_nal(1, nal_type, r.ctypes.data, len(rbsp), o.ctypes.data)
        return bytes(o[:m])

    # --- NAL framing on the device
    def pack_nal_device(self, dst_ptr, index_ptr, cap, flags=0):
        """ferhip_pack_nal: the last picture's Annex-B NAL units -> device memory at dst_ptr (16-byte aligned, cap bytes) and
        their index (S + 1 records of dtype AU) at index_ptr, on the library's stream (asynchronous; sync() before reading)."""
        _chk(self.lib.ferhip_pack_nal(self.ctx, int(flags), C.c_void_p(int(dst_ptr) if dst_ptr else None), int(cap),
                                      C.c_void_p(int(index_ptr))), "ferhip_pack_nal")

    def fetch_nal_raw(self, cap, flags=0):
        """ferhip_fetch_nal into a new host buffer of cap bytes -> (return code, buffer, index [S + 1] of dtype AU)"""
        buf = np.empty(max(int(cap), 1), np.uint8)
        idx = np.zeros(self.S + 1, AU)
        rc = self.lib.ferhip_fetch_nal(self.ctx, int(flags), buf.ctypes.data, int(cap), idx.ctypes.data)
        return rc, buf, idx

    def fetch_nal(self, flags=0, cap=None):
        """The last picture of every stream as Annex-B NAL units (waits) -> (list of bytes per stream, b"" for the streams
        without a picture; NAL unit types, 0 for them).  With AU_PARAM_SETS an IDR entry is SPS + PPS + slice; with AU_AVCC
        every unit stands behind its 4-byte length instead of a start code (an MP4 / FLV sample).
        cap: size of the host buffer; None = one that grows to what the pictures need."""
        grow = cap is None
        if grow:
            cap = getattr(self, "_nal_cap", 1 << 20)
        rc, buf, idx = self.fetch_nal_raw(cap, flags)
        if grow and rc == -1 and int(idx["offset"][self.S]) > cap:  # FERHIP_E_ARG with a true index: the buffer was too small
            cap = self._nal_cap = 2 * int(idx["offset"][self.S])
            rc, buf, idx = self.fetch_nal_raw(cap, flags)
        _chk(rc, "ferhip_fetch_nal")
        return ([bytes(buf[int(idx["offset"][s]): int(idx["offset"][s]) + int(idx["bytes"][s])]) for s in range(self.S)],
                [int(t) for t in idx["nal_type"][: self.S]])

    # --- RTP packets on the device
    def pack_rtp_device(self, hdr, max_packet, dst_ptr, cap, pkts_ptr, pkts_cap, index_ptr, flags=0):
        """ferhip_pack_rtp: the last picture's RTP packets (RFC 6184, packetization-mode 1) -> device memory at dst_ptr
        (16-byte aligned, cap bytes), their table (pkts_cap rows of dtype RTP_PKT) at pkts_ptr and the index (S + 1 records of
        dtype RTP_AU) at index_ptr, on the library's stream (asynchronous; sync() before reading).  hdr: S entries of dtype
        RTP_HDR (rtp_hdr); the caller advances seq by index[s].npkts."""
        h = np.ascontiguousarray(hdr, RTP_HDR)
        assert h.size == self.S
        _chk(self.lib.ferhip_pack_rtp(self.ctx, int(flags), int(max_packet), h.ctypes.data, C.c_void_p(int(dst_ptr) if dst_ptr else None),
                                      int(cap), C.c_void_p(int(pkts_ptr) if pkts_ptr else None), int(pkts_cap), C.c_void_p(int(index_ptr))),
             "ferhip_pack_rtp")

    def fetch_rtp_raw(self, hdr, max_packet, cap, pkts_cap, flags=0, fill=0):
        """ferhip_fetch_rtp into new host buffers -> (return code, buffer [cap], table [pkts_cap] of dtype RTP_PKT, index
        [S + 1] of dtype RTP_AU)"""
        h = np.ascontiguousarray(hdr, RTP_HDR)
        assert h.size == self.S
        buf = np.full(max(int(cap), 1), fill, np.uint8)
        pkts = np.zeros(max(int(pkts_cap), 1), RTP_PKT)
        idx = np.zeros(self.S + 1, RTP_AU)
        rc = self.lib.ferhip_fetch_rtp(self.ctx, int(flags), int(max_packet), h.ctypes.data, buf.ctypes.data, int(cap), pkts.ctypes.data,
                                       int(pkts_cap), idx.ctypes.data)
        return rc, buf, pkts, idx

    def fetch_rtp(self, hdr, max_packet=1400, flags=0):
        """The last picture of every stream as RTP packets (waits) -> (list per stream of the packets as bytes, [] for the
        streams without a picture; the index of dtype RTP_AU).  With AU_PARAM_SETS an IDR slice follows a STAP-A packet with
        the SPS and the stream's PPS."""
        cap, pcap = getattr(self, "_rtp_cap", (1 << 20, 1 << 12))
        rc, buf, pkts, idx = self.fetch_rtp_raw(hdr, max_packet, cap, pcap, flags)
        if rc == -1 and (int(idx["offset"][self.S]) > cap or int(idx["first_pkt"][self.S]) > pcap):  # a true index: too small
            cap, pcap = self._rtp_cap = (max(cap, 2 * int(idx["offset"][self.S])), max(pcap, 2 * int(idx["first_pkt"][self.S])))
            rc, buf, pkts, idx = self.fetch_rtp_raw(hdr, max_packet, cap, pcap, flags)
        _chk(rc, "ferhip_fetch_rtp")
        out = []
        for s in range(self.S):
            rows = pkts[int(idx["first_pkt"][s]): int(idx["first_pkt"][s]) + int(idx["npkts"][s])]
            out.append([bytes(buf[int(r["offset"]): int(r["offset"]) + int(r["bytes"])]) for r in rows])
        return out, idx

    def sdp_fmtp(self, stream):
        """ferhip_write_sdp_fmtp: the format parameters of a stream for an SDP a=fmtp line"""
        o = C.create_string_buffer(512)
        n = self.lib.ferhip_write_sdp_fmtp(self.ctx, int(stream), o, 512)
        if n == 0:
            raise FerHipError(f"ferhip_write_sdp_fmtp({stream}) failed")
        return o.raw[:n].decode()

    # --- transport stream packets on the device
    def pack_ts_device(self, hdr, dst_ptr, cap, index_ptr, flags=0):
        """ferhip_pack_ts: the last picture's 188-byte transport stream packets -> device memory at dst_ptr (16-byte aligned,
        cap bytes) and the index (S + 1 records of dtype TS_AU) at index_ptr, on the library's stream (asynchronous; sync()
        before reading).  hdr: S entries of dtype TS_HDR (ts_hdr); the caller advances cc and psi_cc."""
        h = np.ascontiguousarray(hdr, TS_HDR)
        assert h.size == self.S
        _chk(self.lib.ferhip_pack_ts(self.ctx, int(flags), h.ctypes.data, C.c_void_p(int(dst_ptr) if dst_ptr else None), int(cap),
                                     C.c_void_p(int(index_ptr))), "ferhip_pack_ts")

    def fetch_ts_raw(self, hdr, cap, flags=0, fill=0):
        """ferhip_fetch_ts into a new host buffer -> (return code, buffer [cap], index [S + 1] of dtype TS_AU)"""
        h = np.ascontiguousarray(hdr, TS_HDR)
        assert h.size == self.S
        buf = np.full(max(int(cap), 1), fill, np.uint8)
        idx = np.zeros(self.S + 1, TS_AU)
        rc = self.lib.ferhip_fetch_ts(self.ctx, int(flags), h.ctypes.data, buf.ctypes.data, int(cap), idx.ctypes.data)
        return rc, buf, idx

    def fetch_ts(self, hdr, flags=0):
        """The last picture of every stream as transport stream packets (waits) -> (list per stream of its packets as one
        bytes, b"" for the streams without a picture; the index of dtype TS_AU).  With TS_PSI a PAT and a PMT packet stand
        in front of an I picture's packets."""
        cap = getattr(self, "_ts_cap", 1 << 20)
        rc, buf, idx = self.fetch_ts_raw(hdr, cap, flags)
        if rc == -1 and int(idx["offset"][self.S]) > cap:  # a true index: the buffer was too small
            cap = self._ts_cap = 2 * int(idx["offset"][self.S])
            rc, buf, idx = self.fetch_ts_raw(hdr, cap, flags)
        _chk(rc, "ferhip_fetch_ts")
        return [bytes(buf[int(idx["offset"][s]): int(idx["offset"][s]) + int(idx["bytes"][s])]) for s in range(self.S)], idx

    # --- fragmented MP4 segments on the device
    def mp4_open(self, hdr, max_samples, dst_ptr, stride, flags=0):
        """ferhip_mp4_open: begin a segment of at most max_samples pictures per stream in device memory at dst_ptr (16-byte
        aligned; stream s owns stride bytes at dst_ptr + s * stride).  hdr: S entries of dtype MP4_HDR (mp4_hdr); the caller
        advances decode_time by nsamples * duration and sequence by 1 from segment to segment."""
        h = np.ascontiguousarray(hdr, MP4_HDR)
        assert h.size == self.S
        _chk(self.lib.ferhip_mp4_open(self.ctx, int(flags), int(max_samples), h.ctypes.data, C.c_void_p(int(dst_ptr)), int(stride)), "ferhip_mp4_open")

    def mp4_append(self):
        """ferhip_mp4_append: the last picture of every stream that coded one becomes the stream's next sample (asynchronous)"""
        _chk(self.lib.ferhip_mp4_append(self.ctx), "ferhip_mp4_append")

    def mp4_close_device(self, index_ptr):
        """ferhip_mp4_close: moof, free and mdat headers into every region, the index (S + 1 records of dtype MP4_SEG) to
        device memory at index_ptr (asynchronous; sync() before reading)"""
        _chk(self.lib.ferhip_mp4_close(self.ctx, C.c_void_p(int(index_ptr))), "ferhip_mp4_close")

    def mp4_fetch_raw(self, cap, fill=0):
        """ferhip_mp4_fetch into a new host buffer -> (return code, buffer [cap], index [S + 1] of dtype MP4_SEG)"""
        buf = np.full(max(int(cap), 1), fill, np.uint8)
        idx = np.zeros(self.S + 1, MP4_SEG)
        rc = self.lib.ferhip_mp4_fetch(self.ctx, buf.ctypes.data, int(cap), idx.ctypes.data)
        return rc, buf, idx

    def mp4_fetch(self, cap):
        """Close the segment and bring it to the host (waits) -> (list per stream of its moof + mdat as bytes, b"" for the
        streams without a sample; the index of dtype MP4_SEG).  cap: at least the sum of the segments, S * stride at most."""
        rc, buf, idx = self.mp4_fetch_raw(cap)
        _chk(rc, "ferhip_mp4_fetch")
        return [bytes(buf[int(idx["offset"][s]): int(idx["offset"][s]) + int(idx["bytes"][s])]) for s in range(self.S)], idx

    def mp4_init(self, stream, timescale, cap=1024):
        """ferhip_write_mp4_init: the initialisation segment (ftyp + moov) of a stream, b"" where the library refuses"""
        o = np.zeros(max(int(cap), 1), np.uint8)
        n = self.lib.ferhip_write_mp4_init(self.ctx, int(stream), int(timescale), o.ctypes.data, int(cap))
        return bytes(o[:n])

    # --- rate control
    def set_rate(self, stream=-1, mode=RC_CQP, qp=None, qp_min=0, qp_max=51, max_step=2, ip_offset=3, window=0,
                 target_bits=0, target_sse=0, target_psnr=None):
        """ferhip_set_rate for one stream (or every stream, -1) from the next picture on; qp None = params.qp.

        RC_QUALITY holds the luma SSE of every picture at target_sse.  target_psnr (dB, luma) replaces it with
        floor(255^2 * W * H / 10^(target_psnr / 10)), the SSE of a picture with that PSNR."""
        if target_psnr is not None:
            target_sse = self.sse_of_psnr(target_psnr)
        r = Rate(mode, self.params.qp if qp is None else qp, qp_min, qp_max, max_step, ip_offset, window, int(target_bits),
                 int(target_sse))
        _chk(self.lib.ferhip_set_rate(self.ctx, stream, C.byref(r)), "ferhip_set_rate")

    def sse_of_psnr(self, db):
        """the luma SSE of a picture of this context's size at `db` dB: floor(255^2 * W * H / 10^(db / 10))"""
        return int(math.floor(255 ** 2 * self.W * self.H / 10 ** (db / 10)))

    # --- quality measurement
    def set_quality(self, flags):
        """ferhip_set_quality: 0 = off, QM_SSE | QM_SSIM; from the next picture on"""
        _chk(self.lib.ferhip_set_quality(self.ctx, int(flags)), "ferhip_set_quality")

    def quality(self, npic=1):
        """the last min(npic, measured, 64) pictures' records (waits for the last picture) -> Quality"""
        out = np.zeros((max(int(npic), 1), self.S), _QREC)
        n = self.lib.ferhip_get_quality(self.ctx, int(npic), out.ctypes.data)
        if n < 0:
            raise FerHipError(f"ferhip_get_quality failed with code {n}")
        return Quality(out[:n], self.W, self.H)

    def last_qp(self):
        """QP of every stream's last picture (waits for it)"""
        a = (C.c_int * self.S)()
        _chk(self.lib.ferhip_get_qp(self.ctx, a), "ferhip_get_qp")
        return list(a)

    # --- stage entry points / state read-back
    def fill_interpolated(self):
        _chk(self.lib.ferhip_fill_interpolated(self.ctx), "ferhip_fill_interpolated")

    def inter_encoding(self):
        _chk(self.lib.ferhip_inter_encoding(self.ctx), "ferhip_inter_encoding")

    def read(self, name):
        which = BUF[name]
        n = self.nmb * self.S
        px = self.W * self.H * self.S
        count = {1: px * 16, 2: px * 96, 3: px, 4: 16385 * self.S, 5: n, 6: n * 8, 7: n * 8, 8: n * 400, 9: n * 2,
                 10: n * 24, 11: n * 16, 12: self.fsz * self.S, 13: self.fsz * self.S, 14: 64, 15: n * 4, 16: n * 4 * 384 * 2, 17: 8, 18: n * 2,
                 19: n * 20, 20: n * 4 * 99, 21: n * 4, 22: n * 4, 23: n * 16, 24: n * 4 * 34, 25: n * 4 * 66}[which]
        out = np.empty(count, _BUF_DTYPE[which])
        got = self.lib.ferhip_read_buffer(self.ctx, which, out.ctypes.data, out.nbytes)
        if got != out.nbytes:
            raise FerHipError(f"ferhip_read_buffer({name}) returned {got}, expected {out.nbytes}")
        return out

    PHASES = ("interp", "me_pre", "me_resolve", "p_resid", "intra", "cavlc", "frame_sad", "me_spec", "sort", "me_walk",
              "sort_keys", "sort_finish")
    NPHASE = 12

    def tune(self, key, value):
        _chk(self.lib.ferhip_tune(self.ctx, key, value), "ferhip_tune")

    def profile(self, enable=True):
        _chk(self.lib.ferhip_profile(self.ctx, int(enable)), "ferhip_profile")

    def get_profile(self, reset=True):
        """{phase: (milliseconds, launches)} measured with HIP events on the launch stream."""
        ms = (C.c_double * self.NPHASE)()
        ln = (C.c_long * self.NPHASE)()
        _chk(self.lib.ferhip_get_profile(self.ctx, ms, ln, int(reset)), "ferhip_get_profile")
        return {n: (ms[k], ln[k]) for k, n in enumerate(self.PHASES)}

    def stats(self):
        a = (C.c_int * (5 * self.S))()
        _chk(self.lib.ferhip_get_stats(self.ctx, a), "ferhip_get_stats")
        return np.array(a).reshape(self.S, 5)

    def status(self):
        a = (C.c_int * self.S)()
        _chk(self.lib.ferhip_status(self.ctx, a), "ferhip_status")
        return list(a)


def forward_residual(qp, blocks, keep_dc=False):
    """forwardResidual of F/quantizationTransform.h on n 4x4 int32 blocks (device)."""
    lib = load_library()
    a = np.ascontiguousarray(blocks, np.int32).reshape(-1, 16)
    out = np.empty_like(a)
    _chk(lib.ferhip_forward_residual(qp, a.ctypes.data, out.ctypes.data, int(keep_dc), a.shape[0]),
         "ferhip_forward_residual")
    return out


def inverse_residual(qp, blocks, keep_dc=False):
    lib = load_library()
    a = np.ascontiguousarray(blocks, np.int32).reshape(-1, 16)
    out = np.empty_like(a)
    _chk(lib.ferhip_inverse_residual(qp, a.ctypes.data, out.ctypes.data, int(keep_dc), a.shape[0]),
         "ferhip_inverse_residual")
    return out


class MbJob(C.Structure):
    """ferhip_mb_job of include/ferhip.h"""
    _fields_ = [("op", C.c_int32), ("cls", C.c_int32), ("qp", C.c_int32), ("qpc", C.c_int32), ("reconstruct", C.c_int32), ("blk", C.c_int32),
                ("srcY", C.c_int32 * 256), ("srcCb", C.c_int32 * 64), ("srcCr", C.c_int32 * 64),
                ("predY", C.c_int32 * 256), ("predCb", C.c_int32 * 64), ("predCr", C.c_int32 * 64),
                ("lumaLevel", C.c_int32 * 256), ("dc16", C.c_int32 * 16), ("ac16", C.c_int32 * 256), ("cdc", C.c_int32 * 8), ("cac", C.c_int32 * 128)]


class MbResult(C.Structure):
    _fields_ = [("lumaLevel", C.c_int32 * 256), ("dc16", C.c_int32 * 16), ("ac16", C.c_int32 * 256), ("cdc", C.c_int32 * 8), ("cac", C.c_int32 * 128),
                ("recY", C.c_int32 * 256), ("recCb", C.c_int32 * 64), ("recCr", C.c_int32 * 64)]


MBU_QT, MBU_DEC4, MBU_DEC16, MBU_DECC, MBU_SKIP = range(5)


def mb_unit(jobs):
    """ferhip_mb_unit: jobs = list of dicts (fields of ferhip_mb_job, arrays as numpy) -> list of dicts of numpy arrays"""
    lib = load_library()
    n = len(jobs)
    J = (MbJob * n)()
    R = (MbResult * n)()
    for k, j in enumerate(jobs):
        _set_fields(J[k], j)
    lib.ferhip_mb_unit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    _chk(lib.ferhip_mb_unit(J, R, n), "ferhip_mb_unit")
    return [_get_fields(R[k]) for k in range(n)]


def cavlc_blocks(coef, nC, max_num_coeff):
    """ferhip_cavlc_blocks -> (bits [n][64] uint8, nbits [n], total_coeff [n])"""
    lib = load_library()
    c = np.ascontiguousarray(coef, np.int32).reshape(-1, 16)
    n = c.shape[0]
    nc = np.ascontiguousarray(nC, np.int32)
    mx = np.ascontiguousarray(max_num_coeff, np.int32)
    bits = np.zeros((n, 64), np.uint8)
    nb = np.zeros(n, np.uint32)
    tc = np.zeros(n, np.int32)
    lib.ferhip_cavlc_blocks.argtypes = [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 3
    _chk(lib.ferhip_cavlc_blocks(c.ctypes.data, nc.ctypes.data, mx.ctypes.data, n, bits.ctypes.data, nb.ctypes.data, tc.ctypes.data), "ferhip_cavlc_blocks")
    return bits, nb, tc


def cavlc_parse_blocks(bits, bit_pos, nC, max_num_coeff):
    """ferhip_cavlc_parse_blocks: block i read at bit position bit_pos[i] of the stream `bits` (bytes or uint8 array)
    -> (coef [n][16], total_coeff [n] (-1 = malformed), bits_used [n])"""
    lib = load_library()
    b = np.ascontiguousarray(np.frombuffer(bits, np.uint8) if isinstance(bits, (bytes, bytearray)) else bits, np.uint8).reshape(-1)
    pos = np.ascontiguousarray(bit_pos, np.uint64).reshape(-1)
    n = pos.shape[0]
    nc = np.ascontiguousarray(np.broadcast_to(np.asarray(nC, np.int32), (n,)))
    mx = np.ascontiguousarray(np.broadcast_to(np.asarray(max_num_coeff, np.int32), (n,)))
    coef = np.zeros((n, 16), np.int32)
    tc = np.zeros(n, np.int32)
    used = np.zeros(n, np.uint32)
    lib.ferhip_cavlc_parse_blocks.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 3
    _chk(lib.ferhip_cavlc_parse_blocks(b.ctypes.data, b.size, pos.ctypes.data, nc.ctypes.data, mx.ctypes.data, n, coef.ctypes.data, tc.ctypes.data,
                                       used.ctypes.data), "ferhip_cavlc_parse_blocks")
    return coef, tc, used


RES_WRITE, RES_PARSE = 0, 1
RES_BITS_MAX = 2048
_RES_LEVELS = [("lumaLevel", C.c_int32 * 256), ("dc16", C.c_int32 * 16), ("ac16", C.c_int32 * 256), ("cdc", C.c_int32 * 8), ("cac", C.c_int32 * 128)]


class ResNb(C.Structure):
    """ferhip_res_nb of include/ferhip.h: what nC needs from a neighbouring macroblock"""
    _fields_ = [("p_skip", C.c_int32), ("cbp_luma", C.c_int32), ("cbp_chroma", C.c_int32), ("tc_luma", C.c_int32 * 16), ("tc_chroma", C.c_int32 * 8)]


class ResJob(C.Structure):
    """ferhip_res_job of include/ferhip.h"""
    _fields_ = [("op", C.c_int32), ("cls", C.c_int32), ("cbp_luma", C.c_int32), ("cbp_chroma", C.c_int32), ("avail", C.c_int32),
                ("nb", ResNb * 2)] + _RES_LEVELS + [("bit_pos", C.c_uint32), ("nbytes", C.c_uint32), ("bits", C.c_uint8 * RES_BITS_MAX)]


class ResResult(C.Structure):
    _fields_ = [("nbits", C.c_int32), ("tc_luma", C.c_int32 * 16), ("tc_chroma", C.c_int32 * 8)] + _RES_LEVELS + [("bits", C.c_uint8 * RES_BITS_MAX)]


def residual_jobs(jobs):
    """a list of dicts -> a ferhip_res_job array.  Scalars and arrays by field name; nb = (A, B), each None or a dict of
    the fields of ferhip_res_nb; bits = the stream of a PARSE job (bytes or uint8 array; nbytes defaults to its length)"""
    J = (ResJob * len(jobs))()
    for k, j in enumerate(jobs):
        _set_fields(J[k], {f: v for f, v in j.items() if f not in ("nb", "bits")})
        for i, nb in enumerate(j.get("nb", ())):
            _set_fields(J[k].nb[i], nb or {})
        if "bits" in j:
            val = j["bits"]
            a = np.ascontiguousarray(np.frombuffer(val, np.uint8) if isinstance(val, (bytes, bytearray)) else val, np.uint8).reshape(-1)
            if a.size > RES_BITS_MAX:
                raise FerHipError(f"a PARSE job takes at most {RES_BITS_MAX} bytes")
            C.memmove(J[k].bits, a.ctypes.data, a.size)
            if "nbytes" not in j:
                J[k].nbytes = a.size
    return J


def residual_mbs(jobs):
    """ferhip_residual_mbs: jobs = list of dicts (see residual_jobs) -> list of dicts: nbits, tc_luma [16], tc_chroma [8],
    the level arrays (PARSE), bits (uint8 [RES_BITS_MAX], WRITE)"""
    lib = load_library()
    n = len(jobs)
    J = residual_jobs(jobs)
    R = (ResResult * n)()
    lib.ferhip_residual_mbs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    _chk(lib.ferhip_residual_mbs(J, R, n), "ferhip_residual_mbs")
    out = []
    for k in range(n):
        r = {f: np.frombuffer(getattr(R[k], f), np.int32).copy() for f, _ in ResResult._fields_ if f not in ("nbits", "bits")}
        r["nbits"] = int(R[k].nbits)
        r["bits"] = np.frombuffer(R[k].bits, np.uint8).copy()
        out.append(r)
    return out


# ---- the neighbourhood seam (ferhip_intra_mbs, ferhip_mv_mbs): one macroblock at `pos` of a 3 x 2-macroblock picture
INTRA_ENCODE, INTRA_DECODE = 0, 1
MV_DERIVE, MV_PREDICT = 0, 1
NB_W, NB_H, NB_MBS = 48, 32, 6


class NbMb(C.Structure):
    """ferhip_nb_mb of include/ferhip.h: the side information of one macroblock of the little picture"""
    _fields_ = [("mb_type", C.c_int32), ("cbp_luma", C.c_int32), ("cbp_chroma", C.c_int32), ("tc_luma", C.c_int32 * 16), ("tc_chroma", C.c_int32 * 8),
                ("i4mode", C.c_int32 * 16), ("mv", C.c_int32 * 8)]


class IntraJob(C.Structure):
    """ferhip_intra_job of include/ferhip.h"""
    _fields_ = [("op", C.c_int32), ("pos", C.c_int32), ("slice_type", C.c_int32), ("qp", C.c_int32), ("chroma_qp_offset", C.c_int32),
                ("constrained_intra", C.c_int32), ("chroma_mode", C.c_int32), ("prev_flag", C.c_int32 * 16), ("rem_mode", C.c_int32 * 16),
                ("mb", NbMb * NB_MBS), ("Y", C.c_uint8 * (NB_W * NB_H)), ("Cb", C.c_uint8 * (NB_W * NB_H // 4)), ("Cr", C.c_uint8 * (NB_W * NB_H // 4))] + _RES_LEVELS


class IntraResult(C.Structure):
    _fields_ = [("ret", C.c_int32), ("mb_type", C.c_int32), ("cbp_luma", C.c_int32), ("cbp_chroma", C.c_int32), ("chroma_mode", C.c_int32),
                ("mbsize", C.c_int32 * 2), ("i4mode", C.c_int32 * 16), ("prev_flag", C.c_int32 * 16), ("rem_mode", C.c_int32 * 16),
                ("tc_luma", C.c_int32 * 16), ("tc_chroma", C.c_int32 * 8)] + _RES_LEVELS + [
                    ("recY", C.c_int32 * 256), ("recCb", C.c_int32 * 64), ("recCr", C.c_int32 * 64),
                    ("predL", C.c_int32 * 256), ("predCb", C.c_int32 * 64), ("predCr", C.c_int32 * 64)]


class MvJob(C.Structure):
    """ferhip_mv_job of include/ferhip.h"""
    _fields_ = [("op", C.c_int32), ("pos", C.c_int32), ("mb_type", C.c_int32), ("sub_mb_type", C.c_int32 * 4), ("mvd", C.c_int32 * 8), ("mv", C.c_int32 * 8),
                ("mb", NbMb * NB_MBS)]


class MvResult(C.Structure):
    _fields_ = [("mv", C.c_int32 * 8), ("mvd", C.c_int32 * 8), ("fits", C.c_int32)]


def _set_fields(st, fields):
    """a dict into a ctypes structure: scalars and arrays by field name; mb = a list of dicts (or None) per macroblock"""
    for name, val in fields.items():
        if name == "mb":
            for m, nb in enumerate(val):
                if nb:
                    _set_fields(st.mb[m], nb)
        elif isinstance(val, (int, np.integer, bool)):
            setattr(st, name, int(val))
        else:
            fld = getattr(st, name)
            a = np.ascontiguousarray(val, np.uint8 if fld._type_ is C.c_uint8 else np.int32).reshape(-1)
            if a.nbytes != C.sizeof(fld):
                raise FerHipError(f"{name}: {a.size} elements for a field of {len(fld)}")
            C.memmove(fld, a.ctypes.data, a.nbytes)


def _get_fields(st):
    out = {}
    for name, ct in st._fields_:
        v = getattr(st, name)
        out[name] = int(v) if ct is C.c_int32 else np.frombuffer(v, np.int32).copy()
    return out


def nbhd_jobs(jobs, mv=False):
    """a list of dicts -> a ferhip_intra_job (or, mv = True, ferhip_mv_job) array"""
    J = ((MvJob if mv else IntraJob) * len(jobs))()
    for k, j in enumerate(jobs):
        _set_fields(J[k], j)
    return J


def intra_mbs(jobs):
    """ferhip_intra_mbs: jobs = list of dicts with the fields of ferhip_intra_job (Y [32][48], Cb, Cr [16][24] uint8; mb = a list
    of up to six dicts of the fields of ferhip_nb_mb, or None) -> list of dicts of the fields of ferhip_intra_result"""
    lib = load_library()
    n = len(jobs)
    J = nbhd_jobs(jobs)
    R = (IntraResult * n)()
    lib.ferhip_intra_mbs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    _chk(lib.ferhip_intra_mbs(J, R, n), "ferhip_intra_mbs")
    return [_get_fields(R[k]) for k in range(n)]


def mv_mbs(jobs):
    """ferhip_mv_mbs: jobs = list of dicts with the fields of ferhip_mv_job -> list of dicts: mv [8], mvd [8] (x, y per
    quadrant / partition), fits"""
    lib = load_library()
    n = len(jobs)
    J = nbhd_jobs(jobs, mv=True)
    R = (MvResult * n)()
    lib.ferhip_mv_mbs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    _chk(lib.ferhip_mv_mbs(J, R, n), "ferhip_mv_mbs")
    return [_get_fields(R[k]) for k in range(n)]


def frame_nal_blocks_raw(payloads, nal_types, cap=None, fill=0xA5, flags=None):
    """ferhip_frame_nal_blocks on a list of payloads (bytes or uint8 arrays) -> (return code, out [cap] pre-filled with
    `fill`, index [n + 1] of dtype AU).  cap None = room for every payload with every second byte escaped.
    flags not None: through ferhip_frame_nal_blocks_fmt (AU_AVCC: lengths instead of start codes)."""
    lib = load_library()
    n = len(payloads)
    lens = np.array([len(p) for p in payloads], np.uint32)
    stride = max(int(lens.max()) if n else 0, 1)
    src = np.zeros((n, stride), np.uint8)
    for k, p in enumerate(payloads):
        src[k, : len(p)] = np.frombuffer(bytes(p), np.uint8) if not isinstance(p, np.ndarray) else p
    if cap is None:
        cap = int(sum(((int(m) * 3 // 2 + 6 + 15) & ~15) for m in lens))
    out = np.full(max(int(cap), 1), fill, np.uint8)
    idx = np.zeros(n + 1, AU)
    nt = np.ascontiguousarray(nal_types, np.int32)
    if flags is None:
        rc = lib.ferhip_frame_nal_blocks(src.ctypes.data, stride, lens.ctypes.data, nt.ctypes.data, n, out.ctypes.data, int(cap),
                                         idx.ctypes.data)
    else:
        rc = lib.ferhip_frame_nal_blocks_fmt(src.ctypes.data, stride, lens.ctypes.data, nt.ctypes.data, n, int(flags), out.ctypes.data,
                                             int(cap), idx.ctypes.data)
    return rc, out, idx


def rtp_blocks_raw(payloads, nal_types, max_packet, hdr, cap=None, pkts_cap=None, fill=0xA5):
    """ferhip_rtp_blocks on a list of payloads (bytes or uint8 arrays), one slice unit each -> (return code, out [cap]
    pre-filled with `fill`, table [pkts_cap] of dtype RTP_PKT pre-filled with `fill`, index [n + 1] of dtype RTP_AU).
    cap / pkts_cap None = room for every payload with every second byte escaped."""
    lib = load_library()
    n = len(payloads)
    lens = np.array([len(p) for p in payloads], np.uint32)
    stride = max(int(lens.max()) if n else 0, 1)
    src = np.zeros((n, stride), np.uint8)
    for k, p in enumerate(payloads):
        src[k, : len(p)] = np.frombuffer(bytes(p), np.uint8) if not isinstance(p, np.ndarray) else p
    worst = [int(m) * 3 // 2 + 2 for m in lens]  # header byte + escaped payload
    frag = max(int(max_packet) - 14, 1)
    if pkts_cap is None:
        pkts_cap = sum(w // frag + 1 for w in worst)
    if cap is None:
        cap = sum((w // frag + 1) * ((int(max_packet) + 15) & ~15) for w in worst)
    out = np.full(max(int(cap), 1), fill, np.uint8)
    pkts = np.full(max(int(pkts_cap), 1) * RTP_PKT.itemsize, fill, np.uint8).view(RTP_PKT)
    idx = np.zeros(n + 1, RTP_AU)
    h = np.ascontiguousarray(hdr, RTP_HDR)
    nt = np.ascontiguousarray(nal_types, np.int32)
    rc = lib.ferhip_rtp_blocks(src.ctypes.data, stride, lens.ctypes.data, nt.ctypes.data, n, int(max_packet), h.ctypes.data,
                               out.ctypes.data, int(cap), pkts.ctypes.data, int(pkts_cap), idx.ctypes.data)
    return rc, out, pkts, idx


def ts_blocks_raw(payloads, nal_types, hdr, cap=None, fill=0xA5):
    """ferhip_ts_blocks on a list of payloads (bytes or uint8 arrays), one slice unit each -> (return code, out [cap]
    pre-filled with `fill`, index [n + 1] of dtype TS_AU).  cap None = room for every payload with every second byte escaped."""
    lib = load_library()
    n = len(payloads)
    lens = np.array([len(p) for p in payloads], np.uint32)
    stride = max(int(lens.max()) if n else 0, 1)
    src = np.zeros((n, stride), np.uint8)
    for k, p in enumerate(payloads):
        src[k, : len(p)] = np.frombuffer(bytes(p), np.uint8) if not isinstance(p, np.ndarray) else p
    if cap is None:
        cap = sum((((int(m) * 3 // 2 + 26) // 184 + 2) * 188 + 15) & ~15 for m in lens)
    out = np.full(max(int(cap), 1), fill, np.uint8)
    idx = np.zeros(n + 1, TS_AU)
    h = np.ascontiguousarray(hdr, TS_HDR)
    nt = np.ascontiguousarray(nal_types, np.int32)
    rc = lib.ferhip_ts_blocks(src.ctypes.data, stride, lens.ctypes.data, nt.ctypes.data, n, h.ctypes.data, out.ctypes.data, int(cap),
                              idx.ctypes.data)
    return rc, out, idx


def mp4_blocks_raw(payloads, nal_types, m, max_samples, hdr, stride, fill=0xA5):
    """ferhip_mp4_blocks on a list of payloads (bytes or uint8 arrays), one slice unit each, in segments of m consecutive
    payloads -> (return code, out [nseg][stride] pre-filled with `fill`, index [nseg + 1] of dtype MP4_SEG)"""
    lib = load_library()
    n = len(payloads)
    nseg = (n + int(m) - 1) // int(m) if m > 0 else 1
    lens = np.array([len(p) for p in payloads], np.uint32)
    pstride = max(int(lens.max()) if n else 0, 1)
    src = np.zeros((max(n, 1), pstride), np.uint8)
    for k, p in enumerate(payloads):
        src[k, : len(p)] = np.frombuffer(bytes(p), np.uint8) if not isinstance(p, np.ndarray) else p
    out = np.full((max(nseg, 1), max(int(stride), 1)), fill, np.uint8)
    idx = np.zeros(nseg + 1, MP4_SEG)
    h = np.ascontiguousarray(hdr, MP4_HDR)
    nt = np.ascontiguousarray(nal_types, np.int32)
    rc = lib.ferhip_mp4_blocks(src.ctypes.data, pstride, lens.ctypes.data, nt.ctypes.data, n, int(m), int(max_samples), h.ctypes.data,
                               out.ctypes.data, int(stride), idx.ctypes.data)
    return rc, out, idx


def write_ts_psi(pid, pmt_pid, psi_cc, cap=376):
    """ferhip_write_ts_psi -> the PAT and the PMT packet as bytes, b"" where the library refuses"""
    o = np.zeros(max(int(cap), 1), np.uint8)
    n = load_library().ferhip_write_ts_psi(int(pid), int(pmt_pid), int(psi_cc), o.ctypes.data, int(cap))
    return bytes(o[:n])


def unts_blocks_raw(base, runs, pids, cc_expect=None, misalign=0, cap=None, units_cap=None, fill=0xA5):
    """ferhip_unts_blocks: transport stream packets in `base` (bytes or a uint8 array) by the table `runs` (rows of dtype
    TS_RUN) through the device demultiplexer and splitter, stream s listening to pids[s] -> (return code, out [cap]
    pre-filled with `fill`, units [units_cap] of dtype NAL_UNIT with range = the stream, the true unit count, fault
    [nstreams], cc_next [nstreams]).  cc_expect None = no expectation; cap / units_cap None = room for everything."""
    lib = load_library()
    b = base if isinstance(base, np.ndarray) else np.frombuffer(bytes(base), np.uint8)
    rows = np.ascontiguousarray(runs, TS_RUN)
    pid = np.ascontiguousarray(pids, np.uint16)
    nstreams = pid.size
    exp = np.full(nstreams, -1, np.int32) if cc_expect is None else np.ascontiguousarray(cc_expect, np.int32)
    room = int(rows["bytes"].sum()) if rows.size else 0
    if cap is None:
        cap = room + 16 * (room // 4 + 1)
    if units_cap is None:
        units_cap = room // 4 + 1
    out = np.full(max(int(cap), 1), fill, np.uint8)
    units = np.zeros(max(int(units_cap), 1), NAL_UNIT)
    fault, nxt = np.zeros(max(nstreams, 1), np.int32), np.zeros(max(nstreams, 1), np.int32)
    count = C.c_size_t(0)
    rc = lib.ferhip_unts_blocks(b.ctypes.data if b.size else None, b.size, rows.ctypes.data if rows.size else None, rows.size, int(nstreams),
                                int(misalign), pid.ctypes.data if pid.size else None, exp.ctypes.data if exp.size else None, out.ctypes.data,
                                int(cap), units.ctypes.data, int(units_cap), C.byref(count), fault.ctypes.data, nxt.ctypes.data)
    return rc, out, units, count.value, fault[:nstreams], nxt[:nstreams]


def mp4_find_avcc(init):
    """ferhip_mp4_find_avcc -> (offset, length) of the avcC box's content in an initialisation segment, or None"""
    b = np.frombuffer(bytes(init), np.uint8)
    off, n = C.c_size_t(0), C.c_size_t(0)
    rc = load_library().ferhip_mp4_find_avcc(b.ctypes.data if b.size else None, b.size, C.byref(off), C.byref(n))
    return (off.value, n.value) if rc == 0 else None


def unrtp_blocks_raw(base, pkts, nstreams, seq_expect=None, misalign=0, cap=None, units_cap=None, fill=0xA5):
    """ferhip_unrtp_blocks: RTP packets in `base` (bytes or a uint8 array) by the table `pkts` (rows of dtype RTP_PKT) through
    the device depacketiser and splitter -> (return code, out [cap] pre-filled with `fill`, units [units_cap] of dtype
    NAL_UNIT with range = the stream, the true unit count, fault [nstreams], seq_next [nstreams]).  seq_expect None = no
    expectation; cap / units_cap None = room for everything."""
    lib = load_library()
    b = base if isinstance(base, np.ndarray) else np.frombuffer(bytes(base), np.uint8)
    rows = np.ascontiguousarray(pkts, RTP_PKT)
    exp = np.full(nstreams, -1, np.int32) if seq_expect is None else np.ascontiguousarray(seq_expect, np.int32)
    if cap is None:
        cap = int(b.size) + 16 * int(b.size // 3 + rows.size + 1)
    if units_cap is None:
        units_cap = int(b.size // 3 + rows.size + 1)
    out = np.full(max(int(cap), 1), fill, np.uint8)
    units = np.zeros(max(int(units_cap), 1), NAL_UNIT)
    fault, nxt = np.zeros(nstreams, np.int32), np.zeros(nstreams, np.int32)
    count = C.c_size_t(0)
    rc = lib.ferhip_unrtp_blocks(b.ctypes.data if b.size else None, b.size, rows.ctypes.data if rows.size else None, rows.size, int(nstreams),
                                 int(misalign), exp.ctypes.data, out.ctypes.data, int(cap), units.ctypes.data, int(units_cap), C.byref(count),
                                 fault.ctypes.data, nxt.ctypes.data)
    return rc, out, units, count.value, fault, nxt


def srtp_derive(master_key, master_salt):
    """ferhip_srtp_derive (host): the session keys at key derivation rate 0 -> (k_e [16], k_a [20], k_s [14])"""
    lib = load_library()
    k, s, out = np.frombuffer(bytes(master_key), np.uint8), np.frombuffer(bytes(master_salt), np.uint8), np.zeros(50, np.uint8)
    if k.size != 16 or s.size != 14:
        raise FerHipError("srtp_derive: a master key of 16 and a master salt of 14 bytes")
    _chk(lib.ferhip_srtp_derive(k.ctypes.data, s.ctypes.data, out.ctypes.data), "ferhip_srtp_derive")
    out = out.tobytes()
    return out[:16], out[16:36], out[36:]


def srtp_keys(masters):
    """[(master_key, master_salt) or None] -> entries of dtype SRTP_KEY (None: the stream has no key)"""
    keys = np.zeros(len(masters), SRTP_KEY)
    for s, m in enumerate(masters):
        if m is not None:
            keys[s]["master_key"], keys[s]["master_salt"], keys[s]["set"] = np.frombuffer(bytes(m[0]), np.uint8), np.frombuffer(bytes(m[1]), np.uint8), 1
    return keys


def srtp_blocks_raw(op, masters, states, base, pkts, misalign=0, cap=None, fill=0xA5):
    """ferhip_srtp_blocks: the packets in `base` (bytes or a uint8 array) by the table `pkts` (rows of dtype RTP_PKT) through
    the SRTP kernels.  masters: [(master_key, master_salt) or None] per stream, or entries of dtype SRTP_KEY; states:
    [(roc, s_l, set)] per stream -> (return code, out [cap] pre-filled with `fill`, table [npkts + 1] of dtype RTP_PKT,
    status [npkts], the states afterwards as a list of tuples).  cap None = room for everything."""
    lib = load_library()
    b = base if isinstance(base, np.ndarray) else np.frombuffer(bytes(base), np.uint8)
    rows = np.ascontiguousarray(pkts, RTP_PKT)
    keys = masters if isinstance(masters, np.ndarray) else srtp_keys(masters)
    n = len(keys)
    st = np.zeros(n, SRTP_INDEX)
    for s, (roc, s_l, sett) in enumerate(states):
        st[s] = (roc, s_l, sett)
    if cap is None:
        cap = int(sum((int(r["bytes"]) + 10 + 15) & ~15 for r in rows)) + 16
    out = np.full(max(int(cap), 1), fill, np.uint8)
    table = np.full((rows.size + 1) * RTP_PKT.itemsize, fill, np.uint8).view(RTP_PKT)
    status = np.full(max(rows.size, 1), -9, np.int32)
    st_out = np.zeros(n, SRTP_INDEX)
    rc = lib.ferhip_srtp_blocks(int(op), keys.ctypes.data, st.ctypes.data, n, b.ctypes.data if b.size else None, b.size,
                                rows.ctypes.data if rows.size else None, rows.size, int(misalign), out.ctypes.data, int(cap), table.ctypes.data,
                                status.ctypes.data, st_out.ctypes.data)
    return rc, out, table, status[: rows.size], [(int(x["roc"]), int(x["s_l"]), int(x["set"])) for x in st_out]


class Srtp:
    """An SRTP session for nstreams streams on the current device (ferhip_srtp_*): session keys and packet index state in
    device memory.  protect() runs on an encoder context's stream behind its pack_rtp_device(), unprotect() on a
    LiveDecoder's stream in front of its decode_rtp(base_on_device=True)."""

    def __init__(self, nstreams):
        self.lib = load_library()
        self.S = nstreams
        self.h = C.c_void_p()
        _chk(self.lib.ferhip_srtp_create(C.byref(self.h), int(nstreams)), "ferhip_srtp_create")

    def set_key(self, s, master_key, master_salt):
        k, t = np.frombuffer(bytes(master_key), np.uint8), np.frombuffer(bytes(master_salt), np.uint8)
        if k.size != 16 or t.size != 14:
            raise FerHipError("Srtp.set_key: a master key of 16 and a master salt of 14 bytes")
        _chk(self.lib.ferhip_srtp_set_key(self.h, int(s), k.ctypes.data, t.ctypes.data), "ferhip_srtp_set_key")

    def get_index(self, s):
        """-> (roc, s_l, set); waits for the device"""
        roc, s_l, sett = C.c_uint32(), C.c_uint32(), C.c_int()
        _chk(self.lib.ferhip_srtp_get_index(self.h, int(s), C.byref(roc), C.byref(s_l), C.byref(sett)), "ferhip_srtp_get_index")
        return roc.value, s_l.value, sett.value

    def set_index(self, s, roc, s_l, sett=1):
        _chk(self.lib.ferhip_srtp_set_index(self.h, int(s), int(roc), int(s_l), int(sett)), "ferhip_srtp_set_index")

    def protect_raw(self, enc, src_ptr, pkts, npkts, dst_ptr, cap, out_pkts_ptr):
        """ferhip_srtp_protect (pkts: rows of dtype RTP_PKT in host memory) or ferhip_srtp_protect_dev (pkts: an int, the
        table's device address) -> the return code; asynchronous on enc's stream"""
        vp = C.c_void_p
        if isinstance(pkts, (int, np.integer)) or pkts is None:
            return self.lib.ferhip_srtp_protect_dev(self.h, enc.ctx, vp(src_ptr), vp(pkts), int(npkts), vp(dst_ptr), int(cap), vp(out_pkts_ptr))
        rows = np.ascontiguousarray(pkts, RTP_PKT)
        return self.lib.ferhip_srtp_protect(self.h, enc.ctx, vp(src_ptr), rows.ctypes.data if rows.size else None, int(npkts), vp(dst_ptr),
                                            int(cap), vp(out_pkts_ptr))

    def protect(self, enc, src_ptr, pkts, npkts, dst_ptr, cap, out_pkts_ptr):
        _chk(self.protect_raw(enc, src_ptr, pkts, npkts, dst_ptr, cap, out_pkts_ptr), "ferhip_srtp_protect")

    def unprotect_raw(self, dec, base, pkts, dst_ptr, cap, base_on_device=False):
        """ferhip_srtp_unprotect: base = bytes / a uint8 array (host) or a device address -> (return code, table
        [npkts + 1] of dtype RTP_PKT, status [npkts])"""
        rows = np.ascontiguousarray(pkts, RTP_PKT)
        if base_on_device:
            keep, ptr = None, int(base) if base else None
        else:
            keep = base if isinstance(base, np.ndarray) else np.frombuffer(bytes(base), np.uint8)
            ptr = keep.ctypes.data if keep.size else None
        table = np.zeros(rows.size + 1, RTP_PKT)
        status = np.full(max(rows.size, 1), -9, np.int32)
        rc = self.lib.ferhip_srtp_unprotect(self.h, dec.h, C.c_void_p(ptr), int(bool(base_on_device)), rows.ctypes.data if rows.size else None,
                                            rows.size, C.c_void_p(dst_ptr), int(cap), table.ctypes.data, status.ctypes.data)
        return rc, table, status[: rows.size]

    def unprotect(self, dec, base, pkts, dst_ptr, cap, base_on_device=False):
        rc, table, status = self.unprotect_raw(dec, base, pkts, dst_ptr, cap, base_on_device)
        _chk(rc, "ferhip_srtp_unprotect")
        return table, status

    def close(self):
        if self.h:
            self.lib.ferhip_srtp_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def split_nal_blocks_raw(ranges, misalign=0, cap=None, units_cap=None, fill=0xA5):
    """ferhip_split_nal_blocks on a list of byte ranges (bytes or uint8 arrays) -> (return code, out [cap] pre-filled with
    `fill`, units [min(count, units_cap)] of dtype NAL_UNIT, true count).  cap None = room for every range with every unit
    rounded up to 16; units_cap None = one unit per five bytes."""
    lib = load_library()
    n = len(ranges)
    lens = np.array([len(r) for r in ranges], np.uint32)
    stride = max(int(lens.max()) if n else 0, 1)
    src = np.zeros((n, stride), np.uint8)
    for k, r in enumerate(ranges):
        src[k, : len(r)] = np.frombuffer(bytes(r), np.uint8) if not isinstance(r, np.ndarray) else r
    if cap is None:
        cap = int(sum((int(m) // 5 + 1) * 16 + int(m) for m in lens))
    if units_cap is None:
        units_cap = int(sum(int(m) // 5 + 1 for m in lens))
    out = np.full(max(int(cap), 1), fill, np.uint8)
    units = np.zeros(max(int(units_cap), 1), NAL_UNIT)
    count = C.c_size_t(0)
    rc = lib.ferhip_split_nal_blocks(src.ctypes.data, stride, lens.ctypes.data, n, int(misalign), out.ctypes.data, int(cap),
                                     units.ctypes.data, int(units_cap), C.byref(count))
    return rc, out, units[: min(count.value, int(units_cap))], count.value


def split_avcc_blocks_raw(ranges, length_size, misalign=0, cap=None, units_cap=None, fill=0xA5):
    """ferhip_split_avcc_blocks on a list of length-prefixed byte ranges -> (return code, out [cap] pre-filled with `fill`,
    units [min(count, units_cap)] of dtype NAL_UNIT, true count, range_fault [n] int32).  cap None = room for every range
    with every unit rounded up to 16; units_cap None = one unit per two bytes."""
    lib = load_library()
    n = len(ranges)
    lens = np.array([len(r) for r in ranges], np.uint32)
    stride = max(int(lens.max()) if n else 0, 1)
    src = np.zeros((n, stride), np.uint8)
    for k, r in enumerate(ranges):
        src[k, : len(r)] = np.frombuffer(bytes(r), np.uint8) if not isinstance(r, np.ndarray) else r
    if cap is None:
        cap = int(sum((int(m) // 3 + 1) * 16 + int(m) for m in lens))
    if units_cap is None:
        units_cap = int(sum(int(m) // 2 + 1 for m in lens))
    out = np.full(max(int(cap), 1), fill, np.uint8)
    units = np.zeros(max(int(units_cap), 1), NAL_UNIT)
    fault = np.full(max(n, 1), -1, np.int32)
    count = C.c_size_t(0)
    rc = lib.ferhip_split_avcc_blocks(src.ctypes.data, stride, lens.ctypes.data, n, int(misalign), int(length_size), out.ctypes.data,
                                      int(cap), units.ctypes.data, int(units_cap), C.byref(count), fault.ctypes.data)
    return rc, out, units[: min(count.value, int(units_cap))], count.value, fault[:n]


def split_nal_blocks(ranges, misalign=0):
    """The NAL units of every range, split by the kernels of ferhip_decs_decode_dev -> list of (range, nal_unit_type,
    nal_ref_idc, rbsp bytes)"""
    rc, out, units, _ = split_nal_blocks_raw(ranges, misalign)
    _chk(rc, "ferhip_split_nal_blocks")
    return [(int(u["range"]), int(u["nal_type"]), int(u["ref_idc"]), bytes(out[int(u["offset"]): int(u["offset"]) + int(u["bytes"])]))
            for u in units]


def frame_nal_blocks(payloads, nal_types):
    """Annex-B framing (start code, header byte 1 << 5 | type, emulation prevention) of every payload by the kernels of
    ferhip_pack_nal -> list of bytes"""
    rc, out, idx = frame_nal_blocks_raw(payloads, nal_types)
    _chk(rc, "ferhip_frame_nal_blocks")
    return [bytes(out[int(e["offset"]): int(e["offset"]) + int(e["bytes"])]) for e in idx[:-1]]


def mc_sub_mb_parts(ref_i420, width, height, desc):
    """ferhip_mc_sub_mb_parts: desc [n][5] = mb, subMbIdx, subMbPartIdx, mvx, mvy -> (predL [n][4][4], predCb [n][2][2], predCr [n][2][2])"""
    lib = load_library()
    r = np.ascontiguousarray(ref_i420, np.uint8)
    d = np.ascontiguousarray(desc, np.int32).reshape(-1, 5)
    n = d.shape[0]
    pl, pb, pr = np.zeros((n, 4, 4), np.int32), np.zeros((n, 2, 2), np.int32), np.zeros((n, 2, 2), np.int32)
    lib.ferhip_mc_sub_mb_parts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    _chk(lib.ferhip_mc_sub_mb_parts(r.ctypes.data, width, height, d.ctypes.data, n, pl.ctypes.data, pb.ctypes.data, pr.ctypes.data), "ferhip_mc_sub_mb_parts")
    return pl, pb, pr


def block_op(name, blocks, qp=0, flag=None):
    """The per-block entry points of F/quantizationTransform.h / F/scaleTransform.h on n 16-int32 records (device):
    forward_dc_luma_intra, inverse_dc_luma_intra, forward_dc_chroma, inverse_dc_chroma, transform_scan,
    transform_inverse_scan."""
    lib = load_library()
    a = np.ascontiguousarray(blocks, np.int32).reshape(-1, 16)
    out = np.empty_like(a)
    f = getattr(lib, "ferhip_" + name)
    if name == "transform_scan":
        rc = f(a.ctypes.data, out.ctypes.data, int(bool(flag)), a.shape[0])
    elif name == "transform_inverse_scan":
        rc = f(a.ctypes.data, out.ctypes.data, a.shape[0])
    else:
        rc = f(qp, a.ctypes.data, out.ctypes.data, a.shape[0])
    _chk(rc, "ferhip_" + name)
    return out


class Decoder:
    """Streaming decoder for one stream: RBSP_decode(NALunit), NAL unit by NAL unit (ferhip_dec_*)."""

    def __init__(self):
        self.lib = load_library()
        self.h = C.c_void_p()
        _chk(self.lib.ferhip_dec_create(C.byref(self.h)), "ferhip_dec_create")
        self.W = self.H = 0

    def nal(self, nal_unit_type, nal_ref_idc, rbsp):
        """-> decoded picture (uint8 [W*H*3/2]) for slice NAL units, else None"""
        r = np.frombuffer(rbsp, np.uint8)
        got, W, H = C.c_int(), C.c_int(), C.c_int()
        pic = np.empty(self.W * self.H * 3 // 2, np.uint8) if nal_unit_type in (1, 5) else None
        _chk(self.lib.ferhip_dec_nal(self.h, nal_unit_type, nal_ref_idc, r.ctypes.data, len(rbsp),
                                     pic.ctypes.data if pic is not None else None, C.byref(got), C.byref(W), C.byref(H)),
             "ferhip_dec_nal")
        self.W, self.H = W.value, H.value
        return pic if got.value else None

    def close(self):
        if self.h:
            self.lib.ferhip_dec_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LiveDecoder:
    """Live decoder for nstreams streams of one coded picture size (ferhip_decs_*): each decode() call takes whatever
    every stream has now (whole NAL units, see access_units) and decodes all of it together.  A stream's faults come
    back in `status` and do not disturb the other streams."""

    def __init__(self, nstreams, width, height, max_pictures=1):
        self.lib = load_library()
        self.S, self.W, self.H, self.P = nstreams, width, height, max_pictures
        self.fsz = width * height * 3 // 2
        self.cfsz = self.fsz  # a full coded picture; fsz is one slot of `out` (set_display, set_layout)
        self.win, self.layout = (0, 0, width, height), None
        self.h = C.c_void_p()
        _chk(self.lib.ferhip_decs_create(C.byref(self.h), nstreams, width, height, max_pictures), "ferhip_decs_create")

    def get_crop(self, s):
        """ferhip_decs_get_crop: (left, right, top, bottom) of stream s's current SPS in luma samples"""
        c = (C.c_int * 4)()
        _chk(self.lib.ferhip_decs_get_crop(self.h, int(s), c), "ferhip_decs_get_crop")
        return tuple(c)

    def set_display(self, x0, y0, dw, dh):
        """ferhip_decs_set_display: from the next decode() on, every slot of `out` holds the window (x0, y0, dw, dh) of its
        picture, dw*dh*3/2 bytes (self.fsz follows); (0, 0, W, H) restores the full pictures"""
        _chk(self.lib.ferhip_decs_set_display(self.h, int(x0), int(y0), int(dw), int(dh)), "ferhip_decs_set_display")
        self.win = (int(x0), int(y0), int(dw), int(dh))
        self._slot()

    def set_layout(self, fmt, pitch_y, pitch_c):
        """ferhip_decs_set_layout: from the next decode() on (device output only), every slot of `out` holds its picture as
        pitched I420 (Y, Cb, Cr) or NV12 (Y, CbCr): pitch_y * dh + (2 or 1) * pitch_c * dh/2 bytes (self.fsz follows); or in
        a packed format (FMT_YUY2, FMT_UYVY, FMT_BGRA, FMT_RGBA): pitch_y * dh bytes, pitch_y and `out` multiples of 4"""
        _chk(self.lib.ferhip_decs_set_layout(self.h, int(fmt), int(pitch_y), int(pitch_c)), "ferhip_decs_set_layout")
        self.layout = (int(fmt), int(pitch_y), int(pitch_c))
        self._slot()

    def set_csc(self, matrix):
        """ferhip_decs_set_csc: CSC_BT601 (the default) or CSC_BT709 for a FMT_BGRA / FMT_RGBA output layout"""
        _chk(self.lib.ferhip_decs_set_csc(self.h, int(matrix)), "ferhip_decs_set_csc")

    def set_input(self, fmt, length_size=4):
        """ferhip_decs_set_input: from the next decode() / decode_dev() on the chunks are Annex-B (IN_ANNEXB, the default) or
        length-prefixed samples (IN_AVCC, every NAL unit behind its big-endian length of 1, 2 or 4 bytes)"""
        _chk(self.lib.ferhip_decs_set_input(self.h, int(fmt), int(length_size)), "ferhip_decs_set_input")

    def set_config(self, s, record):
        """ferhip_decs_set_config: the SPS and PPS of an AVCDecoderConfigurationRecord (bytes) to stream s, as if they had
        arrived in a chunk -> the return code (0, or the FERHIP_E_* an in-band parameter set would have put in status[s])"""
        r = np.frombuffer(bytes(record), np.uint8)
        return int(self.lib.ferhip_decs_set_config(self.h, int(s), r.ctypes.data if r.size else None, r.size))

    def _slot(self):
        dw, dh = self.win[2:]
        if self.layout is None:
            self.fsz = dw * dh * 3 // 2
        else:
            fmt, py, pc = self.layout
            if fmt in (FMT_YUY2, FMT_UYVY, FMT_BGRA, FMT_RGBA):  # one plane; pitch_c is ignored
                self.fsz = py * dh
                return
            self.fsz = py * dh + (1 if fmt == FMT_NV12 else 2) * pc * (dh // 2)

    def decode(self, chunks, out=None, dev_lens=None):
        """chunks: one bytes or None per stream.  out: [max_pictures][S][W*H*3/2] uint8 (after set_display: [..][dw*dh*3/2]) -- a NumPy array, a DeviceBuffer,
        a torch tensor on the CPU or on the decoder's device -- or None for a new zeroed NumPy array.  -> (out, pictures,
        status): picture k of stream s in out[k, s] for k < pictures[s]; every other slot is left as it was."""
        if len(chunks) != self.S:
            raise FerHipError(f"LiveDecoder.decode: {len(chunks)} chunks for {self.S} streams")
        need = self.P * self.S * self.fsz
        if out is None:
            out = np.zeros((self.P, self.S, self.fsz), np.uint8)
        on_dev = 0
        if isinstance(out, np.ndarray):
            if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
                raise FerHipError("LiveDecoder.decode: out must be a C-contiguous uint8 array of [max_pictures][S][W*H*3/2]")
            ptr = out.ctypes.data
        elif isinstance(out, DeviceBuffer):
            if out.kind != 0 or out.nbytes < need:
                raise FerHipError("LiveDecoder.decode: out must be a device DeviceBuffer of [max_pictures][S][W*H*3/2] bytes")
            ptr, on_dev = out.ptr, 1
        elif isinstance(out, (int, np.integer)):  # a device address of any alignment, max_pictures * S * fsz bytes
            ptr, on_dev = int(out), 1
        else:  # torch tensor
            import torch
            if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < need:
                raise FerHipError("LiveDecoder.decode: out must be a contiguous uint8 tensor of [max_pictures][S][W*H*3/2]")
            if out.is_cuda:
                on_dev = 1
                torch.cuda.current_stream(out.device).synchronize()  # the decoder writes from a stream of its own
            ptr = out.data_ptr()
        pics, status = (C.c_int * self.S)(), (C.c_int * self.S)()
        if dev_lens is None:
            arr = (C.c_char_p * self.S)(*[c if c else None for c in chunks])
            lens = (C.c_size_t * self.S)(*[len(c) if c else 0 for c in chunks])
            _chk(self.lib.ferhip_decs_decode(self.h, arr, lens, C.c_void_p(ptr), on_dev, pics, status), "ferhip_decs_decode")
        else:
            arr = (C.c_void_p * self.S)(*[int(c) if c else None for c in chunks])
            lens = (C.c_size_t * self.S)(*[int(n) if c else 0 for c, n in zip(chunks, dev_lens)])
            _chk(self.lib.ferhip_decs_decode_dev(self.h, arr, lens, C.c_void_p(ptr), on_dev, pics, status), "ferhip_decs_decode_dev")
        return out, list(pics), list(status)

    def decode_rtp(self, base, pkts, out=None, base_on_device=False):
        """ferhip_decs_decode_rtp: RTP packets (RFC 6184, packetization-mode 1) -> (out, pictures, status) like decode().
        base: the bytes that hold the packets (bytes or a uint8 array; an integer device address with base_on_device);
        pkts: rows of dtype RTP_PKT (offset from base, bytes, stream) in arrival order.  out: a host uint8 array or None."""
        if base_on_device:
            ptr_in = int(base)
        else:
            keep = base if isinstance(base, np.ndarray) else np.frombuffer(bytes(base), np.uint8)
            ptr_in = keep.ctypes.data if keep.size else None
        rows = np.ascontiguousarray(pkts, RTP_PKT)
        if out is None:
            out = np.zeros((self.P, self.S, self.fsz), np.uint8)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < self.P * self.S * self.fsz:
            raise FerHipError("LiveDecoder.decode_rtp: out must be a C-contiguous uint8 array of [max_pictures][S][W*H*3/2]")
        pics, status = (C.c_int * self.S)(), (C.c_int * self.S)()
        _chk(self.lib.ferhip_decs_decode_rtp(self.h, C.c_void_p(ptr_in), int(bool(base_on_device)), rows.ctypes.data if rows.size else None,
                                             rows.size, C.c_void_p(out.ctypes.data), 0, pics, status), "ferhip_decs_decode_rtp")
        return out, list(pics), list(status)

    def decode_ts(self, base, runs, pids, out=None, base_on_device=False):
        """ferhip_decs_decode_ts: 188-byte transport stream packets -> (out, pictures, status) like decode().
        base: the bytes that hold the packets (bytes or a uint8 array; an integer device address with base_on_device);
        runs: rows of dtype TS_RUN (offset from base, bytes: a multiple of 188, stream) in arrival order; pids: the PID every
        stream listens to.  out: a host uint8 array or None."""
        if base_on_device:
            ptr_in = int(base)
        else:
            keep = base if isinstance(base, np.ndarray) else np.frombuffer(bytes(base), np.uint8)
            ptr_in = keep.ctypes.data if keep.size else None
        rows = np.ascontiguousarray(runs, TS_RUN)
        pid = np.ascontiguousarray(pids, np.uint16)
        if pid.size != self.S:
            raise FerHipError(f"LiveDecoder.decode_ts: {pid.size} PIDs for {self.S} streams")
        if out is None:
            out = np.zeros((self.P, self.S, self.fsz), np.uint8)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < self.P * self.S * self.fsz:
            raise FerHipError("LiveDecoder.decode_ts: out must be a C-contiguous uint8 array of [max_pictures][S][W*H*3/2]")
        pics, status = (C.c_int * self.S)(), (C.c_int * self.S)()
        _chk(self.lib.ferhip_decs_decode_ts(self.h, C.c_void_p(ptr_in), int(bool(base_on_device)), rows.ctypes.data if rows.size else None,
                                            rows.size, pid.ctypes.data, C.c_void_p(out.ctypes.data), 0, pics, status), "ferhip_decs_decode_ts")
        return out, list(pics), list(status)

    def decode_mp4(self, base, runs, length_size=4, out=None, base_on_device=False):
        """ferhip_decs_decode_mp4: MP4 movie fragments -> (out, pictures, status) like decode().
        base: the bytes that hold the fragments (bytes or a uint8 array; an integer device address with base_on_device,
        which the library refuses for now: FERHIP_E_UNSUP);
        runs: rows of dtype MP4_RUN (offset from base, bytes, stream), each a whole number of top-level boxes, in arrival
        order.  out: a host uint8 array or None."""
        if base_on_device:
            ptr_in = int(base)
        else:
            keep = base if isinstance(base, np.ndarray) else np.frombuffer(bytes(base), np.uint8)
            ptr_in = keep.ctypes.data if keep.size else None
        rows = np.ascontiguousarray(runs, MP4_RUN)
        if out is None:
            out = np.zeros((self.P, self.S, self.fsz), np.uint8)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < self.P * self.S * self.fsz:
            raise FerHipError("LiveDecoder.decode_mp4: out must be a C-contiguous uint8 array of [max_pictures][S][W*H*3/2]")
        pics, status = (C.c_int * self.S)(), (C.c_int * self.S)()
        _chk(self.lib.ferhip_decs_decode_mp4(self.h, C.c_void_p(ptr_in), int(bool(base_on_device)), rows.ctypes.data if rows.size else None,
                                             rows.size, int(length_size), C.c_void_p(out.ctypes.data), 0, pics, status), "ferhip_decs_decode_mp4")
        return out, list(pics), list(status)

    def decode_dev(self, ptrs, lens, out=None):
        """decode() for chunks that lie in device memory on the decoder's device (ferhip_decs_decode_dev): ptrs[s] = device
        address of stream s's chunk (any alignment) or None / 0, lens[s] = its bytes."""
        return self.decode(ptrs, out, dev_lens=lens)

    def timing(self, reset=False):
        """ferhip_decs_timing -> dict of seconds (host split, pack + H2D, parse, reconstruction, device split launches) and
        the bytes the device splitter took"""
        t = (C.c_double * 6)()
        _chk(self.lib.ferhip_decs_timing(self.h, t, int(reset)), "ferhip_decs_timing")
        return dict(zip(("host_split", "pack_h2d", "parse", "recon", "dev_split", "dev_split_bytes"), t))

    def reset_stream(self, s):
        _chk(self.lib.ferhip_decs_reset_stream(self.h, s), "ferhip_decs_reset_stream")

    def close(self):
        if self.h:
            self.lib.ferhip_decs_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def access_units(stream):
    """Split an Annex-B stream (4-byte start codes) into chunks of whole NAL units, each ending with one slice NAL
    unit (what follows the last slice joins the last chunk).  A chunk ends where the decoder's splitter ends that
    slice -- at the zero bytes of the next start code -- so every NAL unit keeps exactly the bytes and the RBSP size it
    has inside the whole stream.  b"".join(access_units(s)) == s.  Host only."""
    chunks, begin, pos, n = [], 0, 0, len(stream)
    while True:
        j = stream.find(b"\x00\x00\x00\x01", pos)
        if j < 0:
            break
        st = j + 4
        ends = [e for e in (stream.find(b"\x00\x00\x00", st), stream.find(b"\x00\x00\x01", st)) if e >= 0]
        en = min(ends) if ends else n
        if en == st:  # an empty NAL unit: the decoder's splitter skips it
            pos = en
            continue
        if en - st == 1:  # a header byte without payload: the decoder's splitter stops there
            break
        if stream[st] & 31 in (1, 5):
            chunks.append(stream[begin:en])
            begin = en
        pos = en
    if begin < n:
        if chunks:
            chunks[-1] += stream[begin:]
        else:
            chunks.append(stream[begin:])
    return chunks


def unescape_nal(nal):
    """Annex-B NAL unit (start code + header + payload) -> (type, ref_idc, rbsp) like getNAL (F/nal.cpp:68-223)"""
    body = nal[4:]
    out = bytearray()
    z = 0
    for b in body[1:]:
        if z >= 2 and b == 3:
            z = 0
            continue
        out.append(b)
        z = z + 1 if b == 0 else 0
    return body[0] & 31, (body[0] >> 5) & 3, bytes(out)


class Y4MReader:
    """LoadY4MHeader / ReadFromY4M (F/fileIO.cpp:228-346): centre crop to multiples of 16."""

    def __init__(self, path):
        self.lib = load_library()
        self.h = C.c_void_p()
        iw, ih, w, h = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _chk(self.lib.ferhip_y4m_open(C.byref(self.h), str(path).encode(), C.byref(iw), C.byref(ih), C.byref(w), C.byref(h)),
             "ferhip_y4m_open")
        self.in_size, self.W, self.H = (iw.value, ih.value), w.value, h.value

    def read(self):
        pic = np.empty(self.W * self.H * 3 // 2, np.uint8)
        rc = self.lib.ferhip_y4m_read(self.h, pic.ctypes.data)
        if rc == 1:
            return None
        _chk(rc, "ferhip_y4m_read")
        return pic

    def close(self):
        if self.h:
            self.lib.ferhip_y4m_close(self.h)
            self.h = C.c_void_p()


def decode_streams(streams, max_pictures, want_pictures=True):
    """decode() for a list of Annex-B byte strings of equal picture size -> (recon [T][S][fsz], pictures, W, H).
    want_pictures=False leaves the decoded pictures on the device (recon is None): what tools/bench_decode.py times."""
    lib = load_library()
    S = len(streams)
    arr = (C.c_char_p * S)(*streams)
    lens = (C.c_size_t * S)(*[len(s) for s in streams])
    pics = (C.c_int * S)()
    W, H = C.c_int(), C.c_int()
    if max_pictures <= 0:
        raise FerHipError("decode_streams: max_pictures must be positive (it sizes the output)")
    out = None
    if want_pictures:  # the output is sized from the first SPS of stream 0 (found by start code, not by splitting the stream)
        at = 0
        while True:
            at = streams[0].find(b"\x00\x00\x01", at)
            if at < 0 or at + 3 >= len(streams[0]):
                raise FerHipError("decode_streams: no sequence parameter set in stream 0")
            at += 3
            if (streams[0][at] & 31) == 7:
                break
        end = streams[0].find(b"\x00\x00\x01", at)
        w, h = _sps_size(streams[0][at + 1:end if end >= 0 else len(streams[0])].replace(b"\x00\x00\x03", b"\x00\x00"))
        out = np.empty((max_pictures, S, w * h * 3 // 2), np.uint8)
    _chk(lib.ferhip_decode_streams(arr, lens, S, out.ctypes.data if want_pictures else None, max_pictures, pics,
                                   C.byref(W), C.byref(H)), "ferhip_decode_streams")
    return out, list(pics), W.value, H.value


def _sps_size(rbsp):
    """width/height from an SPS RBSP (host-side helper for buffer sizing only)."""
    bits = "".join(f"{b:08b}" for b in rbsp)
    pos = [24]

    def ue():
        z = 0
        while bits[pos[0]] == "0":
            z += 1
            pos[0] += 1
        pos[0] += 1
        v = int(bits[pos[0]:pos[0] + z] or "0", 2)
        pos[0] += z
        return (1 << z) - 1 + v

    ue()
    ue()
    poc = ue()
    if poc == 0:
        ue()
    ue()
    pos[0] += 1
    wmb = ue() + 1
    hmu = ue() + 1
    fmo = int(bits[pos[0]])
    return wmb * 16, (2 - fmo) * hmu * 16
