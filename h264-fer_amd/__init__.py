"""h264-fer_amd -- host-side mirror of the fer_h264 encoder interface over libferhip.

The product is the C-ABI shared library ``libferhip.so`` (HIP kernels for gfx950, see
``include/ferhip.h``).  This package only binds it with ctypes so that tests and the
benchmark can drive it the way the reference's GUI drives ``fer_h264::Starter``
(F/fer_h264.cpp:166-216): set parameters, feed pictures, collect the byte stream.
There is no CPU fallback: if the library or a GPU is missing, calls raise.
"""
from .ferhip import (FerHip, FerHipError, Decoder, LiveDecoder, access_units, DeviceBuffer, Y4MReader, decode_streams, unescape_nal, lib_path,  # noqa: F401
                     load_library, mb_unit, cavlc_blocks, cavlc_parse_blocks, residual_mbs, RES_WRITE, RES_PARSE, mc_sub_mb_parts, MBU_QT, MBU_DEC4, MBU_DEC16, MBU_DECC, MBU_SKIP, TUNE_RESOLVE_WGS, TUNE_RESOLVE_GROUP, TUNE_SPECULATE, TUNE_OVERLAP_SORT, RC_CQP, RC_ABR, RC_QUALITY, QM_SSE, QM_SSIM,
                     QUALITY_RING, Quality, NAL_SLICE, NAL_IDR, NAL_AUTO, NAL_NONE, AU_PARAM_SETS, AU, frame_nal_blocks, frame_nal_blocks_raw,
                     NAL_UNIT, SPLIT_PREFIX, split_nal_blocks, split_nal_blocks_raw, FMT_I420, FMT_NV12, FMT_YUY2, FMT_UYVY, FMT_BGRA, FMT_RGBA, CSC_BT601, CSC_BT709, Pic, pic_table,
                     AU_AVCC, IN_ANNEXB, IN_AVCC, split_avcc_blocks_raw, RTP_HDR, RTP_PKT, RTP_AU, rtp_hdr, rtp_blocks_raw, unrtp_blocks_raw,
                     TS_HDR, TS_AU, TS_RUN, TS_PSI, ts_hdr, ts_blocks_raw, unts_blocks_raw, write_ts_psi,
                     MP4_HDR, MP4_SEG, MP4_RUN, mp4_hdr, mp4_data_offset, mp4_blocks_raw, mp4_find_avcc,
                     SRTP_KEY, SRTP_INDEX, SRTP_PROTECT, SRTP_UNPROTECT, Srtp, srtp_derive, srtp_keys, srtp_blocks_raw)
from .synth import gen_frame, gen_frames, crop_to_mb, pad_to_mb  # noqa: F401
from .shard import gops_of_rank, merge_gop_streams, split_nals  # noqa: F401
