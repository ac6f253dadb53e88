/*
 * ferhip.h -- C ABI of libferhip, the MI355X-native drop-in for the per-macroblock hot path
 * of fer_h264 (zoltanmaric/h264-fer).  F/ = fer_h264/fer_h264/ in the reference tree.
 *
 * The reference has no plugin/FFI seam: its NAL/slice driver (F/fer_h264.cpp:55-134) calls
 *     void RBSP_encode(NALunit &nal_unit);      F/rbsp_encoding.h:3, F/rbsp_encoding.cpp:119
 *     int  selectNALUnitType();                 F/ref_frames.h, F/ref_frames.cpp:185
 *     void writeNAL(NALunit nu);                F/nal.h:27, F/nal.cpp:261
 * and communicates through process globals (`frame`, `_qParameter`, `WindowSize`, ...
 * F/h264_globals.h:152-176).  That makes it one stream per process.  This library exports
 *   (1) a context-based ABI in which one context carries what those globals carry for S
 *       independent streams, so that many pictures are in flight on one GPU, and
 *   (2) the legacy global-state entry points (same names, same argument meaning) as thin
 *       shims over a one-stream context: see "legacy seam" below and INTEGRATION.md.
 * All pointers are plain host or device pointers; no C++ or torch types cross the boundary.
 * Every function returns 0 on success or a negative FERHIP_E_* code; nothing falls back to
 * a CPU path.
 */
#ifndef FERHIP_H
#define FERHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FERHIP_E_ARG -1     /* bad argument */
#define FERHIP_E_HIP -2     /* HIP runtime error (no device, out of memory, launch failure) */
#define FERHIP_E_STATE -3   /* call order violated */
#define FERHIP_E_UNSUP -4   /* parameter combination the GPU path does not implement */
#define FERHIP_E_DEVICE -5  /* sticky device-side error flag, see ferhip_status() */

#define FERHIP_NAL_SLICE 1 /* NAL_UNIT_TYPE_NOT_IDR, F/h264_globals.h:84 */
#define FERHIP_NAL_IDR 5   /* NAL_UNIT_TYPE_IDR */
#define FERHIP_NAL_AUTO 0  /* decide like selectNALUnitType() */
#define FERHIP_NAL_NONE -1 /* live contexts: the stream has no picture in this call (see "live encoder" below) */

typedef struct ferhip_ctx ferhip_ctx;

/* Parameters of Starter::PostaviParametre (F/fer_h264.cpp:169-178) minus the frame range. */
typedef struct {
    int qp;          /* _qParameter: QPy of every slice, 10..30 in the reference GUI */
    int basic;       /* BasicInterEncoding: 1 = stage 1 of the search only, counters of the discarded exhaustive pass kept */
    int window;      /* WindowSize: +-window/2 integer search, +-window/16 quarter-pel search */
    int maxdiff;     /* MAXDIFF_SET, -1 = adaptive */
    int intra_every; /* IntraEvery */
} ferhip_params;

/* ---- context ---- */
/* width/height: coded picture size, multiples of 16 (the reference crops to that,
 * F/fileIO.cpp:242-243).  nstreams: independent streams encoded side by side. */
/* width, height: multiples of 16; an encoder context takes pictures of up to (width + 32) * (height + 16) < 2^24 samples
 * (3840x2160 is half of that), larger ones return FERHIP_E_UNSUP */
int ferhip_create(ferhip_ctx **out, int width, int height, int nstreams, const ferhip_params *p);
void ferhip_destroy(ferhip_ctx *c);

/* Device (kind 0) / pinned host (kind 1) memory and synchronous copies for hosts without a HIP binding of their
 * own: device pictures for ferhip_set_frames(host = 0), buffers for ferhip_copy_rbsp, pinned sources for
 * ferhip_upload_frames. */
void *ferhip_mem_alloc(size_t bytes, int kind);
void ferhip_mem_free(void *p, int kind);
int ferhip_mem_copy(void *dst, const void *src, size_t bytes);

/* ---- picture input: replaces ReadFromY4M() filling the global `frame` (F/fileIO.cpp:258) ----
 * I420 pictures of coded size, one per stream, stream-major: [nstreams][W*H*3/2].
 * host = 1: src is host memory (copied H2D); host = 0: src is a device pointer (D2D). */
int ferhip_set_frames(ferhip_ctx *c, const void *src, int host);

/* Asynchronous ingest for many streams (the successor of ReadFromY4M's one-picture read, row f3 of SURVEY.md 8f):
 * ferhip_upload_frames starts the H2D copy of the NEXT pictures ([nstreams][W*H*3/2] in pinned host memory) on the
 * context's copy stream and returns (two uploads may be in flight); ferhip_set_frames_uploaded makes the oldest
 * upload the current picture.  Uploading picture t + 1 before encoding picture t overlaps PCIe with the kernels. */
int ferhip_upload_frames(ferhip_ctx *c, const void *pinned_src);
int ferhip_set_frames_uploaded(ferhip_ctx *c);

/* ---- live encoder: streams that sit out a picture, and slots that change feeds ----
 * The S streams of a context need not tick together.  nal_type[s] = FERHIP_NAL_NONE in ferhip_encode_picture,
 * ferhip_encode_picture_dev or (on input) ferhip_select_nal_type means "stream s has no picture in this call": nothing of
 * that stream is coded or written, nal_type[s] stays FERHIP_NAL_NONE, rbsp_len[s] and the device length are 0, and the
 * stream keeps its reference picture (ferhip_get_recon: its last reconstruction), macroblock types and vectors, frame_num,
 * POC, idr_pic_id, its count of coded pictures (IntraEvery counts a stream's own pictures), brojTipova and the QP of its last
 * picture.  Rate control accounts a stream's previous picture at the first call after it, present or not, exactly once,
 * and chooses no QP for an absent stream.  So a stream's output is a function of the pictures it was given alone: it equals
 * the encode of exactly those pictures, whatever calls it sat out and whatever the other streams did.  A call in which
 * every stream is FERHIP_NAL_NONE returns 0 and changes nothing (no quality row either).  The AUTO decision's SAD
 * read-back is still the only host synchronisation per picture; absent streams take no part in it.
 *
 * ferhip_set_frames_live: ferhip_set_frames for the streams with present[s] != 0 only.  The slots of the other streams in
 * src ([nstreams][W*H*3/2]) are never read -- a host buffer with holes, or the unwritten slots of ferhip_decs_decode's
 * device output -- and none of their bytes cross the bus.
 * ferhip_upload_frames_live: the same for the double-buffered pinned ingest; the mask stays with the staging slot until
 * ferhip_set_frames_uploaded makes that upload current.
 * ferhip_reset_stream: slot s becomes what it is in a freshly created context (a new feed takes the slot): no reference
 * picture, frame_num / POC / idr_pic_id / picture count cleared -- so ferhip_set_rate may set base[s] again --, macroblock
 * types zeroed, rate settings back to CQP at params.qp with base = params.qp, controller state, brojTipova, sticky
 * status bits and the quality `picture` index cleared.  The other slots are untouched.  Ordered on the context's stream
 * behind the slot's last picture; nothing waits.  FERHIP_E_ARG for s outside 0..S-1. */
int ferhip_set_frames_live(ferhip_ctx *c, const void *src, int host, const uint8_t *present);
int ferhip_upload_frames_live(ferhip_ctx *c, const void *pinned_src, const uint8_t *present);
int ferhip_reset_stream(ferhip_ctx *c, int s);

/* ---- display size: pictures of any even size ----
 * The reference answers a picture size that is no multiple of 16 by cropping the source (F/fileIO.cpp:242-243); this section
 * is what every other H.264 encoder does instead: the picture is padded to the macroblock grid and the SPS crops it back.
 * The context is still created at the coded size W x H.  ferhip_set_display_size(dw, dh): dw, dh even, W - 16 < dw <= W,
 * H - 16 < dh <= H, else FERHIP_E_ARG; FERHIP_E_STATE once the context has coded a picture.  The default is (W, H), and
 * calling it with (W, H) is the default again: a context on which none of the calls below is made behaves as before, byte
 * for byte.
 * With dw < W or dh < H, ferhip_write_sps -- and so ferhip_encode_streams and FERHIP_AU_PARAM_SETS -- writes
 * frame_cropping_flag = 1 and the offsets left ue(0), right ue((W - dw) / 2), top ue(0), bottom ue((H - dh) / 2), in units of
 * two luma samples (4:2:0, frame_mbs_only), then vui_parameters_present_flag = 0; every bit in front of the flag is as before.
 *
 * ferhip_set_frames_display: src = [nstreams][dw*dh*3/2] I420 at the display size, host (host = 1) or device memory of any
 * alignment (dw*dh*3/2 is in general no multiple of 16).  Each plane of size (pw, ph) = (dw, dh) for luma, (dw/2, dh/2) for
 * chroma is padded by edge replication, on the device, in one launch:
 *     coded sample (x, y) = source sample (min(x, pw - 1), min(y, ph - 1)).
 * present (NULL = every stream) has the meaning it has in ferhip_set_frames_live: the slots of absent streams are not
 * read (of a device source at most the rest of the aligned 4-byte word that holds a neighbouring picture's first or last
 * byte is fetched, and dropped), none of their bytes cross the bus and their pictures in the context are untouched.
 * ferhip_upload_frames_display: the same for the double-buffered pinned ingest (present may be NULL); the staging slot
 * remembers that it holds display-size pictures and ferhip_set_frames_uploaded pads them.  Display-size and coded-size
 * uploads may alternate.
 * ferhip_get_recon_display: the top-left dw x dh window of the last reconstruction, [nstreams][dw*dh*3/2].
 * ferhip_set_frames, ferhip_upload_frames and ferhip_get_recon keep working at the coded size on such a context (a caller
 * may pad for itself), and ferhip_encode_streams keeps taking coded-size pictures.  Quality measurement (ferhip_quality),
 * FERHIP_RC_QUALITY and the AUTO IDR decision (ferhip_select_nal_type) run over the whole coded picture, the padding
 * included: the padding is part of what is coded. */
int ferhip_set_display_size(ferhip_ctx *c, int dw, int dh);
int ferhip_set_frames_display(ferhip_ctx *c, const void *src, int host, const uint8_t *present /* NULL = every stream */);
int ferhip_upload_frames_display(ferhip_ctx *c, const void *pinned_src, const uint8_t *present /* NULL = every stream */);
int ferhip_get_recon_display(ferhip_ctx *c, void *dst, int host);

/* ---- pictures by descriptor: a pointer and a row pitch per stream and plane, I420 or NV12 ----
 * A feed seldom owns one packed [nstreams][w*h*3/2] array: a capture card, a hardware decoder, a compositor or another
 * library's frame pool hands over one allocation per stream or per plane, rows at a pitch larger than the width (256-byte
 * aligned on most producers), NV12 more often than I420.  A ferhip_pic names one such picture where it lies, in device
 * memory on the context's device; pics is a host array of nstreams of them, read before the call returns.
 * Pictures have the context's display size (dw, dh): (W, H) unless ferhip_set_display_size was called.  A luma row is dw
 * bytes; a chroma row is dw/2 bytes (I420), or dw bytes of CbCr pairs (NV12, dh/2 rows of them).  Row r of plane k starts
 * at plane[k] + r * pitch[k]; bases and pitches may have any value, odd ones included, as long as pitch[k] >= the row's bytes.
 *
 * ferhip_set_pictures fills the current picture set exactly as ferhip_set_frames_display would fill it from the same
 * samples packed tight, the edge-replication padding to W x H included, in one launch for all streams and planes.  A
 * stream with plane[0] == NULL is absent in the sense of ferhip_set_frames_live: nothing of it is read -- the rest of its
 * descriptor is not looked at either -- and its pictures in the context are untouched.  FERHIP_E_ARG for an unknown
 * format, and in a present stream for a pitch below the row's bytes, a NULL chroma plane or reserved != 0.  The pictures
 * must be complete when the call is made, as for ferhip_set_frames(host = 0): the kernel is ordered on the context's
 * stream, not behind the producer's.
 * What is read: of a source row only the aligned 4-byte words that hold at least one byte of the row are fetched, so
 * nothing outside a row is touched except the rest of the word that holds the row's first or last byte (fetched, and
 * dropped).  The bytes between a row's end and the next row are otherwise never read; a row of NV12 chroma is read once.
 *
 * ferhip_get_recon_pictures is the way back: the top-left dw x dh window of each present stream's last reconstruction is
 * written through the descriptor (ferhip_get_recon_display in the caller's own layout).  Only bytes that belong to a row
 * are written: the bytes between a row's end and the next row, and every byte around the planes, are left as they were.
 * It waits for the copy, like ferhip_get_recon_display, and like it delivers whatever the reference picture set holds
 * (zeros in a new context) when the context has not coded a picture yet. */
#define FERHIP_FMT_I420 0 /* plane[0] = Y, plane[1] = Cb, plane[2] = Cr */
#define FERHIP_FMT_NV12 1 /* plane[0] = Y, plane[1] = CbCr interleaved, plane[2] ignored */
typedef struct ferhip_pic {
    const void *plane[3]; /* device pointers, any byte alignment; plane[0] == NULL: the stream is absent */
    uint32_t pitch[3];    /* bytes from one row to the next, >= the row's bytes, otherwise any value (odd included) */
    uint32_t reserved;    /* 0 */
} ferhip_pic;
int ferhip_set_pictures(ferhip_ctx *c, const ferhip_pic *pics /* host, [nstreams] */, int format);
int ferhip_get_recon_pictures(ferhip_ctx *c, const ferhip_pic *pics /* host, [nstreams]; planes are written */, int format);

/* ---- packed 4:2:2 and 32-bit RGB pictures, converted on the device in the same pass ----
 * A capture card delivers packed 4:2:2, a compositor, a renderer or a tensor pipeline 32-bit RGB, and a display or a model
 * wants RGB back.  ferhip_set_pictures, ferhip_get_recon_pictures and ferhip_decs_set_layout take four more formats, all
 * "packed": one plane, so only plane[0] and pitch[0] of a descriptor are looked at.  plane[0] and pitch[0] must be multiples
 * of 4 and pitch[0] >= the row's bytes (2*dw or 4*dw), reserved must be 0, else FERHIP_E_ARG; plane[0] == NULL still means
 * that the stream is absent.  dw is even, so a row is a whole number of aligned 4-byte words: exactly the bytes of the rows
 * are read (in) or written (out), pitch gaps and surroundings are never touched.  The format values 2, 3, 6, 7, 10 and -1
 * are not formats and stay FERHIP_E_ARG (2, 7 and -1 are pinned as invalid by the tests of the planar formats).
 *
 * The conversion, in integers; all shifts are arithmetic (floor), (dw, dh) is the display size.  Limited range only.
 *   4:2:2 in   Y(x, y) = the luma byte.  With c(p, y) the Cb (or Cr) byte of pixel pair p in row y:
 *              C(p, q) = (c(p, 2q) + c(p, 2q + 1) + 1) >> 1
 *   RGB in     (A is ignored)   Y(x, y)  = 16  + ((yr*R + yg*G + yb*B + 128) >> 8)
 *              Rs, Gs, Bs = the sums of R, G, B over the 2x2 block (2p..2p+1, 2q..2q+1)
 *                               Cb(p, q) = 128 + ((br*Rs + bg*Gs + bb*Bs + 512) >> 10)
 *                               Cr(p, q) = 128 + ((rr*Rs + rg*Gs + rb*Bs + 512) >> 10)
 *              (yr, yg, yb | br, bg, bb | rr, rg, rb) = (66, 129, 25 | -38, -74, 112 | 112, -94, -18)   FERHIP_CSC_BT601
 *                                                       (47, 157, 16 | -26, -86, 112 | 112, -102, -10)  FERHIP_CSC_BT709
 *              No clamp is needed: Y stays in 16..235 and chroma in 16..240 for every input.
 *   padding    then as everywhere: coded sample (x, y) of a plane = converted sample (min(x, pw - 1), min(y, ph - 1)), so
 *              ferhip_set_pictures fills the picture set exactly as ferhip_set_frames_display would from the converted I420
 *              picture packed tight.  Quality measurement, the AUTO IDR decision and rate control see the converted pictures.
 *   4:2:2 out  the luma byte = Y(x, y); rows 2q and 2q + 1 both carry C(p, q).  So out followed by in is the identity.
 *   RGB out    chroma is nearest, C(x >> 1, y >> 1).  With c = Y - 16, d = Cb - 128, e = Cr - 128:
 *                               R = clip255((298*c + rv*e + 128) >> 8)
 *                               G = clip255((298*c + gu*d + gv*e + 128) >> 8)
 *                               B = clip255((298*c + bu*d + 128) >> 8),   A = 255
 *              (rv, gu, gv, bu) = (409, -100, -208, 516) FERHIP_CSC_BT601, (459, -55, -136, 541) FERHIP_CSC_BT709
 * ferhip_set_csc chooses the matrix that ferhip_set_pictures and ferhip_get_recon_pictures of the context use in BGRA and
 * RGBA, ferhip_decs_set_csc the one of a live decoder's RGB output layout; it applies from the next call on, has no effect
 * on the other formats, and any other value is FERHIP_E_ARG.  The SPS carries no VUI, so a stream does not announce its
 * matrix: a receiver has to be told.
 * ferhip_decs_set_layout with a packed format: a slot is pitch_y * dh bytes and pitch_c is ignored.  pitch_y must be a
 * multiple of 4 and >= the row bytes of the window current at the decode call, and out must be device memory at a multiple
 * of 4: else that decode call returns FERHIP_E_ARG before it takes anything.
 * Host-memory sources, full-range matrices and other chroma filters are not provided. */
#define FERHIP_FMT_YUY2 4 /* one plane, 2*dw bytes per row: Y0 Cb Y1 Cr per pixel pair */
#define FERHIP_FMT_UYVY 5 /* one plane, 2*dw bytes per row: Cb Y0 Cr Y1 */
#define FERHIP_FMT_BGRA 8 /* one plane, 4*dw bytes per row: B G R A per pixel */
#define FERHIP_FMT_RGBA 9 /* one plane, 4*dw bytes per row: R G B A */
#define FERHIP_CSC_BT601 0 /* default */
#define FERHIP_CSC_BT709 1
int ferhip_set_csc(ferhip_ctx *c, int matrix);

/* ---- RBSP_encode for slice NAL units (F/rbsp_encoding.cpp:139-323) ----
 * nal_type[s]: FERHIP_NAL_IDR / FERHIP_NAL_SLICE / FERHIP_NAL_AUTO / FERHIP_NAL_NONE per stream on input, the
 * type actually used on output (NULL = AUTO for all).  After the call the picture buffers
 * hold the reconstruction (like the reference's `frame`) and become the reference picture.
 * rbsp (host): nstreams * rbsp_stride bytes; rbsp_len[s] receives NumBytesInRBSP.
 * frame_num and pic_order_cnt_lsb wrap modulo 512 / 1024 (the field widths of the SPS): the 513th picture of a run
 * without an IDR picture carries frame_num 0 again.  This is the one place where the encoder does not follow the reference:
 * its bit writer adds a value into the buffer without masking it (writeRawBits, F/rbsp_IO.cpp:123-127), so past 512
 * pictures without an IDR picture the reference's own writer corrupts the slice header.  An IDR picture takes
 * idr_pic_id + 1 only directly behind an IDR picture; that test reads the counter before the wrap, as the reference's does. */
int ferhip_encode_picture(ferhip_ctx *c, int *nal_type, uint8_t *rbsp, size_t rbsp_stride, uint32_t *rbsp_len);

/* selectNALUnitType() (F/ref_frames.cpp:185-234) for the pictures set by ferhip_set_frames: IDR for the
 * first picture, every IntraEvery-th picture and when the luma SAD against the reference picture
 * exceeds 16 per pixel (evaluated on the device); writes FERHIP_NAL_IDR / FERHIP_NAL_SLICE per stream.  A stream whose
 * entry holds FERHIP_NAL_NONE on input has no picture: it is left out and keeps FERHIP_NAL_NONE. */
int ferhip_select_nal_type(ferhip_ctx *c, int *nal_type_out);

/* Same, but leaves the RBSP in device memory (no D2H): *d_rbsp receives the device base,
 * words are big-endian bit order, stream s starts at byte s * *stride. */
int ferhip_encode_picture_dev(ferhip_ctx *c, int *nal_type, const uint8_t **d_rbsp, size_t *stride,
                              const uint32_t **d_rbsp_len);

/* RBSP of the last picture to caller buffers, asynchronously on the context's stream (ordered before the next
 * picture reuses the device buffer): bytes_per_stream bytes per stream to dst + s * dst_stride, the lengths to
 * len_dst[S].  host = 1: dst / len_dst are host memory (pinned for a truly asynchronous copy), else device memory. */
int ferhip_copy_rbsp(ferhip_ctx *c, void *dst, size_t dst_stride, size_t bytes_per_stream, uint32_t *len_dst, int host);
/* waits for everything the context has enqueued */
int ferhip_sync(ferhip_ctx *c);

/* reconstruction of the last encoded picture, [nstreams][W*H*3/2]; host = 1 copies D2H */
int ferhip_get_recon(ferhip_ctx *c, void *dst, int host);

/* SPS / PPS RBSP (F/headers_and_parameter_sets.cpp:305-391,478-513) and NAL framing with
 * emulation prevention (F/nal.cpp:261-299); host-side, byte-serial. */
size_t ferhip_write_sps(ferhip_ctx *c, uint8_t *rbsp, size_t cap);
size_t ferhip_write_pps(ferhip_ctx *c, uint8_t *rbsp, size_t cap);  /* pic_init_qp = 14 + params.qp; see ferhip_write_pps_stream */
size_t ferhip_write_nal(int nal_ref_idc, int nal_type, const uint8_t *rbsp, size_t n, uint8_t *out);

/* ---- NAL framing on the device: the coded pictures as Annex-B NAL units with an offset table ----
 * For every stream that coded a picture in the context's last ferhip_encode_picture[_dev] call the output holds exactly what
 * ferhip_write_nal(1, type, rbsp, len, ...) writes: 00 00 00 01, the header byte 1 << 5 | type (5 for an I picture, 1 for a
 * P picture, taken from the device's own slice headers) and the payload with its emulation prevention bytes.  With
 * FERHIP_AU_PARAM_SETS the framed SPS and the stream's own PPS (ferhip_write_pps_stream) stand in front of every IDR
 * unit, and the three form one entry.
 * Layout: entries in stream order, every offset a multiple of 16; the bytes between an entry's end and the next offset
 * are not written.  index[s] = (offset, bytes, NAL unit type of the slice); a stream without a picture (FERHIP_NAL_NONE)
 * has bytes 0 and nal_type 0.  index[S].offset = the total (the end of the last entry rounded up to 16), index[S].bytes =
 * the number of entries written.
 * Overflow is not an error: the index always holds the true offsets and sizes, an entry is written only if it ends within
 * cap together with its rounding to 16 (offset + bytes rounded up to 16 <= cap: an entry owns whole 16-byte slots, so a
 * buffer one byte short of the total never holds the last entry), and no byte at or beyond cap is touched.  ferhip_pack_nal then still returns 0 -- compare index[S].offset with cap --
 * and ferhip_fetch_nal fills h_index and returns FERHIP_E_ARG.
 * Call order as for ferhip_copy_rbsp: behind the last picture, before the next one.  FERHIP_E_STATE before the context's
 * first picture; after a call in which every stream was absent the total is 0.  Packing changes nothing the encoder reads
 * (RBSP, lengths, rate and quality state) and may be repeated.  A slot that ferhip_reset_stream cleared has no entry until its
 * next picture.
 * ferhip_pack_nal: device to device (d_dst 16-byte aligned, d_index 8-byte aligned, else FERHIP_E_ARG), asynchronous on the
 * context's stream; nothing waits, except that a context's first call, and its first call with the flag, allocate their
 * buffers and wait for the device once.  ferhip_fetch_nal: the same bytes in host memory; it waits, reads the index, grows an
 * internal device buffer when needed and makes exactly one device-to-host copy of `total` bytes.
 * The parameter sets are built on the host and kept in a small device table that exists only once the flag was used; a
 * stream's row is sent again only when it can have changed (its first use, ferhip_set_rate before the stream's first
 * picture, ferhip_reset_stream).
 *
 * Length-prefixed framing.  With FERHIP_AU_AVCC (alone or with FERHIP_AU_PARAM_SETS) every NAL unit of an entry is written
 * as a 4-byte big-endian length N followed by the N bytes of the unit, N = 1 header byte + the payload with its emulation
 * prevention bytes: the NAL framing of ISO/IEC 14496-15 with lengthSizeMinusOne = 3, what an MP4, FLV or Matroska sample
 * holds.  The length stands where the start code 00 00 00 01 stands, and both are four bytes, so nothing else changes:
 * index[] of a pack with FERHIP_AU_AVCC equals index[] of the pack of the same picture without it, entry for entry
 * (offset, bytes, nal_type, and index[S]), the 16-byte slot rule and the overflow rule are the same, and the two outputs
 * differ only in those 4-byte prefixes.  With FERHIP_AU_PARAM_SETS the SPS, the stream's PPS and the IDR slice each carry
 * their own length inside the one entry.  A context may be packed in both framings alternately, as it may be packed
 * repeatedly.  (The flag's value is 4: the value 2 was already pinned as an invalid flag by the suite.)
 * ferhip_write_avcc_config (host): the AVCDecoderConfigurationRecord of stream s for the avcC box -- configurationVersion 1,
 * AVCProfileIndication, profile_compatibility and AVCLevelIndication = the first three bytes of the SPS RBSP, 0xFC | 3
 * (lengthSizeMinusOne = 3), 0xE0 | 1 (one SPS), the u16 length of the SPS NAL unit and the unit (header byte + escaped
 * payload: what ferhip_write_nal(1, 7, ...) writes behind its start code), 1 (one PPS), the u16 length of the PPS NAL unit
 * of ferhip_write_pps_stream(c, s, ...) and the unit.  Returns the bytes written, 0 if cap is too small or s is out of
 * range.  It follows ferhip_set_display_size and ferhip_set_rate exactly as the SPS and PPS writers do. */
#define FERHIP_AU_PARAM_SETS 1
#define FERHIP_AU_AVCC 4
typedef struct { uint64_t offset; uint32_t bytes; int32_t nal_type; } ferhip_au; /* 16 bytes */
int ferhip_pack_nal(ferhip_ctx *c, int flags, void *d_dst, size_t cap, ferhip_au *d_index /* [S+1] */);
int ferhip_fetch_nal(ferhip_ctx *c, int flags, void *h_dst, size_t cap, ferhip_au *h_index /* [S+1] */);
/* Known-answer surface, context-free like ferhip_cavlc_blocks: n host payloads [n][stride] of lens[n] bytes and NAL unit type
 * nal_type[n], framed by the same kernels (a payload of length 0 gives its five prefix bytes); out (host, cap bytes: bytes
 * the kernels do not write keep the caller's values) and index[n + 1] as above.  n <= 65535. */
int ferhip_frame_nal_blocks(const uint8_t *payloads, size_t stride, const uint32_t *lens, const int32_t *nal_type,
                            size_t n, uint8_t *out, size_t cap, ferhip_au *index /* [n+1] */);
/* ... with flags: 0 or FERHIP_AU_AVCC (a payload of length 0 then gives 00 00 00 01 and its header byte); any other bit:
 * FERHIP_E_ARG. */
int ferhip_frame_nal_blocks_fmt(const uint8_t *payloads, size_t stride, const uint32_t *lens, const int32_t *nal_type,
                                size_t n, int flags, uint8_t *out, size_t cap, ferhip_au *index /* [n+1] */);
size_t ferhip_write_avcc_config(ferhip_ctx *c, int s, uint8_t *out, size_t cap);

/* ---- RTP packets on the device: the coded pictures in the payload format of RFC 6184, packetization-mode 1 ----
 * The third framing of the same pictures, for the wire: every NAL unit becomes datagrams of at most max_packet bytes.
 * Let P = max_packet (the whole datagram with its 12-byte RTP header, 80 <= P <= 65535), B = P - 12 and F = B - 2.
 * A stream that coded a picture in the context's last ferhip_encode_picture[_dev] call has one access unit.  Its units, in
 * order: with FERHIP_AU_PARAM_SETS and in front of an IDR slice only, the SPS and the stream's own PPS; then the slice.  A
 * unit is its header byte h (1 << 5 | type) and the payload with its emulation prevention bytes: the N bytes that
 * ferhip_write_nal writes behind the start code.  The packets:
 *   parameter sets   one STAP-A packet: the byte 0x20 | 24, then for the SPS and then the PPS a big-endian u16 size and the
 *                    unit.  It always fits: a context's two parameter sets are at most 63 bytes with their start codes.
 *   slice, N <= B    one single-NAL packet whose payload is the unit;
 *   slice, N > B     n = ceil((N - 1) / F) >= 2 FU-A packets; packet k carries the indicator (h & 0xE0) | 28, the FU header
 *                    S << 7 | E << 6 | (h & 0x1F) with S on k = 0 and E on k = n - 1, and the unit's bytes
 *                    [1 + k F, 1 + min((k + 1) F, N - 1)).
 * RTP header of every packet: 0x80, M << 7 | payload_type, seq + (index of the packet within its stream) mod 65536,
 * timestamp, ssrc, all big-endian; M = 1 on the last packet of the stream's access unit and on no other.
 * The library keeps no RTP state: hdr[s] (host, S entries, those of streams without a picture included) is read before the
 * call returns, and the caller advances seq by index[s].npkts, which it reads anyway to send the packets; a repeated call
 * with the same hdr gives the same bytes.
 * Layout: stream order, then packet order; every packet starts at a multiple of 16, and the bytes between a packet's end
 * and the next multiple of 16 are not written.  pkts[k] = (offset, bytes, stream).  index[s] = (offset of the stream's
 * first packet, sum of its packets' sizes each rounded up to 16, NAL unit type of the slice, first_pkt, npkts); a stream
 * without a picture has zeros.  index[S] = (total bytes, number of streams written, 0, total packets, 0).
 * Overflow is ferhip_pack_nal's rule, per stream: the index always holds the true values; a stream's packets and table
 * rows are written all or none, only if they end within both cap (offset + bytes <= cap) and pkts_cap (first_pkt + npkts
 * <= pkts_cap); nothing at or beyond either is touched.  ferhip_pack_rtp then still returns 0, ferhip_fetch_rtp fills
 * h_index and returns FERHIP_E_ARG.
 * FERHIP_E_ARG: payload_type > 127, reserved != 0, P out of range, a flag other than FERHIP_AU_PARAM_SETS, a null c, hdr
 * or index, a null buffer with a cap, and for ferhip_pack_rtp a d_dst not aligned to 16 or d_pkts / d_index not aligned to
 * 8.  FERHIP_E_STATE before the context's first picture.
 * ferhip_pack_rtp: device to device, asynchronous on the context's stream; it waits for nothing except a context's first
 * call's allocations.  ferhip_fetch_rtp: the same bytes and table in host memory; it waits once for the index and once for
 * the two copies.  Packing changes nothing the encoder reads and may be mixed with the other framings.
 * ferhip_rtp_blocks: known-answer surface with the conventions of ferhip_frame_nal_blocks: host payloads, one slice unit
 * each (no parameter sets), hdr[n], n <= 65535, and bytes and rows the kernels do not write keep the caller's values.
 * ferhip_write_sdp_fmtp (host): the format parameters of stream s for an SDP a=fmtp line,
 * profile-level-id=%02x%02x%02x;packetization-mode=1;sprop-parameter-sets=<base64 SPS unit>,<base64 PPS unit> -- the hex
 * bytes are the first three bytes of the SPS RBSP, the units those of ferhip_write_avcc_config, base64 with padding.
 * Returns the length (out is 0-terminated behind it), 0 if cap is too small or s is out of range. */
typedef struct { uint32_t ssrc, timestamp; uint16_t seq; uint8_t payload_type, reserved; } ferhip_rtp_hdr; /* 12 bytes, host */
typedef struct { uint64_t offset; uint32_t bytes; uint32_t stream; } ferhip_rtp_pkt;                        /* 16 bytes */
typedef struct { uint64_t offset; uint32_t bytes; int32_t nal_type; uint32_t first_pkt, npkts; } ferhip_rtp_au; /* 24 bytes */
int ferhip_pack_rtp(ferhip_ctx *c, int flags, int max_packet, const ferhip_rtp_hdr *hdr /* host [S] */, void *d_dst, size_t cap,
                    ferhip_rtp_pkt *d_pkts, size_t pkts_cap, ferhip_rtp_au *d_index /* [S+1] */);
int ferhip_fetch_rtp(ferhip_ctx *c, int flags, int max_packet, const ferhip_rtp_hdr *hdr, void *h_dst, size_t cap,
                     ferhip_rtp_pkt *h_pkts, size_t pkts_cap, ferhip_rtp_au *h_index);
int ferhip_rtp_blocks(const uint8_t *payloads, size_t stride, const uint32_t *lens, const int32_t *nal_type, size_t n,
                      int max_packet, const ferhip_rtp_hdr *hdr /* [n] */, uint8_t *out, size_t cap, ferhip_rtp_pkt *pkts,
                      size_t pkts_cap, ferhip_rtp_au *index /* [n+1] */);
size_t ferhip_write_sdp_fmtp(ferhip_ctx *c, int s, char *out, size_t cap);

/* ---- Transport stream packets on the device: the coded pictures in the MPEG-2 transport stream of ISO/IEC 13818-1 ----
 * The fourth framing of the same pictures: what UDP multicast, SRT, HLS segments and DVB / ATSC carry.  A stream that coded
 * a picture in the context's last ferhip_encode_picture[_dev] call has one access unit, one PES packet, in 188-byte packets.
 * Elementary-stream bytes E: an access unit delimiter 00 00 00 01 09 a (a = 0x10 for an I picture, slice NAL unit type 5,
 * and 0x30 for a P picture), then the stream's entry exactly as ferhip_pack_nal writes it with flags & FERHIP_AU_PARAM_SETS.
 * PES packet = 14 header bytes + E, L = 14 + |E| bytes: 00 00 01 E0, 00 00 (PES_packet_length 0, as video in a transport
 * stream may), 84 (data_alignment_indicator), 80 (PTS only), 05, then the PTS: 0x21 | ((pts >> 29) & 0x0E), (pts >> 22) & 0xFF,
 * 0x01 | ((pts >> 14) & 0xFE), (pts >> 7) & 0xFF, 0x01 | ((pts << 1) & 0xFE).  No DTS: the encoder never reorders.
 * Packets: 47, PUSI << 6 | pid >> 8, pid & 0xFF, afc << 4 | cc.  n = 1 if L <= 176, else 1 + ceil((L - 176) / 184); cc of
 * packet k is (hdr.cc + k) & 15, counting the PES-carrying packets only.
 *   packet 0       PUSI = 1, afc = 3; adaptation field: length byte a0 = 7 if L >= 176, else 183 - L; the flags byte
 *                  0x10 | (I picture ? 0x40 : 0) -- PCR_flag and random_access_indicator --; the PCR (pcr >> 25) & 0xFF,
 *                  (pcr >> 17) & 0xFF, (pcr >> 9) & 0xFF, (pcr >> 1) & 0xFF, ((pcr & 1) << 7) | 0x7E, 00 (extension 0); a0 - 7
 *                  bytes FF; then PES bytes [0, min(L, 176)).
 *   packet k >= 1  PUSI = 0, c = min(184, L - 176 - 184 (k - 1)) PES bytes.  c = 184: afc = 1, no adaptation field.
 *                  c < 184: afc = 3, length byte 183 - c and, if that is >= 1, a flags byte 00 and 182 - c bytes FF.  The
 *                  payload ends the packet.
 * PSI.  With FERHIP_TS_PSI, and only in front of an I picture's packets, come a PAT and a PMT packet, so that the stream's
 * packets from there on are a single-program transport stream a player can open:
 *   PAT  47 40 00 10|psi_cc 00, the section 00 B0 0D 00 01 C1 00 00 00 01 E0|pmt_pid>>8 pmt_pid&FF + CRC, FF to 188;
 *   PMT  47 40|pmt_pid>>8 pmt_pid&FF 10|psi_cc 00, the section 02 B0 12 00 01 C1 00 00 E0|pid>>8 pid&FF F0 00 1B
 *        E0|pid>>8 pid&FF F0 00 + CRC, FF to 188.
 * The CRC is CRC-32/MPEG-2 (polynomial 0x04C11DB7, initial value 0xFFFFFFFF, no reflection, no final xor, big-endian) over
 * the section from its table_id: 2A B1 04 B2 for pmt_pid = 0x1000, 15 BD 4D 56 for pid = 0x100.  The sections are built on
 * the host and kept in a small device table; a stream's row is sent again only when its (pid, pmt_pid) differ from what the
 * table holds, and the kernel patches in psi_cc.  ferhip_write_ts_psi (host) writes the two packets, 376 bytes; 0 if cap is
 * short or a PID or psi_cc is refused.
 * The library keeps no TS state: the caller advances cc by the access unit's PES-carrying packets (npkts, less 2 where PSI
 * was written) and psi_cc by 1 per access unit that carried PSI; a repeated call with the same hdr gives the same bytes.
 * Layout: stream order; a stream's packets are contiguous, 188 bytes apart, PSI first; every stream begins at a multiple of
 * 16, and the bytes between a stream's end and the next multiple of 16 are not written.  index[s] = (offset, 188 * npkts,
 * NAL unit type of the slice, npkts, 0); a stream without a picture has zeros.  index[S] = (total rounded up to 16,
 * streams written, 0, total packets, 0).
 * Overflow is ferhip_pack_rtp's rule, per stream: the index always holds the true values, a stream is written whole or not
 * at all, only if offset + bytes <= cap, and nothing at or beyond cap is touched.  ferhip_pack_ts then still returns 0,
 * ferhip_fetch_ts fills h_index and returns FERHIP_E_ARG.
 * FERHIP_E_ARG (hdr is read for every stream, those without a picture included): a flag other than FERHIP_AU_PARAM_SETS |
 * FERHIP_TS_PSI, a null c, hdr or index, a null buffer with a cap, pts or pcr >= 2^33, pid or pmt_pid outside
 * 0x0010..0x1FFE, pid == pmt_pid, cc or psi_cc > 15, reserved != 0, and for ferhip_pack_ts a d_dst not aligned to 16 or a
 * d_index not aligned to 8.  FERHIP_E_STATE before the context's first picture.
 * ferhip_pack_ts: device to device, asynchronous on the context's stream; it waits for nothing except a first call's
 * allocations.  ferhip_fetch_ts: the same bytes in host memory; it waits once for the index and once for the copy.  Packing
 * changes nothing the encoder reads, may be repeated and may be mixed with the other framings.
 * ferhip_ts_blocks: known-answer surface with the conventions of ferhip_rtp_blocks: host payloads, one slice unit each (no
 * parameter sets, no PSI), hdr[n], n <= 65535, and bytes the kernels do not write keep the caller's values.  A payload of
 * length 0 gives L = 25.
 * Not provided: multi-program output (the PIDs are the caller's, so the caller may interleave several streams' packets);
 * null-packet padding to a constant rate and PCR pacing; a non-zero PES_packet_length; DTS. */
#define FERHIP_TS_PSI 8
typedef struct { uint64_t pts, pcr; uint16_t pid, pmt_pid; uint8_t cc, psi_cc; uint16_t reserved; } ferhip_ts_hdr; /* 24 bytes, host */
typedef struct { uint64_t offset; uint32_t bytes; int32_t nal_type; uint32_t npkts, reserved; } ferhip_ts_au;      /* 24 bytes */
int ferhip_pack_ts(ferhip_ctx *c, int flags, const ferhip_ts_hdr *hdr /* host [S] */, void *d_dst, size_t cap, ferhip_ts_au *d_index /* [S+1] */);
int ferhip_fetch_ts(ferhip_ctx *c, int flags, const ferhip_ts_hdr *hdr, void *h_dst, size_t cap, ferhip_ts_au *h_index);
int ferhip_ts_blocks(const uint8_t *payloads, size_t stride, const uint32_t *lens, const int32_t *nal_type, size_t n,
                     const ferhip_ts_hdr *hdr /* [n] */, uint8_t *out, size_t cap, ferhip_ts_au *index /* [n+1] */);
size_t ferhip_write_ts_psi(int pid, int pmt_pid, int psi_cc, uint8_t *out, size_t cap);

/* ---- Fragmented MP4 on the device: media segments of many pictures (ISO/IEC 14496-12, 14496-15; CMAF, DASH, MSE) ----
 * The fifth framing, and the first that holds more than one picture: a segment -- one moof and one mdat -- per stream is
 * accumulated in device memory over any number of encode calls, the write cursors live on the device, and the host reads
 * nothing until the segment is closed.  All integers are big-endian; a box is a u32 size, a 4-byte type and size - 8
 * content bytes.
 * Region.  ferhip_mp4_open starts a segment of at most K = max_samples pictures per stream (1 <= K <= 4096).  Stream s
 * owns d_dst + s * stride (d_dst 16-byte aligned, stride a multiple of 16 and < 2^31).  D = 104 + 12 K rounded up to 16 is
 * where the samples begin; stride >= D + 16.  hdr[s] (host, read before the call returns) = the segment's sequence number,
 * the decode time of its first sample and the duration of every sample, in the track's timescale.
 * Samples.  ferhip_mp4_append, behind a ferhip_encode_picture[_dev] call, adds that call's picture of every stream that
 * coded one as the stream's sample n = 0, 1, ...; a stream without a picture (FERHIP_NAL_NONE) adds nothing.  A sample is
 * the stream's entry exactly as ferhip_pack_nal writes it with FERHIP_AU_AVCC -- with FERHIP_AU_PARAM_SETS in the
 * segment's flags, with FERHIP_AU_AVCC | FERHIP_AU_PARAM_SETS -- and starts at D + the sizes of the samples in front:
 * samples are contiguous, at whatever byte phase that gives.  Append also writes trun entry n at region offset 88 + 12 n:
 * u32 hdr[s].duration, u32 sample size, u32 sample_flags = 0x02000000 for an IDR slice (sample_depends_on 2: an I
 * picture, a sync sample) and 0x01010000 otherwise (sample_depends_on 1, sample_is_non_sync_sample).  It waits for
 * nothing, copies nothing to the host and, after the segment's first append, allocates nothing.
 * Faults.  A sample that would end beyond stride sets the stream's fault to 1, a sample number K + 1 sets it to 2; from a
 * faulted sample on nothing more is added to that stream in this segment, and the samples in front stand.  No byte at or
 * beyond a region's end and no byte of another region is ever touched.
 * ferhip_mp4_close writes, for a stream with n >= 1 samples of M bytes in all, the front of its region:
 *      0  moof, size 88 + 12 n
 *      8  mfhd: 00000010 'mfhd' 00000000 (version, flags) u32 sequence
 *     24  traf, size 64 + 12 n
 *     32  tfhd: 00000010 'tfhd' 00020000 (default-base-is-moof) 00000001 (track_ID)
 *     48  tfdt: 00000014 'tfdt' 01000000 (version 1) u64 decode_time
 *     68  trun: size 20 + 12 n, 'trun', 00000701 (data-offset, sample duration, size and flags present), u32 n,
 *         i32 data_offset = D (from the moof's first byte), then the n entries already in place
 *     88 + 12 n  free, size D - 96 - 12 n, content zero
 *     D - 8      mdat, size 8 + M; the samples follow
 * and index[s] = (s * stride, D + M, n, NAL unit type of the first sample's slice, fault).  A stream with n = 0 has zeros
 * (offset and fault only, if it faulted on its first sample) and nothing of its region is written.  index[S] = (0, streams
 * with n >= 1, total samples, 0, OR of the faults).  Close ends the segment and is asynchronous like append (d_index
 * 8-byte aligned).  ferhip_mp4_fetch is close plus the segments back to back in host memory, in stream order without gaps:
 * h_index[s].offset is then the offset in h_dst; it waits once for the index and once for the copies, one per stream.  If
 * cap is short it fills h_index and returns FERHIP_E_ARG; the segment is closed all the same and stays in the regions.
 * The library keeps no MP4 state beyond the open segment: the caller advances decode_time by nsamples * duration and
 * sequence by 1.
 * FERHIP_E_STATE: open while a segment is open; append, close or fetch with none open; append twice behind one encode
 * call; append before the context's first picture.  FERHIP_E_ARG: null pointers, a misaligned d_dst, d_index or stride, K
 * or stride out of range, a flag other than FERHIP_AU_PARAM_SETS.  The other framings may be called freely while a segment
 * is open and change nothing of it; ferhip_reset_stream inside a segment is allowed (the stream's next sample is then an
 * IDR slice), and ferhip_destroy with a segment open is clean.
 * ferhip_write_mp4_init (host): the initialisation segment of stream s, 0 if cap is short, s is out of range or timescale
 * is 0; it follows ferhip_set_display_size and ferhip_set_rate as the SPS and PPS writers do.  Fields not named are 0:
 *   ftyp  major 'iso6', minor 0, compatible 'iso6' 'cmfc' 'avc1'
 *   moov
 *     mvhd  version 0; timescale; duration 0; rate 00010000; volume 0100; the unity matrix 00010000 0 0 0 00010000 0 0 0
 *           40000000; next_track_ID 2
 *     trak
 *       tkhd  version 0, flags 000003 (enabled, in movie); track_ID 1; duration 0; the unity matrix; width and height =
 *             the display size in 16.16
 *       mdia
 *         mdhd  version 0; timescale; duration 0; language 55C4 ('und')
 *         hdlr  handler 'vide'; name = one 00 byte
 *         minf
 *           vmhd  flags 000001
 *           dinf  dref: entry_count 1, one 'url ' box with flags 000001 (the media is in this file) and no content
 *           stbl
 *             stsd  entry_count 1, one 'avc1' entry: data_reference_index 1; u16 width, u16 height = the display size;
 *                   horizontal and vertical resolution 00480000 (72 dpi); frame_count 1; a compressor name of 32 zero
 *                   bytes; depth 0018; pre_defined FFFF (-1); then the avcC box, whose content is the record of
 *                   ferhip_write_avcc_config(c, s, ...)
 *             stts, stsc, stco  entry_count 0;  stsz  sample_size 0, sample_count 0
 *     mvex  trex: track_ID 1, default_sample_description_index 1, default duration, size and flags 0
 * ferhip_mp4_blocks: known-answer surface with the conventions of ferhip_ts_blocks: n host payloads, one slice unit each
 * with its nal_type (no parameter sets), in segments of m consecutive payloads (the last may be shorter: nseg = ceil(n /
 * m)), hdr[nseg], K = max_samples and stride as above; out (host, nseg * stride bytes: bytes the kernels do not write keep
 * the caller's values) receives the regions and index[nseg + 1] the index.  n <= 65535, m >= 1.
 * The way in is ferhip_decs_decode_mp4, with the decoders below. */
typedef struct { uint64_t decode_time; uint32_t sequence, duration; } ferhip_mp4_hdr; /* 16 bytes, host */
typedef struct { uint64_t offset; uint32_t bytes, nsamples; int32_t first_nal_type; uint32_t fault; } ferhip_mp4_seg; /* 24 bytes */
int ferhip_mp4_open(ferhip_ctx *c, int flags, int max_samples, const ferhip_mp4_hdr *hdr /* host [S] */, void *d_dst, size_t stride);
int ferhip_mp4_append(ferhip_ctx *c);
int ferhip_mp4_close(ferhip_ctx *c, ferhip_mp4_seg *d_index /* [S+1] */);
int ferhip_mp4_fetch(ferhip_ctx *c, void *h_dst, size_t cap, ferhip_mp4_seg *h_index /* [S+1] */);
size_t ferhip_write_mp4_init(ferhip_ctx *c, int s, uint32_t timescale, uint8_t *out, size_t cap);
int ferhip_mp4_blocks(const uint8_t *payloads, size_t pstride, const uint32_t *lens, const int32_t *nal_type, size_t n, size_t m,
                      int max_samples, const ferhip_mp4_hdr *hdr /* [nseg] */, uint8_t *out, size_t stride, ferhip_mp4_seg *index /* [nseg+1] */);

/* encode() + NastaviEncode() for S streams of T pictures each (F/fer_h264.cpp:55-134), each stream with its own PPS:
 * frames host [T][S][W*H*3/2]; out host [S][out_stride] Annex-B; out_len[S].
 * recon (optional) host [T][S][W*H*3/2]. */
int ferhip_encode_streams(ferhip_ctx *c, const uint8_t *frames, int nframes, uint8_t *out, size_t out_stride,
                          size_t *out_len, uint8_t *recon);

/* ---- rate control: per-stream QP of every picture ----
 * Each stream of a context codes every picture at one QP (mb_qp_delta stays 0) and chooses it per picture.  The choice is
 * made on the device, by a kernel that runs before the picture's first quantising launch, from the RBSP length of the
 * stream's previous picture already in device memory: rate control adds no host synchronisation to the picture pipeline.
 *
 * base[s] = the QP in stream s's PPS (pic_init_qp = 14 + base[s], ferhip_write_pps_stream).  It starts as params.qp; a
 * ferhip_set_rate call made before the stream's first picture sets it to r->qp (which must then be <= 37, so that
 * pic_init_qp_minus26 = base - 12 stays within -26..25); after the first picture it is frozen.  Every slice header carries
 * slice_qp_delta = qp - base[s] - 14, so a stream kept at one QP q is byte-identical to the reference run with _qParameter = q.
 *
 * FERHIP_RC_CQP: every picture at r->qp (0..51), from the next picture on; may change between any two pictures.
 * FERHIP_RC_ABR: steers to target_bits RBSP bits per picture on average, in integer arithmetic:
 *   P6 = {65536, 73562, 82570, 92682, 104032, 116772} (2^16 * 2^(k/6));  pow2q16(d) = P6[d mod 6] shifted by floor(d / 6)
 *   est(y, q) = (last_bits[y] * pow2q16(last_qp[y] - q)) >> 16, y = 0 for P, 1 for I pictures
 *   before choosing, the stream's previous picture (type y', QP q', b = 8 * its RBSP bytes), if it was coded in ABR, is accounted:
 *     err += b - target; last_bits[y'] = b; last_qp[y'] = q'; have[y'] = 1
 *   window = r->window > 0 ? r->window : intra_every
 *   T = clamp(target - err / window (truncating), max(target / 8, 1), 8 * target)
 *   P picture: have[P] ? the smallest q in [qp_min, qp_max] with est(P, q) <= T (qp_max if none), clamped to last_qp[P] +- max_step
 *              : have[I] ? last_qp[I] + ip_offset : r->qp
 *   I picture: have[P] ? last_qp[P] - ip_offset : have[I] ? last_qp[I] : r->qp
 *   then clamped to [qp_min, qp_max].  An I picture's extra bits land in err and the P pictures of the next window pictures pay
 *   them back.  Entering ABR (from CQP or at create) clears err and have[]; a call in ABR keeps them.
 * FERHIP_RC_QUALITY: holds the luma SSE of every picture (ferhip_quality.sse[0]) at target_sse, in integer arithmetic:
 *   est(y, q) = (last_sse[y] * pow2q16(2 * (q - last_qp[y]))) >> 16   (exact: 128-bit intermediate; SSE ~ Qstep^2)
 *   before choosing, the stream's previous picture (type y', QP q', luma SSE e), if it was coded in QUALITY, is accounted:
 *     last_sse[y'] = e; last_qp[y'] = q'; have[y'] = 1
 *   picture of type y: have[y]   ? the largest q in [qp_min, qp_max] with est(y, q) <= target_sse (qp_min if none),
 *                                  clamped to last_qp[y] +- max_step
 *                    : have[1-y] ? last_qp[1-y] + (y == P ? ip_offset : -ip_offset)
 *                    : r->qp
 *   then clamped to [qp_min, qp_max].  Entering QUALITY (from CQP, ABR or at create) clears have[]; a call in QUALITY keeps it.
 *   The SSE is the one k_quality measured on the device after the previous picture: a stream in QUALITY turns the measurement
 *   of its context on (at least FERHIP_QM_SSE) whatever ferhip_set_quality says, and window is ignored.
 * Invalid arguments return FERHIP_E_ARG: s outside -1..S-1, qp outside 0..51, a base of 38 or more before the first picture,
 * and in ABR or QUALITY qp_min < 0, qp_max > 51, qp_min > qp_max, max_step < 1, |ip_offset| > 51, in ABR also window < 0
 * and target_bits <= 0, in QUALITY target_sse <= 0.
 * ferhip_set_rate only records the settings; ferhip_get_qp is the only rate-control call that waits (for the last picture). */
#define FERHIP_RC_CQP 0
#define FERHIP_RC_ABR 1
#define FERHIP_RC_QUALITY 2
typedef struct {
    int mode;              /* FERHIP_RC_CQP / FERHIP_RC_ABR / FERHIP_RC_QUALITY */
    int qp;                /* CQP: QP of every picture from the next one on; ABR, QUALITY: QP of the first picture */
    int qp_min, qp_max;    /* ABR, QUALITY: 0 <= qp_min <= qp_max <= 51 */
    int max_step;          /* >= 1; ABR: largest change between P pictures, QUALITY: between pictures of one type */
    int ip_offset;         /* ABR, QUALITY: an I picture takes the last P QP minus this */
    int window;            /* ABR: pictures over which the accumulated error is paid back; 0 = intra_every */
    long long target_bits; /* ABR: RBSP bits per picture, > 0 */
    long long target_sse;  /* QUALITY: luma SSE per picture, > 0 */
} ferhip_rate;
int ferhip_set_rate(ferhip_ctx *c, int s, const ferhip_rate *r); /* s = -1: every stream; applies from the next picture */
int ferhip_get_qp(ferhip_ctx *c, int *qp_per_stream);            /* QP of each stream's last picture (waits for it) */
size_t ferhip_write_pps_stream(ferhip_ctx *c, int s, uint8_t *rbsp, size_t cap); /* pic_init_qp = 14 + base[s] */

/* ---- quality measurement: SSE and SSIM of every picture, on the device ----
 * With measurement on, every picture run_picture codes is compared with its source after entropy coding, by one kernel
 * (k_quality) per picture, and one record per stream lands in a device ring of FERHIP_QUALITY_RING pictures.  Nothing
 * waits for it: ferhip_get_quality reads the ring, so a caller that reads once every few dozen pictures adds one sync.
 * Measuring changes no byte of the output.  It costs a copy of the source pictures (a buffer as large as one picture set,
 * allocated on the first enable) and the kernel; off (the default) runs nothing and allocates nothing.
 *   sse[p]      = sum over plane p (W x H luma, W/2 x H/2 chroma) of (source - reconstruction)^2, exact integers
 *   SSIM window = the 8x8 luma block at every (x, y) with x, y multiples of 4, x <= W - 8, y <= H - 8:
 *                 ssim_windows = (W/4 - 1) * (H/4 - 1)
 *   in a window, a = source, b = reconstruction: s1 = sum a, s2 = sum b, ss = sum a^2 + sum b^2, s12 = sum ab,
 *                 vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2
 *                 num = (2 s1 s2 + 416) (2 covar + 235963), den = (s1^2 + s2^2 + 416) (vars + 235963)  (int64, den > 0)
 *                 value = (double)num / (double)den
 *   ssim_sum    = the sum of the window values, added in an order fixed by W, H and S: identical from run to run.
 *   mean SSIM = ssim_sum / ssim_windows; PSNR = 10 log10(255^2 N / sse), +inf for sse = 0. */
#define FERHIP_QM_SSE 1  /* per-plane sum of squared differences source - reconstruction */
#define FERHIP_QM_SSIM 2 /* luma SSIM (implies the luma sums) */
#define FERHIP_QUALITY_RING 64
typedef struct ferhip_quality {
    uint64_t sse[3];       /* Y, Cb, Cr over the coded picture (measured whenever the picture is) */
    double ssim_sum;       /* sum of the per-window SSIM values above; 0 without FERHIP_QM_SSIM */
    uint32_t ssim_windows; /* 0 without FERHIP_QM_SSIM */
    int32_t qp, nal_type;  /* the picture's QP and FERHIP_NAL_IDR / FERHIP_NAL_SLICE; nal_type 0 = the stream had no picture
                              in this call (FERHIP_NAL_NONE): sse, ssim_*, rbsp_bytes are 0, qp is its last picture's */
    uint32_t rbsp_bytes;
    uint32_t picture;      /* index of the picture in its own stream (0 = first picture encoded); for a stream without a
                              picture in this call: the number of pictures it has coded so far */
} ferhip_quality;
/* flags: 0 (default) = off, else FERHIP_QM_SSE | FERHIP_QM_SSIM; applies from the next picture.  FERHIP_E_ARG for other
 * bits, FERHIP_E_HIP when the buffers cannot be allocated. */
int ferhip_set_quality(ferhip_ctx *c, int flags);
/* The last min(npic, pictures measured so far, FERHIP_QUALITY_RING) pictures, oldest first, as out[k][S]; returns how many,
 * or an error.  Waits for the last picture.  FERHIP_E_STATE if the context has never measured. */
int ferhip_get_quality(ferhip_ctx *c, int npic, ferhip_quality *out);

/* statistics of Starter::DohvatiStatistiku: brojTipova[5] per stream, accumulated */
int ferhip_get_stats(ferhip_ctx *c, int *counts5_per_stream);
/* sticky device error flags per stream (bits 0, 1: unused, bit 2: RBSP buffer overflow, bits 3, 4: decoder syntax
 * error / unsupported syntax, bit 5: motion chain timeout, bit 6: a P macroblock without this picture's vectors, bit 7: a slice header with its
 * slice_qp_delta longer than 64 bits -- more than about 4000 IDR pictures in a row) */
int ferhip_status(ferhip_ctx *c, int *flags_per_stream);
const char *ferhip_version(void);

/* Live kernel timing: when enabled every kernel group of a picture is bracketed by HIP events
 * on the launch stream.  ferhip_get_profile synchronises and returns accumulated milliseconds
 * and launch counts per phase. */
#define FERHIP_PH_INTERP 0     /* k_interp: the 16 quarter-pel planes */
#define FERHIP_PH_ME_PRE 1     /* k_me_pre: box sums, stage-3 search, its SADs */
#define FERHIP_PH_ME_RESOLVE 2 /* k_me_resolve, one persistent launch per picture */
#define FERHIP_PH_P_RESID 3    /* k_p_resid (partition merge, mvd, snapping, residual) */
#define FERHIP_PH_INTRA 4      /* k_intra_mb, one launch per MB anti-diagonal */
#define FERHIP_PH_CAVLC 5      /* size + scan + emit */
#define FERHIP_PH_FRAME_SAD 6
#define FERHIP_PH_ME_SPEC 7    /* k_me_spec: the predictor-dependent searches for a guessed predictor */
#define FERHIP_PH_SORT 8       /* the two radix passes: k_rs_hist, k_rs_scan, k_rs_scatter, each twice */
#define FERHIP_PH_ME_WALK 9    /* k_me_walk: stage-2 candidate sets */
#define FERHIP_PH_SORT_KEYS 10   /* k_feat0: plane-0 features + the sort's input records */
#define FERHIP_PH_SORT_FINISH 11 /* k_sort_index (+ k_bucket_classes, k_sort_quirk): bucket index of the sorted order */
#define FERHIP_NPHASE 12
int ferhip_profile(ferhip_ctx *c, int enable);
/* launch-shape knobs; results never depend on them.  RESOLVE_WGS = workgroups of the persistent motion-chain launch
 * (default 6144 single-wavefront workgroups; any value >= 1 resolves every row: a workgroup whose own queue is empty takes rows of the others) */
#define FERHIP_TUNE_RESOLVE_WGS 1
#define FERHIP_TUNE_RESOLVE_GROUP 2 /* streams whose rows the motion chain keeps in flight together (cache footprint); clamped to the context's streams */
#define FERHIP_TUNE_OVERLAP_SORT 4  /* 0 (default): the radix sort + bucket index of the reference picture run before k_me_pre; 1 / 2: on a
                                       second stream beside it (measured on MI355X / ROCm 7.2: the two launches do not share the
                                       GPU, the sort simply ends later -- kept as an experiment switch) */
#define FERHIP_TUNE_SPECULATE 3     /* 1 (default): k_me_spec runs the predictor-dependent searches for a guessed predictor and the
                                       chain verifies; 0: the chain searches everything itself */
int ferhip_tune(ferhip_ctx *c, int key, int value);
int ferhip_get_profile(ferhip_ctx *c, double *ms, long *launches, int reset);

/* ---- per-stage entry points (unit-parity surface, SURVEY.md 8b "per-MB") ----
 * They operate on the pictures currently in the context, for all streams. */
/* FillInterpolatedRefFrame(), F/moestimation.h / F/moestimation.cpp:74 */
int ferhip_fill_interpolated(ferhip_ctx *c);
/* motion decision of every MB = interEncoding() over the picture, F/moestimation.cpp:392; the partition merge
 * shares its wavefront with the residual of the macroblock, so the picture buffers hold the reconstruction of
 * the inter macroblocks afterwards */
int ferhip_inter_encoding(ferhip_ctx *c);
/* debug/test read-back of device state; which: see FERHIP_BUF_*; returns bytes copied */
#define FERHIP_BUF_INTERP 1   /* uint8  [S][16][H][W] */
#define FERHIP_BUF_FEAT 2     /* uint16 [S][H][W][16][6] (k0..k4, pad) */
#define FERHIP_BUF_SORTPOS 3  /* uint32 [S][W*H] */
#define FERHIP_BUF_KOLIKO 4   /* int32  [S][16385] */
#define FERHIP_BUF_MBTYPE 5   /* int32  [S][nmb] */
#define FERHIP_BUF_MV 6       /* int16  [S][nmb][4][2] */
#define FERHIP_BUF_MVD 7      /* int16  [S][nmb][4][2] */
#define FERHIP_BUF_LEVELS 8   /* int16  [S][nmb][400] */
#define FERHIP_BUF_CBP 9      /* uint8  [S][nmb][2] */
#define FERHIP_BUF_TC 10      /* uint8  [S][nmb][24] */
#define FERHIP_BUF_I4MODE 11  /* uint8  [S][nmb][16] */
#define FERHIP_BUF_CUR 12     /* uint8  [S][W*H*3/2] current picture buffers */
#define FERHIP_BUF_REF 13     /* uint8  [S][W*H*3/2] reference picture buffers */
#define FERHIP_BUF_TIMING 14  /* int64  [64] in-kernel wall-clock sums (10 ns units) when FER_DBG bit 7 is set */
#define FERHIP_BUF_ST2N 15    /* int32  [S][nmb][4] stage-2 candidates of every 8x8 partition (before the list cap) */
#define FERHIP_BUF_SPEC_STAT 17 /* uint64 [8] since the context was created: partitions the motion chain decided, of which the guessed
                                 predictor was right, P_Skip verdicts needed, of which taken from the guess (kept per workgroup of the
                                 chain on the device, summed here), then four zero words */
#define FERHIP_BUF_MBSIZE 18   /* int32  [S][nmb][2] coded_mb_size (F/rbsp_encoding.cpp:330) of the Intra16x16 and of the Intra4x4 alternative of every
                                 macroblock of the last I picture */
#define FERHIP_BUF_ST2 16     /* int32  [S][nmb][4][384][2] the candidates (position relative to the block, feature distance); a crowded
                                 partition (count > 384) holds its summary instead (k_me_walk, read by resolve_crowded):
                                   [0 .. 32]   the first candidates of distance 0 in arrival order, (position, 0)
                                   [40]        (J = the step the walk stopped in, the smallest positive distance: a lower bound)
                                   [41]        (zeros = how many of [0 .. 32] are set, np2 | nbig << 16 | fallback << 30):
                                               np2 = listed candidates in [64 .. 64 + np2), at most 320; nbig = big bucket
                                               slices (more than 1024 records) described in [42 .. 44], at most 3; fallback =
                                               more than 3 big slices, or one with more than 512 records outside its class, or
                                               more than 320 candidates to list: no class is used then, and with nbig = 0 the
                                               chain walks the buckets again
                                   [42 .. 44]  (bucket, feature distance of its class; 0x7fffffff = no member can be a candidate)
                                   [46]        (the smallest of the class distances, 0)
                                   [64 ..]     listed candidates: (position, D | step << 20 | side << 28) */
/* The lists the four motion kernels hand each other, as they stand after ferhip_inter_encoding (list-level parity
 * tests; the layouts below are ABI for tests).  A "packed vector" is one int32: (x & 0xffff) | (y << 16), x and y
 * signed 16-bit, in quarter samples for vectors and in whole samples for the centre of SPEC_HDR.  SPEC_HDR, SPEC_L1 and
 * SPEC_L2 are written by k_me_spec only: with FERHIP_TUNE_SPECULATE = 0, for a stream whose picture is an I picture, and
 * (the two lists) for a partition whose header has bit 16 clear they hold stale or uninitialised data; SUMA, ST3, ST3N
 * and V0 likewise belong to the last P picture of the stream. */
#define FERHIP_BUF_SUMA 19    /* int32  [S][nmb][4][5] the five box sums of every 8x8 source block (F/moestimation.cpp:440-451), k_me_pre */
#define FERHIP_BUF_ST3 20     /* int32  [S][nmb][4][33][3] stage-3 survivors in list order: (x, y, SAD), x and y in quarter samples;
                                 entries [0, ST3N) are set, k_me_pre */
#define FERHIP_BUF_ST3N 21    /* int32  [S][nmb][4] number of stage-3 survivors, k_me_pre */
#define FERHIP_BUF_V0 22      /* int32  [S][nmb][4] packed vector: the first stage-3 survivor of smallest SAD (0 with no survivor), k_me_pre */
#define FERHIP_BUF_SPEC_HDR 23 /* int32 [S][nmb][4][4], k_me_spec: [0] = packed guessed integer centre (genx, geny) = guessed predictor >> 2;
                                 [1] = cnt1 | cnt2 << 8 | lists written << 16 | P_Skip verdict present << 17 (cnt1 / cnt2 = entries of
                                 SPEC_L1 / SPEC_L2; bit 17 is set on partition 0 only); [2] = packed guessed P_Skip vector (partition 0);
                                 [3] = 1 when the guessed P_Skip test passed: no lists for any partition of the macroblock */
#define FERHIP_BUF_SPEC_L1 24 /* int32  [S][nmb][4][17][2] stage-1 list for the guessed centre, list order: (packed vector, SAD); entries [0, cnt1) */
#define FERHIP_BUF_SPEC_L2 25 /* int32  [S][nmb][4][33][2] re-ranked stage-2 list for the guessed centre: (packed vector, SAD); entries [0, cnt2) */
size_t ferhip_read_buffer(ferhip_ctx *c, int which, void *dst, size_t cap);
/* set the reference picture (dpb) directly, [S][W*H*3/2] host */
int ferhip_set_reference(ferhip_ctx *c, const void *src);

/* ---- decode twin (row a19): decode() / RBSP_decode(), F/fer_h264.cpp:26-53, F/rbsp_decoding.cpp:17 ----
 * S Annex-B streams (4-byte start codes, as the reference reads them) of equal picture size are
 * decoded side by side: slice_data parsing runs one wavefront per picture over a window of pictures of
 * every stream at once, reconstruction one wavefront per macroblock, picture by picture.  out (host, may be NULL): [max_pictures][S][W*H*3/2], picture t of
 * stream s at (t*S + s)*W*H*3/2; pictures[s] = number decoded; the slots behind a stream's last picture are left as they
 * were.  Sub-8x8 partitions, ref_idx_l0 and
 * reference list modification are handled the way the reference handles them; syntax the
 * GPU path does not implement (I_PCM, CABAC, High profiles, field coding, slice groups) returns FERHIP_E_UNSUP.
 *
 * Illegal and damaged streams (all three decode paths).  The rule is no silent divergence from the reference decoder: a
 * stream it decodes gives its pictures, bit for bit, or a fault for that stream at that picture.  Meaning that no
 * conformant encoder produces is decoded like the reference decodes it: an intra prediction mode that reads a neighbour
 * which does not exist predicts from the reference's -1 "unavailable" samples, a motion vector may point anywhere (every
 * sample coordinate is clamped to the picture).  Where the reference stops with one of its fatal errors (mb_type,
 * intra_chroma_pred_mode, coded_block_pattern or mb_qp_delta out of range, TotalCoeff above 16), the picture is a fault:
 * FERHIP_E_DEVICE.  One limit: with data left behind a skip run that ends a picture the reference parses one more
 * macroblock, past the picture.  That macroblock is followed only through mb_type (above 31 is its fatal error) and, for
 * an intra type, the prediction modes and intra_chroma_pred_mode (above 3); short of these the picture is complete and
 * is delivered.  An inter type's fields, the coded_block_pattern, mb_qp_delta and residual of that macroblock, and
 * whatever the reference parses after it, are not followed: a fatal error the reference meets there goes unreported.
 * What the decoders refuse although the reference decodes on -- the complete list:
 *   - I_PCM (mb_type 25 in an I slice, 30 in a P slice): FERHIP_E_UNSUP;
 *   - any other mb_type above 25 in an I slice written with slice_type 7 (the reference tests slice_type == 2 only),
 *     bits that no entry of a CAVLC table matches (the reference settles on the nearest lower code): FERHIP_E_DEVICE;
 *   - a motion vector component outside [-32768, 32767] quarter samples (vectors are kept in 16 bits; a level allows
 *     +-8192): FERHIP_E_DEVICE;
 *   - a residual block whose coefficients do not fit it -- TotalCoeff or total_zeros too large for a 15-coefficient
 *     block, a run_before above the zeros that are left -- which the reference stores into the neighbouring block of
 *     its level array or outside it: FERHIP_E_DEVICE.
 * Where the reference itself divides by zero or indexes outside its arrays (a sub_mb_type above 3, a level_prefix above
 * 15, a level stored outside its level array, a macroblock type without partitions in motion prediction) there is
 * nothing to follow; such a stream decodes or faults (a sub_mb_type above 3 and a level_prefix of more than 31 zeros
 * always fault, FERHIP_E_DEVICE), and never disturbs another stream or a later call. */
int ferhip_decode_streams(const uint8_t *const *streams, const size_t *lens, int nstreams, uint8_t *out,
                          int max_pictures, int *pictures, int *width, int *height);
/* frees the window buffers ferhip_decode_streams keeps between calls (tens of GB of HBM for large batches) and the
 * calling thread's host copy of the streams' RBSP (as large as the streams of its last call); FERHIP_E_STATE while a
 * decode is running */
int ferhip_decode_release(void);

/* ---- streaming decoder: RBSP_decode(NALunit) of F/rbsp_decoding.cpp:17 for one stream, NAL unit by NAL unit ----
 * rbsp = the NAL unit's payload without header byte and emulation prevention bytes (what getNAL delivers,
 * F/nal.cpp:68-223).  nal_unit_type 7 (SPS) sizes the decoder, 8 (PPS) is kept, 5 / 1 decode one picture: when
 * `picture` is not NULL it receives W*H*3/2 bytes of I420 and *got_picture = 1.  Other NAL unit types are ignored. */
typedef struct ferhip_dec ferhip_dec;
int ferhip_dec_create(ferhip_dec **out);
int ferhip_dec_nal(ferhip_dec *d, int nal_unit_type, int nal_ref_idc, const uint8_t *rbsp, size_t n, uint8_t *picture,
                   int *got_picture, int *width, int *height);
void ferhip_dec_destroy(ferhip_dec *d);

/* ---- live decoder: S streams of one coded picture size whose NAL units arrive piece by piece ----
 * Each call takes what every stream has now, parses the slices of all streams with one launch and reconstructs them
 * together; a stream's pictures over all calls, in order, are byte-identical to what ferhip_decode_streams gives for
 * the concatenation of its chunks, however its NAL units are spread over calls and whichever other streams are present.
 * width, height: multiples of 16.  max_pictures: slice NAL units per stream and call.  One thread at a time per decoder;
 * it lives on the HIP device that is current at create.
 *
 * chunks[s], lens[s]: whole NAL units of stream s, Annex-B with 4-byte start codes (or length-prefixed, once
 * ferhip_decs_set_input asked for it: "length-prefixed input" below), or NULL / 0 = nothing new for stream s in this call.  out: [max_pictures][nstreams][W*H*3/2] I420, picture k of stream s of this call at
 * (k*nstreams + s)*W*H*3/2; out_on_device = 1: out is device memory on the decoder's device; out = NULL: no copy.
 * Slots of stream s from pictures[s] on are not written.  pictures[s] = pictures of stream s decoded in this call.
 * status[s] = 0 or the fault of stream s in this call: FERHIP_E_DEVICE (syntax error in slice data), FERHIP_E_UNSUP
 * (syntax the GPU path does not implement, an SPS of another picture size), FERHIP_E_ARG (a slice header that runs
 * past its NAL unit, more than max_pictures slices), FERHIP_E_STATE (a slice before the stream's SPS and PPS, a P
 * slice after a fault before the next IDR slice).  A fault affects only its stream: the faulted picture and the rest
 * of the stream's chunk are dropped, pictures[s] counts the pictures before it, and the stream restarts as a new
 * decoder that has received its last SPS and PPS, from the next IDR slice on.  The other streams decode as if that
 * stream had been absent.
 * Returns 0 when the call ran, even if some streams failed; FERHIP_E_ARG / _HIP for the call as a whole.
 *
 * ferhip_decs_reset_stream: stream s forgets everything, its parameter sets included (a new feed on that slot).
 *
 * Cropping.  The live decoder reads an SPS on past frame_mbs_only_flag, where the reference stops: direct_8x8_inference_flag,
 * frame_cropping_flag and the four offsets.  ferhip_decs_get_crop returns left, right, top, bottom of stream s's current SPS
 * in luma samples (offset * 2); FERHIP_E_STATE before the stream has an SPS, FERHIP_E_ARG for s outside 0..S-1.  An SPS
 * without cropping, one that ends before its offsets do and one whose offsets leave no picture (left + right >= W or
 * top + bottom >= H) report zeros; cropping never changes a status or a decoded sample.
 * ferhip_decs_set_display(x0, y0, dw, dh): all four even, x0 + dw <= W, y0 + dh <= H, dw, dh >= 2, else FERHIP_E_ARG.  From
 * the next ferhip_decs_decode / ferhip_decs_decode_dev call on, out is [max_pictures][nstreams][dw*dh*3/2] and slot (k, s)
 * holds that window of picture k of stream s (host or device out, of any alignment; slots from pictures[s] on are still not
 * written).  (0, 0, W, H) is the default and restores the full pictures.  The decoder does not apply a stream's cropping by
 * itself: a caller reads it with ferhip_decs_get_crop and asks for the window it wants.
 * ferhip_decs_set_layout(format, pitch_y, pitch_c): from the next decode call on every output slot holds its picture -- the
 * current window of ferhip_decs_set_display, or the full coded picture -- in a pitched layout, as a consumer's frame pool
 * wants it: Y rows at pitch_y, then for FERHIP_FMT_I420 the Cb rows and the Cr rows at pitch_c, for FERHIP_FMT_NV12 the
 * dh/2 rows of CbCr pairs at pitch_c.  The Y plane takes pitch_y * dh bytes and each chroma plane pitch_c * dh/2, so a
 * slot is pitch_y*dh + 2*pitch_c*(dh/2) bytes (I420) or pitch_y*dh + pitch_c*(dh/2) bytes (NV12), and out is
 * [max_pictures][nstreams][slot] at any alignment.  Only bytes that belong to a row are written: the pitch gaps keep what
 * they held.  FERHIP_E_ARG for an unknown format.  The pitches must hold a row of the window that is current when a decode
 * call is made (pitch_y >= dw; pitch_c >= dw/2 for I420, >= dw for NV12), and a layout other than the default needs
 * out_on_device = 1: else that decode call returns FERHIP_E_ARG before it takes anything.  The default is I420 with pitches
 * equal to the row bytes; (FERHIP_FMT_I420, dw, dw/2) is the default again, and a decoder on which the call is never made
 * behaves as before, byte for byte.  The packed formats (FERHIP_FMT_YUY2, UYVY, BGRA, RGBA: one plane of pitch_y * dh bytes,
 * converted on the way out) and ferhip_decs_set_csc are described with ferhip_set_csc above.
 * ferhip_decode_streams and the single-stream ferhip_dec_* always deliver the full coded pictures. */
typedef struct ferhip_decs ferhip_decs;
int ferhip_decs_create(ferhip_decs **out, int nstreams, int width, int height, int max_pictures);
int ferhip_decs_decode(ferhip_decs *d, const uint8_t *const *chunks, const size_t *lens, uint8_t *out, int out_on_device,
                       int *pictures, int *status);
int ferhip_decs_reset_stream(ferhip_decs *d, int s);
int ferhip_decs_get_crop(ferhip_decs *d, int s, int crop[4] /* left, right, top, bottom */);
int ferhip_decs_set_display(ferhip_decs *d, int x0, int y0, int dw, int dh);
int ferhip_decs_set_layout(ferhip_decs *d, int format, uint32_t pitch_y, uint32_t pitch_c);
int ferhip_decs_set_csc(ferhip_decs *d, int matrix); /* FERHIP_CSC_*: the matrix of a BGRA / RGBA output layout (see ferhip_set_csc) */
void ferhip_decs_destroy(ferhip_decs *d);

/* ---- Annex-B input in device memory: the splitter on the device ----
 * What the decoder's host splitter computes, by kernels.  For a range s[0..n): a unit begins at st = z + 4 for every z with
 * s[z..z+3] = 00 00 00 01 (z + 3 < n); it ends at en = the smallest i >= st with s[i] = s[i+1] = 0, s[i+2] in {0, 1} and
 * i + 2 < n, or at n (a three-byte start code ends a unit and begins none); en <= st is no unit.  The header byte is s[st]
 * (nal_ref_idc = (s[st] & 0x7f) >> 5, nal_unit_type = s[st] & 0x1f), the RBSP is s[st+1..en) without every byte s[p] = 03
 * with p - 2 >= st + 1 and s[p-2] = s[p-1] = 0.  A unit whose RBSP is empty ends its range: it and what follows are dropped.
 * The RBSP of the units goes to one buffer, every unit at the next multiple of 16 (the units behind an empty one included:
 * they are cut from the table, not from the buffer); bytes between units are not written.
 *
 * ferhip_split_nal_blocks: known-answer surface, context-free like ferhip_frame_nal_blocks.  n host byte ranges
 * ([n][stride], lens[n] <= 2^30, n <= 65535) are copied to the device, each to `misalign` (0..15) bytes past a 16-byte
 * boundary and ending at the end of its allocation, split and read back.  out (host, cap bytes: bytes the kernels do not
 * write keep the caller's values); units[k] = (range, nal_unit_type, nal_ref_idc, RBSP bytes, offset in out) in range order,
 * then stream order, after the cut; *nunits receives the true count even when it exceeds units_cap.  FERHIP_E_ARG when
 * units_cap or cap is too small (no byte at or behind cap is written), or for arguments out of range.
 *
 * ferhip_decs_decode_dev: ferhip_decs_decode for chunks that lie in device memory on the decoder's device.  d_chunks[s] is a
 * device pointer of any alignment (the array itself and lens are host memory; NULL / 0 = nothing new for stream s), for
 * example d_dst + index[s].offset with index[s].bytes of ferhip_pack_nal once the producing context was synchronised
 * (ferhip_sync); lens[s] <= 2^30.  The chunks are split on the device into a store the decoder owns, the table and the
 * first FERHIP_SPLIT_PREFIX bytes of every unit's RBSP come back in one copy, parameter sets and slice headers are parsed
 * from those on the host (a unit whose header is longer is fetched whole, that unit alone), and the slice data is parsed
 * where the splitter left it: no chunk byte crosses the bus and nothing is staged.  One host synchronisation for the
 * split, unless its table or store has to grow.  Results, pictures[], status[] and the isolation rules are those of
 * ferhip_decs_decode given the same bytes; the two calls may be mixed on one decoder.
 * ferhip_decs_timing: seconds this decoder has spent so far in t[0] the host splitter, t[1] gathering and copying slices to
 * the device, t[2] the slice data parse, t[3] reconstruction and output, t[4] the launches of the device splitter (HIP
 * events); t[5] = the bytes those launches split.  reset != 0 clears the sums. */
#define FERHIP_SPLIT_PREFIX 64
typedef struct { uint32_t range; int32_t nal_type, ref_idc; uint32_t bytes; uint64_t offset; } ferhip_nal_unit; /* 24 bytes */
int ferhip_split_nal_blocks(const uint8_t *ranges, size_t stride, const uint32_t *lens, size_t n, int misalign, uint8_t *out,
                            size_t cap, ferhip_nal_unit *units, size_t units_cap, size_t *nunits);
int ferhip_decs_decode_dev(ferhip_decs *d, const uint8_t *const *d_chunks, const size_t *lens, uint8_t *out, int out_on_device,
                           int *pictures, int *status);
int ferhip_decs_timing(ferhip_decs *d, double *t /* [6] */, int reset);

/* ---- length-prefixed (AVCC) input: demuxed samples, in host or in device memory ----
 * The NAL framing of ISO/IEC 14496-15: every NAL unit is preceded by its length.  The definition, which is the contract of
 * the host walk and of the kernels alike.  For a range s[0..n) and a length size L in {1, 2, 4}, start with pos = 0 and
 * repeat while pos + L <= n:
 *   1. Read len as the big-endian integer at s[pos..pos+L).
 *   2. Set st = pos + L and en = st + len.
 *   3. If len == 0, the unit is empty.
 *   4. If en > n, the unit overruns.
 *   5. Otherwise the unit is [st, en).  Its header byte is s[st], with nal_ref_idc = (s[st] & 0x7f) >> 5 and
 *      nal_unit_type = s[st] & 0x1f.
 *   6. The RBSP is s[st+1..en) without every byte s[p] = 03 that has p - 2 >= st + 1 and s[p-2] = s[p-1] = 0.  This is the
 *      rule the Annex-B splitter states above.
 *   7. Set pos = en.
 * An empty unit, a unit with an empty RBSP (len == 1) or an overrunning unit ends its range: that unit and everything
 * behind it are dropped, as an empty unit is dropped in Annex-B.  An overrun additionally faults the range; fewer than L
 * bytes left over at the end of the range also count as an overrun, of a unit that cannot even state its length.
 * Start-code patterns inside a unit mean nothing: boundaries come from the lengths alone.
 * The output is the Annex-B splitter's: the same ferhip_nal_unit table, the same store with every unit at the next
 * multiple of 16, the same prefixes.  The walk itself stops at the unit that ends a range, so neither the table nor the
 * store holds anything of the units behind it.
 *
 * ferhip_decs_set_input(format, length_size): from the next ferhip_decs_decode or ferhip_decs_decode_dev call on, both calls
 * take chunks of that framing.  FERHIP_E_ARG for an unknown format, and in FERHIP_IN_AVCC for a length_size outside
 * {1, 2, 4}; in FERHIP_IN_ANNEXB length_size is ignored.  The default is Annex-B, and a decoder on which the call is never
 * made behaves as before, byte for byte; the two framings may alternate from call to call on one decoder.
 * ferhip_decs_decode walks the chunks on the host, ferhip_decs_decode_dev by kernels, still with one host synchronisation
 * for the split unless its table or store has to grow.  Pictures, pictures[], status[] and the isolation rules are those
 * of the Annex-B calls given the same NAL units.  A chunk that overruns gives status[s] = FERHIP_E_ARG: the units in front
 * of the overrun decode, the stream restarts at its next IDR slice like after every other fault, the other streams are
 * untouched.
 * ferhip_decs_set_config(s, avcc, n): parses an AVCDecoderConfigurationRecord and feeds its SPS and then its PPS units to
 * stream s exactly as if they had arrived as NAL units in a chunk, with the same outcome (FERHIP_E_UNSUP for an SPS of
 * another picture size, and the stream then waits for its next IDR slice, ...).  FERHIP_E_ARG if the record is truncated,
 * its configurationVersion is not 1, it holds no SPS or no PPS, s is out of range, or the decoder is in FERHIP_IN_AVCC and
 * the record's lengthSizeMinusOne + 1 differs from the decoder's length_size.  It can be called in either input format.
 * ferhip_split_avcc_blocks: known-answer surface with the contract of ferhip_split_nal_blocks (ranges are copied so that
 * they end at the end of their allocation, `misalign` bytes past a 16-byte boundary); range_fault[r] (may be NULL) = 1 where
 * range r overran.  FERHIP_E_ARG also for a length_size outside {1, 2, 4}. */
#define FERHIP_IN_ANNEXB 0
#define FERHIP_IN_AVCC 1
int ferhip_decs_set_input(ferhip_decs *d, int format, int length_size);
int ferhip_decs_set_config(ferhip_decs *d, int s, const uint8_t *avcc, size_t n);
int ferhip_split_avcc_blocks(const uint8_t *ranges, size_t stride, const uint32_t *lens, size_t n, int misalign, int length_size,
                             uint8_t *out, size_t cap, ferhip_nal_unit *units, size_t units_cap, size_t *nunits,
                             int32_t *range_fault /* [n], may be NULL */);

/* ---- RTP input: the live decoder takes the packets of RFC 6184 (packetization-mode 1) where a receiver has them ----
 * A packet is pkts[k].bytes bytes at base + pkts[k].offset, at any alignment; the packets of stream pkts[k].stream are
 * taken in table order, and streams may interleave: the table ferhip_pack_rtp writes, and what recvmmsg leaves.
 * Per stream the state is the expected sequence number (none at first) and an open FU-A unit (none).  For a packet of L
 * bytes:
 *   1. header: L >= 12 and version b0 >> 6 == 2, else malformed.  hl = 12 + 4 CC; with X another 4 + 4 * (the u16 at
 *      hl + 2), which must lie within the packet; with the P bit pad = the last byte, >= 1; hl + pad < L, else malformed.
 *      The payload is [hl, L - pad).  The payload type and M are not looked at.
 *   2. sequence: with an expectation that seq differs from, a gap.  Then the expectation is seq + 1 mod 65536.
 *   3. payload, t = payload[0] & 31.  1..23: the payload is one unit.  24 (STAP-A): behind the first byte [u16 size][unit]
 *      to the payload's end, at least one; a size of 0 or one that overruns is malformed (the units in front of it stand).
 *      28 (FU-A): at least 2 bytes; S and E together are malformed; S opens a unit with the header byte
 *      (payload[0] & 0xE0) | (payload[1] & 0x1F); the bytes behind the FU header are appended (there may be none); E
 *      closes it; a fragment without S while none is open, S while one is open, and any other type while one is open are
 *      malformed.  Every other t is malformed.
 *   4. a unit still open when the stream's packets of this call end is truncated: a call takes whole access units.
 * The first fault ends the stream's walk (2 malformed, 3 gap, 4 truncated; 1 is the overrun of the length walk); the units
 * completed in front of it stand, and the expectation is cleared.  The units then are units of the length-prefixed
 * definition above (steps 5 to 6): header byte, RBSP without emulation prevention bytes -- one that lies across a fragment
 * seam included -- and a unit without payload ends the stream's units of the call.
 * ferhip_decs_decode_rtp: pictures, pictures[], status[] and the isolation rules are those of ferhip_decs_decode given the
 * same NAL units in Annex-B.  Every fault gives status[s] = FERHIP_E_ARG: the units in front of it decode, the stream
 * restarts at its next IDR slice, the other streams are untouched.  ferhip_decs_reset_stream clears the expectation.
 * FERHIP_E_ARG for the call, before anything is taken: pkts[k].stream >= S, a stream with more than max_pictures slices,
 * null pointers.  It may be mixed freely with the other decode calls.
 * base_on_device = 0: the depacketiser runs on the host (no synchronisation of its own).  base_on_device = 1: base is device
 * memory on the decoder's device, and nothing but the table crosses the bus: the table is sorted by stream on the host, one
 * lane per packet parses its header, one wavefront per stream walks the sequence numbers and the FU-A state, the payloads
 * are gathered behind 4-byte lengths into a staging range per stream, and the length-prefixed splitter above does the rest.
 * Two host synchronisations: one for the walk's results, one for the splitter's table (more only when a buffer had to grow).
 * ferhip_unrtp_blocks: known-answer surface of that path, context-free like ferhip_split_avcc_blocks.  The packets lie in
 * base[0, base_bytes) (host; copied to device memory `misalign` bytes behind a 16-byte boundary; a row that leaves it is
 * FERHIP_E_ARG); seq_expect[s] = the expectation stream s starts with, -1 = none; fault[s] and seq_next[s] (-1 after a fault)
 * come back; out, units (units[k].range = the stream), *nunits and the overflow rule are ferhip_split_avcc_blocks'. */
int ferhip_decs_decode_rtp(ferhip_decs *d, const void *base, int base_on_device, const ferhip_rtp_pkt *pkts /* host */, size_t npkts,
                           uint8_t *out, int out_on_device, int *pictures, int *status);
int ferhip_unrtp_blocks(const uint8_t *base, size_t base_bytes, const ferhip_rtp_pkt *pkts, size_t npkts, int nstreams, int misalign,
                        const int32_t *seq_expect /* [nstreams], -1 = none */, uint8_t *out, size_t cap, ferhip_nal_unit *units,
                        size_t units_cap, size_t *nunits, int32_t *fault /* [nstreams] */, int32_t *seq_next /* [nstreams] */);

/* ---- SRTP on the device: RTP packets protected on the way out, checked and decrypted on the way into the decoder ----
 * The profile is SRTP (RFC 3711) with its default transforms: AES-128 in counter mode, HMAC-SHA1 with an 80-bit tag, no MKI,
 * key derivation rate 0.  Not provided: a replay list, SRTCP, an MKI, the other cipher suites, a key derivation rate other
 * than 0.  AES(k, x) is the AES-128 encryption of the 16-byte block x (FIPS-197), HMAC-SHA1 that of RFC 2104 over SHA-1.
 * Session: ferhip_srtp holds, for S streams, the session keys and the packet index state (roc: u32, s_l: u16, set: 0 / 1) in
 * device memory, on the device that was current at ferhip_srtp_create.  The stream in the third column of a packet table
 * selects the row of the session.
 * Keys: ferhip_srtp_set_key(h, s, master_key[16], master_salt[14]) derives on the host, with r = 0: x_label = the 14-byte
 * salt with `label` XORed into byte 7; the session key material of a label is the first bytes of the keystream
 * AES(master_key, x_label || 00 00), AES(master_key, x_label || 00 01), ...; label 0 gives k_e (16 bytes), label 1 k_a (20),
 * label 2 k_s (14).  ferhip_srtp_derive writes k_e | k_a | k_s into out[50].  The call uploads the 176 bytes of k_e's
 * expanded round keys, k_s, and the two HMAC midstates (the SHA-1 state after the block k_a ^ 36 36 .. and after the block
 * k_a ^ 5c 5c ..), and sets roc = 0, s_l = 0, set = 0.  It waits for the device: a call in flight keeps its key.
 * Packet: a row (offset, bytes = L, stream) of a ferhip_rtp_pkt table names a packet at base + offset, at any alignment.
 * Header rule: step 1 of the RTP input definition above without its padding clause -- L >= 12 and b0 >> 6 == 2, else
 * malformed; hl = 12 + 4 CC; with X another 4 + 4 * (the u16 at hl + 2), which must lie within the packet; hl <= L, else
 * malformed.  The P bit is not examined: padding is payload and is encrypted with it.  A payload of more than 2^20 bytes
 * (65536 keystream blocks) is malformed too.
 * Index: seq = the u16 at byte 2, ssrc = the u32 at byte 8, big-endian.  If the stream's state has set == 0, then for this
 * call s_l is the seq of the stream's first well-formed row in table order (on the way in: well-formed without its tag,
 * authentic or not).  v is the estimate of RFC 3711 section 3.3.1 against the state the call started with:
 *   s_l < 32768:   v = roc - 1 when seq - s_l > 32768, else roc;
 *   otherwise:     v = roc + 1 when s_l - 32768 > seq, else roc;    all modulo 2^32, and i = v << 16 | seq (48 bits).
 * Every row of a call is estimated against the same starting state, whatever its place in the table; that is exact while a
 * stream has fewer than 32768 packets in one call.
 * Cipher: IV = k_s || 00 00 with ssrc XORed big-endian into bytes 4..7 and the 48-bit i into bytes 8..13.  Keystream block
 * b = AES(k_e, IV + b), the sum in the last two bytes (b < 65536).  Payload byte p, at packet byte hl + p, is XORed with
 * keystream byte p (byte p % 16 of block p / 16); the header's hl bytes are copied unchanged.
 * Tag: the first 10 bytes of HMAC-SHA1(k_a, packet[0, L) with the payload encrypted || v as 4 big-endian bytes), appended:
 * an SRTP packet has L + 10 bytes.
 * ferhip_srtp_protect(h, c, d_src, src_pkts, npkts, d_dst, cap, d_out_pkts): device to device, asynchronous on the stream of
 * encoder context c -- the one whose ferhip_pack_rtp wrote d_src; it waits for nothing except buffers that have to grow and
 * the table copy of the fourth call before it (src_pkts is host memory, read before the call returns).
 * ferhip_srtp_protect_dev is the same call with the table in device memory (aligned to 8), where ferhip_pack_rtp wrote it:
 * that table never comes back to the host.  There a row whose stream is >= S or has no key cannot be refused: it is
 * malformed.  Output row k = (offset: the sum over the rows in front of it of (bytes_j + 10) rounded up to 16 -- of 0 for a
 * malformed row --, bytes: L + 10, the same stream); a malformed row has bytes 0 and takes no slot.  Row npkts = (total
 * bytes, packets written, 0).  Overflow is ferhip_pack_rtp's rule, per packet: the table is always true, a packet is
 * written only if it ends within cap (offset + bytes <= cap), and no byte at or beyond cap and no byte between a packet's
 * end and the next multiple of 16 is touched.
 * ferhip_srtp_unprotect(h, d, base, base_on_device, pkts, npkts, d_dst, cap, h_out_pkts, h_status): on the stream of live
 * decoder d; it returns after one host synchronisation with the table and the status in host memory.  status[k]: 0
 * authentic, 1 the tag differs, 2 malformed -- L < 10, the header rule on the L - 10 bytes without the tag, which is also
 * L < hl + 10.  The tag is checked before anything is decrypted.  A row with status 0 is written as a plain RTP packet of
 * L - 10 bytes under the slot rule above (sizes L - 10); every other row has bytes 0 and no slot.  base_on_device = 0: the
 * range of base the rows span is copied up once; there is no host cipher.  The caller drops the rows with bytes 0 and hands
 * the rest to the RTP input call above with d_dst as its base on the device; a dropped packet is then a gap, which that
 * call isolates per stream.
 * State update, both directions: the stream's state becomes (roc, s_l, set) = (i >> 16, i & 65535, 1) for the largest i over
 * its rows of the call -- all well-formed rows on the way out, whether or not they fit cap, the status-0 rows on the way in --
 * if that i is larger than the state's own index roc << 16 | s_l or the state has set == 0; else it stays.  The state stays
 * on the device: consecutive calls continue it without the host.  ferhip_srtp_get_index reads it and ferhip_srtp_set_index
 * writes it (s_l <= 65535, set 0 or 1); both wait for the device.
 * FERHIP_E_ARG, before any HIP call: null pointers (a null table or base with npkts = 0 is fine), a null buffer with a cap,
 * a d_dst not aligned to 16 or a device table not aligned to 8, pkts[k].stream >= S in a host table, s out of range, a
 * session and a context or decoder on different devices; FERHIP_E_STATE: a host table that uses a stream whose key was
 * never set.
 * ferhip_srtp_blocks: known-answer surface, context-free and synchronous, host memory in and out, with the conventions of
 * ferhip_unrtp_blocks: the packets lie in base[0, base_bytes) (copied to device memory `misalign` bytes behind a 16-byte
 * boundary; a row that leaves it is FERHIP_E_ARG), and the bytes of out[0, cap) the kernels do not write keep the caller's
 * values.  op = FERHIP_SRTP_PROTECT or FERHIP_SRTP_UNPROTECT, anything else FERHIP_E_ARG; keys[s].set = 0: stream s has no
 * key; state_in / state_out [nstreams]: the index state before and after; out_pkts[npkts + 1]; status[npkts] (may be NULL
 * for FERHIP_SRTP_PROTECT).  It runs the same kernels.
 * Published vectors that hold (tests/test_srtp_model_host.py, tools/srtp_host_check.cpp): FIPS-197 appendix C.1, the
 * keystream of RFC 3711 B.2, the derivation of RFC 3711 B.3, HMAC-SHA1 of RFC 2202 case 1; the model the device is compared
 * with byte for byte is pinned to records made with the openssl command line (tests/golden/srtp_kat.json). */
#define FERHIP_SRTP_PROTECT 0
#define FERHIP_SRTP_UNPROTECT 1
typedef struct ferhip_srtp ferhip_srtp;
typedef struct { uint8_t master_key[16]; uint8_t master_salt[14]; uint8_t set, reserved; } ferhip_srtp_key; /* 32 bytes */
typedef struct { uint32_t roc; uint16_t s_l, set; } ferhip_srtp_index;                                       /* 8 bytes */
int ferhip_srtp_create(ferhip_srtp **out, int nstreams /* S <= 65535 */);
void ferhip_srtp_destroy(ferhip_srtp *h);
int ferhip_srtp_set_key(ferhip_srtp *h, int s, const uint8_t *master_key /* [16] */, const uint8_t *master_salt /* [14] */);
int ferhip_srtp_derive(const uint8_t *master_key, const uint8_t *master_salt, uint8_t *out /* [50] */);
int ferhip_srtp_get_index(ferhip_srtp *h, int s, uint32_t *roc, uint32_t *s_l, int *set);
int ferhip_srtp_set_index(ferhip_srtp *h, int s, uint32_t roc, uint32_t s_l, int set);
int ferhip_srtp_protect(ferhip_srtp *h, ferhip_ctx *c, const void *d_src, const ferhip_rtp_pkt *src_pkts /* host */, size_t npkts,
                        void *d_dst, size_t cap, ferhip_rtp_pkt *d_out_pkts /* [npkts + 1] */);
int ferhip_srtp_protect_dev(ferhip_srtp *h, ferhip_ctx *c, const void *d_src, const ferhip_rtp_pkt *d_src_pkts, size_t npkts,
                            void *d_dst, size_t cap, ferhip_rtp_pkt *d_out_pkts /* [npkts + 1] */);
int ferhip_srtp_unprotect(ferhip_srtp *h, ferhip_decs *d, const void *base, int base_on_device, const ferhip_rtp_pkt *pkts /* host */,
                          size_t npkts, void *d_dst, size_t cap, ferhip_rtp_pkt *h_out_pkts /* [npkts + 1] */, int32_t *h_status /* [npkts] */);
int ferhip_srtp_blocks(int op, const ferhip_srtp_key *keys, const ferhip_srtp_index *state_in, int nstreams, const uint8_t *base,
                       size_t base_bytes, const ferhip_rtp_pkt *pkts, size_t npkts, int misalign, uint8_t *out, size_t cap,
                       ferhip_rtp_pkt *out_pkts /* [npkts + 1] */, int32_t *status /* [npkts] */, ferhip_srtp_index *state_out);

/* ---- Transport stream input: the live decoder takes 188-byte packets where a receiver has them ----
 * runs[k] (host) names runs[k].bytes bytes at base + runs[k].offset: a whole number of 188-byte packets at any alignment,
 * for stream runs[k].stream.  Runs of one stream are taken in table order, streams may interleave, and two runs may name the
 * same bytes for different streams: a multi-program transport stream read by several slots.  pids[s] is the PID stream s
 * listens to.  Per stream the state is the expected continuity counter (none at first); it survives calls, and
 * ferhip_decs_reset_stream clears it.  For every packet of the stream's runs:
 *   1. b0 != 0x47 or transport_error_indicator (b1 & 0x80): malformed.
 *   2. PID != pids[s]: the packet is skipped, and nothing else of it is looked at.
 *   3. scrambling control (b3 >> 6) != 0: malformed.
 *   4. afc = (b3 >> 4) & 3.  0: malformed.  2: no payload, skipped, the counter not looked at.  1: payload [4, 188).
 *      3: a = b4, a > 183 is malformed, payload [5 + a, 188), which may be empty.  The field's content is not looked at.
 *   5. counter: with an expectation that b3 & 15 differs from, a gap (a duplicate is one, too).  Then the expectation is
 *      (b3 & 15) + 1 mod 16.
 *   6. with PUSI a PES packet begins: the payload p begins 00 00 01, its stream_id p[3] is E0..EF, (p[6] & 0xC0) == 0x80 and
 *      it holds at least 9 + p[8] bytes, else malformed.  Its elementary-stream bytes begin at 9 + p[8]; PES_packet_length,
 *      PTS and DTS are not looked at.
 *   7. without PUSI the whole payload continues the open PES packet; with none open in this call the packet is malformed: a
 *      call takes whole access units.
 * A PES packet is complete at the stream's next PUSI packet that passes these rules, or when the stream's packets of the call
 * end.  The first fault (2 malformed, 3 gap) ends the stream's walk: the PES packets completed in front of it stand, the
 * open one is dropped, and the expectation is cleared.  The elementary-stream bytes that stand, concatenated, are one
 * Annex-B range, and from there on the definition is the Annex-B splitter's and the decoder's: four-byte start codes begin
 * units, a three-byte one ends a unit and begins none, and the delimiter is a unit of type 9 that is ignored like every other
 * type the decoder does not know.
 * ferhip_decs_decode_ts: pictures, pictures[], status[] and the isolation rules are those of ferhip_decs_decode given the
 * same NAL units.  Every fault gives status[s] = FERHIP_E_ARG: the units in front of it decode, the stream restarts at its
 * next IDR slice, the other streams are untouched.  FERHIP_E_ARG for the call, before anything is taken: runs[k].stream >= S,
 * a bytes that is no multiple of 188, a pids[s] > 0x1FFF, a stream with more than max_pictures slices, null pointers.  It may
 * be mixed freely with the other decode calls.
 * base_on_device = 0: the walk runs on the host.  base_on_device = 1: base is device memory on the decoder's device and
 * nothing but the table crosses the bus: the runs are sorted by stream on the host, one lane per 188-byte packet applies
 * rules 1 to 4 and 6, one wavefront per stream walks the counter and the open PES packet with ballots and wave scans, the
 * spans that stand are gathered into one staging range per stream, and the Annex-B splitter does the rest.  Two host
 * synchronisations, more only when a buffer had to grow.  The kernels read nothing outside the runs' packets.
 * ferhip_unts_blocks: known-answer surface of that path with the conventions of ferhip_unrtp_blocks; cc_expect[s] in
 * -1..15, fault[s] and cc_next[s] (-1 after a fault) come back.
 * Not provided: PSI parsing (the caller names the PID), and splitting at three-byte start codes. */
typedef ferhip_rtp_pkt ferhip_ts_run; /* (offset, bytes: a multiple of 188, stream) */
int ferhip_decs_decode_ts(ferhip_decs *d, const void *base, int base_on_device, const ferhip_ts_run *runs /* host */, size_t nruns,
                          const uint16_t *pids /* host [S] */, uint8_t *out, int out_on_device, int *pictures, int *status);
int ferhip_unts_blocks(const uint8_t *base, size_t base_bytes, const ferhip_ts_run *runs, size_t nruns, int nstreams, int misalign,
                       const uint16_t *pids, const int32_t *cc_expect /* [nstreams], -1 = none */, uint8_t *out, size_t cap,
                       ferhip_nal_unit *units, size_t units_cap, size_t *nunits, int32_t *fault, int32_t *cc_next /* -1 after a fault */);

/* ---- MP4 fragments into the live decoder ----
 * ferhip_decs_decode_mp4 takes movie fragments as ferhip_mp4_close writes them -- or as another muxer does -- "where they
 * lie": runs[] (host) names byte ranges of base (host memory), each a whole number of
 * top-level boxes of one stream; the runs of one stream are taken in table order, and streams may interleave.
 * The box walk.  A run r[0, n) is walked from pos = 0 while pos < n:
 *  1. Box header.  Fewer than 8 bytes left: malformed.  size = the u32 at pos, type = the next four bytes, h = 8.  size 1:
 *     h = 16, fewer than 16 bytes left is malformed, and size = the u64 at pos + 8.  size 0: the box runs to the end of its
 *     container.  Otherwise size < h, or pos + size beyond the container, is malformed.  The same rule walks the children of
 *     moof and traf, and all of a container's children are walked before any of them is read.  pos advances by size >= 8.
 *  2. moof.  Its first traf that holds a trun is the track; a second such traf is unsupported; a traf without a trun is
 *     skipped.  The track's first tfhd (none: malformed): base-data-offset (flag 0x000001) is unsupported; the optional
 *     fields are skipped in order by the flags 0x2, 0x8, 0x10 (default_sample_size, kept) and 0x20; a field beyond the
 *     box is malformed.  Every trun in order: version above 1 is unsupported; sample_count; data_offset (0x1, signed);
 *     first_sample_flags (0x4, skipped); then per sample duration (0x100, skipped), size (0x200), flags (0x400, skipped),
 *     composition offset (0x800, skipped); fields or entries beyond the box are malformed.  A sample's size is its
 *     entry's, else the tfhd default; with neither (and a count above 0) malformed.  The first trun must carry a
 *     data_offset, else unsupported; its samples begin at the moof's first byte + data_offset and follow each other; a
 *     later trun begins at its own data_offset, or behind the previous trun's samples.  A trun without any per-sample
 *     field has entries of no bytes, so nothing above bounds its count: it is malformed if it would bring the samples of
 *     its run (those of the fragments in front included) above the run's n bytes.
 *  3. mdat.  With a moof pending, every one of its samples must lie inside this box's content, else malformed; the
 *     samples then stand, in order.  Without a pending moof the box is skipped.
 *  4. A moof still pending at another moof or at the run's end is truncated: a call takes whole fragments.
 *  5. Every other type is skipped by its size: ftyp, styp, moov, sidx, free, skip, emsg and anything unknown.
 * Faults: 2 malformed, 3 unsupported, 4 truncated, and 1 the overrun of the length walk inside a sample.  The first fault
 * ends the stream's walk; the samples of the fragments completed in front of it stand.  Each standing sample is one range of
 * the length-prefixed definition above with L = length_size in {1, 2, 4}; a sample of size 0 holds no units; behind a
 * sample whose walk overruns, nothing more of the stream is taken.
 * Pictures, pictures[], status[] and the isolation rules are those of ferhip_decs_decode given the same NAL units; every
 * fault gives status[s] = FERHIP_E_ARG: the units in front of it decode, the stream restarts at its next IDR slice, the other
 * streams are untouched.  Refused before anything is taken (FERHIP_E_ARG), as ferhip_decs_decode_ts refuses: null
 * pointers, a stream outside [0, S), a length_size outside {1, 2, 4}, and a call in which a stream's units hold more
 * slices than max_pictures.  The call mixes freely with the other decode calls and does not depend on
 * ferhip_decs_set_input.  The parameter sets come inside the IDR samples (FERHIP_AU_PARAM_SETS) or from
 * ferhip_decs_set_config with the record that ferhip_mp4_find_avcc finds in the initialisation segment.
 * base_on_device = 0: the walk runs on the host (split_mp4), without a synchronisation of its own.  base_on_device = 1 is
 * not provided yet and returns FERHIP_E_UNSUP before anything is taken: a device walk needs the length-prefixed splitter to
 * take its ranges from a table in device memory, which it does not do yet.  Until then a receiver whose fragments lie in
 * device memory copies them to the host, or hands the decoder the samples as FERHIP_IN_AVCC chunks.
 * ferhip_mp4_find_avcc (host): walks moov, trak, mdia, minf, stbl, stsd of an initialisation segment; behind the 8 bytes of
 * stsd the first entry must be avc1 or avc3, and behind the 78 bytes of its visual sample entry the child avcC is looked
 * for; off and len name that child's content.  FERHIP_E_ARG if anything is missing or overruns. */
typedef ferhip_rtp_pkt ferhip_mp4_run; /* (offset, bytes, stream): a whole number of top-level boxes */
int ferhip_decs_decode_mp4(ferhip_decs *d, const void *base, int base_on_device, const ferhip_mp4_run *runs /* host */, size_t nruns,
                           int length_size, uint8_t *out, int out_on_device, int *pictures, int *status);
int ferhip_mp4_find_avcc(const uint8_t *init, size_t n, size_t *off, size_t *len);

/* ---- Y4M ingest (row f3): LoadY4MHeader / ReadFromY4M of F/fileIO.cpp:228-346 without the globals ----
 * The picture size comes from the header's " W" / " H" tokens; coded size = cropped to multiples of 16 around the
 * centre, as the reference does (a caller that wants every sample coded reads the file itself and uses "display size" above).  ferhip_y4m_read fills one coded-size I420 picture (use pinned memory when it feeds ferhip_set_frames);
 * returns 0, or 1 at the end of the stream. */
typedef struct ferhip_y4m ferhip_y4m;
int ferhip_y4m_open(ferhip_y4m **out, const char *path, int *in_width, int *in_height, int *coded_width, int *coded_height);
int ferhip_y4m_read(ferhip_y4m *y, unsigned char *dst);
void ferhip_y4m_close(ferhip_y4m *y);
/* emit, F/fileIO.cpp:100-176: the stream header "YUV4MPEG2 C420jpeg W%d H%d F24:1 Ip A1:1\n" and one picture
 * ("FRAME\n" + I420 when with_frame_line, bare I420 = writeToYUV otherwise); file = a FILE* */
int ferhip_y4m_write_header(void *file, int width, int height);
int ferhip_y4m_write_frame(void *file, const unsigned char *i420, int width, int height, int with_frame_line);

/* ---- block-level KAT surface: the reference's own signatures as batched device calls ----
 * forwardResidual(qP, c, r, Intra, Intra16x16OrChroma), F/quantizationTransform.h:
 * n blocks of 16 int32 (raster) in, 16 int32 out. */
int ferhip_forward_residual(int qP, const int32_t *in, int32_t *out, int keep_dc, size_t nblocks);
/* inverseResidual(bitDepth, qP, c, r, intra16x16OrChroma), F/scaleTransform.h */
int ferhip_inverse_residual(int qP, const int32_t *in, int32_t *out, int keep_dc, size_t nblocks);
/* forwardDCLumaIntra(qP, dcY, c) (F/quantizationTransform.cpp:293) / InverseDCLumaIntra(bitDepth, qP, c, dcY)
 * (F/scaleTransform.h): 16 int32 raster in, 16 out */
int ferhip_forward_dc_luma_intra(int qP, const int32_t *in, int32_t *out, size_t nblocks);
int ferhip_inverse_dc_luma_intra(int qP, const int32_t *in, int32_t *out, size_t nblocks);
/* forwardDCChroma(qP, dcC, c, Intra) (F/quantizationTransform.cpp:303) / InverseDCChroma: the 2x2 block (raster) in
 * slots 0..3 of a 16-int32 record, the rest ignored / zero */
int ferhip_forward_dc_chroma(int qP, const int32_t *in, int32_t *out, size_t nblocks);
int ferhip_inverse_dc_chroma(int qP, const int32_t *in, int32_t *out, size_t nblocks);
/* transformScan(c, list, Intra16x16AC) (F/quantizationTransform.cpp:310; AC variant: 15 entries from index 1,
 * = scanChroma) and transformInverseScan(list, c) (F/scaleTransform.cpp:454) */
int ferhip_transform_scan(const int32_t *in, int32_t *out, int intra16x16_ac, size_t nblocks);
int ferhip_transform_inverse_scan(const int32_t *in, int32_t *out, size_t nblocks);

/* ---- per-macroblock unit-parity surface (SURVEY.md 8b "per-MB"): the reference's macroblock-level functions as batched
 * device calls over the same device functions the encode / decode kernels are built from.  A seam for known-answer tests,
 * not a fast path.  Arrays use the reference's own layouts: samples raster [y][x], levels per luma4x4BlkIdx in scan order
 * (the Intra16x16 AC / chroma AC lists hold 15 entries from index 0). */
#define FERHIP_MBU_QT 0    /* quantizationTransform(predL, predCb, predCr, reconstruct), F/quantizationTransform.cpp:349 */
#define FERHIP_MBU_DEC4 1  /* transformDecoding4x4LumaResidual(LumaLevel, predL, luma4x4BlkIdx, QPy), F/inttransform.cpp:133 */
#define FERHIP_MBU_DEC16 2 /* transformDecodingIntra_16x16Luma(DC, AC, predL, QPy), F/inttransform.cpp:157 */
#define FERHIP_MBU_DECC 3  /* transformDecodingChroma(DC, AC, predC, QPy, Cb) for both planes, F/inttransform.cpp:237 */
#define FERHIP_MBU_SKIP 4  /* transformDecodingP_Skip(predL, predCb, predCr, QPy), F/inttransform.cpp:215 */
typedef struct {
    int32_t op, cls /* MbPartPredMode(mb_type,0): 0 Intra_4x4, 1 Intra_16x16, 2 inter */, qp /* QPy */, qpc /* QPc */, reconstruct, blk;
    int32_t srcY[256], srcCb[64], srcCr[64];    /* the macroblock of `frame` (FERHIP_MBU_QT) */
    int32_t predY[256], predCb[64], predCr[64];
    int32_t lumaLevel[16][16], dc16[16], ac16[16][16], cdc[2][4], cac[2][4][16]; /* levels in (decode-side ops) */
} ferhip_mb_job;
typedef struct {
    int32_t lumaLevel[16][16], dc16[16], ac16[16][16], cdc[2][4], cac[2][4][16]; /* levels out (FERHIP_MBU_QT) */
    int32_t recY[256], recCb[64], recCr[64];    /* samples written into `frame` (0 where the call writes none) */
} ferhip_mb_result;
int ferhip_mb_unit(const ferhip_mb_job *jobs, ferhip_mb_result *results, size_t njobs);
/* residual_block_cavlc_write(coeffLevel, 0, maxNumCoeff - 1, maxNumCoeff) (F/residual.cpp:374) for n blocks with nC given
 * (-1 = chroma DC): bits[n][64] receives each block's code MSB first, nbits[n] its length -- also what
 * residual_block_cavlc_size (F/residual.cpp:673) returns; the call fails if the device's counting form disagrees --,
 * total_coeff[n] the TotalCoeff the block leaves for its neighbours */
int ferhip_cavlc_blocks(const int32_t *coef, const int32_t *nC, const int32_t *max_num_coeff, size_t nblocks, uint8_t *bits,
                        uint32_t *nbits, int32_t *total_coeff);
/* residual_block_cavlc(coeffLevel, 0, maxNumCoeff - 1, maxNumCoeff) (F/residual.cpp:1069) for n blocks with nC given
 * (-1 = chroma DC).  Block i is read from bit position bit_pos[i] (MSB first) of the nbytes bytes at `bits`.
 * coef[n][16] receives the levels (zero behind maxNumCoeff).
 * total_coeff[n] receives TotalCoeff, or -1 for a malformed block (its coef row is then all zero); a block that runs
 * past the end of the stream is malformed.
 * bits_used[n] receives the bits consumed (undefined where total_coeff is -1).
 * nbytes is at most 2^28 (the device reader keeps bit positions in 32 bits). */
int ferhip_cavlc_parse_blocks(const uint8_t *bits, size_t nbytes, const uint64_t *bit_pos, const int32_t *nC,
                              const int32_t *max_num_coeff, size_t nblocks, int32_t *coef, int32_t *total_coeff,
                              uint32_t *bits_used);
/* The residual of one macroblock with nC derived from its neighbours, both directions: residual_write() through the
 * encoder's block order and cavlc_nC, residual(0, 15) through the decoder's dec_block and dec_nC.  A job is one macroblock
 * and the state of its left (A) and upper (B) neighbours; levels use the layouts of ferhip_mb_job and must fit 16 bits.
 * cbp_luma is 0..15 (0 or 15 for cls 1), cbp_chroma 0..2; a neighbour's tc entries are 0..16.
 * WRITE reports 0 in the tc entries of the blocks the CBP leaves out (the reference leaves those entries as they were);
 * PARSE zeroes their levels and counts, as residual() does.  Of the level arrays PARSE fills lumaLevel (cls 0, 2) or dc16
 * and ac16 (cls 1), cdc and cac; the others come back zero. */
#define FERHIP_RES_WRITE 0 /* residual_write(), F/residual.cpp:300-372 */
#define FERHIP_RES_PARSE 1 /* residual(0, 15),  F/residual.cpp:959-1067 */
#define FERHIP_RES_BITS_MAX 2048
typedef struct {
    int32_t p_skip, cbp_luma, cbp_chroma, tc_luma[16], tc_chroma[2][4];
} ferhip_res_nb;
typedef struct {
    int32_t op, cls /* MbPartPredMode(mb_type, 0) as in ferhip_mb_job */, cbp_luma, cbp_chroma;
    int32_t avail;                                                                /* bit 0: mbAddrA exists, bit 1: mbAddrB exists */
    ferhip_res_nb nb[2];                                                          /* A, B (ignored where not available) */
    int32_t lumaLevel[16][16], dc16[16], ac16[16][16], cdc[2][4], cac[2][4][16]; /* WRITE: in (layouts of ferhip_mb_job) */
    uint32_t bit_pos, nbytes;                                                     /* PARSE: in */
    uint8_t bits[FERHIP_RES_BITS_MAX];                                            /* PARSE: in */
} ferhip_res_job;
typedef struct {
    int32_t nbits;                        /* bits written / consumed; -1: malformed (PARSE) or longer than the buffer (WRITE) */
    int32_t tc_luma[16], tc_chroma[2][4]; /* what the macroblock leaves for its neighbours (the reference's TotalCoeff arrays) */
    int32_t lumaLevel[16][16], dc16[16], ac16[16][16], cdc[2][4], cac[2][4][16]; /* PARSE: out */
    uint8_t bits[FERHIP_RES_BITS_MAX];    /* WRITE: out, MSB first */
} ferhip_res_result;
int ferhip_residual_mbs(const ferhip_res_job *jobs, ferhip_res_result *results, size_t njobs);
/* ---- the neighbourhood seam: intra prediction and motion-vector derivation of one macroblock among its neighbours.
 * A job carries a picture of 3 x 2 macroblocks (48 x 32 luma, two 24 x 16 chroma planes), the smallest in which a macroblock
 * can have every neighbour the rules read -- A (left), B (above), C (above right), D (above left) --, and pos, the address
 * of its macroblock in that picture.  Which neighbours exist follows from pos exactly as in a real picture:
 *     pos 0: none    1: A    2: A (last column)    3: B, C    4: A, B, C, D    5: A, B, D (no C: last column)
 * Job j is stream j of a context of such pictures over a hand-built FerDev, so the job runs the device code a real picture
 * runs: k_intra_mb, k_dec_intra, dec_i4_modes, dec_derive_mvs, predict_luma_tbl.  mb[m] is the side information of
 * macroblock m of the little picture; only the entries in front of pos (raster order) are read, plus mb[pos] where stated.
 * mb_type is in the numbering of the job's slice_type (I: 0 I_4x4, 1..24 Intra16x16; P: 0..4 inter, 5 I_4x4, 6..29
 * Intra16x16) or 31, P_Skip, under either; I_PCM is not part of the surface.  mv holds one vector per 8x8 quadrant in quarter
 * samples, as the decoder and the encoder keep them: the quadrants that one partition of mb_type covers carry its vector.
 * What this surface cannot reach: a picture ONE macroblock wide, where B exists without C and D and the macroblock is in
 * the first and the last column at once; that stays with the whole pictures of tests/test_gpu_hard_content.py. */
typedef struct {
    int32_t mb_type;
    int32_t cbp_luma, cbp_chroma;         /* 0..15, 0..2 */
    int32_t tc_luma[16], tc_chroma[2][4]; /* TotalCoeff, 0..16 */
    int32_t i4mode[16];                   /* Intra4x4PredMode, 0..8 (read where mb_type is I_4x4) */
    int32_t mv[4][2];                     /* (x, y) of quadrant 0..3, each within 16 bits (read where mb_type is inter) */
} ferhip_nb_mb;
#define FERHIP_NB_W 48
#define FERHIP_NB_H 32
#define FERHIP_NB_MBS 6

/* FERHIP_INTRA_ENCODE = intraPredictionEncoding (F/intra.cpp:949) and the tail of RBSP_encode for an I macroblock
 * (F/rbsp_encoding.cpp:194-219): slice_type must be 2.  In: the picture with the source at pos and the reconstruction
 * elsewhere, qp, mb[pos].mb_type = the stale mb_type_array entry the first coded_mb_size call reads (see
 * FERHIP_BUF_MBSIZE: 31, a P_Skip left by the previous picture, changes the size estimate), the neighbours in front of pos.
 * The body is k_intra_mb.  Out: ret = what the function returns (the Intra16x16 mode 0..3, or -1 for Intra4x4), i4mode,
 * chroma_mode, mbsize = the two coded_mb_size values (F/rbsp_encoding.cpp:330; [0] the Intra16x16, [1] the Intra4x4
 * alternative: the only two the reference ever asks for), the final mb_type, cbp, tc (the non-zero levels of every block's
 * list; Intra16x16: of its AC list), the levels (lumaLevel for Intra4x4, dc16 and ac16 for Intra16x16, cdc, cac; the others
 * zero), the reconstructed macroblock, predL / predCb / predCr as the function leaves them (evaluated by the decode-side
 * predictors on the reconstruction), and prev_flag / rem_mode as the macroblock layer writes them.
 * FERHIP_INTRA_DECODE = intraPrediction (F/intra.cpp:770) with getIntra4x4PredMode, in an I or a P slice (slice_type 2 or
 * 0), and the reconstruction of the macroblock.  In: mb[pos].mb_type (intra), prev_flag, rem_mode, chroma_mode,
 * constrained_intra, qp, chroma_qp_offset (-12..12), the levels (within 16 bits), the picture (the macroblock's own samples
 * are ignored), the neighbours in front of pos.  The body is dec_i4_modes followed by k_dec_intra.  Out: i4mode (Intra4x4),
 * predL / predCb / predCr, the reconstructed macroblock; ret, mb_type, chroma_mode repeat the input, the rest is zero.
 * Jobs are legal only: a prediction mode that reads a neighbour pos does not provide is refused with FERHIP_E_ARG (what the
 * decoder does with such modes is pinned on whole pictures, tests/test_gpu_decode_illegal.py). */
#define FERHIP_INTRA_ENCODE 0
#define FERHIP_INTRA_DECODE 1
typedef struct {
    int32_t op, pos, slice_type, qp, chroma_qp_offset, constrained_intra;
    int32_t chroma_mode, prev_flag[16], rem_mode[16];                             /* DECODE: in */
    ferhip_nb_mb mb[FERHIP_NB_MBS];
    uint8_t Y[FERHIP_NB_H][FERHIP_NB_W], Cb[FERHIP_NB_H / 2][FERHIP_NB_W / 2], Cr[FERHIP_NB_H / 2][FERHIP_NB_W / 2];
    int32_t lumaLevel[16][16], dc16[16], ac16[16][16], cdc[2][4], cac[2][4][16]; /* DECODE: in (layouts of ferhip_mb_job) */
} ferhip_intra_job;
typedef struct {
    int32_t ret, mb_type, cbp_luma, cbp_chroma, chroma_mode, mbsize[2];
    int32_t i4mode[16], prev_flag[16], rem_mode[16];
    int32_t tc_luma[16], tc_chroma[2][4];
    int32_t lumaLevel[16][16], dc16[16], ac16[16][16], cdc[2][4], cac[2][4][16];
    int32_t recY[256], recCb[64], recCr[64];
    int32_t predL[256], predCb[64], predCr[64];
} ferhip_intra_result;
int ferhip_intra_mbs(const ferhip_intra_job *jobs, ferhip_intra_result *results, size_t njobs);

/* FERHIP_MV_DERIVE = DeriveMVs (F/mode_pred.cpp:428) in a P slice, through the decoder's dec_derive_mvs.  In: pos, mb_type
 * (0..4, or 31 P_Skip), sub_mb_type (0..3, read for mb_type 3 and 4), mvd (the vector difference of partition i, for P_8x8
 * of the first sub-partition of quadrant i; |mvd| <= 65536), the neighbours' mb_type and mv.  Out: mv, and fits = 0 when a
 * component leaves 16 bits: the device keeps vectors in 16 bits and refuses the picture there, the reference keeps ints
 * (mv is then undefined).
 * FERHIP_MV_PREDICT = the encoder's direction: given the macroblock's final mv and mb_type (0..4; the quadrants of one
 * partition equal, sub_mb_type 0, every neighbour inter, as in the encoder's P pictures), the mvd that k_p_resid writes,
 * through its predictor predict_luma_tbl.  Out: mvd (zero behind the last partition).  DERIVE of it gives mv back. */
#define FERHIP_MV_DERIVE 0
#define FERHIP_MV_PREDICT 1
typedef struct {
    int32_t op, pos, mb_type, sub_mb_type[4];
    int32_t mvd[4][2]; /* DERIVE: in */
    int32_t mv[4][2];  /* PREDICT: in */
    ferhip_nb_mb mb[FERHIP_NB_MBS];
} ferhip_mv_job;
typedef struct {
    int32_t mv[4][2], mvd[4][2], fits;
} ferhip_mv_result;
int ferhip_mv_mbs(const ferhip_mv_job *jobs, ferhip_mv_result *results, size_t njobs);

/* All seven entry points of this surface check their arguments before the first HIP call and return FERHIP_E_ARG for a null
 * pointer, n == 0, max_num_coeff outside {4, 15, 16}, nC < -1, nC == -1 with max_num_coeff != 4, an op, cls, blk, qp, qpc,
 * cbp, avail, sub / part index or macroblock address out of range, a bit_pos at or behind 8 * nbytes, nbytes == 0 or above
 * its limit; the two calls of the neighbourhood seam also for a pos, slice_type, chroma_qp_offset, mb_type, tc, prediction
 * mode, flag, sub type or vector out of range, for levels outside 16 bits and for a job that is not legal. */
/* MotionCompensateSubMBPart(predL, predCr, predCb, refPic, mbPartIdx, subMbIdx, subMbPartIdx) (F/mocomp.cpp:152) for n
 * sub-blocks of one reference picture (host I420, width x height): desc[n][5] = macroblock address, subMbIdx, subMbPartIdx,
 * mvx, mvy (quarter samples); predL[n][16] = the 4x4 luma block, predCb / predCr[n][4] = the 2x2 chroma blocks (raster).
 * Chroma is also evaluated through the four-samples-per-row form the residual kernel uses; the call fails if they differ. */
int ferhip_mc_sub_mb_parts(const uint8_t *ref_i420, int width, int height, const int32_t *desc, size_t n, int32_t *predL,
                           int32_t *predCb, int32_t *predCr);

#ifdef __cplusplus
}
#endif
#endif
