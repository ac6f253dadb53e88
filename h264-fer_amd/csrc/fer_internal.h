// fer_internal.h -- host-side declarations shared by the translation units of libferhip.
#pragma once
#include "fer_dev.h"
#include "../../include/ferhip.h"

struct FerSortTmp {
    uint4 *rec1;        // [S][n] plane-0 records + position (k0|k1, k2|k3, k4, tx<<16|ty) after the first radix pass
    uint16_t *keyT;     // [S][W][H] sort keys in arrival order
    uint8_t *dig2;      // [S][n] high digit of the keys after the first pass
    uint16_t *skey;     // [S][n] sorted keys
    uint32_t *rec_tmp;  // [S][n][3] plain sorted records of streams that take the reference's mis-filed layout 
    void *tmp;          // digit histograms
    size_t tmp_bytes;
};

size_t fer_sort_tmp_bytes(int n, int S);
void fer_launch_refprep(const FerDev &d, FerSortTmp &t, const int *types, hipStream_t st);
void fer_launch_interp(const FerDev &d, hipStream_t st);
void fer_launch_features(const FerDev &d, hipStream_t st);
void fer_launch_sort(const FerDev &d, FerSortTmp &t, hipStream_t st);
void fer_launch_sort_keys(const FerDev &d, FerSortTmp &t, hipStream_t st);
void fer_launch_sort_radix(const FerDev &d, FerSortTmp &t, hipStream_t st);
void fer_launch_sort_finish(const FerDev &d, FerSortTmp &t, hipStream_t st);
void fer_launch_me_walk(const FerDev &d, hipStream_t st);
// skip: device [S], non-zero = the stream takes no part (null = every stream does)
void fer_launch_frame_sad(const FerDev &d, const uint8_t *skip, hipStream_t st);
void fer_launch_me_pre(const FerDev &d, hipStream_t st);
void fer_launch_me_spec(const FerDev &d, hipStream_t st);
void fer_launch_me_resolve(const FerDev &d, hipStream_t st);
void fer_launch_basic_stat(const FerDev &d, hipStream_t st);
void fer_launch_p_resid(const FerDev &d, hipStream_t st);
void fer_launch_type_count(const FerDev &d, hipStream_t st);
void fer_launch_intra(const FerDev &d, hipStream_t st);
void fer_launch_intra_diag(const FerDev &d, int diag, hipStream_t st);  // one anti-diagonal of k_intra_mb
void fer_launch_cavlc(const FerDev &d, hipStream_t st);
void fer_launch_rc_plan(const FerDev &d, hipStream_t st);
int fer_quality_groups(const FerDev &d);
void fer_launch_quality(const FerDev &d, int flags, int slot, hipStream_t st);
void fer_launch_carry_ref(const FerDev &d, hipStream_t st);
void fer_launch_reset_stream(const FerDev &d, int s, int qpw, hipStream_t st);
// the decode tables of the current device (DecLuts of fer_decode_dev.h), built on first use on stream st and waited for;
// null if they cannot be allocated
struct DecLuts;
const DecLuts *dec_luts(hipStream_t st);
void fer_launch_decode_parse(const FerDev &d, const DecBatch &B, hipStream_t st);
void fer_launch_decode_recon(const FerDev &dslice, bool anyP, bool anyIntra, hipStream_t st);
void fer_launch_decode_intra_diag(const FerDev &dslice, int diag, hipStream_t st);  // one anti-diagonal of k_dec_intra
// map[j] = (stream, slot): picture of stream map[j].x in `set` -> dst + map[j].y * W*H*3/2 (I420), for j < n; dst is
// 16-byte aligned (any other output of the live decoder goes through fer_launch_pic_emit_slots)
void fer_launch_decode_out(const FerDev &d, const uint8_t *set, const int2 *map, int n, uint8_t *dst, hipStream_t st);
// display-size ingest (fer_pic.hip): src = [S][dw*dh*3/2] I420 in device memory, any alignment -> `set`, padded by edge
// replication to the coded size; present: device [S], 0 = the stream is left out (null = every stream)
void fer_launch_pad_ingest(const FerDev &d, uint8_t *set, const uint8_t *src, int dw, int dh, const uint8_t *present, hipStream_t st);
// pictures by descriptor (fer_pic.hip).  d_pics: device [S], a stream with plane[0] == NULL is left out.
// ingest: pitched I420 / NV12 pictures of dw x dh -> `set`, padded by edge replication to the coded size
void fer_launch_pic_ingest(const FerDev &d, uint8_t *set, const ferhip_pic *d_pics, int format, int dw, int dh, hipStream_t st);
// emit: the window win = (x0, y0, dw, dh) of every stream's picture in `set` -> through its descriptor ...
void fer_launch_pic_emit(const FerDev &d, const uint8_t *set, const ferhip_pic *d_pics, int format, const int *win, hipStream_t st);
// ... or, for the pictures map[j] = (stream, slot), j < n, -> the pitched slot at dst + slot * slot_bytes (Y, then Cb, Cr or CbCr)
void fer_launch_pic_emit_slots(const FerDev &d, const uint8_t *set, const int2 *map, int n, uint8_t *dst, int format, uint32_t pitch_y,
                               uint32_t pitch_c, size_t slot_bytes, const int *win, hipStream_t st);
// the same two ways for the packed formats (FERHIP_FMT_YUY2, UYVY, BGRA, RGBA), converted in the pass; csc = FERHIP_CSC_*.
// emit: through d_pics (n = S), or, with d_pics null, the pictures map[j], j < n, to the slots of `pitch` * dh bytes in dst
void fer_launch_pic_ingest_packed(const FerDev &d, uint8_t *set, const ferhip_pic *d_pics, int format, int csc, int dw, int dh, hipStream_t st);
void fer_launch_pic_emit_packed(const FerDev &d, const uint8_t *set, const ferhip_pic *d_pics, const int2 *map, int n, uint8_t *dst, int format,
                                int csc, uint32_t pitch, size_t slot_bytes, const int *win, hipStream_t st);
