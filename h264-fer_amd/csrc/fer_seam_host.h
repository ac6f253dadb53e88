// fer_seam_host.h -- argument checks of the per-macroblock unit-parity surface (ferhip_mb_unit, ferhip_cavlc_blocks,
// ferhip_cavlc_parse_blocks, ferhip_residual_mbs, ferhip_mc_sub_mb_parts, ferhip_intra_mbs, ferhip_mv_mbs; fer_mbunit.hip).
// The kernels behind these entry points index device tables and LDS with what the caller states (QP, block and macroblock
// indices, nC, maxNumCoeff, bit positions, prediction modes), so every call is checked here before its first HIP call.
// Plain C++ without the HIP runtime, so that it can be compiled into a stand-alone host program and run under a sanitizer
// (tools/seam_host_check.cpp, tools/seam_nbhd_host_check.cpp).
#pragma once
#include "../../include/ferhip.h"
#include <stddef.h>
#include <stdint.h>

// the device bit reader keeps bit positions in 32 bits: streams of ferhip_cavlc_parse_blocks stay below 2^28 bytes
#define FER_SEAM_STREAM_MAX ((size_t)1 << 28)
// the kernels count blocks and jobs in an int; a job with its result is 10 KB
#define FER_SEAM_BLOCKS_MAX ((size_t)1 << 30)
#define FER_SEAM_JOBS_MAX ((size_t)1 << 20)

static inline bool fer_seam_in(int32_t v, int32_t lo, int32_t hi) { return v >= lo && v <= hi; }

// one CAVLC block: maxNumCoeff is 4 (chroma DC), 15 (Intra16x16 AC, chroma AC) or 16; nC >= -1, and -1 (chroma DC) goes
// with maxNumCoeff 4 only
static inline bool fer_seam_block_ok(int32_t nC, int32_t max_num_coeff)
{
    if (max_num_coeff != 4 && max_num_coeff != 15 && max_num_coeff != 16) return false;
    if (nC < -1) return false;
    return nC != -1 || max_num_coeff == 4;
}

static inline int fer_seam_check_mb_unit(const ferhip_mb_job *jobs, const ferhip_mb_result *results, size_t n)
{
    if (!jobs || !results || n == 0) return FERHIP_E_ARG;
    for (size_t i = 0; i < n; i++) {
        const ferhip_mb_job &J = jobs[i];
        if (!fer_seam_in(J.op, FERHIP_MBU_QT, FERHIP_MBU_SKIP) || !fer_seam_in(J.cls, 0, 2) || !fer_seam_in(J.qp, 0, 51) ||
            !fer_seam_in(J.qpc, 0, 51) || !fer_seam_in(J.blk, 0, 15))
            return FERHIP_E_ARG;
    }
    return 0;
}

static inline int fer_seam_check_cavlc_blocks(const int32_t *coef, const int32_t *nC, const int32_t *max_num_coeff, size_t n, const uint8_t *bits,
                                              const uint32_t *nbits, const int32_t *total_coeff)
{
    if (!coef || !nC || !max_num_coeff || !bits || !nbits || !total_coeff || n == 0) return FERHIP_E_ARG;
    for (size_t i = 0; i < n; i++)
        if (!fer_seam_block_ok(nC[i], max_num_coeff[i])) return FERHIP_E_ARG;
    return 0;
}

static inline int fer_seam_check_parse_blocks(const uint8_t *bits, size_t nbytes, const uint64_t *bit_pos, const int32_t *nC,
                                              const int32_t *max_num_coeff, size_t n, const int32_t *coef, const int32_t *total_coeff,
                                              const uint32_t *bits_used)
{
    if (!bits || !bit_pos || !nC || !max_num_coeff || !coef || !total_coeff || !bits_used || n == 0) return FERHIP_E_ARG;
    if (nbytes == 0 || nbytes > FER_SEAM_STREAM_MAX || n > FER_SEAM_BLOCKS_MAX) return FERHIP_E_ARG;
    for (size_t i = 0; i < n; i++)
        if (!fer_seam_block_ok(nC[i], max_num_coeff[i]) || bit_pos[i] >= (uint64_t)nbytes * 8) return FERHIP_E_ARG;
    return 0;
}

// desc[n][5] = macroblock address, subMbIdx, subMbPartIdx, mvx, mvy of a width x height picture (the vectors may point
// anywhere: the interpolation clamps coordinates, it never indexes with them)
static inline int fer_seam_check_mc_parts(const uint8_t *ref_i420, int width, int height, const int32_t *desc, size_t n, const int32_t *predL,
                                          const int32_t *predCb, const int32_t *predCr)
{
    if (!ref_i420 || !desc || !predL || !predCb || !predCr || n == 0 || width <= 0 || height <= 0 || (width & 15) || (height & 15))
        return FERHIP_E_ARG;
    const int64_t nmb = (int64_t)(width >> 4) * (height >> 4);
    for (size_t i = 0; i < n; i++)
        if (desc[i * 5] < 0 || desc[i * 5] >= nmb || !fer_seam_in(desc[i * 5 + 1], 0, 3) || !fer_seam_in(desc[i * 5 + 2], 0, 3)) return FERHIP_E_ARG;
    return 0;
}

// the block-level KATs (ferhip_forward_residual .. ferhip_transform_inverse_scan): any number of blocks, none included
static inline int fer_seam_check_block_kat(int qP, const int32_t *in, const int32_t *out)
{
    return (!in || !out || qP < 0 || qP > 51) ? FERHIP_E_ARG : 0;
}

static inline bool fer_seam_levels16(const int32_t *v, size_t n)  // the device keeps levels in 16 bits
{
    for (size_t i = 0; i < n; i++)
        if (v[i] < -32768 || v[i] > 32767) return false;
    return true;
}

static inline int fer_seam_check_residual_mbs(const ferhip_res_job *jobs, const ferhip_res_result *results, size_t n)
{
    if (!jobs || !results || n == 0 || n > FER_SEAM_JOBS_MAX) return FERHIP_E_ARG;
    for (size_t i = 0; i < n; i++) {
        const ferhip_res_job &J = jobs[i];
        if (!fer_seam_in(J.op, FERHIP_RES_WRITE, FERHIP_RES_PARSE) || !fer_seam_in(J.cls, 0, 2) || !fer_seam_in(J.cbp_luma, 0, 15) ||
            !fer_seam_in(J.cbp_chroma, 0, 2) || !fer_seam_in(J.avail, 0, 3))
            return FERHIP_E_ARG;
        if (J.cls == 1 && J.cbp_luma != 0 && J.cbp_luma != 15) return FERHIP_E_ARG;  // Intra16x16: all of the AC blocks or none
        for (int k = 0; k < 2; k++) {
            if (!(J.avail & (1 << k))) continue;  // nothing of an absent neighbour is looked at
            const ferhip_res_nb &N = J.nb[k];
            if (!fer_seam_in(N.p_skip, 0, 1) || !fer_seam_in(N.cbp_luma, 0, 15) || !fer_seam_in(N.cbp_chroma, 0, 2)) return FERHIP_E_ARG;
            for (int b = 0; b < 16; b++)
                if (!fer_seam_in(N.tc_luma[b], 0, 16)) return FERHIP_E_ARG;
            for (int b = 0; b < 8; b++)
                if (!fer_seam_in(N.tc_chroma[b >> 2][b & 3], 0, 16)) return FERHIP_E_ARG;
        }
        if (J.op == FERHIP_RES_PARSE) {
            if (J.nbytes == 0 || J.nbytes > FERHIP_RES_BITS_MAX || J.bit_pos >= J.nbytes * 8u) return FERHIP_E_ARG;
        } else if (!fer_seam_levels16(&J.lumaLevel[0][0], 256) || !fer_seam_levels16(J.dc16, 16) || !fer_seam_levels16(&J.ac16[0][0], 256) ||
                   !fer_seam_levels16(&J.cdc[0][0], 8) || !fer_seam_levels16(&J.cac[0][0][0], 128)) {
            return FERHIP_E_ARG;
        }
    }
    return 0;
}

// ---- the neighbourhood seam (ferhip_intra_mbs, ferhip_mv_mbs): a macroblock at pos of a 3 x 2-macroblock picture
// neighbours that pos provides: bit 0 = A (pos - 1), 1 = B (pos - 3), 2 = C (pos - 2), 3 = D (pos - 4)
static inline int fer_seam_pos_nb(int pos)
{
    static const int k[FERHIP_NB_MBS] = {0, 1, 1, 2 | 4, 1 | 2 | 4 | 8, 1 | 2 | 8};
    return k[pos];
}
// mb_type in the numbering of slice_type (2 = I, 0 = P); 31 = P_Skip under either; no I_PCM
static inline bool fer_seam_mb_type_ok(int32_t t, int32_t slice_type) { return t == 31 || fer_seam_in(t, 0, slice_type == 2 ? 24 : 29); }
static inline bool fer_seam_is_i4(int32_t t, int32_t slice_type) { return t == (slice_type == 2 ? 0 : 5); }
static inline bool fer_seam_is_i16(int32_t t, int32_t slice_type) { return slice_type == 2 ? fer_seam_in(t, 1, 24) : fer_seam_in(t, 6, 29); }
static inline bool fer_seam_is_inter(int32_t t) { return fer_seam_in(t, 0, 4) || t == 31; }  // P numbering
static inline bool fer_seam_mv16(const int32_t mv[4][2]) { return fer_seam_levels16(&mv[0][0], 8); }
// the quadrants that one partition of an inter type covers carry one vector
static inline bool fer_seam_mv_consistent(int32_t t, const int32_t mv[4][2])
{
    auto eq = [&](int a, int b) { return mv[a][0] == mv[b][0] && mv[a][1] == mv[b][1]; };
    if (t == 0 || t == 31) return eq(0, 1) && eq(0, 2) && eq(0, 3);
    if (t == 1) return eq(0, 1) && eq(2, 3);
    if (t == 2) return eq(0, 2) && eq(1, 3);
    return true;
}
static inline bool fer_seam_nb_ok(const ferhip_nb_mb &N, int32_t slice_type)
{
    if (!fer_seam_mb_type_ok(N.mb_type, slice_type) || !fer_seam_in(N.cbp_luma, 0, 15) || !fer_seam_in(N.cbp_chroma, 0, 2) || !fer_seam_mv16(N.mv))
        return false;
    for (int b = 0; b < 16; b++)
        if (!fer_seam_in(N.tc_luma[b], 0, 16) || !fer_seam_in(N.i4mode[b], 0, 8)) return false;
    for (int b = 0; b < 8; b++)
        if (!fer_seam_in(N.tc_chroma[b >> 2][b & 3], 0, 16)) return false;
    return true;
}

// getIntra4x4PredMode (F/intra.cpp:77-136) of a DECODE job, restated on the host only to tell whether the job is legal
static inline void fer_seam_i4_modes(const ferhip_intra_job &J, int mode[16])
{
    static const int8_t nbA[16] = {5, 0, 7, 2, 1, 4, 3, 6, 13, 8, 15, 10, 9, 12, 11, 14}, nbB[16] = {10, 11, 0, 1, 14, 15, 4, 5, 2, 3, 8, 9, 6, 7, 12, 13};
    const int nb = fer_seam_pos_nb(J.pos);
    for (int blk = 0; blk < 16; blk++) {
        const bool edgeA = blk == 0 || blk == 2 || blk == 8 || blk == 10, edgeB = blk == 0 || blk == 1 || blk == 4 || blk == 5;
        int mA = 2, mB = 2;
        if (!(edgeA && !(nb & 1)) && !(edgeB && !(nb & 2)) && !J.constrained_intra) {
            if (edgeA) {
                const ferhip_nb_mb &N = J.mb[J.pos - 1];
                mA = fer_seam_is_i4(N.mb_type, J.slice_type) ? N.i4mode[nbA[blk]] : 2;
            } else {
                mA = mode[nbA[blk]];
            }
            if (edgeB) {
                const ferhip_nb_mb &N = J.mb[J.pos - 3];
                mB = fer_seam_is_i4(N.mb_type, J.slice_type) ? N.i4mode[nbB[blk]] : 2;
            } else {
                mB = mode[nbB[blk]];
            }
        }
        const int pm = mA <= mB ? mA : mB, rem = J.rem_mode[blk];
        mode[blk] = J.prev_flag[blk] ? pm : (rem < pm ? rem : rem + 1);
    }
}
// a DECODE job whose prediction modes read only neighbours that pos provides (fields already in range)
static inline bool fer_seam_intra_legal(const ferhip_intra_job &J)
{
    static const int8_t bx[16] = {0, 4, 0, 4, 8, 12, 8, 12, 0, 4, 0, 4, 8, 12, 8, 12}, by[16] = {0, 0, 4, 4, 0, 0, 4, 4, 8, 8, 12, 12, 8, 8, 12, 12};
    const int nb = fer_seam_pos_nb(J.pos);
    const bool A = (nb & 1) != 0, B = (nb & 2) != 0;
    if ((J.chroma_mode == 1 && !A) || (J.chroma_mode == 2 && !B) || (J.chroma_mode == 3 && !(A && B))) return false;
    const int32_t t = J.mb[J.pos].mb_type;
    if (fer_seam_is_i16(t, J.slice_type)) {
        const int m = ((J.slice_type == 2 ? t : t - 5) - 1) & 3;  // vertical, horizontal, DC, plane
        return !((m == 0 && !B) || (m == 1 && !A) || (m == 3 && !(A && B)));
    }
    int mode[16];
    fer_seam_i4_modes(J, mode);
    for (int blk = 0; blk < 16; blk++) {
        const bool left = bx[blk] > 0 || A, top = by[blk] > 0 || B;  // the corner sample exists where both do (D exists with A and B)
        const int m = mode[blk];  // 0..8: a prediction is at most 8, and rem_mode 7 is below a prediction of 8
        if ((m == 0 || m == 3 || m == 7) && !top) return false;
        if ((m == 1 || m == 8) && !left) return false;
        if ((m == 4 || m == 5 || m == 6) && !(left && top)) return false;
    }
    return true;
}

static inline int fer_seam_check_intra_mbs(const ferhip_intra_job *jobs, const ferhip_intra_result *results, size_t n)
{
    if (!jobs || !results || n == 0 || n > FER_SEAM_JOBS_MAX) return FERHIP_E_ARG;
    for (size_t i = 0; i < n; i++) {
        const ferhip_intra_job &J = jobs[i];
        if (!fer_seam_in(J.op, FERHIP_INTRA_ENCODE, FERHIP_INTRA_DECODE) || !fer_seam_in(J.pos, 0, FERHIP_NB_MBS - 1) ||
            (J.slice_type != 0 && J.slice_type != 2) || !fer_seam_in(J.qp, 0, 51) || !fer_seam_in(J.chroma_qp_offset, -12, 12) ||
            !fer_seam_in(J.constrained_intra, 0, 1))
            return FERHIP_E_ARG;
        for (int m = 0; m < J.pos; m++)
            if (!fer_seam_nb_ok(J.mb[m], J.slice_type)) return FERHIP_E_ARG;
        const int32_t t = J.mb[J.pos].mb_type;
        if (J.op == FERHIP_INTRA_ENCODE) {  // I slices only; mb[pos].mb_type is the stale entry of the previous picture
            if (J.slice_type != 2 || !fer_seam_mb_type_ok(t, 2)) return FERHIP_E_ARG;
            continue;
        }
        if (!fer_seam_is_i4(t, J.slice_type) && !fer_seam_is_i16(t, J.slice_type)) return FERHIP_E_ARG;
        if (!fer_seam_in(J.chroma_mode, 0, 3)) return FERHIP_E_ARG;
        for (int b = 0; b < 16; b++)
            if (!fer_seam_in(J.prev_flag[b], 0, 1) || !fer_seam_in(J.rem_mode[b], 0, 7)) return FERHIP_E_ARG;
        if (!fer_seam_levels16(&J.lumaLevel[0][0], 256) || !fer_seam_levels16(J.dc16, 16) || !fer_seam_levels16(&J.ac16[0][0], 256) ||
            !fer_seam_levels16(&J.cdc[0][0], 8) || !fer_seam_levels16(&J.cac[0][0][0], 128))
            return FERHIP_E_ARG;
        if (!fer_seam_intra_legal(J)) return FERHIP_E_ARG;
    }
    return 0;
}

#define FER_SEAM_MVD_MAX 65536
static inline int fer_seam_check_mv_mbs(const ferhip_mv_job *jobs, const ferhip_mv_result *results, size_t n)
{
    if (!jobs || !results || n == 0 || n > FER_SEAM_JOBS_MAX) return FERHIP_E_ARG;
    for (size_t i = 0; i < n; i++) {
        const ferhip_mv_job &J = jobs[i];
        if (!fer_seam_in(J.op, FERHIP_MV_DERIVE, FERHIP_MV_PREDICT) || !fer_seam_in(J.pos, 0, FERHIP_NB_MBS - 1)) return FERHIP_E_ARG;
        const bool predict = J.op == FERHIP_MV_PREDICT;
        if (!(predict ? fer_seam_in(J.mb_type, 0, 4) : fer_seam_is_inter(J.mb_type))) return FERHIP_E_ARG;
        for (int k = 0; k < 4; k++)
            if (!fer_seam_in(J.sub_mb_type[k], 0, predict ? 0 : 3)) return FERHIP_E_ARG;
        for (int m = 0; m < J.pos; m++) {  // of a neighbour, mb_type and mv are read (P numbering)
            const ferhip_nb_mb &N = J.mb[m];
            if (!fer_seam_mb_type_ok(N.mb_type, 0) || !fer_seam_mv16(N.mv)) return FERHIP_E_ARG;
            if (fer_seam_is_inter(N.mb_type) ? !fer_seam_mv_consistent(N.mb_type, N.mv) : predict) return FERHIP_E_ARG;
        }
        if (predict) {
            if (!fer_seam_mv16(J.mv) || !fer_seam_mv_consistent(J.mb_type, J.mv)) return FERHIP_E_ARG;
        } else {
            for (int k = 0; k < 8; k++)
                if (!fer_seam_in(J.mvd[k >> 1][k & 1], -FER_SEAM_MVD_MAX, FER_SEAM_MVD_MAX)) return FERHIP_E_ARG;
        }
    }
    return 0;
}

// the legacy shims: CurrMbAddr against the macroblock count of the last AllocateMemory
static inline bool fer_seam_mb_addr_ok(int mb, int nmb) { return mb >= 0 && mb < nmb; }
