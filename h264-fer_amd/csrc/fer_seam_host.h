// fer_seam_host.h -- argument checks of the per-macroblock unit-parity surface (ferhip_mb_unit, ferhip_cavlc_blocks,
// ferhip_cavlc_parse_blocks, ferhip_residual_mbs, ferhip_mc_sub_mb_parts; fer_mbunit.hip).  The kernels behind these entry
// points index device tables and LDS with what the caller states (QP, block and macroblock indices, nC, maxNumCoeff, bit
// positions), so every call is checked here before its first HIP call.  Plain C++ without the HIP runtime, so that it
// can be compiled into a stand-alone host program and run under a sanitizer (tools/seam_host_check.cpp).
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

// the legacy shims: CurrMbAddr against the macroblock count of the last AllocateMemory
static inline bool fer_seam_mb_addr_ok(int mb, int nmb) { return mb >= 0 && mb < nmb; }
