// fer_mbunit.hip -- the per-macroblock unit-parity surface of SURVEY.md 8b: the reference's macroblock-level functions
// as batched device calls over the SAME device functions the encode / decode kernels are built from (fer_dev.h,
// fer_cavlc_dev.h, fer_decode_dev.h), so that a known-answer test pins them one function at a time:
//   quantizationTransform                       F/quantizationTransform.cpp:349-486   k_mb_unit, MBU_QT
//   transformDecoding4x4LumaResidual            F/inttransform.cpp:133-155            MBU_DEC4
//   transformDecodingIntra_16x16Luma            F/inttransform.cpp:157-213            MBU_DEC16
//   transformDecodingChroma                     F/inttransform.cpp:237-320            MBU_DECC
//   transformDecodingP_Skip                     F/inttransform.cpp:215-231            MBU_SKIP
//   residual_block_cavlc_write / _size          F/residual.cpp:374-666 / :673-957     k_cavlc_blocks
//   residual_block_cavlc                        F/residual.cpp:1069-1386              k_cavlc_parse_blocks
//   residual_write / residual(0, 15)            F/residual.cpp:300-372 / :959-1067    k_residual_write, k_residual_parse
//   MotionCompensateSubMBPart                   F/mocomp.cpp:152-195                  k_mc_parts
//   intraPredictionEncoding + coded_mb_size     F/intra.cpp:949, F/rbsp_encoding.cpp:330   k_intra_mb over a 3x2 neighbourhood
//   intraPrediction, getIntra4x4PredMode        F/intra.cpp:770, :77                  k_seam_i4_modes + k_dec_intra
//   DeriveMVs and the encoder's mvd             F/mode_pred.cpp:428                   k_seam_mv
//   forward / inverse residual, DC, scan        F/quantizationTransform.h, scaleTransform.h  k_block_kat
// Not a fast path: one wavefront (or thread) per job, records of plain int32.  Every entry point checks its arguments
// (fer_seam_host.h) before its first HIP call and keeps its device memory in DevBuf (fer_ctx.h); the hand-built FerDev of the
// neighbour-aware ones is packed by fer_seam_pack_host.h and held by SeamDev.  The legacy-name shims are in fer_legacy.hip.
#include "fer_cavlc_dev.h"
#include "fer_ctx.h"
#include "fer_decode_dev.h"
#include "fer_intra_dev.h"
#include "fer_mvpred.h"
#include "fer_seam_pack_host.h"

static_assert(SEAM_P_SKIP == FER_P_SKIP, "fer_seam_pack_host.h restates it");

// list[k] = c[zig-zag k] (transformScan, F/quantizationTransform.cpp:310-325); the Intra16x16AC / chroma AC form drops the DC
__device__ __forceinline__ void mbu_scan(const int c[16], int32_t *list, bool ac)
{
#pragma unroll
    for (int k = ac ? 1 : 0; k < 16; k++) list[ac ? k - 1 : k] = c[c_zz[k]];
    if (ac) list[15] = 0;
}
__device__ __forceinline__ void mbu_invscan(const int32_t *list, int c[16], bool ac, int dc)
{
#pragma unroll
    for (int k = 0; k < 16; k++) c[c_zz[k]] = ac ? (k == 0 ? dc : list[k - 1]) : list[k];
}

// One job = one macroblock.  lanes 0..15 own the luma 4x4 blocks (luma4x4BlkIdx order), lanes 16..23 the chroma blocks
// (Cb 0..3, Cr 0..3); the DC transforms run on the lane of block 0 of their plane.
__global__ __launch_bounds__(64) void k_mb_unit(const ferhip_mb_job *jobs, ferhip_mb_result *res, int n)
{
    __shared__ int dcl[16], dcc[2][4], dcdeq[2][4], dcy[16];
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= n) return;
    const ferhip_mb_job &J = jobs[j];
    ferhip_mb_result &R = res[j];
    const int op = J.op, qp = J.qp, qpc = J.qpc;
    const bool luma = lane < 16, chroma = lane >= 16 && lane < 24;
    const int blk = lane & 15, cpl = (lane - 16) >> 2, cblk = (lane - 16) & 3;
    const int x0 = luma ? c_bx[blk] : (cblk & 1) * 4, y0 = luma ? c_by[blk] : (cblk >> 1) * 4;
    int src[16], pred[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int yy = y0 + (i >> 2), xx = x0 + (i & 3);
        if (luma) {
            src[i] = J.srcY[yy * 16 + xx];
            pred[i] = J.predY[yy * 16 + xx];
        } else if (chroma) {
            src[i] = (cpl ? J.srcCr : J.srcCb)[yy * 8 + xx];
            pred[i] = (cpl ? J.predCr : J.predCb)[yy * 8 + xx];
        } else {
            src[i] = pred[i] = 0;
        }
    }
    auto store_rec = [&](const int r[16]) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int yy = y0 + (i >> 2), xx = x0 + (i & 3);
            const int v = clip255(pred[i] + r[i]);
            if (luma)
                R.recY[yy * 16 + xx] = v;
            else if (chroma)
                (cpl ? R.recCr : R.recCb)[yy * 8 + xx] = v;
        }
    };
    if (op == FERHIP_MBU_QT) {
        // ---- quantizationTransform(predL, predCb, predCr, reconstruct); cls = MbPartPredMode(mb_type, 0): 0 Intra_4x4
        // (luma is left to the prediction loop), 1 Intra_16x16, 2 inter
        const int cls = J.cls;
        int diff[16], d[16], c[16], r[16];
#pragma unroll
        for (int i = 0; i < 16; i++) diff[i] = src[i] - pred[i];
        fwd4x4(diff, d);
        if (luma && cls != 0) {
            quant4x4(d, c, qp, cls == 1);
            if (cls == 1) {
                dcl[(y0 >> 2) * 4 + (x0 >> 2)] = c[0];
                mbu_scan(c, R.ac16[blk], true);
            } else {
                mbu_scan(c, R.lumaLevel[blk], false);
                if (J.reconstruct) {
                    int cc[16];
                    mbu_invscan(R.lumaLevel[blk], cc, false, 0);
                    inv4x4(cc, r, qp, false);
                    store_rec(r);
                }
            }
        }
        if (chroma) {
            quant4x4(d, c, qpc, true);
            dcc[cpl][cblk] = c[0];
            mbu_scan(c, R.cac[cpl][cblk], true);
        }
        __syncthreads();
        if (lane == 0 && cls == 1) {
            int t[16], q[16];
#pragma unroll
            for (int i = 0; i < 16; i++) t[i] = dcl[i];
            fwd_dc_luma(t, q, qp);
            mbu_scan(q, R.dc16, false);
            if (J.reconstruct) {
                int cc[16], dq[16];
                mbu_invscan(R.dc16, cc, false, 0);
                inv_dc_luma(cc, dq, qp);
#pragma unroll
                for (int i = 0; i < 16; i++) dcy[i] = dq[i];
            }
        }
        if ((lane == 16 || lane == 20)) {
            int f[4], q[4], dq[4];
#pragma unroll
            for (int i = 0; i < 4; i++) f[i] = dcc[cpl][i];
            fwd_dc_chroma(f, q, qpc);
#pragma unroll
            for (int i = 0; i < 4; i++) R.cdc[cpl][i] = q[i];
            inv_dc_chroma(q, dq, qpc);
#pragma unroll
            for (int i = 0; i < 4; i++) dcdeq[cpl][i] = dq[i];
        }
        __syncthreads();
        if (J.reconstruct) {
            if (luma && cls == 1) {
                int cc[16];
                mbu_invscan(R.ac16[blk], cc, true, dcy[(y0 >> 2) * 4 + (x0 >> 2)]);
                inv4x4(cc, r, qp, true);
                store_rec(r);
            }
            if (chroma) {
                int cc[16];
                mbu_invscan(R.cac[cpl][cblk], cc, true, dcdeq[cpl][cblk]);
                inv4x4(cc, r, qpc, true);
                store_rec(r);
            }
        }
        return;
    }
    // ---- the decode-side drivers: levels in, samples out
    int r[16], cc[16];
    if (op == FERHIP_MBU_DEC4) {  // transformDecoding4x4LumaResidual(LumaLevel, predL, luma4x4BlkIdx = J.blk, QPy)
        if (luma && blk == J.blk) {
            mbu_invscan(J.lumaLevel[blk], cc, false, 0);
            inv4x4(cc, r, qp, false);
            store_rec(r);
        }
    } else if (op == FERHIP_MBU_DEC16) {  // transformDecodingIntra_16x16Luma(Intra16x16DCLevel, Intra16x16ACLevel, predL, QPy)
        if (lane == 0) {
            int dq[16];
            mbu_invscan(J.dc16, cc, false, 0);
            inv_dc_luma(cc, dq, qp);
#pragma unroll
            for (int i = 0; i < 16; i++) dcy[i] = dq[i];
        }
        __syncthreads();
        if (luma) {
            mbu_invscan(J.ac16[blk], cc, true, dcy[(y0 >> 2) * 4 + (x0 >> 2)]);
            inv4x4(cc, r, qp, true);
            store_rec(r);
        }
    } else if (op == FERHIP_MBU_DECC) {  // transformDecodingChroma(ChromaDCLevel, ChromaACLevel, predC, QPy, Cb) for both planes
        if (lane == 16 || lane == 20) {
            int q[4], dq[4];
#pragma unroll
            for (int i = 0; i < 4; i++) q[i] = J.cdc[cpl][i];
            inv_dc_chroma(q, dq, qpc);
#pragma unroll
            for (int i = 0; i < 4; i++) dcdeq[cpl][i] = dq[i];
        }
        __syncthreads();
        if (chroma) {
            mbu_invscan(J.cac[cpl][cblk], cc, true, dcdeq[cpl][cblk]);
            inv4x4(cc, r, qpc, true);
            store_rec(r);
        }
    } else if (op == FERHIP_MBU_SKIP) {  // transformDecodingP_Skip: all levels zero
#pragma unroll
        for (int i = 0; i < 16; i++) cc[i] = 0;
        inv4x4(cc, r, luma ? qp : qpc, !luma);
        if (luma || chroma) store_rec(r);
    }
}

extern "C" int ferhip_mb_unit(const ferhip_mb_job *jobs, ferhip_mb_result *results, size_t n)
{
    if (fer_seam_check_mb_unit(jobs, results, n)) return FERHIP_E_ARG;
    DevBuf<ferhip_mb_job> dj;
    DevBuf<ferhip_mb_result> dr;
    if (dj.reserve(n) || dr.reserve(n)) return FERHIP_E_HIP;
    CK(hipMemcpy(dj, jobs, n * sizeof *jobs, hipMemcpyHostToDevice));
    CK(hipMemset(dr, 0, n * sizeof *results));
    hipLaunchKernelGGL(k_mb_unit, dim3((unsigned)n), dim3(64), 0, 0, dj.p, dr.p, (int)n);
    CK(hipGetLastError());
    CK(hipMemcpy(results, dr, n * sizeof *results, hipMemcpyDeviceToHost));
    return 0;
}

// ---- residual_block_cavlc_write / _size for n blocks: the device block coder of the entropy pass and of coded_mb_size
__global__ __launch_bounds__(64) void k_cavlc_blocks(const int32_t *coef, const int32_t *nC, const int32_t *maxn, int n, uint32_t *bits,
                                                     uint32_t *nbits, int32_t *tc, uint32_t *nbits_size)
{
    __shared__ int16_t stage[16 * 64];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    int16_t *st = stage + threadIdx.x;
    const int m = maxn[i];
    unsigned nz = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int v = k < m ? coef[(size_t)i * 16 + k] : 0;
        st[k * 64] = (int16_t)v;
        nz |= (v != 0 ? 1u : 0u) << k;
    }
    BitW w;
    bw_init<true>(w, bits + (size_t)i * 16, 16, 0);
    cavlc_block_core<true>(w, nz, m, nC[i], st, 64);
    bw_flush<true>(w);
    nbits[i] = w.bits;
    tc[i] = __popc(nz);
    BitW ws;  // the counting form (residual_block_cavlc_size) must agree with the writer
    bw_init<false>(ws, nullptr, 0, 0);
    cavlc_block_core<false>(ws, nz, m, nC[i], st, 64);
    nbits_size[i] = ws.bits;
}

extern "C" int ferhip_cavlc_blocks(const int32_t *coef, const int32_t *nC, const int32_t *max_num_coeff, size_t n, uint8_t *bits,
                                   uint32_t *nbits, int32_t *total_coeff)
{
    if (fer_seam_check_cavlc_blocks(coef, nC, max_num_coeff, n, bits, nbits, total_coeff)) return FERHIP_E_ARG;
    DevBuf<int32_t> dc, dn, dm, dt;
    DevBuf<uint32_t> db, dl, ds;
    std::vector<uint32_t> sz(n);
    if (dc.reserve(n * 16) || dn.reserve(n) || dm.reserve(n) || dt.reserve(n) || db.reserve(n * 16) || dl.reserve(n) || ds.reserve(n))
        return FERHIP_E_HIP;
    CK(hipMemcpy(dc, coef, n * 64, hipMemcpyHostToDevice));
    CK(hipMemcpy(dn, nC, n * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dm, max_num_coeff, n * 4, hipMemcpyHostToDevice));
    CK(hipMemset(db, 0, n * 64));
    hipLaunchKernelGGL(k_cavlc_blocks, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, dc.p, dn.p, dm.p, (int)n, db.p, dl.p, dt.p, ds.p);
    CK(hipGetLastError());
    CK(hipMemcpy(bits, db, n * 64, hipMemcpyDeviceToHost));
    CK(hipMemcpy(nbits, dl, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(total_coeff, dt, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(sz.data(), ds, n * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)
        if (sz[i] != nbits[i]) {
            fprintf(stderr, "ferhip_cavlc_blocks: block %zu: the counting form gives %u bits, the writer %u\n", i, sz[i], nbits[i]);
            return FERHIP_E_DEVICE;
        }
    return 0;
}

// ---- the parse direction.  dec_block is wave-uniform (fer_decode_dev.h), so the unit of work is a wavefront; the SEAM_PW
// wavefronts of a workgroup share the decode tables in LDS, filled once, and the grid is capped so that the fill is
// amortised over the blocks / macroblocks a wavefront walks.
#define SEAM_PW 4
#define SEAM_GRID_MAX 64  // 256 wavefronts
__device__ __forceinline__ void mbu_wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void mbu_fill_luts(DecLutsLds &lut, const DecLuts *__restrict__ luts)
{
    const uint32_t *src = (const uint32_t *)&luts->ct1[0][0];
    uint32_t *dst = (uint32_t *)&lut;
    for (int i = threadIdx.x; i < (int)(sizeof(DecLutsLds) / 4); i += 64 * SEAM_PW) dst[i] = src[i];
    __syncthreads();
}

// residual_block_cavlc for n blocks of one stream (4-byte aligned, padded by 16 bytes): block i starts at bit_pos[i]
__global__ __launch_bounds__(64 * SEAM_PW) void k_cavlc_parse_blocks(const uint8_t *bits, unsigned nbytes, const uint64_t *bit_pos,
                                                                    const int32_t *nC, const int32_t *maxn, int n, int32_t *coef, int32_t *tc,
                                                                    uint32_t *used, const DecLuts *__restrict__ luts)
{
    __shared__ uint32_t ring_w[SEAM_PW][128];
    __shared__ __attribute__((aligned(4))) int16_t cf_w[SEAM_PW][16];
    __shared__ DecLutsLds lut;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int16_t *cf = cf_w[wv];
    mbu_fill_luts(lut, luts);
    for (int i = blockIdx.x * SEAM_PW + wv; i < n; i += gridDim.x * SEAM_PW) {
        const unsigned pos0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)bit_pos[i]);  // < 8 * nbytes <= 2^31
        const int m = __builtin_amdgcn_readfirstlane(maxn[i]), c = __builtin_amdgcn_readfirstlane(nC[i]);
        if (lane < 16) cf[lane] = 0;
        mbu_wsync();
        DecBits b;
        db_open(b, bits, nbytes, pos0, ring_w[wv]);
        int t = dec_block(b, &lut, cf, m, c);
        mbu_wsync();
        if (t >= 0 && b.pos > nbytes * 8u) t = -1;  // the reader zero-extends the stream: a block that ran out of it
        if (lane < 16) coef[(size_t)i * 16 + lane] = t < 0 ? 0 : cf[lane];
        if (lane == 0) {
            tc[i] = t;
            used[i] = b.pos - pos0;
        }
        mbu_wsync();  // cf and the ring are the next block's
    }
}

extern "C" int ferhip_cavlc_parse_blocks(const uint8_t *bits, size_t nbytes, const uint64_t *bit_pos, const int32_t *nC,
                                         const int32_t *max_num_coeff, size_t n, int32_t *coef, int32_t *total_coeff, uint32_t *bits_used)
{
    if (fer_seam_check_parse_blocks(bits, nbytes, bit_pos, nC, max_num_coeff, n, coef, total_coeff, bits_used)) return FERHIP_E_ARG;
    DevBuf<uint8_t> dbits;
    DevBuf<uint64_t> dpos;
    DevBuf<int32_t> dn, dm, dc, dt;
    DevBuf<uint32_t> du;
    const size_t padded = ((nbytes + 3) & ~(size_t)3) + 16;  // what DecBits asks for: the buffer is aligned, the tail is zero
    if (dbits.reserve(padded) || dpos.reserve(n) || dn.reserve(n) || dm.reserve(n) || dc.reserve(n * 16) || dt.reserve(n) || du.reserve(n))
        return FERHIP_E_HIP;
    const DecLuts *luts = dec_luts(0);
    if (!luts) return FERHIP_E_HIP;
    CK(hipMemset(dbits, 0, padded));
    CK(hipMemcpy(dbits, bits, nbytes, hipMemcpyHostToDevice));
    CK(hipMemcpy(dpos, bit_pos, n * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dn, nC, n * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dm, max_num_coeff, n * 4, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)std::min<size_t>((n + SEAM_PW - 1) / SEAM_PW, SEAM_GRID_MAX);
    hipLaunchKernelGGL(k_cavlc_parse_blocks, dim3(grid), dim3(64 * SEAM_PW), 0, 0, dbits.p, (unsigned)nbytes, dpos.p, dn.p, dm.p, (int)n, dc.p,
                       dt.p, du.p, luts);
    CK(hipGetLastError());
    CK(hipMemcpy(coef, dc, n * 64, hipMemcpyDeviceToHost));
    CK(hipMemcpy(total_coeff, dt, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(bits_used, du, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- residual_write() / residual(0, 15) of one macroblock with nC derived from its neighbours.
// WRITE: the encoder's block order and cavlc_nC (cavlc_residual_mb of fer_cavlc_dev.h, the body of k_cavlc), one thread
// per job as in k_cavlc.  cavlc_nC reads the FerDev side information, so job j is stream j of a context of 2x2-macroblock
// pictures (mbw = 2) and its macroblock sits at address cur[j], where exactly the neighbours it states exist.
__global__ __launch_bounds__(64) void k_residual_write(FerDev d, const ferhip_res_job *jobs, const uint8_t *cur, int n, ferhip_res_result *res)
{
    __shared__ int16_t stage[16 * 64];
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n || jobs[s].op != FERHIP_RES_WRITE) return;
    const int mb = cur[s];
    const size_t mbi = (size_t)s * d.nmb + mb;
    const int16_t *lv = d.levels + mbi * FER_LEVELS;
    ferhip_res_result &R = res[s];
    BitW w;
    bw_init<true>(w, (uint32_t *)R.bits, FERHIP_RES_BITS_MAX / 4, 0);  // (zeroed by the host: the writer merges words with atomicOr)
    cavlc_residual_mb<true, 64>(w, d, s, mb, lv, d.cbp[mbi * 2], d.cbp[mbi * 2 + 1], jobs[s].cls == 1, stage + threadIdx.x);
    bw_flush<true>(w);
    R.nbits = w.bits > FERHIP_RES_BITS_MAX * 8u ? -1 : (int)w.bits;  // (words behind the buffer are dropped by the writer)
    for (int k = 0; k < 16; k++) R.tc_luma[k] = d.tc[mbi * 24 + k];
    for (int k = 0; k < 8; k++) R.tc_chroma[k >> 2][k & 3] = d.tc[mbi * 24 + 16 + k];
}

// PARSE: the decoder's dec_block with dec_nC over a two-entry DecNb row (the residual part of k_dec_parse's macroblock
// loop), one wavefront per job.  dec_nC takes entry x - 1 of the row for A and entry x for B: with A the macroblock is at
// x = 1, without at x = 0, and y says whether B exists.
__global__ __launch_bounds__(64 * SEAM_PW) void k_residual_parse(const ferhip_res_job *jobs, ferhip_res_result *res, int n,
                                                                const DecLuts *__restrict__ luts)
{
    __shared__ uint8_t tcur_w[SEAM_PW][24];
    __shared__ uint32_t ring_w[SEAM_PW][128];
    __shared__ int16_t cac_w[SEAM_PW][2][4][16];
    __shared__ __attribute__((aligned(16))) int16_t mblv_w[SEAM_PW][FER_LEVELS];
    __shared__ DecNb row_w[SEAM_PW][2];
    __shared__ DecLutsLds lut;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint8_t *tcur = tcur_w[wv];
    int16_t(*cac)[4][16] = cac_w[wv];
    int16_t *lv = mblv_w[wv];
    DecNb *row = row_w[wv];
    mbu_fill_luts(lut, luts);
    for (int j = blockIdx.x * SEAM_PW + wv; j < n; j += gridDim.x * SEAM_PW) {
        const ferhip_res_job &J = jobs[j];
        if (__builtin_amdgcn_readfirstlane(J.op) != FERHIP_RES_PARSE) continue;
        ferhip_res_result &R = res[j];
        const bool i16 = __builtin_amdgcn_readfirstlane(J.cls) == 1;
        const int cbpL = __builtin_amdgcn_readfirstlane(J.cbp_luma), cbpC = __builtin_amdgcn_readfirstlane(J.cbp_chroma);
        const int avail = __builtin_amdgcn_readfirstlane(J.avail);
        const unsigned pos0 = (unsigned)__builtin_amdgcn_readfirstlane((int)J.bit_pos), nbytes = (unsigned)__builtin_amdgcn_readfirstlane((int)J.nbytes);
        const int mbx = avail & 1, mby = (avail >> 1) & 1;
        for (int k = 0; k < 2; k++) {  // A into entry 0, B into entry mbx
            if (!(avail & (1 << k))) continue;
            const ferhip_res_nb &N = J.nb[k];
            DecNb &e = row[k ? mbx : 0];
            if (lane < 24) e.tc[lane] = (uint8_t)(lane < 16 ? N.tc_luma[lane] : N.tc_chroma[(lane - 16) >> 2][lane & 3]);
            if (lane == 0) {
                e.cbpL = (uint8_t)N.cbp_luma;
                e.cbpC = (uint8_t)N.cbp_chroma;
                e.skip = N.p_skip ? 1 : 0;
                e.i4 = 0;
            }
        }
        for (int i = lane; i < FER_LEVELS / 2; i += 64) ((uint32_t *)lv)[i] = 0;
        for (int i = lane; i < 2 * 4 * 16; i += 64) (&cac[0][0][0])[i] = 0;
        if (lane < 24) tcur[lane] = 0;
        mbu_wsync();
        DecBits b;
        db_open(b, J.bits, nbytes, pos0, ring_w[wv]);
        bool bad = false;
        // residual(0,15), F/residual.cpp:959-1067, as in k_dec_parse; the blocks the CBP leaves out stay zero
        if (i16) {
            int t = dec_block(b, &lut, lv + FER_LV_DC16, 16, dec_nC(row, mbx, mby, true, 0, 0, tcur, cbpL, cbpC));
            bad |= t < 0;
            if (t >= 0) tcur[0] = (uint8_t)t;
            mbu_wsync();
        }
        for (int i8 = 0; i8 < 4 && !bad; i8++)
            if (cbpL & (1 << i8)) {
                for (int i4x = 0; i4x < 4 && !bad; i4x++) {
                    int blk = i8 * 4 + i4x;
                    int t = dec_block(b, &lut, lv + blk * 16, i16 ? 15 : 16, dec_nC(row, mbx, mby, true, blk, 0, tcur, cbpL, cbpC));
                    bad |= t < 0;
                    if (t >= 0) tcur[blk] = (uint8_t)t;
                    mbu_wsync();
                }
            } else {  // F/residual.cpp:1051,1059: also entry 0 of an Intra16x16 macroblock, where the DC block's count stood
                if (lane < 4) tcur[i8 * 4 + lane] = 0;
                mbu_wsync();
            }
        for (int pl = 0; pl < 2 && !bad; pl++)
            if (cbpC & 3) bad |= dec_block(b, &lut, lv + FER_LV_CDC + pl * 4, 4, -1) < 0;
        for (int pl = 0; pl < 2 && !bad; pl++)
            for (int cb = 0; cb < 4 && !bad; cb++)
                if (cbpC & 2) {
                    int t = dec_block(b, &lut, &cac[pl][cb][0], 15, dec_nC(row, mbx, mby, false, cb, pl, tcur, cbpL, cbpC));
                    bad |= t < 0;
                    if (t >= 0) tcur[16 + pl * 4 + cb] = (uint8_t)t;
                    mbu_wsync();
                }
        mbu_wsync();
        bad |= b.pos > nbytes * 8u;  // ran out of the stream (the reader zero-extends it)
        if (lane == 0) R.nbits = bad ? -1 : (int)(b.pos - pos0);
        if (!bad) {  // (the results start out zero)
            if (lane < 16) R.tc_luma[lane] = tcur[lane];
            if (lane >= 16 && lane < 24) R.tc_chroma[(lane - 16) >> 2][lane & 3] = tcur[lane];
            int32_t *ll = i16 ? &R.ac16[0][0] : &R.lumaLevel[0][0];
            for (int i = lane; i < 256; i += 64) ll[i] = lv[i];
            if (i16 && lane < 16) R.dc16[lane] = lv[FER_LV_DC16 + lane];
            if (lane < 8) R.cdc[lane >> 2][lane & 3] = lv[FER_LV_CDC + lane];
            for (int i = lane; i < 2 * 4 * 16; i += 64) (&R.cac[0][0][0])[i] = (&cac[0][0][0])[i];
        }
        mbu_wsync();  // the LDS of this wavefront is the next job's
    }
}

// The hand-built context on the device: one buffer per array of SEAM_ARRAYS (fer_seam_pack_host.h) in use, and the FerDev
// over them.  Sizes, copies and the offsets of a stream range all come from that table.
struct __attribute__((visibility("hidden"))) SeamDev {
#define X(n, T, per, e) DevBuf<T> n;
    SEAM_ARRAYS(X)
#undef X
    int reserve(size_t S, int nmb, unsigned use)
    {
        return seam_each(*this, [&](int a, auto &b) { return (use >> a & 1) ? b.reserve(S * seam_stride(a, nmb)) : 0; });
    }
    int copy(SeamHost &h, unsigned which, bool up)  // the arrays in `which`: host to device, or back
    {
        return seam_each(*this, h, [&](int a, auto &b, auto &v) {
            if ((which >> a & 1) && up) CK(hipMemcpy(b, v.data(), v.size() * sizeof v[0], hipMemcpyHostToDevice));
            if ((which >> a & 1) && !up) CK(hipMemcpy(v.data(), b, v.size() * sizeof v[0], hipMemcpyDeviceToHost));
            return 0;
        });
    }
    // the context of S streams of W x H pictures (mbw x mbh = nmb macroblocks) that begins at stream s0 of the buffers
    FerDev dev(int W, int H, int mbw, int mbh, int nmb, size_t S, size_t s0 = 0) const
    {
        FerDev d = {};
        d.W = W, d.H = H, d.Wc = W / 2, d.Hc = H / 2;
        d.mbw = mbw, d.mbh = mbh, d.nmb = nmb, d.S = (int)S;
        d.ysz = (size_t)W * H, d.csz = d.ysz / 4;
        seam_each(*this, d, [&](int a, auto &b, auto *&q) { return b.p ? (q = b.p + s0 * seam_stride(a, nmb), 0) : 0; });
        return d;
    }
};

extern "C" int ferhip_residual_mbs(const ferhip_res_job *jobs, ferhip_res_result *results, size_t n)
{
    if (fer_seam_check_residual_mbs(jobs, results, n)) return FERHIP_E_ARG;
    bool any_write = false, any_parse = false;
    for (size_t j = 0; j < n; j++) (jobs[j].op == FERHIP_RES_WRITE ? any_write : any_parse) = true;
    // the FerDev side information cavlc_nC and the block loop read: mb_type, cbp, tc, levels of [n streams][4 macroblocks]
    const unsigned use = any_write ? SEAM_RES_USE : 0;
    SeamHost h(n, SEAM_RES_NMB, use);
    std::vector<uint8_t> cur(n, 0);
    seam_pack_res_write(h, cur.data(), jobs);
    SeamDev sd;
    DevBuf<uint8_t> dj, dr, dcur;
    const size_t jbytes = n * sizeof(ferhip_res_job) + 16;  // DecBits reads a padded stream: behind the last job's bits
    if (dj.reserve(jbytes) || dr.reserve(n * sizeof(ferhip_res_result))) return FERHIP_E_HIP;
    if (any_write && (sd.reserve(n, SEAM_RES_NMB, use) || dcur.reserve(n))) return FERHIP_E_HIP;
    const DecLuts *luts = any_parse ? dec_luts(0) : nullptr;
    if (any_parse && !luts) return FERHIP_E_HIP;
    CK(hipMemset(dj, 0, jbytes));
    CK(hipMemcpy(dj, jobs, n * sizeof(ferhip_res_job), hipMemcpyHostToDevice));
    CK(hipMemset(dr, 0, n * sizeof(ferhip_res_result)));
    const ferhip_res_job *djobs = (const ferhip_res_job *)dj.p;
    ferhip_res_result *dres = (ferhip_res_result *)dr.p;
    if (any_write) {
        if (sd.copy(h, use, true)) return FERHIP_E_HIP;
        CK(hipMemcpy(dcur, cur.data(), n, hipMemcpyHostToDevice));
        const FerDev d = sd.dev(0, 0, SEAM_RES_MBW, SEAM_RES_NMB / SEAM_RES_MBW, SEAM_RES_NMB, n);
        hipLaunchKernelGGL(k_residual_write, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, d, djobs, dcur.p, (int)n, dres);
        CK(hipGetLastError());
    }
    if (any_parse) {
        const unsigned grid = (unsigned)std::min<size_t>((n + SEAM_PW - 1) / SEAM_PW, SEAM_GRID_MAX);
        hipLaunchKernelGGL(k_residual_parse, dim3(grid), dim3(64 * SEAM_PW), 0, 0, djobs, dres, (int)n, luts);
        CK(hipGetLastError());
    }
    CK(hipMemcpy(results, dr, n * sizeof(ferhip_res_result), hipMemcpyDeviceToHost));
    // TotalCoeff_luma_array[CurrMbAddr][0] of an Intra16x16 macroblock without AC blocks is what its DC block left there
    // (F/residual.cpp:530-541); no neighbour can read it (the CBP gates it), the encoder's side information keeps the AC count
    for (size_t j = 0; j < n; j++)
        if (jobs[j].op == FERHIP_RES_WRITE && jobs[j].cls == 1 && !(jobs[j].cbp_luma & 1)) results[j].tc_luma[0] = seam_count_nz(jobs[j].dc16, 16);
    return 0;
}

// ---- the neighbourhood seam: intraPredictionEncoding / intraPrediction and DeriveMVs of one macroblock among its
// neighbours.  Job j is stream j of a context of 3x2-macroblock pictures (FERHIP_NB_W x FERHIP_NB_H) over a hand-built
// FerDev, its macroblock sits at address pos, and the picture kernels run on it as they stand: k_intra_mb (ENCODE) and
// k_dec_intra (DECODE) are launched for the one anti-diagonal of pos, over the streams of the jobs with that pos.  A
// diagonal launch also visits the other macroblock of the diagonal (2 and 3 share one); nothing it reads or writes there
// is a neighbour of the job's macroblock, and in DECODE its type is set to P_Skip so that k_dec_intra passes it by.

// getIntra4x4PredMode of the DECODE jobs: dec_i4_modes (fer_decode_dev.h) fed from the FerDev side information the way
// k_dec_parse feeds it from its neighbour rows.  One thread per stream (the function is scalar code).
__global__ __launch_bounds__(64) void k_seam_i4_modes(FerDev d, const uint8_t *pos)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= d.S) return;
    const int p = pos[s], mbx = p % d.mbw, mby = p / d.mbw;
    const size_t mbi = (size_t)s * d.nmb + p;
    const int i4t = d.hdr[s * 4 + 3] == 2 ? 0 : 5;
    if (d.mb_type[mbi] != i4t) return;
    unsigned long long i4flags = 0, left_modes = 0;
    unsigned above_modes = 0;
    for (int blk = 0; blk < 16; blk++) i4flags |= (unsigned long long)(d.i4flag[mbi * 16 + blk] & 15) << (4 * blk);
    const bool left_i4 = mbx > 0 && d.mb_type[mbi - 1] == i4t, above_i4 = mby > 0 && d.mb_type[mbi - d.mbw] == i4t;
    if (left_i4)
        for (int blk = 0; blk < 16; blk++) left_modes |= (unsigned long long)(d.i4mode[(mbi - 1) * 16 + blk] & 15) << (4 * blk);
    if (above_i4) {
        const uint8_t *m = d.i4mode + (mbi - d.mbw) * 16;
        above_modes = (unsigned)m[10] | ((unsigned)m[11] << 4) | ((unsigned)m[14] << 8) | ((unsigned)m[15] << 12);
    }
    const unsigned long long cm = dec_i4_modes(i4flags, mbx, mby, d.hdr[s * 4 + 1] != 0, left_i4, left_modes, above_i4, above_modes);
    for (int blk = 0; blk < 16; blk++) d.i4mode[mbi * 16 + blk] = (uint8_t)((cm >> (4 * blk)) & 15);
}

// predL / predCb / predCr of the macroblock at pos, by the decode-side predictors (fetch4 + pred4x4, pred16_px,
// pred_chroma_px of fer_intra_dev.h) on the reconstructed picture: every sample an Intra4x4 block predicts from belongs
// to a neighbouring macroblock or to a block in front of it, so the sixteen blocks are evaluated side by side.
// One wavefront per stream; pred[s] = 256 luma, 64 Cb, 64 Cr.
__global__ __launch_bounds__(64) void k_seam_intra_pred(FerDev d, const uint8_t *pos, int32_t *pred)
{
    __shared__ IntraLds L;
    const int lane = threadIdx.x, s = blockIdx.x;
    const int p = pos[s], mbx = p % d.mbw, mby = p / d.mbw;
    const size_t mbi = (size_t)s * d.nmb + p;
    const int W = d.W, Wc = d.Wc, xp = mbx << 4, yp = mby << 4;
    const uint8_t *Y = d.curY + (size_t)s * d.ysz;
    const uint8_t *Cp[2] = {d.curCb + (size_t)s * d.csz, d.curCr + (size_t)s * d.csz};
    const bool availL = mbx > 0, availT = mby > 0, lastcol = mbx == d.mbw - 1;
    for (int i = lane; i < 17 * 21; i += 64) {  // the window of k_intra_mb: the macroblock, its left column, the row above with four more
        const int r = i / 21, c = i % 21;
        const int gx = xp + c - 1, gy = yp + r - 1;
        int v = -1;
        if (gx >= 0 && gy >= 0 && gx < W && (r == 0 || c <= 16)) v = Y[(size_t)gy * W + gx];
        L.fr[r][c] = (int16_t)v;
    }
    for (int i = lane; i < 2 * 9 * 9; i += 64) {
        const int pl = i / 81, r = (i % 81) / 9, c = i % 9;
        const int gx = xp / 2 + c - 1, gy = yp / 2 + r - 1;
        L.cfr[pl][r][c] = (int16_t)((gx >= 0 && gy >= 0) ? Cp[pl][(size_t)gy * Wc + gx] : -1);
    }
    __syncthreads();
    int32_t *o = pred + (size_t)s * 384;
    const int stype = (int)d.hdr[s * 4 + 3], t = d.mb_type[mbi], chroma_mode = d.chroma_mode[mbi];
    {
        const int cx = lane & 7, cy = lane >> 3;
        for (int pl = 0; pl < 2; pl++) o[256 + pl * 64 + lane] = pred_chroma_px(L.cfr[pl], chroma_mode, cx, cy, availL, availT);
    }
    if (t == (stype == 2 ? 0 : 5)) {
        if (lane < 16) {
            int q[13], b[16];
            fetch4(L, lane, lastcol, q);
            pred4x4(d.i4mode[mbi * 16 + lane], q, b);
            for (int i = 0; i < 16; i++) o[(c_by[lane] + (i >> 2)) * 16 + c_bx[lane] + (i & 3)] = b[i];
        }
    } else {
        P16 q16;
        pred16_params(L, availL, availT, q16);
        const int mode = ((stype == 2 ? t : t - 5) - 1) & 3;
        for (int i = lane; i < 256; i += 64) o[i] = pred16_px(L, q16, mode, i & 15, i >> 4);
    }
}

extern "C" int ferhip_chroma_qp(int qpy);  // fer_api.hip: qPiToQPc for chroma_qp_index_offset 0, the encoder's

extern "C" int ferhip_intra_mbs(const ferhip_intra_job *jobs, ferhip_intra_result *results, size_t n)
{
    if (fer_seam_check_intra_mbs(jobs, results, n)) return FERHIP_E_ARG;
    const SeamOrder o = seam_intra_order(jobs, n);  // stream s = job o.order[s]
    SeamHost h(n, FERHIP_NB_MBS, SEAM_INTRA_USE);
    std::vector<uint8_t> pos(n);
    std::vector<int32_t> pred(n * 384);
    seam_pack_intra(h, pos.data(), jobs, o.order.data(), ferhip_chroma_qp);
    SeamDev sd;
    DevBuf<uint8_t> dpos;
    DevBuf<int32_t> dpred;
    if (sd.reserve(n, FERHIP_NB_MBS, SEAM_INTRA_USE) || dpos.reserve(n) || dpred.reserve(pred.size())) return FERHIP_E_HIP;
    if (sd.copy(h, SEAM_INTRA_USE, true)) return FERHIP_E_HIP;
    CK(hipMemcpy(dpos, pos.data(), n, hipMemcpyHostToDevice));
    for (size_t r = 0; r + 1 < o.run.size(); r++) {  // one launch per (op, pos)
        const size_t s0 = o.run[r], cnt = o.run[r + 1] - s0;
        const ferhip_intra_job &J = jobs[o.order[s0]];
        const FerDev g = sd.dev(FERHIP_NB_W, FERHIP_NB_H, SEAM_MBW, FERHIP_NB_H / 16, FERHIP_NB_MBS, cnt, s0);
        const int diag = J.pos % SEAM_MBW + 2 * (J.pos / SEAM_MBW);
        if (J.op == FERHIP_INTRA_ENCODE) {
            fer_launch_intra_diag(g, diag, 0);
        } else {
            hipLaunchKernelGGL(k_seam_i4_modes, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, 0, g, dpos.p + s0);
            fer_launch_decode_intra_diag(g, diag, 0);
        }
        CK(hipGetLastError());
    }
    const FerDev d = sd.dev(FERHIP_NB_W, FERHIP_NB_H, SEAM_MBW, FERHIP_NB_H / 16, FERHIP_NB_MBS, n);
    hipLaunchKernelGGL(k_seam_intra_pred, dim3((unsigned)n), dim3(64), 0, 0, d, dpos.p, dpred.p);
    CK(hipGetLastError());
    if (sd.copy(h, SEAM_INTRA_DOWN, false)) return FERHIP_E_HIP;
    CK(hipMemcpy(pred.data(), dpred, pred.size() * sizeof pred[0], hipMemcpyDeviceToHost));
    seam_unpack_intra(results, h, pred.data(), jobs, o.order.data());
    return 0;
}

// DeriveMVs and its inverse.  One wavefront per job: the job's neighbours go into the vector field and the type array of
// stream j; DERIVE is dec_derive_mvs (fer_mvpred.h), scalar code run by lane 0 as k_dec_parse runs it; PREDICT is the
// mvd step of k_p_resid -- lane i < 4 derives partition i through predict_luma_tbl from the vectors held one per lane.
__global__ __launch_bounds__(64) void k_seam_mv(FerDev d, const ferhip_mv_job *jobs, ferhip_mv_result *res)
{
    const int j = blockIdx.x, lane = threadIdx.x;
    const ferhip_mv_job &J = jobs[j];
    ferhip_mv_result &R = res[j];
    const int p = J.pos, type = J.mb_type;
    short *mvs = d.mv + (size_t)j * d.nmb * 8;
    int *mbt = d.mb_type + (size_t)j * d.nmb;
    if (lane < d.nmb * 8) {
        const int m = lane >> 3;
        short v = 0;
        if (m < p) v = (short)J.mb[m].mv[(lane & 7) >> 1][lane & 1];
        if (m == p && J.op == FERHIP_MV_PREDICT) v = (short)J.mv[(lane & 7) >> 1][lane & 1];
        mvs[lane] = v;
    }
    if (lane < d.nmb) mbt[lane] = lane < p ? J.mb[lane].mb_type : 0;
    __syncthreads();
    if (J.op == FERHIP_MV_DERIVE) {
        if (lane == 0) {
            int mvd[4][2], sub[4];
            for (int i = 0; i < 4; i++) {
                mvd[i][0] = J.mvd[i][0];
                mvd[i][1] = J.mvd[i][1];
                sub[i] = J.sub_mb_type[i];
            }
            R.fits = dec_derive_mvs(d, mvs, mbt, p, type, mvd, sub) ? 1 : 0;
            for (int k = 0; k < 8; k++) R.mv[k >> 1][k & 1] = mvs[p * 8 + k];
        }
        return;
    }
    const int mbx = p % d.mbw, mby = p / d.mbw;
    int tbl;  // as in k_p_resid: the vectors of this macroblock and of its left / above / above-right / above-left neighbours
    {
        const int which = min(lane >> 2, 4), q = lane & 3;
        const int off = which == 0 ? 0 : (which == 1 ? -1 : (which == 2 ? -d.mbw : (which == 3 ? 1 - d.mbw : -1 - d.mbw)));
        tbl = ((const int *)mvs)[(size_t)iclamp(p + off, 0, d.nmb - 1) * 4 + q];
    }
    const int np = type == FER_P_L0_16x16 ? 1 : (type <= FER_P_8x16 ? 2 : 4);
    const int i = lane & 3, pi = i < np ? i : 0;
    const int q = (type == FER_P_16x8 && pi == 1) ? 2 : pi;  // quadrant that carries partition i's vector
    int px, py;
    predict_luma_tbl(tbl, d.mbw, mbx, mby, type, pi, px, py);
    const int w = __shfl(tbl, q);
    if (lane < 4) {
        R.mvd[lane][0] = i < np ? (int)(short)(w & 0xffff) - px : 0;
        R.mvd[lane][1] = i < np ? (w >> 16) - py : 0;
        R.mv[lane][0] = J.mv[lane][0];
        R.mv[lane][1] = J.mv[lane][1];
    }
    if (lane == 0) R.fits = 1;
}

extern "C" int ferhip_mv_mbs(const ferhip_mv_job *jobs, ferhip_mv_result *results, size_t n)
{
    if (fer_seam_check_mv_mbs(jobs, results, n)) return FERHIP_E_ARG;
    DevBuf<ferhip_mv_job> dj;
    DevBuf<ferhip_mv_result> dr;
    SeamDev sd;  // the kernel fills the vector field and the type array itself
    if (dj.reserve(n) || dr.reserve(n) || sd.reserve(n, FERHIP_NB_MBS, SA_BIT(mv) | SA_BIT(mb_type))) return FERHIP_E_HIP;
    CK(hipMemcpy(dj, jobs, n * sizeof *jobs, hipMemcpyHostToDevice));
    CK(hipMemset(dr, 0, n * sizeof *results));
    const FerDev d = sd.dev(FERHIP_NB_W, FERHIP_NB_H, SEAM_MBW, FERHIP_NB_H / 16, FERHIP_NB_MBS, n);
    hipLaunchKernelGGL(k_seam_mv, dim3((unsigned)n), dim3(64), 0, 0, d, dj.p, dr.p);
    CK(hipGetLastError());
    CK(hipMemcpy(results, dr, n * sizeof *results, hipMemcpyDeviceToHost));
    return 0;
}

// ---- MotionCompensateSubMBPart for n (macroblock, 4x4 sub-block, vector) triples on one reference picture:
// thread = one luma sample of the 4x4 block (lanes 0..15), one chroma sample of either plane's 2x2 block (16..23),
// and the four-sample row form the residual kernel uses for the same chroma samples (24..27: Cb rows, 28..31: Cr rows)
__global__ __launch_bounds__(64) void k_mc_parts(const uint8_t *ref, int W, int H, const int32_t *desc, int n, int32_t *predL, int32_t *predCb,
                                                 int32_t *predCr, int32_t *rowCb, int32_t *rowCr)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const int mbw = W >> 4, Wc = W >> 1, Hc = H >> 1;
    const uint8_t *RY = ref, *RCb = ref + (size_t)W * H, *RCr = RCb + (size_t)Wc * Hc;
    const int mb = desc[i * 5], sub = desc[i * 5 + 1], part = desc[i * 5 + 2], mvx = desc[i * 5 + 3], mvy = desc[i * 5 + 4];
    const int org_y = ((sub & 2) << 2) + ((part & 2) << 1), org_x = ((sub & 1) << 3) + ((part & 1) << 2);
    const int xP = (mb % mbw) << 4, yP = (mb / mbw) << 4;
    if (lane < 16) {
        predL[i * 16 + lane] = mc_luma(RY, W, H, xP, yP, org_x + (lane & 3), org_y + (lane >> 2), mvx, mvy);
    } else if (lane < 24) {
        const int k = lane & 3, pl = (lane >> 2) & 1;
        const int v = mc_chroma(pl ? RCr : RCb, Wc, Hc, xP >> 1, yP >> 1, (org_x >> 1) + (k & 1), (org_y >> 1) + (k >> 1), mvx, mvy);
        (pl ? predCr : predCb)[i * 4 + k] = v;
    } else if (lane < 32) {
        // mc_chroma_row4 computes the four samples x0 .. x0 + 3 of a chroma row with the vector of the first one; the
        // 2x2 block of this sub-block lies in the row's first or second half
        const int pl = (lane >> 2) & 1, ry = (lane & 3) >> 1, half = lane & 1;
        const int cy = (org_y >> 1) + ry, cx0 = ((org_x >> 1) & ~3);
        int o[4];
        mc_chroma_row4(pl ? RCr : RCb, Wc, Hc, xP >> 1, yP >> 1, cx0, cy, mvx, mvy, o);
        const int within = (org_x >> 1) & 3;  // 0 or 2: where the 2x2 block sits in the row of four
        if (half == 0) {
            (pl ? rowCr : rowCb)[i * 4 + ry * 2 + 0] = o[within];
            (pl ? rowCr : rowCb)[i * 4 + ry * 2 + 1] = o[within + 1];
        }
    }
}

extern "C" int ferhip_mc_sub_mb_parts(const uint8_t *ref_i420, int width, int height, const int32_t *desc, size_t n, int32_t *predL,
                                      int32_t *predCb, int32_t *predCr)
{
    if (fer_seam_check_mc_parts(ref_i420, width, height, desc, n, predL, predCb, predCr)) return FERHIP_E_ARG;
    const size_t fsz = (size_t)width * height * 3 / 2;
    DevBuf<uint8_t> dref;
    DevBuf<int32_t> dd, dl, db, dr, rb, rr;
    std::vector<int32_t> hb(n * 4), hr(n * 4);
    if (dref.reserve(fsz + 256) || dd.reserve(n * 5) || dl.reserve(n * 16) || db.reserve(n * 4) || dr.reserve(n * 4) || rb.reserve(n * 4) ||
        rr.reserve(n * 4))
        return FERHIP_E_HIP;
    CK(hipMemcpy(dref, ref_i420, fsz, hipMemcpyHostToDevice));
    CK(hipMemcpy(dd, desc, n * 20, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_mc_parts, dim3((unsigned)n), dim3(64), 0, 0, dref.p, width, height, dd.p, (int)n, dl.p, db.p, dr.p, rb.p, rr.p);
    CK(hipGetLastError());
    CK(hipMemcpy(predL, dl, n * 64, hipMemcpyDeviceToHost));
    CK(hipMemcpy(predCb, db, n * 16, hipMemcpyDeviceToHost));
    CK(hipMemcpy(predCr, dr, n * 16, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hb.data(), rb, n * 16, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hr.data(), rr, n * 16, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n * 4; i++)
        if (hb[i] != predCb[i] || hr[i] != predCr[i]) {
            fprintf(stderr, "ferhip_mc_sub_mb_parts: the row form of the chroma interpolation differs at sub-block %zu\n", i / 4);
            return FERHIP_E_DEVICE;
        }
    return 0;
}

// ---- block-level KATs: the reference's per-block entry points (F/quantizationTransform.h, F/scaleTransform.h) as
// batched device calls over the SAME device functions the production kernels use (fer_dev.h)
#define KAT_FWD_RESIDUAL 0
#define KAT_INV_RESIDUAL 1
#define KAT_FWD_DC_LUMA 2
#define KAT_INV_DC_LUMA 3
#define KAT_FWD_DC_CHROMA 4
#define KAT_INV_DC_CHROMA 5
#define KAT_SCAN 6
#define KAT_INV_SCAN 7
__global__ void k_block_kat(int op, int qP, const int32_t *in, int32_t *out, int flag, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int a[16], t[16], b[16];
    for (int k = 0; k < 16; k++) {
        a[k] = in[i * 16 + k];
        b[k] = 0;
    }
    switch (op) {
    case KAT_FWD_RESIDUAL:
        fwd4x4(a, t);
        quant4x4(t, b, qP, flag != 0);
        break;
    case KAT_INV_RESIDUAL: inv4x4(a, b, qP, flag != 0); break;
    case KAT_FWD_DC_LUMA: fwd_dc_luma(a, b, qP); break;
    case KAT_INV_DC_LUMA: inv_dc_luma(a, b, qP); break;
    case KAT_FWD_DC_CHROMA: fwd_dc_chroma(a, b, qP); break;   // 2x2 raster in slots 0..3
    case KAT_INV_DC_CHROMA: inv_dc_chroma(a, b, qP); break;
    case KAT_SCAN:  // transformScan: flag = Intra16x16AC (15 entries from index 1)
        for (int k = flag ? 1 : 0; k < 16; k++) b[k - (flag ? 1 : 0)] = a[c_zz[k]];
        break;
    default:  // transformInverseScan
        for (int k = 0; k < 16; k++) b[c_zz[k]] = a[k];
        break;
    }
    for (int k = 0; k < 16; k++) out[i * 16 + k] = b[k];
}

static int block_kat(int op, int qP, const int32_t *in, int32_t *out, int flag, size_t n)
{
    if (fer_seam_check_block_kat(qP, in, out)) return FERHIP_E_ARG;
    if (n == 0) return 0;
    DevBuf<int32_t> di, dout;
    if (di.reserve(n * 16) || dout.reserve(n * 16)) return FERHIP_E_HIP;
    CK(hipMemcpy(di, in, n * 64, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_block_kat, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, qP, di.p, dout.p, flag, n);
    CK(hipGetLastError());
    CK(hipMemcpy(out, dout, n * 64, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ferhip_forward_residual(int qP, const int32_t *in, int32_t *out, int keep_dc, size_t n)
{
    return block_kat(KAT_FWD_RESIDUAL, qP, in, out, keep_dc, n);
}
extern "C" int ferhip_inverse_residual(int qP, const int32_t *in, int32_t *out, int keep_dc, size_t n)
{
    return block_kat(KAT_INV_RESIDUAL, qP, in, out, keep_dc, n);
}
extern "C" int ferhip_forward_dc_luma_intra(int qP, const int32_t *in, int32_t *out, size_t n) { return block_kat(KAT_FWD_DC_LUMA, qP, in, out, 0, n); }
extern "C" int ferhip_inverse_dc_luma_intra(int qP, const int32_t *in, int32_t *out, size_t n) { return block_kat(KAT_INV_DC_LUMA, qP, in, out, 0, n); }
extern "C" int ferhip_forward_dc_chroma(int qP, const int32_t *in, int32_t *out, size_t n) { return block_kat(KAT_FWD_DC_CHROMA, qP, in, out, 0, n); }
extern "C" int ferhip_inverse_dc_chroma(int qP, const int32_t *in, int32_t *out, size_t n) { return block_kat(KAT_INV_DC_CHROMA, qP, in, out, 0, n); }
extern "C" int ferhip_transform_scan(const int32_t *in, int32_t *out, int intra16x16_ac, size_t n) { return block_kat(KAT_SCAN, 0, in, out, intra16x16_ac, n); }
extern "C" int ferhip_transform_inverse_scan(const int32_t *in, int32_t *out, size_t n) { return block_kat(KAT_INV_SCAN, 0, in, out, 0, n); }
