// fer_decode.hip -- the decode twin of the hot path (row a19 of SURVEY.md 8a, BASELINE configs[4]):
// the macroblock loop of RBSP_decode (F/rbsp_decoding.cpp:77-351) on the GPU.
//
//   k_dec_parse   slice_data parsing is bit-serial inside a slice (one slice per picture), so one
//                 WAVEFRONT walks one picture and the parallelism is pictures: every picture of a
//                 window of all streams is parsed by one launch (k_dec_carry / k_dec_patch then
//                 resolve what a picture inherits from its predecessor).  The code is
//                 lane-independent and kept on the scalar unit; it emits, per macroblock, mb_type,
//                 QP, final motion vectors (DeriveMVs, F/mode_pred.cpp:428), Intra4x4 modes, CBP,
//                 TotalCoeff and the coefficient levels -- CAVLC of F/residual.cpp:959-1386.
//   k_dec_inter   every inter / P_Skip macroblock in parallel: motion compensation
//                 (F/mocomp.cpp), dequantisation + inverse transform, clipped reconstruction.
//   k_dec_intra   intra macroblocks along the anti-diagonal wavefront x + 2y (they read
//                 reconstructed neighbours): intraPrediction (F/intra.cpp:770) + residual.
//   k_dec_out     the live decoder's output of whole pictures as tight I420 at a 16-byte aligned address; every other
//                 output (a window, an unaligned address, a pitched layout, NV12) is k_pic_emit's in fer_pic.hip.
//
// Supported syntax: what the reference encoder emits plus intra macroblocks inside P slices and
// non-zero mb_qp_delta.  All four P sub-macroblock types are parsed (like the reference's DeriveMVs, the first vector
// difference of a sub-macroblock stands for all of it); a sub_mb_type above 3 is a syntax error, and I_PCM (mb_type 25 in
// an I slice, 30 in a P slice) sets FER_ERR_DEC_UNSUPPORTED.
// Decoder quirks of the reference that its output depends on are kept: mb_qp_delta persists when
// absent (F/rbsp_decoding.cpp:298,322), chroma AC levels persist into cbp == 0 macroblocks
// (F/residual.cpp:28-49), the more_rbsp_data heuristic (F/rbsp_IO.cpp:193).
#include "fer_decode_dev.h"
#include "fer_internal.h"
#include "fer_intra_dev.h"
#include "fer_mvpred.h"

#include <algorithm>
#include <map>
#include <mutex>

// the decode tables of every device that has decoded (built on first use, kept until exit)
static std::mutex g_dec_luts_mu;
static std::map<int, DecLuts *> g_dec_luts;

// second build step: split the 16-bit coeff_token table by its first 8 bits
__global__ void k_dec_split_luts(DecLuts *L)
{
    const int cls = blockIdx.x, p = threadIdx.x;  // 4 x 256
    const uint16_t e0 = L->ct[cls][p << 8];
    bool uniform = true;  // a code of <= 8 bits fills all 256 completions of its prefix
    for (int x = 1; x < 256; x++) uniform &= L->ct[cls][(p << 8) | x] == e0;
    if (uniform && (e0 == 0 || (e0 >> 8) <= 8)) {
        L->ct1[cls][p] = e0;
        return;
    }
    int id = atomicAdd(&L->nsub, 1);
    if (id >= DEC_CT_SUBS) {
        L->ct1[cls][p] = 0;
        return;
    }
    L->ct1[cls][p] = (uint16_t)(0x8000 | id);
    for (int x = 0; x < 256; x++) L->ct2[id][x] = L->ct[cls][(p << 8) | x];
}

__global__ void k_dec_build_luts(DecLuts *L)
{
    const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;  // 16-bit window
    if (v < 65536) {
        for (int cls = 0; cls < 4; cls++) {
            uint16_t e = 0;
            const int maxtc = cls == 3 ? 4 : 16;
            for (int T = 0; T <= maxtc && !e; T++)
                for (int o = 0; o <= 3 && o <= T; o++) {
                    int len = cls == 3 ? c_ctdc_len[o][T] : c_ct_len[cls][o][T];
                    unsigned code = cls == 3 ? c_ctdc_code[o][T] : c_ct_code[cls][o][T];
                    if (len > 0 && (v >> (16 - len)) == code) {
                        e = (uint16_t)((len << 8) | (T << 2) | o);
                        break;
                    }
                }
            L->ct[cls][v] = e;
        }
    }
    if (v < (1u << DEC_LEV_BITS))
        for (int st = 0; st < DEC_LEV_STATES; st++) {
            const int sl = st < 7 ? st : st - 7;
            uint16_t e = 0;
            if (v != 0) {
                const int prefix = __clz((int)v) - (32 - DEC_LEV_BITS);  // < 14: no escape, the suffix has sl bits
                const int total = prefix + 1 + sl;
                if (total <= DEC_LEV_BITS) {
                    const int suffix = (int)((v >> (DEC_LEV_BITS - total)) & ((1u << sl) - 1u));
                    int levelCode = (prefix << sl) + suffix;
                    if (st >= 7) levelCode += 2;
                    const int lev = (levelCode & 1) == 0 ? (levelCode + 2) >> 1 : (-levelCode - 1) >> 1;
                    int nsl = sl == 0 ? 1 : sl;
                    if (iabs(lev) > (3 << (nsl - 1)) && nsl < 6) nsl++;
                    e = (uint16_t)(total | (nsl << 4) | ((lev & 0x1ff) << 7));
                }
            }
            L->lev[st][v] = e;
        }
    if (v < 512)
        for (int tcm1 = 0; tcm1 < 15; tcm1++) {
            uint16_t e = 0;
            for (int tz = 0; tz <= 15; tz++) {
                int len = c_tz_len[tcm1][tz];
                if (len > 0 && (v >> (9 - len)) == c_tz_code[tcm1][tz]) {
                    e = (uint16_t)((len << 8) | tz);
                    break;
                }
            }
            L->tz[tcm1][v] = e;
        }
    if (v < 8) {
        for (int tcm1 = 0; tcm1 < 3; tcm1++) {
            uint16_t e = 0;
            for (int tz = 0; tz <= 3; tz++) {
                int len = c_tzdc_len[tcm1][tz];
                if (len > 0 && (v >> (3 - len)) == c_tzdc_code[tcm1][tz]) {
                    e = (uint16_t)((len << 8) | tz);
                    break;
                }
            }
            L->tzdc[tcm1][v] = e;
        }
        for (int zl = 0; zl < 6; zl++) {
            uint16_t e = 0;
            for (int k = 0; k <= zl + 1; k++) {
                int len = c_rb_len[zl][k];
                if (len > 0 && (v >> (3 - len)) == c_rb_code[zl][k]) {
                    e = (uint16_t)((len << 8) | k);
                    break;
                }
            }
            L->rb[zl][v] = e;
        }
    }
}

// One wavefront per (stream, picture of the window).  What a picture inherits from its predecessor -- the
// mb_qp_delta that persists when absent and the ChromaACLevel block that persists into macroblocks without
// residual (reference quirks) -- changes no bit position, so every picture is parsed as if it inherited zeros;
// it reports how many macroblocks ran on the inherited delta and flags those that show the inherited block,
// k_dec_carry hands the true values down the pictures of a stream and k_dec_patch applies them.
// PW pictures (wavefronts) per workgroup share the decode tables in LDS; the launch takes the largest PW whose tables,
// per-wavefront scratch and neighbour rows fit the CU's 160 KB (16 at 1080p: the scalar chains of 16 pictures hide
// each other's table round trips, 8 left the scalar unit half idle).
#define DEC_WSYNC()                                        \
    do {                                                   \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                   \
    } while (0)
template <int DEC_PW>
__global__ __launch_bounds__(64 * DEC_PW) void k_dec_parse(FerDev d, DecBatch B, const DecLuts *__restrict__ luts)
{
    __shared__ uint8_t tcur_w[DEC_PW][24];
    __shared__ uint32_t ring_w[DEC_PW][128];  // the bit reader's window on the stream
    __shared__ int16_t cac_w[DEC_PW][2][4][16];  // ChromaACLevel persists across macroblocks (reference quirk)
    __shared__ __attribute__((aligned(16))) int16_t mblv_w[DEC_PW][FER_LEVELS];  // levels of the macroblock being parsed
    __shared__ DecLutsLds lut;
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    DecNb *row = (DecNb *)dyn_lds + (size_t)wv * d.mbw;  // [mbw] per wavefront
    // Intra4x4PredMode of blocks 10, 11, 14, 15 of the macroblock above, 4 bits each: getIntra4x4PredMode reads its neighbours
    // from here and from scalar registers, not from the mode array in memory (16 dependent round trips per macroblock)
    uint16_t *i4row = (uint16_t *)((DecNb *)dyn_lds + (size_t)DEC_PW * d.mbw) + (size_t)wv * d.mbw;
    unsigned long long left_modes = 0;  // the modes of the last Intra4x4 macroblock parsed (the left neighbour when its i4 flag says so)
    uint8_t *tcur = tcur_w[wv];
    int16_t(*cac)[4][16] = cac_w[wv];
    int16_t *mblv = mblv_w[wv];
    {  // decode tables into LDS, once per workgroup
        const uint32_t *src = (const uint32_t *)&luts->ct1[0][0];
        uint32_t *dst = (uint32_t *)&lut;
        for (int i = threadIdx.x; i < (int)(sizeof(DecLutsLds) / 4); i += 64 * DEC_PW) dst[i] = src[i];
        __syncthreads();
    }
    // Pictures are handed out through a counter (B.state[2] of the window's first picture, cleared by the launch): the
    // I pictures of the window's first step -- the longest scalar chains of the launch -- go out first, one to each
    // workgroup in turn (so to different CUs), and a wavefront that has finished a short P picture takes the next one
    // instead of idling beside an I picture until the workgroup ends.
    for (;;) {
        size_t pic;
        {
            int tk = 0;
            if (lane == 0) tk = atomicAdd(&B.state[2], 1);
            tk = __builtin_amdgcn_readfirstlane(tk);
            if (tk >= (int)gridDim.x * DEC_PW) break;
            pic = (size_t)(tk % DEC_PW) * gridDim.x + (size_t)(tk / DEC_PW);  // ticket -> picture: DEC_PW consecutive tickets are gridDim.x pictures apart
        }
        if (pic >= (size_t)B.TW * d.S) continue;
        const int tpic = (int)(pic / d.S), s = (int)(pic % d.S);
        const uint32_t *info = B.info + pic * 6;
        // this picture's slice of the side information (the kernel argument d itself is never written: a modified copy of
        // that 900-byte structure would live in scratch memory)
        const size_t po = (size_t)tpic * d.S * d.nmb;
        int *const p_mb_type = B.mb_type + po;
        short *const p_mv = B.mv + po * 8;
        uint8_t *const p_cbp = B.cbp + po * 2, *const p_tc = B.tc + po * 24, *const p_i4mode = B.i4mode + po * 16;
        uint8_t *const p_i4flag = B.i4flag + po * 16, *const p_chroma_mode = B.chroma_mode + po, *const p_dec_qp = B.dec_qp + po;
        int16_t *const p_levels = B.levels + po * FER_LEVELS;
        uint8_t *carry = B.carry + pic * d.nmb;
        int *st = B.state + pic * 4, *summ = B.summ + pic * 4;
        // the slice parameters are the same in every lane: scalar registers, so that everything derived from them
        // (bit position, window, QP) stays on the scalar unit
        const unsigned i_size = (unsigned)__builtin_amdgcn_readfirstlane((int)info[0]);
        const unsigned i_pos = (unsigned)__builtin_amdgcn_readfirstlane((int)info[1]);
        const int i_slice = __builtin_amdgcn_readfirstlane((int)info[2]);
        const int stype = i_slice & 255;
        // ref_idx_l0 is parsed and dropped (every prediction uses the one stored picture): in sub_mb_pred the reference
        // reads it when the slice carried num_ref_idx_active_override_flag, in mb_pred when the active count left behind
        // by the last override is > 1 (F/rbsp_decoding.cpp:156-161, :217-221)
        const bool ref_sub = ((i_slice >> 8) & 1) != 0, ref_mb = (i_slice >> 16) > 0;
        const unsigned i_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)info[4]), i_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)info[5]);
        if (i_size == 0) {  // no picture for this stream at this step
            if (lane == 0) {
                st[1] = 0;
                st[3] = 0;
                summ[0] = summ[3] = 0;
            }
            continue;
        }
        const bool constrained_intra = __builtin_amdgcn_readfirstlane((int)B.hdr[pic * 4 + 1]) != 0;
        DecBits b;
        db_open(b, B.rbsp + (((size_t)i_hi << 32) | i_lo), i_size, i_pos, ring_w[wv]);
        int QPy = __builtin_amdgcn_readfirstlane((int)info[3]);
        int *mbt = p_mb_type + (size_t)s * d.nmb;
        short *mvs = p_mv + (size_t)s * d.nmb * 8;
        int mb_qp_delta = 0;  // the inherited value is added by k_dec_patch
        bool delta_known = false, cac_known = false;
        int n_inherit = 0;    // macroblocks whose QP step used the inherited delta
        for (int i = lane; i < 2 * 4 * 16; i += 64) (&cac[0][0][0])[i] = 0;
        DEC_WSYNC();
        int cur = 0;
        int perr = 0;  // the error that ended this picture's parse (d.status only says which stream)
        bool more = true;
        int mvd[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
        int sub[4] = {0, 0, 0, 0};
#ifdef FER_PROBE
        long long tacc[4] = {0, 0, 0, 0}, tmark = wall_clock64();
#define DP_MARK(k)                        \
        {                                     \
            long long now_ = wall_clock64();  \
            tacc[k] += now_ - tmark;          \
            tmark = now_;                     \
        }
#else
#define DP_MARK(k)
#endif
        while (more && cur < d.nmb) {
            DP_MARK(3)
            if (stype != 2) {
                int run = (int)db_ue(b);
                for (int i = 0; i < run && cur < d.nmb; i++) {
                    size_t mbi = (size_t)s * d.nmb + cur;
                    mbt[cur] = FER_P_SKIP;
                    if (lane == 0) {
                        row[cur % d.mbw].skip = 1;
                        row[cur % d.mbw].i4 = 0;
                    }
                    for (int k = 0; k < 4; k++) mvd[k][0] = mvd[k][1] = 0;  // ClearMVD in PredictMV
                    dec_derive_mvs(d, mvs, mbt, cur, FER_P_SKIP, mvd, sub);
                    QPy = (QPy + mb_qp_delta + 52) % 52;
                    n_inherit += delta_known ? 0 : 1;
                    p_dec_qp[mbi] = (uint8_t)QPy;
                    if (lane == 0) carry[cur] = 0;
                    cur++;
                }
                if (cur != 0 || run > 0) more = db_more(b);
                if (more && cur >= d.nmb) {
                    // data behind a skip run that ends the picture: the reference goes on to parse a macroblock past the picture
                    // (F/rbsp_decoding.cpp:121 tests moreDataFlag alone).  It is followed as far as it only reads the stream --
                    // mb_type and an intra type's prediction modes, with the fatal errors the reference has there -- not into
                    // what it then decodes behind its pictures: short of those errors the picture is complete.
                    const int t = (int)db_ue(b);
                    bool past = t > 31;
                    if (!past && t >= 5 && t <= 29) {
                        if (t == 5)
                            for (int blk = 0; blk < 16; blk++)
                                if (!db_bit(b)) db_bits(b, 3);
                        past = db_ue(b) > 3;
                    }
                    if (past) {
                        atomicOr(&d.status[s], FER_ERR_DEC_SYNTAX);
                        perr = FER_ERR_DEC_SYNTAX;
                    }
                    break;
                }
            }
            if (!(more && cur < d.nmb)) break;
            const size_t mbi = (size_t)s * d.nmb + cur;
            const int mbx = cur % d.mbw, mby = cur / d.mbw;
            int16_t *lv = mblv;
            for (int i = lane; i < FER_LEVELS / 2; i += 64) ((uint32_t *)mblv)[i] = 0;
            int t = (int)db_ue(b);
            if (t > 30 || (stype == 2 && t > 25)) {  // (25 / 30 is I_PCM, below)
                atomicOr(&d.status[s], FER_ERR_DEC_SYNTAX);
                perr = FER_ERR_DEC_SYNTAX;
                break;
            }
            mbt[cur] = t;
            const int k = stype == 2 ? t : t - 5;  // index into the I macroblock table
            const bool i4 = stype == 2 ? t == 0 : t == 5;
            const bool i16 = stype == 2 ? (t >= 1 && t <= 24) : (t >= 6 && t <= 29);
            const bool inter = !i4 && !i16;
            if ((t == 25 && stype == 2) || (t == 30 && stype != 2)) {
                atomicOr(&d.status[s], FER_ERR_DEC_UNSUPPORTED);  // I_PCM
                perr = FER_ERR_DEC_UNSUPPORTED;
                break;
            }
            int chroma_mode = 0;
            unsigned long long i4flags = 0;  // prev_intra4x4_pred_mode_flag << 3 | rem_intra4x4_pred_mode, 4 bits per block
            bool left_i4 = false, above_i4 = false;
            unsigned above_modes = 0;
            if (inter) {
                if (t == 3 || t == 4) {
                    bool badsub = false;
                    for (int i = 0; i < 4; i++) {
                        sub[i] = (int)db_ue(b);
                        badsub |= sub[i] > 3;
                    }
                    if (badsub) {
                        atomicOr(&d.status[s], FER_ERR_DEC_SYNTAX);
                        perr = FER_ERR_DEC_SYNTAX;
                        break;
                    }
                    if (ref_sub && t != FER_P_8x8ref0)
                        for (int i = 0; i < 4; i++) db_te(b);
                    for (int i = 0; i < 4; i++) {
                        // sub-partitions: 8x8 1, 8x4 2, 4x8 2, 4x4 4 vector differences, of which DeriveMVs keeps the first
                        const int nsub = sub[i] == 0 ? 1 : (sub[i] == 3 ? 4 : 2);
                        for (int j = 0; j < nsub; j++) {
                            int dx = db_se(b), dy = db_se(b);
                            if (j == 0) {
                                mvd[i][0] = dx;
                                mvd[i][1] = dy;
                            }
                        }
                    }
                } else {
                    int np = t == 0 ? 1 : 2;
                    if (ref_mb)
                        for (int i = 0; i < np; i++) db_te(b);
                    for (int i = 0; i < np; i++) {
                        mvd[i][0] = db_se(b);
                        mvd[i][1] = db_se(b);
                    }
                }
            } else {
                if (i4) {
                    for (int blk = 0; blk < 16; blk++) {
                        int f = (int)db_bit(b);
                        int rem = f ? 0 : (int)db_bits(b, 3);
                        i4flags |= (unsigned long long)((f << 3) | rem) << (4 * blk);
                    }
                    if (lane < 16) p_i4flag[mbi * 16 + lane] = (uint8_t)((i4flags >> (4 * lane)) & 15);
                    // the neighbours' side of getIntra4x4PredMode, before this macroblock takes the place of the one above
                    left_i4 = mbx > 0 && __builtin_amdgcn_readfirstlane((int)row[mbx - 1].i4) != 0;
                    above_i4 = mby > 0 && __builtin_amdgcn_readfirstlane((int)row[mbx].i4) != 0;
                    above_modes = (unsigned)__builtin_amdgcn_readfirstlane((int)i4row[mbx]);
                }
                chroma_mode = (int)db_ue(b);
                if (chroma_mode > 3) {
                    atomicOr(&d.status[s], FER_ERR_DEC_SYNTAX);
                    perr = FER_ERR_DEC_SYNTAX;
                    break;
                }
            }
            int cbpL, cbpC;
            if (!i16) {
                unsigned code = db_ue(b);
                if (code > 47) {
                    atomicOr(&d.status[s], FER_ERR_DEC_SYNTAX);
                    perr = FER_ERR_DEC_SYNTAX;
                    break;
                }
                int cbp = i4 ? c_code_cbp_intra[code] : c_code_cbp_inter[code];
                cbpL = cbp & 15;
                cbpC = cbp >> 4;
            } else {
                cbpC = ((k - 1) / 4) % 3;
                cbpL = k >= 13 ? 15 : 0;
            }
            p_cbp[mbi * 2] = (uint8_t)cbpL;
            p_cbp[mbi * 2 + 1] = (uint8_t)cbpC;
            p_chroma_mode[mbi] = (uint8_t)chroma_mode;
            for (int i = lane; i < 24; i += 64) tcur[i] = 0;
            DEC_WSYNC();
            DP_MARK(0)
            bool bad = false;
            if (cbpL > 0 || cbpC > 0 || i16) {
                mb_qp_delta = db_se(b);
                delta_known = true;
                if (mb_qp_delta < -26 || mb_qp_delta > 25) bad = true;
                // residual(0,15), F/residual.cpp:959-1067
                if (i16 && !bad) {
                    int n = dec_block(b, &lut, lv + FER_LV_DC16, 16, dec_nC(row, mbx, mby, true, 0, 0, tcur, cbpL, cbpC));
                    bad |= n < 0;
                    if (n >= 0) tcur[0] = (uint8_t)n;
                    DEC_WSYNC();
                }
                for (int i8 = 0; i8 < 4 && !bad; i8++)
                    if (cbpL & (1 << i8))
                        for (int i4x = 0; i4x < 4 && !bad; i4x++) {
                            int blk = i8 * 4 + i4x;
                            int n = dec_block(b, &lut, lv + blk * 16, i16 ? 15 : 16, dec_nC(row, mbx, mby, true, blk, 0, tcur, cbpL, cbpC));
                            bad |= n < 0;
                            if (n >= 0) tcur[blk] = (uint8_t)n;
                            DEC_WSYNC();
                        }
                for (int pl = 0; pl < 2 && !bad; pl++)
                    if (cbpC & 3) bad |= dec_block(b, &lut, lv + FER_LV_CDC + pl * 4, 4, -1) < 0;
                for (int pl = 0; pl < 2 && !bad; pl++)
                    for (int cb = 0; cb < 4 && !bad; cb++) {
                        if (cbpC & 2) {
                            for (int i = lane; i < 16; i += 64) cac[pl][cb][i] = 0;
                            DEC_WSYNC();
                            int n = dec_block(b, &lut, &cac[pl][cb][0], 15, dec_nC(row, mbx, mby, false, cb, pl, tcur, cbpL, cbpC));
                            bad |= n < 0;
                            if (n >= 0) tcur[16 + pl * 4 + cb] = (uint8_t)n;
                            DEC_WSYNC();
                        } else {
                            for (int i = lane; i < 16; i += 64) cac[pl][cb][i] = 0;
                            DEC_WSYNC();
                        }
                    }
            }
            DP_MARK(1)
            if (bad) {
                atomicOr(&d.status[s], FER_ERR_DEC_SYNTAX);
                perr = FER_ERR_DEC_SYNTAX;
                break;
            }
            // chroma AC of this macroblock = the persistent ChromaACLevel (stale when cbp == 0)
            if (cbpL > 0 || cbpC > 0 || i16) cac_known = true;  // every block was parsed or cleared above
            if (lane == 0) carry[cur] = cac_known ? 0 : 1;
            for (int i = lane; i < 120; i += 64) lv[FER_LV_CAC + i] = cac[i / 60][(i % 60) / 15][i % 15];
            DEC_WSYNC();
            {  // the finished macroblock: levels to memory (one coalesced pass), counts into the neighbour row
                uint32_t *g = (uint32_t *)(p_levels + mbi * FER_LEVELS);
                for (int i = lane; i < FER_LEVELS / 2; i += 64) g[i] = ((const uint32_t *)mblv)[i];
                DecNb &me = row[mbx];
                if (lane < 24) {
                    p_tc[mbi * 24 + lane] = tcur[lane];
                    me.tc[lane] = tcur[lane];
                }
                if (lane == 0) {
                    me.cbpL = (uint8_t)cbpL;
                    me.cbpC = (uint8_t)cbpC;
                    me.skip = 0;
                    me.i4 = i4 ? 1 : 0;
                }
            }
            DEC_WSYNC();
            QPy = (QPy + mb_qp_delta + 52) % 52;
            n_inherit += delta_known ? 0 : 1;
            p_dec_qp[mbi] = (uint8_t)QPy;
            if (inter) {
                if (!dec_derive_mvs(d, mvs, mbt, cur, t, mvd, sub)) {  // a vector past 16 bits
                    atomicOr(&d.status[s], FER_ERR_DEC_SYNTAX);
                    perr = FER_ERR_DEC_SYNTAX;
                    break;
                }
            } else if (i4) {
                // this macroblock's modes, 4 bits per block
                const unsigned long long cm = dec_i4_modes(i4flags, mbx, mby, constrained_intra, left_i4, left_modes, above_i4, above_modes);
                if (lane < 16) p_i4mode[mbi * 16 + lane] = (uint8_t)((cm >> (4 * lane)) & 15);
                if (lane == 0) i4row[mbx] = (uint16_t)(((cm >> 40) & 0xff) | (((cm >> 56) & 0xff) << 8));  // blocks 10, 11 | 14, 15
                left_modes = cm;
            }
            more = db_more(b);
            cur++;
            DP_MARK(2)
        }
#ifdef FER_PROBE
        if (s == 0 && lane == 0) {
            for (int k = 0; k < 4; k++) d.timing[48 + k] += tacc[k];
            d.timing[52] += cur;
        }
#endif
#undef DP_MARK
        DEC_WSYNC();
        for (int i = lane; i < 128; i += 64) B.cac_out[pic * 128 + i] = (&cac[0][0][0])[i];
        if (lane == 0) {
            st[1] = cur;  // macroblocks reached (the rest of the picture keeps the previous content)
            st[3] = perr;
            summ[0] = delta_known;
            summ[1] = mb_qp_delta;
            summ[2] = n_inherit;
            summ[3] = cac_known;
        }
        DEC_WSYNC();
    }  // next picture
}

// per stream, down the pictures of the window: what each picture inherits (FerDev.dec_state / dec_cac hold the
// state between windows)
__global__ __launch_bounds__(128) void k_dec_carry(FerDev d, DecBatch B)
{
    const int s = blockIdx.x, i = threadIdx.x;  // thread i carries ChromaACLevel entry i
    int delta = d.dec_state[(size_t)s * 4];
    int16_t v = d.dec_cac[(size_t)s * 128 + i];
    for (int t = 0; t < B.TW; t++) {
        const size_t pic = (size_t)t * d.S + s;
        if (B.info[pic * 6] == 0) continue;
        B.cac_in[pic * 128 + i] = v;
        if (i == 0) B.state[pic * 4] = delta;
        if (B.summ[pic * 4 + 0]) delta = B.summ[pic * 4 + 1];
        if (B.summ[pic * 4 + 3]) v = B.cac_out[pic * 128 + i];
    }
    d.dec_cac[(size_t)s * 128 + i] = v;
    if (i == 0) d.dec_state[(size_t)s * 4] = delta;
}

// QP of the macroblocks that ran on the inherited mb_qp_delta, chroma AC of those that show the inherited block
__global__ __launch_bounds__(256) void k_dec_patch(FerDev d, DecBatch B)
{
    const int s = blockIdx.y, t = blockIdx.z;
    const int mb = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t pic = (size_t)t * d.S + s;
    if (mb >= B.state[pic * 4 + 1]) return;
    const size_t mbi = pic * d.nmb + mb;
    const int delta = B.state[pic * 4];
    if (delta != 0) {
        int steps = min(mb + 1, B.summ[pic * 4 + 2]);
        int q = ((int)B.dec_qp[mbi] + steps * delta) % 52;
        B.dec_qp[mbi] = (uint8_t)(q < 0 ? q + 52 : q);
    }
    if (B.carry[mbi]) {
        int16_t *lv = B.levels + mbi * FER_LEVELS + FER_LV_CAC;
        const int16_t *c = B.cac_in + pic * 128;
        for (int i = 0; i < 120; i++) lv[i] = c[(i / 60) * 64 + ((i % 60) / 15) * 16 + i % 15];
    }
}

// ---- reconstruction of one 4x4 block owned by a lane
__device__ __forceinline__ void recon_block(const int16_t *__restrict__ lvl, int n, int dc, bool keepDC, int qP,
                                            const int p[16], uint8_t *dst, int stride)
{
    int c[16], r[16];
#pragma unroll
    for (int i = 0; i < 16; i++) c[i] = 0;
    if (keepDC) {
        c[0] = dc;
        for (int k = 1; k < 16; k++) c[c_zz[k]] = lvl[k - 1];
    } else {
        for (int k = 0; k < n; k++) c[c_zz[k]] = lvl[k];
    }
    inv4x4(c, r, qP, keepDC);
#pragma unroll
    for (int i = 0; i < 16; i++) dst[(size_t)(i >> 2) * stride + (i & 3)] = (uint8_t)clip255(p[i] + r[i]);
}

// chroma_qp_index_offset and constrained_intra_pred_flag belong to the stream's PPS: they travel with the picture in
// hdr[s][0] and hdr[s][1] (hdr[s][3] = slice type)
__device__ __forceinline__ int dec_qpc(const FerDev &d, int s, int QPy)
{
    const int qpc[52] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17,
                         18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32, 32, 33,
                         34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};
    return qpc[iclamp(QPy + (int)d.hdr[s * 4], 0, 51)];
}

// chroma residual of lanes 16..23 (dc Hadamard shared through shuffles), F/inttransform.cpp:237-320.  pred: uint8_t samples
// (motion compensation) or int16_t (intra prediction, which may hold the -1 of a neighbour that does not exist)
template <typename PredT>
__device__ __forceinline__ void recon_chroma(const FerDev &d, const int16_t *lv, int lane, int qpc_, const PredT *pred,
                                             uint8_t *C0, uint8_t *C1, int Wc, int xp, int yp)
{
    const bool isC = lane >= 16 && lane < 24;
    const int pl = (lane - 16) >> 2, cb = (lane - 16) & 3;
    int cq[4], dq[4];
    int base = lane >= 20 ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 4; i++) cq[i] = lv[FER_LV_CDC + base * 4 + i];
    inv_dc_chroma(cq, dq, qpc_);
    if (isC) {
        int x0 = (cb & 1) * 4, y0 = (cb >> 1) * 4;
        int p[16];
#pragma unroll
        for (int i = 0; i < 16; i++) p[i] = pred[pl * 64 + (y0 + (i >> 2)) * 8 + x0 + (i & 3)];
        uint8_t *dst = (pl ? C1 : C0) + (size_t)(yp / 2 + y0) * Wc + xp / 2 + x0;
        recon_block(lv + FER_LV_CAC + (pl * 4 + cb) * 15, 15, dq[cb], true, qpc_, p, dst, Wc);
    }
}

__global__ __launch_bounds__(64) void k_dec_inter(FerDev d)
{
    __shared__ uint8_t pL[16][16], pC[2 * 64];
    const int lane = threadIdx.x;
    const int s = blockIdx.y, mb = blockIdx.x;
    const size_t mbi = (size_t)s * d.nmb + mb;
    if (mb >= d.dec_state[s * 4 + 1]) return;  // not reached by the parser
    const int t = d.mb_type[mbi];
    const bool inter = t <= 4 || t == FER_P_SKIP;
    if (d.hdr[s * 4 + 3] != 0 || !inter) return;
    const int W = d.W, H = d.H, Wc = d.Wc, Hc = d.Hc;
    uint8_t *Y = d.curY + (size_t)s * d.ysz;
    uint8_t *C0 = d.curCb + (size_t)s * d.csz, *C1 = d.curCr + (size_t)s * d.csz;
    const uint8_t *RY = d.refY + (size_t)s * d.ysz;
    const uint8_t *RC0 = d.refCb + (size_t)s * d.csz, *RC1 = d.refCr + (size_t)s * d.csz;
    const short *mv = d.mv + mbi * 8;
    const int xp = (mb % d.mbw) << 4, yp = (mb / d.mbw) << 4;
    {
        int lx = (lane & 3) * 4, ly = lane >> 2;
        int q = (ly >> 3) * 2 + (lx >> 3);
#pragma unroll
        for (int k = 0; k < 4; k++) pL[ly][lx + k] = (uint8_t)mc_luma(RY, W, H, xp, yp, lx + k, ly, mv[q * 2], mv[q * 2 + 1]);
        int cx = lane & 7, cy = lane >> 3;
        int qc = (cy >> 2) * 2 + (cx >> 2);
        pC[cy * 8 + cx] = (uint8_t)mc_chroma(RC0, Wc, Hc, xp / 2, yp / 2, cx, cy, mv[qc * 2], mv[qc * 2 + 1]);
        pC[64 + cy * 8 + cx] = (uint8_t)mc_chroma(RC1, Wc, Hc, xp / 2, yp / 2, cx, cy, mv[qc * 2], mv[qc * 2 + 1]);
    }
    __syncthreads();
    const int16_t *lv = d.levels + mbi * FER_LEVELS;
    const int QPy = d.dec_qp[mbi];
    if (t == FER_P_SKIP) {  // all levels zero: reconstruction == prediction
        int lx = (lane & 3) * 4, ly = lane >> 2;
#pragma unroll
        for (int k = 0; k < 4; k++) Y[(size_t)(yp + ly) * W + xp + lx + k] = pL[ly][lx + k];
        int cx = lane & 7, cy = lane >> 3;
        C0[(size_t)(yp / 2 + cy) * Wc + xp / 2 + cx] = pC[cy * 8 + cx];
        C1[(size_t)(yp / 2 + cy) * Wc + xp / 2 + cx] = pC[64 + cy * 8 + cx];
        return;
    }
    if (lane < 16) {
        int x0 = c_bx[lane], y0 = c_by[lane];
        int p[16];
#pragma unroll
        for (int i = 0; i < 16; i++) p[i] = pL[y0 + (i >> 2)][x0 + (i & 3)];
        recon_block(lv + lane * 16, 16, 0, false, QPy, p, Y + (size_t)(yp + y0) * W + xp + x0, W);
    }
    recon_chroma(d, lv, lane, dec_qpc(d, s, QPy), pC, C0, C1, Wc, xp, yp);
}

__global__ __launch_bounds__(64) void k_dec_intra(FerDev d, int diag)
{
    __shared__ IntraLds L;
    // chroma prediction as the reference's ints: a stream may name the horizontal / vertical mode where the left / upper
    // macroblock does not exist, and the prediction is then the -1 marker itself (IntraLds.predC, 8 bits, is the encoder's)
    __shared__ int16_t predC[2][8][8];
    const int lane = threadIdx.x;
    const int s = blockIdx.y;
    int y_lo = diag - (d.mbw - 1);
    y_lo = y_lo > 0 ? (y_lo + 1) >> 1 : 0;
    const int mby = y_lo + blockIdx.x, mbx = diag - 2 * mby;
    if (mby >= d.mbh || mbx < 0 || mbx >= d.mbw) return;
    const int mb = mby * d.mbw + mbx;
    const size_t mbi = (size_t)s * d.nmb + mb;
    if (mb >= d.dec_state[s * 4 + 1]) return;
    const int stype = (int)d.hdr[s * 4 + 3];
    const int t = d.mb_type[mbi];
    const bool i4 = stype == 2 ? t == 0 : t == 5;
    const bool i16 = stype == 2 ? (t >= 1 && t <= 24) : (t >= 6 && t <= 29);
    if (!i4 && !i16) return;
    const int W = d.W, Wc = d.Wc;
    uint8_t *Y = d.curY + (size_t)s * d.ysz;
    uint8_t *Cp[2] = {d.curCb + (size_t)s * d.csz, d.curCr + (size_t)s * d.csz};
    const int xp = mbx << 4, yp = mby << 4;
    const bool availL = mbx > 0, availT = mby > 0, lastcol = mbx == d.mbw - 1;
    for (int i = lane; i < 17 * 21; i += 64) {
        int r = i / 21, c = i % 21;
        int gx = xp + c - 1, gy = yp + r - 1;
        int v = -1;
        if (gx >= 0 && gy >= 0 && gx < W && (r == 0 || c == 0)) v = Y[(size_t)gy * W + gx];
        L.fr[r][c] = (int16_t)v;
    }
    for (int i = lane; i < 2 * 9 * 9; i += 64) {
        int pl = i / 81, r = (i % 81) / 9, c = i % 9;
        int gx = xp / 2 + c - 1, gy = yp / 2 + r - 1;
        L.cfr[pl][r][c] = (int16_t)((gx >= 0 && gy >= 0 && (r == 0 || c == 0)) ? Cp[pl][(size_t)gy * Wc + gx] : -1);
    }
    __syncthreads();
    const int16_t *lv = d.levels + mbi * FER_LEVELS;
    const int QPy = d.dec_qp[mbi];
    const int chroma_mode = d.chroma_mode[mbi];
    // chroma prediction (pred_chroma_px: the code of the encoder's phase 2a)
    {
        int cx = lane & 7, cy = lane >> 3;
        for (int pl = 0; pl < 2; pl++) predC[pl][cy][cx] = (int16_t)pred_chroma_px(L.cfr[pl], chroma_mode, cx, cy, availL, availT);
    }
    if (i16) {
        P16 q16;
        pred16_params(L, availL, availT, q16);
        int k = stype == 2 ? t : t - 5;
        int mode = (k - 1) & 3;
        if (lane == 0) {
            int c[16], dq[16];
            for (int i = 0; i < 16; i++) c[c_zz[i]] = lv[FER_LV_DC16 + i];
            inv_dc_luma(c, dq, QPy);
            for (int i = 0; i < 16; i++) L.dcdeq[i] = dq[i];
        }
        __syncthreads();
        if (lane < 16) {
            int x0 = c_bx[lane], y0 = c_by[lane];
            int p[16];
            for (int i = 0; i < 16; i++) p[i] = pred16_px(L, q16, mode, x0 + (i & 3), y0 + (i >> 2));
            recon_block(lv + lane * 16, 15, L.dcdeq[(y0 >> 2) * 4 + (x0 >> 2)], true, QPy, p,
                        Y + (size_t)(yp + y0) * W + xp + x0, W);
        }
    } else {
        // Intra4x4: the blocks reconstruct one after the other (each predicts from the ones before it); four lanes per
        // block, lane r < 4 = row r (inv_row: the vertical half of the inverse transform crosses the quad with DPP),
        // the levels of the macroblock staged in LDS by one coalesced read
        ((uint32_t *)&L.lv4[0][0])[lane] = ((const uint32_t *)lv)[lane];
        ((uint32_t *)&L.lv4[0][0])[64 + lane] = ((const uint32_t *)lv)[64 + lane];
        __syncthreads();
        const int row = lane & 3;
        RowQ rq;
        rq.row = row;
        {
            const int m = QPy % 6;
            const int s_ee = level_scale(m, 0, 0), s_oo = level_scale(m, 1, 1), s_eo = level_scale(m, 0, 1);
            rq.ls[0] = rq.ls[2] = (row & 1) ? s_eo : s_ee;
            rq.ls[1] = rq.ls[3] = (row & 1) ? s_oo : s_eo;
        }
        const uint32_t zrow = ((const uint32_t *)c_izz)[row];
        for (int blk = 0; blk < 16; blk++) {
            int p[13], o[16], c[4], r[4];
            fetch4(L, blk, lastcol, p);
            pred4x4(d.i4mode[mbi * 16 + blk], p, o);
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = L.lv4[blk][(zrow >> (8 * k)) & 15u];
            inv_row(rq, c, QPy, false, r);
            const int x0 = c_bx[blk], y0 = c_by[blk];
            if (lane < 4) {
                uint32_t pk = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int po = row == 0 ? o[k] : (row == 1 ? o[4 + k] : (row == 2 ? o[8 + k] : o[12 + k]));
                    const int v = clip255(po + r[k]);
                    L.fr[1 + y0 + row][1 + x0 + k] = (int16_t)v;
                    pk |= (uint32_t)v << (8 * k);
                }
                *(uint32_t *)(Y + (size_t)(yp + y0 + row) * W + xp + x0) = pk;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    recon_chroma(d, lv, lane, dec_qpc(d, s, QPy), &predC[0][0][0], Cp[0], Cp[1], Wc, xp, yp);
}

// the decode tables of the current device; null if they cannot be allocated
const DecLuts *dec_luts(hipStream_t st)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_dec_luts_mu);
    auto it = g_dec_luts.find(dev);
    if (it != g_dec_luts.end()) return it->second;
    // once per device: invert the code tables.  The build is waited for before the tables are published, so a decoder
    // on another stream of the same device never reads them half-built.
    DecLuts *L = nullptr;
    if (hipMalloc((void **)&L, sizeof(DecLuts)) != hipSuccess) return nullptr;
    hipMemsetAsync(L, 0, sizeof(DecLuts), st);
    hipLaunchKernelGGL(k_dec_build_luts, dim3(256), dim3(256), 0, st, L);
    hipLaunchKernelGGL(k_dec_split_luts, dim3(4), dim3(256), 0, st, L);
    if (hipStreamSynchronize(st) != hipSuccess) {
        hipFree(L);
        return nullptr;
    }
    g_dec_luts[dev] = L;
    return L;
}

void fer_launch_decode_parse(const FerDev &d, const DecBatch &B, hipStream_t st)
{
    const DecLuts *luts = dec_luts(st);
    if (!luts) return;
    // static LDS of k_dec_parse<PW>: the tables + PW * (tcur 24 + stream ring 512 + ChromaACLevel 256 + the macroblock's levels); dynamic: the rows
    const size_t fixed = sizeof(DecLutsLds), per_wave = 24 + 512 + 256 + FER_LEVELS * 2 + (size_t)d.mbw * (sizeof(DecNb) + 2);
    const int npic = d.S * B.TW;
#define DEC_PARSE_LAUNCH(PW)                                                                                                          \
    hipLaunchKernelGGL(k_dec_parse<PW>, dim3((npic + PW - 1) / PW), dim3(64 * PW), (size_t)PW * d.mbw * (sizeof(DecNb) + 2), st, d, B, \
                       luts)
    const size_t lds = 160 * 1024 - 512;
    hipMemsetAsync(B.state + 2, 0, sizeof(int), st);
    if (fixed + 16 * per_wave <= lds)
        DEC_PARSE_LAUNCH(16);
    else if (fixed + 8 * per_wave <= lds)
        DEC_PARSE_LAUNCH(8);
    else if (fixed + 4 * per_wave <= lds)
        DEC_PARSE_LAUNCH(4);
    else
        DEC_PARSE_LAUNCH(1);
#undef DEC_PARSE_LAUNCH
    hipLaunchKernelGGL(k_dec_carry, dim3(d.S), dim3(128), 0, st, d, B);
    hipLaunchKernelGGL(k_dec_patch, dim3((d.nmb + 255) / 256, d.S, B.TW), dim3(256), 0, st, d, B);
}

// reconstruction of one picture per stream; dslice = FerDev whose side-information pointers are the picture's slice
void fer_launch_decode_recon(const FerDev &d, bool anyP, bool anyIntra, hipStream_t st)
{
    if (anyP) hipLaunchKernelGGL(k_dec_inter, dim3(d.nmb, d.S), dim3(64), 0, st, d);
    if (anyIntra) {
        int ndiag = d.mbw + 2 * (d.mbh - 1);
        int maxk = min(d.mbh, (d.mbw + 1) / 2);
        for (int dg = 0; dg < ndiag; dg++) hipLaunchKernelGGL(k_dec_intra, dim3(maxk, d.S), dim3(64), 0, st, d, dg);
    }
}

// k_dec_intra of one anti-diagonal alone (the neighbourhood seam, ferhip_intra_mbs in fer_mbunit.hip)
void fer_launch_decode_intra_diag(const FerDev &d, int diag, hipStream_t st)
{
    hipLaunchKernelGGL(k_dec_intra, dim3(min(d.mbh, (d.mbw + 1) / 2), d.S), dim3(64), 0, st, d, diag);
}

// The decoded pictures of one step, whole and as tight I420, from the plane-major picture set `set` ([S] Y, [S] Cb, [S] Cr)
// into slots of W*H*3/2 bytes at a 16-byte aligned dst: map[j] = (stream, slot), blockIdx.y = j.  Consecutive lanes move
// consecutive V-sized pieces of a slot (every plane is a multiple of 64 bytes, so a piece never straddles two); no other slot
// is touched.  Every other output of the live decoder -- a window, an unaligned dst, pitched slots, NV12 -- is k_pic_emit's
// (fer_pic.hip).
template <typename V>
__global__ __launch_bounds__(256) void k_dec_out(const uint8_t *__restrict__ set, const int2 *__restrict__ map, uint8_t *__restrict__ dst,
                                                 int S, size_t ysz, size_t csz)
{
    const int2 m = map[blockIdx.y];
    const size_t fsz = ysz + 2 * csz, n = fsz / sizeof(V);
    const V *sy = (const V *)(set + (size_t)m.x * ysz);
    const V *su = (const V *)(set + (size_t)S * ysz + (size_t)m.x * csz);
    const V *sv = (const V *)(set + (size_t)S * (ysz + csz) + (size_t)m.x * csz);
    V *o = (V *)(dst + (size_t)m.y * fsz);
    const size_t ny = ysz / sizeof(V), nc = csz / sizeof(V);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        o[i] = i < ny ? sy[i] : (i < ny + nc ? su[i - ny] : sv[i - ny - nc]);
}

void fer_launch_decode_out(const FerDev &d, const uint8_t *set, const int2 *map, int n, uint8_t *dst, hipStream_t st)
{
    if (n <= 0) return;
    const unsigned nb = (unsigned)std::min<size_t>(((d.ysz + 2 * d.csz) / 16 + 255) / 256, 1024);
    hipLaunchKernelGGL(k_dec_out<uint4>, dim3(nb, n), dim3(256), 0, st, set, map, dst, d.S, d.ysz, d.csz);
}
