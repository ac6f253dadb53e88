// fer_seam_pack_host.h -- the hand-built context of the per-macroblock seam (ferhip_residual_mbs, ferhip_intra_mbs,
// ferhip_mv_mbs; fer_mbunit.hip), as far as it is no HIP call: the table of the FerDev side-information arrays the seam
// fills, the host copies of them, the packing of jobs into them and of them into results, and the job order of
// ferhip_intra_mbs.  Plain C++ without the HIP runtime, like fer_seam_host.h, so that the index arithmetic runs in a
// stand-alone program under a sanitizer (tools/seam_pack_host_check.cpp).  Jobs are those fer_seam_host.h has passed.
#pragma once
#include "fer_levels.h"
#include "fer_seam_host.h"
#include <algorithm>
#include <string.h>
#include <vector>

#define SEAM_P_SKIP 31  // FER_P_SKIP of fer_dev.h
#define SEAM_MBW (FERHIP_NB_W / 16)
#define SEAM_YSZ (FERHIP_NB_W * FERHIP_NB_H)  // the picture of a job: Y of ferhip_intra_job; Cb and Cr hold a quarter each
#define SEAM_PER_MB true
#define SEAM_PER_STREAM false

// X(FerDev member, element type, one record per MB or per STREAM, elements of a record).  The one place a stride is
// written: the host vectors, the device buffers, the copies and the per-stream offsets all walk this table.
#define SEAM_ARRAYS(X)                                 \
    X(mb_type, int, MB, 1)                             \
    X(cbp, uint8_t, MB, 2)                             \
    X(tc, uint8_t, MB, 24)                             \
    X(i4mode, uint8_t, MB, 16)                         \
    X(i4flag, uint8_t, MB, 16)                         \
    X(chroma_mode, uint8_t, MB, 1)                     \
    X(levels, int16_t, MB, FER_LEVELS)                 \
    X(mbsize, int, MB, 2)                              \
    X(dec_qp, uint8_t, MB, 1)                          \
    X(mv, short, MB, 8)                                \
    X(qp, int, STREAM, 1)                              \
    X(hdr, uint32_t, STREAM, 4)                        \
    X(dec_state, int, STREAM, 4)                       \
    X(curY, uint8_t, STREAM, SEAM_YSZ)                 \
    X(curCb, uint8_t, STREAM, SEAM_YSZ / 4)            \
    X(curCr, uint8_t, STREAM, SEAM_YSZ / 4)

enum SeamArr {
#define X(n, T, per, e) SA_##n,
    SEAM_ARRAYS(X)
#undef X
        SA_COUNT
};
#define SA_BIT(n) (1u << SA_##n)
// elements of array a that one stream of a context of nmb-macroblock pictures holds: stream s0 begins s0 times as many in
static inline size_t seam_stride(int a, int nmb)
{
#define X(n, T, per, e) \
    if (a == SA_##n) return (size_t)(e) * (SEAM_PER_##per ? (size_t)nmb : 1);
    SEAM_ARRAYS(X)
#undef X
    return 0;
}
// f(SA_name, a.name, b.name), or f(SA_name, a.name), for every array of the table, until one returns non-zero
template <typename A, typename B, typename F>
static inline int seam_each(A &a, B &b, F f)
{
#define X(n, T, per, e) \
    if (int rc = f(SA_##n, a.n, b.n)) return rc;
    SEAM_ARRAYS(X)
#undef X
    return 0;
}
template <typename A, typename F>
static inline int seam_each(A &a, F f) { return seam_each(a, a, [&](int i, auto &m, auto &) { return f(i, m); }); }

// The host copies of the arrays in `use` (SA_BIT()s) for S streams, zeroed; the others stay empty.  name_at(i) = record i
// of the array: of macroblock i = s * nmb + m, or of stream i.
struct __attribute__((visibility("hidden"))) SeamHost {
    size_t S;
    int nmb;
#define X(n, T, per, e)                                \
    std::vector<T> n;                                  \
    T *n##_at(size_t i) { return n.data() + i * (e); } \
    const T *n##_at(size_t i) const { return n.data() + i * (e); }
    SEAM_ARRAYS(X)
#undef X
    SeamHost(size_t S_, int nmb_, unsigned use) : S(S_), nmb(nmb_)
    {
        seam_each(*this, [&](int a, auto &v) { return (use >> a & 1) ? (v.assign(S * seam_stride(a, nmb), 0), 0) : 0; });
    }
};

static inline int seam_count_nz(const int32_t *v, int n) { return n - (int)std::count(v, v + n, 0); }

// The public five-array level group (lumaLevel, dc16, ac16, cdc, cac of any job or result struct) and the FER_LEVELS record
// of the device: 16 entries per Intra4x4 / inter luma block, 15 per Intra16x16 AC and chroma AC block; dc16 goes with
// Intra16x16 only (cavlc_residual_mb and k_dec_intra read FER_LV_DC16 of no other macroblock).  lv starts out zero.
template <typename J>
static inline void seam_put_levels(int16_t *lv, const J &job, bool i16)
{
    for (int b = 0; b < 16; b++) {
        for (int k = 0; k < (i16 ? 15 : 16); k++) lv[b * 16 + k] = (int16_t)(i16 ? job.ac16[b][k] : job.lumaLevel[b][k]);
        if (i16) lv[FER_LV_DC16 + b] = (int16_t)job.dc16[b];
    }
    for (int b = 0; b < 8; b++) {
        lv[FER_LV_CDC + b] = (int16_t)job.cdc[b >> 2][b & 3];
        for (int k = 0; k < 15; k++) lv[FER_LV_CAC + b * 15 + k] = (int16_t)job.cac[b >> 2][b & 3][k];
    }
}
template <typename R>
static inline void seam_get_levels(R &res, const int16_t *lv, bool i4)  // (what it does not write stays as it is: zero)
{
    for (int b = 0; b < 16; b++) {
        for (int k = 0; k < (i4 ? 16 : 15); k++) (i4 ? res.lumaLevel : res.ac16)[b][k] = lv[b * 16 + k];
        if (!i4) res.dc16[b] = lv[FER_LV_DC16 + b];
    }
    for (int b = 0; b < 8; b++) {
        res.cdc[b >> 2][b & 3] = lv[FER_LV_CDC + b];
        for (int k = 0; k < 15; k++) res.cac[b >> 2][b & 3][k] = lv[FER_LV_CAC + b * 15 + k];
    }
}

// a neighbour's side information into macroblock mi: its type, cbp and tc, and its Intra4x4 modes where the struct has them
static inline int seam_nb_type(const ferhip_res_nb &N) { return N.p_skip ? SEAM_P_SKIP : 0; }
static inline int seam_nb_type(const ferhip_nb_mb &N) { return N.mb_type; }
static inline void seam_nb_i4mode(SeamHost &, size_t, const ferhip_res_nb &) {}
static inline void seam_nb_i4mode(SeamHost &h, size_t mi, const ferhip_nb_mb &N) { std::copy(N.i4mode, N.i4mode + 16, h.i4mode_at(mi)); }
template <typename NB>
static inline void seam_put_nb(SeamHost &h, size_t mi, const NB &N)
{
    uint8_t *cbp = h.cbp_at(mi), *tc = h.tc_at(mi);
    *h.mb_type_at(mi) = seam_nb_type(N);
    cbp[0] = (uint8_t)N.cbp_luma;
    cbp[1] = (uint8_t)N.cbp_chroma;
    for (int b = 0; b < 16; b++) tc[b] = (uint8_t)N.tc_luma[b];
    for (int b = 0; b < 8; b++) tc[16 + b] = (uint8_t)N.tc_chroma[b >> 2][b & 3];
    seam_nb_i4mode(h, mi, N);
}

// ---- ferhip_residual_mbs, WRITE: job j is stream j of a context of 2x2-macroblock pictures, and its macroblock sits at
// address cur[j] = avail, where exactly the neighbours it states exist: both: address 3 (A = 2, B = 1); A only: 1 (A = 0);
// B only: 2 (B = 0); neither: 0.  A PARSE job leaves its stream zero.
#define SEAM_RES_MBW 2
#define SEAM_RES_NMB 4
static const unsigned SEAM_RES_USE = SA_BIT(mb_type) | SA_BIT(cbp) | SA_BIT(tc) | SA_BIT(levels);
static inline void seam_pack_res_write(SeamHost &h, uint8_t *cur, const ferhip_res_job *jobs)
{
    for (size_t j = 0; j < h.S; j++) {
        const ferhip_res_job &J = jobs[j];
        if (J.op != FERHIP_RES_WRITE) continue;
        const int c = J.avail;
        cur[j] = (uint8_t)c;
        for (int k = 0; k < 2; k++)
            if (J.avail & (1 << k)) seam_put_nb(h, j * SEAM_RES_NMB + (size_t)(k == 0 ? c - 1 : c - SEAM_RES_MBW), J.nb[k]);
        // the macroblock itself: its levels, and its own cbp and tc, which the blocks inside it read -- tc by the rule of
        // k_p_resid / k_intra_mb: the non-zero levels of each block's list (15 entries for Intra16x16 AC and chroma AC)
        const size_t m = j * SEAM_RES_NMB + (size_t)c;
        const bool i16 = J.cls == 1;
        uint8_t *cbp = h.cbp_at(m), *tc = h.tc_at(m);
        seam_put_levels(h.levels_at(m), J, i16);
        cbp[0] = (uint8_t)J.cbp_luma;
        cbp[1] = (uint8_t)J.cbp_chroma;
        for (int b = 0; b < 16; b++)  // (0 for a block the CBP leaves out)
            if (J.cbp_luma & (1 << (b >> 2))) tc[b] = (uint8_t)seam_count_nz(i16 ? J.ac16[b] : J.lumaLevel[b], i16 ? 15 : 16);
        for (int b = 0; b < 8; b++)
            if (J.cbp_chroma & 2) tc[16 + b] = (uint8_t)seam_count_nz(J.cac[b >> 2][b & 3], 15);
    }
}

// ---- ferhip_intra_mbs: stream s = job order[s] of a context of 3x2-macroblock pictures, its macroblock at address pos
static const unsigned SEAM_INTRA_USE = (1u << SA_COUNT) - 1 - SA_BIT(mv);
static const unsigned SEAM_INTRA_DOWN = SA_BIT(curY) | SA_BIT(curCb) | SA_BIT(curCr) | SA_BIT(cbp) | SA_BIT(tc) | SA_BIT(i4mode) | SA_BIT(i4flag) |
                                        SA_BIT(chroma_mode) | SA_BIT(mb_type) | SA_BIT(mbsize) | SA_BIT(levels);
static_assert(sizeof(ferhip_intra_job::Y) == SEAM_YSZ && sizeof(ferhip_intra_job::Cb) == SEAM_YSZ / 4, "the table's pictures are the job's");

// The jobs of one (op, pos) side by side, so that a launch covers a range of streams: order = the jobs sorted by
// (op, pos), stably; run[r] .. run[r + 1] - 1 = the streams of the r-th (op, pos) present, the last entry of run = n.
struct __attribute__((visibility("hidden"))) SeamOrder {
    std::vector<uint32_t> order;
    std::vector<size_t> run;
};
static inline SeamOrder seam_intra_order(const ferhip_intra_job *jobs, size_t n)
{
    SeamOrder o{std::vector<uint32_t>(n), {}};
    for (size_t j = 0; j < n; j++) o.order[j] = (uint32_t)j;
    auto key = [&](uint32_t j) { return jobs[j].op * FERHIP_NB_MBS + jobs[j].pos; };
    std::stable_sort(o.order.begin(), o.order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    for (size_t s = 0; s < n; s++)
        if (s == 0 || key(o.order[s]) != key(o.order[s - 1])) o.run.push_back(s);
    o.run.push_back(n);
    return o;
}

// chroma_qp = qPiToQPc for chroma_qp_index_offset 0, the encoder's (ferhip_chroma_qp)
static inline void seam_pack_intra(SeamHost &h, uint8_t *pos, const ferhip_intra_job *jobs, const uint32_t *order, int (*chroma_qp)(int))
{
    const int NM = FERHIP_NB_MBS;
    for (size_t s = 0; s < h.S; s++) {
        const ferhip_intra_job &J = jobs[order[s]];
        const bool dec = J.op == FERHIP_INTRA_DECODE;
        memcpy(h.curY_at(s), J.Y, sizeof J.Y);
        memcpy(h.curCb_at(s), J.Cb, sizeof J.Cb);
        memcpy(h.curCr_at(s), J.Cr, sizeof J.Cr);
        pos[s] = (uint8_t)J.pos;
        *h.qp_at(s) = J.qp | (chroma_qp(J.qp) << 8);
        uint32_t *hdr = h.hdr_at(s);
        hdr[0] = (uint32_t)J.chroma_qp_offset;
        hdr[1] = (uint32_t)J.constrained_intra;
        hdr[3] = (uint32_t)J.slice_type;
        h.dec_state_at(s)[1] = NM;  // k_dec_intra: every macroblock was reached by the parser
        for (int m = 0; m < NM; m++) {
            const size_t mi = s * NM + m;
            *h.dec_qp_at(mi) = (uint8_t)J.qp;
            if (m > J.pos) *h.mb_type_at(mi) = dec ? SEAM_P_SKIP : 0;
            if (m < J.pos) seam_put_nb(h, mi, J.mb[m]);
        }
        if (dec && J.pos == 3) *h.mb_type_at(s * NM + 2) = SEAM_P_SKIP;  // shares the diagonal of pos 3 and is none of its neighbours
        const size_t mi = s * NM + J.pos;
        *h.mb_type_at(mi) = J.mb[J.pos].mb_type;
        if (!dec) continue;
        *h.chroma_mode_at(mi) = (uint8_t)J.chroma_mode;
        for (int b = 0; b < 16; b++) h.i4flag_at(mi)[b] = (uint8_t)((J.prev_flag[b] << 3) | J.rem_mode[b]);
        seam_put_levels(h.levels_at(mi), J, fer_seam_is_i16(J.mb[J.pos].mb_type, J.slice_type));
    }
}

// the arrays as the kernels left them (SEAM_INTRA_DOWN) and pred[S][384] of k_seam_intra_pred into results[order[s]]
static inline void seam_unpack_intra(ferhip_intra_result *results, const SeamHost &h, const int32_t *pred, const ferhip_intra_job *jobs,
                                     const uint32_t *order)
{
    for (size_t s = 0; s < h.S; s++) {
        const ferhip_intra_job &J = jobs[order[s]];
        ferhip_intra_result &R = results[order[s]];
        memset(&R, 0, sizeof R);
        const bool enc = J.op == FERHIP_INTRA_ENCODE;
        const size_t mi = s * FERHIP_NB_MBS + J.pos;
        const int t = *h.mb_type_at(mi);
        const bool i4 = fer_seam_is_i4(t, J.slice_type);
        R.mb_type = t;
        R.ret = i4 ? -1 : ((J.slice_type == 2 ? t : t - 5) - 1) & 3;
        R.chroma_mode = *h.chroma_mode_at(mi);
        for (int b = 0; b < 16; b++) R.i4mode[b] = (enc || i4) ? h.i4mode_at(mi)[b] : 0;
        const int xp = (J.pos % SEAM_MBW) << 4, yp = (J.pos / SEAM_MBW) << 4;
        for (int i = 0; i < 256; i++) R.recY[i] = h.curY_at(s)[(size_t)(yp + (i >> 4)) * FERHIP_NB_W + xp + (i & 15)];
        for (int i = 0; i < 64; i++) {
            const size_t o = (size_t)(yp / 2 + (i >> 3)) * (FERHIP_NB_W / 2) + xp / 2 + (i & 7);
            R.recCb[i] = h.curCb_at(s)[o];
            R.recCr[i] = h.curCr_at(s)[o];
        }
        memcpy(R.predL, pred + s * 384, sizeof R.predL);
        memcpy(R.predCb, pred + s * 384 + 256, sizeof R.predCb);
        memcpy(R.predCr, pred + s * 384 + 320, sizeof R.predCr);
        if (!enc) continue;
        const uint8_t *cbp = h.cbp_at(mi), *tc = h.tc_at(mi), *i4f = h.i4flag_at(mi);
        R.cbp_luma = cbp[0];
        R.cbp_chroma = cbp[1];
        R.mbsize[0] = h.mbsize_at(mi)[0];
        R.mbsize[1] = h.mbsize_at(mi)[1];
        for (int b = 0; b < 16; b++) {  // as the macroblock layer reads them (k_cavlc): bit 3 = the flag, bits 0..2 = rem
            R.prev_flag[b] = (i4f[b] >> 3) & 1;
            R.rem_mode[b] = i4f[b] & 7;
            R.tc_luma[b] = tc[b];
        }
        for (int b = 0; b < 8; b++) R.tc_chroma[b >> 2][b & 3] = tc[16 + b];
        seam_get_levels(R, h.levels_at(mi), i4);
    }
}
