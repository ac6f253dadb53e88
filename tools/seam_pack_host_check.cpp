// The host packer of the per-macroblock seam (h264-fer_amd/csrc/fer_seam_pack_host.h: the table of side-information
// arrays, the level record, the neighbour copy, the packing of ferhip_residual_mbs and ferhip_intra_mbs jobs, the job order)
// as a stand-alone program, for a run under a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/seam_pack_host_check.cpp -o seam_pack_host_check && ./seam_pack_host_check
// Every vector is on the heap and exactly as long as the table says, so a stride that disagrees anywhere is an error the
// sanitizer reports.  The expected values are written here with the literal strides of the device code (2, 24, 16, 400,
// 256 / 272 / 280, 4, 48 * 32), never through the table.
#include "../h264-fer_amd/csrc/fer_seam_pack_host.h"
#include "../include/ferhip.h"
#include <stdio.h>
#include <memory>

static int fails = 0;
#define EXPECT(x)                                  \
    do {                                           \
        if (!(x)) {                                \
            printf("line %d: %s\n", __LINE__, #x); \
            fails++;                               \
        }                                          \
    } while (0)

static uint32_t rng = 12345;
static int rnd(int lo, int hi)
{
    rng = rng * 1664525u + 1013904223u;
    return lo + (int)((rng >> 8) % (uint32_t)(hi - lo + 1));
}
static int level() { return rnd(0, 9) == 0 ? (rnd(0, 1) ? 32767 : -32768) : rnd(-2, 2); }  // zeros, small ones, both ends of int16_t
static int chroma_qp(int qp) { return qp < 30 ? qp : 29 + (qp - 30) / 3; }                  // stands in for ferhip_chroma_qp
static const unsigned ALL = (1u << SA_COUNT) - 1;

template <typename T>
static bool same(const char *what, const std::vector<T> &got, const std::vector<T> &want)
{
    if (got.size() != want.size()) return printf("%s: %zu entries, expected %zu\n", what, got.size(), want.size()), false;
    for (size_t i = 0; i < got.size(); i++)
        if (got[i] != want[i]) return printf("%s[%zu] = %d, expected %d\n", what, i, (int)got[i], (int)want[i]), false;
    return true;
}

static void strides()
{
    static const struct {
        int a;
        size_t per;
        bool mb;
    } want[] = {{SA_mb_type, 1, true}, {SA_cbp, 2, true},       {SA_tc, 24, true},       {SA_i4mode, 16, true},    {SA_i4flag, 16, true},      {SA_chroma_mode, 1, true},
                {SA_levels, 400, true}, {SA_mbsize, 2, true},   {SA_dec_qp, 1, true},    {SA_mv, 8, true},         {SA_qp, 1, false},          {SA_hdr, 4, false},
                {SA_dec_state, 4, false}, {SA_curY, 48 * 32, false}, {SA_curCb, 24 * 16, false}, {SA_curCr, 24 * 16, false}};
    EXPECT(sizeof want / sizeof want[0] == SA_COUNT);
    for (const auto &w : want)
        for (int nmb : {1, 4, 6}) EXPECT(seam_stride(w.a, nmb) == w.per * (w.mb ? (size_t)nmb : 1));
    EXPECT(FER_LEVELS == 400 && FER_LV_DC16 == 256 && FER_LV_CDC == 272 && FER_LV_CAC == 280);
    SeamHost h(3, 6, ALL);
#define AT(name, per) EXPECT(h.name##_at(2) == h.name.data() + 2 * (per));
    AT(mb_type, 1) AT(cbp, 2) AT(tc, 24) AT(i4mode, 16) AT(i4flag, 16) AT(chroma_mode, 1) AT(levels, 400) AT(mbsize, 2)
    AT(dec_qp, 1) AT(mv, 8) AT(qp, 1) AT(hdr, 4) AT(dec_state, 4) AT(curY, 1536) AT(curCb, 384) AT(curCr, 384)
#undef AT
    EXPECT(sizeof h.mb_type[0] == 4 && sizeof h.levels[0] == 2 && sizeof h.mv[0] == 2 && sizeof h.hdr[0] == 4 && sizeof h.tc[0] == 1);
    SeamHost part(3, 4, SEAM_RES_USE);  // only what is asked for
    EXPECT(part.mb_type.size() == 12 && part.cbp.size() == 24 && part.tc.size() == 288 && part.levels.size() == 4800);
    EXPECT(part.mv.empty() && part.curY.empty() && part.i4mode.empty() && part.qp.empty() && part.hdr.empty());
}

// the streams s0 .. s0 + cnt - 1 of every array lie inside it (the first and the last entry of the range are written)
static void offsets()
{
    for (size_t n : {1, 2, 7})
        for (int nmb : {4, 6}) {
            SeamHost h(n, nmb, ALL);
            seam_each(h, [&](int a, auto &v) {
                const size_t st = seam_stride(a, nmb);
                EXPECT(st > 0 && v.size() == n * st);
                for (size_t s0 = 0; s0 < n; s0++)
                    for (size_t cnt = 1; s0 + cnt <= n; cnt++) {
                        auto *p = v.data() + s0 * st;
                        EXPECT(s0 * st + cnt * st <= v.size());
                        p[0] = 1, p[cnt * st - 1] = 1;
                    }
                return 0;
            });
        }
}

template <typename T>
static void fill_levels(T &x)
{
    for (int i = 0; i < 256; i++) (&x.lumaLevel[0][0])[i] = level(), (&x.ac16[0][0])[i] = level();
    for (int i = 0; i < 16; i++) x.dc16[i] = level();
    for (int i = 0; i < 8; i++) (&x.cdc[0][0])[i] = level();
    for (int i = 0; i < 128; i++) (&x.cac[0][0][0])[i] = level();
    x.lumaLevel[0][0] = x.ac16[15][14] = x.dc16[15] = x.cdc[1][3] = x.cac[1][3][14] = 32767;
    x.lumaLevel[15][15] = x.ac16[0][0] = x.dc16[0] = x.cdc[0][0] = x.cac[0][0][0] = -32768;
}
// the record of one macroblock by the literal layout: 16 x 16 luma, 16 DC at 256, 8 chroma DC at 272, 8 x 15 chroma AC at 280
template <typename T>
static std::vector<int16_t> want_levels(const T &x, bool i16)
{
    std::vector<int16_t> lv(400, 0);
    for (int b = 0; b < 16; b++) {
        for (int k = 0; k < (i16 ? 15 : 16); k++) lv[b * 16 + k] = (int16_t)(i16 ? x.ac16[b][k] : x.lumaLevel[b][k]);
        if (i16) lv[256 + b] = (int16_t)x.dc16[b];
    }
    for (int b = 0; b < 8; b++) {
        lv[272 + b] = (int16_t)x.cdc[b / 4][b % 4];
        for (int k = 0; k < 15; k++) lv[280 + b * 15 + k] = (int16_t)x.cac[b / 4][b % 4][k];
    }
    return lv;
}
template <typename J, typename R>
static void round_trip()
{
    std::unique_ptr<J> job(new J());
    std::unique_ptr<R> res(new R());
    fill_levels(*job);
    for (bool i16 : {false, true}) {
        std::vector<int16_t> lv(FER_LEVELS, 0);
        seam_put_levels(lv.data(), *job, i16);
        EXPECT(same("levels", lv, want_levels(*job, i16)));
        EXPECT(lv[399] == 32767 && lv[280] == -32768 && lv[272] == -32768 && lv[279] == 32767);  // by hand: the ends fill_levels sets
        EXPECT(lv[0] == (i16 ? -32768 : 32767) && lv[254] == (i16 ? 32767 : job->lumaLevel[15][14]) && lv[255] == (i16 ? 0 : -32768));
        EXPECT(lv[256] == (i16 ? -32768 : 0) && lv[271] == (i16 ? 32767 : 0));
        *res = R();
        seam_get_levels(*res, lv.data(), !i16);
        for (int b = 0; b < 16; b++) {
            for (int k = 0; k < 16; k++) {
                EXPECT(res->lumaLevel[b][k] == (i16 ? 0 : job->lumaLevel[b][k]));
                EXPECT(res->ac16[b][k] == (i16 && k < 15 ? job->ac16[b][k] : 0));
            }
            EXPECT(res->dc16[b] == (i16 ? job->dc16[b] : 0));
        }
        for (int b = 0; b < 8; b++) {
            EXPECT(res->cdc[b / 4][b % 4] == job->cdc[b / 4][b % 4]);
            for (int k = 0; k < 16; k++) EXPECT(res->cac[b / 4][b % 4][k] == (k < 15 ? job->cac[b / 4][b % 4][k] : 0));
        }
    }
}

template <typename N>
static void fill_nb(N &nb)
{
    nb.cbp_luma = rnd(0, 15), nb.cbp_chroma = rnd(0, 2);
    for (int b = 0; b < 16; b++) nb.tc_luma[b] = rnd(0, 16);
    for (int b = 0; b < 8; b++) nb.tc_chroma[b / 4][b % 4] = rnd(0, 16);
}
template <typename N>
static void want_nb(const N &nb, int type, size_t m, std::vector<int> &mbt, std::vector<uint8_t> &cbp, std::vector<uint8_t> &tc)
{
    mbt[m] = type;
    cbp[m * 2] = (uint8_t)nb.cbp_luma, cbp[m * 2 + 1] = (uint8_t)nb.cbp_chroma;
    for (int b = 0; b < 16; b++) tc[m * 24 + b] = (uint8_t)nb.tc_luma[b];
    for (int b = 0; b < 8; b++) tc[m * 24 + 16 + b] = (uint8_t)nb.tc_chroma[b / 4][b % 4];
}
static int nonzero(const int32_t *v, int n)
{
    int c = 0;
    for (int i = 0; i < n; i++) c += v[i] != 0;
    return c;
}

// ferhip_residual_mbs: every avail with every class as WRITE jobs, and a PARSE job between them
static void residual()
{
    const size_t n = 13;
    std::unique_ptr<ferhip_res_job[]> J(new ferhip_res_job[n]());
    for (size_t j = 0; j < n; j++) {
        ferhip_res_job &x = J[j];
        x.op = j == 6 ? FERHIP_RES_PARSE : FERHIP_RES_WRITE;
        const size_t w = j - (j > 6);
        x.avail = (int)(w & 3), x.cls = (int)(w >> 2);
        x.cbp_luma = x.cls == 1 ? 15 * rnd(0, 1) : rnd(0, 15), x.cbp_chroma = rnd(0, 2);
        fill_levels(x);
        for (int k = 0; k < 2; k++) fill_nb(x.nb[k]), x.nb[k].p_skip = k == 0;  // (of an absent neighbour nothing is looked at)
    }
    SeamHost h(n, 4, SEAM_RES_USE);
    std::vector<uint8_t> cur(n, 0);
    seam_pack_res_write(h, cur.data(), J.get());
    std::vector<int> mbt(n * 4, 0);
    std::vector<uint8_t> cbp(n * 8, 0), tc(n * 96, 0);
    std::vector<int16_t> lev(n * 1600, 0);
    static const int A[4] = {-1, 0, -1, 2}, B[4] = {-1, -1, 0, 1};  // the addresses of the neighbours of address avail in a 2x2 picture
    for (size_t j = 0; j < n; j++) {
        const ferhip_res_job &x = J[j];
        if (x.op != FERHIP_RES_WRITE) {
            EXPECT(cur[j] == 0);
            continue;
        }
        EXPECT(cur[j] == x.avail);
        if (A[x.avail] >= 0) want_nb(x.nb[0], 31, j * 4 + A[x.avail], mbt, cbp, tc);  // A is a P_Skip, B is not
        if (B[x.avail] >= 0) want_nb(x.nb[1], 0, j * 4 + B[x.avail], mbt, cbp, tc);
        const size_t m = j * 4 + x.avail;
        const bool i16 = x.cls == 1;
        cbp[m * 2] = (uint8_t)x.cbp_luma, cbp[m * 2 + 1] = (uint8_t)x.cbp_chroma;
        const std::vector<int16_t> lv = want_levels(x, i16);
        std::copy(lv.begin(), lv.end(), lev.begin() + m * 400);
        for (int b = 0; b < 16; b++)
            if (x.cbp_luma & (1 << (b / 4))) tc[m * 24 + b] = (uint8_t)nonzero(i16 ? x.ac16[b] : x.lumaLevel[b], i16 ? 15 : 16);
        for (int b = 0; b < 8; b++)
            if (x.cbp_chroma & 2) tc[m * 24 + 16 + b] = (uint8_t)nonzero(x.cac[b / 4][b % 4], 15);
    }
    EXPECT(same("mb_type", h.mb_type, mbt) && same("cbp", h.cbp, cbp) && same("tc", h.tc, tc) && same("levels", h.levels, lev));
    // by hand: the type rows of the first four jobs (avail 0..3; A = P_Skip at 0, 0, -, 2), and the PARSE job's stream
    const int rows[4][4] = {{0, 0, 0, 0}, {31, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 31, 0}};
    for (int j = 0; j < 4; j++)
        for (int m = 0; m < 4; m++) EXPECT(h.mb_type[j * 4 + m] == rows[j][m]);
    for (int i = 0; i < 1600; i++) EXPECT(h.levels[6 * 1600 + i] == 0);
    EXPECT(seam_count_nz(J[0].dc16, 16) == nonzero(J[0].dc16, 16) && seam_count_nz(J[0].dc16, 0) == 0);
}

static void order()
{
    const size_t n = 40;
    std::unique_ptr<ferhip_intra_job[]> J(new ferhip_intra_job[n]());
    for (size_t j = 0; j < n; j++) J[j].op = rnd(0, 1), J[j].pos = rnd(0, 5);
    for (size_t cnt : {(size_t)1, n}) {
        const SeamOrder o = seam_intra_order(J.get(), cnt);
        std::vector<int> seen(cnt, 0);
        EXPECT(o.order.size() == cnt && o.run.size() >= 2 && o.run.front() == 0 && o.run.back() == cnt);
        for (uint32_t j : o.order) EXPECT(j < cnt && !seen[j]++);  // a permutation
        for (size_t r = 0; r + 1 < o.run.size(); r++) {            // the runs partition [0, n): each one (op, pos), in rising order
            EXPECT(o.run[r] < o.run[r + 1]);
            const ferhip_intra_job &F = J[o.order[o.run[r]]];
            for (size_t s = o.run[r]; s < o.run[r + 1]; s++) {
                EXPECT(J[o.order[s]].op == F.op && J[o.order[s]].pos == F.pos);
                if (s > o.run[r]) EXPECT(o.order[s - 1] < o.order[s]);  // stable
            }
            if (r) {
                const ferhip_intra_job &P = J[o.order[o.run[r] - 1]];
                EXPECT(P.op * 6 + P.pos < F.op * 6 + F.pos);
            }
        }
    }
}

// ferhip_intra_mbs: every pos under both ops, twice, submitted in descending pos with the ops alternating
static void intra()
{
    const size_t n = 24;
    std::unique_ptr<ferhip_intra_job[]> J(new ferhip_intra_job[n]());
    for (size_t j = 0; j < n; j++) {
        ferhip_intra_job &x = J[j];
        x.op = (int)(j & 1), x.pos = 5 - (int)(j / 2 % 6);
        const bool dec = x.op == FERHIP_INTRA_DECODE;
        x.slice_type = dec && j < 12 ? 0 : 2;
        x.qp = rnd(0, 51), x.chroma_qp_offset = rnd(-12, 12), x.constrained_intra = rnd(0, 1), x.chroma_mode = rnd(0, 3);
        for (int b = 0; b < 16; b++) x.prev_flag[b] = rnd(0, 1), x.rem_mode[b] = rnd(0, 7);
        for (int m = 0; m < 6; m++) {
            ferhip_nb_mb &N = x.mb[m];
            fill_nb(N);
            N.mb_type = 10 + m;  // Intra16x16 under either numbering
            for (int b = 0; b < 16; b++) N.i4mode[b] = rnd(0, 8);
        }
        x.mb[x.pos].mb_type = !dec ? 31 : (j % 4 == 1 ? (x.slice_type == 2 ? 0 : 5) : 20);  // stale P_Skip; Intra4x4 or Intra16x16
        for (size_t i = 0; i < sizeof x.Y; i++) (&x.Y[0][0])[i] = (uint8_t)rnd(0, 255);
        for (size_t i = 0; i < sizeof x.Cb; i++) (&x.Cb[0][0])[i] = (uint8_t)rnd(0, 255), (&x.Cr[0][0])[i] = (uint8_t)rnd(0, 255);
        fill_levels(x);
    }
    const SeamOrder o = seam_intra_order(J.get(), n);
    EXPECT(o.run.size() == 13);
    SeamHost h(n, 6, SEAM_INTRA_USE);
    std::vector<uint8_t> pos(n, 0xee);
    seam_pack_intra(h, pos.data(), J.get(), o.order.data(), chroma_qp);
    std::vector<uint8_t> Y(n * 1536), Cb(n * 384), Cr(n * 384), cbp(n * 12, 0), tc(n * 144, 0), i4m(n * 96, 0), i4f(n * 96, 0), cmode(n * 6, 0), dqp(n * 6, 0);
    std::vector<int> mbt(n * 6, 0), qp(n), dst(n * 4, 0), mbsz(n * 12, 0);
    std::vector<uint32_t> hdr(n * 4, 0);
    std::vector<int16_t> lev(n * 2400, 0);
    for (size_t s = 0; s < n; s++) {
        const ferhip_intra_job &x = J[o.order[s]];
        const bool dec = x.op == FERHIP_INTRA_DECODE;
        EXPECT(pos[s] == x.pos && (s < 12) == !dec && x.pos == (int)(s / 2 % 6));  // stream s = job order[s]: ENCODE first, pos rising
        memcpy(&Y[s * 1536], x.Y, 1536), memcpy(&Cb[s * 384], x.Cb, 384), memcpy(&Cr[s * 384], x.Cr, 384);
        qp[s] = x.qp | chroma_qp(x.qp) << 8;
        hdr[s * 4] = (uint32_t)x.chroma_qp_offset, hdr[s * 4 + 1] = (uint32_t)x.constrained_intra, hdr[s * 4 + 3] = (uint32_t)x.slice_type;
        dst[s * 4 + 1] = 6;  // dec_state[1] = nmb
        for (int m = 0; m < 6; m++) {
            const size_t mi = s * 6 + m;
            dqp[mi] = (uint8_t)x.qp;
            if (m < x.pos) {  // the macroblocks in front of pos: as the job states them
                want_nb(x.mb[m], 10 + m, mi, mbt, cbp, tc);
                for (int b = 0; b < 16; b++) i4m[mi * 16 + b] = (uint8_t)x.mb[m].i4mode[b];
            } else if (m == x.pos) {
                mbt[mi] = x.mb[m].mb_type;
            } else {
                mbt[mi] = dec ? 31 : 0;  // P_Skip for m > pos in DECODE
            }
        }
        if (dec && x.pos == 3) mbt[s * 6 + 2] = 31;  // macroblock 2 shares the diagonal of pos 3
        if (!dec) continue;
        const size_t mi = s * 6 + x.pos;
        cmode[mi] = (uint8_t)x.chroma_mode;
        for (int b = 0; b < 16; b++) i4f[mi * 16 + b] = (uint8_t)(x.prev_flag[b] * 8 + x.rem_mode[b]);
        const std::vector<int16_t> lv = want_levels(x, x.mb[x.pos].mb_type == 20);
        std::copy(lv.begin(), lv.end(), lev.begin() + mi * 400);
    }
    EXPECT(same("Y", h.curY, Y) && same("Cb", h.curCb, Cb) && same("Cr", h.curCr, Cr) && same("cbp", h.cbp, cbp) && same("tc", h.tc, tc));
    EXPECT(same("i4mode", h.i4mode, i4m) && same("i4flag", h.i4flag, i4f) && same("chroma_mode", h.chroma_mode, cmode) && same("dec_qp", h.dec_qp, dqp));
    EXPECT(same("mb_type", h.mb_type, mbt) && same("qp", h.qp, qp) && same("dec_state", h.dec_state, dst) && same("mbsize", h.mbsize, mbsz));
    EXPECT(same("hdr", h.hdr, hdr) && same("levels", h.levels, lev) && h.mv.empty());
    // by hand: the type rows of ENCODE at pos 2 and 5 (streams 4 and 10) and of DECODE at pos 0 and 3 (streams 12 and 18)
    const int rows[4][7] = {{4, 10, 11, 31, 0, 0, 0}, {10, 10, 11, 12, 13, 14, 31}, {12, -1, 31, 31, 31, 31, 31}, {18, 10, 11, 31, -1, 31, 31}};
    for (const auto &r : rows)
        for (int m = 0; m < 6; m++) EXPECT(r[m + 1] < 0 || h.mb_type[r[0] * 6 + m] == r[m + 1]);  // (-1: the job's own type)

    // the way back: what the kernels leave in the arrays, scattered to results[order[s]]
    std::unique_ptr<ferhip_intra_result[]> R(new ferhip_intra_result[n]);
    std::vector<int32_t> pred(n * 384);
    for (auto &v : pred) v = rnd(0, 255);
    for (auto &v : h.mbsize) v = rnd(0, 4000);
    for (auto &v : h.i4flag) v = (uint8_t)rnd(0, 15);
    for (size_t s = 0; s < 12; s++) h.mb_type[s * 6 + s / 2] = s & 1 ? 0 : 3;  // ENCODE decided: Intra4x4, or Intra16x16 of mode 2
    seam_unpack_intra(R.get(), h, pred.data(), J.get(), o.order.data());
    for (size_t s = 0; s < n; s++) {
        const ferhip_intra_job &x = J[o.order[s]];
        const ferhip_intra_result &r = R[o.order[s]];
        const size_t mi = s * 6 + x.pos;
        const bool enc = s < 12, i4 = enc ? (s & 1) : x.mb[x.pos].mb_type != 20;
        EXPECT(r.mb_type == h.mb_type[mi] && r.chroma_mode == h.chroma_mode[mi]);
        EXPECT(r.ret == (i4 ? -1 : enc ? 2 : x.slice_type == 2 ? 3 : 2));  // (3 - 1) & 3; type 20: (20 - 1) & 3 in an I, (20 - 5 - 1) & 3 in a P slice
        const int xp = x.pos % 3 * 16, yp = x.pos / 3 * 16;
        for (int i = 0; i < 256; i++) EXPECT(r.recY[i] == h.curY[s * 1536 + (yp + i / 16) * 48 + xp + i % 16] && r.predL[i] == pred[s * 384 + i]);
        for (int i = 0; i < 64; i++) {
            const size_t c = s * 384 + (yp / 2 + i / 8) * 24 + xp / 2 + i % 8;
            EXPECT(r.recCb[i] == h.curCb[c] && r.recCr[i] == h.curCr[c] && r.predCb[i] == pred[s * 384 + 256 + i] && r.predCr[i] == pred[s * 384 + 320 + i]);
        }
        for (int b = 0; b < 16; b++) {
            EXPECT(r.i4mode[b] == (enc || i4 ? h.i4mode[mi * 16 + b] : 0));
            EXPECT(r.prev_flag[b] == (enc ? h.i4flag[mi * 16 + b] >> 3 : 0) && r.rem_mode[b] == (enc ? h.i4flag[mi * 16 + b] & 7 : 0));
            EXPECT(r.tc_luma[b] == (enc ? h.tc[mi * 24 + b] : 0));
        }
        for (int b = 0; b < 8; b++) EXPECT(r.tc_chroma[b / 4][b % 4] == (enc ? h.tc[mi * 24 + 16 + b] : 0));
        EXPECT(r.cbp_luma == (enc ? h.cbp[mi * 2] : 0) && r.cbp_chroma == (enc ? h.cbp[mi * 2 + 1] : 0));
        EXPECT(r.mbsize[0] == (enc ? h.mbsize[mi * 2] : 0) && r.mbsize[1] == (enc ? h.mbsize[mi * 2 + 1] : 0));
        ferhip_intra_result lv = {};
        if (enc) seam_get_levels(lv, &h.levels[mi * 400], i4);
        EXPECT(!memcmp(r.lumaLevel, lv.lumaLevel, sizeof lv.lumaLevel) && !memcmp(r.dc16, lv.dc16, sizeof lv.dc16) && !memcmp(r.ac16, lv.ac16, sizeof lv.ac16));
        EXPECT(!memcmp(r.cdc, lv.cdc, sizeof lv.cdc) && !memcmp(r.cac, lv.cac, sizeof lv.cac));
    }
}

int main()
{
    strides();
    offsets();
    round_trip<ferhip_res_job, ferhip_res_result>();
    round_trip<ferhip_intra_job, ferhip_intra_result>();
    round_trip<ferhip_intra_job, ferhip_mb_job>();  // (the level group of ferhip_mb_job and ferhip_mb_result is the same)
    residual();
    order();
    intra();
    printf(fails ? "%d checks failed\n" : "seam_pack_host_check ok\n", fails);
    return fails != 0;
}
