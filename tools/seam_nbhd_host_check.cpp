// Argument checks of the neighbourhood seam (ferhip_intra_mbs, ferhip_mv_mbs; h264-fer_amd/csrc/fer_seam_host.h) as a
// stand-alone program, for a run under a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/seam_nbhd_host_check.cpp -o seam_nbhd_host_check && ./seam_nbhd_host_check
// The job and result arrays are exactly as long as the call says, on the heap: a check that reads past what it was given is
// an error.  It goes through every refusal of the two entry points and through good calls at the edges of every range.
#include "../h264-fer_amd/csrc/fer_seam_host.h"
#include <stdio.h>
#include <initializer_list>
#include <memory>

static int fails = 0;
#define EXPECT(x)                                  \
    do {                                           \
        if (!(x)) {                                \
            printf("line %d: %s\n", __LINE__, #x); \
            fails++;                               \
        }                                          \
    } while (0)
#define BAD(x) EXPECT((x) == FERHIP_E_ARG)
#define GOOD(x) EXPECT((x) == 0)

static void nb(ferhip_nb_mb &N, int32_t t, int32_t vx = 32767, int32_t vy = -32768)  // at the top of every range
{
    N.mb_type = t;
    N.cbp_luma = 15;
    N.cbp_chroma = 2;
    for (int b = 0; b < 16; b++) N.tc_luma[b] = 16, N.i4mode[b] = 8;
    for (int b = 0; b < 8; b++) N.tc_chroma[b >> 2][b & 3] = 16;
    for (int q = 0; q < 4; q++) N.mv[q][0] = vx, N.mv[q][1] = vy;
}
static void garbage(ferhip_nb_mb &N)  // an entry nothing may look at
{
    N.mb_type = 99;
    N.cbp_luma = -1;
    N.tc_luma[3] = 99;
    N.i4mode[0] = -3;
    N.mv[0][0] = 1 << 20;
}
template <typename F>
static void sweep(F call, int32_t &v, int32_t lo, int32_t hi)
{
    const int32_t keep = v;
    for (int32_t x : {lo - 1, hi + 1, INT32_MIN, INT32_MAX}) {
        v = x;
        BAD(call());
    }
    for (int32_t x : {lo, hi}) {
        v = x;
        GOOD(call());
    }
    v = keep;
}

static void intra()
{
    const size_t n = 3;
    std::unique_ptr<ferhip_intra_job[]> J(new ferhip_intra_job[n]());
    std::unique_ptr<ferhip_intra_result[]> R(new ferhip_intra_result[n]());
    auto call = [&]() { return fer_seam_check_intra_mbs(J.get(), R.get(), n); };
    // 0: ENCODE at pos 0 (no entry but the stale type is looked at); 1: ENCODE at pos 5; 2: DECODE, P slice, Intra4x4 at pos 4
    J[0].slice_type = 2, J[0].mb[0].mb_type = 31;
    for (int m = 1; m < 6; m++) garbage(J[0].mb[m]);
    J[1].pos = 5, J[1].slice_type = 2, J[1].qp = 51;
    nb(J[1].mb[0], 24), nb(J[1].mb[1], 0), nb(J[1].mb[2], 31), nb(J[1].mb[3], 1), nb(J[1].mb[4], 12);
    J[1].mb[5].mb_type = 24;
    ferhip_intra_job &D = J[2];
    D.op = FERHIP_INTRA_DECODE, D.pos = 4, D.slice_type = 0, D.qp = 51, D.chroma_qp_offset = -12, D.chroma_mode = 3;
    nb(D.mb[0], 4), nb(D.mb[1], 5), nb(D.mb[2], 29), nb(D.mb[3], 31);
    D.mb[4].mb_type = 5;
    garbage(D.mb[5]);
    for (int b = 0; b < 16; b++) D.prev_flag[b] = 1, D.rem_mode[b] = 7;
    D.lumaLevel[15][15] = 32767, D.cac[1][3][15] = -32768;
    GOOD(call());
    BAD(fer_seam_check_intra_mbs(nullptr, R.get(), n));
    BAD(fer_seam_check_intra_mbs(J.get(), nullptr, n));
    BAD(fer_seam_check_intra_mbs(J.get(), R.get(), 0));
    BAD(fer_seam_check_intra_mbs(J.get(), R.get(), FER_SEAM_JOBS_MAX + 1));  // (refused before any job is read)
    sweep(call, J[1].qp, 0, 51);
    sweep(call, J[1].chroma_qp_offset, -12, 12);
    sweep(call, J[1].constrained_intra, 0, 1);
    sweep(call, D.qp, 0, 51);
    sweep(call, D.chroma_mode, 0, 3);
    for (int32_t v : {-1, 2, INT32_MIN, INT32_MAX}) {
        J[0].op = v;
        BAD(call());
    }
    J[0].op = 0;
    for (int32_t v : {-1, 6, INT32_MIN, INT32_MAX}) {  // (a pos out of range must not index mb[])
        J[1].pos = v;
        BAD(call());
        D.pos = v;
        BAD(call());
        D.pos = 4;
    }
    J[1].pos = 5;
    for (int32_t v : {1, 3, 7, -1, INT32_MAX}) {
        D.slice_type = v;
        BAD(call());
    }
    D.slice_type = 0;
    J[1].slice_type = 0;  // ENCODE is for I slices
    BAD(call());
    J[1].slice_type = 2;
    for (int32_t v : {25, 30, 32, -1}) {
        J[1].mb[5].mb_type = v;  // the stale entry
        BAD(call());
        J[1].mb[5].mb_type = 24;
        J[1].mb[2].mb_type = v;  // a neighbour, I slice
        BAD(call());
        J[1].mb[2].mb_type = 31;
    }
    for (int32_t v : {30, 32, -1, INT32_MAX}) {
        D.mb[1].mb_type = v;  // a neighbour, P slice
        BAD(call());
    }
    D.mb[1].mb_type = 5;
    for (int32_t v : {0, 4, 31, 30}) {
        D.mb[4].mb_type = v;  // DECODE: the macroblock is intra
        BAD(call());
    }
    D.mb[4].mb_type = 5;
    ferhip_nb_mb &N = D.mb[3];
    sweep(call, N.cbp_luma, 0, 15);
    sweep(call, N.cbp_chroma, 0, 2);
    sweep(call, N.tc_luma[0], 0, 16);
    sweep(call, N.tc_luma[15], 0, 16);
    sweep(call, N.tc_chroma[0][0], 0, 16);
    sweep(call, N.tc_chroma[1][3], 0, 16);
    sweep(call, N.i4mode[0], 0, 8);
    sweep(call, N.i4mode[15], 0, 8);
    sweep(call, N.mv[0][0], -32768, 32767);
    sweep(call, N.mv[3][1], -32768, 32767);
    sweep(call, D.prev_flag[0], 0, 1);
    sweep(call, D.prev_flag[15], 0, 1);
    D.prev_flag[6] = 0;  // (block 6 lies inside the macroblock: every mode has its samples)
    sweep(call, D.rem_mode[6], 0, 7);
    D.prev_flag[6] = 1;
    int32_t *const lv[] = {&D.lumaLevel[0][0], &D.lumaLevel[15][15], &D.dc16[0], &D.dc16[15], &D.ac16[0][0], &D.ac16[15][15], &D.cdc[0][0], &D.cdc[1][3],
                           &D.cac[0][0][0], &D.cac[1][3][15]};
    for (int32_t *p : lv) sweep(call, *p, -32768, 32767);
    // jobs that are not legal
    D.pos = 3, D.mb[3].mb_type = 5;  // B and C, no A: the plane chroma mode reads the column to the left
    BAD(call());
    D.chroma_mode = 1;
    BAD(call());
    D.chroma_mode = 2;
    GOOD(call());
    D.prev_flag[0] = 0, D.rem_mode[0] = 1;  // block 0: horizontal
    BAD(call());
    D.rem_mode[0] = 0;  // vertical: the row above exists
    GOOD(call());
    D.prev_flag[0] = 1;
    D.mb[3].mb_type = 6 + 1;  // Intra16x16 horizontal in a P slice
    BAD(call());
    D.mb[3].mb_type = 6;  // vertical
    GOOD(call());
    D.pos = 0, D.chroma_mode = 0;
    D.mb[0].mb_type = 6;
    BAD(call());
    D.mb[0].mb_type = 6 + 2;  // DC
    GOOD(call());
}

static void mv()
{
    const size_t n = 3;
    std::unique_ptr<ferhip_mv_job[]> J(new ferhip_mv_job[n]());
    std::unique_ptr<ferhip_mv_result[]> R(new ferhip_mv_result[n]());
    auto call = [&]() { return fer_seam_check_mv_mbs(J.get(), R.get(), n); };
    J[0].mb_type = 31;
    for (int m = 0; m < 6; m++) garbage(J[0].mb[m]);
    ferhip_mv_job &A = J[1], &P = J[2];
    A.pos = 5, A.mb_type = 4;
    for (int k = 0; k < 4; k++) A.sub_mb_type[k] = 3, A.mvd[k][0] = FER_SEAM_MVD_MAX, A.mvd[k][1] = -FER_SEAM_MVD_MAX;
    nb(A.mb[0], 0), nb(A.mb[1], 29), nb(A.mb[2], 31), nb(A.mb[3], 3), nb(A.mb[4], 1);
    A.mb[3].mv[2][0] = 77;  // (8x8: any four vectors)
    A.mb[4].mv[2][1] = A.mb[4].mv[3][1] = 5;
    garbage(A.mb[5]);
    P.op = FERHIP_MV_PREDICT, P.pos = 4, P.mb_type = 2;
    P.mv[0][0] = P.mv[2][0] = -32768, P.mv[1][1] = P.mv[3][1] = 32767;
    nb(P.mb[0], 0), nb(P.mb[1], 2), nb(P.mb[2], 31), nb(P.mb[3], 4);
    P.mb[1].mv[1][0] = P.mb[1].mv[3][0] = 9;
    P.mvd[0][0] = 1 << 30;  // (an input of DERIVE only)
    GOOD(call());
    BAD(fer_seam_check_mv_mbs(nullptr, R.get(), n));
    BAD(fer_seam_check_mv_mbs(J.get(), nullptr, n));
    BAD(fer_seam_check_mv_mbs(J.get(), R.get(), 0));
    BAD(fer_seam_check_mv_mbs(J.get(), R.get(), FER_SEAM_JOBS_MAX + 1));
    for (int32_t v : {-1, 2, INT32_MIN, INT32_MAX}) {
        A.op = v;
        BAD(call());
    }
    A.op = 0;
    for (int32_t v : {-1, 6, INT32_MIN, INT32_MAX}) {
        A.pos = v;
        BAD(call());
    }
    A.pos = 5;
    for (int32_t v : {5, 30, 32, -1}) {
        A.mb_type = v;
        BAD(call());
    }
    A.mb_type = 4;
    for (int32_t v : {5, 31, -1}) {
        P.mb_type = v;
        BAD(call());
    }
    P.mb_type = 2;
    sweep(call, A.sub_mb_type[0], 0, 3);
    sweep(call, A.sub_mb_type[3], 0, 3);
    sweep(call, P.sub_mb_type[3], 0, 0);
    sweep(call, A.mvd[0][0], -FER_SEAM_MVD_MAX, FER_SEAM_MVD_MAX);
    sweep(call, A.mvd[3][1], -FER_SEAM_MVD_MAX, FER_SEAM_MVD_MAX);
    sweep(call, A.mb[1].mv[0][0], -32768, 32767);  // (an intra neighbour: its vectors are only held to 16 bits)
    sweep(call, A.mb[3].mv[3][1], -32768, 32767);
    for (int32_t v : {30, 32, -1}) {
        A.mb[2].mb_type = v;
        BAD(call());
    }
    A.mb[2].mb_type = 31;
    int32_t *const one[] = {&A.mb[0].mv[3][1], &A.mb[2].mv[1][1], &A.mb[4].mv[1][1], &A.mb[4].mv[3][1], &P.mb[1].mv[2][1], &P.mv[2][1], &P.mv[3][0]};
    for (int32_t *p : one) {  // the quadrants of one partition carry one vector
        *p += 1;
        BAD(call());
        *p -= 1;
    }
    GOOD(call());
    P.mb[0].mb_type = 7;  // PREDICT: every neighbour is inter
    BAD(call());
    P.mb[0].mb_type = 0;
    GOOD(call());
}

int main()
{
    intra();
    mv();
    for (int p = 0; p < FERHIP_NB_MBS; p++) EXPECT((fer_seam_pos_nb(p) & 8) == 0 || (fer_seam_pos_nb(p) & 3) == 3);  // D exists with A and B only
    printf(fails ? "%d checks failed\n" : "seam_nbhd_host_check ok\n", fails);
    return fails != 0;
}
