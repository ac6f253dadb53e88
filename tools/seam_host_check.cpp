// Argument checks of the per-macroblock entry points (h264-fer_amd/csrc/fer_seam_host.h) as a stand-alone program, for a
// run under a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/seam_host_check.cpp -o seam_host_check && ./seam_host_check
// Every array is exactly as long as the call says, on the heap: a check that reads past what it was given is an error.
// It goes through every refusal of the five entry points and through good calls at the edges of every range.
#include "../h264-fer_amd/csrc/fer_seam_host.h"
#include <stdio.h>
#include <memory>
#include <vector>

static int fails = 0;
#define EXPECT(x)                                              \
    do {                                                       \
        if (!(x)) {                                            \
            printf("line %d: %s\n", __LINE__, #x);             \
            fails++;                                           \
        }                                                      \
    } while (0)
#define BAD(x) EXPECT((x) == FERHIP_E_ARG)
#define GOOD(x) EXPECT((x) == 0)

static void blocks()
{
    const size_t n = 5;
    std::vector<int32_t> coef(n * 16, 1), nC{0, 3, 8, 16, -1}, mx{16, 15, 16, 4, 4}, tc(n);
    std::vector<uint8_t> bits(n * 64);
    std::vector<uint32_t> nb(n);
    auto call = [&]() { return fer_seam_check_cavlc_blocks(coef.data(), nC.data(), mx.data(), n, bits.data(), nb.data(), tc.data()); };
    GOOD(call());
    BAD(fer_seam_check_cavlc_blocks(nullptr, nC.data(), mx.data(), n, bits.data(), nb.data(), tc.data()));
    BAD(fer_seam_check_cavlc_blocks(coef.data(), nullptr, mx.data(), n, bits.data(), nb.data(), tc.data()));
    BAD(fer_seam_check_cavlc_blocks(coef.data(), nC.data(), nullptr, n, bits.data(), nb.data(), tc.data()));
    BAD(fer_seam_check_cavlc_blocks(coef.data(), nC.data(), mx.data(), n, nullptr, nb.data(), tc.data()));
    BAD(fer_seam_check_cavlc_blocks(coef.data(), nC.data(), mx.data(), n, bits.data(), nullptr, tc.data()));
    BAD(fer_seam_check_cavlc_blocks(coef.data(), nC.data(), mx.data(), n, bits.data(), nb.data(), nullptr));
    BAD(fer_seam_check_cavlc_blocks(coef.data(), nC.data(), mx.data(), 0, bits.data(), nb.data(), tc.data()));
    for (int32_t m : {0, 3, 5, 14, 17, -4, 1 << 20}) {
        mx[4] = m;
        BAD(call());
    }
    mx[4] = 4;
    nC[1] = -2;
    BAD(call());
    nC[1] = -1;  // chroma DC with maxNumCoeff 15
    BAD(call());
    nC[1] = INT32_MIN;
    BAD(call());
    nC[1] = INT32_MAX;
    GOOD(call());

    // the parser: the same rules, and a stream with a bit position for every block
    std::vector<uint8_t> stream(7);
    std::vector<uint64_t> pos{0, 8, 31, 55, 54};
    nC = {0, 3, 8, 16, -1};
    std::vector<uint32_t> used(n);
    auto parse = [&](size_t nbytes) {
        return fer_seam_check_parse_blocks(stream.data(), nbytes, pos.data(), nC.data(), mx.data(), n, coef.data(), tc.data(), used.data());
    };
    GOOD(parse(7));
    BAD(parse(0));
    BAD(parse(6));  // position 55 is behind 48 bits
    pos[3] = 56;
    BAD(parse(7));
    pos[3] = ~0ull;
    BAD(parse(7));
    pos[3] = 1ull << 32;  // would wrap a 32-bit position to 0
    BAD(parse(7));
    pos[3] = 55;
    BAD(fer_seam_check_parse_blocks(stream.data(), FER_SEAM_STREAM_MAX + 1, pos.data(), nC.data(), mx.data(), n, coef.data(), tc.data(), used.data()));
    BAD(fer_seam_check_parse_blocks(nullptr, 7, pos.data(), nC.data(), mx.data(), n, coef.data(), tc.data(), used.data()));
    BAD(fer_seam_check_parse_blocks(stream.data(), 7, nullptr, nC.data(), mx.data(), n, coef.data(), tc.data(), used.data()));
    BAD(fer_seam_check_parse_blocks(stream.data(), 7, pos.data(), nullptr, mx.data(), n, coef.data(), tc.data(), used.data()));
    BAD(fer_seam_check_parse_blocks(stream.data(), 7, pos.data(), nC.data(), nullptr, n, coef.data(), tc.data(), used.data()));
    BAD(fer_seam_check_parse_blocks(stream.data(), 7, pos.data(), nC.data(), mx.data(), n, nullptr, tc.data(), used.data()));
    BAD(fer_seam_check_parse_blocks(stream.data(), 7, pos.data(), nC.data(), mx.data(), n, coef.data(), nullptr, used.data()));
    BAD(fer_seam_check_parse_blocks(stream.data(), 7, pos.data(), nC.data(), mx.data(), n, coef.data(), tc.data(), nullptr));
    BAD(fer_seam_check_parse_blocks(stream.data(), 7, pos.data(), nC.data(), mx.data(), 0, coef.data(), tc.data(), used.data()));
    mx[0] = 8;
    BAD(parse(7));
    mx[0] = 16;
    nC[0] = -1;
    BAD(parse(7));
}

static void mb_unit()
{
    const size_t n = 2;
    std::unique_ptr<ferhip_mb_job[]> J(new ferhip_mb_job[n]());
    std::unique_ptr<ferhip_mb_result[]> R(new ferhip_mb_result[n]());
    auto call = [&]() { return fer_seam_check_mb_unit(J.get(), R.get(), n); };
    J[1].op = FERHIP_MBU_SKIP, J[1].cls = 2, J[1].qp = 51, J[1].qpc = 51, J[1].blk = 15;
    GOOD(call());
    BAD(fer_seam_check_mb_unit(nullptr, R.get(), n));
    BAD(fer_seam_check_mb_unit(J.get(), nullptr, n));
    BAD(fer_seam_check_mb_unit(J.get(), R.get(), 0));
    struct {
        int32_t ferhip_mb_job::*f;
        int32_t lo, hi;
    } const fields[] = {{&ferhip_mb_job::op, 0, 4}, {&ferhip_mb_job::cls, 0, 2}, {&ferhip_mb_job::qp, 0, 51}, {&ferhip_mb_job::qpc, 0, 51}, {&ferhip_mb_job::blk, 0, 15}};
    for (const auto &f : fields) {
        const int32_t keep = J[1].*f.f;
        for (int32_t v : {f.lo - 1, f.hi + 1, INT32_MIN, INT32_MAX}) {
            J[1].*f.f = v;
            BAD(call());
        }
        for (int32_t v : {f.lo, f.hi}) {
            J[1].*f.f = v;
            GOOD(call());
        }
        J[1].*f.f = keep;
    }
}

static void mc_parts()
{
    const int W = 48, H = 32;  // 3 x 2 macroblocks
    std::vector<uint8_t> ref(W * H * 3 / 2);
    std::vector<int32_t> desc{0, 0, 0, 0, 0, 5, 3, 3, 1 << 30, -(1 << 30)}, pl(32), pb(8), pr(8);
    const size_t n = 2;
    auto call = [&](int w, int h) { return fer_seam_check_mc_parts(ref.data(), w, h, desc.data(), n, pl.data(), pb.data(), pr.data()); };
    GOOD(call(W, H));
    BAD(call(W, 16));  // macroblock 5 is not in a 3 x 1 picture
    BAD(call(0, H));
    BAD(call(W, -16));
    BAD(call(W + 1, H));
    BAD(fer_seam_check_mc_parts(nullptr, W, H, desc.data(), n, pl.data(), pb.data(), pr.data()));
    BAD(fer_seam_check_mc_parts(ref.data(), W, H, nullptr, n, pl.data(), pb.data(), pr.data()));
    BAD(fer_seam_check_mc_parts(ref.data(), W, H, desc.data(), n, nullptr, pb.data(), pr.data()));
    BAD(fer_seam_check_mc_parts(ref.data(), W, H, desc.data(), n, pl.data(), nullptr, pr.data()));
    BAD(fer_seam_check_mc_parts(ref.data(), W, H, desc.data(), n, pl.data(), pb.data(), nullptr));
    BAD(fer_seam_check_mc_parts(ref.data(), W, H, desc.data(), 0, pl.data(), pb.data(), pr.data()));
    for (int k = 0; k < 3; k++) {
        const int32_t keep = desc[5 + k], hi = k == 0 ? 5 : 3;
        for (int32_t v : {-1, hi + 1, INT32_MIN, INT32_MAX}) {
            desc[5 + k] = v;
            BAD(call(W, H));
        }
        desc[5 + k] = keep;
    }
    GOOD(call(W, H));
}

static void residual_mbs()
{
    const size_t n = 3;
    std::unique_ptr<ferhip_res_job[]> J(new ferhip_res_job[n]());
    std::unique_ptr<ferhip_res_result[]> R(new ferhip_res_result[n]());
    auto call = [&]() { return fer_seam_check_residual_mbs(J.get(), R.get(), n); };
    // job 0: WRITE without neighbours (their records are garbage and not looked at); 1: WRITE at the top of every range;
    // 2: PARSE of a full buffer at its last bit
    J[0].nb[0].p_skip = 7, J[0].nb[1].cbp_luma = -1, J[0].nb[1].tc_luma[3] = 99;
    J[1].cls = 1, J[1].cbp_luma = 15, J[1].cbp_chroma = 2, J[1].avail = 3;
    for (int k = 0; k < 2; k++) {
        J[1].nb[k].p_skip = 1, J[1].nb[k].cbp_luma = 15, J[1].nb[k].cbp_chroma = 2;
        for (int b = 0; b < 16; b++) J[1].nb[k].tc_luma[b] = 16;
        for (int b = 0; b < 8; b++) J[1].nb[k].tc_chroma[b >> 2][b & 3] = 16;
    }
    J[1].lumaLevel[15][15] = 32767, J[1].cac[1][3][15] = -32768;
    J[2].op = FERHIP_RES_PARSE, J[2].cls = 2, J[2].nbytes = FERHIP_RES_BITS_MAX, J[2].bit_pos = FERHIP_RES_BITS_MAX * 8 - 1;
    J[2].lumaLevel[0][0] = 1 << 20;  // (levels are an input of WRITE only)
    GOOD(call());
    BAD(fer_seam_check_residual_mbs(nullptr, R.get(), n));
    BAD(fer_seam_check_residual_mbs(J.get(), nullptr, n));
    BAD(fer_seam_check_residual_mbs(J.get(), R.get(), 0));
    BAD(fer_seam_check_residual_mbs(J.get(), R.get(), FER_SEAM_JOBS_MAX + 1));  // (refused before any job is read)
    struct {
        int32_t ferhip_res_job::*f;
        int32_t lo, hi;
    } const fields[] = {{&ferhip_res_job::op, 0, 1}, {&ferhip_res_job::cls, 0, 2}, {&ferhip_res_job::cbp_luma, 0, 15}, {&ferhip_res_job::cbp_chroma, 0, 2}, {&ferhip_res_job::avail, 0, 3}};
    for (const auto &f : fields) {
        const int32_t keep = J[2].*f.f;
        for (int32_t v : {f.lo - 1, f.hi + 1, INT32_MIN, INT32_MAX}) {
            J[2].*f.f = v;
            BAD(call());
        }
        J[2].*f.f = keep;
    }
    J[1].cbp_luma = 7;  // Intra16x16 codes all of its AC blocks or none
    BAD(call());
    J[1].cbp_luma = 0;
    GOOD(call());
    J[1].cbp_luma = 15;
    for (int k = 0; k < 2; k++) {
        ferhip_res_nb &N = J[1].nb[k];
        int32_t *const f[] = {&N.p_skip, &N.cbp_luma, &N.cbp_chroma, &N.tc_luma[0], &N.tc_luma[15], &N.tc_chroma[0][0], &N.tc_chroma[1][3]};
        const int32_t hi[] = {1, 15, 2, 16, 16, 16, 16};
        for (int i = 0; i < 7; i++) {
            const int32_t keep = *f[i];
            for (int32_t v : {-1, hi[i] + 1, INT32_MIN, INT32_MAX}) {
                *f[i] = v;
                BAD(call());
            }
            *f[i] = keep;
        }
    }
    J[2].bit_pos = FERHIP_RES_BITS_MAX * 8;
    BAD(call());
    J[2].bit_pos = 0xffffffffu;
    BAD(call());
    J[2].bit_pos = 0, J[2].nbytes = FERHIP_RES_BITS_MAX + 1;
    BAD(call());
    J[2].nbytes = 0xffffffffu;
    BAD(call());
    J[2].nbytes = 0x20000000u;  // 8 * nbytes wraps to 0
    BAD(call());
    J[2].nbytes = 0;
    BAD(call());
    J[2].nbytes = 1, J[2].bit_pos = 7;
    GOOD(call());
    J[2].bit_pos = 8;
    BAD(call());
    J[2].bit_pos = 7;
    J[1].dc16[5] = 32768;
    BAD(call());
    J[1].dc16[5] = 0, J[1].cdc[1][3] = -32769;
    BAD(call());
    J[1].cdc[1][3] = 0;
    GOOD(call());
}

static void block_kat()  // the pointers are only compared: a call of no blocks is a good call
{
    std::unique_ptr<int32_t[]> in(new int32_t[16]()), out(new int32_t[16]());
    for (int qP : {0, 26, 51}) GOOD(fer_seam_check_block_kat(qP, in.get(), out.get()));
    for (int qP : {-1, 52, INT32_MIN, INT32_MAX}) BAD(fer_seam_check_block_kat(qP, in.get(), out.get()));
    BAD(fer_seam_check_block_kat(26, nullptr, out.get()));
    BAD(fer_seam_check_block_kat(26, in.get(), nullptr));
}

int main()
{
    blocks();
    block_kat();
    mb_unit();
    mc_parts();
    residual_mbs();
    EXPECT(fer_seam_mb_addr_ok(0, 1) && fer_seam_mb_addr_ok(8, 9));
    EXPECT(!fer_seam_mb_addr_ok(-1, 9) && !fer_seam_mb_addr_ok(9, 9) && !fer_seam_mb_addr_ok(0, 0) && !fer_seam_mb_addr_ok(INT32_MAX, 9));
    printf(fails ? "%d checks failed\n" : "seam_host_check ok\n", fails);
    return fails != 0;
}
