// Stand-alone host check of h264-fer_amd/csrc/fer_chain_idx.h (no HIP runtime): the index arithmetic with which
// k_me_resolve asks for the guessed lists of a later step.
//   c++ -std=c++17 -O1 tools/chain_idx_host_check.cpp -o tools/chain_idx_host_check && tools/chain_idx_host_check
//   (a developer's run under sanitizers: add -fsanitize=address,undefined -fno-sanitize-recover=all)
// For every even row length gw = 2 .. 480, every step gx, every distance 0 .. 2 (0 = the request that starts a row) and
// every lane it checks, against the layout stated here independently ([macroblock][quadrant], a row of partitions owns
// two quadrants of a row of macroblocks):
//   * the step asked for lies in the row, and is gx + ahead wherever that lies in the row;
//   * every offset addresses an entry of that step's partition, lanes beyond a list's length its last entry;
//   * in a model of the arrays of the LAST row of the last stream -- allocated with exactly their size, so that a
//     sanitizer sees an overrun -- every offset is read, and nothing outside the row's own entries.
// Prints "ok <number of index sets checked>" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../h264-fer_amd/csrc/fer_chain_idx.h"

static int fail(const char *what, int gw, int gx, int k, int lane)
{
    std::printf("FAILED %s: gw %d gx %d ahead %d lane %d\n", what, gw, gx, k, lane);
    return 1;
}

int main()
{
    long long checked = 0;
    for (int gw = 2; gw <= 480; gw += 2) {
        const int mbw = gw / 2;
        // the last row (gy odd: quadrants 2 and 3) of a picture one macroblock row high: the arrays end with the row
        const size_t nparts = (size_t)mbw * 4, first = 2;  // entry of partition (0, gy)
        std::vector<int> hdr(nparts * 4), st3n(nparts), l1(nparts * 17 * 2), l2(nparts * 33 * 2), st3(nparts * 33 * 3);
        for (size_t i = 0; i < nparts; i++) {  // every word knows its partition; quadrants 0 and 1 are the row above
            for (int j = 0; j < 4; j++) hdr[i * 4 + j] = (int)i;
            st3n[i] = (int)i;
            for (int j = 0; j < 17 * 2; j++) l1[i * 17 * 2 + j] = (int)i;
            for (int j = 0; j < 33 * 2; j++) l2[i * 33 * 2 + j] = (int)i;
            for (int j = 0; j < 33 * 3; j++) st3[i * 33 * 3 + j] = (int)i;
        }
        const int *row_hdr = hdr.data() + first * 4, *row_n = st3n.data() + first, *row_l1 = l1.data() + first * 17 * 2,
                  *row_l2 = l2.data() + first * 33 * 2, *row_st3 = st3.data() + first * 33 * 3;
        for (int gx = 0; gx < gw; gx++)
            for (int k = 0; k <= 2; k++) {
                const int g = chain_ahead_step(gx, k, gw);
                if (g < 0 || g >= gw) return fail("step outside the row", gw, gx, k, -1);
                if (gx + k < gw && g != gx + k) return fail("clamped although inside", gw, gx, k, -1);
                if (gx + k >= gw && g != gw - 1) return fail("not clamped to the last step", gw, gx, k, -1);
                const unsigned rp = chain_rel_part(g);
                const size_t want = (size_t)(g >> 1) * 4 + (size_t)(g & 1);  // macroblock g / 2, quadrant g % 2 of the row's two
                if (rp != want) return fail("relative partition", gw, gx, k, -1);
                const int part = (int)(first + want);  // what every word of that partition holds
                for (int lane = 0; lane < 64; lane++) {
                    const ChainIdx a = chain_idx_ahead(gx, k, gw, lane), b = chain_idx(rp, lane);
                    if (a.rp != b.rp || a.l1 != b.l1 || a.l2 != b.l2 || a.st3 != b.st3) return fail("chain_idx_ahead", gw, gx, k, lane);
                    if (a.rp != rp) return fail("header offset", gw, gx, k, lane);
                    if (a.l1 != rp * 17 + (unsigned)(lane < 17 ? lane : 16)) return fail("list 1 offset", gw, gx, k, lane);
                    if (a.l2 != rp * 33 + (unsigned)(lane < 33 ? lane : 32)) return fail("list 2 offset", gw, gx, k, lane);
                    if (a.st3 != a.l2 * 3) return fail("stage 3 offset", gw, gx, k, lane);
                    // the reads themselves, widths as in the kernel: int4, int, int2, int2, three ints
                    int sum = row_n[a.rp];
                    for (int j = 0; j < 4; j++) sum += row_hdr[(size_t)a.rp * 4 + j];
                    for (int j = 0; j < 2; j++) sum += row_l1[(size_t)a.l1 * 2 + j] + row_l2[(size_t)a.l2 * 2 + j];
                    for (int j = 0; j < 3; j++) sum += row_st3[(size_t)a.st3 + j];
                    if (sum != part * 12) return fail("an entry of another partition was read", gw, gx, k, lane);
                    checked++;
                }
            }
    }
    std::printf("ok %lld\n", checked);
    return 0;
}
