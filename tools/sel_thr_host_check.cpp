// Stand-alone host check of h264-fer_amd/csrc/fer_sel_thr.h (no HIP runtime): the coarse threshold of the motion search's
// selections and the two bit-descending searches the kernels run.
//   c++ -std=c++17 -O1 tools/sel_thr_host_check.cpp -o tools/sel_thr_host_check && tools/sel_thr_host_check
//   (under sanitizers: add -fsanitize=address,undefined -fno-sanitize-recover=all)
// 1. Over every t in [0, 2^21): sel_code_of is monotone and at most FER_SEL_CODE_MAX; sel_thr(sel_code_of(t)) is
//    monotone, >= t, == t below 8 and <= t + (t >> 3) - 1 from 8 on (the granule bound the header states), below 2^21,
//    and it is the LAST value of its code (the next value has the next code).  Codes beyond FER_SEL_CODE_MAX, up to the
//    code of 2^31 - 1, give 2^21 - 1.
// 2. Over sets of 64 lane minima (random over several magnitudes, and adversarial: all equal, granule ends and starts,
//    2^21 - 1, zeros, lanes without a candidate = 0x7fffffff, minima at or above 2^21) and every need 1 .. 33 for which
//    at least `need` lanes lie below 2^21 (what the kernel counts before it searches): the coarse bound, found as the
//    kernel finds it -- sel_search_bits over the lanes' codes -- is >= the exact need-th smallest minimum, admits at least
//    `need` lanes, is the threshold of that minimum's own code (so within the granule bound of it) and below 2^21; and the
//    21-step search over the values gives the exact need-th smallest.
// Prints "ok <values swept> <searches checked>" and returns 0, or says what failed and returns 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../h264-fer_amd/csrc/fer_sel_thr.h"

static int fail(const char *what, long long a, long long b)
{
    std::printf("FAILED %s: %lld %lld\n", what, a, b);
    return 1;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static long long searches = 0;

static int check_set(const std::vector<int> &lmin)
{
    std::vector<int> srt(lmin);
    std::sort(srt.begin(), srt.end());
    int code[64];
    for (int i = 0; i < 64; i++) code[i] = sel_code_of((unsigned)lmin[i]);
    for (int need = 1; need <= 33; need++) {
        const int exact = srt[need - 1];
        if (exact >= FER_SEL_LIMIT) break;  // the kernel takes its general route: no search
        const int c = sel_search_bits<FER_SEL_CODE_BITS, FER_SEL_CODE_BITS>(need, [&](int trial) {
            int n = 0;
            for (int i = 0; i < 64; i++) n += code[i] < trial;
            return n;
        });
        const int coarse = sel_thr(c);
        int admitted = 0;
        for (int i = 0; i < 64; i++) admitted += lmin[i] <= coarse;
        if (coarse < exact) return fail("coarse bound below the exact one", coarse, exact);
        if (admitted < need) return fail("coarse bound admits too few lanes", admitted, need);
        if (coarse != sel_thr(sel_code_of((unsigned)exact))) return fail("coarse bound is not the threshold of the exact one's code", coarse, exact);
        if (exact >= 8 && coarse > exact + (exact >> 3) - 1) return fail("coarse bound beyond the granule bound", coarse, exact);
        if (exact < 8 && coarse != exact) return fail("coarse bound of a small value", coarse, exact);
        if (coarse >= FER_SEL_LIMIT) return fail("coarse bound reaches 2^21", coarse, exact);
        const int ex = sel_search_bits<21, 1>(need, [&](int trial) {
            int n = 0;
            for (int i = 0; i < 64; i++) n += lmin[i] < trial;
            return n;
        });
        if (ex != exact) return fail("21-step search", ex, exact);
        searches++;
    }
    return 0;
}

int main()
{
    // ---- 1. every value below 2^21
    int prev_code = -1, prev_thr = -1;
    for (int t = 0; t < FER_SEL_LIMIT; t++) {
        const int c = sel_code_of((unsigned)t), th = sel_thr(c);
        if (c < prev_code || c > prev_code + 1) return fail("code not monotone / skips", t, c);
        if (c > FER_SEL_CODE_MAX) return fail("code beyond FER_SEL_CODE_MAX", t, c);
        if (th < prev_thr) return fail("threshold not monotone", t, th);
        if (th < t) return fail("threshold below the value", t, th);
        if (t < 8 ? th != t : th > t + (t >> 3) - 1) return fail("granule bound", t, th);
        if (th >= FER_SEL_LIMIT) return fail("threshold reaches 2^21", t, th);
        if (sel_code_of((unsigned)th) != c) return fail("threshold outside its code", t, th);
        if (th + 1 < FER_SEL_LIMIT && sel_code_of((unsigned)th + 1u) != c + 1) return fail("threshold is not the last value of its code", t, th);
        prev_code = c;
        prev_thr = th;
    }
    if (prev_code != FER_SEL_CODE_MAX || prev_thr != FER_SEL_LIMIT - 1) return fail("the last code", prev_code, prev_thr);
    if ((1 << FER_SEL_CODE_BITS) <= FER_SEL_CODE_MAX) return fail("FER_SEL_CODE_BITS", FER_SEL_CODE_BITS, FER_SEL_CODE_MAX);
    {
        int pc = FER_SEL_CODE_MAX;
        for (unsigned t = FER_SEL_LIMIT; t < 0x80000000u; t += 1u + (t >> 12)) {  // codes of larger values stay monotone, their threshold capped
            const int c = sel_code_of(t);
            if (c < pc || c <= FER_SEL_CODE_MAX) return fail("code of a large value", t, c);
            if (sel_thr(c) != FER_SEL_LIMIT - 1) return fail("cap", t, sel_thr(c));
            pc = c;
        }
        if (sel_code_of(0x7fffffffu) != 231) return fail("code of 2^31 - 1", sel_code_of(0x7fffffffu), 231);
    }
    // ---- 2. sets of 64 lane minima
    std::vector<int> v(64);
    for (int rep = 0; rep < 6000; rep++) {  // random: magnitude, spread and the number of empty / large lanes vary
        const int bits = 1 + (int)(rnd() % 21), empty = rep % 3 == 0 ? (int)(rnd() % 40) : 0, large = rep % 5 == 0 ? (int)(rnd() % 20) : 0;
        const unsigned base = rep % 2 ? rnd() % (1u << bits) : 0u;
        for (int i = 0; i < 64; i++) {
            unsigned x = base + rnd() % (1u << (1 + rnd() % bits));
            v[i] = (int)std::min(x, (unsigned)FER_SEL_LIMIT - 1u);
        }
        for (int i = 0; i < empty; i++) v[rnd() % 64] = 0x7fffffff;
        for (int i = 0; i < large; i++) v[rnd() % 64] = FER_SEL_LIMIT + (int)(rnd() % (1u << 24));
        if (check_set(v)) return 1;
    }
    for (int c = 0; c <= FER_SEL_CODE_MAX; c++) {  // adversarial: around every granule's end
        const int th = sel_thr(c);
        const int nxt = std::min(th + 1, FER_SEL_LIMIT - 1), first = c ? sel_thr(c - 1) + 1 : 0;
        for (int k = 0; k <= 64; k += (k < 34 || k > 62) ? 1 : 7) {
            for (int i = 0; i < 64; i++) v[i] = i < k ? th : nxt;  // k lanes at the end of the granule, the others just behind it
            if (check_set(v)) return 1;
            for (int i = 0; i < 64; i++) v[(i * 37) % 64] = i < k ? first : th;  // the granule's two ends, lanes shuffled
            if (check_set(v)) return 1;
            for (int i = 0; i < 64; i++) v[i] = i < k ? th : 0x7fffffff;  // lanes without a candidate
            if (check_set(v)) return 1;
            for (int i = 0; i < 64; i++) v[i] = i < k ? 0 : th;  // zeros in front
            if (check_set(v)) return 1;
        }
    }
    for (int i = 0; i < 64; i++) v[i] = FER_SEL_LIMIT - 1;
    if (check_set(v)) return 1;
    for (int i = 0; i < 64; i++) v[i] = i < 33 ? FER_SEL_LIMIT - 1 : FER_SEL_LIMIT;  // exactly 33 lanes below the limit
    if (check_set(v)) return 1;
    for (int i = 0; i < 64; i++) v[i] = i;  // distinct small values
    if (check_set(v)) return 1;
    std::printf("ok %d %lld\n", FER_SEL_LIMIT, searches);
    return 0;
}
