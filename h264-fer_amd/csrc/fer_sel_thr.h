// fer_sel_thr.h -- the coarse threshold of the motion search's selections (select_topk_ex, fer_me.hip).
// The selection gathers every candidate <= T0 and places the winners by their exact rank, so T0 is a filter: any bound
// between the need-th smallest per-lane minimum and 2^21 - 1 gives the same list while at most 64 candidates pass.  The
// search for it therefore runs over a monotone code of the value with 4 significant bits -- 8 steps where the value
// itself takes 21 -- and takes the LARGEST value of the code it finds.  Plain C++ without the HIP runtime, so that the
// arithmetic can be swept on the host (tools/sel_thr_host_check.cpp); under hipcc it is device code as well, and the
// kernels use these functions and nothing else for the coarse bound.
//
// Layout: a value t < 8 is its own code.  Otherwise e = floor(log2 t) >= 3, the code is (e - 2) << 3 | the three bits
// below the leading one: an exponent field of 5 bits (1 .. 29 for t < 2^31) over 3 mantissa bits.  A code with exponent
// field E >= 1 covers the granule [(8 + mant) << (E - 1), ((9 + mant) << (E - 1)) - 1] of 2^(E - 1) values, and
// t >= 8 << (E - 1), so
//     t <= sel_thr(sel_code_of(t)) <= t + (t >> 3) - 1    for t >= 8,    sel_thr(sel_code_of(t)) == t    for t < 8.
// The largest metric the selection's fast route ranks is 2^21 - 1 = the top of its granule (code FER_SEL_CODE_MAX),
// so no threshold of a code <= FER_SEL_CODE_MAX reaches 2^21; the cap below holds whatever code comes in.
#pragma once

#ifdef __HIPCC__
#define FER_SEL_HD __host__ __device__ inline
#else
#define FER_SEL_HD inline
#endif

#define FER_SEL_LIMIT (1 << 21)  // metrics at or above take the selection's general route
#define FER_SEL_CODE_MAX 151     // sel_code_of(FER_SEL_LIMIT - 1): exponent field 18, mantissa 7
#define FER_SEL_CODE_BITS 8      // codes of values below FER_SEL_LIMIT fit: steps of the search

// monotone code of a value 0 <= t < 2^31
FER_SEL_HD int sel_code_of(unsigned t)
{
    if (t < 8u) return (int)t;
    const int e = 31 - __builtin_clz(t);
    return ((e - 2) << 3) | (int)((t >> (e - 3)) & 7u);
}

// the largest value of the code's granule, capped at FER_SEL_LIMIT - 1 (code >= 0)
FER_SEL_HD int sel_thr(int code)
{
    const int E = code >> 3, mant = code & 7;
    if (E == 0) return mant;
    if (E > 18) return FER_SEL_LIMIT - 1;
    return ((9 + mant) << (E - 1)) - 1;
}

// The searches themselves, as the kernels run them: count_below(c) = how many of the 64 lanes hold a number < c (a ballot
// and a population count there).  -> the smallest c with at least `need` lanes <= c, built from its top bit down: a bit
// stays set while fewer than `need` lanes lie below the trial.  Needs at least `need` lanes below 1 << BITS (the caller has
// counted).  Over the lanes' codes it takes FER_SEL_CODE_BITS steps, over their values 21.  UNROLL = 1 keeps a loop.
template <int BITS, int UNROLL, class COUNT>
FER_SEL_HD int sel_search_bits(int need, COUNT count_below)
{
    int r = 0;
#pragma unroll UNROLL
    for (int b = BITS - 1; b >= 0; b--) {
        const int trial = r | (1 << b);
        r = count_below(trial) < need ? trial : r;
    }
    return r;
}
