// fer_scan.h -- the scans of the byte-stream passes (fer_nalpack.hip, fer_nalsplit.hip), device code only.  A pass gives every
// run of bytes a value of a monoid (a count, or a function that composes) and needs, for every run, the combination of the
// runs in front of it.  Three levels, each one helper here:
//   wave_scan, wave_excl         the 64 lanes of a wavefront, by shuffles;
//   wg_put, wg_front, wg_total   the four wavefronts of a 256-lane workgroup, through four LDS words and the caller's barrier;
//   carry_scan                   any number of summaries in HBM, 64 to a step of one wavefront, with a running carry.
// `op(f, g)` is always "f first, then g"; it need not commute.  store_span is the way a workgroup's output leaves LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma GCC visibility push(hidden)

__device__ __forceinline__ uint32_t scan_shfl_up(uint32_t v, int m) { return __shfl_up(v, m); }
__device__ __forceinline__ unsigned long long scan_shfl_up(unsigned long long v, int m) { return __shfl_up(v, m); }
__device__ __forceinline__ uint4 scan_shfl_up(const uint4 &f, int m)
{
    return make_uint4(__shfl_up(f.x, m), __shfl_up(f.y, m), __shfl_up(f.z, m), __shfl_up(f.w, m));
}
__device__ __forceinline__ uint32_t scan_shfl(uint32_t v, int l) { return __shfl(v, l); }
__device__ __forceinline__ unsigned long long scan_shfl(unsigned long long v, int l) { return __shfl(v, l); }
__device__ __forceinline__ uint4 scan_shfl(const uint4 &f, int l) { return make_uint4(__shfl(f.x, l), __shfl(f.y, l), __shfl(f.z, l), __shfl(f.w, l)); }

struct ScanAdd {  // the sums: uint32_t and unsigned long long
    template <typename T>
    __device__ __forceinline__ T operator()(T f, T g) const { return f + g; }
};

// inclusive scan over the wavefront, lane order
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan(T f, int lane, Op op)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const T t = scan_shfl_up(f, m);
        if (lane >= m) f = op(t, f);
    }
    return f;
}

// the exclusive form of an inclusive scan: shifted by one lane, the identity in lane 0
template <typename T>
__device__ __forceinline__ T wave_excl(const T &incl, int lane, const T &identity)
{
    T e = scan_shfl_up(incl, 1);
    if (lane == 0) e = identity;
    return e;
}

// The four wavefronts of a workgroup: wg_put leaves every wavefront's total (lane 63's inclusive value) in wtot[4]; behind
// the caller's barrier wg_front composes `pre` -- what comes into the workgroup -- with the wavefronts in front of this one,
// and wg_total is the workgroup's total.  wtot may be written again only behind another barrier.
template <typename T>
__device__ __forceinline__ void wg_put(T *wtot, const T &incl, int wave, int lane)
{
    if (lane == 63) wtot[wave] = incl;
}
template <typename T, typename Op>
__device__ __forceinline__ T wg_front(const T *wtot, int wave, T pre, Op op)
{
    for (int w = 0; w < wave; w++) pre = op(pre, wtot[w]);
    return pre;
}
template <typename T, typename Op>
__device__ __forceinline__ T wg_total(const T *wtot, Op op)
{
    return op(op(wtot[0], wtot[1]), op(wtot[2], wtot[3]));
}

// One wavefront over n summaries, 64 to a step: store(i, what comes into summary i) for every i < n, where load(i) is
// summary i; returns the combination of all n.
template <typename T, typename Op, typename Load, typename Store>
__device__ __forceinline__ T carry_scan(uint32_t n, int lane, T identity, Op op, Load load, Store store)
{
    T run = identity;  // everything in front of the step's 64 summaries
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        const T incl = wave_scan(i < n ? load(i) : identity, lane, op);
        const T excl = wave_excl(incl, lane, identity);  // the shuffle stays outside the branch: every lane takes part
        if (i < n) store(i, op(run, excl));
        run = op(run, scan_shfl(incl, 63));
    }
    return run;
}

// A workgroup of THREADS lanes stores img[sh, end) -- LDS, staged at the output's 16-byte phase sh < 16 -- to
// dst16[sh, end), dst16 16-byte aligned: the words the span fills go out whole, the ragged bytes at its two ends share a
// word with a neighbouring span and go out byte-wise.  The loops carry no other bound: one tested per byte keeps the
// compiler from widening the byte loop's stores, so a caller whose output may end early cuts `end` first (span_cut).
template <int THREADS>
__device__ __forceinline__ void store_span(uint8_t *dst16, const uint8_t *img, uint32_t sh, uint32_t end)
{
    const uint32_t nwords = (end + 15u) >> 4;
    for (uint32_t w = threadIdx.x; w < nwords; w += THREADS) {
        const uint32_t lo = w << 4, hi = lo + 16u;
        if (lo >= sh && hi <= end) {
            *(uint4 *)(dst16 + lo) = *(const uint4 *)(img + lo);
        } else {
            for (uint32_t k = max(lo, sh); k < min(hi, end); k++) dst16[k] = img[k];
        }
    }
}
// `end` of a span whose dst16 lies g0 bytes into an output of cap bytes: nothing at or behind cap is stored
__device__ __forceinline__ uint32_t span_cut(unsigned long long g0, uint32_t end, unsigned long long cap)
{
    return (uint32_t)min((unsigned long long)end, cap > g0 ? cap - g0 : 0ull);
}

#pragma GCC visibility pop
