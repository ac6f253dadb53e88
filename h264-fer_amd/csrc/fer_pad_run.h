// fer_pad_run.h -- device helpers under the ingest kernels of fer_pic.hip (pad_run under ingest_planar_word, which
// k_pad_ingest and k_pic_ingest share; pad_run_pairs under k_pic_ingest's NV12 chroma): a run of coded samples of one row,
// fetched from a source row of any alignment as the aligned dwords that hold it and padded by edge replication.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

// 4 * N coded samples of one row from column col on: source bytes min(col + i, pw - 1) of the row that starts at `row`
template <int N>
__device__ __forceinline__ void pad_run(const uint8_t *row, uint32_t col, uint32_t pw, uint32_t (&out)[N])
{
    const uint32_t c0 = min(col, pw - 1u), c1 = min(col + 4u * N - 1u, pw - 1u);
    const uintptr_t a = (uintptr_t)(row + c0), last = (uintptr_t)(row + c1) & ~(uintptr_t)3;
    const uint32_t *p = (const uint32_t *)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)a & 3u;
    uint32_t w[N + 1];
#pragma unroll
    for (int i = 0; i <= N; i++) w[i] = (uintptr_t)(p + i) <= last ? p[i] : 0u;  // a dword past the run's last byte is not read
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
    const uint32_t nvalid = c1 - c0 + 1u;  // 1 .. 4N bytes of the run come from the source, the rest repeat the last of them
    if (nvalid < 4u * N) {
        const uint32_t k = nvalid - 1u;
        uint32_t e = 0u;
#pragma unroll
        for (int i = 0; i < N; i++)
            if ((k >> 2) == (uint32_t)i) e = out[i];
        e = ((e >> (8u * (k & 3u))) & 0xffu) * 0x01010101u;
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int keep = (int)nvalid - 4 * i;  // bytes of dword i that stay
            if (keep <= 0) {
                out[i] = e;
            } else if (keep < 4) {
                const uint32_t m = (1u << (8 * keep)) - 1u;
                out[i] = (out[i] & m) | (e & ~m);
            }
        }
    }
}

// pad_run's replication for a run that is already in registers: the first nvalid (1 .. 4N) bytes of out[] stay, the rest
// repeat the last of them
// (pad_run keeps its own copy of these lines on purpose.  With pad_run ending in pad_edge<N>(out, c1 - c0 + 1u) both
// kernels that call it through ingest_planar_word take two more VGPRs and two more instructions on gfx950 at -O3:
// k_pad_ingest 26 -> 28 VGPRs, 429 -> 431 instructions; k_pic_ingest 30 -> 32 VGPRs, 1014 -> 1016.  Neither count changes
// the occupancy, but the merge was to cost nothing; it is on record in DESIGN.md, R16.)
template <int N>
__device__ __forceinline__ void pad_edge(uint32_t (&out)[N], uint32_t nvalid)
{
    if (nvalid < 4u * N) {
        const uint32_t k = nvalid - 1u;
        uint32_t e = 0u;
#pragma unroll
        for (int i = 0; i < N; i++)
            if ((k >> 2) == (uint32_t)i) e = out[i];
        e = ((e >> (8u * (k & 3u))) & 0xffu) * 0x01010101u;
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int keep = (int)nvalid - 4 * i;  // bytes of dword i that stay
            if (keep <= 0) {
                out[i] = e;
            } else if (keep < 4) {
                const uint32_t m = (1u << (8 * keep)) - 1u;
                out[i] = (out[i] & m) | (e & ~m);
            }
        }
    }
}

// The same for a row of interleaved CbCr pairs (NV12): 4 * N coded samples of each of the two planes from column col on,
// pair min(col + i, pw - 1) of the row.  The 8 * N interleaved bytes are fetched once, as the up to 2N + 1 aligned dwords
// that hold them, shifted into place and separated with byte permutes; the replicated right edge is the run's last pair.
template <int N>
__device__ __forceinline__ void pad_run_pairs(const uint8_t *row, uint32_t col, uint32_t pw, uint32_t (&cb)[N], uint32_t (&cr)[N])
{
    const uint32_t c0 = min(col, pw - 1u), c1 = min(col + 4u * N - 1u, pw - 1u);
    const uintptr_t a = (uintptr_t)(row + 2u * c0), last = (uintptr_t)(row + 2u * c1 + 1u) & ~(uintptr_t)3;
    const uint32_t *p = (const uint32_t *)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)a & 3u;
    uint32_t w[2 * N + 1];
#pragma unroll
    for (int i = 0; i <= 2 * N; i++) w[i] = (uintptr_t)(p + i) <= last ? p[i] : 0u;  // a dword past the run's last byte is not read
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint32_t lo = __builtin_amdgcn_alignbyte(w[2 * i + 1], w[2 * i], sh);       // Cb Cr Cb Cr of pairs 4i, 4i + 1
        const uint32_t hi = __builtin_amdgcn_alignbyte(w[2 * i + 2], w[2 * i + 1], sh);   // ... of pairs 4i + 2, 4i + 3
        cb[i] = __builtin_amdgcn_perm(hi, lo, 0x06040200u);  // v_perm_b32: selector bytes 0-3 name lo's bytes, 4-7 hi's
        cr[i] = __builtin_amdgcn_perm(hi, lo, 0x07050301u);
    }
    pad_edge<N>(cb, c1 - c0 + 1u);
    pad_edge<N>(cr, c1 - c0 + 1u);
}
