// fer_live.hip -- what a live context needs beside the picture pipeline (FERHIP_NAL_NONE, ferhip_reset_stream):
//   k_carry_ref     a stream with no picture in a call keeps its reference picture across the swap of the picture sets
//   k_reset_stream  the device half of ferhip_reset_stream
#include "../../include/ferhip.h"
#include "fer_internal.h"

// The two picture sets are swapped after every picture, never copied: the set that was coded in place becomes the
// reference, the old reference set receives the next sources.  A stream that sat the call out has nothing in the coded
// set, so its three reference planes are copied there before the swap.  The copy is unconditional for an absent stream,
// whatever either set held before: correctness does not depend on how many calls in a row the stream has been absent
// or on which ingest call filled the sets.
//
// One launch over (chunk, stream); the workgroups of a present stream leave at once.  A stream's picture is taken as
// one run of fsz / 16 words of 16 bytes (every plane is a multiple of 64 bytes and starts on a multiple of 64, so no
// word straddles two planes and no byte tail exists; a small picture simply leaves most lanes without a word: 16x16 is
// 24 words).  Workgroup g takes the g-th contiguous share of the run; workgroups are dealt in XCD bands.
#define CARRY_THREADS 256
__global__ __launch_bounds__(CARRY_THREADS) void k_carry_ref(FerDev d)
{
    const int s = blockIdx.y;
    if (d.hdr[s * 4 + 3] != FER_PIC_ABSENT) return;
    const unsigned G = gridDim.x, g = xcd_swizzle(blockIdx.x, G);
    const size_t ysz = d.ysz, csz = d.csz, n16 = (ysz + 2 * csz) >> 4;
    const size_t i0 = n16 * g / G, i1 = n16 * (g + 1) / G;
    const uint8_t *ref = d.refY;  // base of the reference set (plane-major: [Y of all streams][Cb ...][Cr ...])
    uint8_t *cur = d.curY;
    for (size_t i = i0 + threadIdx.x; i < i1; i += CARRY_THREADS) {
        const size_t o = i << 4;
        size_t po;
        if (o < ysz)
            po = (size_t)s * ysz + o;
        else if (o < ysz + csz)
            po = (size_t)d.S * ysz + (size_t)s * csz + (o - ysz);
        else
            po = (size_t)d.S * (ysz + csz) + (size_t)s * csz + (o - ysz - csz);
        *(uint4 *)(cur + po) = *(const uint4 *)(ref + po);
    }
}

void fer_launch_carry_ref(const FerDev &d, hipStream_t st)
{
    // about eight words per lane, at most 64 workgroups per stream, a multiple of 8 (one band per XCD) from 8 on
    const size_t n16 = (d.ysz + 2 * d.csz) >> 4;
    size_t gx = n16 / (CARRY_THREADS * 8);
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    if (gx >= 8) gx &= ~(size_t)7;
    hipLaunchKernelGGL(k_carry_ref, dim3((unsigned)gx, d.S), dim3(CARRY_THREADS), 0, st, d);
}

// Slot s as in a freshly created context: mb_type (the Intra16x16 size estimate of the first IDR reads it), controller
// state with the picture count, brojTipova, the sticky status bits, the QP word, the lengths the controller would account.
__global__ __launch_bounds__(256) void k_reset_stream(FerDev d, int s, int qpw)
{
    int *mbt = d.mb_type + (size_t)s * d.nmb;
    for (int i = threadIdx.x; i < d.nmb; i += 256) mbt[i] = 0;
    if (threadIdx.x < 5) d.stats[s * 5 + threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        FerRcState z = {};
        d.rc[s] = z;
        d.status[s] = 0;
        d.qp[s] = qpw;
        d.out_bytes[s] = 0;
        if (d.q_lsse) d.q_lsse[s] = 0;
    }
}

void fer_launch_reset_stream(const FerDev &d, int s, int qpw, hipStream_t st)
{
    hipLaunchKernelGGL(k_reset_stream, dim3(1), dim3(256), 0, st, d, s, qpw);
}
