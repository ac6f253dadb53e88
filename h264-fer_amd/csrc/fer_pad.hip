// fer_pad.hip -- display-size ingest (ferhip_set_frames_display, ferhip_upload_frames_display): I420 pictures of the display
// size dw x dh, stream-major [S][dw*dh*3/2] at any byte alignment, into the context's plane-major picture set of the coded
// size W x H ([S] Y, [S] Cb, [S] Cr), padded by edge replication:
//     coded sample (x, y) of a plane = source sample (min(x, pw - 1), min(y, ph - 1)),  (pw, ph) = the plane's display size.
//
//   k_pad_ingest  grid (chunk, stream), one launch for every present stream and all three planes.  A lane owns one 16-byte
//                 word of the destination and stores it whole.  A word lies in one row when the plane's coded width is a
//                 multiple of 16; a chroma plane of width W/2 = 8 (mod 16) has words that hold the last 8 samples of one row
//                 and the first 8 of the next, which are fetched as two runs of 8.  A run of source bytes starts anywhere:
//                 it is read as the aligned dwords that hold it and shifted into place (v_alignbyte_b32).  Only dwords that
//                 hold a byte of the run are read, so nothing outside the stream's own slot is touched except the rest of
//                 the dword that holds a row's first or last byte.  The replicated right edge is the run's last byte,
//                 taken from the registers; the replicated bottom rows read the last source row again (cache hits).
// No LDS, no scratch; the kernel moves (dw*dh + W*H) * 3/2 bytes per stream and is bound by HBM like k_repack.
#include "fer_internal.h"
#include "fer_pad_run.h"

struct FerPadJob {
    uint8_t *set;            // the picture set, coded size, plane-major
    const uint8_t *src;      // [S][dw*dh*3/2], any alignment
    const uint8_t *present;  // device [S] or null = every stream
    uint32_t W, H, dw, dh;
    int S;
};

__global__ __launch_bounds__(256) void k_pad_ingest(FerPadJob j)
{
    const uint32_t s = blockIdx.y;
    if (j.present && !j.present[s]) return;
    const uint32_t ysz = j.W * j.H, csz = ysz >> 2, dys = j.dw * j.dh, dcs = dys >> 2;  // (an encoder context's planes stay below 2^24)
    const uint32_t nword = (ysz + 2u * csz) >> 4;
    const uint8_t *src = j.src + (size_t)s * (dys + 2u * dcs);
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < nword; u += gridDim.x * blockDim.x) {
        uint32_t o = u << 4, PW, pw, ph;  // offset in the stream's coded picture, then in its plane
        const uint8_t *sp;
        uint8_t *dp;
        if (o < ysz) {
            PW = j.W, pw = j.dw, ph = j.dh;
            sp = src;
            dp = j.set + (size_t)s * ysz;
        } else {
            const uint32_t cr = o >= ysz + csz ? 1u : 0u;
            o -= ysz + cr * csz;
            PW = j.W >> 1, pw = j.dw >> 1, ph = j.dh >> 1;
            sp = src + dys + cr * dcs;
            dp = j.set + (size_t)j.S * (ysz + cr * csz) + (size_t)s * csz;
        }
        uint4 v;
        if ((PW & 15u) == 0u) {  // the word lies in one row
            const uint32_t y = o / PW, x = o - y * PW;
            uint32_t r[4];
            pad_run<4>(sp + min(y, ph - 1u) * pw, x, pw, r);
            v = make_uint4(r[0], r[1], r[2], r[3]);
        } else {  // PW = 8 (mod 16): each half lies in one row, the two in neighbouring rows or side by side
            const uint32_t y0 = o / PW, x0 = o - y0 * PW;
            const uint32_t y1 = (o + 8u) / PW, x1 = o + 8u - y1 * PW;
            uint32_t a[2], b[2];
            pad_run<2>(sp + min(y0, ph - 1u) * pw, x0, pw, a);
            pad_run<2>(sp + min(y1, ph - 1u) * pw, x1, pw, b);
            v = make_uint4(a[0], a[1], b[0], b[1]);
        }
        *(uint4 *)(dp + o) = v;
    }
}

void fer_launch_pad_ingest(const FerDev &d, uint8_t *set, const uint8_t *src, int dw, int dh, const uint8_t *present, hipStream_t st)
{
    FerPadJob j;
    j.set = set;
    j.src = src;
    j.present = present;
    j.W = (uint32_t)d.W;
    j.H = (uint32_t)d.H;
    j.dw = (uint32_t)dw;
    j.dh = (uint32_t)dh;
    j.S = d.S;
    const uint32_t nword = (uint32_t)(d.ysz * 3 / 2 / 16);
    const unsigned nb = (nword + 255u) / 256u;
    hipLaunchKernelGGL(k_pad_ingest, dim3(nb < 256u ? nb : 256u, d.S), dim3(256), 0, st, j);
}
