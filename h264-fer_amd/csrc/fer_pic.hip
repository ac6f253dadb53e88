// fer_pic.hip -- pictures by descriptor (ferhip_set_pictures, ferhip_get_recon_pictures, ferhip_decs_set_layout): between the
// context's plane-major picture set of the coded size W x H ([S] Y, [S] Cb, [S] Cr) and pictures that lie where a producer
// or consumer keeps them: a base pointer and a row pitch per stream and plane, any byte alignment, I420 or NV12.
//
//   k_pic_ingest  grid (chunk, stream), one launch for every present stream and all planes; a stream whose descriptor has
//                 plane[0] == NULL exits after that one load.  k_pad_ingest with a row address of plane + min(y, ph - 1) *
//                 pitch: a lane owns one 16-byte word of the destination, fetches its run as the aligned dwords that hold it
//                 (pad_run, fer_pad_run.h) and stores the word whole.  For NV12 a chroma lane owns the Cb word and the Cr
//                 word at the same (x, y): the 32 interleaved bytes of the run are fetched once, as up to nine aligned
//                 dwords, and separated with v_perm_b32 (pad_run_pairs).  A chroma plane of width W/2 = 8 (mod 16) has
//                 words of two 8-sample runs in neighbouring rows, as in k_pad_ingest.
//   k_pic_emit    grid (piece, picture), the way back: the window (x0, y0, dw, dh) of a picture of the set into pitched I420
//                 or NV12.  A lane owns one aligned dword of a destination row; its four samples come from the one or two
//                 aligned source dwords that hold them (for NV12 chroma from the Cb and the Cr dwords, interleaved with
//                 v_perm_b32).  A dword that is not wholly inside its row's bytes is written byte by byte, so the pitch gaps
//                 and a neighbour's bytes are never written.  The destination of a picture comes from the descriptor table
//                 (ferhip_get_recon_pictures) or from the live decoder's map and slot size (ferhip_decs_set_layout).
// No LDS, no scratch.  k_pic_ingest moves (dw*dh + W*H) * 3/2 bytes per stream like k_pad_ingest, k_pic_emit dw*dh*3 bytes.
#include "fer_internal.h"
#include "fer_pad_run.h"

struct FerPicIn {
    uint8_t *set;            // the picture set, coded size, plane-major
    const ferhip_pic *pics;  // device [S]
    uint32_t W, H, dw, dh;
    int S, nv12;
};

__global__ __launch_bounds__(256) void k_pic_ingest(FerPicIn j)
{
    const uint32_t s = blockIdx.y;
    const ferhip_pic *pd = j.pics + s;
    const uint8_t *p0 = (const uint8_t *)pd->plane[0];
    if (!p0) return;
    const uint8_t *p1 = (const uint8_t *)pd->plane[1], *p2 = (const uint8_t *)pd->plane[2];
    const uint32_t t0 = pd->pitch[0], t1 = pd->pitch[1], t2 = pd->pitch[2];
    const uint32_t ysz = j.W * j.H, csz = ysz >> 2;  // (an encoder context's planes stay below 2^24)
    const uint32_t nyw = ysz >> 4, ncw = csz >> 4;
    const uint32_t nword = nyw + (j.nv12 ? ncw : 2u * ncw);
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < nword; u += gridDim.x * blockDim.x) {
        if (j.nv12 && u >= nyw) {  // the Cb word and the Cr word at one place, from one run of CbCr pairs
            const uint32_t o = (u - nyw) << 4, PW = j.W >> 1, pw = j.dw >> 1, ph = j.dh >> 1;
            uint8_t *dcb = j.set + (size_t)j.S * ysz + (size_t)s * csz, *dcr = dcb + (size_t)j.S * csz;
            uint4 vb, vr;
            if ((PW & 15u) == 0u) {
                const uint32_t y = o / PW, x = o - y * PW;
                uint32_t b[4], r[4];
                pad_run_pairs<4>(p1 + (size_t)min(y, ph - 1u) * t1, x, pw, b, r);
                vb = make_uint4(b[0], b[1], b[2], b[3]);
                vr = make_uint4(r[0], r[1], r[2], r[3]);
            } else {
                const uint32_t y0 = o / PW, x0 = o - y0 * PW;
                const uint32_t y1 = (o + 8u) / PW, x1 = o + 8u - y1 * PW;
                uint32_t b0[2], r0[2], b1[2], r1[2];
                pad_run_pairs<2>(p1 + (size_t)min(y0, ph - 1u) * t1, x0, pw, b0, r0);
                pad_run_pairs<2>(p1 + (size_t)min(y1, ph - 1u) * t1, x1, pw, b1, r1);
                vb = make_uint4(b0[0], b0[1], b1[0], b1[1]);
                vr = make_uint4(r0[0], r0[1], r1[0], r1[1]);
            }
            *(uint4 *)(dcb + o) = vb;
            *(uint4 *)(dcr + o) = vr;
            continue;
        }
        uint32_t o = u << 4, PW, pw, ph, pitch;  // offset in the stream's coded picture, then in its plane
        const uint8_t *sp;
        uint8_t *dp;
        if (o < ysz) {
            PW = j.W, pw = j.dw, ph = j.dh;
            sp = p0, pitch = t0;
            dp = j.set + (size_t)s * ysz;
        } else {
            const uint32_t cr = o >= ysz + csz ? 1u : 0u;
            o -= ysz + cr * csz;
            PW = j.W >> 1, pw = j.dw >> 1, ph = j.dh >> 1;
            sp = cr ? p2 : p1, pitch = cr ? t2 : t1;
            dp = j.set + (size_t)j.S * (ysz + cr * csz) + (size_t)s * csz;
        }
        uint4 v;
        if ((PW & 15u) == 0u) {  // the word lies in one row
            const uint32_t y = o / PW, x = o - y * PW;
            uint32_t r[4];
            pad_run<4>(sp + (size_t)min(y, ph - 1u) * pitch, x, pw, r);
            v = make_uint4(r[0], r[1], r[2], r[3]);
        } else {  // PW = 8 (mod 16): each half lies in one row, the two in neighbouring rows or side by side
            const uint32_t y0 = o / PW, x0 = o - y0 * PW;
            const uint32_t y1 = (o + 8u) / PW, x1 = o + 8u - y1 * PW;
            uint32_t a[2], b[2];
            pad_run<2>(sp + (size_t)min(y0, ph - 1u) * pitch, x0, pw, a);
            pad_run<2>(sp + (size_t)min(y1, ph - 1u) * pitch, x1, pw, b);
            v = make_uint4(a[0], a[1], b[0], b[1]);
        }
        *(uint4 *)(dp + o) = v;
    }
}

void fer_launch_pic_ingest(const FerDev &d, uint8_t *set, const ferhip_pic *d_pics, int format, int dw, int dh, hipStream_t st)
{
    FerPicIn j;
    j.set = set;
    j.pics = d_pics;
    j.W = (uint32_t)d.W;
    j.H = (uint32_t)d.H;
    j.dw = (uint32_t)dw;
    j.dh = (uint32_t)dh;
    j.S = d.S;
    j.nv12 = format == FERHIP_FMT_NV12;
    const uint32_t nword = (uint32_t)((d.ysz + (j.nv12 ? d.csz : 2 * d.csz)) / 16);
    const unsigned nb = (nword + 255u) / 256u;
    hipLaunchKernelGGL(k_pic_ingest, dim3(nb < 256u ? nb : 256u, d.S), dim3(256), 0, st, j);
}

struct FerPicOut {
    const uint8_t *set;      // the picture set, coded size, plane-major
    const ferhip_pic *pics;  // device [S]: picture blockIdx.y is stream blockIdx.y, written through its descriptor; or null:
    const int2 *map;         // map[blockIdx.y] = (stream, slot), the slot at dst + slot * slot_bytes, planes one behind the other
    uint8_t *dst;
    size_t slot_bytes;
    uint32_t pitch_y, pitch_c;
    uint32_t W, ysz, x0, y0, dw, dh;
    int S, nv12;
};

// n (1 .. 4) samples from p on, in the low bytes: the aligned dword that holds *p, and the next one only if it holds one of the n
__device__ __forceinline__ uint32_t emit_fetch(const uint8_t *p, uint32_t n)
{
    const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
    const uint32_t *a = (const uint32_t *)((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t w0 = a[0], w1 = sh + n > 4u ? a[1] : 0u;
    return __builtin_amdgcn_alignbyte(w1, w0, sh);
}

__global__ __launch_bounds__(256) void k_pic_emit(FerPicOut j)
{
    uint8_t *pl[3];
    uint32_t pt[3];
    uint32_t s;
    if (j.pics) {
        s = blockIdx.y;
        const ferhip_pic *pd = j.pics + s;
        pl[0] = (uint8_t *)pd->plane[0];
        if (!pl[0]) return;
        pl[1] = (uint8_t *)pd->plane[1], pl[2] = (uint8_t *)pd->plane[2];
        pt[0] = pd->pitch[0], pt[1] = pd->pitch[1], pt[2] = pd->pitch[2];
    } else {
        const int2 m = j.map[blockIdx.y];
        s = (uint32_t)m.x;
        pl[0] = j.dst + (size_t)m.y * j.slot_bytes;
        pl[1] = pl[0] + (size_t)j.pitch_y * j.dh;
        pl[2] = pl[1] + (size_t)j.pitch_c * (j.dh >> 1);
        pt[0] = j.pitch_y, pt[1] = pt[2] = j.pitch_c;
    }
    const uint32_t csz = j.ysz >> 2, Wc = j.W >> 1;
    const uint32_t rbc = j.nv12 ? j.dw : j.dw >> 1;                       // bytes of a chroma row
    const uint32_t npy = ((j.dw + 3u) >> 2) + 1u, npc = ((rbc + 3u) >> 2) + 1u;  // aligned dwords a row can touch, at most
    const uint32_t nY = j.dh * npy, nC = (j.dh >> 1) * npc;
    const uint32_t npiece = nY + (j.nv12 ? nC : 2u * nC);
    const uint8_t *sy = j.set + (size_t)s * j.ysz + (size_t)j.y0 * j.W + j.x0;
    const uint8_t *scb = j.set + (size_t)j.S * j.ysz + (size_t)s * csz + (size_t)(j.y0 >> 1) * Wc + (j.x0 >> 1);
    const size_t cr_off = (size_t)j.S * csz;  // from a Cb sample to the Cr sample of the same place
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npiece; k += gridDim.x * blockDim.x) {
        uint32_t q = k, np = npy, rb = j.dw, SW = j.W, pi = 0u;
        const uint8_t *sp = sy;
        if (q >= nY) {
            q -= nY, np = npc, rb = rbc, SW = Wc, pi = 1u, sp = scb;
            if (q >= nC) q -= nC, pi = 2u, sp = scb + cr_off;  // (I420 only)
        }
        const uint32_t r = q / np, i = q - r * np;
        const uintptr_t ra = (uintptr_t)((pi == 0u ? pl[0] : pi == 1u ? pl[1] : pl[2]) + (size_t)r * (pi == 0u ? pt[0] : pi == 1u ? pt[1] : pt[2]));
        const uintptr_t A = (ra & ~(uintptr_t)3) + 4u * i, end = ra + rb;  // this lane's dword; the row is [ra, end)
        if (A >= end) continue;
        const uint8_t *srow = sp + (size_t)r * SW;
        const bool pairs = j.nv12 && pi == 1u;
        if (A >= ra && A + 4u <= end) {
            const uint32_t c = (uint32_t)(A - ra);
            uint32_t v;
            if (!pairs) {
                v = emit_fetch(srow + c, 4u);
            } else {  // bytes c .. c + 3 of a CbCr row: pairs c/2 .. (c + 3)/2
                // An odd column uses Cb of pairs p + 1, p + 2 and Cr of pairs p, p + 1; both fetches ask for three samples from
                // pair p on.  The Cr fetch could ask for two: at shift 2 it then reads one dword less.  The dword it reads too
                // many holds Cr of pair p + 2, which is in the row, so it lies inside the picture set.
                const uint32_t n = 2u + (c & 1u);
                const uint32_t b = emit_fetch(srow + (c >> 1), n), rr = emit_fetch(srow + cr_off + (c >> 1), n);
                // v_perm_b32: selector bytes 0-3 name b's bytes, 4-7 rr's.  c even: Cb0 Cr0 Cb1 Cr1; c odd: Cr0 Cb1 Cr1 Cb2
                v = (c & 1u) ? __builtin_amdgcn_perm(rr, b, 0x02050104u) : __builtin_amdgcn_perm(rr, b, 0x05010400u);
            }
            *(uint32_t *)A = v;
        } else {
            const uintptr_t b0 = A > ra ? A : ra, b1 = A + 4u < end ? A + 4u : end;
#pragma unroll 1
            for (uintptr_t b = b0; b < b1; b++) {
                const uint32_t c = (uint32_t)(b - ra);
                *(uint8_t *)b = pairs ? srow[((c & 1u) ? cr_off : (size_t)0) + (c >> 1)] : srow[c];
            }
        }
    }
}

static void pic_emit_launch(FerPicOut &j, const FerDev &d, const uint8_t *set, int format, const int *win, int npic, hipStream_t st)
{
    j.set = set;
    j.W = (uint32_t)d.W;
    j.ysz = (uint32_t)d.ysz;
    j.x0 = (uint32_t)win[0];
    j.y0 = (uint32_t)win[1];
    j.dw = (uint32_t)win[2];
    j.dh = (uint32_t)win[3];
    j.S = d.S;
    j.nv12 = format == FERHIP_FMT_NV12;
    const uint32_t rbc = j.nv12 ? j.dw : j.dw / 2u;
    const uint32_t npiece = j.dh * ((j.dw + 3u) / 4u + 1u) + (j.nv12 ? 1u : 2u) * (j.dh / 2u) * ((rbc + 3u) / 4u + 1u);
    const unsigned nb = (npiece + 255u) / 256u;
    hipLaunchKernelGGL(k_pic_emit, dim3(nb < 1024u ? nb : 1024u, npic), dim3(256), 0, st, j);
}

void fer_launch_pic_emit(const FerDev &d, const uint8_t *set, const ferhip_pic *d_pics, int format, const int *win, hipStream_t st)
{
    FerPicOut j = {};
    j.pics = d_pics;
    pic_emit_launch(j, d, set, format, win, d.S, st);
}

void fer_launch_pic_emit_slots(const FerDev &d, const uint8_t *set, const int2 *map, int n, uint8_t *dst, int format, uint32_t pitch_y,
                               uint32_t pitch_c, size_t slot_bytes, const int *win, hipStream_t st)
{
    if (n <= 0) return;
    FerPicOut j = {};
    j.map = map;
    j.dst = dst;
    j.slot_bytes = slot_bytes;
    j.pitch_y = pitch_y;
    j.pitch_c = pitch_c;
    pic_emit_launch(j, d, set, format, win, n, st);
}
