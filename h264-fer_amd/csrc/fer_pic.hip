// fer_pic.hip -- the planar picture movers: between the context's plane-major picture set of the coded size W x H ([S] Y,
// [S] Cb, [S] Cr) and pictures of the display size dw x dh that lie where a producer or consumer keeps them, at any byte
// alignment.  On the way in the coded picture is padded by edge replication:
//     coded sample (x, y) of a plane = source sample (min(x, pw - 1), min(y, ph - 1)),  (pw, ph) = the plane's display size.
//
//   ingest_planar_word  the body both ingest kernels share: three plane bases and three row pitches in, one 16-byte word of
//                 the destination out.  A word lies in one row when the plane's coded width is a multiple of 16; a chroma
//                 plane of width W/2 = 8 (mod 16) has words that hold the last 8 samples of one row and the first 8 of the
//                 next, which are fetched as two runs of 8.  A run of source bytes starts anywhere: it is read as the
//                 aligned dwords that hold it and shifted into place (pad_run, fer_pad_run.h).  Only dwords that hold a byte
//                 of the run are read; the replicated right edge is the run's last byte, taken from the registers; the
//                 replicated bottom rows read the last source row again (cache hits).
//   k_pad_ingest  (ferhip_set_frames_display, ferhip_upload_frames_display) grid (chunk, stream), one launch for every stream
//                 of the `present` mask and all three planes.  The pictures are I420, stream-major [S][dw*dh*3/2]: the bases
//                 follow from the stream, the pitches are dw, dw/2, dw/2, and the row offset is a 32-bit product.
//   k_pic_ingest  (ferhip_set_pictures) the same grid; bases and pitches come from the stream's descriptor, the row offset is
//                 a size_t product, and a stream whose descriptor has plane[0] == NULL exits after that one load.  For NV12 a
//                 chroma lane owns the Cb word and the Cr word at the same (x, y): the 32 interleaved bytes of the run are
//                 fetched once, as up to nine aligned dwords, and separated with v_perm_b32 (pad_run_pairs).
//   k_pic_emit    grid (piece, picture), the way back: the window (x0, y0, dw, dh) of a picture of the set into pitched I420
//                 or NV12.  A lane owns one aligned dword of a destination row; its four samples come from the one or two
//                 aligned source dwords that hold them (for NV12 chroma from the Cb and the Cr dwords, interleaved with
//                 v_perm_b32).  A dword that is not wholly inside its row's bytes is written byte by byte, so the pitch gaps
//                 and a neighbour's bytes are never written.  The destination of a picture comes from the descriptor table
//                 (ferhip_get_recon_pictures) or from the live decoder's map, pitches and slot size: every output of the
//                 live decoder but whole coded pictures at a 16-byte aligned address (k_dec_out, fer_decode.hip).
// No LDS, no scratch.  The ingest kernels move (dw*dh + W*H) * 3/2 bytes per stream and are bound by HBM like k_repack,
// k_pic_emit moves dw*dh*3 bytes.
// The packed formats (YUY2, UYVY, BGRA, RGBA: one plane, converted in the pass) have kernels of their own at the end of the
// file, k_pic_ingest_packed and k_pic_emit_packed; the two above are launched for I420 and NV12 only.
#include "fer_internal.h"
#include "fer_pad_run.h"
#include "fer_pic_host.h"

struct FerPicSet {
    uint8_t *set;  // the picture set, coded size, plane-major
    uint32_t W, H, dw, dh;
    int S;
};
static FerPicSet pic_set(const FerDev &d, uint8_t *set, int dw, int dh) { return {set, (uint32_t)d.W, (uint32_t)d.H, (uint32_t)dw, (uint32_t)dh, d.S}; }

// The 16-byte word at offset o of stream s's coded I420 picture (Y, Cb, Cr one behind the other, ysz = W * H), from planes
// p[] of the display size with row pitches t[].  OFF is the type of the row-offset product: uint32_t where every plane and
// its pitches stay below 2^24 bytes, else size_t.
template <typename OFF>
__device__ __forceinline__ void ingest_planar_word(const FerPicSet &j, uint32_t ysz, uint32_t s, const uint8_t *const (&p)[3], const uint32_t (&t)[3],
                                                   uint32_t o)
{
    const uint32_t csz = ysz >> 2;
    uint32_t PW, pw, ph, pitch;  // o becomes the offset in the plane
    const uint8_t *sp;
    uint8_t *dp;
    if (o < ysz) {
        PW = j.W, pw = j.dw, ph = j.dh;
        sp = p[0], pitch = t[0];
        dp = j.set + (size_t)s * ysz;
    } else {
        const uint32_t cr = o >= ysz + csz ? 1u : 0u;
        o -= ysz + cr * csz;
        PW = j.W >> 1, pw = j.dw >> 1, ph = j.dh >> 1;
        sp = cr ? p[2] : p[1], pitch = cr ? t[2] : t[1];
        dp = j.set + (size_t)j.S * (ysz + cr * csz) + (size_t)s * csz;
    }
    uint4 v;
    if ((PW & 15u) == 0u) {  // the word lies in one row
        const uint32_t y = o / PW, x = o - y * PW;
        uint32_t r[4];
        pad_run<4>(sp + (OFF)min(y, ph - 1u) * pitch, x, pw, r);
        v = make_uint4(r[0], r[1], r[2], r[3]);
    } else {  // PW = 8 (mod 16): each half lies in one row, the two in neighbouring rows or side by side
        const uint32_t y0 = o / PW, x0 = o - y0 * PW;
        const uint32_t y1 = (o + 8u) / PW, x1 = o + 8u - y1 * PW;
        uint32_t a[2], b[2];
        pad_run<2>(sp + (OFF)min(y0, ph - 1u) * pitch, x0, pw, a);
        pad_run<2>(sp + (OFF)min(y1, ph - 1u) * pitch, x1, pw, b);
        v = make_uint4(a[0], a[1], b[0], b[1]);
    }
    *(uint4 *)(dp + o) = v;
}

__global__ __launch_bounds__(256) void k_pad_ingest(FerPicSet j, const uint8_t *src, const uint8_t *present)
{
    const uint32_t s = blockIdx.y;
    if (present && !present[s]) return;
    const uint32_t ysz = j.W * j.H, dys = j.dw * j.dh, dcs = dys >> 2;  // (an encoder context's planes stay below 2^24)
    src += (size_t)s * (dys + 2u * dcs);
    const uint8_t *const p[3] = {src, src + dys, src + dys + dcs};
    const uint32_t t[3] = {j.dw, j.dw >> 1, j.dw >> 1};
    const uint32_t nword = (ysz + (ysz >> 1)) >> 4;
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < nword; u += gridDim.x * blockDim.x)
        ingest_planar_word<uint32_t>(j, ysz, s, p, t, u << 4);
}

void fer_launch_pad_ingest(const FerDev &d, uint8_t *set, const uint8_t *src, int dw, int dh, const uint8_t *present, hipStream_t st)
{
    const uint32_t nword = (uint32_t)(d.ysz * 3 / 2 / 16);
    const unsigned nb = (nword + 255u) / 256u;
    hipLaunchKernelGGL(k_pad_ingest, dim3(nb < 256u ? nb : 256u, d.S), dim3(256), 0, st, pic_set(d, set, dw, dh), src, present);
}

__global__ __launch_bounds__(256) void k_pic_ingest(FerPicSet j, const ferhip_pic *pics, int nv12)
{
    const uint32_t s = blockIdx.y;
    const ferhip_pic *pd = pics + s;
    if (!pd->plane[0]) return;
    const uint8_t *const p[3] = {(const uint8_t *)pd->plane[0], (const uint8_t *)pd->plane[1], (const uint8_t *)pd->plane[2]};
    const uint32_t t[3] = {pd->pitch[0], pd->pitch[1], pd->pitch[2]};
    const uint32_t ysz = j.W * j.H, csz = ysz >> 2;  // (an encoder context's planes stay below 2^24)
    const uint32_t nyw = ysz >> 4, ncw = csz >> 4;
    const uint32_t nword = nyw + (nv12 ? ncw : 2u * ncw);
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < nword; u += gridDim.x * blockDim.x) {
        if (!nv12 || u < nyw) {
            ingest_planar_word<size_t>(j, ysz, s, p, t, u << 4);
        } else {  // the Cb word and the Cr word at one place, from one run of CbCr pairs
            const uint32_t o = (u - nyw) << 4, PW = j.W >> 1, pw = j.dw >> 1, ph = j.dh >> 1;
            uint8_t *dcb = j.set + (size_t)j.S * ysz + (size_t)s * csz, *dcr = dcb + (size_t)j.S * csz;
            uint4 vb, vr;
            if ((PW & 15u) == 0u) {
                const uint32_t y = o / PW, x = o - y * PW;
                uint32_t b[4], r[4];
                pad_run_pairs<4>(p[1] + (size_t)min(y, ph - 1u) * t[1], x, pw, b, r);
                vb = make_uint4(b[0], b[1], b[2], b[3]);
                vr = make_uint4(r[0], r[1], r[2], r[3]);
            } else {
                const uint32_t y0 = o / PW, x0 = o - y0 * PW;
                const uint32_t y1 = (o + 8u) / PW, x1 = o + 8u - y1 * PW;
                uint32_t b0[2], r0[2], b1[2], r1[2];
                pad_run_pairs<2>(p[1] + (size_t)min(y0, ph - 1u) * t[1], x0, pw, b0, r0);
                pad_run_pairs<2>(p[1] + (size_t)min(y1, ph - 1u) * t[1], x1, pw, b1, r1);
                vb = make_uint4(b0[0], b0[1], b1[0], b1[1]);
                vr = make_uint4(r0[0], r0[1], r1[0], r1[1]);
            }
            *(uint4 *)(dcb + o) = vb;
            *(uint4 *)(dcr + o) = vr;
        }
    }
}

void fer_launch_pic_ingest(const FerDev &d, uint8_t *set, const ferhip_pic *d_pics, int format, int dw, int dh, hipStream_t st)
{
    const int nv12 = format == FERHIP_FMT_NV12;
    const uint32_t nword = (uint32_t)((d.ysz + (nv12 ? d.csz : 2 * d.csz)) / 16);
    const unsigned nb = (nword + 255u) / 256u;
    hipLaunchKernelGGL(k_pic_ingest, dim3(nb < 256u ? nb : 256u, d.S), dim3(256), 0, st, pic_set(d, set, dw, dh), d_pics, nv12);
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

// ---- packed 4:2:2 (YUY2, UYVY) and 32-bit RGB (BGRA, RGBA), converted in the same pass (ferhip.h has the definition) ----
//   k_pic_ingest_packed  grid (chunk, stream).  A lane owns a strip of two coded rows (chroma needs both) and 64 source
//                 bytes of each: 32 pixels of 4:2:2 or 16 of RGB.  A row is a whole number of aligned dwords, so a strip is
//                 fetched as four uint4 per row when its address is 16-byte aligned and as dwords otherwise, never past the
//                 row's last byte and never below row dh - 1.  The padding is made in the source domain: the dwords right of
//                 the row repeat its last pixel (strip_fill; for RGB chroma its last pixel pair, the 2x2 block of the last
//                 chroma sample), a strip below the picture takes rows dh - 2 and dh - 1 for its chroma and row dh - 1 for
//                 both luma rows.  Bytes are separated with v_perm_b32; RGB goes through
//                 v_dot4_u32_u8 with the coefficients of one sign per word (the negative ones in a word of their own), so
//                 the kernel knows neither the matrix nor the byte order.  Every byte of the coded picture is stored once:
//                 luma as uint4, chroma as uint4 or -- RGB, and a chroma plane of width W/2 = 8 (mod 16) -- as uint2.
//   k_pic_emit_packed    grid (piece, picture), the way back.  A lane owns 16 destination bytes of a row (8 pixels of 4:2:2,
//                 4 of RGB), stored as one uint4 when aligned and whole, else as the dwords that belong to the row.
// No LDS, no scratch.
struct FerPackIn {
    uint8_t *set;            // the picture set, coded size, plane-major
    const ferhip_pic *pics;  // device [S]
    uint32_t W, H, dw, dh;
    int S;
    uint32_t sel_y, sel_c, sel_fill;   // v_perm_b32 selectors: the luma and the chroma bytes of two dwords; the dword that repeats a row's last pixel
    uint32_t ky, kbp, kbn, krp, krn;   // RGB: the coefficients per byte of a pixel, Y; Cb positive, negative; Cr positive, negative
};

// n (1 .. 16) dwords of a row from p on (p is a multiple of 4); the others are not read
__device__ __forceinline__ void strip_load(const uint8_t *p, uint32_t n, uint32_t (&w)[16])
{
    const bool al = ((uintptr_t)p & 15u) == 0u;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        if (al && 4u * g + 4u <= n) {
            const uint4 v = *(const uint4 *)(p + 16 * g);
            w[4 * g] = v.x, w[4 * g + 1] = v.y, w[4 * g + 2] = v.z, w[4 * g + 3] = v.w;
        } else {
#pragma unroll
            for (int k = 4 * g; k < 4 * g + 4; k++) w[k] = (uint32_t)k < n ? ((const uint32_t *)p)[k] : 0u;
        }
    }
}

// the dwords from n on repeat the last pixel of dword n - 1 (sel makes that dword from it)
__device__ __forceinline__ void strip_fill(uint32_t (&w)[16], uint32_t n, uint32_t sel)
{
    uint32_t e = 0u;
#pragma unroll
    for (int k = 0; k < 16; k++)
        if ((uint32_t)k + 1u == n) e = w[k];
    e = __builtin_amdgcn_perm(e, e, sel);
#pragma unroll
    for (int k = 0; k < 16; k++)
        if ((uint32_t)k >= n) w[k] = e;
}

// RGB chroma is made of whole 2x2 blocks, so for it the dwords (pixels) from n on (n is even) repeat the last pixel pair
__device__ __forceinline__ void strip_fill_pairs(uint32_t (&w)[16], uint32_t n)
{
    uint32_t e0 = 0u, e1 = 0u;
#pragma unroll
    for (int k = 0; k < 16; k += 2)
        if ((uint32_t)k + 2u == n) e0 = w[k], e1 = w[k + 1];
#pragma unroll
    for (int k = 0; k < 16; k += 2)
        if ((uint32_t)k >= n) w[k] = e0, w[k + 1] = e1;
}

// (a + b + 1) >> 1 in each of the four bytes
__device__ __forceinline__ uint32_t avg_up4(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu); }

template <bool RGB>
__global__ __launch_bounds__(256) void k_pic_ingest_packed(FerPackIn j)
{
    const uint32_t s = blockIdx.y;
    const ferhip_pic *pd = j.pics + s;
    const uint8_t *p0 = (const uint8_t *)pd->plane[0];
    if (!p0) return;
    const uint32_t pitch = pd->pitch[0];
    constexpr uint32_t NP = RGB ? 16u : 32u;          // pixels in 64 source bytes
    const uint32_t ysz = j.W * j.H, csz = ysz >> 2;   // (an encoder context's planes stay below 2^24)
    const uint32_t Wc = j.W >> 1, L = (j.W + NP - 1u) / NP, nunit = L * (j.H >> 1);
    const uint32_t rowb = j.dw * (RGB ? 4u : 2u);
    uint8_t *dy = j.set + (size_t)s * ysz, *dcb = j.set + (size_t)j.S * ysz + (size_t)s * csz, *dcr = dcb + (size_t)j.S * csz;
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < nunit; u += gridDim.x * blockDim.x) {
        const uint32_t q = u / L, i = u - q * L, b0 = 64u * i;  // strip q, source bytes b0 .. b0 + 63 of its rows
        // dwords of the coded strip (a 4:2:2 picture of W = 16 (mod 32) ends in half a strip), and those of them in the
        // source row: at least one, because dw > W - 16
        const uint32_t ncd = RGB ? 16u : min(16u, (2u * j.W - b0) >> 2), nld = min(ncd, (rowb - b0) >> 2);
        const uint32_t r0 = min(2u * q, j.dh - 2u);
        uint32_t w0[16], w1[16];
        strip_load(p0 + (size_t)r0 * pitch + b0, nld, w0);
        strip_load(p0 + (size_t)(r0 + 1u) * pitch + b0, nld, w1);
        if (nld < 16u) {
            if (RGB) {  // for chroma first; luma follows below
                strip_fill_pairs(w0, nld);
                strip_fill_pairs(w1, nld);
            } else {
                strip_fill(w0, nld, j.sel_fill);
                strip_fill(w1, nld, j.sel_fill);
            }
        }
        const bool below = 2u * q >= j.dh;  // both luma rows repeat row dh - 1
        uint8_t *y0p = dy + (size_t)(2u * q) * j.W + NP * i, *y1p = y0p + j.W;
        if (!RGB) {
            uint32_t cb[4], cr[4];
#pragma unroll
            for (int m = 0; m < 4; m++) {  // Cb Cr Cb Cr of two pixel pairs per dword, averaged over the rows, then separated
                const uint32_t a0 = avg_up4(__builtin_amdgcn_perm(w0[4 * m + 1], w0[4 * m], j.sel_c), __builtin_amdgcn_perm(w1[4 * m + 1], w1[4 * m], j.sel_c));
                const uint32_t a1 = avg_up4(__builtin_amdgcn_perm(w0[4 * m + 3], w0[4 * m + 2], j.sel_c), __builtin_amdgcn_perm(w1[4 * m + 3], w1[4 * m + 2], j.sel_c));
                cb[m] = __builtin_amdgcn_perm(a1, a0, 0x06040200u);
                cr[m] = __builtin_amdgcn_perm(a1, a0, 0x07050301u);
            }
            uint32_t ya[8], yb[8];
#pragma unroll
            for (int m = 0; m < 8; m++) {
                yb[m] = __builtin_amdgcn_perm(w1[2 * m + 1], w1[2 * m], j.sel_y);
                ya[m] = below ? yb[m] : __builtin_amdgcn_perm(w0[2 * m + 1], w0[2 * m], j.sel_y);
            }
            *(uint4 *)y0p = make_uint4(ya[0], ya[1], ya[2], ya[3]);
            *(uint4 *)y1p = make_uint4(yb[0], yb[1], yb[2], yb[3]);
            if (ncd == 16u) {
                *(uint4 *)(y0p + 16) = make_uint4(ya[4], ya[5], ya[6], ya[7]);
                *(uint4 *)(y1p + 16) = make_uint4(yb[4], yb[5], yb[6], yb[7]);
            }
            const size_t co = (size_t)q * Wc + 16u * i;
            if ((Wc & 15u) == 0u) {  // every strip is whole and its 16 chroma bytes are aligned
                *(uint4 *)(dcb + co) = make_uint4(cb[0], cb[1], cb[2], cb[3]);
                *(uint4 *)(dcr + co) = make_uint4(cr[0], cr[1], cr[2], cr[3]);
            } else {  // Wc = 8 (mod 16): rows start at multiples of 8, and the last strip of a row has 8 bytes
                *(uint2 *)(dcb + co) = make_uint2(cb[0], cb[1]);
                *(uint2 *)(dcr + co) = make_uint2(cr[0], cr[1]);
                if (ncd == 16u) {
                    *(uint2 *)(dcb + co + 8) = make_uint2(cb[2], cb[3]);
                    *(uint2 *)(dcr + co + 8) = make_uint2(cr[2], cr[3]);
                }
            }
        } else {
            uint32_t cb[2], cr[2];
#pragma unroll
            for (int m = 0; m < 2; m++) {
                uint32_t vb = 0u, vr = 0u;
#pragma unroll
                for (int k = 0; k < 4; k++) {  // the 2x2 block of pixels 2p, 2p + 1; 128 << 10 and the rounding ride in the sum
                    const int p = 4 * m + k;
                    uint32_t bp = (128u << 10) + 512u, bn = 0u, rp = (128u << 10) + 512u, rn = 0u;
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const uint32_t px = (t & 2) ? w1[2 * p + (t & 1)] : w0[2 * p + (t & 1)];
                        bp = __builtin_amdgcn_udot4(px, j.kbp, bp, false);
                        bn = __builtin_amdgcn_udot4(px, j.kbn, bn, false);
                        rp = __builtin_amdgcn_udot4(px, j.krp, rp, false);
                        rn = __builtin_amdgcn_udot4(px, j.krn, rn, false);
                    }
                    vb |= ((bp - bn) >> 10) << (8 * k);
                    vr |= ((rp - rn) >> 10) << (8 * k);
                }
                cb[m] = vb, cr[m] = vr;
            }
            if (nld < 16u) {  // luma repeats the last pixel
                strip_fill(w0, nld, j.sel_fill);
                strip_fill(w1, nld, j.sel_fill);
            }
            uint32_t ya[4], yb[4];
#pragma unroll
            for (int m = 0; m < 4; m++) {  // 16 + (sum + 128 >> 8) is byte 1 of sum + 128 + (16 << 8)
                uint32_t a[4], b[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    b[k] = __builtin_amdgcn_udot4(w1[4 * m + k], j.ky, 128u + (16u << 8), false);
                    a[k] = below ? b[k] : __builtin_amdgcn_udot4(w0[4 * m + k], j.ky, 128u + (16u << 8), false);
                }
                ya[m] = __builtin_amdgcn_perm(__builtin_amdgcn_perm(a[3], a[2], 0x0c0c0501u), __builtin_amdgcn_perm(a[1], a[0], 0x0c0c0501u), 0x05040100u);
                yb[m] = __builtin_amdgcn_perm(__builtin_amdgcn_perm(b[3], b[2], 0x0c0c0501u), __builtin_amdgcn_perm(b[1], b[0], 0x0c0c0501u), 0x05040100u);
            }
            *(uint4 *)y0p = make_uint4(ya[0], ya[1], ya[2], ya[3]);
            *(uint4 *)y1p = make_uint4(yb[0], yb[1], yb[2], yb[3]);
            const size_t co = (size_t)q * Wc + 8u * i;  // Wc is a multiple of 8
            *(uint2 *)(dcb + co) = make_uint2(cb[0], cb[1]);
            *(uint2 *)(dcr + co) = make_uint2(cr[0], cr[1]);
        }
    }
}

// (yr yg yb | br bg bb | rr rg rb) of Y, Cb, Cr from R, G, B, and (rv, gu, gv, bu) of the way back, per FERHIP_CSC_*
static const int csc_fwd[2][9] = {{66, 129, 25, -38, -74, 112, 112, -94, -18}, {47, 157, 16, -26, -86, 112, 112, -102, -10}};
static const int csc_inv[2][4] = {{409, -100, -208, 516}, {459, -55, -136, 541}};

// the coefficients of R, G, B that have the sign `sign`, as magnitudes in the bytes of a pixel (A gets 0)
static uint32_t csc_word(const int *k, int sign, bool bgr)
{
    uint32_t m[3];
    for (int n = 0; n < 3; n++) m[n] = k[n] * sign > 0 ? (uint32_t)(k[n] * sign) : 0u;
    return bgr ? m[2] | m[1] << 8 | m[0] << 16 : m[0] | m[1] << 8 | m[2] << 16;
}

void fer_launch_pic_ingest_packed(const FerDev &d, uint8_t *set, const ferhip_pic *d_pics, int format, int csc, int dw, int dh, hipStream_t st)
{
    FerPackIn j = {};
    j.set = set;
    j.pics = d_pics;
    j.W = (uint32_t)d.W;
    j.H = (uint32_t)d.H;
    j.dw = (uint32_t)dw;
    j.dh = (uint32_t)dh;
    j.S = d.S;
    const bool rgb = fer_pic_packed_rgb(format);
    const uint32_t nunit = (j.W + (rgb ? 15u : 31u)) / (rgb ? 16u : 32u) * (j.H / 2u);
    const unsigned nb = (nunit + 255u) / 256u;
    const dim3 grid(nb < 256u ? nb : 256u, d.S);
    if (rgb) {
        const int *k = csc_fwd[csc];
        const bool bgr = format == FERHIP_FMT_BGRA;
        j.sel_fill = 0x03020100u;
        j.ky = csc_word(k, 1, bgr);
        j.kbp = csc_word(k + 3, 1, bgr), j.kbn = csc_word(k + 3, -1, bgr);
        j.krp = csc_word(k + 6, 1, bgr), j.krn = csc_word(k + 6, -1, bgr);
        hipLaunchKernelGGL(k_pic_ingest_packed<true>, grid, dim3(256), 0, st, j);
    } else {
        const bool yuy2 = format == FERHIP_FMT_YUY2;  // Y0 Cb Y1 Cr, else Cb Y0 Cr Y1
        j.sel_y = yuy2 ? 0x06040200u : 0x07050301u;
        j.sel_c = yuy2 ? 0x07050301u : 0x06040200u;
        j.sel_fill = yuy2 ? 0x03020102u : 0x03020300u;  // Y1 Cb Y1 Cr, Cb Y1 Cr Y1
        hipLaunchKernelGGL(k_pic_ingest_packed<false>, grid, dim3(256), 0, st, j);
    }
}

struct FerPackOut {
    const uint8_t *set;      // the picture set, coded size, plane-major
    const ferhip_pic *pics;  // device [S]: picture blockIdx.y is stream blockIdx.y, written through its descriptor; or null:
    const int2 *map;         // map[blockIdx.y] = (stream, slot), the slot at dst + slot * slot_bytes
    uint8_t *dst;
    size_t slot_bytes;
    uint32_t pitch;
    uint32_t W, ysz, x0, y0, dw, dh;
    int S;
    uint32_t sel0, sel1;     // 4:2:2: v_perm_b32 selectors of a pixel pair's dword from (Cb Cr Cb Cr, Y Y Y Y), pairs 0 and 1
    int rv, gu, gv, bu, bgr; // RGB
};

__device__ __forceinline__ uint32_t csc_clip(int v) { return (uint32_t)min(max(v, 0), 255); }

template <bool RGB>
__global__ __launch_bounds__(256) void k_pic_emit_packed(FerPackOut j)
{
    uint8_t *pl;
    uint32_t pt, s;
    if (j.pics) {
        s = blockIdx.y;
        const ferhip_pic *pd = j.pics + s;
        pl = (uint8_t *)pd->plane[0];
        if (!pl) return;
        pt = pd->pitch[0];
    } else {
        const int2 m = j.map[blockIdx.y];
        s = (uint32_t)m.x;
        pl = j.dst + (size_t)m.y * j.slot_bytes;
        pt = j.pitch;
    }
    const uint32_t csz = j.ysz >> 2, Wc = j.W >> 1;
    const uint32_t rowb = j.dw * (RGB ? 4u : 2u), np = (rowb + 15u) >> 4, npiece = j.dh * np;
    const uint8_t *sy = j.set + (size_t)s * j.ysz + (size_t)j.y0 * j.W + j.x0;
    const uint8_t *scb = j.set + (size_t)j.S * j.ysz + (size_t)s * csz + (size_t)(j.y0 >> 1) * Wc + (j.x0 >> 1);
    const size_t cr_off = (size_t)j.S * csz;  // from a Cb sample to the Cr sample of the same place
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npiece; k += gridDim.x * blockDim.x) {
        const uint32_t r = k / np, m = k - r * np;
        const uint32_t nd = min(4u, (rowb - 16u * m) >> 2);  // dwords of the row in this piece
        uint8_t *A = pl + (size_t)r * pt + 16u * m;
        const uint8_t *yrow = sy + (size_t)r * j.W, *crow = scb + (size_t)(r >> 1) * Wc;  // (x0, y0 are even)
        uint32_t o[4];
        if (!RGB) {  // 2 * nd pixels, nd of each chroma
            const uint32_t ya = emit_fetch(yrow + 8u * m, min(2u * nd, 4u)), yb = nd > 2u ? emit_fetch(yrow + 8u * m + 4u, 2u * nd - 4u) : 0u;
            const uint32_t cb = emit_fetch(crow + 4u * m, nd), cr = emit_fetch(crow + cr_off + 4u * m, nd);
            const uint32_t c01 = __builtin_amdgcn_perm(cr, cb, 0x05010400u), c23 = __builtin_amdgcn_perm(cr, cb, 0x07030602u);  // Cb Cr Cb Cr
            o[0] = __builtin_amdgcn_perm(c01, ya, j.sel0);
            o[1] = __builtin_amdgcn_perm(c01, ya, j.sel1);
            o[2] = __builtin_amdgcn_perm(c23, yb, j.sel0);
            o[3] = __builtin_amdgcn_perm(c23, yb, j.sel1);
        } else {  // nd pixels, (nd + 1) / 2 of each chroma
            const uint32_t yv = emit_fetch(yrow + 4u * m, nd);
            const uint32_t cb = emit_fetch(crow + 2u * m, (nd + 1u) >> 1), cr = emit_fetch(crow + cr_off + 2u * m, (nd + 1u) >> 1);
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const int c = (int)((yv >> (8 * x)) & 0xffu) - 16, dd = (int)((cb >> (8 * (x >> 1))) & 0xffu) - 128, e = (int)((cr >> (8 * (x >> 1))) & 0xffu) - 128;
                const int l = 298 * c + 128;
                const uint32_t R = csc_clip((l + j.rv * e) >> 8), G = csc_clip((l + j.gu * dd + j.gv * e) >> 8), B = csc_clip((l + j.bu * dd) >> 8);
                o[x] = (j.bgr ? B | R << 16 : R | B << 16) | G << 8 | 0xff000000u;
            }
        }
        if (nd == 4u && ((uintptr_t)A & 15u) == 0u) {
            *(uint4 *)A = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int x = 0; x < 4; x++)
                if ((uint32_t)x < nd) ((uint32_t *)A)[x] = o[x];
        }
    }
}

void fer_launch_pic_emit_packed(const FerDev &d, const uint8_t *set, const ferhip_pic *d_pics, const int2 *map, int n, uint8_t *dst, int format,
                                int csc, uint32_t pitch, size_t slot_bytes, const int *win, hipStream_t st)
{
    if (n <= 0) return;
    FerPackOut j = {};
    j.set = set;
    j.pics = d_pics;
    j.map = map;
    j.dst = dst;
    j.slot_bytes = slot_bytes;
    j.pitch = pitch;
    j.W = (uint32_t)d.W;
    j.ysz = (uint32_t)d.ysz;
    j.x0 = (uint32_t)win[0];
    j.y0 = (uint32_t)win[1];
    j.dw = (uint32_t)win[2];
    j.dh = (uint32_t)win[3];
    j.S = d.S;
    const bool rgb = fer_pic_packed_rgb(format);
    const uint32_t npiece = j.dh * ((j.dw * (rgb ? 4u : 2u) + 15u) / 16u);
    const unsigned nb = (npiece + 255u) / 256u;
    const dim3 grid(nb < 1024u ? nb : 1024u, n);
    if (rgb) {
        const int *k = csc_inv[csc];
        j.rv = k[0], j.gu = k[1], j.gv = k[2], j.bu = k[3];
        j.bgr = format == FERHIP_FMT_BGRA;
        hipLaunchKernelGGL(k_pic_emit_packed<true>, grid, dim3(256), 0, st, j);
    } else {
        const bool yuy2 = format == FERHIP_FMT_YUY2;  // selector bytes 0-3 name the Y dword's bytes, 4-7 Cb Cr Cb Cr
        j.sel0 = yuy2 ? 0x05010400u : 0x01050004u;    // Y0 Cb0 Y1 Cr0, else Cb0 Y0 Cr0 Y1
        j.sel1 = yuy2 ? 0x07030602u : 0x03070206u;    // Y2 Cb1 Y3 Cr1, else Cb1 Y2 Cr1 Y3
        hipLaunchKernelGGL(k_pic_emit_packed<false>, grid, dim3(256), 0, st, j);
    }
}
