// fer_api.hip -- the encoder side of the C ABI of libferhip (include/ferhip.h): the context and its HBM layout, ingest,
// the picture driver (the RBSP_encode sequence of F/rbsp_encoding.cpp:139-323 expressed as kernel launches), getters and
// setters.  Headers are in fer_headers.hip, NAL framing in fer_nalpack.hip, the decoder's host side in fer_decode_host.hip.
// Host code is C-style C++; nothing here runs the hot path on the CPU.
#include "fer_ctx.h"
#include "fer_pic_host.h"
#include <stdlib.h>
#include <string.h>

static const int k_qpc[52] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17,
                              18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32, 32, 33,
                              34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};

// qPiToQPc (F/inttransform.cpp:8-14) for chroma_qp_index_offset 0: what the per-macroblock shims of fer_legacy.hip need
extern "C" int ferhip_chroma_qp(int qpy) { return k_qpc[qpy < 0 ? 0 : (qpy > 51 ? 51 : qpy)]; }

int PinnedRing::create(size_t bytes_per_slot, size_t second_bytes)
{
    slot_bytes = bytes_per_slot + second_bytes;
    second_off = bytes_per_slot;
    if (!mem) CK(hipHostMalloc((void **)&mem, slot_bytes * FER_HDR_SLOTS));
    for (int i = 0; i < FER_HDR_SLOTS; i++)
        if (!ev[i]) CK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    return 0;
}
void *PinnedRing::next()
{
    slot = (slot + 1) % FER_HDR_SLOTS;
    if (hipEventSynchronize(ev[slot]) != hipSuccess) return nullptr;
    return mem + (size_t)slot * slot_bytes;
}
int PinnedRing::sent(hipStream_t st)
{
    CK(hipEventRecord(ev[slot], st));
    return 0;
}
void PinnedRing::destroy()
{
    if (mem) hipHostFree(mem);
    for (hipEvent_t &e : ev)
        if (e) hipEventDestroy(e);
    *this = PinnedRing();
}

int ealloc(ferhip_ctx *c, hipEvent_t *e)
{
    if (*e) return 0;
    CK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    c->events.push_back(*e);
    return 0;
}

void bind_planes(ferhip_ctx *c)
{
    FerDev &d = c->d;
    uint8_t *cur = c->planes[c->cur_set], *ref = c->planes[c->cur_set ^ 1];
    d.curY = cur;
    d.curCb = cur + (size_t)d.S * d.ysz;
    d.curCr = cur + (size_t)d.S * (d.ysz + d.csz);
    d.refY = ref;
    d.refCb = ref + (size_t)d.S * d.ysz;
    d.refCr = ref + (size_t)d.S * (d.ysz + d.csz);
}

extern "C" const char *ferhip_version(void) { return "ferhip 0.2 (gfx950)"; }

// ---- device / pinned memory for hosts without a HIP binding of their own (cgo, JNI, ctypes ...): the pictures of
// ferhip_set_frames(host = 0), the buffers of ferhip_copy_rbsp and the pinned sources of ferhip_upload_frames
extern "C" void *ferhip_mem_alloc(size_t bytes, int kind)  // kind 0 = device (HBM), 1 = pinned host
{
    void *p = nullptr;
    hipError_t e = kind ? hipHostMalloc(&p, bytes) : hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
extern "C" void ferhip_mem_free(void *p, int kind)
{
    if (!p) return;
    if (kind)
        hipHostFree(p);
    else
        hipFree(p);
}
// synchronous copy between host and device memory (direction inferred by the runtime)
extern "C" int ferhip_mem_copy(void *dst, const void *src, size_t bytes)
{
    if (!dst || !src) return FERHIP_E_ARG;
    CK(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
    return 0;
}

extern "C" int ferhip_create(ferhip_ctx **out, int W, int H, int S, const ferhip_params *p)
{
    return ctx_create(out, W, H, S, p, false);
}
int ctx_create(ferhip_ctx **out, int W, int H, int S, const ferhip_params *p, bool decode_only)
{
    if (!out || !p || W <= 0 || H <= 0 || (W & 15) || (H & 15) || S <= 0 || W > 16384 || H > 16384) return FERHIP_E_ARG;
    if (p->qp < 0 || p->qp > 51 || p->window < 16 || p->intra_every <= 0) return FERHIP_E_ARG;
    // the motion kernels address a stream's planes and records with 24-bit multiplies and 32-bit byte offsets: a padded
    // plane stays below 2^24 samples (4K is 8.4 M; the reference itself stops at 10 000 macroblocks)
    if (!decode_only && (size_t)(W + FER_IP_L + FER_IP_R) * (size_t)(H + FER_IP_T + FER_IP_B) >= ((size_t)1 << 24)) return FERHIP_E_UNSUP;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        fprintf(stderr, "ferhip: no HIP device; the hot path has no CPU fallback\n");
        return FERHIP_E_HIP;
    }
    ferhip_ctx *c = new ferhip_ctx();
    memset(&c->d, 0, sizeof c->d);
    c->p = *p;
    FerDev &d = c->d;
    d.W = W;
    d.H = H;
    d.Wc = W / 2;
    d.Hc = H / 2;
    d.mbw = W / 16;
    d.mbh = H / 16;
    d.nmb = d.mbw * d.mbh;
    d.S = S;
    d.window = p->window;
    d.maxdiff_set = p->maxdiff;
    d.basic = p->basic ? 1 : 0;
#ifdef FER_PROBE
    d.dbg = getenv("FER_DBG") ? atoi(getenv("FER_DBG")) : 0;
#else
    d.dbg = 0;  // no environment variable changes what the shipped library computes
#endif
    d.ysz = (size_t)W * H;
    d.csz = d.ysz / 4;
    d.resolve_wgs = 6144;
    d.resolve_group = S;  // all streams of a ticket queue in one group (measured: 4.9 ms against 6.1 with a short last group)
    {
        int lo = 0, hi = 0;  // numerically lower = higher priority
        if (hipGetDevice(&c->device) != hipSuccess || hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess ||
            hipStreamCreateWithPriority(&c->st, hipStreamNonBlocking, lo) != hipSuccess ||
            hipStreamCreateWithPriority(&c->st_hi, hipStreamNonBlocking, hi) != hipSuccess ||
            hipStreamCreateWithPriority(&c->st_aux, hipStreamNonBlocking, lo) != hipSuccess ||
            ealloc(c, &c->ev_c) || ealloc(c, &c->ev_d) || ealloc(c, &c->ev_a) || ealloc(c, &c->ev_b)) {
            ferhip_destroy(c);
            return FERHIP_E_HIP;
        }
    }
    size_t fsz = d.ysz * 3 / 2;
    int rc = 0;
    rc |= dalloc(c, &c->planes[0], fsz * S);
    rc |= dalloc(c, &c->planes[1], fsz * S);
    d.ipitch = W + FER_IP_L + FER_IP_R;
    d.iplane = (((size_t)d.ipitch * (H + FER_IP_T + FER_IP_B)) + 255) & ~(size_t)255;
    d.ioff = FER_IP_T * d.ipitch + FER_IP_L;
    rc |= dalloc(c, &d.interp, decode_only ? (size_t)1 : (size_t)(d.iplane * 16 * S));
    d.feat = nullptr;  // the 16-plane feature table exists only as a test read-back (FERHIP_BUF_FEAT)
    rc |= dalloc(c, &d.feat0, decode_only ? (size_t)1 : (size_t)(d.ysz * 6 * S));
    rc |= dalloc(c, &d.sort_pos, decode_only ? (size_t)1 : (size_t)(d.ysz * S));
    rc |= dalloc(c, &d.sort_rec, decode_only ? (size_t)1 : (size_t)(d.ysz * S * 3));
    d.ktw_shift = 3;  // column tiles of the bucket index: at most 64 per row, at least 8 columns wide
    while (((W + (1 << d.ktw_shift) - 1) >> d.ktw_shift) > 64) d.ktw_shift++;
    d.kt = (W + (1 << d.ktw_shift) - 1) >> d.ktw_shift;
    const size_t nbins = (size_t)S * 16384 * d.kt + 1;
    rc |= dalloc(c, &d.kol2, decode_only ? (size_t)1 : (size_t)(nbins));
    rc |= dalloc(c, &d.brange, decode_only ? (size_t)1 : (size_t)S * 16384 * 8);
    rc |= dalloc(c, &d.bmodal, decode_only ? (size_t)1 : (size_t)S * 16384 * 4);
    d.nlists = W * H / FER_BRANGE_MIN + 1;
    rc |= dalloc(c, &d.boutl, decode_only ? (size_t)1 : (size_t)S * d.nlists * FER_OUTL);
    rc |= dalloc(c, &d.nbig, (size_t)S);
    rc |= dalloc(c, &d.zero_cnt, (size_t)S);
    size_t nm = (size_t)d.nmb * S;
    rc |= dalloc(c, &d.mb_type, nm);
    rc |= dalloc(c, &d.mv, nm * 8);
    rc |= dalloc(c, &d.mvd, nm * 8);
    rc |= dalloc(c, &d.cbp, nm * 2);
    rc |= dalloc(c, &d.tc, nm * 24);
    rc |= dalloc(c, &d.i4mode, nm * 16);
    rc |= dalloc(c, &d.i4flag, nm * 16);
    rc |= dalloc(c, &d.chroma_mode, nm);
    rc |= dalloc(c, &d.levels, nm * FER_LEVELS);
    rc |= dalloc(c, &d.mbsize, nm * 2);
    rc |= dalloc(c, &d.suma, decode_only ? (size_t)1 : (size_t)(nm * 20));
    rc |= dalloc(c, &d.st3, decode_only ? (size_t)1 : (size_t)(nm * 4 * 33 * 3));
    rc |= dalloc(c, &d.st3n, decode_only ? (size_t)1 : (size_t)(nm * 4));
    rc |= dalloc(c, &d.st2, decode_only ? (size_t)1 : (size_t)(nm * 4 * FER_ST2_CAP * 2));
    rc |= dalloc(c, &d.st2n, decode_only ? (size_t)1 : (size_t)(nm * 4));
    rc |= dalloc(c, &d.v0, decode_only ? (size_t)1 : (size_t)(nm * 4));
    rc |= dalloc(c, &d.spec_hdr, decode_only ? (size_t)1 : (size_t)(nm * 4));
    rc |= dalloc(c, &d.spec_l1, decode_only ? (size_t)1 : (size_t)(nm * 4 * 17));
    rc |= dalloc(c, &d.spec_l2, decode_only ? (size_t)1 : (size_t)(nm * 4 * 33));
    // one slot per workgroup of the chain: its grid is min(rows of all streams, FERHIP_TUNE_RESOLVE_WGS <= 65535)
    d.spec_slots = decode_only ? 1 : (int)std::min<size_t>(65535, (size_t)2 * d.mbh * S);
    rc |= dalloc(c, &d.spec_stat, (size_t)4 * d.spec_slots);
    d.speculate = 1;
    rc |= dalloc(c, &d.chain, (size_t)64);
    rc |= dalloc(c, &d.timing, (size_t)64);
    rc |= dalloc(c, &d.chain64, decode_only ? (size_t)1 : (size_t)(nm * 4));
    rc |= dalloc(c, &d.mb_bits, ((size_t)d.nmb + 1) * S);
    d.bits_cap_words = ((size_t)d.nmb * 1024 + 4096) / 4;
    rc |= dalloc(c, &d.bits, decode_only ? (size_t)1 : (size_t)(d.bits_cap_words * S));
    rc |= dalloc(c, &d.hdr, (size_t)4 * S);
    rc |= dalloc(c, &d.qp, (size_t)S);
    rc |= dalloc(c, &d.rc_par, (size_t)S);
    rc |= dalloc(c, &d.rc, (size_t)S);
    rc |= dalloc(c, &d.out_bytes, (size_t)S);
    rc |= dalloc(c, &d.status, (size_t)S);
    rc |= dalloc(c, &d.sad, (size_t)S);
    rc |= dalloc(c, &d.sad_part, (size_t)FER_SAD_G * S);
    rc |= dalloc(c, &d.stats, (size_t)5 * S);
    rc |= dalloc(c, &d.dec_qp, nm);
    rc |= dalloc(c, &d.dec_state, (size_t)4 * S);
    rc |= dalloc(c, &d.dec_cac, (size_t)128 * S);
    rc |= dalloc(c, &c->d_present, (size_t)S);
    rc |= dalloc(c, &c->d_sadskip, (size_t)S);
    int n = W * H;
    c->sort.tmp_bytes = fer_sort_tmp_bytes(n, S);
    rc |= dalloc(c, &c->sort.rec_tmp, decode_only ? (size_t)1 : (size_t)((size_t)n * S * 3));
    rc |= dalloc(c, &c->sort.rec1, decode_only ? (size_t)1 : (size_t)((size_t)n * S));
    rc |= dalloc(c, &c->sort.keyT, decode_only ? (size_t)1 : (size_t)((size_t)n * S));
    rc |= dalloc(c, &c->sort.dig2, decode_only ? (size_t)1 : (size_t)((size_t)n * S));
    rc |= dalloc(c, &c->sort.skey, decode_only ? (size_t)1 : (size_t)((size_t)n * S));
    uint8_t *tmp = nullptr;
    rc |= dalloc(c, &tmp, decode_only ? (size_t)1 : (size_t)(c->sort.tmp_bytes));
    c->sort.tmp = tmp;
    if (rc) {
        ferhip_destroy(c);
        return FERHIP_E_HIP;
    }
    if (c->hdr_ring.create(sizeof(uint32_t) * 4 * S, sizeof(FerRcPar) * S) || c->pres_ring.create((size_t)S) ||
        halloc(c, &c->h_len, (size_t)S) || halloc(c, &c->h_sadskip, (size_t)S) || halloc(c, &c->h_status, (size_t)S) ||
        halloc(c, &c->h_sad, (size_t)S)) {
        ferhip_destroy(c);
        return FERHIP_E_HIP;
    }
    c->ss.assign(S, StreamState{0, 0, 0, 0, 0, 0});
    // every stream starts in constant QP at params.qp, which is also the QP of its PPS; chroma_qp_index_offset == 0
    // (F/headers_and_parameter_sets.cpp:490)
    c->rate.assign(S, FerRcPar{FERHIP_RC_CQP, p->qp, 0, 51, 1, 0, p->intra_every, p->qp, 0, 0, 0});
    {
        std::vector<int> q0(S, p->qp | k_qpc[p->qp] << 8);
        if (hipMemcpy(d.qp, q0.data(), sizeof(int) * S, hipMemcpyHostToDevice) != hipSuccess) {
            ferhip_destroy(c);
            return FERHIP_E_HIP;
        }
    }
    c->types.assign(S, 2);
    c->disp_w = W;
    c->disp_h = H;
    bind_planes(c);
    // the buffers were cleared on the null stream, which the context's non-blocking streams do not wait for: without
    // this the clearing of a large buffer can land after the first picture's kernels have written into it
    if (hipDeviceSynchronize() != hipSuccess) {
        ferhip_destroy(c);
        return FERHIP_E_HIP;
    }
    *out = c;
    return 0;
}

extern "C" void ferhip_destroy(ferhip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->st) hipStreamSynchronize(c->st);
    if (c->st_hi) hipStreamSynchronize(c->st_hi);
    if (c->st_aux) hipStreamSynchronize(c->st_aux);
    if (c->st_copy) hipStreamSynchronize(c->st_copy);
    for (void *p : c->allocs) hipFree(p);
    if (c->nal_buf) hipFree(c->nal_buf);
    for (void *p : c->pinned) hipHostFree(p);
    for (hipEvent_t e : c->events) hipEventDestroy(e);
    for (PinnedRing *r : {&c->hdr_ring, &c->pres_ring, &c->ps_ring, &c->pic_ring, &c->rtp_ring, &c->ts_ring, &c->ts_psi_ring, &c->mp4_ring}) r->destroy();
    for (hipStream_t st : {c->st, c->st_hi, c->st_aux, c->st_copy})
        if (st) hipStreamDestroy(st);
    delete c;
}

// [S][Y|U|V] interleaved per stream  <->  plane-major [Y of all streams][U ...][V ...]
// I420 pictures, stream-major [S][Y|Cb|Cr] <-> the context's plane-major picture set [plane][S][...], both in
// device memory: one launch instead of three copies per stream.  16 bytes per thread (plane sizes are multiples of 64).
// present (device [S], or null = every stream): a stream whose byte is 0 is left out -- its slot of `frames` is never read
__global__ __launch_bounds__(256) void k_repack(uint8_t *set, uint8_t *frames, size_t ysz, size_t csz, int S, int to_set,
                                                const uint8_t *present)
{
    const size_t fsz = ysz + 2 * csz;
    const int s = blockIdx.y;
    if (present && !present[s]) return;
    for (size_t o = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; o < fsz; o += (size_t)gridDim.x * blockDim.x * 16) {
        size_t po;
        if (o < ysz)
            po = (size_t)s * ysz + o;
        else if (o < ysz + csz)
            po = (size_t)S * ysz + (size_t)s * csz + (o - ysz);
        else
            po = (size_t)S * (ysz + csz) + (size_t)s * csz + (o - ysz - csz);
        uint4 *a = (uint4 *)(set + po), *b = (uint4 *)(frames + (size_t)s * fsz + o);
        if (to_set)
            *a = *b;
        else
            *b = *a;
    }
}

// A presence mask (host [S]) rides a pinned ring to the device, ordered before the kernel that reads it on the context's
// stream; null stays null (= every stream)
static int send_mask(ferhip_ctx *c, const uint8_t *present, const uint8_t **d_mask)
{
    *d_mask = nullptr;
    if (!present) return 0;
    const int S = c->d.S;
    uint8_t *h = (uint8_t *)c->pres_ring.next();
    if (!h) return FERHIP_E_HIP;
    for (int s = 0; s < S; s++) h[s] = present[s] ? 1 : 0;
    CK(hipMemcpyAsync(c->d_present, h, (size_t)S, hipMemcpyHostToDevice, c->st));
    if (c->pres_ring.sent(c->st)) return FERHIP_E_HIP;
    *d_mask = c->d_present;
    return 0;
}

// A device buffer on first use.  dalloc clears on the null stream and the buffer's users run on streams that do not wait
// for that one, so the clear is waited for here.  On failure *p stays null and a later call tries again.
template <typename T>
static int dalloc_first_use(ferhip_ctx *c, T **p, size_t n)
{
    if (*p) return 0;
    T *v = nullptr;
    if (dalloc(c, &v, n) || hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        return FERHIP_E_HIP;
    }
    *p = v;
    return 0;
}

// host pictures [S][fsz] to the same places of a device buffer, on stream st: only the pictures of present streams cross
// the bus (null = every stream), one copy per run of neighbouring present streams
static int copy_present_runs(uint8_t *dst, const void *src, size_t fsz, int S, const uint8_t *present, hipStream_t st)
{
    for (int s = 0; s < S;) {
        if (present && !present[s]) {
            s++;
            continue;
        }
        int e = s;
        while (e < S && (!present || present[e])) e++;
        CK(hipMemcpyAsync(dst + (size_t)s * fsz, (const uint8_t *)src + (size_t)s * fsz, (size_t)(e - s) * fsz, hipMemcpyHostToDevice, st));
        s = e;
    }
    return 0;
}

// present (host [S], or null = every stream): only the pictures of streams with a non-zero byte are read from src
static int copy_frames(ferhip_ctx *c, uint8_t *set, const uint8_t *src, uint8_t *dst, hipMemcpyKind kind,
                       const uint8_t *present = nullptr)
{
    FerDev &d = c->d;
    size_t fsz = d.ysz * 3 / 2;
    if (kind == hipMemcpyDeviceToDevice && (((uintptr_t)(src ? src : dst)) & 15) == 0) {
        const uint8_t *d_mask = nullptr;
        if (send_mask(c, present, &d_mask)) return FERHIP_E_HIP;
        hipLaunchKernelGGL(k_repack, dim3(256, d.S), dim3(256), 0, c->st, set, (uint8_t *)(src ? src : dst), d.ysz, d.csz, d.S,
                           src ? 1 : 0, d_mask);
        return 0;
    }
    for (int s = 0; s < d.S; s++) {
        if (present && !present[s]) continue;
        uint8_t *py = set + (size_t)s * d.ysz;
        uint8_t *pu = set + (size_t)d.S * d.ysz + (size_t)s * d.csz;
        uint8_t *pv = set + (size_t)d.S * (d.ysz + d.csz) + (size_t)s * d.csz;
        if (src) {
            const uint8_t *f = src + (size_t)s * fsz;
            CK(hipMemcpyAsync(py, f, d.ysz, kind, c->st));
            CK(hipMemcpyAsync(pu, f + d.ysz, d.csz, kind, c->st));
            CK(hipMemcpyAsync(pv, f + d.ysz + d.csz, d.csz, kind, c->st));
        } else {
            uint8_t *f = dst + (size_t)s * fsz;
            CK(hipMemcpyAsync(f, py, d.ysz, kind, c->st));
            CK(hipMemcpyAsync(f + d.ysz, pu, d.csz, kind, c->st));
            CK(hipMemcpyAsync(f + d.ysz + d.csz, pv, d.csz, kind, c->st));
        }
    }
    return 0;
}

extern "C" int ferhip_set_frames(ferhip_ctx *c, const void *src, int host)
{
    if (!c || !src) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    int rc = copy_frames(c, c->planes[c->cur_set], (const uint8_t *)src, nullptr,
                         host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice);
    if (rc) return rc;
    if (host) CK(hipStreamSynchronize(c->st));
    return 0;
}

// The pictures of the streams that have one in this call (present[s] != 0); the slots of the others are never read
extern "C" int ferhip_set_frames_live(ferhip_ctx *c, const void *src, int host, const uint8_t *present)
{
    if (!c || !src || !present) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    int rc = copy_frames(c, c->planes[c->cur_set], (const uint8_t *)src, nullptr,
                         host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, present);
    if (rc) return rc;
    if (host) CK(hipStreamSynchronize(c->st));
    return 0;
}

// ---- display size: pictures coded at W x H that the SPS crops to dw x dh (k_pad_ingest of fer_pic.hip, fer_headers.hip) ----
extern "C" int ferhip_set_display_size(ferhip_ctx *c, int dw, int dh)
{
    if (!c) return FERHIP_E_ARG;
    const FerDev &d = c->d;
    if (dw <= 0 || dh <= 0 || (dw & 1) || (dh & 1) || dw <= d.W - 16 || dw > d.W || dh <= d.H - 16 || dh > d.H) return FERHIP_E_ARG;
    if (c->coded) return FERHIP_E_STATE;
    c->disp_w = dw;
    c->disp_h = dh;
    for (uint8_t &x : c->ps_dirty) x = 1;  // the SPS in the device table changes
    return 0;
}

// display-size pictures in device memory ([S][dw*dh*3/2], any alignment) -> the current picture set, padded
static int pad_frames(ferhip_ctx *c, const uint8_t *d_src, const uint8_t *present)
{
    const uint8_t *d_mask = nullptr;
    if (send_mask(c, present, &d_mask)) return FERHIP_E_HIP;
    fer_launch_pad_ingest(c->d, c->planes[c->cur_set], d_src, c->disp_w, c->disp_h, d_mask, c->st);
    CK(hipGetLastError());
    return 0;
}

extern "C" int ferhip_set_frames_display(ferhip_ctx *c, const void *src, int host, const uint8_t *present)
{
    if (!c || !src) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    const FerDev &d = c->d;
    if (!host) return pad_frames(c, (const uint8_t *)src, present);
    // host pictures: the present ones cross the bus into a device buffer, the pad kernel takes them from there
    const size_t fsz = (size_t)c->disp_w * c->disp_h * 3 / 2;
    int rc = dalloc_first_use(c, &c->disp_stage, d.ysz * 3 / 2 * d.S);
    if (!rc) rc = copy_present_runs(c->disp_stage, src, fsz, d.S, present, c->st);
    if (!rc) rc = pad_frames(c, c->disp_stage, present);
    if (rc) return rc;
    CK(hipStreamSynchronize(c->st));
    return 0;
}

// the top-left dw x dh window of the last reconstruction, [S][dw*dh*3/2]: one strided copy per plane and stream
extern "C" int ferhip_get_recon_display(ferhip_ctx *c, void *dst, int host)
{
    if (!c || !dst) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    const FerDev &d = c->d;
    const size_t dw = (size_t)c->disp_w, dh = (size_t)c->disp_h, dys = dw * dh, fsz = dys * 3 / 2;
    const uint8_t *set = c->planes[c->cur_set ^ 1];  // after encode_picture the reconstruction is the reference set
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    for (int s = 0; s < d.S; s++) {
        uint8_t *o = (uint8_t *)dst + (size_t)s * fsz;
        CK(hipMemcpy2DAsync(o, dw, set + (size_t)s * d.ysz, (size_t)d.W, dw, dh, kind, c->st));
        for (int k = 0; k < 2; k++)
            CK(hipMemcpy2DAsync(o + dys + (size_t)k * (dys / 4), dw / 2, set + (size_t)d.S * (d.ysz + k * d.csz) + (size_t)s * d.csz,
                                (size_t)d.Wc, dw / 2, dh / 2, kind, c->st));
    }
    CK(hipStreamSynchronize(c->st));
    return 0;
}

// ---- pictures by descriptor (fer_pic.hip): a pointer and a pitch per stream and plane, I420 or NV12 ----
// The checked descriptors (host [S]) ride a pinned ring to the device table, ordered before the kernel that reads it on the
// context's stream.  Table and ring are made on first use.  Of an absent stream only the NULL plane[0] is passed on.
static int send_pics(ferhip_ctx *c, const ferhip_pic *pics, int format)
{
    const int S = c->d.S;
    int rc = fer_pic_check(pics, S, format, (uint32_t)c->disp_w);
    if (rc) return rc;
    if (!c->d_pics && (c->pic_ring.create(sizeof(ferhip_pic) * S) || dalloc_first_use(c, &c->d_pics, (size_t)S))) return FERHIP_E_HIP;
    ferhip_pic *h = (ferhip_pic *)c->pic_ring.next();
    if (!h) return FERHIP_E_HIP;
    for (int s = 0; s < S; s++) h[s] = pics[s].plane[0] ? pics[s] : ferhip_pic{};
    CK(hipMemcpyAsync(c->d_pics, h, sizeof(ferhip_pic) * S, hipMemcpyHostToDevice, c->st));
    return c->pic_ring.sent(c->st);
}

extern "C" int ferhip_set_pictures(ferhip_ctx *c, const ferhip_pic *pics, int format)
{
    if (!c || !pics) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    int rc = send_pics(c, pics, format);
    if (rc) return rc;
    if (fer_pic_packed(format))
        fer_launch_pic_ingest_packed(c->d, c->planes[c->cur_set], c->d_pics, format, c->csc, c->disp_w, c->disp_h, c->st);
    else
        fer_launch_pic_ingest(c->d, c->planes[c->cur_set], c->d_pics, format, c->disp_w, c->disp_h, c->st);
    CK(hipGetLastError());
    return 0;
}

extern "C" int ferhip_get_recon_pictures(ferhip_ctx *c, const ferhip_pic *pics, int format)
{
    if (!c || !pics) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    int rc = send_pics(c, pics, format);
    if (rc) return rc;
    const int win[4] = {0, 0, c->disp_w, c->disp_h};
    const uint8_t *set = c->planes[c->cur_set ^ 1];  // the reconstruction is the reference set
    if (fer_pic_packed(format))
        fer_launch_pic_emit_packed(c->d, set, c->d_pics, nullptr, c->d.S, nullptr, format, c->csc, 0, 0, win, c->st);
    else
        fer_launch_pic_emit(c->d, set, c->d_pics, format, win, c->st);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(c->st));
    return 0;
}

// the matrix of the RGB formats (FERHIP_CSC_*), from the next ferhip_set_pictures / ferhip_get_recon_pictures on
extern "C" int ferhip_set_csc(ferhip_ctx *c, int matrix)
{
    if (!c || (matrix != FERHIP_CSC_BT601 && matrix != FERHIP_CSC_BT709)) return FERHIP_E_ARG;
    c->csc = matrix;
    return 0;
}

// ---- asynchronous ingest: ReadFromY4M's successor for many streams (row f3) ----
// ferhip_upload_frames starts the H2D copy of the NEXT pictures ([S][W*H*3/2], pinned host memory) on a copy stream
// of its own and returns; up to two uploads may be in flight.  ferhip_set_frames_uploaded makes the oldest one the
// current picture (the repack runs on the encode stream behind the copy).  So the upload of picture t + 1 overlaps
// the encode of picture t.
// display: the pictures are [S][dw*dh*3/2] at the display size; the staging slot (sized for coded pictures) remembers it
static int upload_frames(ferhip_ctx *c, const void *pinned_src, const uint8_t *present, bool display);
extern "C" int ferhip_upload_frames(ferhip_ctx *c, const void *pinned_src) { return upload_frames(c, pinned_src, nullptr, false); }
extern "C" int ferhip_upload_frames_live(ferhip_ctx *c, const void *pinned_src, const uint8_t *present)
{
    if (!present) return FERHIP_E_ARG;
    return upload_frames(c, pinned_src, present, false);
}
extern "C" int ferhip_upload_frames_display(ferhip_ctx *c, const void *pinned_src, const uint8_t *present)
{
    return upload_frames(c, pinned_src, present, true);
}
static int upload_frames(ferhip_ctx *c, const void *pinned_src, const uint8_t *present, bool display)
{
    if (!c || !pinned_src) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    FerDev &d = c->d;
    const size_t bytes = d.ysz * 3 / 2 * d.S;
    const size_t fsz = display ? (size_t)c->disp_w * c->disp_h * 3 / 2 : d.ysz * 3 / 2;  // one picture of the source
    if (!c->st_copy) {
        // first call: the copy stream, two staging sets, their events.  A failure on the way leaves the context as it
        // was before the call (st_copy null), so that a later call tries again instead of meeting half a setup.
        hipStream_t stc = nullptr;
        CK(hipStreamCreateWithFlags(&stc, hipStreamNonBlocking));
        bool ok = true;
        for (int i = 0; i < 2 && ok; i++)
            ok = !dalloc_first_use(c, &c->stage[i], bytes) && !ealloc(c, &c->up_done[i]) && !ealloc(c, &c->up_used[i]);
        if (!ok) {
            (void)hipGetLastError();
            hipStreamDestroy(stc);
            fprintf(stderr, "ferhip_upload_frames: could not set up the staging buffers\n");
            return FERHIP_E_HIP;
        }
        c->st_copy = stc;
    }
    if (c->up_ready >= 2) return FERHIP_E_STATE;
    const int k = c->up_next;
    CK(hipStreamWaitEvent(c->st_copy, c->up_used[k], 0));  // the repack that last read this slot
    c->up_disp[k] = display;
    c->up_mask[k].clear();  // the mask stays with the staging slot until ferhip_set_frames_uploaded repacks it
    if (present) c->up_mask[k].assign(present, present + d.S);
    if (copy_present_runs(c->stage[k], pinned_src, fsz, d.S, present, c->st_copy)) return FERHIP_E_HIP;
    CK(hipEventRecord(c->up_done[k], c->st_copy));
    c->up_next ^= 1;
    c->up_ready++;
    return 0;
}

extern "C" int ferhip_set_frames_uploaded(ferhip_ctx *c)
{
    if (!c) return FERHIP_E_ARG;
    if (c->up_ready <= 0) return FERHIP_E_STATE;
    (void)hipSetDevice(c->device);
    const int k = (c->up_next + 2 - c->up_ready) & 1;  // oldest upload in flight
    CK(hipStreamWaitEvent(c->st, c->up_done[k], 0));
    const uint8_t *mask = c->up_mask[k].empty() ? nullptr : c->up_mask[k].data();
    int rc = c->up_disp[k] ? pad_frames(c, c->stage[k], mask) : copy_frames(c, c->planes[c->cur_set], c->stage[k], nullptr, hipMemcpyDeviceToDevice, mask);
    if (rc) return rc;
    CK(hipEventRecord(c->up_used[k], c->st));
    c->up_ready--;
    return 0;
}

extern "C" int ferhip_set_reference(ferhip_ctx *c, const void *src)
{
    if (!c || !src) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    int rc = copy_frames(c, c->planes[c->cur_set ^ 1], (const uint8_t *)src, nullptr, hipMemcpyHostToDevice);
    if (rc) return rc;
    CK(hipStreamSynchronize(c->st));
    for (auto &s : c->ss) s.have_dpb = 1;
    c->refprep_valid = false;
    return 0;
}

extern "C" int ferhip_get_recon(ferhip_ctx *c, void *dst, int host)
{
    if (!c || !dst) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    // after encode_picture the reconstruction is the reference set
    int rc = copy_frames(c, c->planes[c->cur_set ^ 1], nullptr, (uint8_t *)dst,
                         host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    if (rc) return rc;
    CK(hipStreamSynchronize(c->st));
    return 0;
}


// Start filling the next slot of the header ring (waits for the copy that used it FER_HDR_SLOTS pictures ago) ...
static int hdr_begin(ferhip_ctx *c)
{
    c->h_hdr = (uint32_t *)c->hdr_ring.next();
    return c->h_hdr ? 0 : FERHIP_E_HIP;
}
// ... and send it, with the rate settings when they changed
static int hdr_upload(ferhip_ctx *c)
{
    CK(hipMemcpyAsync(c->d.hdr, c->h_hdr, sizeof(uint32_t) * 4 * c->d.S, hipMemcpyHostToDevice, c->st));
    if (c->rate_dirty) {
        FerRcPar *h = (FerRcPar *)c->hdr_ring.second();
        memcpy(h, c->rate.data(), sizeof(FerRcPar) * c->d.S);
        CK(hipMemcpyAsync(c->d.rc_par, h, sizeof(FerRcPar) * c->d.S, hipMemcpyHostToDevice, c->st));
        c->rate_dirty = false;
    }
    return c->hdr_ring.sent(c->st);
}

// Quality measurement: what run_picture measures -- the flags of ferhip_set_quality, and at least the SSE when a stream is in
// FERHIP_RC_QUALITY (its controller reads the luma SSE of the stream's last picture)
static int quality_flags(ferhip_ctx *c)
{
    int f = c->qflags;
    for (const FerRcPar &r : c->rate)
        if (r.mode == FERHIP_RC_QUALITY) {
            f |= FERHIP_QM_SSE;
            break;
        }
    return f;
}

// the snapshot of the source, the ring and k_quality's partials, on first use
static int quality_alloc(ferhip_ctx *c)
{
    FerDev &d = c->d;
    if (d.qsrc) return 0;
    const int G = fer_quality_groups(d);
    uint8_t *src = nullptr;
    ferhip_quality *ring = nullptr;
    unsigned long long *lsse = nullptr;
    FerQPart *part = nullptr;
    unsigned *ticket = nullptr;
    if (dalloc(c, &src, d.ysz * 3 / 2 * d.S) || dalloc(c, &ring, (size_t)FERHIP_QUALITY_RING * d.S) || dalloc(c, &lsse, (size_t)d.S) ||
        dalloc(c, &part, (size_t)G * d.S) || dalloc(c, &ticket, (size_t)d.S) || hipDeviceSynchronize() != hipSuccess) {  // dalloc clears on the null stream
        (void)hipGetLastError();
        fprintf(stderr, "ferhip: could not allocate the quality measurement buffers\n");
        return FERHIP_E_HIP;
    }
    d.qgroups = G;
    d.qring = ring;
    d.q_lsse = lsse;
    d.qpart = part;
    d.qticket = ticket;
    d.qsrc = src;
    return 0;
}

// selectNALUnitType, F/ref_frames.cpp:185-234: nt[s] in = request (AUTO / IDR / SLICE / NONE), out = decision (NONE stays)
static int decide_types(ferhip_ctx *c, const int *nal_type, std::vector<int> &nt)
{
    FerDev &d = c->d;
    const int S = d.S;
    nt.assign(S, 0);
    const int UNDECIDED = -2;
    bool need_sad = false, any_none = false;
    for (int s = 0; s < S; s++) {
        int req = nal_type ? nal_type[s] : FERHIP_NAL_AUTO;
        StreamState &t = c->ss[s];
        if (req == FERHIP_NAL_NONE) {
            nt[s] = FERHIP_NAL_NONE;
            any_none = true;
        } else if (req == FERHIP_NAL_IDR || req == FERHIP_NAL_SLICE) {
            nt[s] = (!t.have_dpb) ? FERHIP_NAL_IDR : req;
        } else if (!t.have_dpb || t.frames_done % c->p.intra_every == 0) {
            nt[s] = FERHIP_NAL_IDR;
        } else {
            nt[s] = UNDECIDED;
            need_sad = true;
        }
    }
    if (need_sad) {
        const uint8_t *skip = nullptr;
        if (any_none) {
            // absent streams take no part: with the SAD read-back waiting for the stream below, one pinned slot serves
            for (int s = 0; s < S; s++) c->h_sadskip[s] = nt[s] == FERHIP_NAL_NONE;
            CK(hipMemcpyAsync(c->d_sadskip, c->h_sadskip, (size_t)S, hipMemcpyHostToDevice, c->st));
            skip = c->d_sadskip;
        }
        {
            ProfScope ps(c, FERHIP_PH_FRAME_SAD, 1);
            fer_launch_frame_sad(d, skip, c->st);
        }
        CK(hipMemcpyAsync(c->h_sad, d.sad, sizeof(unsigned long long) * S, hipMemcpyDeviceToHost, c->st));
        CK(hipStreamSynchronize(c->st));
        for (int s = 0; s < S; s++)
            if (nt[s] == UNDECIDED) nt[s] = c->h_sad[s] > ((unsigned long long)d.nmb << 12) ? FERHIP_NAL_IDR : FERHIP_NAL_SLICE;
    }
    return 0;
}

extern "C" int ferhip_select_nal_type(ferhip_ctx *c, int *nal_type_out)
{
    if (!c || !nal_type_out) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    std::vector<int> nt;
    // on input FERHIP_NAL_NONE marks the streams that have no picture (they keep it); every other stream is decided as AUTO
    std::vector<int> req(c->d.S);
    for (int s = 0; s < c->d.S; s++) req[s] = nal_type_out[s] == FERHIP_NAL_NONE ? FERHIP_NAL_NONE : FERHIP_NAL_AUTO;
    int rc = decide_types(c, req.data(), nt);
    if (rc) return rc;
    for (int s = 0; s < c->d.S; s++) nal_type_out[s] = nt[s];
    return 0;
}

static int run_picture(ferhip_ctx *c, int *nal_type)
{
    FerDev &d = c->d;
    const int S = d.S;
    std::vector<int> nt;
    int rc0 = decide_types(c, nal_type, nt);
    if (rc0) return rc0;
    bool anyP = false, anyI = false, anyNone = false;
    if (hdr_begin(c)) return FERHIP_E_HIP;
    for (int s = 0; s < S; s++) {
        build_header(c, s, nt[s]);
        if (nal_type) nal_type[s] = nt[s];
        anyP |= c->types[s] == 0;
        anyI |= c->types[s] == 2;
        anyNone |= c->types[s] == FER_PIC_ABSENT;
    }
    if (hdr_upload(c)) return FERHIP_E_HIP;
    c->nal_ready = true;
    c->pic_serial++;
    fer_launch_rc_plan(d, c->st);  // each stream's QP and slice_qp_delta, before anything reads qp[] or hdr[] (fer_rate.hip)
    if (!anyP && !anyI) {
        // every stream sat the call out: k_rc_plan has accounted what was pending and set every RBSP length to 0; no
        // picture set is touched or swapped, nothing is measured, no stream's state moves
        CK(hipGetLastError());
        return 0;
    }
    c->coded = true;  // from here on the display size is fixed (ferhip_set_display_size)
    if (anyNone) fer_launch_carry_ref(d, c->st);  // absent streams keep their reference picture across the swap below
    // quality measurement: the source is reconstructed in place, so it is kept before the first launch that reconstructs
    const int qflags = quality_flags(c);
    if (qflags) {
        if (quality_alloc(c)) return FERHIP_E_HIP;
        CK(hipMemcpyAsync(d.qsrc, d.curY, d.ysz * 3 / 2 * S, hipMemcpyDeviceToDevice, c->st));
    }
    const int ndiag = d.mbw + 2 * (d.mbh - 1);
    if (anyP) {
        // The radix sort of the reference picture's positions and its bucket index are a stream of HBM traffic that only
        // the bucket walk needs; the stage-3 search (k_me_pre) is bound by VALU issue and needs only the quarter-sample
        // planes and the plane-0 features.  The two run side by side: the sort on st_aux, k_me_pre on st.
        bool sort_aside = false;
        if (!c->refprep_valid) {
            {
                ProfScope ps(c, FERHIP_PH_INTERP, 1);
                fer_launch_interp(d, c->st);
            }
            // BasicInterEncoding never walks the buckets (F/moestimation.cpp:470): the sorted order is not built
            if (!d.basic) {
                {
                    ProfScope ps(c, FERHIP_PH_SORT_KEYS, 1);
                    fer_launch_sort_keys(d, c->sort, c->st);
                }
                hipStream_t ss = c->st;
                if (c->overlap_sort) {
                    sort_aside = true;
                    ss = c->overlap_sort == 2 ? c->st_hi : c->st_aux;
                    CK(hipEventRecord(c->ev_c, c->st));
                    CK(hipStreamWaitEvent(ss, c->ev_c, 0));
                }
                {
                    ProfScope ps(c, FERHIP_PH_SORT, 1, ss);
                    fer_launch_sort_radix(d, c->sort, ss);
                }
                {
                    ProfScope ps(c, FERHIP_PH_SORT_FINISH, 1, ss);
                    fer_launch_sort_finish(d, c->sort, ss);
                }
                if (sort_aside) CK(hipEventRecord(c->ev_d, ss));
            }
        }
        {
            ProfScope ps(c, FERHIP_PH_ME_PRE, 1);
            fer_launch_me_pre(d, c->st);
        }
        if (sort_aside) CK(hipStreamWaitEvent(c->st, c->ev_d, 0));
        {
            ProfScope ps(c, FERHIP_PH_ME_WALK, 1);
            fer_launch_me_walk(d, c->st);
        }
        if (d.speculate) {
            ProfScope ps(c, FERHIP_PH_ME_SPEC, 1);
            fer_launch_me_spec(d, c->st);
        }
        {
            // the per-diagonal chain is latency bound: run it on the high-priority stream so that its small
            // launches are dispatched ahead of other contexts' throughput kernels
            CK(hipEventRecord(c->ev_a, c->st));
            CK(hipStreamWaitEvent(c->st_hi, c->ev_a, 0));
            {
                ProfScope ps(c, FERHIP_PH_ME_RESOLVE, 1, c->st_hi);
                d.serial = d.serial % 0x7ffffff0 + 1;  // validates this picture's words in chain64
                fer_launch_me_resolve(d, c->st_hi);
            }
            CK(hipEventRecord(c->ev_b, c->st_hi));
            CK(hipStreamWaitEvent(c->st, c->ev_b, 0));
        }
        {
            ProfScope ps(c, FERHIP_PH_P_RESID, 1);
            fer_launch_basic_stat(d, c->st);  // BasicInterEncoding only: brojTipova of the discarded exhaustive pass
            fer_launch_p_resid(d, c->st);
            fer_launch_type_count(d, c->st);  // brojTipova of the P streams, from the types the two launches above left
        }
    }
    if (anyI) {
        CK(hipEventRecord(c->ev_a, c->st));
        CK(hipStreamWaitEvent(c->st_hi, c->ev_a, 0));
        {
            ProfScope ps(c, FERHIP_PH_INTRA, ndiag, c->st_hi);
            fer_launch_intra(d, c->st_hi);
        }
        CK(hipEventRecord(c->ev_b, c->st_hi));
        CK(hipStreamWaitEvent(c->st, c->ev_b, 0));
    }
    {
        ProfScope ps(c, FERHIP_PH_CAVLC, 1);
        fer_launch_cavlc(d, c->st);
    }
    if (qflags) {  // after entropy coding: the record carries the RBSP length (fer_quality.hip)
        fer_launch_quality(d, qflags, (int)(c->q_count % FERHIP_QUALITY_RING), c->st);
        c->q_count++;
    }
    CK(hipGetLastError());
    // the reconstruction becomes the reference picture (frameDeepCopy, F/ref_frames.cpp:17)
    c->cur_set ^= 1;
    bind_planes(c);
    c->refprep_valid = false;
    for (int s = 0; s < S; s++) {
        if (c->types[s] == FER_PIC_ABSENT) continue;
        c->ss[s].have_dpb = 1;
        c->ss[s].frames_done++;
    }
    return 0;
}

extern "C" int ferhip_encode_picture_dev(ferhip_ctx *c, int *nal_type, const uint8_t **d_rbsp, size_t *stride,
                                         const uint32_t **d_rbsp_len)
{
    if (!c) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    int rc = run_picture(c, nal_type);
    if (rc) return rc;
    if (d_rbsp) *d_rbsp = (const uint8_t *)c->d.bits;
    if (stride) *stride = c->d.bits_cap_words * 4;
    if (d_rbsp_len) *d_rbsp_len = c->d.out_bytes;
    return 0;
}

// RBSP of the last picture -> caller buffers, asynchronously on the context's stream (so it is ordered before the
// next picture reuses the device buffer): bytes_per_stream bytes of every stream's RBSP to dst + s * dst_stride and
// the S lengths to len_dst.  host = 1: dst / len_dst are (pinned) host memory.  ferhip_sync() waits.
extern "C" int ferhip_copy_rbsp(ferhip_ctx *c, void *dst, size_t dst_stride, size_t bytes_per_stream, uint32_t *len_dst, int host)
{
    if (!c || !dst || !len_dst) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    FerDev &d = c->d;
    const size_t cap = d.bits_cap_words * 4;
    if (bytes_per_stream > cap) bytes_per_stream = cap;
    if (bytes_per_stream > dst_stride) return FERHIP_E_ARG;
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    CK(hipMemcpy2DAsync(dst, dst_stride, d.bits, cap, bytes_per_stream, (size_t)d.S, kind, c->st));
    CK(hipMemcpyAsync(len_dst, d.out_bytes, sizeof(uint32_t) * d.S, kind, c->st));
    return 0;
}


extern "C" int ferhip_sync(ferhip_ctx *c)
{
    if (!c) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    CK(hipStreamSynchronize(c->st));
    CK(hipStreamSynchronize(c->st_hi));
    return 0;
}

extern "C" int ferhip_encode_picture(ferhip_ctx *c, int *nal_type, uint8_t *rbsp, size_t rbsp_stride, uint32_t *rbsp_len)
{
    if (!c || !rbsp || !rbsp_len) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    int rc = run_picture(c, nal_type);
    if (rc) return rc;
    FerDev &d = c->d;
    CK(hipMemcpyAsync(c->h_len, d.out_bytes, sizeof(uint32_t) * d.S, hipMemcpyDeviceToHost, c->st));
    CK(hipMemcpyAsync(c->h_status, d.status, sizeof(int) * d.S, hipMemcpyDeviceToHost, c->st));
    CK(hipStreamSynchronize(c->st));
    for (int s = 0; s < d.S; s++) {
        if (c->h_status[s]) {
            fprintf(stderr, "ferhip: stream %d device status 0x%x\n", s, c->h_status[s]);
            return FERHIP_E_DEVICE;
        }
        rbsp_len[s] = c->h_len[s];
        if (c->h_len[s] > rbsp_stride) return FERHIP_E_ARG;
        if (c->h_len[s] == 0) continue;  // FERHIP_NAL_NONE
        CK(hipMemcpyAsync(rbsp + (size_t)s * rbsp_stride, (const uint8_t *)d.bits + (size_t)s * d.bits_cap_words * 4,
                          c->h_len[s], hipMemcpyDeviceToHost, c->st));
    }
    CK(hipStreamSynchronize(c->st));
    return 0;
}

extern "C" int ferhip_encode_streams(ferhip_ctx *c, const uint8_t *frames, int nframes, uint8_t *out, size_t out_stride,
                                     size_t *out_len, uint8_t *recon)
{
    if (!c || !frames || !out || !out_len || nframes <= 0) return FERHIP_E_ARG;
    FerDev &d = c->d;
    const int S = d.S;
    size_t fsz = d.ysz * 3 / 2;
    size_t rstride = d.bits_cap_words * 4;
    std::vector<uint8_t> rbsp(rstride * S);
    std::vector<uint32_t> len(S);
    std::vector<int> nt(S);
    uint8_t hdr[64];
    for (int s = 0; s < S; s++) {
        size_t pos = 0, n;
        n = ferhip_write_sps(c, hdr, sizeof hdr);
        pos += ferhip_write_nal(1, 7, hdr, n, out + (size_t)s * out_stride + pos);
        n = ferhip_write_pps_stream(c, s, hdr, sizeof hdr);
        pos += ferhip_write_nal(1, 8, hdr, n, out + (size_t)s * out_stride + pos);
        out_len[s] = pos;
    }
    for (int f = 0; f < nframes; f++) {
        int rc = ferhip_set_frames(c, frames + (size_t)f * S * fsz, 1);
        if (rc) return rc;
        for (int s = 0; s < S; s++) nt[s] = FERHIP_NAL_AUTO;
        rc = ferhip_encode_picture(c, nt.data(), rbsp.data(), rstride, len.data());
        if (rc) return rc;
        for (int s = 0; s < S; s++) {
            if (out_len[s] + (size_t)len[s] * 3 / 2 + 16 > out_stride) return FERHIP_E_ARG;
            out_len[s] += ferhip_write_nal(1, nt[s], rbsp.data() + (size_t)s * rstride, len[s],
                                           out + (size_t)s * out_stride + out_len[s]);
        }
        if (recon) {
            rc = ferhip_get_recon(c, recon + (size_t)f * S * fsz, 1);
            if (rc) return rc;
        }
    }
    return 0;
}

// The context's streams are non-blocking: a synchronous copy on the null stream does not wait for them.
static hipError_t ctx_sync(ferhip_ctx *c)
{
    hipError_t e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(c->st_aux);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(c->st_hi);
}

extern "C" int ferhip_get_stats(ferhip_ctx *c, int *out)
{
    if (!c || !out) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    CK(ctx_sync(c));
    CK(hipMemcpy(out, c->d.stats, sizeof(int) * 5 * c->d.S, hipMemcpyDeviceToHost));
    return 0;
}

// rate control: the settings take effect with the next picture, k_rc_plan applies them on the device
extern "C" int ferhip_set_rate(ferhip_ctx *c, int s, const ferhip_rate *r)
{
    if (!c || !r || s < -1 || s >= c->d.S) return FERHIP_E_ARG;
    if (r->mode != FERHIP_RC_CQP && r->mode != FERHIP_RC_ABR && r->mode != FERHIP_RC_QUALITY) return FERHIP_E_ARG;
    if (r->qp < 0 || r->qp > 51) return FERHIP_E_ARG;
    if (r->mode != FERHIP_RC_CQP &&
        (r->qp_min < 0 || r->qp_max > 51 || r->qp_min > r->qp_max || r->max_step < 1 || r->ip_offset < -51 || r->ip_offset > 51))
        return FERHIP_E_ARG;
    if (r->mode == FERHIP_RC_ABR && (r->window < 0 || r->target_bits <= 0)) return FERHIP_E_ARG;
    if (r->mode == FERHIP_RC_QUALITY && r->target_sse <= 0) return FERHIP_E_ARG;
    const int s0 = s < 0 ? 0 : s, s1 = s < 0 ? c->d.S : s + 1;
    // before a stream's first picture its PPS is not sent yet: r->qp becomes its base, which pic_init_qp_minus26 must hold
    for (int k = s0; k < s1; k++)
        if (c->ss[k].frames_done == 0 && r->qp > 37) return FERHIP_E_ARG;
    for (int k = s0; k < s1; k++) {
        FerRcPar &p = c->rate[k];
        if (r->mode != FERHIP_RC_CQP && p.mode != r->mode) p.gen++;
        p.mode = r->mode;
        p.qp = r->qp;
        if (r->mode != FERHIP_RC_CQP) {
            p.qp_min = r->qp_min;
            p.qp_max = r->qp_max;
            p.max_step = r->max_step;
            p.ip_offset = r->ip_offset;
        }
        if (r->mode == FERHIP_RC_ABR) {
            p.window = r->window > 0 ? r->window : c->p.intra_every;
            p.target = r->target_bits;
        }
        if (r->mode == FERHIP_RC_QUALITY) p.tsse = r->target_sse;
        if (c->ss[k].frames_done == 0) {
            p.base = r->qp;
            if (!c->ps_dirty.empty()) c->ps_dirty[k] = 1;  // its PPS changes
        }
    }
    c->rate_dirty = true;
    return 0;
}

// Slot s as in a freshly created context (a new feed takes the slot); the other slots are untouched.  The device half is
// one small kernel on the context's stream, behind the slot's last picture; nothing waits.
extern "C" int ferhip_reset_stream(ferhip_ctx *c, int s)
{
    if (!c || s < 0 || s >= c->d.S) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    c->ss[s] = StreamState{0, 0, 0, 0, 0, 0};
    c->rate[s] = FerRcPar{FERHIP_RC_CQP, c->p.qp, 0, 51, 1, 0, c->p.intra_every, c->p.qp, 0, 0, 0};
    c->rate_dirty = true;
    if (!c->ps_dirty.empty()) c->ps_dirty[s] = 1;
    c->types[s] = 2;
    fer_launch_reset_stream(c->d, s, c->p.qp | k_qpc[c->p.qp] << 8, c->st);
    CK(hipGetLastError());
    return 0;
}

extern "C" int ferhip_set_quality(ferhip_ctx *c, int flags)
{
    if (!c || (flags & ~(FERHIP_QM_SSE | FERHIP_QM_SSIM))) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    if (flags && quality_alloc(c)) return FERHIP_E_HIP;
    c->qflags = flags;
    return 0;
}

// the ring, oldest record first; waits for the last picture
extern "C" int ferhip_get_quality(ferhip_ctx *c, int npic, ferhip_quality *out)
{
    if (!c || !out || npic <= 0) return FERHIP_E_ARG;
    if (c->q_count == 0) return FERHIP_E_STATE;
    (void)hipSetDevice(c->device);
    const int S = c->d.S;
    long long n = c->q_count < FERHIP_QUALITY_RING ? c->q_count : FERHIP_QUALITY_RING;
    if (n > npic) n = npic;
    std::vector<ferhip_quality> ring((size_t)FERHIP_QUALITY_RING * S);
    CK(ctx_sync(c));
    CK(hipMemcpy(ring.data(), c->d.qring, sizeof(ferhip_quality) * ring.size(), hipMemcpyDeviceToHost));
    for (long long k = 0; k < n; k++) {
        const long long slot = (c->q_count - n + k) % FERHIP_QUALITY_RING;
        memcpy(out + (size_t)k * S, ring.data() + (size_t)slot * S, sizeof(ferhip_quality) * S);
    }
    return (int)n;
}

// QP of every stream's last picture (params.qp before the first); waits for that picture
extern "C" int ferhip_get_qp(ferhip_ctx *c, int *out)
{
    if (!c || !out) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    CK(ctx_sync(c));
    CK(hipMemcpy(out, c->d.qp, sizeof(int) * c->d.S, hipMemcpyDeviceToHost));
    for (int s = 0; s < c->d.S; s++) out[s] &= 0xff;
    return 0;
}

extern "C" int ferhip_status(ferhip_ctx *c, int *out)
{
    if (!c || !out) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    CK(ctx_sync(c));
    CK(hipMemcpy(out, c->d.status, sizeof(int) * c->d.S, hipMemcpyDeviceToHost));
    return 0;
}

// launch-shape knobs (results never depend on them)
extern "C" int ferhip_tune(ferhip_ctx *c, int key, int value)
{
    if (!c) return FERHIP_E_ARG;
    switch (key) {
    case FERHIP_TUNE_RESOLVE_WGS:
        if (value < 1 || value > 65535) return FERHIP_E_ARG;  // (any grid takes every row: workgroups move from queue to queue)
        c->d.resolve_wgs = value;
        return 0;
    case FERHIP_TUNE_RESOLVE_GROUP:
        if (value < 1) return FERHIP_E_ARG;
        c->d.resolve_group = value < c->d.S ? value : c->d.S;  // (more streams than the context has add nothing)
        return 0;
    case FERHIP_TUNE_OVERLAP_SORT:
        if (value < 0 || value > 2) return FERHIP_E_ARG;  // (2: on the high-priority stream -- an experiment)
        c->overlap_sort = value;
        return 0;
    case FERHIP_TUNE_SPECULATE:
        if (value != 0 && value != 1) return FERHIP_E_ARG;
        c->d.speculate = value;
        return 0;
    default: return FERHIP_E_ARG;
    }
}

extern "C" int ferhip_profile(ferhip_ctx *c, int enable)
{
    if (!c) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    c->prof = enable != 0;
    return 0;
}

extern "C" int ferhip_get_profile(ferhip_ctx *c, double *ms, long *launches, int reset)
{
    if (!c || !ms || !launches) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    CK(hipStreamSynchronize(c->st));
    for (auto &sp : c->spans) {
        float t = 0;
        CK(hipEventElapsedTime(&t, sp.a, sp.b));
        c->prof_ms[sp.phase] += t;
        c->prof_launches[sp.phase] += sp.launches;
        hipEventDestroy(sp.a);
        hipEventDestroy(sp.b);
    }
    c->spans.clear();
    for (int i = 0; i < FERHIP_NPHASE; i++) {
        ms[i] = c->prof_ms[i];
        launches[i] = c->prof_launches[i];
    }
    if (reset) {
        memset(c->prof_ms, 0, sizeof c->prof_ms);
        memset(c->prof_launches, 0, sizeof c->prof_launches);
    }
    return 0;
}

// ---- per-stage entry points
static void set_all_types(ferhip_ctx *c, int slice_type)
{
    if (hdr_begin(c)) return;
    for (int s = 0; s < c->d.S; s++) {
        c->h_hdr[s * 4 + 0] = c->h_hdr[s * 4 + 1] = 0;
        c->h_hdr[s * 4 + 2] = 1;
        c->h_hdr[s * 4 + 3] = (uint32_t)slice_type;
        c->types[s] = slice_type;
    }
    (void)hdr_upload(c);
}

extern "C" int ferhip_fill_interpolated(ferhip_ctx *c)
{
    if (!c) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    set_all_types(c, 0);
    fer_launch_refprep(c->d, c->sort, nullptr, c->st);
    CK(hipStreamSynchronize(c->st));
    CK(hipGetLastError());
    c->refprep_valid = true;
    return 0;
}

extern "C" int ferhip_inter_encoding(ferhip_ctx *c)
{
    if (!c) return FERHIP_E_ARG;
    (void)hipSetDevice(c->device);
    set_all_types(c, 0);
    if (!c->refprep_valid) fer_launch_refprep(c->d, c->sort, nullptr, c->st);
    c->refprep_valid = true;
    {
        ProfScope ps(c, FERHIP_PH_ME_PRE, 1);
        fer_launch_me_pre(c->d, c->st);
    }
    {
        ProfScope ps(c, FERHIP_PH_ME_WALK, 1);
        fer_launch_me_walk(c->d, c->st);
    }
    if (c->d.speculate) {
        ProfScope ps(c, FERHIP_PH_ME_SPEC, 1);
        fer_launch_me_spec(c->d, c->st);
    }
    {
        ProfScope ps(c, FERHIP_PH_ME_RESOLVE, 1);
        c->d.serial = c->d.serial % 0x7ffffff0 + 1;
        fer_launch_me_resolve(c->d, c->st);
    }
    fer_launch_basic_stat(c->d, c->st);
    fer_launch_p_resid(c->d, c->st);  // partition merge + mvd share the residual wavefront of the macroblock
    fer_launch_type_count(c->d, c->st);
    CK(hipStreamSynchronize(c->st));
    CK(hipGetLastError());
    return 0;
}

extern "C" size_t ferhip_read_buffer(ferhip_ctx *c, int which, void *dst, size_t cap)
{
    if (!c || !dst) return 0;
    (void)hipSetDevice(c->device);
    if (ctx_sync(c) != hipSuccess) return 0;
    FerDev &d = c->d;
    size_t nm = (size_t)d.nmb * d.S;
    const void *src = nullptr;
    size_t n = 0;
    switch (which) {
    case FERHIP_BUF_INTERP: {  // the planes without their margins
        n = d.ysz * 16 * d.S;
        if (n > cap) return 0;
        for (int pl = 0; pl < 16 * d.S; pl++)
            if (hipMemcpy2D((uint8_t *)dst + (size_t)pl * d.ysz, (size_t)d.W, d.interp + (size_t)pl * d.iplane + d.ioff, (size_t)d.ipitch,
                            (size_t)d.W, (size_t)d.H, hipMemcpyDeviceToHost) != hipSuccess)
                return 0;
        return n;
    }
    case FERHIP_BUF_FEAT: {
        // refFrameKar[0..4][frac] for every position: the searches derive what they need of it on chip, the full table
        // is built here on request from the interpolated planes (parity tests of row a16)
        n = d.ysz * 96 * d.S * 2;
        if (n > cap) return 0;
        if (dalloc(c, &d.feat, d.ysz * 96 * d.S)) return 0;
        if (hipDeviceSynchronize() != hipSuccess) return 0;
        fer_launch_features(d, c->st);
        src = d.feat;
        break;
    }
    case FERHIP_BUF_SORTPOS: src = d.sort_pos; n = d.ysz * d.S * 4; break;
    case FERHIP_BUF_KOLIKO: {  // the reference's koliko[] = first level of the bucket index, relative to the stream's segment
        n = (size_t)16385 * d.S * 4;
        if (n > cap) return 0;
        if (hipStreamSynchronize(c->st) != hipSuccess) return 0;
        for (int s = 0; s < d.S; s++) {
            int *o = (int *)dst + (size_t)s * 16385;
            if (hipMemcpy2D(o, 4, d.kol2 + (size_t)s * 16384 * d.kt, (size_t)d.kt * 4, 4, 16385, hipMemcpyDeviceToHost) != hipSuccess)
                return 0;
            for (int a = 0; a <= 16384; a++) o[a] -= (int)((size_t)s * d.ysz);
        }
        return n;
    }
    case FERHIP_BUF_MBTYPE: src = d.mb_type; n = nm * 4; break;
    case FERHIP_BUF_MV: src = d.mv; n = nm * 16; break;
    case FERHIP_BUF_MVD: src = d.mvd; n = nm * 16; break;
    case FERHIP_BUF_LEVELS: src = d.levels; n = nm * FER_LEVELS * 2; break;
    case FERHIP_BUF_CBP: src = d.cbp; n = nm * 2; break;
    case FERHIP_BUF_TC: src = d.tc; n = nm * 24; break;
    case FERHIP_BUF_I4MODE: src = d.i4mode; n = nm * 16; break;
    case FERHIP_BUF_TIMING: src = d.timing; n = 64 * 8; break;
    case FERHIP_BUF_ST2N: src = d.st2n; n = nm * 16; break;
    case FERHIP_BUF_SUMA: src = d.suma; n = nm * 4 * 5 * 4; break;
    case FERHIP_BUF_ST3: src = d.st3; n = nm * 4 * 33 * 3 * 4; break;
    case FERHIP_BUF_ST3N: src = d.st3n; n = nm * 16; break;
    case FERHIP_BUF_V0: src = d.v0; n = nm * 16; break;
    case FERHIP_BUF_SPEC_HDR: src = d.spec_hdr; n = nm * 4 * 16; break;
    case FERHIP_BUF_SPEC_L1: src = d.spec_l1; n = nm * 4 * 17 * 8; break;
    case FERHIP_BUF_SPEC_L2: src = d.spec_l2; n = nm * 4 * 33 * 8; break;
    case FERHIP_BUF_ST2: src = d.st2; n = nm * 4 * FER_ST2_CAP * 8; break;
    case FERHIP_BUF_SPEC_STAT: {  // the four totals over the workgroups' slots, then four zero words
        n = 8 * 8;
        if (n > cap) return 0;
        if (hipStreamSynchronize(c->st) != hipSuccess) return 0;
        std::vector<unsigned long long> slots((size_t)4 * d.spec_slots);
        if (hipMemcpy(slots.data(), d.spec_stat, slots.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
        unsigned long long tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < slots.size(); i++) tot[i & 3] += slots[i];
        memcpy(dst, tot, n);
        return n;
    }
    case FERHIP_BUF_MBSIZE: src = d.mbsize; n = nm * 8; break;
    case FERHIP_BUF_CUR:
    case FERHIP_BUF_REF: {
        n = d.ysz * 3 / 2 * d.S;
        if (n > cap) return 0;
        uint8_t *set = c->planes[which == FERHIP_BUF_CUR ? c->cur_set : c->cur_set ^ 1];
        if (copy_frames(c, set, nullptr, (uint8_t *)dst, hipMemcpyDeviceToHost)) return 0;
        if (hipStreamSynchronize(c->st) != hipSuccess) return 0;
        return n;
    }
    default: return 0;
    }
    if (n > cap) return 0;
    if (hipStreamSynchronize(c->st) != hipSuccess) return 0;
    if (hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
}

