// fer_decode_host.hip -- the decoder's host driver: decode() / RBSP_decode() of F/fer_h264.cpp:26-53,
// F/rbsp_decoding.cpp:17-367.  Annex-B scan + emulation-prevention removal (F/nal.cpp:68-223), parameter sets and slice
// header (F/headers_and_parameter_sets.cpp:245-298,398-537) -- a few dozen bits per NAL -- then windows of pictures through
// the device's macroblock loop (fer_decode.hip).  ferhip_decode_streams, the streaming decoder (ferhip_dec_*) and the
// live decoder with per-stream fault isolation (ferhip_decs_*) share one session type over a decode-only context.
#include "fer_nalsplit.h"
#include "fer_pic_host.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <mutex>
#include <thread>
#include <utility>

struct HostBR {
    const uint8_t *b;
    size_t n, pos;
    unsigned bit()
    {
        size_t by = pos >> 3;
        unsigned v = by < n ? (b[by] >> (7 - (pos & 7))) & 1u : 0u;
        pos++;
        return v;
    }
    unsigned bits(int k)
    {
        unsigned v = 0;
        for (int i = 0; i < k; i++) v = (v << 1) | bit();
        return v;
    }
    unsigned ue()
    {
        int z = 0;
        while (z < 24 && bit() == 0) z++;  // the reference searches a 24-bit window (F/expgolomb.cpp:122)
        return (1u << z) - 1u + bits(z);
    }
    int se()
    {
        int v = (int)ue();
        return (v & 1) ? (v + 1) / 2 : -v / 2;
    }
};

struct DecHdr {
    int have_sps, have_pps, W, H, log2_max_frame_num, poc_type, log2_max_poc_lsb;
    int pic_init_qp, chroma_qp_offset, deblock_ctl, constrained_intra;
    // slice-header state the reference keeps in globals between slices: the active reference count is only ever set
    // by an override (never reset to the PPS default), the list-modification flag and its entry count only by P slices
    int nref_active_minus1, mod_flag, mod_copies;
    int crop[4];  // frame cropping of the SPS in luma samples: left, right, top, bottom (zeros = none)
};

// seq_parameter_set_rbsp, F/headers_and_parameter_sets.cpp:398-470.  Returns 0, or FERHIP_E_UNSUP for syntax the
// slice parser does not implement (the reference would mis-decode it silently).
static int dec_parse_sps(DecHdr &h, HostBR &r)
{
    const unsigned profile_idc = r.bits(8);
    r.bits(16);
    r.ue();
    if (profile_idc >= 100) return FERHIP_E_UNSUP;  // High profiles carry chroma_format_idc ... here
    h.log2_max_frame_num = (int)r.ue() + 4;
    h.poc_type = (int)r.ue();
    h.log2_max_poc_lsb = 0;
    if (h.poc_type == 0) {
        h.log2_max_poc_lsb = (int)r.ue() + 4;
    } else if (h.poc_type == 1) {
        r.bits(1);
        r.se();
        r.se();
        int n = (int)r.ue();
        for (int i = 0; i < n; i++) r.se();
    }
    r.ue();
    r.bits(1);
    int wmb = (int)r.ue() + 1, hmu = (int)r.ue() + 1, fmo = (int)r.bits(1);
    if (!fmo) return FERHIP_E_UNSUP;  // field / MBAFF coding
    h.W = wmb * 16;
    h.H = hmu * 16;
    h.have_sps = 1;
    // The reference stops here.  direct_8x8_inference_flag, then the frame cropping: offsets in units of two luma samples
    // (4:2:0, frame_mbs_only).  Cropping is information for the caller (ferhip_decs_get_crop) and never a reason to refuse a
    // stream: an SPS that ends before the offsets do, or whose offsets leave no picture, counts as uncropped.
    h.crop[0] = h.crop[1] = h.crop[2] = h.crop[3] = 0;
    r.bits(1);
    if (r.bits(1)) {
        unsigned o[4];
        for (int k = 0; k < 4; k++) o[k] = r.ue();
        const bool whole = r.pos < r.n * 8;  // vui_parameters_present_flag and the stop bit still follow
        if (whole && (unsigned long long)o[0] + o[1] < (unsigned)h.W / 2u && (unsigned long long)o[2] + o[3] < (unsigned)h.H / 2u)
            for (int k = 0; k < 4; k++) h.crop[k] = (int)(o[k] * 2u);
    }
    return 0;
}

// pic_parameter_set_rbsp, F/headers_and_parameter_sets.cpp:520-537
static int dec_parse_pps(DecHdr &h, HostBR &r)
{
    r.ue();
    r.ue();
    if (r.bits(1)) return FERHIP_E_UNSUP;  // entropy_coding_mode_flag: CABAC
    r.bits(1);
    if (r.ue() > 0) return FERHIP_E_UNSUP;  // slice groups
    if (r.ue() > 0) return FERHIP_E_UNSUP;  // num_ref_idx_l0_default_active_minus1: several reference indices
    r.ue();
    r.bits(3);
    h.pic_init_qp = r.se() + 26;
    r.se();
    h.chroma_qp_offset = r.se();
    h.deblock_ctl = (int)r.bits(1);
    h.constrained_intra = (int)r.bits(1);
    h.have_pps = 1;
    return 0;
}

// slice header -> info[4] = {rbsp bytes, first bit of slice_data, slice_type % 5, SliceQPy}; returns 0 or error
static int dec_parse_slice_header(DecHdr &h, const uint8_t *rbsp, size_t n, int nal_type, int ref_idc, uint32_t *info,
                                  int &override_flag)
{
    if (!h.have_sps || !h.have_pps) return FERHIP_E_STATE;
    HostBR r{rbsp, n, 0};
    r.ue();
    int st = (int)r.ue() % 5;
    r.ue();
    r.bits(h.log2_max_frame_num);
    if (nal_type == 5) r.ue();
    r.bits(h.log2_max_poc_lsb);
    if (st == 0 || st == 1 || st == 3) {
        override_flag = (int)r.bits(1);
        if (override_flag) h.nref_active_minus1 = (int)r.ue();  // only tells the macroblock layer whether ref_idx is coded
    }
    if (st != 2 && st != 4) {  // ref_pic_list_modification (F/headers_and_parameter_sets.cpp:196-215)
        h.mod_flag = (int)r.bits(1);
        h.mod_copies = 0;
        if (h.mod_flag) {
            unsigned idc;
            int guard = 0;
            do {
                idc = r.ue();
                if (idc <= 2) {
                    r.ue();
                    h.mod_copies++;
                }
            } while (idc != 3 && ++guard < 64 && r.pos < n * 8);
        }
    }
    if (ref_idc != 0) {
        if (nal_type == 5) {
            r.bits(2);
        } else if (r.bits(1)) {
            unsigned op;
            do {
                op = r.ue();
                if (op == 1 || op == 3) r.ue();
                if (op == 2) r.ue();
                if (op == 3 || op == 6) r.ue();
                if (op == 4) r.ue();
            } while (op != 0);
        }
    }
    int qp = h.pic_init_qp + r.se();
    if (h.deblock_ctl == 1) {
        if (r.ue() != 1) {
            r.se();
            r.se();
        }
    }
    if (st != 0 && st != 2) return FERHIP_E_UNSUP;
    info[0] = (uint32_t)n;
    info[1] = (uint32_t)r.pos;
    // slice type | ref_idx coded in sub-macroblock prediction (the reference tests the override FLAG there,
    // F/rbsp_decoding.cpp:156) << 8 | active reference count - 1 (what it tests in mb_pred, :217) << 16
    info[2] = (uint32_t)st | ((uint32_t)(override_flag ? 1 : 0) << 8) | ((uint32_t)std::min(h.nref_active_minus1, 255) << 16);
    info[3] = (uint32_t)qp;
    return 0;
}

// split an Annex-B stream like findNALstart/findNALend/parseNAL (4-byte start codes only)
struct ByteView {  // bytes owned elsewhere: a stream's RBSP store (split_stream) or the caller's buffer (ferhip_dec_nal)
    const uint8_t *p = nullptr;
    size_t n = 0;
    const uint8_t *data() const { return p; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
};
struct NalRef {
    int type, ref_idc;
    ByteView rbsp;
    // a unit the device splitter left in the decoder's store (ferhip_decs_decode_dev): its RBSP is dev_n bytes at `dev`, and
    // rbsp holds the first min(dev_n, FER_SPLIT_PREFIX) of them (all of them once the unit was fetched whole)
    const uint8_t *dev = nullptr;
    size_t dev_n = 0;
};
// next position i in [from, n - 2) with s[i] == 0, s[i+1] == 0 and s[i+2] in `third` (two allowed values), or npos;
// zero bytes are rare in entropy-coded data, so the scan is driven by memchr
static size_t find_zz(const uint8_t *s, size_t from, size_t n, uint8_t t0, uint8_t t1)
{
    while (from + 2 < n) {
        const uint8_t *p = (const uint8_t *)memchr(s + from, 0, n - 2 - from);
        if (!p) break;
        size_t i = (size_t)(p - s);
        if (s[i + 1] == 0 && (s[i + 2] == t0 || s[i + 2] == t1)) return i;
        from = i + 1;
    }
    return (size_t)-1;
}
// s[from..en) without every s[p] = 03 with s[p-2] = s[p-1] = 0 and p - 2 >= from (the emulation prevention byte of every
// 00 00 03), appended at w; returns the new end
static uint8_t *unescape_rbsp(const uint8_t *s, size_t from, size_t en, uint8_t *w)
{
    for (;;) {
        size_t z = find_zz(s, from, en, 3, 3);
        if (z == (size_t)-1) break;
        memcpy(w, s + from, z + 2 - from);
        w += z + 2 - from;
        from = z + 3;
    }
    if (from < en) {
        memcpy(w, s + from, en - from);
        w += en - from;
    }
    return w;
}

// `store` receives the RBSP of every NAL unit back to back (never more than the stream itself) and must outlive `out`
static void split_stream(const uint8_t *s, size_t n, std::vector<NalRef> &out, std::vector<uint8_t> &store)
{
    if (store.size() < n) store.resize(n);
    uint8_t *w = store.data();
    size_t pos = 0;
    for (;;) {
        size_t st = (size_t)-1;
        for (size_t i = pos; i + 3 < n;) {  // 00 00 00 01
            size_t z = find_zz(s, i, n - 1, 0, 0);
            if (z == (size_t)-1) break;
            if (s[z + 3] == 1) {
                st = z + 4;
                break;
            }
            i = z + 1;
        }
        if (st == (size_t)-1) break;
        size_t en = find_zz(s, st, n, 0, 1);
        if (en == (size_t)-1) en = n;
        pos = en;
        if (en <= st) continue;
        NalRef nal;
        nal.ref_idc = (s[st] & 0x7f) >> 5;
        nal.type = s[st] & 0x1f;
        uint8_t *w0 = w;
        w = unescape_rbsp(s, st + 1, en, w);
        nal.rbsp.p = w0;
        nal.rbsp.n = (size_t)(w - w0);
        if (nal.rbsp.empty()) break;
        out.push_back(std::move(nal));
    }
}

// split a length-prefixed range (every unit behind its length of L = 1, 2 or 4 bytes, big-endian; the definition: ferhip.h)
// like split_stream; an empty unit, one without payload and one that overruns the range end it.  Returns 1 if it overran.
static int split_avcc(const uint8_t *s, size_t n, int L, std::vector<NalRef> &out, std::vector<uint8_t> &store)
{
    if (store.size() < n) store.resize(n);
    uint8_t *w = store.data();
    size_t pos = 0;
    while (n - pos >= (size_t)L) {
        size_t len = 0;
        for (int k = 0; k < L; k++) len = len << 8 | s[pos + k];
        const size_t st = pos + L;
        if (len == 0) return 0;
        if (len > n - st) return 1;
        if (len == 1) return 0;
        const size_t en = st + len;
        NalRef nal;
        nal.ref_idc = (s[st] & 0x7f) >> 5;
        nal.type = s[st] & 0x1f;
        uint8_t *w0 = w;
        w = unescape_rbsp(s, st + 1, en, w);
        nal.rbsp.p = w0;
        nal.rbsp.n = (size_t)(w - w0);
        out.push_back(std::move(nal));
        pos = en;
    }
    return pos < n;  // fewer than L bytes are left: a unit that cannot state its length
}

// Window buffers of the decode twin.  ferhip_decode_streams keeps one arena per process between calls (releasing
// tens of GB costs more than a window's reconstruction); it is tied to the HIP device it was allocated on and
// can be dropped with ferhip_decode_release().  A streaming decoder (ferhip_dec_*) owns a small one of its own.
struct DecArena {
    void *dev = nullptr;
    size_t bytes = 0;
    int device = -1;
    uint8_t *d_rbsp = nullptr, *h_rbsp = nullptr;  // slices of a window: device buffer and pinned staging
    size_t rbsp_cap = 0;
    bool busy = false, cached = false;
};
static DecArena g_dec_arena;
static std::mutex g_dec_arena_mu;
static thread_local std::vector<std::vector<uint8_t>> tl_rbsp_store;  // ferhip_decode_streams: the streams' RBSP, per calling thread
static void dec_arena_free(DecArena *a)
{
    if (a->dev) hipFree(a->dev);
    if (a->d_rbsp) hipFree(a->d_rbsp);
    if (a->h_rbsp) hipHostFree(a->h_rbsp);
    a->dev = nullptr;
    a->d_rbsp = a->h_rbsp = nullptr;
    a->bytes = a->rbsp_cap = 0;
    a->device = -1;
}
static DecArena *dec_arena_acquire(size_t need, int device, bool use_cache)
{
    DecArena *a = nullptr;
    if (use_cache) {
        std::lock_guard<std::mutex> lk(g_dec_arena_mu);
        if (!g_dec_arena.busy) {
            a = &g_dec_arena;
            a->busy = true;
            a->cached = true;
        }
    }
    if (!a) {
        a = new DecArena();
        a->busy = true;
    }
    if (a->device != device && a->device >= 0) {  // allocated on another device: its pointers are useless here
        int cur = device;
        (void)hipSetDevice(a->device);
        dec_arena_free(a);
        (void)hipSetDevice(cur);
    }
    a->device = device;
    if (a->bytes < need) {
        if (a->dev) hipFree(a->dev);
        a->dev = nullptr;
        a->bytes = 0;
        if (hipMalloc(&a->dev, need) != hipSuccess) {
            (void)hipGetLastError();
            a->dev = nullptr;
            std::lock_guard<std::mutex> lk(g_dec_arena_mu);
            if (a->cached)
                a->busy = false;
            else
                delete a;
            return nullptr;
        }
        a->bytes = need;
    }
    return a;
}
static void dec_arena_release(DecArena *a)
{
    if (!a) return;
    if (a->cached) {
        std::lock_guard<std::mutex> lk(g_dec_arena_mu);
        a->busy = false;
    } else {
        dec_arena_free(a);
        delete a;
    }
}

extern "C" int ferhip_decode_release(void)
{
    std::vector<std::vector<uint8_t>>().swap(tl_rbsp_store);
    std::lock_guard<std::mutex> lk(g_dec_arena_mu);
    if (g_dec_arena.busy) return FERHIP_E_STATE;
    if (g_dec_arena.device >= 0) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(g_dec_arena.device);
        dec_arena_free(&g_dec_arena);
        (void)hipSetDevice(cur);
    }
    return 0;
}

// One decoding session: S streams of one picture size, a window of up to TWmax pictures per stream parsed by one
// launch, parameter sets and the state the reference keeps in globals (mb_qp_delta, ChromaACLevel) per stream.
struct DecSession {
    ferhip_ctx *c = nullptr;
    int S = 0;
    std::vector<DecHdr> hs;  // parameter sets of every stream (the QP of this codec lives in the PPS)
    DecArena *ar = nullptr;
    DecBatch B;
    uint32_t *d_info = nullptr;
    size_t TWmax = 0, nm = 0, fsz = 0;
    std::vector<uint32_t> info, hdr;
    std::vector<char> anyP, anyAny, keep, pres;  // pres[t * S + s]: stream s has a picture at step t of the window
    // A picture whose slice carries an empty reference-list modification is NOT stored as the reference picture
    // (modificationProcess, F/ref_frames.cpp:130-183): the stream's last decoded picture (what `frame` holds, what a
    // slice that ends early leaves in place) then differs from its reference picture and waits in `hold`.
    uint8_t *hold = nullptr;
    std::vector<char> held;
    double t_pack = 0, t_parse = 0, t_recon = 0;
    const uint8_t *dev_rbsp = nullptr;  // the device splitter's store: where the `dev` units of a window lie
    std::vector<uint8_t> whole;         // a device unit whose slice header runs past its prefix, fetched to be parsed again
};

static double dec_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static void dec_session_close(DecSession &ss)
{
    if (ss.c) {
        (void)hipSetDevice(ss.c->device);
        hipStreamSynchronize(ss.c->st);
    }
    dec_arena_release(ss.ar);
    ss.ar = nullptr;
    if (ss.hold) hipFree(ss.hold);
    ss.hold = nullptr;
    if (ss.c) ferhip_destroy(ss.c);
    ss.c = nullptr;
}

// T = pictures per stream the caller expects (sizes the window); use_cache = take the process-wide arena
static int dec_session_open(DecSession &ss, int W, int H, int S, size_t T, bool use_cache)
{
    ferhip_params p = {26, 0, 16, 3, 1 << 30};
    int rc = ctx_create(&ss.c, W, H, S, &p, true);
    if (rc) return rc;
    FerDev &d = ss.c->d;
    ss.S = S;
    ss.nm = (size_t)S * d.nmb;
    ss.fsz = (size_t)W * H * 3 / 2;
    const size_t nm = ss.nm;
    const size_t per_pic = nm * (4 + 16 + 2 + 24 + 16 + 16 + 1 + FER_LEVELS * 2 + 1 + 1);
    size_t budget = (size_t)48e9, freeb = 0, totalb = 0;
    if (hipMemGetInfo(&freeb, &totalb) == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_dec_arena_mu);
        if (use_cache && !g_dec_arena.busy && g_dec_arena.device == ss.c->device) freeb += g_dec_arena.bytes;
        budget = std::min(budget, freeb / 2);
    }
    size_t TWmax = std::min<size_t>(std::max<size_t>(budget / per_pic, 1), 256);
    TWmax = std::max<size_t>(std::min(TWmax, T), 1);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    uint8_t *base = nullptr;
    size_t sizes[16];
    for (;;) {  // halve the window until its buffers fit
        const size_t sz[16] = {TWmax * nm * 4, TWmax * nm * 16, TWmax * nm * 2, TWmax * nm * 24, TWmax * nm * 16, TWmax * nm * 16,
                               TWmax * nm, TWmax * nm * FER_LEVELS * 2, TWmax * nm, TWmax * nm, TWmax * S * 16, TWmax * S * 16,
                               TWmax * S * 16, TWmax * S * 256, TWmax * S * 256, TWmax * S * 24};
        size_t need = 0;
        for (int i = 0; i < 16; i++) {
            sizes[i] = sz[i];
            need += up(sz[i]) + 256;
        }
        ss.ar = dec_arena_acquire(need, ss.c->device, use_cache);
        if (ss.ar) break;
        if (TWmax == 1) {
            dec_session_close(ss);
            return FERHIP_E_HIP;
        }
        TWmax = (TWmax + 1) / 2;
    }
    ss.TWmax = TWmax;
    base = (uint8_t *)ss.ar->dev;
    size_t off = 0;
    auto wmalloc = [&](size_t bytes) -> void * {
        void *v = base + off;
        off += up(bytes) + 256;
        return v;
    };
    DecBatch &B = ss.B;
    B.mb_type = (int *)wmalloc(sizes[0]);
    B.mv = (short *)wmalloc(sizes[1]);
    B.cbp = (uint8_t *)wmalloc(sizes[2]);
    B.tc = (uint8_t *)wmalloc(sizes[3]);
    B.i4mode = (uint8_t *)wmalloc(sizes[4]);
    B.i4flag = (uint8_t *)wmalloc(sizes[5]);
    B.chroma_mode = (uint8_t *)wmalloc(sizes[6]);
    B.levels = (int16_t *)wmalloc(sizes[7]);
    B.dec_qp = (uint8_t *)wmalloc(sizes[8]);
    B.carry = (uint8_t *)wmalloc(sizes[9]);
    B.hdr = (uint32_t *)wmalloc(sizes[10]);
    B.state = (int *)wmalloc(sizes[11]);
    B.summ = (int *)wmalloc(sizes[12]);
    B.cac_in = (int16_t *)wmalloc(sizes[13]);
    B.cac_out = (int16_t *)wmalloc(sizes[14]);
    ss.d_info = (uint32_t *)wmalloc(sizes[15]);
    ss.hs.assign(S, DecHdr{});
    ss.held.assign(S, 0);
    return 0;
}

// the three planes of stream s from one plane-major picture set to another (same stream order)
static int dec_copy_stream(ferhip_ctx *c, uint8_t *dst, const uint8_t *src, int s)
{
    const FerDev &d = c->d;
    const size_t S = (size_t)d.S;
    const size_t off[3] = {(size_t)s * d.ysz, S * d.ysz + (size_t)s * d.csz, S * (d.ysz + d.csz) + (size_t)s * d.csz};
    const size_t len[3] = {d.ysz, d.csz, d.csz};
    for (int k = 0; k < 3; k++)
        if (hipMemcpyAsync(dst + off[k], src + off[k], len[k], hipMemcpyDeviceToDevice, c->st) != hipSuccess) return FERHIP_E_HIP;
    return 0;
}

// Per-stream error isolation of a window (the live decoder, ferhip_decs_*).  Without it the first stream that fails
// fails the window.  With it a stream's fault ends that stream's part of the window: the faulted picture and the ones
// after it are not reconstructed, status[s] records the FERHIP_E_* and the other streams go on.  The output then goes
// through k_dec_out or k_pic_emit, which write only the slots of pictures that were decoded.
struct DecIsolate {
    int *status = nullptr;       // [S] 0, or the first fault of stream s in this call
    std::vector<char> stop;      // [S] stream s faulted inside a window: it takes no more pictures in this call
    uint8_t *out = nullptr;      // [max_pictures][S][fsz]: picture k of stream s at (k * S + s) * fsz, or NULL
    bool out_dev = false;        // out is device memory
    int2 *d_map = nullptr;       // [TWmax][S] device: the (stream, slot) pairs of every step for the output kernel
    std::vector<int2> map;       // ... host side
    std::vector<int> nmap;       // [TW] pairs per step
    std::vector<size_t> fin;     // host output: slot (k * S + s) of the caller's buffer of every staged picture, in order
    uint8_t *d_stage = nullptr, *h_stage = nullptr;  // host output: the window's pictures, packed, on the device and pinned
    size_t stage_cap = 0;        // pictures
    // ferhip_decs_set_display: the window (x0, y0, dw, dh) of every picture that goes to `out`; ofsz = bytes of one slot
    int win[4] = {};
    size_t ofsz = 0;
    // ferhip_decs_set_layout: the slots of device output are pitched I420 or NV12 (k_pic_emit) or a packed format
    // (k_pic_emit_packed); layout_set stays false on a decoder that never makes the call, and the slots are then tight I420
    bool layout_set = false;
    int fmt = FERHIP_FMT_I420;
    uint32_t pitch_y = 0, pitch_c = 0;
    int csc = FERHIP_CSC_BT601;  // ferhip_decs_set_csc: the matrix of a BGRA / RGBA layout
    uint32_t row_y() const { return layout_set ? pitch_y : (uint32_t)win[2]; }
    uint32_t row_c() const { return layout_set ? pitch_c : (uint32_t)win[2] / 2u; }
    // a layout other than tight I420 slots of the window: it needs device output and a check of its pitches
    bool own_layout() const { return !(fmt == FERHIP_FMT_I420 && row_y() == (uint32_t)win[2] && row_c() == (uint32_t)win[2] / 2u); }
    // whole coded pictures as tight I420 at a 16-byte aligned address: k_dec_out's case
    bool whole(const FerDev &d, const uint8_t *to) const { return !own_layout() && win[2] == d.W && win[3] == d.H && !((uintptr_t)to & 15u); }
};

// After the parse of an isolated window: find each faulted stream's first faulted picture (B.state[pic * 4 + 3]), drop it
// and the stream's later pictures from the window (macroblocks reached = 0, so the reconstruction leaves them alone),
// clear the sticky status, then lay out the output of the pictures that remain.  pictures[s] = pictures of stream s
// before this window.
static int dec_isolate_faults(DecSession &ss, size_t TW, DecIsolate &iso, const int *pictures)
{
    ferhip_ctx *c = ss.c;
    const int S = ss.S;
    bool any = false;
    for (int s = 0; s < S; s++) any |= c->h_status[s] != 0;
    if (any) {
        std::vector<int> st(TW * S * 4);
        if (hipMemcpyAsync(st.data(), ss.B.state, st.size() * 4, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
            hipStreamSynchronize(c->st) != hipSuccess)
            return FERHIP_E_HIP;
        for (int s = 0; s < S; s++) {
            if (!c->h_status[s]) continue;
            bool hit = false;
            for (size_t t = 0; t < TW; t++) {
                const size_t pic = t * S + s;
                if (!ss.pres[pic]) continue;
                if (!hit && st[pic * 4 + 3]) {
                    hit = true;
                    iso.stop[s] = 1;
                    iso.status[s] = (st[pic * 4 + 3] & FER_ERR_DEC_UNSUPPORTED) ? FERHIP_E_UNSUP : FERHIP_E_DEVICE;
                }
                if (hit) {
                    ss.pres[pic] = 0;
                    st[pic * 4 + 1] = 0;
                }
            }
            if (!hit) return FERHIP_E_HIP;  // a status bit without a faulted picture: the device state is not to be trusted
        }
        if (hipMemcpyAsync(ss.B.state, st.data(), st.size() * 4, hipMemcpyHostToDevice, c->st) != hipSuccess ||
            hipMemsetAsync(c->d.status, 0, sizeof(int) * S, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess)
            return FERHIP_E_HIP;
        for (size_t t = 0; t < TW; t++) {
            ss.anyP[t] = ss.anyAny[t] = 0;
            for (int s = 0; s < S; s++)
                if (ss.pres[t * S + s]) {
                    ss.anyAny[t] = 1;
                    ss.anyP[t] |= ss.hdr[(t * S + s) * 4 + 3] == 0;
                }
        }
    }
    if (!iso.out) return 0;
    // output: step t writes map[t * S + k], k < nmap[t] = (stream, slot); the slot is the caller's (picture * S + stream)
    // for device output, the next free picture of the staging buffer for host output
    iso.map.resize(TW * S);
    iso.nmap.assign(TW, 0);
    iso.fin.clear();
    for (size_t t = 0; t < TW; t++)
        for (int s = 0; s < S; s++) {
            if (!ss.pres[t * S + s]) continue;
            const size_t slot = (size_t)(pictures[s] + (int)t) * S + s;
            int2 &e = iso.map[t * S + iso.nmap[t]++];
            e.x = s;
            e.y = iso.out_dev ? (int)slot : (int)iso.fin.size();
            if (!iso.out_dev) iso.fin.push_back(slot);
        }
    if (!iso.out_dev && iso.fin.size() > iso.stage_cap) {  // grows to the largest window seen, then stays
        if (iso.d_stage) hipFree(iso.d_stage);
        if (iso.h_stage) hipHostFree(iso.h_stage);
        iso.d_stage = iso.h_stage = nullptr;
        iso.stage_cap = 0;
        const size_t cap = std::min(std::max(iso.fin.size(), (size_t)S), ss.TWmax * S);
        if (hipMalloc((void **)&iso.d_stage, cap * iso.ofsz) != hipSuccess || hipHostMalloc((void **)&iso.h_stage, cap * iso.ofsz) != hipSuccess)
            return FERHIP_E_HIP;
        iso.stage_cap = cap;
    }
    if (hipMemcpyAsync(iso.d_map, iso.map.data(), TW * S * sizeof(int2), hipMemcpyHostToDevice, c->st) != hipSuccess) return FERHIP_E_HIP;
    return 0;
}

// Decode pictures [t0, t0 + TW) of every stream: slices[s][t] = the slice NAL of picture t of stream s (streams may
// be shorter; nullptr = no picture at that step).  out (host, may be NULL) receives picture t of stream s at
// (t * S + s) * fsz; pictures[s] counts.  iso: see DecIsolate (out is then unused).
static int dec_session_window(DecSession &ss, const std::vector<std::vector<const NalRef *>> &slices, size_t t0, size_t TW,
                              uint8_t *out, int *pictures, DecIsolate *iso = nullptr)
{
    ferhip_ctx *c = ss.c;
    FerDev &d = c->d;
    const int S = ss.S;
    const size_t nm = ss.nm;
    DecBatch &B = ss.B;
    DecArena *ar = ss.ar;
    double ta = dec_now();
    ss.info.assign(TW * S * 6, 0);
    ss.hdr.assign(TW * S * 4, 0);
    ss.anyP.assign(TW, 0);
    ss.anyAny.assign(TW, 0);
    ss.keep.assign(TW * S, 1);
    ss.pres.assign(TW * S, 0);
    // slice headers and the offsets of the slices in the window's RBSP buffer
    size_t total = 0;
    bool on_dev = false;  // the window's slices lie in the device splitter's store (a call's units are all of one kind)
    for (size_t t = 0; t < TW; t++)
        for (int s = 0; s < S; s++) {
            uint32_t *in = &ss.info[(t * S + s) * 6];
            uint32_t *hd = &ss.hdr[(t * S + s) * 4];
            hd[3] = 2;
            if (t0 + t >= slices[s].size() || !slices[s][t0 + t] || (iso && iso->stop[s])) continue;
            const NalRef &n = *slices[s][t0 + t];
            const size_t full = n.dev ? n.dev_n : n.rbsp.size();
            int ov = 0;
            const DecHdr before = ss.hs[s];
            int rc = dec_parse_slice_header(ss.hs[s], n.rbsp.data(), n.rbsp.size(), n.type, n.ref_idc, in, ov);
            if (full > n.rbsp.size() && (rc || in[1] > n.rbsp.size() * 8)) {
                // the header is longer than the prefix that came back with the table: this unit is fetched whole and
                // parsed again from the state in front of it
                ss.whole.resize(full);
                if (hipMemcpyAsync(ss.whole.data(), n.dev, full, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
                    hipStreamSynchronize(c->st) != hipSuccess)
                    return FERHIP_E_HIP;
                ss.hs[s] = before;
                ov = 0;
                rc = dec_parse_slice_header(ss.hs[s], ss.whole.data(), full, n.type, n.ref_idc, in, ov);
            }
            in[0] = rc ? in[0] : (uint32_t)full;
            // a header that runs past the end of its NAL unit, or a SliceQPY outside 0..51: damaged
            if (!rc && iso && (in[1] > full * 8 || in[3] > 51)) rc = FERHIP_E_ARG;
            if (rc) {
                if (!iso) return rc;
                iso->status[s] = rc;
                iso->stop[s] = 1;
                for (int k = 0; k < 6; k++) in[k] = 0;
                continue;
            }
            ss.pres[t * S + s] = 1;
            if (n.dev) {  // parsed where the splitter left it
                const size_t at = (size_t)(n.dev - ss.dev_rbsp);
                in[4] = (uint32_t)at;
                in[5] = (uint32_t)((unsigned long long)at >> 32);
                on_dev = true;
            } else {
                in[4] = (uint32_t)total;
                in[5] = (uint32_t)(total >> 32);
                total += (n.rbsp.size() + 15) & ~(size_t)15;
            }
            // what the kernels need of this stream's PPS travels with the picture
            hd[0] = (uint32_t)ss.hs[s].chroma_qp_offset;
            hd[1] = (uint32_t)ss.hs[s].constrained_intra;
            hd[3] = in[2] & 255u;
            ss.anyP[t] |= (in[2] & 255u) == 0;
            ss.anyAny[t] = 1;
            ss.keep[t * S + s] = !ss.hs[s].mod_flag || ss.hs[s].mod_copies > 0;
        }
    if (!on_dev && total + 64 > ar->rbsp_cap) {
        if (ar->d_rbsp) hipFree(ar->d_rbsp);
        if (ar->h_rbsp) hipHostFree(ar->h_rbsp);
        ar->d_rbsp = ar->h_rbsp = nullptr;
        ar->rbsp_cap = total + total / 4 + 4096;
        if (hipMalloc((void **)&ar->d_rbsp, ar->rbsp_cap) != hipSuccess || hipHostMalloc((void **)&ar->h_rbsp, ar->rbsp_cap) != hipSuccess) {
            ar->rbsp_cap = 0;
            return FERHIP_E_HIP;
        }
    }
    if (!on_dev) {  // gather the slices into the pinned staging buffer with a few threads, then one H2D copy
        const int nth = std::max(1, std::min(std::min(S, 16), (int)std::thread::hardware_concurrency()));
        auto gather = [&](int k) {
            for (int s = k; s < S; s += nth)
                for (size_t t = 0; t < TW; t++) {
                    if (!ss.pres[t * S + s]) continue;
                    const NalRef &n = *slices[s][t0 + t];
                    const uint32_t *in = &ss.info[(t * S + s) * 6];
                    memcpy(ar->h_rbsp + (((size_t)in[5] << 32) | in[4]), n.rbsp.data(), n.rbsp.size());
                }
        };
        if (nth == 1) {
            gather(0);
        } else {
            std::vector<std::thread> th;
            for (int k = 0; k < nth; k++) th.emplace_back(gather, k);
            for (auto &x : th) x.join();
        }
    }
    if ((!on_dev && hipMemcpyAsync(ar->d_rbsp, ar->h_rbsp, total, hipMemcpyHostToDevice, c->st) != hipSuccess) ||
        hipMemcpyAsync(ss.d_info, ss.info.data(), ss.info.size() * 4, hipMemcpyHostToDevice, c->st) != hipSuccess ||
        hipMemcpyAsync(B.hdr, ss.hdr.data(), ss.hdr.size() * 4, hipMemcpyHostToDevice, c->st) != hipSuccess)
        return FERHIP_E_HIP;
    B.TW = (int)TW;
    B.rbsp = on_dev ? ss.dev_rbsp : ar->d_rbsp;
    B.info = ss.d_info;
    ss.t_pack += dec_now() - ta;
    ta = dec_now();
    fer_launch_decode_parse(d, B, c->st);
    // the host vectors above are read by the copies when they execute: the synchronisation below covers them
    if (hipMemcpyAsync(c->h_status, d.status, sizeof(int) * S, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
        hipStreamSynchronize(c->st) != hipSuccess || hipGetLastError() != hipSuccess)
        return FERHIP_E_HIP;
    if (iso) {
        int rc = dec_isolate_faults(ss, TW, *iso, pictures);
        if (rc) return rc;
    } else {
        for (int s = 0; s < S; s++)
            if (c->h_status[s]) {
                fprintf(stderr, "ferhip: stream %d decode status 0x%x\n", s, c->h_status[s]);
                return (c->h_status[s] & FER_ERR_DEC_UNSUPPORTED) ? FERHIP_E_UNSUP : FERHIP_E_DEVICE;
            }
    }
    ss.t_parse += dec_now() - ta;
    ta = dec_now();
    for (size_t t = 0; t < TW; t++) {
        if (!ss.anyAny[t]) break;
        // `frame` keeps the previous picture where the parser does not reach (F/rbsp_decoding.cpp:77)
        if (hipMemcpyAsync(c->planes[c->cur_set], c->planes[c->cur_set ^ 1], d.ysz * 3 / 2 * S, hipMemcpyDeviceToDevice, c->st) !=
            hipSuccess)
            return FERHIP_E_HIP;
        for (int s = 0; s < S; s++)  // ... which, for a stream whose last picture was not stored as reference, waits in `hold`
            if (ss.held[s] && (!iso || ss.pres[t * S + s]) && dec_copy_stream(c, c->planes[c->cur_set], ss.hold, s)) return FERHIP_E_HIP;
        FerDev ds = d;  // this picture's slice of the window
        const size_t o = t * nm;
        ds.mb_type = B.mb_type + o;
        ds.mv = B.mv + o * 8;
        ds.cbp = B.cbp + o * 2;
        ds.tc = B.tc + o * 24;
        ds.i4mode = B.i4mode + o * 16;
        ds.i4flag = B.i4flag + o * 16;
        ds.chroma_mode = B.chroma_mode + o;
        ds.levels = B.levels + o * FER_LEVELS;
        ds.dec_qp = B.dec_qp + o;
        ds.hdr = B.hdr + t * S * 4;
        ds.dec_state = B.state + t * S * 4;
        fer_launch_decode_recon(ds, ss.anyP[t] != 0, true, c->st);
        c->cur_set ^= 1;  // the decoded picture becomes the reference (modificationProcess -> frameDeepCopy)
        bind_planes(c);
        if (iso && iso->out) {  // (the staged pictures of host output are tight slots)
            uint8_t *to = iso->out_dev ? iso->out : iso->d_stage;
            const uint8_t *set = c->planes[c->cur_set ^ 1];
            const int2 *map = iso->d_map + t * S;
            const uint32_t py = iso->row_y(), pc = iso->row_c();
            const size_t slot = fer_pic_slot_bytes(iso->fmt, py, pc, (uint32_t)iso->win[3]);
            if (fer_pic_packed(iso->fmt))
                fer_launch_pic_emit_packed(d, set, nullptr, map, iso->nmap[t], to, iso->fmt, iso->csc, py, slot, iso->win, c->st);
            else if (iso->whole(d, to))
                fer_launch_decode_out(d, set, map, iso->nmap[t], to, c->st);
            else
                fer_launch_pic_emit_slots(d, set, map, iso->nmap[t], to, iso->fmt, py, pc, slot, iso->win, c->st);
        } else if (!iso && out) {
            uint8_t *row = out + (t0 + t) * S * ss.fsz;
            bool all = true;
            for (int s = 0; s < S; s++) all &= ss.pres[t * S + s] != 0;
            if (all) {
                int rc = ferhip_get_recon(c, row, 1);
                if (rc) return rc;
            } else {
                // a stream that has ended has no picture at this step: its slot of `out` keeps what the caller put there
                const uint8_t *set = c->planes[c->cur_set ^ 1];
                for (int s = 0; s < S; s++) {
                    if (!ss.pres[t * S + s]) continue;
                    const size_t off[3] = {(size_t)s * d.ysz, (size_t)S * d.ysz + (size_t)s * d.csz,
                                           (size_t)S * (d.ysz + d.csz) + (size_t)s * d.csz};
                    uint8_t *f = row + (size_t)s * ss.fsz;
                    if (hipMemcpyAsync(f, set + off[0], d.ysz, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
                        hipMemcpyAsync(f + d.ysz, set + off[1], d.csz, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
                        hipMemcpyAsync(f + d.ysz + d.csz, set + off[2], d.csz, hipMemcpyDeviceToHost, c->st) != hipSuccess)
                        return FERHIP_E_HIP;
                }
                if (hipStreamSynchronize(c->st) != hipSuccess) return FERHIP_E_HIP;
            }
        }
        for (int s = 0; s < S; s++) {
            if (!ss.pres[t * S + s]) continue;
            if (!ss.keep[t * S + s]) {
                // not stored: the picture moves to `hold`, the stream's reference picture (still intact in the other
                // set) moves back into the reference set
                if (!ss.hold) {
                    if (hipMalloc((void **)&ss.hold, d.ysz * 3 / 2 * S + 256) != hipSuccess) return FERHIP_E_HIP;
                }
                if (dec_copy_stream(c, ss.hold, c->planes[c->cur_set ^ 1], s) ||
                    dec_copy_stream(c, c->planes[c->cur_set ^ 1], c->planes[c->cur_set], s))
                    return FERHIP_E_HIP;
                ss.held[s] = 1;
            } else {
                ss.held[s] = 0;
            }
        }
        if (pictures)
            for (int s = 0; s < S; s++)
                if (ss.pres[t * S + s]) pictures[s]++;
    }
    size_t staged = 0;
    if (iso && iso->out && !iso->out_dev) {
        for (size_t t = 0; t < TW; t++) staged += (size_t)iso->nmap[t];
        if (staged && hipMemcpyAsync(iso->h_stage, iso->d_stage, staged * iso->ofsz, hipMemcpyDeviceToHost, c->st) != hipSuccess)
            return FERHIP_E_HIP;
    }
    if (hipStreamSynchronize(c->st) != hipSuccess || hipGetLastError() != hipSuccess) return FERHIP_E_HIP;
    if (staged) {  // the staged pictures to their slots of the caller's buffer (nothing else of it is written)
        const size_t fsz = iso->ofsz;
        auto scatter = [&](size_t j0, size_t j1) {
            for (size_t j = j0; j < j1; j++) memcpy(iso->out + iso->fin[j] * fsz, iso->h_stage + j * fsz, fsz);
        };
        const size_t nth = std::min<size_t>(std::min<size_t>(staged * fsz >> 23, 16), std::max(1u, std::thread::hardware_concurrency()));
        if (nth <= 1) {
            scatter(0, staged);
        } else {
            std::vector<std::thread> th;
            for (size_t k = 0; k < nth; k++) th.emplace_back(scatter, staged * k / nth, staged * (k + 1) / nth);
            for (auto &x : th) x.join();
        }
    }
    ss.t_recon += dec_now() - ta;
    return 0;
}

// decode() for S Annex-B streams side by side.  All streams must carry the same picture size.
// out: host [T][S][W*H*3/2] (T = max_pictures); pictures[s] = pictures decoded of stream s.
extern "C" int ferhip_decode_streams(const uint8_t *const *streams, const size_t *lens, int S, uint8_t *out,
                                     int max_pictures, int *pictures, int *W_out, int *H_out)
{
    if (!streams || !lens || S <= 0 || !pictures) return FERHIP_E_ARG;
    if (out && max_pictures <= 0) return FERHIP_E_ARG;  // `out` holds max_pictures pictures per stream: its size must be known
    const bool verbose = getenv("FER_DEC_TIMING") != nullptr;
    double t_start = dec_now();
    std::vector<std::vector<NalRef>> nals(S);
    // the RBSP of every stream, kept by the calling thread between calls like the device arena: 240 MB of fresh heap per
    // call (128 1080p GOPs) cost 0.25 s in page faults and unmapping, a fifth of the decode itself
    std::vector<std::vector<uint8_t>> &rbsp_store = tl_rbsp_store;
    if ((int)rbsp_store.size() < S) rbsp_store.resize(S);
    {  // NAL splitting is host work per stream: spread it over a few threads
        const int nth = std::max(1, std::min(std::min(S, 16), (int)std::thread::hardware_concurrency()));
        std::vector<std::thread> th;
        std::vector<std::vector<uint8_t>> &store = rbsp_store;
        for (int k = 0; k < nth; k++)
            th.emplace_back([&, k]() {
                for (int s = k; s < S; s += nth) split_stream(streams[s], lens[s], nals[s], store[s]);
            });
        for (auto &x : th) x.join();
    }
    // parameter sets per stream (the last SPS / PPS of a stream wins, as in the reference, which keeps one of each)
    std::vector<DecHdr> hs(S, DecHdr{});
    for (int s = 0; s < S; s++) {
        for (auto &n : nals[s]) {
            HostBR r{n.rbsp.data(), n.rbsp.size(), 0};
            int rc = 0;
            if (n.type == 7)
                rc = dec_parse_sps(hs[s], r);
            else if (n.type == 8)
                rc = dec_parse_pps(hs[s], r);
            if (rc) return rc;
        }
        if (!hs[s].have_sps || !hs[s].have_pps) return FERHIP_E_ARG;
        if (hs[s].W != hs[0].W || hs[s].H != hs[0].H) return FERHIP_E_ARG;
    }
    if (W_out) *W_out = hs[0].W;
    if (H_out) *H_out = hs[0].H;
    const double t_split = dec_now();
    // the slice NALs of every stream, in order
    std::vector<std::vector<const NalRef *>> slices(S);
    size_t T = 0;
    for (int s = 0; s < S; s++) {
        for (auto &n : nals[s])
            if (n.type == 1 || n.type == 5) slices[s].push_back(&n);
        T = std::max(T, slices[s].size());
        pictures[s] = 0;
    }
    if (max_pictures > 0) T = std::min(T, (size_t)max_pictures);
    for (int s = 0; s < S; s++)
        if (slices[s].size() > T) slices[s].resize(T);
    DecSession ss;
    int rc = dec_session_open(ss, hs[0].W, hs[0].H, S, T, true);
    if (rc) return rc;
    ss.hs = hs;
    const double t_open = dec_now();
    // Slice data is bit-serial, so the parser's parallelism is pictures: a window of TW pictures of all streams is
    // parsed by one launch (one wavefront each), then reconstructed picture by picture.
    for (size_t t0 = 0; t0 < T && rc == 0; t0 += ss.TWmax) rc = dec_session_window(ss, slices, t0, std::min(ss.TWmax, T - t0), out, pictures);
    if (verbose)
        fprintf(stderr, "ferhip_decode_streams: %d streams, %zu pictures, window %zu: split %.3f s, context + buffers %.3f s, "
                        "pack+H2D %.3f s, parse %.3f s, reconstruction %.3f s\n", S, T, ss.TWmax, t_split - t_start, t_open - t_split,
                ss.t_pack, ss.t_parse, ss.t_recon);
#ifdef FER_PROBE
    {
        long long tm[64];
        hipDeviceSynchronize();
        hipMemcpy(tm, ss.c->d.timing, sizeof tm, hipMemcpyDeviceToHost);
        double n = tm[52] > 0 ? (double)tm[52] : 1.0;
        fprintf(stderr, "k_dec_parse stream 0: %lld MBs, us per MB: header %.2f residual %.2f tail %.2f skip/loop %.2f\n", tm[52],
                tm[48] / n / 100, tm[49] / n / 100, tm[50] / n / 100, tm[51] / n / 100);
    }
#endif
    const double t_free0 = dec_now();
    dec_session_close(ss);
    if (verbose) fprintf(stderr, "ferhip_decode_streams: release %.3f s, total %.3f s\n", dec_now() - t_free0, dec_now() - t_start);
    return rc;
}

// ---- streaming decoder: RBSP_decode(NALunit) of F/rbsp_decoding.cpp:17 for one stream, NAL unit by NAL unit ----
struct ferhip_dec {
    DecSession ss;
    DecHdr h{};
    bool open = false;
    int pictures = 0;
};

extern "C" int ferhip_dec_create(ferhip_dec **out)
{
    if (!out) return FERHIP_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        fprintf(stderr, "ferhip: no HIP device; the hot path has no CPU fallback\n");
        return FERHIP_E_HIP;
    }
    *out = new ferhip_dec();
    return 0;
}

extern "C" void ferhip_dec_destroy(ferhip_dec *dc)
{
    if (!dc) return;
    if (dc->open) dec_session_close(dc->ss);
    delete dc;
}

extern "C" int ferhip_dec_nal(ferhip_dec *dc, int nal_unit_type, int nal_ref_idc, const uint8_t *rbsp, size_t n, uint8_t *picture,
                              int *got_picture, int *width, int *height)
{
    if (!dc || !rbsp || n == 0) return FERHIP_E_ARG;
    if (got_picture) *got_picture = 0;
    HostBR r{rbsp, n, 0};
    if (nal_unit_type == 7) {  // fill_sps + init_h264_structures + AllocateMemory
        DecHdr hn = dc->h;
        int rc = dec_parse_sps(hn, r);
        if (rc) return rc;
        if (dc->open && (hn.W != dc->h.W || hn.H != dc->h.H)) {
            dec_session_close(dc->ss);
            dc->open = false;
        }
        dc->h = hn;
        if (!dc->open) {
            dc->ss = DecSession();
            rc = dec_session_open(dc->ss, hn.W, hn.H, 1, 1, false);
            if (rc) return rc;
            dc->open = true;
        }
    } else if (nal_unit_type == 8) {
        int rc = dec_parse_pps(dc->h, r);
        if (rc) return rc;
    } else if (nal_unit_type == 5 || nal_unit_type == 1) {
        if (!dc->open) return FERHIP_E_STATE;
        (void)hipSetDevice(dc->ss.c->device);
        dc->ss.hs[0] = dc->h;
        NalRef nal;
        nal.type = nal_unit_type;
        nal.ref_idc = nal_ref_idc;
        nal.rbsp.p = rbsp;
        nal.rbsp.n = n;
        std::vector<std::vector<const NalRef *>> slices(1);
        slices[0].push_back(&nal);
        int rc = dec_session_window(dc->ss, slices, 0, 1, picture, nullptr);
        if (rc) return rc;
        dc->h = dc->ss.hs[0];  // the slice header leaves state behind (reference count override, list modification)
        dc->pictures++;
        if (got_picture) *got_picture = 1;
    }  // every other NAL unit type (SEI, AUD ...) is ignored, as in the reference
    if (width) *width = dc->h.W;
    if (height) *height = dc->h.H;
    return 0;
}

// ---- live decoder: S streams that arrive piece by piece, one window of all of them per call ----
struct ferhip_decs {
    DecSession ss;
    int S = 0, W = 0, H = 0, P = 0;
    std::vector<std::vector<uint8_t>> store;  // RBSP of each stream's chunk (kept between calls)
    std::vector<std::vector<NalRef>> nals;
    std::vector<size_t> cursor;               // next NAL unit of each stream's chunk
    std::vector<int> queued;                  // slice NAL units taken from each stream's chunk in this call
    std::vector<char> need_idr;               // after a fault: P slices are refused until an IDR slice
    DecIsolate iso;
    FerSplit split;                           // ferhip_decs_decode_dev: the splitter's buffers and the store of the units' RBSP
    std::vector<std::vector<uint8_t>> whole;  // ... parameter sets longer than the prefix, fetched whole
    int in_format = FERHIP_IN_ANNEXB, length_size = 4;  // ferhip_decs_set_input
    std::vector<int> overrun;                 // [S] AVCC input: the stream's chunk of this call overran
    double t_split = 0;                       // seconds in the host splitter
};

// Stream s back to the state of a new decoder; forget_ps = also forget its parameter sets, else keep them and refuse
// P slices until the next IDR slice
static int decs_reset(ferhip_decs *d, int s, bool forget_ps)
{
    ferhip_ctx *c = d->ss.c;
    const FerDev &dv = c->d;
    const size_t S = (size_t)d->S;
    hipError_t e = hipMemsetAsync(dv.dec_state + s * 4, 0, 4 * sizeof(int), c->st);
    if (e == hipSuccess) e = hipMemsetAsync(dv.dec_cac + s * 128, 0, 128 * sizeof(int16_t), c->st);
    if (e == hipSuccess) e = hipMemsetAsync(dv.status + s, 0, sizeof(int), c->st);
    const size_t off[3] = {(size_t)s * dv.ysz, S * dv.ysz + (size_t)s * dv.csz, S * (dv.ysz + dv.csz) + (size_t)s * dv.csz};
    const size_t len[3] = {dv.ysz, dv.csz, dv.csz};
    for (int set = 0; set < 2; set++)
        for (int k = 0; k < 3 && e == hipSuccess; k++) e = hipMemsetAsync(c->planes[set] + off[k], 0, len[k], c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) return FERHIP_E_HIP;
    d->ss.held[s] = 0;
    DecHdr &h = d->ss.hs[s];
    if (forget_ps) {
        h = DecHdr{};
    } else {
        h.nref_active_minus1 = h.mod_flag = h.mod_copies = 0;
    }
    d->need_idr[s] = !forget_ps;
    return 0;
}

extern "C" int ferhip_decs_create(ferhip_decs **out, int nstreams, int width, int height, int max_pictures)
{
    if (!out) return FERHIP_E_ARG;
    *out = nullptr;
    if (nstreams <= 0 || width <= 0 || height <= 0 || width % 16 || height % 16 || max_pictures <= 0) return FERHIP_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        fprintf(stderr, "ferhip: no HIP device; the hot path has no CPU fallback\n");
        return FERHIP_E_HIP;
    }
    ferhip_decs *d = new ferhip_decs();
    int rc = dec_session_open(d->ss, width, height, nstreams, (size_t)max_pictures, false);
    if (rc) {
        delete d;
        return rc;
    }
    d->S = nstreams;
    d->W = width;
    d->H = height;
    d->P = max_pictures;
    d->store.resize(nstreams);
    d->nals.resize(nstreams);
    d->cursor.assign(nstreams, 0);
    d->queued.assign(nstreams, 0);
    d->need_idr.assign(nstreams, 0);
    d->overrun.assign(nstreams, 0);
    d->iso.win[2] = width;
    d->iso.win[3] = height;
    d->iso.ofsz = d->ss.fsz;
    if (hipMalloc((void **)&d->iso.d_map, d->ss.TWmax * nstreams * sizeof(int2)) != hipSuccess) {
        ferhip_decs_destroy(d);
        return FERHIP_E_HIP;
    }
    *out = d;
    return 0;
}

extern "C" void ferhip_decs_destroy(ferhip_decs *d)
{
    if (!d) return;
    if (d->ss.c) {
        (void)hipSetDevice(d->ss.c->device);
        hipStreamSynchronize(d->ss.c->st);
    }
    if (d->iso.d_map) hipFree(d->iso.d_map);
    if (d->iso.d_stage) hipFree(d->iso.d_stage);
    if (d->iso.h_stage) hipHostFree(d->iso.h_stage);
    fer_split_free(d->split);
    dec_session_close(d->ss);
    delete d;
}

extern "C" int ferhip_decs_reset_stream(ferhip_decs *d, int s)
{
    if (!d || s < 0 || s >= d->S) return FERHIP_E_ARG;
    (void)hipSetDevice(d->ss.c->device);
    return decs_reset(d, s, true);
}

// frame cropping of stream s's current SPS, in luma samples: left, right, top, bottom
extern "C" int ferhip_decs_get_crop(ferhip_decs *d, int s, int crop[4])
{
    if (!d || !crop || s < 0 || s >= d->S) return FERHIP_E_ARG;
    const DecHdr &h = d->ss.hs[s];
    if (!h.have_sps) return FERHIP_E_STATE;
    for (int k = 0; k < 4; k++) crop[k] = h.crop[k];
    return 0;
}

// From the next decode call on `out` holds the window (x0, y0, dw, dh) of every picture; (0, 0, W, H) is today's path
extern "C" int ferhip_decs_set_display(ferhip_decs *d, int x0, int y0, int dw, int dh)
{
    if (!d || x0 < 0 || y0 < 0 || dw < 2 || dh < 2 || ((x0 | y0 | dw | dh) & 1) || x0 > d->W - dw || y0 > d->H - dh) return FERHIP_E_ARG;
    DecIsolate &iso = d->iso;
    const size_t ofsz = (size_t)dw * dh * 3 / 2;
    if (ofsz != iso.ofsz) {  // the staging buffers of host output are sized in slots: they are made again at the next call
        (void)hipSetDevice(d->ss.c->device);
        if (iso.d_stage) hipFree(iso.d_stage);
        if (iso.h_stage) hipHostFree(iso.h_stage);
        iso.d_stage = iso.h_stage = nullptr;
        iso.stage_cap = 0;
    }
    iso.win[0] = x0;
    iso.win[1] = y0;
    iso.win[2] = dw;
    iso.win[3] = dh;
    iso.ofsz = ofsz;
    return 0;
}

// From the next decode call on the slots of `out` are pitched I420 or NV12; the pitches are checked against the window
// when a decode call is made (decs_layout_check), since ferhip_decs_set_display may change it in between
extern "C" int ferhip_decs_set_layout(ferhip_decs *d, int format, uint32_t pitch_y, uint32_t pitch_c)
{
    if (!d || (format != FERHIP_FMT_I420 && format != FERHIP_FMT_NV12 && !fer_pic_packed(format))) return FERHIP_E_ARG;
    d->iso.layout_set = true;
    d->iso.fmt = format;
    d->iso.pitch_y = pitch_y;
    d->iso.pitch_c = pitch_c;
    return 0;
}

// the matrix of a BGRA / RGBA output layout (FERHIP_CSC_*), from the next decode call on
extern "C" int ferhip_decs_set_csc(ferhip_decs *d, int matrix)
{
    if (!d || (matrix != FERHIP_CSC_BT601 && matrix != FERHIP_CSC_BT709)) return FERHIP_E_ARG;
    d->iso.csc = matrix;
    return 0;
}

// a layout other than the default: device output only, and pitches that hold a row of the current window; a packed format
// is written in aligned dwords, so its slots must start at multiples of 4
static int decs_layout_check(const ferhip_decs *d, const uint8_t *out, int out_on_device)
{
    const DecIsolate &iso = d->iso;
    if (!iso.own_layout()) return 0;
    if (!out_on_device) return FERHIP_E_ARG;
    if (fer_pic_packed(iso.fmt) && ((uintptr_t)out & 3u)) return FERHIP_E_ARG;
    return fer_pic_layout_check(iso.fmt, iso.pitch_y, iso.pitch_c, (uint32_t)iso.win[2]);  // (the internal tight pitches never get here)
}

extern "C" int ferhip_decs_set_input(ferhip_decs *d, int format, int length_size)
{
    if (!d || (format != FERHIP_IN_ANNEXB && format != FERHIP_IN_AVCC)) return FERHIP_E_ARG;
    if (format == FERHIP_IN_AVCC) {
        if (length_size != 1 && length_size != 2 && length_size != 4) return FERHIP_E_ARG;
        d->length_size = length_size;
    }
    d->in_format = format;
    return 0;
}

// one parameter set of stream s: it replaces the stream's current one only if it parses and keeps the decoder's picture size
static int decs_param_set(ferhip_decs *d, int s, int type, const uint8_t *rbsp, size_t n)
{
    DecHdr hn = d->ss.hs[s];
    HostBR r{rbsp, n, 0};
    int rc = type == 7 ? dec_parse_sps(hn, r) : dec_parse_pps(hn, r);
    if (!rc && type == 7 && (hn.W != d->W || hn.H != d->H)) rc = FERHIP_E_UNSUP;  // one picture size per decoder
    if (!rc) d->ss.hs[s] = hn;
    return rc;
}

// AVCDecoderConfigurationRecord -> the SPS units, then the PPS units, to stream s as if they had come in a chunk
extern "C" int ferhip_decs_set_config(ferhip_decs *d, int s, const uint8_t *avcc, size_t n)
{
    if (!d || !avcc || s < 0 || s >= d->S || n < 7 || avcc[0] != 1) return FERHIP_E_ARG;
    if (d->in_format == FERHIP_IN_AVCC && (avcc[4] & 3) + 1 != d->length_size) return FERHIP_E_ARG;
    struct Span { size_t at, len; };
    std::vector<Span> units;
    size_t pos = 5, longest = 0;
    for (int pass = 0; pass < 2; pass++) {  // numOfSequenceParameterSets (5 bits), numOfPictureParameterSets
        if (pos >= n) return FERHIP_E_ARG;
        const int count = pass ? avcc[pos] : avcc[pos] & 31;
        pos++;
        if (count == 0) return FERHIP_E_ARG;
        for (int k = 0; k < count; k++) {
            if (n - pos < 2) return FERHIP_E_ARG;
            const size_t len = (size_t)avcc[pos] << 8 | avcc[pos + 1];
            pos += 2;
            if (len == 0 || len > n - pos) return FERHIP_E_ARG;
            units.push_back({pos, len});
            longest = std::max(longest, len);
            pos += len;
        }
    }
    if (hipSetDevice(d->ss.c->device) != hipSuccess) return FERHIP_E_HIP;
    std::vector<uint8_t> rbsp(longest);
    for (const Span &u : units) {
        const int type = avcc[u.at] & 0x1f;
        if (type != 7 && type != 8) continue;  // ignored, as in a chunk
        const size_t m = (size_t)(unescape_rbsp(avcc, u.at + 1, u.at + u.len, rbsp.data()) - rbsp.data());
        if (m == 0) break;  // a unit without payload ends a chunk
        if (int rc = decs_param_set(d, s, type, rbsp.data(), m)) {
            // the stream's fault, as in a chunk: it restarts at its next IDR slice
            if (int rr = decs_reset(d, s, false)) return rr;
            return rc;
        }
    }
    return 0;
}

// Take stream s's next NAL units up to the first parameter set that follows a slice (that one belongs to the next
// window: a slice is parsed with the parameter sets that precede it), appending its slices to `slices`.
static void decs_take(ferhip_decs *d, int s, std::vector<const NalRef *> &slices, int *status)
{
    DecHdr &h = d->ss.hs[s];
    std::vector<NalRef> &nals = d->nals[s];
    for (size_t &i = d->cursor[s]; i < nals.size() && !status[s]; i++) {
        const NalRef &n = nals[i];
        if (n.type == 7 || n.type == 8) {
            if (!slices.empty()) return;
            if (int rc = decs_param_set(d, s, n.type, n.rbsp.data(), n.rbsp.size())) status[s] = rc;
        } else if (n.type == 1 || n.type == 5) {
            if (!h.have_sps || !h.have_pps || (n.type == 1 && d->need_idr[s]))
                status[s] = FERHIP_E_STATE;
            else if (d->queued[s] >= d->P)
                status[s] = FERHIP_E_ARG;
            else {
                slices.push_back(&n);
                d->queued[s]++;
                if (n.type == 5) d->need_idr[s] = 0;
            }
        }  // every other NAL unit type (SEI, AUD ...) is ignored, as in the reference
    }
}

static int decs_run(ferhip_decs *d, uint8_t *out, int out_on_device, int *pictures, int *status);

// a call starts from empty results and empty unit lists; returns the bytes of its chunks (NULL / 0 = no chunk)
static size_t decs_begin_call(ferhip_decs *d, const uint8_t *const *chunks, const size_t *lens, int *pictures, int *status)
{
    size_t bytes = 0;
    for (int s = 0; s < d->S; s++) {
        pictures[s] = status[s] = 0;
        d->nals[s].clear();
        d->cursor[s] = 0;
        d->queued[s] = 0;
        d->overrun[s] = 0;
        if (chunks[s] && lens[s]) bytes += lens[s];
    }
    return bytes;
}

extern "C" int ferhip_decs_decode(ferhip_decs *d, const uint8_t *const *chunks, const size_t *lens, uint8_t *out, int out_on_device,
                                  int *pictures, int *status)
{
    if (!d || !chunks || !lens || !pictures || !status || decs_layout_check(d, out, out_on_device)) return FERHIP_E_ARG;
    const int S = d->S;
    if (hipSetDevice(d->ss.c->device) != hipSuccess) return FERHIP_E_HIP;
    const size_t bytes = decs_begin_call(d, chunks, lens, pictures, status);
    const double ts = dec_now();
    {  // NAL splitting: a few threads when there is much of it
        const int nth = bytes < ((size_t)1 << 20) ? 1 : std::max(1, std::min(std::min(S, 16), (int)std::thread::hardware_concurrency()));
        auto split = [&](int k) {
            for (int s = k; s < S; s += nth) {
                if (!chunks[s] || !lens[s]) continue;
                if (d->in_format == FERHIP_IN_AVCC)
                    d->overrun[s] = split_avcc(chunks[s], lens[s], d->length_size, d->nals[s], d->store[s]);
                else
                    split_stream(chunks[s], lens[s], d->nals[s], d->store[s]);
            }
        };
        if (nth == 1) {
            split(0);
        } else {
            std::vector<std::thread> th;
            for (int k = 0; k < nth; k++) th.emplace_back(split, k);
            for (auto &x : th) x.join();
        }
    }
    d->t_split += dec_now() - ts;
    return decs_run(d, out, out_on_device, pictures, status);
}

extern "C" int ferhip_decs_decode_dev(ferhip_decs *d, const uint8_t *const *d_chunks, const size_t *lens, uint8_t *out,
                                      int out_on_device, int *pictures, int *status)
{
    if (!d || !d_chunks || !lens || !pictures || !status || decs_layout_check(d, out, out_on_device)) return FERHIP_E_ARG;
    const int S = d->S;
    ferhip_ctx *c = d->ss.c;
    if (hipSetDevice(c->device) != hipSuccess) return FERHIP_E_HIP;
    if (!decs_begin_call(d, d_chunks, lens, pictures, status)) return 0;
    // range s = the chunk of stream s: one set of launches splits them all into the decoder's store
    const bool avcc = d->in_format == FERHIP_IN_AVCC;
    int rc = fer_split_run(d->split, c->st, d_chunks, lens, S, nullptr, 0, avcc ? d->length_size : 0);
    if (rc) return rc;
    const FerSplit &sp = d->split;
    for (int s = 0; avcc && s < S; s++) d->overrun[s] = sp.h_fault[s];
    d->whole.clear();
    rc = fer_split_each_unit(sp, [&](size_t k, const ferhip_nal_unit &u) -> int {
        NalRef n;
        n.type = u.nal_type;
        n.ref_idc = u.ref_idc;
        n.dev = sp.d_store + u.offset;
        n.dev_n = u.bytes;
        n.rbsp.p = sp.prefix(k);
        n.rbsp.n = std::min<size_t>(u.bytes, FER_SPLIT_PREFIX);
        if ((n.type == 7 || n.type == 8) && n.dev_n > n.rbsp.n) {  // a parameter set longer than the prefix
            d->whole.emplace_back(n.dev_n);
            if (hipMemcpyAsync(d->whole.back().data(), n.dev, n.dev_n, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
                hipStreamSynchronize(c->st) != hipSuccess)
                return FERHIP_E_HIP;
            n.rbsp.p = d->whole.back().data();  // (the vector's buffer stays where it is when `whole` grows)
            n.rbsp.n = n.dev_n;
        }
        d->nals[u.range].push_back(n);
        return 0;
    });
    if (rc) return rc;
    d->ss.dev_rbsp = sp.d_store;
    return decs_run(d, out, out_on_device, pictures, status);
}

extern "C" int ferhip_decs_timing(ferhip_decs *d, double *t, int reset)
{
    if (!d || !t) return FERHIP_E_ARG;
    t[0] = d->t_split;
    t[1] = d->ss.t_pack;
    t[2] = d->ss.t_parse;
    t[3] = d->ss.t_recon;
    t[4] = d->split.ms * 1e-3;
    t[5] = (double)d->split.in_bytes;
    if (reset) {
        d->t_split = d->ss.t_pack = d->ss.t_parse = d->ss.t_recon = d->split.ms = 0;
        d->split.in_bytes = 0;
    }
    return 0;
}

// the chunks of a call are split into d->nals: take them window by window
static int decs_run(ferhip_decs *d, uint8_t *out, int out_on_device, int *pictures, int *status)
{
    const int S = d->S;
    d->iso.status = status;
    d->iso.stop.assign(S, 0);
    d->iso.out = out;
    d->iso.out_dev = out_on_device != 0;
    std::vector<std::vector<const NalRef *>> slices(S);
    int rc = 0;
    for (;;) {  // one window per call, unless a chunk carries a parameter set behind one of its slices
        size_t T = 0;
        for (int s = 0; s < S; s++) {
            slices[s].clear();
            decs_take(d, s, slices[s], status);
            T = std::max(T, slices[s].size());
        }
        if (T == 0) break;
        for (size_t t0 = 0; t0 < T && !rc; t0 += d->ss.TWmax) rc = dec_session_window(d->ss, slices, t0, std::min(d->ss.TWmax, T - t0), nullptr, pictures, &d->iso);
        if (rc) break;
    }
    for (int s = 0; s < S && !rc; s++) {
        // a chunk that overran (AVCC input): its units in front of the overrun were taken, then the stream faults
        if (d->overrun[s] && !status[s]) status[s] = FERHIP_E_ARG;
        if (status[s]) rc = decs_reset(d, s, false);
    }
    return rc;
}
