// fer_dec_session.hip -- the decode session (fer_dec_session.h): the window arena, open / close, and one window of pictures
// through fer_decode.hip as a list of steps.  decode() / RBSP_decode() of F/fer_h264.cpp:26-53, F/rbsp_decoding.cpp:17-367.
#include "fer_dec_session.h"
#include <mutex>

// The process-wide arena lives behind a pointer that is never deleted: its buffers' destructors must not run at exit,
// when the HIP runtime may be gone.
static DecArena &g_dec_arena = *new DecArena();
static std::mutex g_dec_arena_mu;
thread_local std::vector<std::vector<uint8_t>> tl_rbsp_store;
// frees the arena's buffers on its own device, then makes `back` the current one
static void dec_arena_free(DecArena *a, int back)
{
    (void)hipSetDevice(a->device);
    a->dev.release();
    a->d_rbsp.release();
    a->h_rbsp.release();
    a->device = -1;
    (void)hipSetDevice(back);
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
    if (a->device != device && a->device >= 0) dec_arena_free(a, device);  // its pointers are useless on this device
    a->device = device;
    if (a->dev.reserve(need)) {
        std::lock_guard<std::mutex> lk(g_dec_arena_mu);
        if (a->cached)
            a->busy = false;
        else
            delete a;
        return nullptr;
    }
    return a;
}
extern "C" int ferhip_decode_release(void)
{
    std::vector<std::vector<uint8_t>>().swap(tl_rbsp_store);
    std::lock_guard<std::mutex> lk(g_dec_arena_mu);
    if (g_dec_arena.busy) return FERHIP_E_STATE;
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (g_dec_arena.device >= 0) dec_arena_free(&g_dec_arena, cur);
    return 0;
}
void dec_session_close(DecSession &ss)
{
    if (ss.c) {
        (void)hipSetDevice(ss.c->device);
        hipStreamSynchronize(ss.c->st);
    }
    if (ss.ar && ss.ar->cached) {
        std::lock_guard<std::mutex> lk(g_dec_arena_mu);
        ss.ar->busy = false;
    } else if (ss.ar) {
        dec_arena_free(ss.ar, ss.c->device);
        delete ss.ar;
    }
    ss.ar = nullptr;
    ss.hold.release();
    if (ss.c) ferhip_destroy(ss.c);
    ss.c = nullptr;
}

int dec_session_open(DecSession &ss, int W, int H, int S, size_t T, bool use_cache)
{
    ferhip_params p = {26, 0, 16, 3, 1 << 30};
    int rc = ctx_create(&ss.c, W, H, S, &p, true);
    if (rc) return rc;
    FerDev &d = ss.c->d;
    ss.S = S;
    ss.nm = (size_t)S * d.nmb;
    ss.fsz = (size_t)W * H * 3 / 2;
    ss.t_pack = ss.t_parse = ss.t_recon = 0;
    const size_t nm = ss.nm, nS = (size_t)S;
    const size_t per_pic = nm * (4 + 16 + 2 + 24 + 16 + 16 + 1 + FER_LEVELS * 2 + 1 + 1);
    size_t budget = (size_t)48e9, freeb = 0, totalb = 0;
    if (hipMemGetInfo(&freeb, &totalb) == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_dec_arena_mu);
        if (use_cache && !g_dec_arena.busy && g_dec_arena.device == ss.c->device) freeb += g_dec_arena.dev.cap;
        budget = std::min(budget, freeb / 2);
    }
    size_t TWmax = std::min<size_t>(std::max<size_t>(budget / per_pic, 1), 256);
    TWmax = std::max<size_t>(std::min(TWmax, T), 1);
    // bytes per picture of the window: the ten per-macroblock arrays of DecBatch, then hdr, state, summ, cac_in, cac_out, info
    const size_t per[16] = {nm * 4, nm * 16, nm * 2, nm * 24, nm * 16, nm * 16, nm, nm * FER_LEVELS * 2, nm, nm,
                            nS * 16, nS * 16, nS * 16, nS * 256, nS * 256, nS * 24};
    auto room = [&](int i) { return ((TWmax * per[i] + 255) & ~(size_t)255) + 256; };
    for (;;) {  // halve the window until its buffers fit
        size_t need = 0;
        for (int i = 0; i < 16; i++) need += room(i);
        ss.ar = dec_arena_acquire(need, ss.c->device, use_cache);
        if (ss.ar) break;
        if (TWmax == 1) {
            dec_session_close(ss);
            return FERHIP_E_HIP;
        }
        TWmax = (TWmax + 1) / 2;
    }
    ss.TWmax = TWmax;
    DecBatch &B = ss.B;  // the arena's parts, in the order of per[]
    void **const part[16] = {(void **)&B.mb_type, (void **)&B.mv, (void **)&B.cbp, (void **)&B.tc, (void **)&B.i4mode, (void **)&B.i4flag,
                             (void **)&B.chroma_mode, (void **)&B.levels, (void **)&B.dec_qp, (void **)&B.carry, (void **)&B.hdr,
                             (void **)&B.state, (void **)&B.summ, (void **)&B.cac_in, (void **)&B.cac_out, (void **)&ss.d_info};
    uint8_t *next = ss.ar->dev;
    for (int i = 0; i < 16; next += room(i++)) *part[i] = next;
    ss.hs.assign(S, DecHdr{});
    ss.held.assign(S, 0);
    return 0;
}

// the three planes of stream s from one plane-major picture set to another (same stream order)
static int dec_copy_stream(ferhip_ctx *c, uint8_t *dst, const uint8_t *src, int s)
{
    const PlaneSpans p = dec_stream_planes(c->d, s);
    for (int k = 0; k < 3; k++)
        if (hipMemcpyAsync(dst + p.off[k], src + p.off[k], p.len[k], hipMemcpyDeviceToDevice, c->st) != hipSuccess) return FERHIP_E_HIP;
    return 0;
}

// One call of dec_session_window: what it was given, what its steps leave for one another, and the steps in their order.
// Each returns 0 or the FERHIP_E_* that ends the window.
namespace {
struct DecWindow {
    DecSession &ss;
    const std::vector<std::vector<const NalRef *>> &slices;
    const size_t t0, TW;
    DecIsolate *const iso;
    ferhip_ctx *const c = ss.c;
    const int S = ss.S;
    size_t total = 0;     // bytes the slices take in the staging buffer, or
    bool on_dev = false;  // they lie in the device splitter's store (a call's units are all of one kind)
    // Headers: leaves info (header words and where each slice lies), hdr (what the kernels need of the stream's PPS), pres,
    // keep, anyP and anyAny of the window.  A unit at fault fails the window, or with iso its stream.
    int headers()
    {
        ss.info.assign(TW * S * 6, 0);
        ss.hdr.assign(TW * S * 4, 0);
        ss.anyP.assign(TW, 0);
        ss.anyAny.assign(TW, 0);
        ss.keep.assign(TW * S, 1);
        ss.pres.assign(TW * S, 0);
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
                const size_t at = n.dev ? (size_t)(n.dev - ss.dev_rbsp) : total;  // a device unit is parsed where the splitter left it
                in[4] = (uint32_t)at;
                in[5] = (uint32_t)((unsigned long long)at >> 32);
                if (n.dev)
                    on_dev = true;
                else
                    total += (n.rbsp.size() + 15) & ~(size_t)15;
                // what the kernels need of this stream's PPS travels with the picture
                hd[0] = (uint32_t)ss.hs[s].chroma_qp_offset;
                hd[1] = (uint32_t)ss.hs[s].constrained_intra;
                hd[3] = in[2] & 255u;
                ss.anyP[t] |= (in[2] & 255u) == 0;
                ss.anyAny[t] = 1;
                ss.keep[t * S + s] = !ss.hs[s].mod_flag || ss.hs[s].mod_copies > 0;
            }
        return 0;
    }

    // Stage: leaves the slices in device memory (gathered into the pinned staging buffer with a few threads, then one H2D
    // copy, unless they are there already), info and hdr on their way behind them, and B describing the window.  The host
    // vectors are read by the copies when they execute: the synchronisation after the parse covers them.
    int stage()
    {
        DecArena *ar = ss.ar;
        if (!on_dev) {
            const size_t want = total + total / 4 + 4096;
            if (ar->d_rbsp.reserve(total + 64, want) || ar->h_rbsp.reserve(total + 64, want)) return FERHIP_E_HIP;
            dec_fan_out((size_t)S, dec_stream_threads(S), [&](size_t s) {
                for (size_t t = 0; t < TW; t++) {
                    if (!ss.pres[t * S + s]) continue;
                    const NalRef &n = *slices[s][t0 + t];
                    const uint32_t *in = &ss.info[(t * S + s) * 6];
                    memcpy(ar->h_rbsp.p + (((size_t)in[5] << 32) | in[4]), n.rbsp.data(), n.rbsp.size());
                }
            });
        }
        if ((!on_dev && hipMemcpyAsync(ar->d_rbsp, ar->h_rbsp, total, hipMemcpyHostToDevice, c->st) != hipSuccess) ||
            hipMemcpyAsync(ss.d_info, ss.info.data(), ss.info.size() * 4, hipMemcpyHostToDevice, c->st) != hipSuccess ||
            hipMemcpyAsync(ss.B.hdr, ss.hdr.data(), ss.hdr.size() * 4, hipMemcpyHostToDevice, c->st) != hipSuccess)
            return FERHIP_E_HIP;
        ss.B.TW = (int)TW;
        ss.B.rbsp = on_dev ? ss.dev_rbsp : ar->d_rbsp.p;
        ss.B.info = ss.d_info;
        return 0;
    }

    // Parse and faults: leaves the window's macroblocks parsed (B) and every stream's status read.  A stream that faulted
    // fails the window.  With iso it leaves the window instead: its first faulted picture (B.state[pic * 4 + 3]) and its later
    // ones are dropped (macroblocks reached = 0, so the reconstruction leaves them alone) and the sticky status is cleared.
    int parse()
    {
        fer_launch_decode_parse(c->d, ss.B, c->st);
        if (hipMemcpyAsync(c->h_status, c->d.status, sizeof(int) * S, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
            hipStreamSynchronize(c->st) != hipSuccess || hipGetLastError() != hipSuccess)
            return FERHIP_E_HIP;
        bool any = false;
        for (int s = 0; s < S; s++) any |= c->h_status[s] != 0;
        if (!any) return 0;
        for (int s = 0; s < S && !iso; s++)
            if (c->h_status[s]) {
                fprintf(stderr, "ferhip: stream %d decode status 0x%x\n", s, c->h_status[s]);
                return (c->h_status[s] & FER_ERR_DEC_UNSUPPORTED) ? FERHIP_E_UNSUP : FERHIP_E_DEVICE;
            }
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
                    iso->stop[s] = 1;
                    iso->status[s] = (st[pic * 4 + 3] & FER_ERR_DEC_UNSUPPORTED) ? FERHIP_E_UNSUP : FERHIP_E_DEVICE;
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
        return 0;
    }

    // Picture t.  Begin: the previous picture of every stream goes to the current set, where the parser does not reach
    // (`frame`, F/rbsp_decoding.cpp:77) -- which, for a stream whose last picture was not stored as reference, waits in `hold`.
    // Reconstruct: the set that was current holds the picture and becomes the reference set (modificationProcess ->
    // frameDeepCopy).  Emit.  Store: a picture that is not stored as reference moves to `hold`, and the stream's reference
    // picture (still intact in the other set) moves back into the reference set; leaves held[] and the counts up to date.
    int picture(size_t t, DecOutput &dst, int *pictures)
    {
        if (hipMemcpyAsync(c->planes[c->cur_set], c->planes[c->cur_set ^ 1], c->d.ysz * 3 / 2 * S, hipMemcpyDeviceToDevice, c->st) != hipSuccess)
            return FERHIP_E_HIP;
        for (int s = 0; s < S; s++)
            if (ss.held[s] && (!iso || ss.pres[t * S + s]) && dec_copy_stream(c, c->planes[c->cur_set], ss.hold, s)) return FERHIP_E_HIP;
        const DecBatch &B = ss.B;
        FerDev ds = c->d;  // this picture's slice of the window
        const size_t o = t * ss.nm;
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
        c->cur_set ^= 1;
        bind_planes(c);
        if (int rc = dst.emit(ss, t0, t)) return rc;
        for (int s = 0; s < S; s++) {
            if (!ss.pres[t * S + s]) continue;
            if (ss.keep[t * S + s]) {
                ss.held[s] = 0;
                continue;
            }
            if (ss.hold.reserve(c->d.ysz * 3 / 2 * S + 256)) return FERHIP_E_HIP;
            if (dec_copy_stream(c, ss.hold, c->planes[c->cur_set ^ 1], s) || dec_copy_stream(c, c->planes[c->cur_set ^ 1], c->planes[c->cur_set], s))
                return FERHIP_E_HIP;
            ss.held[s] = 1;
        }
        for (int s = 0; s < S && pictures; s++)
            if (ss.pres[t * S + s]) pictures[s]++;
        return 0;
    }
};
}  // namespace

int DecOutput::plan(DecSession &ss, size_t TW, const int *pictures)
{
    if (!out || rows) return 0;
    const int S = ss.S;
    // step t writes map[t * S + k], k < nmap[t] = (stream, slot); the slot is the caller's (picture * S + stream) for device
    // output, the next free picture of the staging buffer for host output
    map.resize(TW * S);
    nmap.assign(TW, 0);
    fin.clear();
    for (size_t t = 0; t < TW; t++)
        for (int s = 0; s < S; s++) {
            if (!ss.pres[t * S + s]) continue;
            const size_t slot = (size_t)(pictures[s] + (int)t) * S + s;
            int2 &e = map[t * S + nmap[t]++];
            e.x = s;
            e.y = out_dev ? (int)slot : (int)fin.size();
            if (!out_dev) fin.push_back(slot);
        }
    if (!out_dev) {  // the staging buffers grow to the largest window seen, then stay
        const size_t cap = std::min(std::max(fin.size(), (size_t)S), ss.TWmax * S);
        if (d_stage.reserve(fin.size() * ofsz, cap * ofsz) || h_stage.reserve(fin.size() * ofsz, cap * ofsz)) return FERHIP_E_HIP;
    }
    if (hipMemcpyAsync(d_map, map.data(), TW * S * sizeof(int2), hipMemcpyHostToDevice, ss.c->st) != hipSuccess) return FERHIP_E_HIP;
    return 0;
}

int DecOutput::emit(DecSession &ss, size_t t0, size_t t)
{
    if (!out) return 0;
    ferhip_ctx *c = ss.c;
    const FerDev &d = c->d;
    const int S = ss.S;
    const uint8_t *set = c->planes[c->cur_set ^ 1];
    if (rows) {
        uint8_t *row = out + (t0 + t) * S * ss.fsz;
        bool all = true;
        for (int s = 0; s < S; s++) all &= ss.pres[t * S + s] != 0;
        if (all) return ferhip_get_recon(c, row, 1);
        // a stream that has ended has no picture at this step: its slot of `out` keeps what the caller put there
        for (int s = 0; s < S; s++) {
            if (!ss.pres[t * S + s]) continue;
            const PlaneSpans p = dec_stream_planes(d, s);
            uint8_t *f = row + (size_t)s * ss.fsz;
            for (int k = 0; k < 3; f += p.len[k++])
                if (hipMemcpyAsync(f, set + p.off[k], p.len[k], hipMemcpyDeviceToHost, c->st) != hipSuccess) return FERHIP_E_HIP;
        }
        return hipStreamSynchronize(c->st) != hipSuccess ? FERHIP_E_HIP : 0;
    }
    uint8_t *to = out_dev ? out : d_stage.p;  // (the staged pictures of host output are tight slots)
    const int2 *m = d_map.p + t * S;
    const uint32_t py = row_y(), pc = row_c();
    const size_t slot = fer_pic_slot_bytes(fmt, py, pc, (uint32_t)win[3]);
    if (fer_pic_packed(fmt))
        fer_launch_pic_emit_packed(d, set, nullptr, m, nmap[t], to, fmt, csc, py, slot, win, c->st);
    else if (whole(d, to))
        fer_launch_decode_out(d, set, m, nmap[t], to, c->st);
    else
        fer_launch_pic_emit_slots(d, set, m, nmap[t], to, fmt, py, pc, slot, win, c->st);
    return 0;
}

int DecOutput::finish(DecSession &ss, size_t TW)
{
    hipStream_t st = ss.c->st;
    size_t staged = 0;
    if (out && !rows && !out_dev) {
        for (size_t t = 0; t < TW; t++) staged += (size_t)nmap[t];
        if (staged && hipMemcpyAsync(h_stage, d_stage, staged * ofsz, hipMemcpyDeviceToHost, st) != hipSuccess) return FERHIP_E_HIP;
    }
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) return FERHIP_E_HIP;
    // the staged pictures to their slots of the caller's buffer (nothing else of it is written)
    const size_t threads = std::min<size_t>(std::min<size_t>(staged * ofsz >> 23, 16), std::max(1u, std::thread::hardware_concurrency()));
    dec_fan_out(staged, threads, [&](size_t j) { memcpy(out + fin[j] * ofsz, h_stage.p + j * ofsz, ofsz); });
    return 0;
}

int dec_session_window(DecSession &ss, const std::vector<std::vector<const NalRef *>> &slices, size_t t0, size_t TW, DecOutput &o,
                       int *pictures, DecIsolate *iso)
{
    DecWindow w{ss, slices, t0, TW, iso};
    double ta = dec_now();
    int rc = w.headers();
    if (!rc) rc = w.stage();
    if (rc) return rc;
    ss.t_pack += dec_now() - ta;
    ta = dec_now();
    rc = w.parse();
    if (!rc) rc = o.plan(ss, TW, pictures);
    if (rc) return rc;
    ss.t_parse += dec_now() - ta;
    ta = dec_now();
    for (size_t t = 0; t < TW && ss.anyAny[t]; t++)
        if ((rc = w.picture(t, o, pictures)) != 0) return rc;
    if ((rc = o.finish(ss, TW)) != 0) return rc;
    ss.t_recon += dec_now() - ta;
    return 0;
}
