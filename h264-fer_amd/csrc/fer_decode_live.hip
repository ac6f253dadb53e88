// fer_decode_live.hip -- the live decoder (ferhip_decs_*): S streams that arrive piece by piece, one window of all of them per
// call, with per-stream fault isolation; split on the host or on the device (fer_nalsplit.h), decoded by fer_dec_session.h.
#include "fer_dec_session.h"
#include "fer_nalsplit.h"

struct ferhip_decs {
    DecSession ss;
    int S = 0, W = 0, H = 0, P = 0;
    std::vector<std::vector<uint8_t>> store;  // RBSP of each stream's chunk (kept between calls)
    std::vector<std::vector<NalRef>> nals;
    std::vector<size_t> cursor;               // next NAL unit of each stream's chunk
    std::vector<int> queued;                  // slice NAL units taken from each stream's chunk in this call
    std::vector<char> need_idr;               // after a fault: P slices are refused until an IDR slice
    DecIsolate iso;
    DecOutput out;                            // ferhip_decs_set_display, _set_layout, _set_csc: where the pictures go
    FerSplit split;                           // ferhip_decs_decode_dev: the splitter's buffers and the store of the units' RBSP
    FerUnrtp unrtp;                           // ferhip_decs_decode_rtp from device memory: the depacketiser's buffers in front of it
    std::vector<std::vector<uint8_t>> whole;  // ... parameter sets longer than the prefix, fetched whole
    int in_format = FERHIP_IN_ANNEXB, length_size = 4;  // ferhip_decs_set_input
    std::vector<int> overrun;                 // [S] AVCC input: the stream's chunk of this call overran; RTP: its packets faulted
    std::vector<int32_t> rtp_expect;          // [S] ferhip_decs_decode_rtp: the sequence number the stream's next packet must carry, -1 = any
    FerUnts unts;                             // ferhip_decs_decode_ts from device memory: the demultiplexer's buffers in front of the splitter
    std::vector<int32_t> ts_expect;           // [S] ferhip_decs_decode_ts: the continuity counter the stream's next payload packet must carry, -1 = any
    double t_split = 0;                       // seconds in the host splitter
};

// the decoder's context for a pass that runs in front of it on its stream (fer_srtp.hip)
__attribute__((visibility("hidden"))) ferhip_ctx *fer_decs_ctx(ferhip_decs *d) { return d->ss.c; }

// Stream s back to the state of a new decoder; forget_ps = also forget its parameter sets, else keep them and refuse
// P slices until the next IDR slice
static int decs_reset(ferhip_decs *d, int s, bool forget_ps)
{
    ferhip_ctx *c = d->ss.c;
    const FerDev &dv = c->d;
    hipError_t e = hipMemsetAsync(dv.dec_state + s * 4, 0, 4 * sizeof(int), c->st);
    if (e == hipSuccess) e = hipMemsetAsync(dv.dec_cac + s * 128, 0, 128 * sizeof(int16_t), c->st);
    if (e == hipSuccess) e = hipMemsetAsync(dv.status + s, 0, sizeof(int), c->st);
    const PlaneSpans p = dec_stream_planes(dv, s);
    for (int set = 0; set < 2; set++)
        for (int k = 0; k < 3 && e == hipSuccess; k++) e = hipMemsetAsync(c->planes[set] + p.off[k], 0, p.len[k], c->st);
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
    d->rtp_expect.assign(nstreams, -1);
    d->ts_expect.assign(nstreams, -1);
    d->out.win[2] = width;
    d->out.win[3] = height;
    d->out.ofsz = d->ss.fsz;
    if (d->out.d_map.reserve(d->ss.TWmax * nstreams)) {
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
    fer_split_free(d->split);
    dec_session_close(d->ss);
    delete d;  // (the output's buffers go with it, on the device selected above)
}

extern "C" int ferhip_decs_reset_stream(ferhip_decs *d, int s)
{
    if (!d || s < 0 || s >= d->S) return FERHIP_E_ARG;
    (void)hipSetDevice(d->ss.c->device);
    d->rtp_expect[s] = -1;
    d->ts_expect[s] = -1;
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
    DecOutput &o = d->out;
    const size_t ofsz = (size_t)dw * dh * 3 / 2;
    if (ofsz != o.ofsz) {  // the staging buffers of host output are sized in slots: they are made again at the next call
        (void)hipSetDevice(d->ss.c->device);
        o.d_stage.release();
        o.h_stage.release();
    }
    o.win[0] = x0, o.win[1] = y0, o.win[2] = dw, o.win[3] = dh;
    o.ofsz = ofsz;
    return 0;
}

// From the next decode call on the slots of `out` are pitched I420 or NV12; the pitches are checked against the window
// when a decode call is made (decs_layout_check), since ferhip_decs_set_display may change it in between
extern "C" int ferhip_decs_set_layout(ferhip_decs *d, int format, uint32_t pitch_y, uint32_t pitch_c)
{
    if (!d || (format != FERHIP_FMT_I420 && format != FERHIP_FMT_NV12 && !fer_pic_packed(format))) return FERHIP_E_ARG;
    d->out.layout_set = true;
    d->out.fmt = format;
    d->out.pitch_y = pitch_y;
    d->out.pitch_c = pitch_c;
    return 0;
}

// the matrix of a BGRA / RGBA output layout (FERHIP_CSC_*), from the next decode call on
extern "C" int ferhip_decs_set_csc(ferhip_decs *d, int matrix)
{
    if (!d || (matrix != FERHIP_CSC_BT601 && matrix != FERHIP_CSC_BT709)) return FERHIP_E_ARG;
    d->out.csc = matrix;
    return 0;
}

// a layout other than the default: device output only, and pitches that hold a row of the current window; a packed format
// is written in aligned dwords, so its slots must start at multiples of 4
static int decs_layout_check(const ferhip_decs *d, const uint8_t *out, int out_on_device)
{
    const DecOutput &o = d->out;
    if (!o.own_layout()) return 0;
    if (!out_on_device) return FERHIP_E_ARG;
    if (fer_pic_packed(o.fmt) && ((uintptr_t)out & 3u)) return FERHIP_E_ARG;
    return fer_pic_layout_check(o.fmt, o.pitch_y, o.pitch_c, (uint32_t)o.win[2]);  // (the internal tight pitches never get here)
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
    std::vector<AvccSpan> units;
    size_t longest = 0;
    if (int rc = split_avcc_config(avcc, n, units, longest)) return rc;
    if (hipSetDevice(d->ss.c->device) != hipSuccess) return FERHIP_E_HIP;
    std::vector<uint8_t> rbsp(longest);
    for (const AvccSpan &u : units) {
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

// the chunks of a call are split into d->nals: take them window by window
static int decs_run(ferhip_decs *d, uint8_t *out, int out_on_device, int *pictures, int *status)
{
    const int S = d->S;
    d->iso.status = status;
    d->iso.stop.assign(S, 0);
    d->out.out = out;
    d->out.out_dev = out_on_device != 0;
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
        for (size_t t0 = 0; t0 < T && !rc; t0 += d->ss.TWmax) rc = dec_session_window(d->ss, slices, t0, std::min(d->ss.TWmax, T - t0), d->out, pictures, &d->iso);
        if (rc) break;
    }
    for (int s = 0; s < S && !rc; s++) {
        // a chunk that overran (AVCC input): its units in front of the overrun were taken, then the stream faults
        if (d->overrun[s] && !status[s]) status[s] = FERHIP_E_ARG;
        if (status[s]) rc = decs_reset(d, s, false);
    }
    return rc;
}

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
    // NAL splitting: a few threads when there is much of it
    dec_fan_out((size_t)S, bytes < ((size_t)1 << 20) ? 1 : dec_stream_threads(S), [&](size_t s) {
        if (!chunks[s] || !lens[s]) return;
        if (d->in_format == FERHIP_IN_AVCC)
            d->overrun[s] = split_avcc(chunks[s], lens[s], d->length_size, d->nals[s], d->store[s]);
        else
            split_stream(chunks[s], lens[s], d->nals[s], d->store[s]);
    });
    d->t_split += dec_now() - ts;
    return decs_run(d, out, out_on_device, pictures, status);
}

// the last job of the decoder's splitter -> the unit lists: a unit's RBSP stays in the splitter's store, its prefix is on the host
static int decs_take_table(ferhip_decs *d)
{
    ferhip_ctx *c = d->ss.c;
    const FerSplit &sp = d->split;
    d->whole.clear();
    int rc = fer_split_each_unit(sp, [&](size_t k, const ferhip_nal_unit &u) -> int {
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
    return 0;
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
    for (int s = 0; avcc && s < S; s++) d->overrun[s] = d->split.h_fault[s];
    if ((rc = decs_take_table(d))) return rc;
    return decs_run(d, out, out_on_device, pictures, status);
}

// RTP packets (RFC 6184, packetization-mode 1), the packets of every stream in table order, into the same unit lists as the
// other two framings: from host memory through split_rtp (no synchronisation of its own), from device memory through
// fer_unrtp_run and the length-prefixed splitter (two).
extern "C" int ferhip_decs_decode_rtp(ferhip_decs *d, const void *base, int base_on_device, const ferhip_rtp_pkt *pkts, size_t npkts,
                                      uint8_t *out, int out_on_device, int *pictures, int *status)
{
    if (!d || !pictures || !status || (npkts && (!base || !pkts)) || decs_layout_check(d, out, out_on_device)) return FERHIP_E_ARG;
    const int S = d->S;
    for (size_t k = 0; k < npkts; k++)
        if (pkts[k].stream >= (uint32_t)S) return FERHIP_E_ARG;
    if (hipSetDevice(d->ss.c->device) != hipSuccess) return FERHIP_E_HIP;
    const uint8_t *const none = nullptr;
    std::vector<const uint8_t *> no_chunks(S, none);
    std::vector<size_t> no_lens(S, 0);
    decs_begin_call(d, no_chunks.data(), no_lens.data(), pictures, status);
    const double ts = dec_now();
    std::vector<std::vector<RtpPacket>> per(S);  // a stable sort by stream
    for (size_t k = 0; k < npkts && !base_on_device; k++) per[pkts[k].stream].push_back({(const uint8_t *)base + pkts[k].offset, pkts[k].bytes});
    const std::vector<int32_t> before = d->rtp_expect;
    bool too_many = false;
    if (base_on_device && npkts) {
        // parse, walk and gather on the device (fer_rtp.hip), then the length-prefixed splitter on the staged units: one
        // synchronisation for the walk's results and one for the splitter's table
        std::vector<ferhip_rtp_pkt> sorted;
        std::vector<uint32_t> first;
        std::vector<int32_t> fault(S, 0);
        int rc = fer_rtp_sort(pkts, npkts, S, sorted, first);
        if (!rc) rc = fer_unrtp_run(d->unrtp, d->ss.c->st, (const uint8_t *)base, sorted.data(), npkts, first.data(), S, d->rtp_expect.data(), fault.data());
        size_t staged = 0;
        for (int s = 0; s < S && !rc; s++) {
            d->overrun[s] = fault[s] != 0;
            staged += d->unrtp.lens[s];
        }
        if (!rc && staged) {
            rc = fer_split_run(d->split, d->ss.c->st, d->unrtp.ptrs.data(), d->unrtp.lens.data(), S, nullptr, 0, 4);
            if (!rc) rc = decs_take_table(d);
        }
        if (rc) {
            d->rtp_expect = before;
            return rc;
        }
    }
    for (int s = 0; s < S; s++) {
        if (!base_on_device && !per[s].empty())
            d->overrun[s] = split_rtp(per[s].data(), per[s].size(), d->rtp_expect[s], d->nals[s], d->store[s]) != 0;
        size_t slices = 0;
        for (const NalRef &n : d->nals[s]) slices += n.type == 1 || n.type == 5;
        too_many |= slices > (size_t)d->P;
    }
    d->t_split += dec_now() - ts;
    if (too_many) {  // refused as a whole: nothing was taken
        d->rtp_expect = before;
        for (int s = 0; s < S; s++) {
            d->nals[s].clear();
            d->overrun[s] = 0;
        }
        return FERHIP_E_ARG;
    }
    return decs_run(d, out, out_on_device, pictures, status);
}

// Transport stream packets (ISO/IEC 13818-1), the runs of every stream in table order, into the same unit lists as the other
// framings: from host memory through split_ts (no synchronisation of its own), from device memory through fer_unts_run and
// the Annex-B splitter (two).
extern "C" int ferhip_decs_decode_ts(ferhip_decs *d, const void *base, int base_on_device, const ferhip_ts_run *runs, size_t nruns,
                                     const uint16_t *pids, uint8_t *out, int out_on_device, int *pictures, int *status)
{
    if (!d || !pictures || !status || !pids || (nruns && (!base || !runs)) || decs_layout_check(d, out, out_on_device)) return FERHIP_E_ARG;
    const int S = d->S;
    for (size_t k = 0; k < nruns; k++)
        if (runs[k].stream >= (uint32_t)S || runs[k].bytes % 188u) return FERHIP_E_ARG;
    for (int s = 0; s < S; s++)
        if (pids[s] > 0x1FFF) return FERHIP_E_ARG;
    if (hipSetDevice(d->ss.c->device) != hipSuccess) return FERHIP_E_HIP;
    const uint8_t *const none = nullptr;
    std::vector<const uint8_t *> no_chunks(S, none);
    std::vector<size_t> no_lens(S, 0);
    decs_begin_call(d, no_chunks.data(), no_lens.data(), pictures, status);
    const double ts = dec_now();
    std::vector<std::vector<TsRun>> per(S);  // a stable sort by stream
    for (size_t k = 0; k < nruns && !base_on_device; k++) per[runs[k].stream].push_back({(const uint8_t *)base + runs[k].offset, runs[k].bytes});
    const std::vector<int32_t> before = d->ts_expect;
    bool too_many = false;
    if (base_on_device && nruns) {
        // parse, walk and gather on the device (fer_ts.hip), then the Annex-B splitter on the staged bytes: one
        // synchronisation for the walk's results and one for the splitter's table
        std::vector<ferhip_ts_run> sorted;
        std::vector<uint32_t> first;
        std::vector<int32_t> fault(S, 0);
        int rc = fer_rtp_sort(runs, nruns, S, sorted, first);
        if (!rc) rc = fer_unts_run(d->unts, d->ss.c->st, (const uint8_t *)base, sorted.data(), nruns, first.data(), S, pids, d->ts_expect.data(), fault.data());
        size_t staged = 0;
        for (int s = 0; s < S && !rc; s++) {
            d->overrun[s] = fault[s] != 0;
            staged += d->unts.lens[s];
        }
        if (!rc && staged) {
            rc = fer_split_run(d->split, d->ss.c->st, d->unts.ptrs.data(), d->unts.lens.data(), S, nullptr, 0, 0);
            if (!rc) rc = decs_take_table(d);
        }
        if (rc) {
            d->ts_expect = before;
            return rc;
        }
    }
    for (int s = 0; s < S; s++) {
        if (!base_on_device && !per[s].empty())
            d->overrun[s] = split_ts(per[s].data(), per[s].size(), pids[s], d->ts_expect[s], d->nals[s], d->store[s]) != 0;
        size_t slices = 0;
        for (const NalRef &n : d->nals[s]) slices += n.type == 1 || n.type == 5;
        too_many |= slices > (size_t)d->P;
    }
    d->t_split += dec_now() - ts;
    if (too_many) {  // refused as a whole: nothing was taken
        d->ts_expect = before;
        for (int s = 0; s < S; s++) {
            d->nals[s].clear();
            d->overrun[s] = 0;
        }
        return FERHIP_E_ARG;
    }
    return decs_run(d, out, out_on_device, pictures, status);
}

// MP4 movie fragments (ISO/IEC 14496-12), the runs of every stream in table order, into the same unit lists as the other
// framings, from host memory through split_mp4 (no synchronisation of its own).  Fragments in device memory are not taken
// yet: FERHIP_E_UNSUP.
extern "C" int ferhip_decs_decode_mp4(ferhip_decs *d, const void *base, int base_on_device, const ferhip_mp4_run *runs, size_t nruns,
                                      int length_size, uint8_t *out, int out_on_device, int *pictures, int *status)
{
    if (!d || !pictures || !status || (nruns && (!base || !runs)) || (length_size != 1 && length_size != 2 && length_size != 4) ||
        decs_layout_check(d, out, out_on_device))
        return FERHIP_E_ARG;
    const int S = d->S;
    for (size_t k = 0; k < nruns; k++)
        if (runs[k].stream >= (uint32_t)S) return FERHIP_E_ARG;
    if (base_on_device) return FERHIP_E_UNSUP;
    if (hipSetDevice(d->ss.c->device) != hipSuccess) return FERHIP_E_HIP;
    const uint8_t *const none = nullptr;
    std::vector<const uint8_t *> no_chunks(S, none);
    std::vector<size_t> no_lens(S, 0);
    decs_begin_call(d, no_chunks.data(), no_lens.data(), pictures, status);
    const double ts = dec_now();
    std::vector<std::vector<TsRun>> per(S);  // a stable sort by stream
    for (size_t k = 0; k < nruns; k++) per[runs[k].stream].push_back({(const uint8_t *)base + runs[k].offset, runs[k].bytes});
    bool too_many = false;
    for (int s = 0; s < S; s++) {
        if (!per[s].empty()) d->overrun[s] = split_mp4(per[s].data(), per[s].size(), length_size, d->nals[s], d->store[s]) != 0;
        size_t slices = 0;
        for (const NalRef &n : d->nals[s]) slices += n.type == 1 || n.type == 5;
        too_many |= slices > (size_t)d->P;
    }
    d->t_split += dec_now() - ts;
    if (too_many) {  // refused as a whole: nothing was taken
        for (int s = 0; s < S; s++) {
            d->nals[s].clear();
            d->overrun[s] = 0;
        }
        return FERHIP_E_ARG;
    }
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
