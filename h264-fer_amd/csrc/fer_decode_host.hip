// fer_decode_host.hip -- the decoder's batch and streaming front ends: decode() of F/fer_h264.cpp:26-53 for S streams side by
// side (ferhip_decode_streams) and RBSP_decode(NALunit) of F/rbsp_decoding.cpp:17 for one stream (ferhip_dec_*), over
// fer_dec_session.h.  The live decoder is in fer_decode_live.hip.
#include "fer_dec_session.h"
#include <stdlib.h>

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
    // NAL splitting is host work per stream
    dec_fan_out((size_t)S, dec_stream_threads(S), [&](size_t s) { split_stream(streams[s], lens[s], nals[s], rbsp_store[s]); });
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
    DecOutput o;
    o.out = out;
    o.rows = true;
    for (size_t t0 = 0; t0 < T && rc == 0; t0 += ss.TWmax) rc = dec_session_window(ss, slices, t0, std::min(ss.TWmax, T - t0), o, pictures);
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
    DecOutput o;  // the caller's picture buffer of the current call
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
        dc->o.out = picture;
        dc->o.rows = true;
        int rc = dec_session_window(dc->ss, slices, 0, 1, dc->o, nullptr);
        if (rc) return rc;
        dc->h = dc->ss.hs[0];  // the slice header leaves state behind (reference count override, list modification)
        dc->pictures++;
        if (got_picture) *got_picture = 1;
    }  // every other NAL unit type (SEI, AUD ...) is ignored, as in the reference
    if (width) *width = dc->h.W;
    if (height) *height = dc->h.H;
    return 0;
}
