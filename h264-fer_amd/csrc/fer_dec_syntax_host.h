// fer_dec_syntax_host.h -- the first readers of the bytes a caller hands the decoders (ferhip_decode_streams, ferhip_dec_nal,
// ferhip_decs_*): the bit reader and the SPS, PPS and slice-header parsers (F/headers_and_parameter_sets.cpp:245-298,398-537),
// the Annex-B and length-prefixed splitters with emulation-prevention removal (F/nal.cpp:68-223), the RTP depacketiser
// (split_rtp), the transport stream and MP4 fragment demultiplexers (split_ts, split_mp4) and the walk over an
// AVCDecoderConfigurationRecord.  Plain C++ without the HIP runtime, so that it can be compiled into a stand-alone host
// program and run under a sanitizer (tools/dec_syntax_host_check.cpp, tools/rtp_host_check.cpp, tools/ts_host_check.cpp,
// tools/mp4_host_check.cpp).
#pragma once
#include "../../include/ferhip.h"
#include "fer_mp4_host.h"
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

struct HostBR {  // bits of b[0, n), most significant first; zeros past the end
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
static inline int dec_parse_sps(DecHdr &h, HostBR &r)
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
static inline int dec_parse_pps(DecHdr &h, HostBR &r)
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
static inline int dec_parse_slice_header(DecHdr &h, const uint8_t *rbsp, size_t n, int nal_type, int ref_idc, uint32_t *info,
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
    // rbsp holds the first min(dev_n, FERHIP_SPLIT_PREFIX) of them (all of them once the unit was fetched whole)
    const uint8_t *dev = nullptr;
    size_t dev_n = 0;
};
// next position i in [from, n - 2) with s[i] == 0, s[i+1] == 0 and s[i+2] in `third` (two allowed values), or npos;
// zero bytes are rare in entropy-coded data, so the scan is driven by memchr
static inline size_t find_zz(const uint8_t *s, size_t from, size_t n, uint8_t t0, uint8_t t1)
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
static inline uint8_t *unescape_rbsp(const uint8_t *s, size_t from, size_t en, uint8_t *w)
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

// the unit s[st..en): its header byte, and its RBSP appended at w, which moves behind it
static inline NalRef nal_unit(const uint8_t *s, size_t st, size_t en, uint8_t *&w)
{
    NalRef nal;
    nal.ref_idc = (s[st] & 0x7f) >> 5;
    nal.type = s[st] & 0x1f;
    nal.rbsp.p = w;
    w = unescape_rbsp(s, st + 1, en, w);
    nal.rbsp.n = (size_t)(w - nal.rbsp.p);
    return nal;
}

// `store` receives the RBSP of every NAL unit back to back (never more than the stream itself) and must outlive `out`
static inline void split_stream(const uint8_t *s, size_t n, std::vector<NalRef> &out, std::vector<uint8_t> &store)
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
        NalRef nal = nal_unit(s, st, en, w);
        if (nal.rbsp.empty()) break;
        out.push_back(nal);
    }
}

// split a length-prefixed range (every unit behind its length of L = 1, 2 or 4 bytes, big-endian; the definition: ferhip.h)
// like split_stream; an empty unit, one without payload and one that overruns the range end it.  Returns 1 if it overran.
static inline int split_avcc_at(const uint8_t *s, size_t n, int L, std::vector<NalRef> &out, uint8_t *&w);
static inline int split_avcc(const uint8_t *s, size_t n, int L, std::vector<NalRef> &out, std::vector<uint8_t> &store)
{
    if (store.size() < n) store.resize(n);
    uint8_t *w = store.data();
    return split_avcc_at(s, n, L, out, w);
}
// ... with the RBSP appended at w, which moves behind it (room for n bytes)
static inline int split_avcc_at(const uint8_t *s, size_t n, int L, std::vector<NalRef> &out, uint8_t *&w)
{
    size_t pos = 0;
    while (n - pos >= (size_t)L) {
        size_t len = 0;
        for (int k = 0; k < L; k++) len = len << 8 | s[pos + k];
        const size_t st = pos + L;
        if (len == 0) return 0;
        if (len > n - st) return 1;
        if (len == 1) return 0;
        const size_t en = st + len;
        out.push_back(nal_unit(s, st, en, w));
        pos = en;
    }
    return pos < n;  // fewer than L bytes are left: a unit that cannot state its length
}

// The RTP packets of one stream, in order (RFC 6184, packetization-mode 1; the definition: ferhip.h) -> its NAL units like
// split_avcc.  expect: the sequence number the first packet must carry, -1 = any; it leaves as the one behind the last
// packet, or -1 after a fault.  Returns the fault: 0, or the first of FER_RTP_MALFORMED, _GAP, _TRUNCATED, which ends the
// walk; the units completed in front of it stand.  A unit without payload ends the unit list (not the walk), as it ends a
// length-prefixed range.  A fragmented unit is joined in `fu` before its emulation prevention bytes are dropped, so that a
// 00 00 03 across a fragment seam is one.
#define FER_RTP_MALFORMED 2
#define FER_RTP_GAP 3
#define FER_RTP_TRUNCATED 4
struct RtpPacket {
    const uint8_t *p;
    size_t n;
};
static inline int split_rtp(const RtpPacket *pk, size_t npk, int32_t &expect, std::vector<NalRef> &out, std::vector<uint8_t> &store)
{
    size_t total = 0;
    for (size_t k = 0; k < npk; k++) total += pk[k].n;
    if (store.size() < total) store.resize(total);  // an RBSP is shorter than the packets that carried its unit
    uint8_t *w = store.data();
    std::vector<uint8_t> fu;
    bool open = false, ended = false;  // an FU-A unit is being joined; a unit without payload has ended the list
    auto unit = [&](const uint8_t *s, size_t n) {
        if (ended) return;
        if (n == 1)
            ended = true;
        else
            out.push_back(nal_unit(s, 0, n, w));
    };
    const auto fault = [&](int f) {
        expect = -1;
        return f;
    };
    for (size_t k = 0; k < npk; k++) {
        const uint8_t *p = pk[k].p;
        const size_t L = pk[k].n;
        if (L < 12 || p[0] >> 6 != 2) return fault(FER_RTP_MALFORMED);
        size_t hl = 12 + 4 * (size_t)(p[0] & 15);
        if (p[0] & 0x10) {  // the extension: a 4-byte header whose last two bytes count its words
            if (hl + 4 > L) return fault(FER_RTP_MALFORMED);
            hl += 4 + 4 * ((size_t)p[hl + 2] << 8 | p[hl + 3]);
            if (hl > L) return fault(FER_RTP_MALFORMED);
        }
        size_t pad = 0;
        if (p[0] & 0x20) {
            pad = p[L - 1];
            if (pad < 1) return fault(FER_RTP_MALFORMED);
        }
        if (hl + pad >= L) return fault(FER_RTP_MALFORMED);
        const int32_t seq = (int32_t)p[2] << 8 | p[3];
        if (expect >= 0 && seq != expect) return fault(FER_RTP_GAP);
        expect = (seq + 1) & 0xffff;
        const uint8_t *s = p + hl;
        const size_t n = L - pad - hl;  // >= 1
        const int t = s[0] & 31;
        if (open && t != 28) return fault(FER_RTP_MALFORMED);
        if (t >= 1 && t <= 23) {
            unit(s, n);
        } else if (t == 24) {
            size_t pos = 1;
            if (pos == n) return fault(FER_RTP_MALFORMED);
            while (pos < n) {
                if (n - pos < 2) return fault(FER_RTP_MALFORMED);
                const size_t size = (size_t)s[pos] << 8 | s[pos + 1];
                pos += 2;
                if (size == 0 || size > n - pos) return fault(FER_RTP_MALFORMED);
                unit(s + pos, size);
                pos += size;
            }
        } else if (t == 28) {
            if (n < 2) return fault(FER_RTP_MALFORMED);
            const bool S = (s[1] & 0x80) != 0, E = (s[1] & 0x40) != 0;
            if ((S && E) || (S && open) || (!S && !open)) return fault(FER_RTP_MALFORMED);
            if (S) {
                fu.assign(1, (uint8_t)((s[0] & 0xE0) | (s[1] & 0x1F)));
                open = true;
            }
            fu.insert(fu.end(), s + 2, s + n);
            if (E) {
                unit(fu.data(), fu.size());
                open = false;
            }
        } else {
            return fault(FER_RTP_MALFORMED);
        }
    }
    return open ? fault(FER_RTP_TRUNCATED) : 0;
}

// The transport stream packets of one stream's runs, in order (ISO/IEC 13818-1; the definition: ferhip.h) -> its NAL units
// like split_stream.  Every run is a whole number of 188-byte packets; pid: the PID the stream listens to; expect: the
// continuity counter the first payload packet must carry, -1 = any; it leaves as the one behind the last payload packet, or
// -1 after a fault.  Returns the fault: 0, or the first of FER_TS_MALFORMED and FER_TS_GAP, which ends the walk; the PES
// packets completed in front of it stand, the open one is dropped.  The elementary-stream bytes that stand are joined in
// `es` and split as one Annex-B range.
#define FER_TS_MALFORMED 2
#define FER_TS_GAP 3
typedef RtpPacket TsRun;
static inline int split_ts(const TsRun *runs, size_t nruns, unsigned pid, int32_t &expect, std::vector<NalRef> &out, std::vector<uint8_t> &store)
{
    std::vector<uint8_t> es;
    size_t pes_at = 0;  // where the open PES packet's bytes begin in es
    bool open = false;
    int fault = 0;
    for (size_t r = 0; r < nruns && !fault; r++) {
        for (size_t at = 0; at + 188 <= runs[r].n && !fault; at += 188) {
            const uint8_t *p = runs[r].p + at;
            if (p[0] != 0x47 || (p[1] & 0x80)) {
                fault = FER_TS_MALFORMED;
                break;
            }
            if ((((unsigned)p[1] & 0x1F) << 8 | p[2]) != pid) continue;
            const unsigned afc = (p[3] >> 4) & 3;
            if (p[3] >> 6 || afc == 0) {
                fault = FER_TS_MALFORMED;
                break;
            }
            if (afc == 2) continue;
            size_t pay = 4;
            if (afc == 3) {
                if (p[4] > 183) {
                    fault = FER_TS_MALFORMED;
                    break;
                }
                pay = 5 + (size_t)p[4];
            }
            const int32_t cc = p[3] & 15;
            if (expect >= 0 && cc != expect) {
                fault = FER_TS_GAP;
                break;
            }
            expect = (cc + 1) & 15;
            const size_t n = 188 - pay;
            const uint8_t *q = p + pay;
            if (p[1] & 0x40) {
                if (n < 9 || q[0] != 0 || q[1] != 0 || q[2] != 1 || (q[3] & 0xF0) != 0xE0 || (q[6] & 0xC0) != 0x80 || n < 9 + (size_t)q[8]) {
                    fault = FER_TS_MALFORMED;
                    break;
                }
                open = true;
                pes_at = es.size();
                es.insert(es.end(), q + 9 + q[8], q + n);
            } else if (!open) {
                fault = FER_TS_MALFORMED;
            } else {
                es.insert(es.end(), q, q + n);
            }
        }
    }
    if (fault) {
        expect = -1;
        if (open) es.resize(pes_at);
    }
    if (!es.empty()) split_stream(es.data(), es.size(), out, store);
    return fault;
}

// The fragments of one stream's runs, in order (ISO/IEC 14496-12 movie fragments; the definition: ferhip.h) -> its NAL units:
// every run is a whole number of top-level boxes, fer_mp4_walk_run (fer_mp4_host.h) gives the samples of its whole fragments,
// and every sample is one length-prefixed range as split_avcc takes it.  Returns the fault: 0, or the first of
// FER_MP4_MALFORMED, _UNSUP, _TRUNCATED (the box walk: the samples of the fragments completed in front of it stand) and
// FER_MP4_OVERRUN (the length walk of a sample: its units in front of the overrun stand), which ends the stream's walk.
// spans (optional) receives every sample that stands as (run, offset in the run, bytes).
struct Mp4Span {
    size_t run;
    uint64_t at;
    uint32_t len;
};
struct Mp4HostSink {
    std::vector<Mp4Span> &spans;
    size_t run;
    int64_t entries(const uint8_t *sizes, uint32_t count, uint32_t e, uint32_t dflt, int64_t at, uint64_t index)
    {
        if (spans.size() < index + count) spans.resize((size_t)(index + count));
        for (uint32_t k = 0; k < count; k++) {
            const uint32_t size = sizes ? fer_mp4_be32(sizes + (size_t)k * e) : dflt;
            spans[(size_t)index + k] = {run, (uint64_t)at, size};
            at += size;
        }
        return at;
    }
};
static inline int split_mp4(const TsRun *runs, size_t nruns, int L, std::vector<NalRef> &out, std::vector<uint8_t> &store,
                            std::vector<Mp4Span> *spans_out = nullptr)
{
    std::vector<Mp4Span> spans;
    uint64_t done = 0;
    int fault = 0;
    for (size_t r = 0; r < nruns && !fault; r++) {
        Mp4HostSink sink{spans, r};
        fault = fer_mp4_walk_run(runs[r].p, runs[r].n, done, sink);
    }
    spans.resize((size_t)done);  // what a fragment that did not complete recorded goes
    size_t total = 0;
    for (const Mp4Span &sp : spans) total += sp.len;
    if (store.size() < total) store.resize(total);
    uint8_t *w = store.data();
    size_t kept = spans.size();
    for (size_t k = 0; k < spans.size(); k++) {
        if (split_avcc_at(runs[spans[k].run].p + spans[k].at, spans[k].len, L, out, w)) {
            if (!fault) fault = FER_MP4_OVERRUN;
            kept = k + 1;
            break;
        }
    }
    if (spans_out) {
        spans.resize(kept);
        *spans_out = spans;
    }
    return fault;
}

// AVCDecoderConfigurationRecord avcc[0, n) -> the (at, len) spans of its SPS, then of its PPS units (header byte included) and
// the longest.  FERHIP_E_ARG: another version, a record that ends inside a count, length or unit, a count or length of zero.
struct AvccSpan { size_t at, len; };
static inline int split_avcc_config(const uint8_t *avcc, size_t n, std::vector<AvccSpan> &units, size_t &longest)
{
    units.clear();
    longest = 0;
    if (!avcc || n < 7 || avcc[0] != 1) return FERHIP_E_ARG;
    size_t pos = 5;
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
    return 0;
}
