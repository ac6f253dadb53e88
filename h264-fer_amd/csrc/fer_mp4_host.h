// fer_mp4_host.h -- the bytes of the fragmented MP4 framing that are built from a handful of numbers (fer_mp4.hip; the
// definition stands in include/ferhip.h): the geometry of a stream's region, the 32-bit words of a segment's front -- moof,
// mfhd, traf, tfhd, tfdt, the head of the trun, the free box behind the trun entries and the head of the mdat -- which the
// close kernel stores, and the initialisation segment with its avcC record, which is written on the host.
// Plain C++ without the HIP runtime, so that it can be compiled into a stand-alone host program and run under a sanitizer
// (tools/mp4_host_check.cpp); under hipcc the word function is also device code, so the kernel and that program run the same.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#ifdef __HIPCC__
#define FER_MP4_HD __host__ __device__ inline
#else
#define FER_MP4_HD inline
#endif

#define FER_MP4_KMAX 4096u
#define FER_MP4_FOURCC(a, b, c, d) ((uint32_t)(a) << 24 | (uint32_t)(b) << 16 | (uint32_t)(c) << 8 | (uint32_t)(d))

// where the samples of a region begin: 88 bytes up to the trun entries, 12 per entry, 8 of a free box at least, 8 of the mdat
FER_MP4_HD uint32_t fer_mp4_data_offset(uint32_t K) { return (104u + 12u * K + 15u) & ~15u; }

// sample_flags of a trun entry
FER_MP4_HD uint32_t fer_mp4_sample_flags(bool idr) { return idr ? 0x02000000u : 0x01010000u; }

// Word w (the big-endian u32 at region offset 4 w) of the front of a segment of n >= 1 samples and M sample bytes, w < D / 4;
// *keep = the word belongs to a trun entry, which append has written.
FER_MP4_HD uint32_t fer_mp4_front_word(uint32_t w, uint32_t n, uint32_t D, uint32_t M, uint64_t decode_time, uint32_t sequence, bool *keep)
{
    *keep = false;
    switch (w) {
    case 0: return 88u + 12u * n;
    case 1: return FER_MP4_FOURCC('m', 'o', 'o', 'f');
    case 2: return 16u;
    case 3: return FER_MP4_FOURCC('m', 'f', 'h', 'd');
    case 4: return 0u;
    case 5: return sequence;
    case 6: return 64u + 12u * n;
    case 7: return FER_MP4_FOURCC('t', 'r', 'a', 'f');
    case 8: return 16u;
    case 9: return FER_MP4_FOURCC('t', 'f', 'h', 'd');
    case 10: return 0x00020000u;  // default-base-is-moof
    case 11: return 1u;           // track_ID
    case 12: return 20u;
    case 13: return FER_MP4_FOURCC('t', 'f', 'd', 't');
    case 14: return 0x01000000u;  // version 1: a 64-bit baseMediaDecodeTime
    case 15: return (uint32_t)(decode_time >> 32);
    case 16: return (uint32_t)decode_time;
    case 17: return 20u + 12u * n;
    case 18: return FER_MP4_FOURCC('t', 'r', 'u', 'n');
    case 19: return 0x00000701u;  // data-offset, sample-duration, sample-size and sample-flags present
    case 20: return n;
    case 21: return D;            // data_offset, from the moof's first byte
    default: break;
    }
    const uint32_t f = 22u + 3u * n, last = D / 4u;  // the free box begins at word f, the mdat at word last - 2
    if (w < f) {
        *keep = true;
        return 0u;
    }
    if (w == f) return D - 96u - 12u * n;
    if (w == f + 1u) return FER_MP4_FOURCC('f', 'r', 'e', 'e');
    if (w == last - 2u) return 8u + M;
    if (w == last - 1u) return FER_MP4_FOURCC('m', 'd', 'a', 't');
    return 0u;
}

// ---- the initialisation segment: a byte vector with boxes that are closed by patching their size
struct FerMp4Bytes {
    std::vector<uint8_t> v;
    void u8(uint32_t x) { v.push_back((uint8_t)x); }
    void u16(uint32_t x) { u8(x >> 8), u8(x); }
    void u32(uint32_t x) { u16(x >> 16), u16(x); }
    void zeros(size_t n) { v.insert(v.end(), n, 0); }
    void bytes(const uint8_t *p, size_t n) { v.insert(v.end(), p, p + n); }
    size_t open(const char *type)  // -> the box's first byte, for close()
    {
        const size_t at = v.size();
        u32(0);
        bytes((const uint8_t *)type, 4);
        return at;
    }
    size_t open_full(const char *type, uint32_t version, uint32_t flags)
    {
        const size_t at = open(type);
        u32(version << 24 | flags);
        return at;
    }
    void close(size_t at)
    {
        const uint32_t n = (uint32_t)(v.size() - at);
        v[at] = (uint8_t)(n >> 24), v[at + 1] = (uint8_t)(n >> 16), v[at + 2] = (uint8_t)(n >> 8), v[at + 3] = (uint8_t)n;
    }
    void matrix()
    {
        const uint32_t m[9] = {0x00010000u, 0, 0, 0, 0x00010000u, 0, 0, 0, 0x40000000u};
        for (uint32_t x : m) u32(x);
    }
};

// AVCDecoderConfigurationRecord from the two units (header byte + escaped payload): ferhip_write_avcc_config's bytes.
// Empty where a unit is too short or too long for the record.
static inline std::vector<uint8_t> fer_mp4_avcc_record(const uint8_t *sps, size_t ns, const uint8_t *pps, size_t np)
{
    FerMp4Bytes b;
    if (!sps || !pps || ns < 4 || np < 1 || ns > 65535 || np > 65535) return b.v;
    b.u8(1);
    b.bytes(sps + 1, 3);  // profile, compatibility, level: no emulation prevention byte can stand in front of them
    b.u8(0xFC | 3);
    b.u8(0xE0 | 1);
    b.u16((uint32_t)ns);
    b.bytes(sps, ns);
    b.u8(1);
    b.u16((uint32_t)np);
    b.bytes(pps, np);
    return b.v;
}

// ftyp + moov of one video track; empty where an argument is refused (a record that cannot be built, a display size
// outside 1..65535, timescale 0)
static inline std::vector<uint8_t> fer_mp4_init_segment(const uint8_t *sps, size_t ns, const uint8_t *pps, size_t np, int dw, int dh,
                                                        uint32_t timescale)
{
    FerMp4Bytes b;
    const std::vector<uint8_t> rec = fer_mp4_avcc_record(sps, ns, pps, np);
    if (rec.empty() || dw < 1 || dh < 1 || dw > 65535 || dh > 65535 || timescale == 0) return b.v;
    const size_t ftyp = b.open("ftyp");
    b.bytes((const uint8_t *)"iso6", 4);
    b.u32(0);
    b.bytes((const uint8_t *)"iso6cmfcavc1", 12);
    b.close(ftyp);
    const size_t moov = b.open("moov");
    {
        const size_t mvhd = b.open_full("mvhd", 0, 0);
        b.u32(0), b.u32(0), b.u32(timescale), b.u32(0);  // creation, modification, timescale, duration
        b.u32(0x00010000u), b.u16(0x0100), b.zeros(10);   // rate, volume, reserved
        b.matrix();
        b.zeros(24);  // pre_defined
        b.u32(2);     // next_track_ID
        b.close(mvhd);
        const size_t trak = b.open("trak");
        const size_t tkhd = b.open_full("tkhd", 0, 3);
        b.u32(0), b.u32(0), b.u32(1), b.u32(0), b.u32(0);  // creation, modification, track_ID, reserved, duration
        b.zeros(8);                                         // reserved
        b.u16(0), b.u16(0), b.u16(0), b.u16(0);             // layer, alternate_group, volume, reserved
        b.matrix();
        b.u32((uint32_t)dw << 16), b.u32((uint32_t)dh << 16);
        b.close(tkhd);
        const size_t mdia = b.open("mdia");
        const size_t mdhd = b.open_full("mdhd", 0, 0);
        b.u32(0), b.u32(0), b.u32(timescale), b.u32(0);
        b.u16(0x55C4), b.u16(0);  // 'und', pre_defined
        b.close(mdhd);
        const size_t hdlr = b.open_full("hdlr", 0, 0);
        b.u32(0);
        b.bytes((const uint8_t *)"vide", 4);
        b.zeros(12);
        b.u8(0);  // name: an empty string
        b.close(hdlr);
        const size_t minf = b.open("minf");
        const size_t vmhd = b.open_full("vmhd", 0, 1);
        b.zeros(8);  // graphicsmode, opcolor
        b.close(vmhd);
        const size_t dinf = b.open("dinf");
        const size_t dref = b.open_full("dref", 0, 0);
        b.u32(1);
        b.close(b.open_full("url ", 0, 1));
        b.close(dref);
        b.close(dinf);
        const size_t stbl = b.open("stbl");
        const size_t stsd = b.open_full("stsd", 0, 0);
        b.u32(1);
        const size_t avc1 = b.open("avc1");
        b.zeros(6), b.u16(1);  // reserved, data_reference_index
        b.zeros(16);           // pre_defined, reserved, pre_defined[3]
        b.u16((uint32_t)dw), b.u16((uint32_t)dh);
        b.u32(0x00480000u), b.u32(0x00480000u), b.u32(0);  // 72 dpi twice, reserved
        b.u16(1);                                           // frame_count
        b.zeros(32);                                        // compressorname
        b.u16(0x0018), b.u16(0xFFFF);                       // depth, pre_defined = -1
        const size_t avcc = b.open("avcC");
        b.bytes(rec.data(), rec.size());
        b.close(avcc);
        b.close(avc1);
        b.close(stsd);
        for (const char *t : {"stts", "stsc"}) {
            const size_t at = b.open_full(t, 0, 0);
            b.u32(0);
            b.close(at);
        }
        const size_t stsz = b.open_full("stsz", 0, 0);
        b.u32(0), b.u32(0);
        b.close(stsz);
        const size_t stco = b.open_full("stco", 0, 0);
        b.u32(0);
        b.close(stco);
        b.close(stbl);
        b.close(minf);
        b.close(mdia);
        b.close(trak);
        const size_t mvex = b.open("mvex");
        const size_t trex = b.open_full("trex", 0, 0);
        b.u32(1), b.u32(1), b.u32(0), b.u32(0), b.u32(0);
        b.close(trex);
        b.close(mvex);
    }
    b.close(moov);
    return b.v;
}

// ---- the way in: the box walk over one run of top-level boxes (the rules: include/ferhip.h).
// The walk is serial -- a box is found at the end of the one in front -- and every loop in it advances a position by at least
// 8 bytes inside a container whose end is fixed, so it is bounded by the run's length whatever the bytes say.  Only the
// entries of a trun are many: they go to the caller's sink.
#define FER_MP4_OVERRUN 1
#define FER_MP4_MALFORMED 2
#define FER_MP4_UNSUP 3
#define FER_MP4_TRUNCATED 4

FER_MP4_HD uint32_t fer_mp4_be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
FER_MP4_HD uint64_t fer_mp4_be64(const uint8_t *p) { return (uint64_t)fer_mp4_be32(p) << 32 | fer_mp4_be32(p + 4); }

struct FerMp4Box {
    uint32_t type;
    uint64_t start, h, end;  // the box is r[start, end), its content begins at start + h
};

// the box at r[pos] of a container that ends at hi (pos < hi); false = malformed.  end - start >= 8.
FER_MP4_HD bool fer_mp4_box_at(const uint8_t *r, uint64_t pos, uint64_t hi, FerMp4Box &b)
{
    if (hi - pos < 8) return false;
    uint64_t size = fer_mp4_be32(r + pos);
    b.type = fer_mp4_be32(r + pos + 4);
    b.h = 8;
    if (size == 1) {
        if (hi - pos < 16) return false;
        size = fer_mp4_be64(r + pos + 8);
        b.h = 16;
    } else if (size == 0) {
        size = hi - pos;
    }
    if (size < b.h || size > hi - pos) return false;
    b.start = pos;
    b.end = pos + size;
    return true;
}

// every box of the container r[lo, hi) ends inside it.  Bounded: pos grows by >= 8 per step and stays below hi.
FER_MP4_HD bool fer_mp4_chain_ok(const uint8_t *r, uint64_t lo, uint64_t hi)
{
    FerMp4Box b;
    for (uint64_t pos = lo; pos < hi; pos = b.end)
        if (!fer_mp4_box_at(r, pos, hi, b)) return false;
    return true;
}

// What a moof says of its track.  sink.entries(sizes, count, e, dflt, at, index) records samples index .. index + count - 1:
// sample k has size be32(sizes + k e), or dflt where sizes is null, and begins where sample k - 1 ends, the first one at
// `at` (bytes from the run's first byte, possibly outside the run: nothing is read there); it returns where the last one ends.
// npend = the samples recorded, [lo, hi) = the bytes they cover (npend > 0).  Returns 0 or the fault.
template <typename Sink>
FER_MP4_HD int fer_mp4_moof(const uint8_t *r, const FerMp4Box &moof, uint64_t budget, uint64_t index, Sink &sink, uint64_t &npend, int64_t &lo,
                            int64_t &hi)
{
    const uint32_t TRAF = FER_MP4_FOURCC('t', 'r', 'a', 'f'), TRUN = FER_MP4_FOURCC('t', 'r', 'u', 'n'), TFHD = FER_MP4_FOURCC('t', 'f', 'h', 'd');
    npend = 0;
    if (!fer_mp4_chain_ok(r, moof.start + moof.h, moof.end)) return FER_MP4_MALFORMED;
    bool track = false;
    FerMp4Box c, k;
    for (uint64_t pos = moof.start + moof.h; pos < moof.end; pos = c.end) {  // (the chain is sound: bounded as fer_mp4_chain_ok)
        fer_mp4_box_at(r, pos, moof.end, c);
        if (c.type != TRAF) continue;
        const uint64_t klo = c.start + c.h, khi = c.end;
        if (!fer_mp4_chain_ok(r, klo, khi)) return FER_MP4_MALFORMED;
        uint32_t ntrun = 0;
        bool have_tf = false;
        FerMp4Box tf = {};
        for (uint64_t q = klo; q < khi; q = k.end) {
            fer_mp4_box_at(r, q, khi, k);
            ntrun += k.type == TRUN;
            if (k.type == TFHD && !have_tf) tf = k, have_tf = true;
        }
        if (!ntrun) continue;  // a track without samples here
        if (track) return FER_MP4_UNSUP;
        track = true;
        if (!have_tf) return FER_MP4_MALFORMED;
        const uint8_t *t = r + tf.start + tf.h;
        const uint64_t tlen = tf.end - tf.start - tf.h;
        if (tlen < 8) return FER_MP4_MALFORMED;
        const uint32_t tflags = fer_mp4_be32(t) & 0xFFFFFFu;
        if (tflags & 1u) return FER_MP4_UNSUP;  // base-data-offset
        uint64_t p = 8;
        bool has_default = false;
        uint32_t dflt = 0;
        for (uint32_t bit = 2u; bit <= 0x20u; bit <<= 1) {  // sample_description_index, default duration, size, flags
            if (bit == 4u || !(tflags & bit)) continue;
            if (p + 4 > tlen) return FER_MP4_MALFORMED;
            if (bit == 0x10u) dflt = fer_mp4_be32(t + p), has_default = true;
            p += 4;
        }
        bool first = true;
        int64_t after = 0;
        for (uint64_t q = klo; q < khi; q = k.end) {
            fer_mp4_box_at(r, q, khi, k);
            if (k.type != TRUN) continue;
            const uint8_t *u = r + k.start + k.h;
            const uint64_t ulen = k.end - k.start - k.h;
            if (ulen < 8) return FER_MP4_MALFORMED;
            if (u[0] > 1) return FER_MP4_UNSUP;
            const uint32_t flags = fer_mp4_be32(u) & 0xFFFFFFu, count = fer_mp4_be32(u + 4);
            p = 8;
            int64_t at = after;
            if (flags & 1u) {
                if (p + 4 > ulen) return FER_MP4_MALFORMED;
                at = (int64_t)moof.start + (int32_t)fer_mp4_be32(u + p);
                p += 4;
            } else if (first) {
                return FER_MP4_UNSUP;
            }
            if (flags & 4u) {  // first_sample_flags
                if (p + 4 > ulen) return FER_MP4_MALFORMED;
                p += 4;
            }
            const uint32_t e = 4u * (((flags >> 8) & 1u) + ((flags >> 9) & 1u) + ((flags >> 10) & 1u) + ((flags >> 11) & 1u));
            if ((uint64_t)count * e > ulen - p) return FER_MP4_MALFORMED;
            // entries of no bytes are bounded by nothing else: a run of n bytes then holds at most n samples in all
            if (e == 0 && count > (budget > npend ? budget - npend : 0)) return FER_MP4_MALFORMED;
            if (count && !(flags & 0x200u) && !has_default) return FER_MP4_MALFORMED;
            const int64_t end = sink.entries((flags & 0x200u) ? u + p + ((flags & 0x100u) ? 4 : 0) : nullptr, count, e, dflt, at, index + npend);
            if (count) {
                lo = npend ? (at < lo ? at : lo) : at;
                hi = npend ? (end > hi ? end : hi) : end;
            }
            npend += count;
            after = end;
            first = false;
        }
    }
    return 0;
}

// One run r[0, n) of a stream: the samples of its whole fragments are recorded at index `done` onwards, and `done` moves
// behind them; the samples of a fragment that does not complete are recorded behind `done` and never counted.  Returns 0 or
// the fault that ended the walk.  Every sample that counts lies inside an mdat, hence inside the run.
template <typename Sink>
FER_MP4_HD int fer_mp4_walk_run(const uint8_t *r, uint64_t n, uint64_t &done, Sink &sink)
{
    const uint32_t MOOF = FER_MP4_FOURCC('m', 'o', 'o', 'f'), MDAT = FER_MP4_FOURCC('m', 'd', 'a', 't');
    const uint64_t budget = n;
    uint64_t taken = 0, npend = 0;
    int64_t lo = 0, hi = 0;
    bool pending = false;
    FerMp4Box b;
    for (uint64_t pos = 0; pos < n; pos = b.end) {  // bounded: pos grows by >= 8 per step and stays below n
        if (!fer_mp4_box_at(r, pos, n, b)) return FER_MP4_MALFORMED;
        if (b.type == MOOF) {
            if (pending) return FER_MP4_TRUNCATED;
            if (int f = fer_mp4_moof(r, b, budget > taken ? budget - taken : 0, done, sink, npend, lo, hi)) return f;
            pending = true;
        } else if (b.type == MDAT && pending) {
            if (npend && (lo < (int64_t)(b.start + b.h) || hi > (int64_t)b.end)) return FER_MP4_MALFORMED;
            done += npend;
            taken += npend;
            pending = false;
        }
    }
    return pending ? FER_MP4_TRUNCATED : 0;
}

// the content of the avcC box of an initialisation segment: moov, trak, mdia, minf, stbl, stsd, the first entry (avc1 or
// avc3), and behind the 78 bytes of its visual sample entry the child avcC.  false if anything is missing or overruns.
static inline bool fer_mp4_find_avcc(const uint8_t *r, size_t n, size_t *off, size_t *len)
{
    const uint32_t path[6] = {FER_MP4_FOURCC('m', 'o', 'o', 'v'), FER_MP4_FOURCC('t', 'r', 'a', 'k'), FER_MP4_FOURCC('m', 'd', 'i', 'a'),
                              FER_MP4_FOURCC('m', 'i', 'n', 'f'), FER_MP4_FOURCC('s', 't', 'b', 'l'), FER_MP4_FOURCC('s', 't', 's', 'd')};
    uint64_t lo = 0, hi = n;
    FerMp4Box b = {};
    // the first box of the wanted type in r[lo, hi), every box in front of it and behind it sound
    const auto find = [&](uint32_t want) {
        if (lo > hi || !fer_mp4_chain_ok(r, lo, hi)) return false;
        for (uint64_t pos = lo; pos < hi; pos = b.end) {
            fer_mp4_box_at(r, pos, hi, b);
            if (b.type == want) return true;
        }
        return false;
    };
    for (uint32_t want : path) {
        if (!r || !find(want)) return false;
        lo = b.start + b.h, hi = b.end;
    }
    lo += 8;  // version and flags, entry_count
    if (lo >= hi || !fer_mp4_chain_ok(r, lo, hi)) return false;
    fer_mp4_box_at(r, lo, hi, b);
    if (b.type != FER_MP4_FOURCC('a', 'v', 'c', '1') && b.type != FER_MP4_FOURCC('a', 'v', 'c', '3')) return false;
    lo = b.start + b.h + 78, hi = b.end;
    if (!find(FER_MP4_FOURCC('a', 'v', 'c', 'C'))) return false;
    *off = (size_t)(b.start + b.h);
    *len = (size_t)(b.end - b.start - b.h);
    return true;
}
