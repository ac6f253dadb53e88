// What the decoder's host side reads of a caller's bytes (h264-fer_amd/csrc/fer_dec_syntax_host.h: bit reader, SPS / PPS / slice
// header parsers, Annex-B and length-prefixed splitters, configuration record walk) as a stand-alone program, for a run under
// a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/dec_syntax_host_check.cpp -o dec_syntax_host_check && ./dec_syntax_host_check
// Every input is a heap array of exactly the stated length and every RBSP store starts empty, so a reader that leaves what it
// was given is an error.  Without arguments it checks constructed streams, headers and records and every truncation of them.
//   dec_syntax_host_check FILE [L]
// lists the units that split_stream (or, with a length size L, split_avcc) keeps of a file: type, ref_idc, RBSP bytes, Adler-32.
// No header with adaptive_ref_pic_marking_mode_flag = 1 is truncated here: that loop of dec_parse_slice_header has no bound
// (open items).
#include "../h264-fer_amd/csrc/fer_dec_syntax_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <memory>

typedef std::vector<uint8_t> Bytes;
static int fails = 0;
#define EXPECT(x)                                              \
    do {                                                       \
        if (!(x)) {                                            \
            printf("line %d: %s\n", __LINE__, #x);             \
            fails++;                                           \
        }                                                      \
    } while (0)

struct Heap {  // exactly n bytes on the heap
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    Heap(const Bytes &b, size_t len) : p(new uint8_t[len]), n(len) { memcpy(p.get(), b.data(), len); }
};
static uint32_t rng_state = 20251020u;
static uint32_t rnd(uint32_t m)  // seeded: the same streams in every run
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (rng_state >> 8) % m;
}

struct Unit {
    int type, ref_idc;
    Bytes rbsp;
    bool operator==(const Unit &o) const { return type == o.type && ref_idc == o.ref_idc && rbsp == o.rbsp; }
};
static std::vector<Unit> units_of(const std::vector<NalRef> &nals)
{
    std::vector<Unit> u;
    for (const NalRef &n : nals) u.push_back({n.type, n.ref_idc, Bytes(n.rbsp.data(), n.rbsp.data() + n.rbsp.size())});
    return u;
}
// s[st+1..en) without every 03 behind two zeros of the payload: the rule, byte by byte
static Unit unit_at(const Bytes &s, size_t st, size_t en)
{
    Unit u{s[st] & 0x1f, (s[st] & 0x7f) >> 5, {}};
    for (size_t p = st + 1; p < en; p++)
        if (!(s[p] == 3 && p >= st + 3 && s[p - 1] == 0 && s[p - 2] == 0)) u.rbsp.push_back(s[p]);
    return u;
}
// The documented rules of split_stream: a unit begins behind every 00 00 00 01, ends at the first 00 00 00 / 00 00 01 whose
// three bytes lie in the range, else at its end; an empty unit is none; a unit without payload ends the range.
static std::vector<Unit> model_annexb(const Bytes &s)
{
    std::vector<Unit> out;
    const size_t n = s.size();
    for (size_t z = 0; z + 3 < n; z++) {
        if (s[z] || s[z + 1] || s[z + 2] || s[z + 3] != 1) continue;
        size_t st = z + 4, en = n;
        for (size_t i = st; i + 2 < n; i++)
            if (!s[i] && !s[i + 1] && s[i + 2] <= 1) {
                en = i;
                break;
            }
        if (en <= st) continue;
        Unit u = unit_at(s, st, en);
        if (u.rbsp.empty()) break;
        out.push_back(u);
    }
    return out;
}
// ... and of split_avcc (include/ferhip.h): fault = the range overran or cannot state a length
static std::vector<Unit> model_avcc(const Bytes &s, int L, int &fault)
{
    std::vector<Unit> out;
    size_t pos = 0;
    fault = 0;
    while (pos + L <= s.size()) {
        size_t len = 0;
        for (int k = 0; k < L; k++) len = len * 256 + s[pos + k];
        const size_t st = pos + L;
        if (len == 0) return out;
        if (len > s.size() - st) return fault = 1, out;
        if (len == 1) return out;
        out.push_back(unit_at(s, st, st + len));
        pos = st + len;
    }
    fault = pos < s.size();
    return out;
}
static std::vector<Unit> run_annexb(const Bytes &s, size_t n)
{
    Heap h(s, n);
    std::vector<NalRef> nals;
    Bytes store;
    split_stream(h.p.get(), n, nals, store);
    return units_of(nals);
}
static std::vector<Unit> run_avcc(const Bytes &s, size_t n, int L, int &fault)
{
    Heap h(s, n);
    std::vector<NalRef> nals;
    Bytes store;
    fault = split_avcc(h.p.get(), n, L, nals, store);
    return units_of(nals);
}

static Bytes escape(const Bytes &rbsp)  // 03 in front of every byte <= 3 behind two zeros
{
    Bytes out;
    int zeros = 0;
    for (uint8_t b : rbsp) {
        if (zeros >= 2 && b <= 3) out.push_back(3), zeros = 0;
        out.push_back(b);
        zeros = b ? 0 : zeros + 1;
    }
    return out;
}
// seeded RBSP with runs of 00 00 0x in it; zeros_at_end of them behind a last non-zero byte
static Bytes draw_rbsp(size_t n, int zeros_at_end)
{
    static const uint8_t alphabet[] = {0, 0, 0, 0, 1, 2, 3, 3, 0x41, 0xab, 0xff};
    Bytes r;
    for (size_t i = 0; i < n; i++) r.push_back(alphabet[rnd(sizeof alphabet)]);
    for (const uint8_t x : {0, 0, 0, 0, 0, 1, 0, 0, 2, 0, 0, 3, 0x80}) r.push_back(x);
    r.insert(r.end(), (size_t)zeros_at_end, (uint8_t)0);
    return r;
}
static void append(Bytes &s, const Bytes &b) { s.insert(s.end(), b.begin(), b.end()); }

static std::vector<Bytes> splitter_streams;  // kept for the truncation runs
static void splitters_constructed()
{
    for (int round = 0; round < 24; round++) {
        // Annex-B: clean units (4-byte code, a header byte that is not 00, no zero at the end) must come back as they were written
        std::vector<Unit> clean;
        Bytes s;
        for (int k = 0; k < 5; k++) {
            Unit u{1 + (int)rnd(31), (int)rnd(4), draw_rbsp(rnd(60), 0)};
            append(s, {0, 0, 0, 1, (uint8_t)(u.ref_idc << 5 | u.type)});
            append(s, escape(u.rbsp));
            clean.push_back(u);
        }
        EXPECT(run_annexb(s, s.size()) == clean);
        EXPECT(model_annexb(s) == clean);
        // ... then units behind 3-byte codes, units that end in zeros, a code right behind a code, a header-only unit
        for (int k = 0; k < 6; k++) {
            const int code = rnd(2) ? 3 : 4;
            append(s, code == 4 ? Bytes{0, 0, 0, 1} : Bytes{0, 0, 1});
            if (k == 3 && round % 3 == 0) continue;
            s.push_back((uint8_t)rnd(128));
            if (k == 5 && round % 4 == 1) continue;
            append(s, escape(draw_rbsp(rnd(40), (int)rnd(4))));
        }
        EXPECT(run_annexb(s, s.size()) == model_annexb(s));
        if (round < 3) splitter_streams.push_back(s);
    }
    for (int L : {1, 2, 4})
        for (int round = 0; round < 12; round++) {
            std::vector<Unit> clean;
            Bytes s;
            auto put = [&](size_t len, const Bytes &body) {
                for (int k = L - 1; k >= 0; k--) s.push_back((uint8_t)(len >> (8 * k)));
                append(s, body);
            };
            for (int k = 0; k < 4; k++) {
                Unit u{(int)rnd(32), (int)rnd(4), draw_rbsp(rnd(50), (int)rnd(3))};
                Bytes body{(uint8_t)(u.ref_idc << 5 | u.type)};
                append(body, escape(u.rbsp));
                put(body.size(), body);
                clean.push_back(u);
            }
            int fault = -1, mf = -1;
            EXPECT(run_avcc(s, s.size(), L, fault) == clean && fault == 0);
            if (round < 1) splitter_streams.push_back(s);
            // what ends a range, and what it returns
            const Bytes head = s;
            const int want[5] = {0, 0, 1, 1, L > 1};
            for (int end = 0; end < 5; end++) {
                s = head;
                if (end == 0) put(0, {});                // a zero length
                if (end == 1) put(1, {0x65});            // a header-only unit
                if (end == 2) put(9, {0x65, 1, 2, 3});   // a unit that overruns
                if (end == 3) put(L == 1 ? 255 : 65535, {0x65});
                if (end == 4) s.insert(s.end(), (size_t)(L - 1), (uint8_t)0);  // fewer than L bytes left
                if (end < 2) put(3, {0x41, 7, 7});       // (what follows a unit that ends the range is not looked at)
                EXPECT(run_avcc(s, s.size(), L, fault) == clean && fault == want[end]);
                EXPECT(model_avcc(s, L, mf) == clean && mf == want[end]);
            }
        }
}

// every prefix of a few streams through both splitters: nothing is asserted beyond the agreement with the byte-wise rules;
// the run must stay inside the arrays
static void splitters_truncated()
{
    for (const Bytes &s : splitter_streams)
        for (size_t n = 0; n <= s.size(); n++) {
            const Bytes pre(s.begin(), s.begin() + n);
            EXPECT(run_annexb(s, n) == model_annexb(pre));
            for (int L : {1, 2, 4}) {
                int fault = -1, mf = -1;
                EXPECT(run_avcc(s, n, L, fault) == model_avcc(pre, L, mf) && fault == mf);
            }
        }
}

struct Bits {  // a header, written bit by bit
    Bytes b;
    size_t n = 0;
    void put(int k, unsigned v)
    {
        for (int i = k - 1; i >= 0; i--, n++) {
            if (n % 8 == 0) b.push_back(0);
            b[n / 8] |= (v >> i & 1u) << (7 - n % 8);
        }
    }
    void ue(unsigned v)
    {
        int z = 0;
        while ((v + 1) >> (z + 1)) z++;
        put(z, 0);
        put(z + 1, v + 1);
    }
    void se(int v) { ue(v > 0 ? 2 * v - 1 : -2 * v); }
};

// 48 x 32, log2_max_frame_num 9, poc type 0 with 10 bits; mark = the bit behind frame_mbs_only_flag, crop_end = the bit
// behind the last cropping offset
static Bits write_sps(unsigned profile, unsigned frame_mbs_only, bool crop, size_t *mark = nullptr, size_t *crop_end = nullptr)
{
    Bits w;
    w.put(8, profile), w.put(16, 0x001e), w.ue(0), w.ue(5), w.ue(0), w.ue(6), w.ue(1), w.put(1, 0), w.ue(2), w.ue(1);
    w.put(1, frame_mbs_only);
    if (mark) *mark = w.n;
    w.put(1, 1), w.put(1, crop);
    if (crop) w.ue(1), w.ue(2), w.ue(0), w.ue(3);
    if (crop_end) *crop_end = w.n;
    w.put(1, 0), w.put(1, 1);
    return w;
}
// pic_init_qp 28, chroma_qp_index_offset -2, deblocking_filter_control_present_flag 1; mark = the bit behind
// num_ref_idx_l0_default_active_minus1
static Bits write_pps(unsigned cabac, unsigned groups, unsigned l0, size_t *mark = nullptr)
{
    Bits w;
    w.ue(0), w.ue(0), w.put(1, cabac), w.put(1, 0), w.ue(groups), w.ue(l0);
    if (mark) *mark = w.n;
    w.ue(0), w.put(3, 0), w.se(2), w.se(0), w.se(-2), w.put(1, 1), w.put(1, 0), w.put(1, 0), w.put(1, 1);
    return w;
}
static int parse_sps(DecHdr &h, const Bits &w, size_t len)
{
    Heap in(w.b, len);
    HostBR r{in.p.get(), len, 0};
    return dec_parse_sps(h, r);
}
static int parse_pps(DecHdr &h, const Bits &w, size_t len)
{
    Heap in(w.b, len);
    HostBR r{in.p.get(), len, 0};
    return dec_parse_pps(h, r);
}

static void parameter_sets(DecHdr &h)
{
    size_t mark = 0, crop_end = 0;
    Bits sps = write_sps(66, 1, false, &mark);
    h = DecHdr{};
    EXPECT(parse_sps(h, sps, sps.b.size()) == 0);
    EXPECT(h.have_sps == 1 && h.W == 48 && h.H == 32 && h.log2_max_frame_num == 9 && h.poc_type == 0 && h.log2_max_poc_lsb == 10);
    EXPECT(!h.crop[0] && !h.crop[1] && !h.crop[2] && !h.crop[3]);
    for (size_t len = 0; len < sps.b.size(); len++) {  // zeros past the end: frame_mbs_only_flag reads as 0 when it is cut off
        DecHdr t{};
        EXPECT(parse_sps(t, sps, len) == (len * 8 >= mark ? 0 : FERHIP_E_UNSUP));
    }
    DecHdr t{};
    EXPECT(parse_sps(t, write_sps(100, 1, false), sps.b.size()) == FERHIP_E_UNSUP);
    EXPECT(parse_sps(t, write_sps(244, 1, false), sps.b.size()) == FERHIP_E_UNSUP);
    EXPECT(parse_sps(t, write_sps(66, 0, false), sps.b.size()) == FERHIP_E_UNSUP && !t.have_sps);
    // cropping: reported when the offsets are followed by more of the SPS, else the picture counts as uncropped
    Bits crop = write_sps(66, 1, true, &mark, &crop_end);
    EXPECT(parse_sps(t, crop, crop.b.size()) == 0 && t.crop[0] == 2 && t.crop[1] == 4 && t.crop[2] == 0 && t.crop[3] == 6);
    for (size_t len = 0; len < crop.b.size(); len++) {
        DecHdr u{};
        const int rc = parse_sps(u, crop, len);
        EXPECT(rc == (len * 8 >= mark ? 0 : FERHIP_E_UNSUP));
        const bool whole = len * 8 > crop_end;
        if (!rc) EXPECT(whole ? u.crop[0] == 2 && u.crop[1] == 4 && u.crop[2] == 0 && u.crop[3] == 6 : !u.crop[0] && !u.crop[1] && !u.crop[2] && !u.crop[3]);
    }
    Bits pps = write_pps(0, 0, 0, &mark);
    EXPECT(parse_pps(h, pps, pps.b.size()) == 0);
    EXPECT(h.have_pps == 1 && h.pic_init_qp == 28 && h.chroma_qp_offset == -2 && h.deblock_ctl == 1 && h.constrained_intra == 0);
    for (size_t len = 0; len < pps.b.size(); len++) {  // a ue that is cut off reads as 2^24 - 1: slice groups
        DecHdr u{};
        EXPECT(parse_pps(u, pps, len) == (len * 8 >= mark ? 0 : FERHIP_E_UNSUP));
    }
    EXPECT(parse_pps(t, write_pps(1, 0, 0), pps.b.size()) == FERHIP_E_UNSUP);
    EXPECT(parse_pps(t, write_pps(0, 1, 0), pps.b.size()) == FERHIP_E_UNSUP);
    EXPECT(parse_pps(t, write_pps(0, 0, 1), pps.b.size()) == FERHIP_E_UNSUP);
}

// one slice header at its full length (want[4] = info) and at every shorter one.  Cut short it may parse as another header,
// but one that is accepted must say that it ran past its end: the parse of a prefix follows the full one until it leaves it.
static void slice_header(const DecHdr &ps, const Bits &w, int nal_type, int ref_idc, const uint32_t *want, int want_ov)
{
    const size_t bits = w.n;
    Bits full = w;
    full.put(1, 1), full.put(15, 0x1234);  // (slice data)
    for (size_t len = 0; len <= full.b.size(); len++) {
        Heap in(full.b, len);
        DecHdr h = ps;
        uint32_t info[4] = {~0u, ~0u, ~0u, ~0u};
        int ov = 0;
        const int rc = dec_parse_slice_header(h, in.p.get(), len, nal_type, ref_idc, info, ov);
        if (len * 8 >= bits) {
            EXPECT(rc == 0 && info[0] == len && info[1] == bits && info[2] == want[2] && info[3] == want[3] && ov == want_ov);
        } else {
            EXPECT(rc == 0 || rc == FERHIP_E_UNSUP);
            if (!rc) EXPECT(info[0] == len && info[1] > len * 8 && info[1] != ~0u);
        }
    }
}

static void slice_headers(const DecHdr &ps)
{
    DecHdr none{};
    uint32_t info[4];
    int ov = 0;
    const uint8_t one = 0x80;
    EXPECT(dec_parse_slice_header(none, &one, 1, 5, 3, info, ov) == FERHIP_E_STATE);
    Bits idr;  // I slice of an IDR picture: SliceQPY 28 - 3, the filter off
    idr.ue(0), idr.ue(7), idr.ue(0), idr.put(9, 0), idr.ue(1), idr.put(10, 0), idr.put(2, 0), idr.se(-3), idr.ue(1);
    const uint32_t want_idr[4] = {0, 0, 2, 25};
    slice_header(ps, idr, 5, 3, want_idr, 0);
    // P slice: reference count override, one list modification entry, adaptive_ref_pic_marking_mode_flag 0, filter offsets
    Bits p;
    p.ue(0), p.ue(5), p.ue(0), p.put(9, 3), p.put(10, 6), p.put(1, 1), p.ue(0), p.put(1, 1), p.ue(0), p.ue(2), p.ue(3), p.put(1, 0);
    p.se(2), p.ue(0), p.se(1), p.se(-1);
    const uint32_t want_p[4] = {0, 0, 0u | 1u << 8, 30};
    slice_header(ps, p, 1, 2, want_p, 1);
    DecHdr h = ps;
    EXPECT(dec_parse_slice_header(h, p.b.data(), p.b.size(), 1, 2, info, ov) == 0 && h.mod_flag == 1 && h.mod_copies == 1 && h.nref_active_minus1 == 0);
    Bits b;  // a B slice is parsed to its end and refused
    b.ue(0), b.ue(1), b.ue(0), b.put(9, 3), b.put(10, 6), b.put(1, 0), b.put(1, 0), b.put(1, 0), b.se(0), b.ue(1);
    EXPECT(dec_parse_slice_header(h, b.b.data(), b.b.size(), 1, 2, info, ov) == FERHIP_E_UNSUP);
}

static void config_record()
{
    const Bytes sps{0x67, 66, 0, 30, 1, 2, 3}, pps0{0x68, 9}, pps1{0x68, 0, 0, 3, 1};
    Bytes rec{1, 66, 0, 30, 0xff, 0xe1, 0, (uint8_t)sps.size()};
    append(rec, sps);
    append(rec, {2, 0, (uint8_t)pps0.size()});
    append(rec, pps0);
    append(rec, {0, (uint8_t)pps1.size()});
    append(rec, pps1);
    std::vector<AvccSpan> u;
    size_t longest = 0;
    auto walk = [&](const Bytes &r, size_t n) {
        Heap h(r, n);
        return split_avcc_config(h.p.get(), n, u, longest);
    };
    EXPECT(walk(rec, rec.size()) == 0 && u.size() == 3 && longest == 7);
    if (u.size() == 3) EXPECT(u[0].at == 8 && u[0].len == 7 && u[1].at == 18 && u[1].len == 2 && u[2].at == 22 && u[2].len == 5 && u[2].at + u[2].len == rec.size());
    for (size_t n = 0; n < rec.size(); n++) EXPECT(walk(rec, n) == FERHIP_E_ARG);
    EXPECT(split_avcc_config(nullptr, 40, u, longest) == FERHIP_E_ARG);
    Bytes r = rec;
    r.push_back(0x55);  // (what follows the last PPS is not looked at)
    EXPECT(walk(r, r.size()) == 0 && u.size() == 3);
    r = rec, r[0] = 0;  // another version
    EXPECT(walk(r, r.size()) == FERHIP_E_ARG);
    r = rec, r[5] = 0xe0;  // no SPS
    EXPECT(walk(r, r.size()) == FERHIP_E_ARG);
    r = rec, r[15] = 0;  // no PPS
    EXPECT(walk(r, r.size()) == FERHIP_E_ARG);
    r = rec, r[7] = 0;  // an SPS of length zero
    EXPECT(walk(r, r.size()) == FERHIP_E_ARG);
    r = rec, r[21] = 0;  // a PPS of length zero
    EXPECT(walk(r, r.size()) == FERHIP_E_ARG);
    r = rec, r[21] = 6;  // a PPS that is longer than the record
    EXPECT(walk(r, r.size()) == FERHIP_E_ARG);
}

static int list_file(const char *path, int L)
{
    FILE *f = fopen(path, "rb");
    if (!f) return printf("cannot read %s\n", path), 1;
    Bytes s;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + k);
    fclose(f);
    int fault = 0;
    for (const Unit &u : L ? run_avcc(s, s.size(), L, fault) : run_annexb(s, s.size())) {
        uint32_t a = 1, b = 0;
        for (uint8_t x : u.rbsp) a = (a + x) % 65521u, b = (b + a) % 65521u;
        printf("%d %d %zu %u\n", u.type, u.ref_idc, u.rbsp.size(), b << 16 | a);
    }
    if (L) printf("overrun %d\n", fault);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        const int L = argc > 2 ? atoi(argv[2]) : 0;
        if (L != 0 && L != 1 && L != 2 && L != 4) return printf("length size %s\n", argv[2]), 1;
        return list_file(argv[1], L);
    }
    splitters_constructed();
    splitters_truncated();
    DecHdr ps;
    parameter_sets(ps);
    slice_headers(ps);
    config_record();
    printf(fails ? "%d checks failed\n" : "dec_syntax_host_check ok\n", fails);
    return fails != 0;
}
