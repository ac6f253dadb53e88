// The fragmented MP4 code that runs on the host (h264-fer_amd/csrc/fer_mp4_host.h, and split_mp4 of fer_dec_syntax_host.h) as a
// stand-alone program, for a run under a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/mp4_host_check.cpp -o mp4_host_check && ./mp4_host_check
// Every run is a heap array of exactly its length and the RBSP store starts empty, so a reader that leaves what it was given
// is an error; the words of a segment's front (fer_mp4_front_word) are the very function the close kernel runs.  Without arguments it checks
// constructed fragments, every truncation and every damaged header byte of them, and runs of drawn bytes.
//   mp4_host_check FILE L          the units split_mp4 keeps of a file (one run) in the format of dec_syntax_host_check (type,
//                                  ref_idc, RBSP bytes, Adler-32), then "samples N" and "fault F"
//   mp4_host_check FILE L trunc    for every k from 0 to the file's length: "k N F" of the run's first k bytes
//   mp4_host_check init SPS PPS DW DH TIMESCALE   (units in hex) the initialisation segment in hex, then "avcc OFF LEN"
//   mp4_host_check front N K M DECODE_TIME SEQUENCE   the first D bytes of a closed region in hex, trun entries as zeros
//   mp4_host_check avcc FILE       "avcc OFF LEN" of fer_mp4_find_avcc, or "none"
#include "../h264-fer_amd/csrc/fer_dec_syntax_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <string>

typedef std::vector<uint8_t> Bytes;
static int fails = 0;
#define EXPECT(x)                                              \
    do {                                                       \
        if (!(x)) {                                            \
            printf("line %d: %s\n", __LINE__, #x);             \
            fails++;                                           \
        }                                                      \
    } while (0)

static uint32_t rng_state = 20261021u;
static uint32_t rnd(uint32_t m)  // seeded: the same bytes in every run
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (rng_state >> 8) % m;
}

struct Unit {
    int type, ref_idc;
    Bytes rbsp;
    bool operator==(const Unit &o) const { return type == o.type && ref_idc == o.ref_idc && rbsp == o.rbsp; }
};
struct Result {
    std::vector<Unit> units;
    std::vector<Mp4Span> spans;
    int fault;
};

// split_mp4 over copies of the runs that are exactly as long as they are
static Result run(const std::vector<Bytes> &runs, int L)
{
    std::vector<std::unique_ptr<uint8_t[]>> heap;
    std::vector<TsRun> rn;
    for (const Bytes &b : runs) {
        heap.emplace_back(new uint8_t[b.size()]);
        if (!b.empty()) memcpy(heap.back().get(), b.data(), b.size());
        rn.push_back({heap.back().get(), b.size()});
    }
    std::vector<NalRef> nals;
    Bytes store;
    Result r;
    r.fault = split_mp4(rn.data(), rn.size(), L, nals, store, &r.spans);
    for (const NalRef &n : nals) r.units.push_back({n.type, n.ref_idc, Bytes(n.rbsp.data(), n.rbsp.data() + n.rbsp.size())});
    return r;
}

static void put32(Bytes &b, uint32_t x)
{
    for (int k = 3; k >= 0; k--) b.push_back((uint8_t)(x >> (8 * k)));
}
static Bytes box(const char *type, const Bytes &content)
{
    Bytes b;
    put32(b, (uint32_t)(8 + content.size()));
    b.insert(b.end(), type, type + 4);
    b.insert(b.end(), content.begin(), content.end());
    return b;
}
static Bytes join(const std::vector<Bytes> &v)
{
    Bytes o;
    for (const Bytes &b : v) o.insert(o.end(), b.begin(), b.end());
    return o;
}

// a fragment as the library writes it: the front of fer_mp4_front_word with the trun entries filled in, then the samples
static Bytes fragment(const std::vector<Bytes> &samples, uint32_t K, uint32_t seq)
{
    const uint32_t D = fer_mp4_data_offset(K), n = (uint32_t)samples.size();
    uint32_t M = 0;
    for (const Bytes &s : samples) M += (uint32_t)s.size();
    Bytes out;
    for (uint32_t w = 0; w < D / 4; w++) {
        bool keep;
        uint32_t x = fer_mp4_front_word(w, n, D, M, 0x100000000ull + seq, seq, &keep);
        if (keep) {
            const uint32_t k = (w - 22) / 3, f = (w - 22) % 3;
            x = f == 0 ? 3000u : f == 1 ? (uint32_t)samples[k].size() : fer_mp4_sample_flags(k == 0);
        }
        put32(out, x);
    }
    for (const Bytes &s : samples) out.insert(out.end(), s.begin(), s.end());
    return out;
}
static Bytes sample(uint8_t hdr, const Bytes &payload)
{
    Bytes s;
    put32(s, (uint32_t)payload.size() + 1);
    s.push_back(hdr);
    s.insert(s.end(), payload.begin(), payload.end());
    return s;
}

static void constructed()
{
    const Bytes s0 = sample(0x65, {1, 2, 0, 0, 3, 1, 9}), s1 = sample(0x41, {7}), s2 = sample(0x41, Bytes(40, 0xAB));
    const Bytes f0 = fragment({s0, s1}, 2, 1), f1 = fragment({s2}, 6, 2);
    const std::vector<Unit> u0 = {{5, 3, {1, 2, 0, 0, 1, 9}}, {1, 2, {7}}}, u1 = {{1, 2, Bytes(40, 0xAB)}};
    std::vector<Unit> both = u0;
    both.insert(both.end(), u1.begin(), u1.end());
    Result r = run({join({f0, f1})}, 4);
    EXPECT(r.fault == 0 && r.units == both && r.spans.size() == 3);
    r = run({f0, f1}, 4);  // a run per fragment
    EXPECT(r.fault == 0 && r.units == both);
    r = run({}, 4);
    EXPECT(r.fault == 0 && r.units.empty());
    r = run({join({box("styp", Bytes(8, 'x')), f0, box("free", {}), f1, box("zzzz", {1})})}, 4);
    EXPECT(r.fault == 0 && r.units == both);
    Bytes sb = s1;
    sb[3] = 9;  // a unit that claims more than its sample holds: the units in front stand, nothing behind it is taken
    r = run({fragment({s0, sb, s2}, 3, 1)}, 4);
    EXPECT(r.fault == FER_MP4_OVERRUN && r.spans.size() == 2 && r.units == std::vector<Unit>(u0.begin(), u0.begin() + 1));
    // every truncation: a fault unless the cut falls between fragments, and exactly the whole fragments' units
    const Bytes all = join({f0, f1});
    for (size_t k = 0; k <= all.size(); k++) {
        r = run({Bytes(all.begin(), all.begin() + k)}, 4);
        const bool whole = k == 0 || k == f0.size() || k == all.size();
        EXPECT((r.fault == 0) == whole);
        EXPECT(r.fault == 0 || r.fault == FER_MP4_MALFORMED || r.fault == FER_MP4_TRUNCATED);
        EXPECT(r.units == (k == all.size() ? both : k >= f0.size() ? u0 : std::vector<Unit>()));
    }
    // every byte of the two fronts damaged in turn: no read leaves the run, and what stands is a prefix of the units
    for (size_t k = 0; k < all.size(); k++) {
        if (k >= fer_mp4_data_offset(2) && k < f0.size()) continue;  // (the first fragment's samples)
        if (k >= f0.size() + fer_mp4_data_offset(6)) break;
        for (int v : {0x00, 0x01, 0xFF, 0x80, 0x10}) {
            Bytes cut = all;
            cut[k] = (uint8_t)v;
            r = run({cut}, 4);
            EXPECT(r.fault >= 0 && r.fault <= 4 && r.spans.size() <= cut.size());
            for (const Mp4Span &sp : r.spans) EXPECT(sp.at <= cut.size() && sp.len <= cut.size() - sp.at);
        }
    }
    // the front word function against the model's table, by the boxes it forms
    size_t off = 0, len = 0;
    EXPECT(!fer_mp4_find_avcc(all.data(), all.size(), &off, &len));
    const Bytes sps = {0x67, 0x42, 0x00, 0x1e, 0xab}, pps = {0x68, 0xce, 0x38, 0x80};
    const Bytes ini = fer_mp4_init_segment(sps.data(), sps.size(), pps.data(), pps.size(), 64, 48, 90000);
    EXPECT(!ini.empty() && fer_mp4_find_avcc(ini.data(), ini.size(), &off, &len));
    EXPECT(Bytes(ini.begin() + off, ini.begin() + off + len) == fer_mp4_avcc_record(sps.data(), sps.size(), pps.data(), pps.size()));
    for (size_t k = 0; k < ini.size(); k++) {  // truncated: never found, never read beyond
        std::unique_ptr<uint8_t[]> h(new uint8_t[k ? k : 1]);
        memcpy(h.get(), ini.data(), k);
        EXPECT(!fer_mp4_find_avcc(h.get(), k, &off, &len));
    }
    for (size_t k = 0; k < ini.size(); k++)
        for (int v : {0x00, 0xFF, 0x01}) {
            std::unique_ptr<uint8_t[]> h(new uint8_t[ini.size()]);
            memcpy(h.get(), ini.data(), ini.size());
            h[k] = (uint8_t)v;
            if (fer_mp4_find_avcc(h.get(), ini.size(), &off, &len)) EXPECT(off <= ini.size() && len <= ini.size() - off);
        }
    EXPECT(fer_mp4_init_segment(sps.data(), sps.size(), pps.data(), pps.size(), 64, 48, 0).empty());
    EXPECT(fer_mp4_init_segment(sps.data(), 3, pps.data(), pps.size(), 64, 48, 1).empty());
    EXPECT(fer_mp4_init_segment(sps.data(), sps.size(), pps.data(), pps.size(), 0, 48, 1).empty());
}

static void drawn()
{
    static const char *types[] = {"moof", "traf", "trun", "tfhd", "mdat", "free", "mfhd", "zzzz"};
    for (int k = 0; k < 20000; k++) {
        std::vector<Bytes> runs(1 + rnd(2));
        size_t total = 0;
        for (Bytes &p : runs) {
            p.resize(rnd(400));
            for (uint8_t &b : p) b = (uint8_t)(rnd(4) ? rnd(4) : rnd(256));
            // box headers at drawn places: sizes that mostly fit, known types
            for (size_t o = 0; o + 8 <= p.size() && rnd(8); o += 8 + rnd(24)) {
                const uint32_t size = rnd(6) ? 8 + rnd((uint32_t)(p.size() - o)) : rnd(3);
                p[o] = p[o + 1] = 0, p[o + 2] = (uint8_t)(size >> 8), p[o + 3] = (uint8_t)size;
                memcpy(&p[o + 4], types[rnd(8)], 4);
            }
            total += p.size();
        }
        const Result r = run(runs, 1 << rnd(3));
        size_t bytes = 0;
        for (const Unit &u : r.units) bytes += u.rbsp.size();
        EXPECT(bytes <= total && r.fault >= 0 && r.fault <= 4);
        for (const Mp4Span &sp : r.spans) EXPECT(sp.run < runs.size() && sp.at <= runs[sp.run].size() && sp.len <= runs[sp.run].size() - sp.at);
    }
}

static Bytes read_file(const char *path, bool &ok)
{
    Bytes s;
    FILE *f = fopen(path, "rb");
    ok = f != nullptr;
    if (!f) return s;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + k);
    fclose(f);
    return s;
}
static Bytes unhex(const char *h)
{
    Bytes b;
    for (size_t k = 0; h[k] && h[k + 1]; k += 2) b.push_back((uint8_t)strtoul(std::string(h + k, 2).c_str(), nullptr, 16));
    return b;
}
static void hex(const Bytes &b)
{
    for (uint8_t x : b) printf("%02x", x);
    printf("\n");
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "init" && argc == 7) {
        const Bytes sps = unhex(argv[2]), pps = unhex(argv[3]);
        const Bytes ini = fer_mp4_init_segment(sps.data(), sps.size(), pps.data(), pps.size(), atoi(argv[4]), atoi(argv[5]), (uint32_t)strtoul(argv[6], nullptr, 10));
        hex(ini);
        size_t off = 0, len = 0;
        if (fer_mp4_find_avcc(ini.data(), ini.size(), &off, &len))
            printf("avcc %zu %zu\n", off, len);
        else
            printf("none\n");
        return 0;
    }
    if (mode == "front" && argc == 7) {
        const uint32_t n = (uint32_t)atoi(argv[2]), K = (uint32_t)atoi(argv[3]), D = fer_mp4_data_offset(K);
        Bytes out;
        for (uint32_t w = 0; w < D / 4; w++) {
            bool keep;
            put32(out, fer_mp4_front_word(w, n, D, (uint32_t)strtoul(argv[4], nullptr, 10), strtoull(argv[5], nullptr, 10), (uint32_t)strtoul(argv[6], nullptr, 10), &keep));
        }
        hex(out);
        return 0;
    }
    if (mode == "avcc" && argc == 3) {
        bool ok;
        const Bytes s = read_file(argv[2], ok);
        if (!ok) return printf("cannot read %s\n", argv[2]), 1;
        std::unique_ptr<uint8_t[]> h(new uint8_t[s.size() ? s.size() : 1]);
        if (!s.empty()) memcpy(h.get(), s.data(), s.size());
        size_t off = 0, len = 0;
        if (fer_mp4_find_avcc(h.get(), s.size(), &off, &len))
            printf("avcc %zu %zu\n", off, len);
        else
            printf("none\n");
        return 0;
    }
    if (argc > 2) {
        bool ok;
        const Bytes s = read_file(argv[1], ok);
        if (!ok) return printf("cannot read %s\n", argv[1]), 1;
        const int L = atoi(argv[2]);
        if (L != 1 && L != 2 && L != 4) return printf("L must be 1, 2 or 4\n"), 1;
        if (argc > 3) {
            for (size_t k = 0; k <= s.size(); k++) {
                const Result r = run({Bytes(s.begin(), s.begin() + k)}, L);
                printf("%zu %zu %d\n", k, r.spans.size(), r.fault);
            }
            return 0;
        }
        const Result r = run({s}, L);
        for (const Unit &u : r.units) {
            uint32_t a = 1, b = 0;
            for (uint8_t x : u.rbsp) a = (a + x) % 65521u, b = (b + a) % 65521u;
            printf("%d %d %zu %u\n", u.type, u.ref_idc, u.rbsp.size(), b << 16 | a);
        }
        printf("samples %zu\nfault %d\n", r.spans.size(), r.fault);
        return 0;
    }
    constructed();
    drawn();
    printf(fails ? "%d checks failed\n" : "mp4_host_check ok\n", fails);
    return fails != 0;
}
