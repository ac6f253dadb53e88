// The RTP depacketiser of the live decoder's host path (split_rtp, h264-fer_amd/csrc/fer_dec_syntax_host.h) as a stand-alone
// program, for a run under a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/rtp_host_check.cpp -o rtp_host_check && ./rtp_host_check
// Every packet is a heap array of exactly its length and the RBSP store starts empty, so a reader that leaves what it was
// given is an error.  Without arguments it checks constructed packets, every truncation of each of them, and packets of
// drawn bytes.
//   rtp_host_check FILE [EXPECT]
// lists the units that split_rtp keeps of a packet file -- every packet behind its length as a little-endian u32 -- in the
// format of dec_syntax_host_check (type, ref_idc, RBSP bytes, Adler-32), then "fault F" and "seq N" (the expectation it
// leaves; EXPECT = the one it starts with, default -1).
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

static uint32_t rng_state = 20261020u;
static uint32_t rnd(uint32_t m)  // seeded: the same packets in every run
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
    int fault;
    int32_t seq;
};

// split_rtp over copies of the packets that are exactly as long as they are
static Result run(const std::vector<Bytes> &packets, int32_t expect)
{
    std::vector<std::unique_ptr<uint8_t[]>> heap;
    std::vector<RtpPacket> pk;
    for (const Bytes &b : packets) {
        heap.emplace_back(new uint8_t[b.size()]);
        if (!b.empty()) memcpy(heap.back().get(), b.data(), b.size());
        pk.push_back({heap.back().get(), b.size()});
    }
    std::vector<NalRef> nals;
    Bytes store;
    Result r;
    r.seq = expect;
    r.fault = split_rtp(pk.data(), pk.size(), r.seq, nals, store);
    for (const NalRef &n : nals) r.units.push_back({n.type, n.ref_idc, Bytes(n.rbsp.data(), n.rbsp.data() + n.rbsp.size())});
    return r;
}

static Bytes packet(const Bytes &payload, unsigned seq, unsigned cc = 0, int ext = -1, unsigned pad = 0)
{
    Bytes p = {(uint8_t)(0x80 | (pad ? 0x20 : 0) | (ext >= 0 ? 0x10 : 0) | cc), 96, (uint8_t)(seq >> 8), (uint8_t)seq, 1, 2, 3, 4, 5, 6, 7, 8};
    p.insert(p.end(), 4 * cc, 0xC5);
    if (ext >= 0) {
        const uint8_t h[4] = {0xBE, 0xDE, (uint8_t)(ext >> 8), (uint8_t)ext};
        p.insert(p.end(), h, h + 4);
        p.insert(p.end(), 4 * (size_t)ext, 0xE7);
    }
    p.insert(p.end(), payload.begin(), payload.end());
    if (pad) {
        p.insert(p.end(), pad - 1, 0);
        p.push_back((uint8_t)pad);
    }
    return p;
}
static Bytes fu(int s, int e, const Bytes &body)
{
    Bytes p = {0x60 | 28, (uint8_t)(s << 7 | e << 6 | 5)};
    p.insert(p.end(), body.begin(), body.end());
    return p;
}

static void constructed()
{
    const Bytes u1 = {0x41, 9, 8, 7}, sps = {0x67, 1, 2}, pps = {0x68, 3};
    const Bytes stap = {0x38, 0, 3, 0x67, 1, 2, 0, 2, 0x68, 3};
    // a single unit, a STAP-A of two, a unit in three fragments whose 00 00 03 lies across both seams; dressed headers
    const std::vector<Bytes> good = {packet(u1, 65534, 2, 1, 3), packet(stap, 65535, 0, 0), packet(fu(1, 0, {4, 0}), 0, 15), packet(fu(0, 0, {0}), 1, 0, -1, 255),
                                     packet(fu(0, 1, {3, 1}), 2)};
    const std::vector<Unit> want = {{1, 2, {9, 8, 7}}, {7, 3, {1, 2}}, {8, 3, {3}}, {5, 3, {4, 0, 0, 1}}};
    Result r = run(good, 65534);
    EXPECT(r.fault == 0 && r.seq == 3 && r.units == want);
    r = run(good, -1);
    EXPECT(r.fault == 0 && r.seq == 3 && r.units == want);
    r = run(good, 65533);
    EXPECT(r.fault == FER_RTP_GAP && r.seq == -1 && r.units.empty());
    r = run({good[0], good[1], good[2], good[4]}, 65534);
    EXPECT(r.fault == FER_RTP_GAP && r.seq == -1 && r.units.size() == 3);
    r = run({good[0], good[1], good[2], good[3]}, 65534);
    EXPECT(r.fault == FER_RTP_TRUNCATED && r.seq == -1 && r.units.size() == 3);
    r = run({good[0], good[1], good[2], packet(u1, 1)}, 65534);
    EXPECT(r.fault == FER_RTP_MALFORMED && r.units.size() == 3);
    r = run({good[0], packet(fu(0, 0, {1}), 65535)}, 65534);
    EXPECT(r.fault == FER_RTP_MALFORMED && r.units.size() == 1);
    r = run({good[0], packet(fu(1, 1, {1}), 65535)}, 65534);
    EXPECT(r.fault == FER_RTP_MALFORMED && r.units.size() == 1);
    for (int t : {0, 25, 26, 27, 29, 30, 31}) {
        r = run({good[0], packet({(uint8_t)(0x60 | t), 1, 2}, 65535)}, 65534);
        EXPECT(r.fault == FER_RTP_MALFORMED && r.units.size() == 1);
    }
    r = run({packet({0x38, 0, 2, 0x67, 1, 0, 0}, 7)}, -1);
    EXPECT(r.fault == FER_RTP_MALFORMED && r.units.size() == 1);
    r = run({packet({0x38, 0, 2, 0x67, 1, 0, 3, 0x68, 1}, 7)}, -1);
    EXPECT(r.fault == FER_RTP_MALFORMED && r.units.size() == 1);
    r = run({packet({0x38}, 7)}, -1);
    EXPECT(r.fault == FER_RTP_MALFORMED && r.units.empty());
    // a unit without payload ends the list, not the walk
    r = run({packet(u1, 5), packet({0x68}, 6), packet(sps, 7)}, 5);
    EXPECT(r.fault == 0 && r.seq == 8 && r.units.size() == 1);
    r = run({packet(u1, 5), packet({0x68}, 6), packet(sps, 9)}, 5);
    EXPECT(r.fault == FER_RTP_GAP && r.units.size() == 1);
    r = run({}, 77);
    EXPECT(r.fault == 0 && r.seq == 77 && r.units.empty());
    // every truncation of every good packet, in its place in the run: no read leaves the packet, and what is cut faults or
    // (a cut inside the payload of a packet that stays well-formed) still walks
    for (size_t k = 0; k < good.size(); k++)
        for (size_t n = 0; n < good[k].size(); n++) {
            std::vector<Bytes> cut(good.begin(), good.begin() + k + 1);
            cut[k].resize(n);
            r = run(cut, 65534);
            EXPECT(r.fault == 0 || r.fault == FER_RTP_MALFORMED || r.fault == FER_RTP_TRUNCATED);
            EXPECT((r.fault != 0) == (r.seq == -1));
            if (n < 12) EXPECT(r.fault == FER_RTP_MALFORMED);
        }
}

static void drawn()
{
    for (int k = 0; k < 20000; k++) {
        std::vector<Bytes> pk(1 + rnd(4));
        for (Bytes &p : pk) {
            p.resize(rnd(48));
            for (uint8_t &b : p) b = (uint8_t)rnd(256);
            if (!p.empty() && rnd(4)) p[0] = (uint8_t)(0x80 | (p[0] & 0x3f));
            if (p.size() > 12 && rnd(2)) p[12 + 4 * (p[0] & 15) < p.size() ? 12 + 4 * (p[0] & 15) : 12] = (uint8_t)(rnd(2) ? 24 : 28);
        }
        size_t total = 0;
        for (const Bytes &p : pk) total += p.size();
        const Result r = run(pk, rnd(2) ? -1 : (int32_t)rnd(65536));
        size_t bytes = 0;
        for (const Unit &u : r.units) bytes += u.rbsp.size();
        EXPECT(bytes <= total && r.fault >= 0 && r.fault <= 4 && r.fault != 1);
    }
}

static int list_file(const char *path, int32_t expect)
{
    FILE *f = fopen(path, "rb");
    if (!f) return printf("cannot read %s\n", path), 1;
    Bytes s;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + k);
    fclose(f);
    std::vector<Bytes> pk;
    for (size_t pos = 0; pos < s.size();) {
        if (s.size() - pos < 4) return printf("packet file: a length is cut\n"), 1;
        const size_t n = (size_t)s[pos] | (size_t)s[pos + 1] << 8 | (size_t)s[pos + 2] << 16 | (size_t)s[pos + 3] << 24;
        pos += 4;
        if (n > s.size() - pos) return printf("packet file: a packet is cut\n"), 1;
        pk.emplace_back(s.begin() + pos, s.begin() + pos + n);
        pos += n;
    }
    const Result r = run(pk, expect);
    for (const Unit &u : r.units) {
        uint32_t a = 1, b = 0;
        for (uint8_t x : u.rbsp) a = (a + x) % 65521u, b = (b + a) % 65521u;
        printf("%d %d %zu %u\n", u.type, u.ref_idc, u.rbsp.size(), b << 16 | a);
    }
    printf("fault %d\nseq %d\n", r.fault, (int)r.seq);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1) return list_file(argv[1], argc > 2 ? atoi(argv[2]) : -1);
    constructed();
    drawn();
    printf(fails ? "%d checks failed\n" : "rtp_host_check ok\n", fails);
    return fails != 0;
}
