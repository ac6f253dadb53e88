// The transport stream demultiplexer of the live decoder's host path (split_ts, h264-fer_amd/csrc/fer_dec_syntax_host.h) as a
// stand-alone program, for a run under a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/ts_host_check.cpp -o ts_host_check && ./ts_host_check
// Every run is a heap array of exactly its length and the RBSP store starts empty, so a reader that leaves what it was given
// is an error.  Without arguments it checks constructed packets, single damaged bytes in each of them, and packets of drawn
// bytes.
//   ts_host_check FILE PID [EXPECT]
// lists the units that split_ts keeps of a file of 188-byte packets (one run) for the stream that listens to PID, in the
// format of dec_syntax_host_check (type, ref_idc, RBSP bytes, Adler-32), then "fault F" and "cc N" (the expectation it
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
    int32_t cc;
};

// split_ts over copies of the runs that are exactly as long as they are
static Result run(const std::vector<Bytes> &runs, unsigned pid, int32_t expect)
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
    r.cc = expect;
    r.fault = split_ts(rn.data(), rn.size(), pid, r.cc, nals, store);
    for (const NalRef &n : nals) r.units.push_back({n.type, n.ref_idc, Bytes(n.rbsp.data(), n.rbsp.data() + n.rbsp.size())});
    return r;
}

// one packet: the payload right-aligned behind an adaptation field of stuffing
static Bytes packet(unsigned pid, unsigned cc, const Bytes &payload, bool pusi)
{
    Bytes p = {0x47, (uint8_t)((pusi ? 0x40 : 0) | pid >> 8), (uint8_t)pid, (uint8_t)((payload.size() < 184 ? 0x30 : 0x10) | (cc & 15))};
    if (payload.size() < 184) {
        const size_t a = 183 - payload.size();
        p.push_back((uint8_t)a);
        if (a) p.push_back(0);
        if (a) p.insert(p.end(), a - 1, 0xFF);
    }
    p.insert(p.end(), payload.begin(), payload.end());
    return p;
}
static Bytes pes(const Bytes &es)
{
    Bytes p = {0, 0, 1, 0xE0, 0, 0, 0x84, 0x80, 5, 0x21, 0, 1, 0, 1};
    p.insert(p.end(), es.begin(), es.end());
    return p;
}
static Bytes join(const std::vector<Bytes> &v)
{
    Bytes o;
    for (const Bytes &b : v) o.insert(o.end(), b.begin(), b.end());
    return o;
}

static void constructed()
{
    const unsigned pid = 0x100;
    // a delimiter and a slice whose 00 00 03 lies across the packet seam; then a second access unit in one packet
    Bytes es1 = {0, 0, 0, 1, 9, 0x30, 0, 0, 0, 1, 0x65};
    es1.insert(es1.end(), 158, 0xAB);
    es1.push_back(0);  // the last byte of the first packet (14 + 11 + 158 + 1 = 184)
    const Bytes tail = {0, 3, 1, 0x77};
    const Bytes first = pes(es1);
    EXPECT(first.size() == 184);
    const Bytes es2 = {0, 0, 0, 1, 9, 0x30, 0, 0, 0, 1, 0x41, 5, 6};
    const std::vector<Bytes> good = {packet(pid, 15, first, true), packet(0x33, 3, Bytes(184, 0x11), false), packet(pid, 0, tail, false),
                                     packet(0x1FFF, 0, Bytes(184, 0xFF), false), packet(pid, 1, pes(es2), true)};
    Bytes rbsp1(158, 0xAB);
    rbsp1.insert(rbsp1.end(), {0, 0, 1, 0x77});
    const std::vector<Unit> want = {{9, 0, {0x30}}, {5, 3, rbsp1}, {9, 0, {0x30}}, {1, 2, {5, 6}}};
    Result r = run({join(good)}, pid, 15);
    EXPECT(r.fault == 0 && r.cc == 2 && r.units == want);
    r = run(good, pid, -1);  // a run per packet
    EXPECT(r.fault == 0 && r.cc == 2 && r.units == want);
    r = run({join(good)}, 0x33, -1);  // the other PID: a continuation with none open
    EXPECT(r.fault == FER_TS_MALFORMED && r.cc == -1 && r.units.empty());
    r = run({join(good)}, 0x44, 7);  // nobody's PID: nothing, the expectation stays
    EXPECT(r.fault == 0 && r.cc == 7 && r.units.empty());
    r = run({join(good)}, pid, 14);
    EXPECT(r.fault == FER_TS_GAP && r.cc == -1 && r.units.empty());
    r = run({join({good[0], good[4]})}, pid, 15);  // the continuation is lost: the first access unit is dropped
    EXPECT(r.fault == FER_TS_GAP && r.units.empty());
    r = run({join({good[0], good[2], good[4], good[4]})}, pid, 15);  // a duplicate: the open one is dropped
    EXPECT(r.fault == FER_TS_GAP && r.units.size() == 2);
    r = run({}, pid, 9);
    EXPECT(r.fault == 0 && r.cc == 9 && r.units.empty());
    // every byte of the header region of every packet damaged in turn: no read leaves the run, and the outcome is a
    // fault or a clean walk
    const Bytes all = join(good);
    for (size_t k = 0; k < all.size(); k += 188)
        for (size_t b = 0; b < 24; b++)
            for (int v : {0x00, 0xFF, 0x47 ^ 0x80, 184}) {
                Bytes cut = all;
                cut[k + b] = (uint8_t)v;
                r = run({cut}, pid, 15);
                EXPECT(r.fault == 0 || r.fault == FER_TS_MALFORMED || r.fault == FER_TS_GAP);
                EXPECT((r.fault != 0) == (r.cc == -1));
            }
}

static void drawn()
{
    for (int k = 0; k < 20000; k++) {
        std::vector<Bytes> runs(1 + rnd(3));
        size_t total = 0;
        for (Bytes &p : runs) {
            p.resize(188 * rnd(4));
            for (uint8_t &b : p) b = (uint8_t)rnd(256);
            for (size_t o = 0; o < p.size(); o += 188) {
                if (rnd(8)) p[o] = 0x47;
                if (rnd(8)) p[o + 1] = (uint8_t)(p[o + 1] & 0x40), p[o + 2] = (uint8_t)rnd(2);
                if (rnd(4)) p[o + 3] = (uint8_t)(p[o + 3] & 0x3F);
                if (rnd(2)) p[o + 4] = (uint8_t)rnd(190);
                const size_t at = ((p[o + 3] >> 4) & 3) == 3 ? 5 + (size_t)p[o + 4] : 4;
                if (at + 9 <= 188 && rnd(2)) p[o + at] = 0, p[o + at + 1] = 0, p[o + at + 2] = 1, p[o + at + 3] = 0xE0, p[o + at + 6] = 0x80, p[o + at + 8] = (uint8_t)rnd(200);
            }
            total += p.size();
        }
        const Result r = run(runs, rnd(2), rnd(2) ? -1 : (int32_t)rnd(16));
        size_t bytes = 0;
        for (const Unit &u : r.units) bytes += u.rbsp.size();
        EXPECT(bytes <= total && (r.fault == 0 || r.fault == FER_TS_MALFORMED || r.fault == FER_TS_GAP) && r.cc >= -1 && r.cc <= 15);
    }
}

static int list_file(const char *path, unsigned pid, int32_t expect)
{
    FILE *f = fopen(path, "rb");
    if (!f) return printf("cannot read %s\n", path), 1;
    Bytes s;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + k);
    fclose(f);
    if (s.size() % 188) return printf("packet file: no whole number of packets\n"), 1;
    const Result r = run({s}, pid, expect);
    for (const Unit &u : r.units) {
        uint32_t a = 1, b = 0;
        for (uint8_t x : u.rbsp) a = (a + x) % 65521u, b = (b + a) % 65521u;
        printf("%d %d %zu %u\n", u.type, u.ref_idc, u.rbsp.size(), b << 16 | a);
    }
    printf("fault %d\ncc %d\n", r.fault, (int)r.cc);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 2) return list_file(argv[1], (unsigned)atoi(argv[2]), argc > 3 ? atoi(argv[3]) : -1);
    constructed();
    drawn();
    printf(fails ? "%d checks failed\n" : "ts_host_check ok\n", fails);
    return fails != 0;
}
