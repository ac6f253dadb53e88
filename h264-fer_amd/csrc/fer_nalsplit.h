// fer_nalsplit.h -- the NAL splitters on the device (fer_nalsplit.hip: Annex-B and length-prefixed ranges) as the live
// decoder drives them (fer_decode_live.hip): byte ranges in device memory -> a table of NAL units and their RBSP in one
// device store.
#pragma once
#include "fer_ctx.h"
#include <new>

#pragma GCC visibility push(hidden)

#define FER_SPLIT_PREFIX FERHIP_SPLIT_PREFIX  // bytes of every unit's RBSP that come back with the table

struct FerSplitRange {  // one input range: `len` bytes at `p` (any alignment); choff = its first entry in the chunk arrays
    const uint8_t *p;
    uint32_t len, choff;
};
struct FerSplitBase {  // what stands in front of a range: RBSP bytes (every unit rounded up to 16) and units
    unsigned long long bytes;
    uint32_t units, pad;
};
struct FerAvccUnit {  // one unit of a length-prefixed range: range | header byte << 16; the unit is s[st..en); its first chunk slot
    uint32_t range, st, en, choff;
};
struct FerSplitHead {  // the totals of a job, in front of the table
    unsigned long long bytes;
    uint32_t units, pad;
};

// The buffers of a splitter, each with its own capacity (DevBuf, fer_ctx.h).  Everything grows to the largest job seen and
// stays; one job at a time.  The buffers go with the splitter (their own destructors), the two events by its destructor: the
// splitter's device must be current where it is destroyed.
struct FerSplit {
    ~FerSplit()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    DevBuf<FerSplitRange> d_rng;       // [n] the ranges of a job ...
    PinBuf<FerSplitRange> h_rng;       // ... as the host writes them
    DevBuf<uint2> d_rtot;              // [n] units and bytes of every range
    DevBuf<FerSplitBase> d_rbase;      // [n]
    DevBuf<uint4> d_summ, d_cin;       // one summary per 4096-byte chunk, and what precedes it
    DevBuf<uint8_t> d_res;             // FerSplitHead, table [tab_cap], prefixes [tab_cap][PREFIX] ...
    PinBuf<uint8_t> h_res;             // ... and the copy the host reads
    size_t tab_cap = 0;                // units the two hold
    DevBuf<uint8_t> d_store;           // the units' RBSP
    DevBuf<int32_t> d_fault;           // [n]: a length-prefixed range overran
    PinBuf<int32_t> h_fault;
    DevBuf<FerAvccUnit> d_aunit;       // [>= tab_cap] the units of length-prefixed ranges
    hipEvent_t ev0 = nullptr, ev1 = nullptr;           // around the launches of a job's first pass
    double ms = 0;                                     // ... their time, summed over the jobs
    unsigned long long in_bytes = 0;                   // input bytes of those jobs
    // the last job's result (pinned memory, valid until the next job)
    const FerSplitHead *head() const { return (const FerSplitHead *)h_res.p; }
    const ferhip_nal_unit *table() const { return (const ferhip_nal_unit *)(h_res.p + sizeof(FerSplitHead)); }
    const uint8_t *prefix(size_t k) const { return h_res.p + sizeof(FerSplitHead) + tab_cap * sizeof(ferhip_nal_unit) + k * FER_SPLIT_PREFIX; }
};

// Splits n ranges (device pointers, NULL / 0 = an empty range) on stream st and waits: afterwards table() holds head()->units
// entries and prefix(k) the first FER_SPLIT_PREFIX bytes of unit k.  dst == NULL: the RBSP goes to sp.d_store, which is grown
// as needed; else to dst[0, cap) as far as whole units fit (head()->bytes tells what all of them need) and no prefixes are
// read back.  One host synchronisation unless the table or the store had to grow.
// length_size = 0: Annex-B ranges.  1, 2, 4: every unit is preceded by its length of that many bytes; h_fault[r] is then 1
// for a range that overran, and the table holds the units in front of the range's first empty, header-only or overrunning one.
int fer_split_run(FerSplit &sp, hipStream_t st, const uint8_t *const *ptrs, const size_t *lens, int n, uint8_t *dst, size_t cap,
                  int length_size = 0);
// Destroys the splitter now, while the caller has its device current, and leaves an empty one that can be used again.
inline void fer_split_free(FerSplit &sp)
{
    sp.~FerSplit();
    new (&sp) FerSplit();
}

// RTP packets in device memory (fer_rtp.hip): the buffers of the depacketiser in front of the splitter, each a DevBuf that
// grows to the largest job seen and stays; one job at a time.
struct FerUnrtp {
    DevBuf<ferhip_rtp_pkt> d_pkts;   // [npk] the table, sorted by stream ...
    PinBuf<ferhip_rtp_pkt> h_pkts;   // ... as the host writes it
    DevBuf<uint4> d_rec;             // [npk] what k_unrtp_parse reads of every packet's header
    DevBuf<uint4> d_piece;           // [npk] what k_unrtp_gather copies for every packet: source, bytes, place in the staging range
    DevBuf<uint32_t> d_job;          // [4][S]: first packet (S + 1), staging base, expectation in
    PinBuf<uint32_t> h_job;
    DevBuf<int32_t> d_res;           // [3][S]: staged bytes, fault, expectation out
    PinBuf<int32_t> h_res;
    DevBuf<uint8_t> d_stage;         // every stream's units behind 4-byte lengths: the ranges fer_split_run takes
    std::vector<const uint8_t *> ptrs;  // [S] the last job's staging ranges
    std::vector<size_t> lens;
};
// pkts[npk] (host) sorted by stream, first[S + 1] = every stream's first row; the packets lie at d_base + offset.  Parses,
// walks (expect[S]: in the expectation or -1, out the next one or -1 after a fault; fault[S]: 0, 2, 3, 4) and gathers every
// stream's units behind 4-byte lengths into u.ptrs / u.lens, on stream st.  One host synchronisation.
int fer_unrtp_run(FerUnrtp &u, hipStream_t st, const uint8_t *d_base, const ferhip_rtp_pkt *pkts, size_t npk, const uint32_t *first, int S,
                  int32_t *expect, int32_t *fault);
// a stable sort of the caller's table by stream, and every stream's first row; FERHIP_E_ARG for a stream outside [0, S)
int fer_rtp_sort(const ferhip_rtp_pkt *pkts, size_t npk, int S, std::vector<ferhip_rtp_pkt> &sorted, std::vector<uint32_t> &first);

// Transport stream packets in device memory (fer_ts.hip): the buffers of the demultiplexer in front of the splitter, as
// FerUnrtp's; one job at a time.
struct FerUnts {
    DevBuf<ferhip_ts_run> d_runs;    // [nruns] the table, sorted by stream ...
    PinBuf<ferhip_ts_run> h_runs;    // ... as the host writes it
    DevBuf<uint4> d_rec;             // [npk] what k_unts_parse reads of every 188-byte packet
    DevBuf<uint4> d_piece;           // [npk] what k_unts_gather copies for every packet: source, bytes | stream << 8, place
    DevBuf<uint32_t> d_job;          // first packet of every stream (S + 1), PID [S], expectation in [S], first packet of every
    PinBuf<uint32_t> h_job;          // run (nruns + 1), staging bases (64-bit) [S]
    DevBuf<int32_t> d_res;           // [3][S]: staged bytes, fault, expectation out
    PinBuf<int32_t> h_res;
    DevBuf<uint8_t> d_stage;         // every stream's elementary-stream bytes: the Annex-B ranges fer_split_run takes
    std::vector<const uint8_t *> ptrs;  // [S] the last job's staging ranges
    std::vector<size_t> lens;
};
// runs[nruns] (host) sorted by stream, first[S + 1] = every stream's first row; the runs' packets lie at d_base + offset and
// stream s listens to pids[s].  Parses, walks (expect[S]: in the continuity counter expected or -1, out the next one or -1
// after a fault; fault[S]: 0, 2, 3) and gathers the elementary-stream bytes that stand into u.ptrs / u.lens, on stream st.
// One host synchronisation.
int fer_unts_run(FerUnts &u, hipStream_t st, const uint8_t *d_base, const ferhip_ts_run *runs, size_t nruns, const uint32_t *first, int S,
                 const uint16_t *pids, int32_t *expect, int32_t *fault);

// The empty-payload cut of split_stream (fer_dec_syntax_host.h), which the device leaves to the host: a unit with bytes == 0
// ends its range, and the later units of that range are skipped.  f(k, unit) for every entry k of the last job's table that
// stays, in table order, until one returns non-zero; returns that value, or 0.
template <typename F>
static int fer_split_each_unit(const FerSplit &sp, F f)
{
    const ferhip_nal_unit *t = sp.table();
    const size_t nt = sp.head()->units;
    uint32_t cut = ~0u;  // the table is in range order: one range is cut at a time
    for (size_t k = 0; k < nt; k++) {
        if (t[k].range == cut) continue;
        if (t[k].bytes == 0) {
            cut = t[k].range;
            continue;
        }
        if (int rc = f(k, t[k])) return rc;
    }
    return 0;
}

#pragma GCC visibility pop
