// fer_nalsplit.h -- the NAL splitters on the device (fer_nalsplit.hip: Annex-B and length-prefixed ranges) as the live
// decoder drives them (fer_decode_host.hip): byte ranges in device memory -> a table of NAL units and their RBSP in one
// device store.
#pragma once
#include "fer_ctx.h"

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

// The buffers of a splitter.  Everything grows to the largest job seen and stays; one job at a time.
struct FerSplit {
    FerSplitRange *d_rng = nullptr, *h_rng = nullptr;  // device / pinned [rng_cap]
    uint2 *d_rtot = nullptr;                           // [rng_cap] units and bytes of every range
    FerSplitBase *d_rbase = nullptr;                   // [rng_cap]
    size_t rng_cap = 0;
    uint4 *d_summ = nullptr, *d_cin = nullptr;         // [ch_cap] one summary per 4096-byte chunk, and what precedes it
    size_t ch_cap = 0;
    uint8_t *d_res = nullptr, *h_res = nullptr;        // device / pinned: FerSplitHead, table [tab_cap], prefixes [tab_cap][PREFIX]
    size_t tab_cap = 0;
    uint8_t *d_store = nullptr;                        // the units' RBSP
    size_t store_cap = 0;
    int32_t *d_fault = nullptr, *h_fault = nullptr;    // device / pinned [fault_cap]: a length-prefixed range overran
    size_t fault_cap = 0;
    FerAvccUnit *d_aunit = nullptr;                    // [aunit_cap >= tab_cap] the units of length-prefixed ranges
    size_t aunit_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;           // around the launches of a job
    double ms = 0;                                     // ... their time, summed over the jobs
    unsigned long long in_bytes = 0;                   // input bytes of those jobs
    // the last job's result (pinned memory, valid until the next job)
    const FerSplitHead *head() const { return (const FerSplitHead *)h_res; }
    const ferhip_nal_unit *table() const { return (const ferhip_nal_unit *)(h_res + sizeof(FerSplitHead)); }
    const uint8_t *prefix(size_t k) const { return h_res + sizeof(FerSplitHead) + tab_cap * sizeof(ferhip_nal_unit) + k * FER_SPLIT_PREFIX; }
};

// Splits n ranges (device pointers, NULL / 0 = an empty range) on stream st and waits: afterwards table() holds head()->units
// entries and prefix(k) the first FER_SPLIT_PREFIX bytes of unit k.  dst == NULL: the RBSP goes to sp.d_store, which is grown
// as needed; else to dst[0, cap) as far as whole units fit (head()->bytes tells what all of them need) and no prefixes are
// read back.  One host synchronisation unless the table or the store had to grow.
// length_size = 0: Annex-B ranges.  1, 2, 4: every unit is preceded by its length of that many bytes; h_fault[r] is then 1
// for a range that overran, and the table holds the units in front of the range's first empty, header-only or overrunning one.
int fer_split_run(FerSplit &sp, hipStream_t st, const uint8_t *const *ptrs, const size_t *lens, int n, uint8_t *dst, size_t cap,
                  int length_size = 0);
void fer_split_free(FerSplit &sp);

#pragma GCC visibility pop
