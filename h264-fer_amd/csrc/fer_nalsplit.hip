// fer_nalsplit.hip -- the Annex-B splitter on the device (ferhip_split_nal_blocks, ferhip_decs_decode_dev): what
// split_stream (fer_decode_host.hip) computes for many byte ranges at once, from and into device memory.
//
// For a range s[0..n) split_stream's result is a set of local predicates:
//   code(z) : s[z..z+3] = 00 00 00 01 (z + 3 < n)        a unit begins at st = z + 4
//   T(i)    : s[i] = s[i+1] = 0, s[i+2] in {0, 1} (i + 2 < n)   the first T at or behind st ends the unit (else n does)
//   H(p)    : code(p - 4) and not T(p) and p < n          p is the header byte of a unit that is not empty
//   D(p)    : s[p] = 3, s[p-1] = s[p-2] = 0, not code(p - 6)    a dropped 03; code(p - 6) is the one case in which the first
//             of the two zeros is the header byte (p - 2 = st)
// Every code is also a T (at z and at z + 1), so a byte belongs to a unit exactly when the last H in front of it is later
// than the last T at or in front of it, and what a run of bytes does to that state is a function that composes: a scan.
// A run's function is (units begun, has a T or an H, payload bytes in front of its first T or H -- they belong to the
// unit that comes in --, is a unit open at its end, that unit's payload bytes so far, the 16-rounded bytes of the units
// begun and ended inside); see SplitCompose.  The scans themselves -- over a wavefront, over the four wavefronts of a
// workgroup, over the chunks of a range -- are fer_scan.h's, shared with fer_nalpack.hip.
//
//   k_split_count  grid (chunk, range): a lane takes 16 bytes of the range's 16-byte-aligned image (a range may start
//                  anywhere: the bytes in front of it and behind it read as ff, which takes part in no pattern) with 8
//                  bytes in front and 4 behind, reduces them to their function; the 256 lanes compose theirs in order
//                  (wavefront scan by shuffles, the four wavefronts through LDS); one function per 4096-byte chunk.
//   k_split_plan   one wavefront per range composes the chunk functions in order: what comes into every chunk, and the
//                  range's units and bytes.
//   k_split_index  one wavefront: exclusive sums of the two counts of every range over the ranges (units and bytes; for
//                  length-prefixed ranges units and chunk slots), and the totals in front of the table.
//   k_split_emit   grid (chunk, range): every lane recomputes its function, the same scan gives it its unit, that unit's
//                  offset and the bytes so far; a lane writes the table entry of a unit whose header byte it holds
//                  (range, type, ref_idc, offset) and the size of a unit that ends in its bytes, and places the payload
//                  bytes in output order in LDS.  Units start at multiples of 16, so a 16-byte word of the output belongs
//                  to one unit: words the chunk fills are stored whole, the others (a unit's last word, the word a unit
//                  shares with the neighbouring chunk) byte-wise.  Nothing at or behind `cap` and nothing of a table
//                  entry at or behind `tab_cap` is written: the host compares the totals and repeats the launch.
//   k_split_prefix one wavefront per unit: the first FER_SPLIT_PREFIX bytes of its RBSP to a dense array behind the table.
// No workgroup waits for another one: the phases are separate launches on one stream.  All loads are naturally aligned
// and made only of pieces that hold a byte of the range, so nothing outside the pages of [p, p + len) is touched.
//
// Length-prefixed (AVCC) ranges, ferhip_split_avcc_blocks and ferhip_decs_decode_dev in AVCC input: the same table, store
// and prefixes from ranges in which every unit is preceded by its length of L = 1, 2 or 4 bytes (the definition: ferhip.h).
// Boundaries come from the lengths alone, so the units are found by following the chain, and what is left per unit is the
// local predicate D(p): s[p] = 3, s[p-1] = s[p-2] = 0, p - 2 >= st + 1.  A unit's payload s[st+1..en) is taken in 4096-byte
// chunks of its own 16-byte-aligned image; the walk ends a range at its first empty, header-only or overrunning unit, so
// the table the device writes is already the one behind the cut.
//   k_avcc_walk   one lane per range follows the length chain with byte loads, twice: first it counts the range's units and
//                 their chunks and finds its fault, then (behind k_split_index, which turns the counts into every range's
//                 first unit and first chunk slot) it writes one record per unit (range, header byte, st, en, first chunk
//                 slot).
//   k_avcc_count  grid (chunk, unit): the dropped 03 bytes of every chunk.
//   k_avcc_plan   one wavefront per unit: exclusive sum of its chunk counts = the 03 bytes in front of every chunk, and the
//                 unit's RBSP size.
//   k_avcc_index  one wavefront: exclusive sum of the 16-rounded RBSP sizes over the units = their offsets; the table
//                 entries and the totals in front of the table.
//   k_avcc_emit   grid (chunk, unit): the chunk's surviving bytes are compacted in LDS in output order and the span is
//                 stored with 16-byte stores, its ragged ends byte-wise (store_span, as in k_nal_emit); nothing at or behind
//                 `cap`.
//   k_split_prefix as above.
// The host side follows the kernels: fer_split_run sizes the buffers of a FerSplit (each a DevBuf with its own capacity), runs
// the launches and repeats them while the totals say that the table or the store was too small; the two known-answer entry
// points are one function.
#include "fer_nalsplit.h"
#include "fer_scan.h"
#include <string.h>
#include <algorithm>

#define SPL_THREADS 256
#define SPL_CHUNK (SPL_THREADS * 16)
// LDS image of a chunk's output: its payload bytes, up to 15 bytes in front (the first word's misalignment) and up to 15
// bytes of rounding for every unit that begins in it (a unit costs five input bytes: 820 units at the most)
#define SPL_IMG (((15 + SPL_CHUNK + 15 * ((SPL_CHUNK + 4) / 5) + 15) & ~15) + 16)
#define AVCC_IMG ((15 + SPL_CHUNK + 15) & ~15)  // a chunk's surviving bytes behind up to 15 bytes of misalignment
#define SPL_MAX_LEN (1u << 30)  // bytes per range: positions, counts and 16-rounded sums stay within 32 bits

struct FerSplitJob {
    const FerSplitRange *rng;
    int n;
    uint4 *summ, *cin;
    uint2 *rtot;
    FerSplitBase *rbase;
    FerSplitHead *head;
    ferhip_nal_unit *tab;
    uint32_t tab_cap;
    uint8_t *dst;
    unsigned long long cap;
    uint8_t *pref;
    // length-prefixed ranges
    int lsize;            // bytes of a length: 1, 2 or 4
    FerAvccUnit *aunit;   // [tab_cap]
    int32_t *fault;       // [n] the range overran
    // ... keep 32-bit counts in the arrays of the chunk functions, four slots to an element: [chunk slots] the dropped 03
    // bytes of a chunk / in front of it within its unit
    __host__ __device__ uint32_t *acnt() const { return (uint32_t *)summ; }
    __host__ __device__ uint32_t *acin() const { return (uint32_t *)cin; }
};

// A run's function as a uint4: x = units begun | has an event << 30 | open at the end << 31, y = head bytes, z = bytes of
// the open unit, w = 16-rounded bytes of the units begun and ended inside.
#define SPL_EV (1u << 30)
#define SPL_OPEN (1u << 31)
#define SPL_CNT (SPL_EV - 1u)
__device__ __forceinline__ uint4 split_identity() { return make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ uint32_t split_r16(uint32_t v) { return (v + 15u) & ~15u; }

// f first, then g (adjacent runs of one range)
struct SplitCompose {
    __device__ __forceinline__ uint4 operator()(const uint4 &f, const uint4 &g) const
    {
        uint4 r;
        const bool fopen = (f.x & SPL_OPEN) != 0;
        r.x = ((f.x & SPL_CNT) + (g.x & SPL_CNT)) | ((f.x | g.x) & SPL_EV);
        r.y = (f.x & SPL_EV) ? f.y : f.y + g.y;
        if (g.x & SPL_EV) {  // g's first event ends what f left open; g's own end state stands
            r.x |= g.x & SPL_OPEN;
            r.z = g.z;
            r.w = f.w + g.w + (fopen ? split_r16(f.z + g.y) : 0u);
        } else {  // g changes nothing: its bytes go to the unit f left open, if any
            r.x |= f.x & SPL_OPEN;
            r.z = fopen ? f.z + g.y : 0u;
            r.w = f.w;
        }
        return r;
    }
};

// the bytes of dword x stand at image positions vd .. vd + 3: those outside [a, end) become ff
__device__ __forceinline__ uint32_t split_mask(uint32_t x, int vd, int a, int end)
{
    const int lo = max(a - vd, 0), hi = min(end - vd, 4);
    if (hi <= lo) return 0xffffffffu;
    const uint32_t keep = (hi >= 4 ? 0xffffffffu : (1u << (8 * hi)) - 1u) & ~((1u << (8 * lo)) - 1u);
    return (x & keep) | ~keep;
}

// A lane's 16 bytes: the word itself and one bit per byte for T, H, D and "inside the range".
struct SplitLane {
    uint32_t b[4];
    uint32_t T, H, D, V;
};

// The range's image starts `a` = p & 15 bytes in front of p, so that image position v is byte v - a of the range and
// words of the image are 16-byte aligned in memory.  Lane tid of chunk `chunk` takes image bytes [v0, v0 + 16).
__device__ __forceinline__ void split_lane(const FerSplitRange &r, uint32_t a, uint32_t chunk, int tid, SplitLane &L)
{
    const uint8_t *base = r.p - a;
    const int end = (int)(a + r.len), ia = (int)a;
    const int v0 = (int)(chunk * SPL_CHUNK) + tid * 16;
    uint32_t w[7] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u};  // the dwords at v0 - 8 .. v0 + 16
    if (v0 > ia && v0 - 8 < end) {
        const uint2 t = *(const uint2 *)(base + v0 - 8);
        w[0] = t.x;
        w[1] = t.y;
    }
    if (v0 + 16 > ia && v0 < end) {
        const uint4 t = *(const uint4 *)(base + v0);
        w[2] = t.x;
        w[3] = t.y;
        w[4] = t.z;
        w[5] = t.w;
    }
    if (v0 + 20 > ia && v0 + 16 < end) w[6] = *(const uint32_t *)(base + v0 + 16);
    uint32_t Z = 0u, O = 0u, Th = 0u;  // bit k: byte k of w is 00 / 01 / 03
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const uint32_t x = split_mask(w[k], v0 - 8 + 4 * k, ia, end);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t c = (x >> (8 * q)) & 0xffu;
            Z |= (uint32_t)(c == 0u) << (4 * k + q);
            O |= (uint32_t)(c == 1u) << (4 * k + q);
            Th |= (uint32_t)(c == 3u) << (4 * k + q);
        }
    }
    const uint32_t code = Z & (Z >> 1) & (Z >> 2) & (O >> 3);  // bit k: a start code begins at byte k of w
    const uint32_t term = Z & (Z >> 1) & ((Z | O) >> 2);
    // the lane's byte j is byte j + 8 of w
    const int lo = max(ia - v0, 0), hi = min(end - v0, 16);
    L.V = hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
    L.T = (term >> 8) & L.V;
    L.H = (code >> 4) & ~L.T & L.V;
    L.D = (Th >> 8) & (Z >> 7) & (Z >> 6) & ~(code >> 2) & L.V;
    L.b[0] = w[2];
    L.b[1] = w[3];
    L.b[2] = w[4];
    L.b[3] = w[5];
}

__device__ __forceinline__ uint4 split_piece(const SplitLane &L)
{
    uint32_t nu = 0u, ev = 0u, open = 0u, head = 0u, tail = 0u, closed = 0u;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t m = 1u << j;
        if (!(L.V & m)) continue;
        if (L.T & m) {
            if (open) closed += split_r16(tail);
            open = 0u;
            tail = 0u;
            ev = 1u;
        } else if (L.H & m) {
            nu++;
            open = 1u;
            tail = 0u;
            ev = 1u;
        } else if (!(L.D & m)) {
            head += ev ^ 1u;
            tail += open;
        }
    }
    return make_uint4(nu | (ev ? SPL_EV : 0u) | (open ? SPL_OPEN : 0u), head, tail, closed);
}

__device__ __forceinline__ uint32_t split_nch(const FerSplitRange &r, uint32_t a) { return r.len ? (a + r.len + SPL_CHUNK - 1) / SPL_CHUNK : 0u; }

__global__ __launch_bounds__(SPL_THREADS) void k_split_count(FerSplitJob j)
{
    const FerSplitRange r = j.rng[blockIdx.y];
    const uint32_t a = (uint32_t)((uintptr_t)r.p & 15u);
    const uint32_t nch = split_nch(r, a);  // 0 for an empty range: its workgroups leave here
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint4 wtot[SPL_THREADS / 64];
    for (uint32_t chunk = blockIdx.x; chunk < nch; chunk += gridDim.x) {
        SplitLane L;
        split_lane(r, a, chunk, tid, L);
        wg_put(wtot, wave_scan(split_piece(L), lane, SplitCompose()), wave, lane);
        __syncthreads();
        if (tid == 0) j.summ[r.choff + chunk] = wg_total(wtot, SplitCompose());
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_split_plan(FerSplitJob j)
{
    const FerSplitRange r = j.rng[blockIdx.x];
    const int lane = threadIdx.x;
    const uint32_t nch = split_nch(r, (uint32_t)((uintptr_t)r.p & 15u));
    const uint4 run = carry_scan(
        nch, lane, split_identity(), SplitCompose(), [&](uint32_t i) { return j.summ[r.choff + i]; },
        [&](uint32_t i, const uint4 &in) { j.cin[r.choff + i] = in; });
    if (lane == 0) j.rtot[blockIdx.x] = make_uint2(run.x & SPL_CNT, run.w + ((run.x & SPL_OPEN) ? split_r16(run.z) : 0u));
}

__global__ __launch_bounds__(64) void k_split_index(FerSplitJob j)
{
    const int lane = threadIdx.x;
    unsigned long long bytes = 0;
    uint32_t units = 0;
    for (int s0 = 0; s0 < j.n; s0 += 64) {
        const int s = s0 + lane;
        const uint2 e = s < j.n ? j.rtot[s] : make_uint2(0u, 0u);
        const unsigned long long ib = wave_scan((unsigned long long)e.y, lane, ScanAdd());
        const uint32_t iu = wave_scan(e.x, lane, ScanAdd());
        if (s < j.n) {
            FerSplitBase b;
            b.bytes = bytes + ib - e.y;
            b.units = units + iu - e.x;
            b.pad = 0;
            j.rbase[s] = b;
        }
        bytes += __shfl(ib, 63);
        units += __shfl(iu, 63);
    }
    if (lane == 0) {
        FerSplitHead h;
        h.bytes = bytes;
        h.units = units;
        h.pad = 0;
        *j.head = h;
    }
}

__global__ __launch_bounds__(SPL_THREADS) void k_split_emit(FerSplitJob j)
{
    const int s = blockIdx.y;
    const FerSplitRange r = j.rng[s];
    const uint32_t a = (uint32_t)((uintptr_t)r.p & 15u);
    const uint32_t nch = split_nch(r, a);
    if (!nch) return;
    const FerSplitBase rb = j.rbase[s];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint4 wtot[SPL_THREADS / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[SPL_IMG];
    __shared__ uint32_t msk[SPL_IMG / 16];  // bit b of word w: the chunk wrote byte b of the image's 16-byte word w
    for (uint32_t chunk = blockIdx.x; chunk < nch; chunk += gridDim.x) {
        for (int w = tid; w < SPL_IMG / 16; w += SPL_THREADS) msk[w] = 0u;
        SplitLane L;
        split_lane(r, a, chunk, tid, L);
        const uint4 incl = wave_scan(split_piece(L), lane, SplitCompose());
        wg_put(wtot, incl, wave, lane);
        uint4 excl = wave_excl(incl, lane, split_identity());
        const uint4 cin = j.cin[r.choff + chunk];
        __syncthreads();
        excl = SplitCompose()(wg_front(wtot, wave, cin, SplitCompose()), excl);  // everything of the range in front of this lane
        const uint4 tot = SplitCompose()(cin, wg_total(wtot, SplitCompose()));
        // the chunk's output lies in [lo, hi) of the range's part of the store; the image starts at lo rounded down to 16
        const uint32_t lo = cin.w + ((cin.x & SPL_OPEN) ? cin.z : 0u);
        const uint32_t hi = tot.w + ((tot.x & SPL_OPEN) ? tot.z : 0u);
        const uint32_t ibase = lo & ~15u;
        {
            uint32_t open = excl.x >> 31, next = rb.units + (excl.x & SPL_CNT), cur = next - 1u, off = excl.w, k = excl.z;
            uint32_t mw = ~0u, mm = 0u;  // the image word this lane is filling and its bits
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const uint32_t m = 1u << q;
                if (!(L.V & m)) continue;
                const uint32_t c = (L.b[q >> 2] >> (8 * (q & 3))) & 0xffu;
                if (L.T & m) {
                    if (open) {
                        if (cur < j.tab_cap) j.tab[cur].bytes = k;
                        off += split_r16(k);
                    }
                    open = 0u;
                    k = 0u;
                } else if (L.H & m) {
                    cur = next++;
                    open = 1u;
                    k = 0u;
                    if (cur < j.tab_cap) {
                        ferhip_nal_unit &u = j.tab[cur];
                        u.range = (uint32_t)s;
                        u.nal_type = (int32_t)(c & 0x1fu);
                        u.ref_idc = (int32_t)((c & 0x7fu) >> 5);
                        u.offset = rb.bytes + off;
                    }
                } else if (open && !(L.D & m)) {
                    const uint32_t at = off + k - ibase;
                    k++;
                    if (at < SPL_IMG) {
                        img[at] = (uint8_t)c;
                        if ((at >> 4) != mw) {
                            if (mm) atomicOr(&msk[mw], mm);
                            mw = at >> 4;
                            mm = 0u;
                        }
                        mm |= 1u << (at & 15u);
                    }
                }
            }
            if (mm) atomicOr(&msk[mw], mm);
            // a unit that is open behind the range's last byte ends there
            const int last = (int)(a + r.len) - 1 - ((int)(chunk * SPL_CHUNK) + tid * 16);
            if (open && last >= 0 && last < 16 && cur < j.tab_cap) j.tab[cur].bytes = k;
        }
        __syncthreads();
        // not store_span: several units share a chunk, so [lo, hi) has holes (the rounding behind a unit) besides its two ends
        const unsigned long long g0 = rb.bytes + ibase;  // a multiple of 16
        const uint32_t nwords = min((hi - ibase + 15u) >> 4, (uint32_t)(SPL_IMG / 16));
        for (uint32_t w = tid; w < nwords; w += SPL_THREADS) {
            const uint32_t m = msk[w];
            const unsigned long long g = g0 + ((unsigned long long)w << 4);
            if (m == 0xffffu && g + 16ull <= j.cap) {
                *(uint4 *)(j.dst + g) = *(const uint4 *)(img + (w << 4));
            } else if (m) {
                for (uint32_t b = 0; b < 16u; b++)
                    if ((m >> b & 1u) && g + b < j.cap) j.dst[g + b] = img[(w << 4) + b];
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(SPL_THREADS) void k_split_prefix(FerSplitJob j)
{
    const uint32_t u = blockIdx.x * (SPL_THREADS / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (u >= min(j.head->units, j.tab_cap) || lane >= FER_SPLIT_PREFIX / 16) return;
    const ferhip_nal_unit e = j.tab[u];
    const unsigned long long slot = ((unsigned long long)e.bytes + 15ull) & ~15ull;
    if (e.offset + slot > j.cap || lane * 16u >= min((uint32_t)slot, (uint32_t)FER_SPLIT_PREFIX)) return;  // not stored / shorter
    *(uint4 *)(j.pref + (size_t)u * FER_SPLIT_PREFIX + lane * 16u) = *(const uint4 *)(j.dst + e.offset + lane * 16u);
}


// ---- length-prefixed ranges

// pass 0 (write == 0): rtot[r] = (units, chunk slots), fault[r]; pass 1: the units' records, from rbase[r] on.  Between the
// two k_split_index sums rtot as it does for Annex-B ranges: rbase[r].bytes is then the range's first chunk slot (the slots of
// a job are a 32-bit count, fer_split_run) and head->bytes their total, which nothing reads before k_avcc_index replaces it.
__global__ __launch_bounds__(64) void k_avcc_walk(FerSplitJob j, int write)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= j.n) return;
    const FerSplitRange r = j.rng[s];
    const uint32_t n = r.len, L = (uint32_t)j.lsize;
    uint32_t ubase = 0u, chbase = 0u;
    if (write) {
        const FerSplitBase b = j.rbase[s];
        ubase = b.units;
        chbase = (uint32_t)b.bytes;
    }
    uint32_t pos = 0u, units = 0u, chunks = 0u, fault = 0u;
    bool cut = false;
    while (!cut && n - pos >= L) {  // pos <= n throughout
        uint32_t len = 0u;
        for (uint32_t k = 0; k < L; k++) len = len << 8 | r.p[pos + k];
        const uint32_t st = pos + L;
        if (len == 0u) {
            cut = true;
        } else if (len > n - st) {
            cut = true;
            fault = 1u;
        } else if (len == 1u) {
            cut = true;
        } else {
            const uint32_t a = (uint32_t)((uintptr_t)(r.p + st + 1u) & 15u);
            const uint32_t u = ubase + units;
            if (write && u < j.tab_cap) {
                FerAvccUnit rec;
                rec.range = (uint32_t)s | (uint32_t)r.p[st] << 16;
                rec.st = st;
                rec.en = st + len;
                rec.choff = chbase + chunks;
                j.aunit[u] = rec;
            }
            units++;
            chunks += (a + (len - 1u) + SPL_CHUNK - 1u) / SPL_CHUNK;
            pos = st + len;
        }
    }
    if (!cut && pos < n) fault = 1u;  // fewer than L bytes are left: a unit that cannot state its length
    if (!write) {
        j.rtot[s] = make_uint2(units, chunks);
        j.fault[s] = (int32_t)fault;
    }
}

// A unit's payload is s[st+1 .. en); its image starts a = (address of s[st+1]) & 15 bytes in front of it.  Lane tid of chunk
// `chunk` takes image bytes [v0, v0 + 16): w = the word, V = one bit per byte inside the payload, D = per dropped 03.
// The two bytes in front of the word come from the dword that ends at v0, read only when it holds a payload byte.
__device__ __forceinline__ void avcc_lane(const uint8_t *pay, uint32_t a, uint32_t paylen, uint32_t chunk, int tid, uint4 &w, uint32_t &V, uint32_t &D)
{
    const uint8_t *base = pay - a;
    const int end = (int)(a + paylen), ia = (int)a;
    const int v0 = (int)(chunk * SPL_CHUNK) + tid * 16;
    w = make_uint4(~0u, ~0u, ~0u, ~0u);
    V = D = 0u;
    if (v0 + 16 <= ia || v0 >= end) return;
    w = *(const uint4 *)(base + v0);
    uint32_t prev = ~0u;
    if (v0 > ia) prev = *(const uint32_t *)(base + v0 - 4);
    const int lo = max(ia - v0, 0), hi = min(end - v0, 16);
    V = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    const uint32_t x[4] = {w.x, w.y, w.z, w.w};
    uint32_t Z = 0u, Th = 0u;  // bit k + 2: byte k of the word is 00 / 03 (and inside the payload); bits 0, 1: the two bytes in front
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t c = (x[k >> 2] >> (8 * (k & 3))) & 0xffu;
        Z |= (uint32_t)(c == 0u) << (k + 2);
        Th |= (uint32_t)(c == 3u) << (k + 2);
    }
    Z &= V << 2;
    Th &= V << 2;
    if (v0 - 2 >= ia) Z |= (uint32_t)(((prev >> 16) & 0xffu) == 0u);
    if (v0 - 1 >= ia) Z |= (uint32_t)((prev >> 24) == 0u) << 1;
    D = (Th & (Z << 1) & (Z << 2)) >> 2;
}

__device__ __forceinline__ uint32_t avcc_nch(uint32_t a, uint32_t paylen) { return (a + paylen + SPL_CHUNK - 1u) / SPL_CHUNK; }

__global__ __launch_bounds__(SPL_THREADS) void k_avcc_count(FerSplitJob j)
{
    const uint32_t nu = min(j.head->units, j.tab_cap);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint32_t wtot[SPL_THREADS / 64];
    for (uint32_t u = blockIdx.y; u < nu; u += gridDim.y) {
    const FerAvccUnit rec = j.aunit[u];
    const uint8_t *pay = j.rng[rec.range & 0xffffu].p + rec.st + 1u;
    const uint32_t paylen = rec.en - rec.st - 1u, a = (uint32_t)((uintptr_t)pay & 15u), nch = avcc_nch(a, paylen);
    for (uint32_t chunk = blockIdx.x; chunk < nch; chunk += gridDim.x) {
        uint4 w;
        uint32_t V, D;
        avcc_lane(pay, a, paylen, chunk, tid, w, V, D);
        uint32_t c = (uint32_t)__popc(D);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
        wg_put(wtot, c, wave, lane);  // every lane holds its wavefront's count
        __syncthreads();
        if (tid == 0) j.acnt()[rec.choff + chunk] = wg_total(wtot, ScanAdd());
        __syncthreads();
    }
    }
}

__global__ __launch_bounds__(64) void k_avcc_plan(FerSplitJob j)
{
    const uint32_t u = blockIdx.x;
    if (u >= min(j.head->units, j.tab_cap)) return;
    const FerAvccUnit rec = j.aunit[u];
    const uint8_t *pay = j.rng[rec.range & 0xffffu].p + rec.st + 1u;
    const uint32_t paylen = rec.en - rec.st - 1u, nch = avcc_nch((uint32_t)((uintptr_t)pay & 15u), paylen);
    const int lane = threadIdx.x;
    const uint32_t run = carry_scan(
        nch, lane, 0u, ScanAdd(), [&](uint32_t i) { return j.acnt()[rec.choff + i]; },
        [&](uint32_t i, uint32_t in) { j.acin()[rec.choff + i] = in; });
    if (lane == 0) j.tab[u].bytes = paylen - run;
}

__global__ __launch_bounds__(64) void k_avcc_index(FerSplitJob j)
{
    const int lane = threadIdx.x;
    const uint32_t nu = min(j.head->units, j.tab_cap);
    unsigned long long run = 0;
    for (uint32_t u0 = 0; u0 < nu; u0 += 64) {
        const uint32_t u = u0 + lane;
        const uint32_t b = u < nu ? j.tab[u].bytes : 0u;
        const unsigned long long r = ((unsigned long long)b + 15ull) & ~15ull;
        const unsigned long long incl = wave_scan(r, lane, ScanAdd());
        if (u < nu) {
            const FerAvccUnit rec = j.aunit[u];
            const uint32_t c = rec.range >> 16;
            ferhip_nal_unit e;
            e.range = rec.range & 0xffffu;
            e.nal_type = (int32_t)(c & 0x1fu);
            e.ref_idc = (int32_t)((c & 0x7fu) >> 5);
            e.bytes = b;
            e.offset = run + incl - r;
            j.tab[u] = e;
        }
        run += __shfl(incl, 63);
    }
    if (lane == 0) j.head->bytes = run;  // of the units in the table: with more units than that the host repeats the job
}

__global__ __launch_bounds__(SPL_THREADS) void k_avcc_emit(FerSplitJob j)
{
    const uint32_t nu = min(j.head->units, j.tab_cap);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint32_t wtot[SPL_THREADS / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[AVCC_IMG];
    for (uint32_t u = blockIdx.y; u < nu; u += gridDim.y) {
    const FerAvccUnit rec = j.aunit[u];
    const uint8_t *pay = j.rng[rec.range & 0xffffu].p + rec.st + 1u;
    const uint32_t paylen = rec.en - rec.st - 1u, a = (uint32_t)((uintptr_t)pay & 15u), nch = avcc_nch(a, paylen);
    const unsigned long long uoff = j.tab[u].offset;
    for (uint32_t chunk = blockIdx.x; chunk < nch; chunk += gridDim.x) {
        uint4 w;
        uint32_t V, D;
        avcc_lane(pay, a, paylen, chunk, tid, w, V, D);
        const uint32_t K = V & ~D, c = (uint32_t)__popc(K);
        const uint32_t incl = wave_scan(c, lane, ScanAdd());
        wg_put(wtot, incl, wave, lane);
        __syncthreads();
        const uint32_t pre = wg_front(wtot, wave, 0u, ScanAdd());
        const uint32_t n = wg_total(wtot, ScanAdd());  // the chunk's surviving bytes
        // the chunk's span of the store: [o, o + n), staged in img at [sh, sh + n) so that 16-byte words line up
        const uint32_t inb = chunk ? chunk * SPL_CHUNK - a : 0u;  // payload bytes in front of the chunk
        const unsigned long long o = uoff + (inb - j.acin()[rec.choff + chunk]);
        const uint32_t sh = (uint32_t)o & 15u;
        {
            uint32_t p = sh + pre + incl - c;
            const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (K >> k & 1u) img[p++] = (uint8_t)(x[k >> 2] >> (8 * (k & 3)));
        }
        __syncthreads();
        store_span<SPL_THREADS>(j.dst + (o - sh), img, sh, span_cut(o - sh, sh + n, j.cap));
        __syncthreads();
    }
    }
}

// The launches of pass `pass` of a job; gx = workgroups per range (Annex-B) or unit (length-prefixed): one of more chunks
// walks them with that stride.  A pass behind the first one follows a table or a store that had to grow.  Annex-B: the plan
// stands (chunk functions, range sums), so only k_split_index -- a new table has no totals yet -- and the emit are repeated.
// Length-prefixed: the whole job, which is a handful of small launches.
static void split_launch(const FerSplitJob &j, unsigned gx, int pass, hipStream_t st)
{
    if (j.lsize) {
        const unsigned gr = (unsigned)((j.n + 63) / 64);
        hipLaunchKernelGGL(k_avcc_walk, dim3(gr), dim3(64), 0, st, j, 0);
        hipLaunchKernelGGL(k_split_index, dim3(1), dim3(64), 0, st, j);
        hipLaunchKernelGGL(k_avcc_walk, dim3(gr), dim3(64), 0, st, j, 1);
        const unsigned gy = (unsigned)std::min<uint32_t>(j.tab_cap, 32768u);  // more units than that: a workgroup takes several
        hipLaunchKernelGGL(k_avcc_count, dim3(gx, gy), dim3(SPL_THREADS), 0, st, j);
        hipLaunchKernelGGL(k_avcc_plan, dim3(j.tab_cap), dim3(64), 0, st, j);
        hipLaunchKernelGGL(k_avcc_index, dim3(1), dim3(64), 0, st, j);
        hipLaunchKernelGGL(k_avcc_emit, dim3(gx, gy), dim3(SPL_THREADS), 0, st, j);
    } else {
        if (pass == 0) {
            hipLaunchKernelGGL(k_split_count, dim3(gx, j.n), dim3(SPL_THREADS), 0, st, j);
            hipLaunchKernelGGL(k_split_plan, dim3(j.n), dim3(64), 0, st, j);
        }
        hipLaunchKernelGGL(k_split_index, dim3(1), dim3(64), 0, st, j);
        hipLaunchKernelGGL(k_split_emit, dim3(gx, j.n), dim3(SPL_THREADS), 0, st, j);
    }
    if (j.pref) hipLaunchKernelGGL(k_split_prefix, dim3((j.tab_cap + 3) / 4), dim3(SPL_THREADS), 0, st, j);
}

// ---- host side
static size_t split_res_bytes(size_t tab_cap) { return sizeof(FerSplitHead) + tab_cap * (sizeof(ferhip_nal_unit) + FER_SPLIT_PREFIX); }

// the table and the prefix array for `units` (>= tab_cap) units, device and pinned
static int split_reserve_table(FerSplit &sp, size_t units)
{
    const bool ok = !sp.d_res.reserve(split_res_bytes(units)) && !sp.h_res.reserve(split_res_bytes(units));
    sp.tab_cap = ok ? units : 0;
    return ok ? 0 : FERHIP_E_HIP;
}

int fer_split_run(FerSplit &sp, hipStream_t st, const uint8_t *const *ptrs, const size_t *lens, int n, uint8_t *dst, size_t cap, int length_size)
{
    if (n <= 0 || n > 65535 || (length_size != 0 && length_size != 1 && length_size != 2 && length_size != 4)) return FERHIP_E_ARG;
    const bool avcc = length_size != 0;
    if (!sp.ev0) CK(hipEventCreate(&sp.ev0));
    if (!sp.ev1) CK(hipEventCreate(&sp.ev1));
    if (sp.d_rng.reserve(n) || sp.h_rng.reserve(n) || sp.d_rtot.reserve(n) || sp.d_rbase.reserve(n)) return FERHIP_E_HIP;
    if (avcc && (sp.d_fault.reserve(n, sp.d_rng.cap) || sp.h_fault.reserve(n, sp.d_rng.cap))) return FERHIP_E_HIP;
    size_t nchunks = 0, nchmax = 1, in_bytes = 0, need = 0;
    for (int s = 0; s < n; s++) {
        const size_t len = ptrs[s] ? lens[s] : 0;
        if (len > SPL_MAX_LEN) return FERHIP_E_ARG;
        FerSplitRange &r = sp.h_rng[s];
        r.p = len ? ptrs[s] : nullptr;
        r.len = (uint32_t)len;
        r.choff = (uint32_t)nchunks;
        const size_t nch = len ? (((uintptr_t)ptrs[s] & 15) + len + SPL_CHUNK - 1) / SPL_CHUNK : 0;
        nchunks += nch;
        nchmax = std::max(nchmax, nch);
        in_bytes += len;
        need += (len + 15) & ~(size_t)15;
    }
    if (nchunks >> 32) return FERHIP_E_ARG;
    if (int rc = split_reserve_table(sp, std::max<size_t>(sp.tab_cap, std::max<size_t>(64, 4 * (size_t)n)))) return rc;
    // length-prefixed: a unit's payload is chunked on an image of its own, which costs a unit up to two chunk slots more than
    // its bytes alone; the slots are 32-bit counts in the arrays of the chunk functions (four to an element), and the records
    // (one per table entry) and the slots follow the table when it grows
    auto avcc_slots = [&]() { return (in_bytes / SPL_CHUNK + 2 * sp.tab_cap + 4) / 4 + 1; };
    if (avcc) nchunks = avcc_slots();
    if (sp.d_summ.reserve(nchunks, nchunks + nchunks / 4 + 64) || sp.d_cin.reserve(nchunks, nchunks + nchunks / 4 + 64)) return FERHIP_E_HIP;
    if (avcc && sp.d_aunit.reserve(sp.tab_cap)) return FERHIP_E_HIP;
    // a unit's RBSP is shorter than its bytes in the range, but every unit is rounded up to 16: the store holds the ranges'
    // lengths, which is enough unless units of a few bytes abound; the true total tells, and the emit launch is repeated.
    // k_dec_parse reads whole dwords up to 4 bytes behind a unit: 64 spare bytes like the host path's buffer
    if (!dst && sp.d_store.reserve(need + 64, need + need / 4 + 4096)) return FERHIP_E_HIP;
    const unsigned gx = (unsigned)std::min<size_t>(nchmax, 64);  // a range of more chunks walks them with that stride
    CK(hipMemcpyAsync(sp.d_rng, sp.h_rng, sizeof(FerSplitRange) * n, hipMemcpyHostToDevice, st));
    // A pass is the launches and one fetch of the totals; they tell whether the table or the store was too small, and then the
    // buffers grow and the job is repeated.  Annex-B totals come from the plan and are exact: one repeat at the most.  Length-
    // prefixed: the first total of the bytes covers the units of the old table only, so behind a table that grew the store is
    // looked at once more: two repeats at the most.
    for (int pass = 0;; pass++) {
        FerSplitJob j;
        j.rng = sp.d_rng;
        j.n = n;
        j.summ = sp.d_summ;
        j.cin = sp.d_cin;
        j.rtot = sp.d_rtot;
        j.rbase = sp.d_rbase;
        j.head = (FerSplitHead *)sp.d_res.p;
        j.tab = (ferhip_nal_unit *)(sp.d_res + sizeof(FerSplitHead));
        j.tab_cap = (uint32_t)sp.tab_cap;
        j.dst = dst ? dst : sp.d_store.p;
        j.cap = dst ? cap : sp.d_store.cap - 64;
        j.pref = dst ? nullptr : sp.d_res + sizeof(FerSplitHead) + sp.tab_cap * sizeof(ferhip_nal_unit);
        j.lsize = length_size;
        j.aunit = sp.d_aunit;
        j.fault = sp.d_fault;
        if (pass == 0) CK(hipEventRecord(sp.ev0, st));
        split_launch(j, gx, pass, st);
        if (pass == 0) CK(hipEventRecord(sp.ev1, st));
        CK(hipGetLastError());
        // the totals, the table and (the decoder's jobs) the prefixes in one copy
        const size_t nb = dst ? sizeof(FerSplitHead) + sp.tab_cap * sizeof(ferhip_nal_unit) : split_res_bytes(sp.tab_cap);
        CK(hipMemcpyAsync(sp.h_res, sp.d_res, nb, hipMemcpyDeviceToHost, st));
        if (avcc) CK(hipMemcpyAsync(sp.h_fault, sp.d_fault, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        CK(hipStreamSynchronize(st));
        if (pass == 0) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, sp.ev0, sp.ev1) == hipSuccess) sp.ms += ms;
            sp.in_bytes += in_bytes;
        }
        const size_t units = sp.head()->units, total = (size_t)sp.head()->bytes;
        const bool more_units = units > sp.tab_cap, more_store = !dst && total > sp.d_store.cap - 64;
        if (pass == 2 || (!more_units && !more_store)) return 0;
        if (more_units)
            if (int rc = split_reserve_table(sp, units + units / 4 + 64)) return rc;
        if (more_store && sp.d_store.reserve(total + 64, total + total / 4 + 4096)) return FERHIP_E_HIP;
        if (avcc && (sp.d_aunit.reserve(sp.tab_cap) || sp.d_summ.reserve(avcc_slots()) || sp.d_cin.reserve(avcc_slots()))) return FERHIP_E_HIP;
    }
}

// known-answer surface: host ranges through the same kernels, on the null stream with buffers of its own
static int split_blocks(const uint8_t *ranges, size_t stride, const uint32_t *lens, size_t n, int misalign, int length_size, uint8_t *out,
                        size_t cap, ferhip_nal_unit *units, size_t units_cap, size_t *nunits, int32_t *range_fault)
{
    if (nunits) *nunits = 0;
    if (!lens || !nunits || n == 0 || n > 65535 || misalign < 0 || misalign > 15 || (!out && cap) || (!units && units_cap)) return FERHIP_E_ARG;
    for (size_t i = 0; i < n; i++)
        if (lens[i] > stride || lens[i] > SPL_MAX_LEN || (lens[i] && !ranges)) return FERHIP_E_ARG;
    // every range ends at the end of an allocation of its own and starts `misalign` bytes behind a 16-byte boundary
    std::vector<DevBuf<uint8_t>> alloc(n);
    std::vector<const uint8_t *> ptrs(n, nullptr);
    std::vector<size_t> ln(n, 0);
    DevBuf<uint8_t> dst;
    FerSplit sp;
    for (size_t i = 0; i < n; i++) {
        if (!lens[i]) continue;
        if (alloc[i].reserve((size_t)misalign + lens[i])) return FERHIP_E_HIP;
        CK(hipMemcpy(alloc[i] + misalign, ranges + i * stride, lens[i], hipMemcpyHostToDevice));
        ptrs[i] = alloc[i] + misalign;
        ln[i] = lens[i];
    }
    if (dst.reserve(std::max<size_t>(cap, 16))) return FERHIP_E_HIP;
    if (cap) CK(hipMemcpy(dst, out, cap, hipMemcpyHostToDevice));
    if (int rc = fer_split_run(sp, nullptr, ptrs.data(), ln.data(), (int)n, dst, cap, length_size)) return rc;
    if (cap) CK(hipMemcpy(out, dst, cap, hipMemcpyDeviceToHost));
    size_t k = 0;
    fer_split_each_unit(sp, [&](size_t, const ferhip_nal_unit &u) {
        if (k < units_cap) units[k] = u;
        k++;
        return 0;
    });
    *nunits = k;
    if (range_fault)
        for (size_t i = 0; i < n; i++) range_fault[i] = length_size ? sp.h_fault[i] : 0;
    return k > units_cap || (size_t)sp.head()->bytes > cap ? FERHIP_E_ARG : 0;
}

extern "C" int ferhip_split_nal_blocks(const uint8_t *ranges, size_t stride, const uint32_t *lens, size_t n, int misalign, uint8_t *out,
                                       size_t cap, ferhip_nal_unit *units, size_t units_cap, size_t *nunits)
{
    return split_blocks(ranges, stride, lens, n, misalign, 0, out, cap, units, units_cap, nunits, nullptr);
}

extern "C" int ferhip_split_avcc_blocks(const uint8_t *ranges, size_t stride, const uint32_t *lens, size_t n, int misalign, int length_size,
                                        uint8_t *out, size_t cap, ferhip_nal_unit *units, size_t units_cap, size_t *nunits,
                                        int32_t *range_fault)
{
    if (length_size != 1 && length_size != 2 && length_size != 4) {
        if (nunits) *nunits = 0;
        return FERHIP_E_ARG;
    }
    return split_blocks(ranges, stride, lens, n, misalign, length_size, out, cap, units, units_cap, nunits, range_fault);
}
