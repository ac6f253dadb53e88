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
// begun and ended inside); see split_compose.
//
//   k_split_count  grid (chunk, range): a lane takes 16 bytes of the range's 16-byte-aligned image (a range may start
//                  anywhere: the bytes in front of it and behind it read as ff, which takes part in no pattern) with 8
//                  bytes in front and 4 behind, reduces them to their function; the 256 lanes compose theirs in order
//                  (wavefront scan by shuffles, the four wavefronts through LDS); one function per 4096-byte chunk.
//   k_split_plan   one wavefront per range composes the chunk functions in order: what comes into every chunk, and the
//                  range's units and bytes.
//   k_split_index  one wavefront: exclusive sums over the ranges, and the totals in front of the table.
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
//                 their chunks and finds its fault, then (behind k_avcc_base) it writes one record per unit (range, header
//                 byte, st, en, first chunk slot).
//   k_avcc_base   one wavefront: exclusive sums of the units and chunks over the ranges, the total of the units.
//   k_avcc_count  grid (chunk, unit): the dropped 03 bytes of every chunk.
//   k_avcc_plan   one wavefront per unit: exclusive sum of its chunk counts = the 03 bytes in front of every chunk, and the
//                 unit's RBSP size.
//   k_avcc_index  one wavefront: exclusive sum of the 16-rounded RBSP sizes over the units = their offsets; the table
//                 entries and the totals in front of the table.
//   k_avcc_emit   grid (chunk, unit): the chunk's surviving bytes are compacted in LDS in output order and the span is
//                 stored with 16-byte stores, its ragged ends byte-wise (k_nal_emit's way); nothing at or behind `cap`.
//   k_split_prefix as above.
#include "fer_nalsplit.h"
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
    uint32_t *acnt, *acin;  // [chunk slots] dropped 03 bytes of a chunk / in front of it within its unit
    int32_t *fault;       // [n] the range overran
};

// A run's function as a uint4: x = units begun | has an event << 30 | open at the end << 31, y = head bytes, z = bytes of
// the open unit, w = 16-rounded bytes of the units begun and ended inside.
#define SPL_EV (1u << 30)
#define SPL_OPEN (1u << 31)
#define SPL_CNT (SPL_EV - 1u)
__device__ __forceinline__ uint4 split_identity() { return make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ uint32_t split_r16(uint32_t v) { return (v + 15u) & ~15u; }

// f first, then g (adjacent runs of one range)
__device__ __forceinline__ uint4 split_compose(const uint4 &f, const uint4 &g)
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

__device__ __forceinline__ uint4 split_shfl_up(const uint4 &f, int m)
{
    return make_uint4(__shfl_up(f.x, m), __shfl_up(f.y, m), __shfl_up(f.z, m), __shfl_up(f.w, m));
}
__device__ __forceinline__ uint4 split_shfl(const uint4 &f, int l) { return make_uint4(__shfl(f.x, l), __shfl(f.y, l), __shfl(f.z, l), __shfl(f.w, l)); }

// inclusive scan over the wavefront, lane order
__device__ __forceinline__ uint4 split_wave_scan(uint4 f, int lane)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint4 t = split_shfl_up(f, m);
        if (lane >= m) f = split_compose(t, f);
    }
    return f;
}

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
        const uint4 incl = split_wave_scan(split_piece(L), lane);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        if (tid == 0) j.summ[r.choff + chunk] = split_compose(split_compose(wtot[0], wtot[1]), split_compose(wtot[2], wtot[3]));
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_split_plan(FerSplitJob j)
{
    const FerSplitRange r = j.rng[blockIdx.x];
    const int lane = threadIdx.x;
    const uint32_t nch = split_nch(r, (uint32_t)((uintptr_t)r.p & 15u));
    uint4 run = split_identity();  // everything in front of the block of 64 chunks
    for (uint32_t i0 = 0; i0 < nch; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint4 f = i < nch ? j.summ[r.choff + i] : split_identity();
        const uint4 incl = split_wave_scan(f, lane);
        uint4 excl = split_shfl_up(incl, 1);
        if (lane == 0) excl = split_identity();
        if (i < nch) j.cin[r.choff + i] = split_compose(run, excl);
        run = split_compose(run, split_shfl(incl, 63));
    }
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
        unsigned long long ib = e.y;
        uint32_t iu = e.x;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned long long tb = __shfl_up(ib, m);
            const uint32_t tu = __shfl_up(iu, m);
            if (lane >= m) {
                ib += tb;
                iu += tu;
            }
        }
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
        const uint4 incl = split_wave_scan(split_piece(L), lane);
        if (lane == 63) wtot[wave] = incl;
        uint4 excl = split_shfl_up(incl, 1);
        if (lane == 0) excl = split_identity();
        const uint4 cin = j.cin[r.choff + chunk];
        __syncthreads();
        uint4 pre = cin;
        for (int w = 0; w < wave; w++) pre = split_compose(pre, wtot[w]);
        excl = split_compose(pre, excl);  // everything of the range in front of this lane
        const uint4 tot = split_compose(cin, split_compose(split_compose(wtot[0], wtot[1]), split_compose(wtot[2], wtot[3])));
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

static void split_launch_plan(const FerSplitJob &j, unsigned gx, hipStream_t st)
{
    hipLaunchKernelGGL(k_split_count, dim3(gx, j.n), dim3(SPL_THREADS), 0, st, j);
    hipLaunchKernelGGL(k_split_plan, dim3(j.n), dim3(64), 0, st, j);
    hipLaunchKernelGGL(k_split_index, dim3(1), dim3(64), 0, st, j);
}
static void split_launch_emit(const FerSplitJob &j, unsigned gx, hipStream_t st)
{
    hipLaunchKernelGGL(k_split_emit, dim3(gx, j.n), dim3(SPL_THREADS), 0, st, j);
    if (j.pref) hipLaunchKernelGGL(k_split_prefix, dim3((j.tab_cap + 3) / 4), dim3(SPL_THREADS), 0, st, j);
}


// ---- length-prefixed ranges

// pass 0 (write == 0): rtot[r] = (units, chunk slots), fault[r]; pass 1: the units' records, from rbase[r] on
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

__global__ __launch_bounds__(64) void k_avcc_base(FerSplitJob j)
{
    const int lane = threadIdx.x;
    uint32_t units = 0u, chunks = 0u;
    for (int s0 = 0; s0 < j.n; s0 += 64) {
        const int s = s0 + lane;
        const uint2 e = s < j.n ? j.rtot[s] : make_uint2(0u, 0u);
        uint32_t iu = e.x, ic = e.y;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t tu = __shfl_up(iu, m), tc = __shfl_up(ic, m);
            if (lane >= m) {
                iu += tu;
                ic += tc;
            }
        }
        if (s < j.n) {
            FerSplitBase b;
            b.bytes = chunks + ic - e.y;  // the range's first chunk slot
            b.units = units + iu - e.x;
            b.pad = 0;
            j.rbase[s] = b;
        }
        units += __shfl(iu, 63);
        chunks += __shfl(ic, 63);
    }
    if (lane == 0) {
        FerSplitHead h;
        h.bytes = 0;
        h.units = units;
        h.pad = 0;
        *j.head = h;
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
        if (lane == 0) wtot[wave] = c;
        __syncthreads();
        if (tid == 0) j.acnt[rec.choff + chunk] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
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
    uint32_t run = 0u;
    for (uint32_t i0 = 0; i0 < nch; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint32_t c = i < nch ? j.acnt[rec.choff + i] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t t = __shfl_up(incl, m);
            if (lane >= m) incl += t;
        }
        if (i < nch) j.acin[rec.choff + i] = run + incl - c;
        run += __shfl(incl, 63);
    }
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
        unsigned long long incl = r;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned long long t = __shfl_up(incl, m);
            if (lane >= m) incl += t;
        }
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
        uint32_t incl = c;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t t = __shfl_up(incl, m);
            if (lane >= m) incl += t;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        uint32_t pre = 0u;
        for (int k = 0; k < wave; k++) pre += wtot[k];
        const uint32_t n = wtot[0] + wtot[1] + wtot[2] + wtot[3];  // the chunk's surviving bytes
        // the chunk's span of the store: [o, o + n), staged in img at [sh, sh + n) so that 16-byte words line up
        const uint32_t inb = chunk ? chunk * SPL_CHUNK - a : 0u;  // payload bytes in front of the chunk
        const unsigned long long o = uoff + (inb - j.acin[rec.choff + chunk]);
        const uint32_t sh = (uint32_t)o & 15u;
        {
            uint32_t p = sh + pre + incl - c;
            const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (K >> k & 1u) img[p++] = (uint8_t)(x[k >> 2] >> (8 * (k & 3)));
        }
        __syncthreads();
        const unsigned long long g0 = o - sh;  // a multiple of 16
        const uint32_t nwords = (sh + n + 15u) >> 4;
        for (uint32_t q = tid; q < nwords; q += SPL_THREADS) {
            const uint32_t lo = q << 4, hi = lo + 16u;
            if (lo >= sh && hi <= sh + n && g0 + hi <= j.cap) {
                *(uint4 *)(j.dst + g0 + lo) = *(const uint4 *)(img + lo);
            } else {
                for (uint32_t k = max(lo, sh); k < min(hi, sh + n); k++)
                    if (g0 + k < j.cap) j.dst[g0 + k] = img[k];
            }
        }
        __syncthreads();
    }
    }
}

// the launches of a length-prefixed job; gx = workgroups per unit (a unit of more chunks walks them with that stride)
static void avcc_launch(const FerSplitJob &j, unsigned gx, hipStream_t st)
{
    const unsigned gr = (unsigned)((j.n + 63) / 64);
    hipLaunchKernelGGL(k_avcc_walk, dim3(gr), dim3(64), 0, st, j, 0);
    hipLaunchKernelGGL(k_avcc_base, dim3(1), dim3(64), 0, st, j);
    hipLaunchKernelGGL(k_avcc_walk, dim3(gr), dim3(64), 0, st, j, 1);
    const unsigned gy = (unsigned)std::min<uint32_t>(j.tab_cap, 32768u);  // more units than that: a workgroup takes several
    hipLaunchKernelGGL(k_avcc_count, dim3(gx, gy), dim3(SPL_THREADS), 0, st, j);
    hipLaunchKernelGGL(k_avcc_plan, dim3(j.tab_cap), dim3(64), 0, st, j);
    hipLaunchKernelGGL(k_avcc_index, dim3(1), dim3(64), 0, st, j);
    hipLaunchKernelGGL(k_avcc_emit, dim3(gx, gy), dim3(SPL_THREADS), 0, st, j);
    if (j.pref) hipLaunchKernelGGL(k_split_prefix, dim3((j.tab_cap + 3) / 4), dim3(SPL_THREADS), 0, st, j);
}

// ---- host side
template <typename T>
static int split_grow(T **p, size_t *cap, size_t want, bool pinned = false)
{
    if (*cap >= want && *p) return 0;
    if (*p) pinned ? (void)hipHostFree(*p) : (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    if ((pinned ? hipHostMalloc((void **)p, want * sizeof(T)) : hipMalloc((void **)p, want * sizeof(T))) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return FERHIP_E_HIP;
    }
    *cap = want;
    return 0;
}

void fer_split_free(FerSplit &sp)
{
    for (void *p : {(void *)sp.d_rng, (void *)sp.d_rtot, (void *)sp.d_rbase, (void *)sp.d_summ, (void *)sp.d_cin, (void *)sp.d_res, (void *)sp.d_store, (void *)sp.d_fault,
                    (void *)sp.d_aunit})
        if (p) hipFree(p);
    if (sp.h_rng) hipHostFree(sp.h_rng);
    if (sp.h_fault) hipHostFree(sp.h_fault);
    if (sp.h_res) hipHostFree(sp.h_res);
    if (sp.ev0) hipEventDestroy(sp.ev0);
    if (sp.ev1) hipEventDestroy(sp.ev1);
    sp = FerSplit();
}

static size_t split_res_bytes(size_t tab_cap) { return sizeof(FerSplitHead) + tab_cap * (sizeof(ferhip_nal_unit) + FER_SPLIT_PREFIX); }

// the table and the prefix array for tab_cap units, device and pinned
static int split_grow_table(FerSplit &sp, size_t want)
{
    if (sp.tab_cap >= want && sp.d_res && sp.h_res) return 0;
    size_t c0 = sp.d_res ? sp.tab_cap : 0, c1 = sp.h_res ? sp.tab_cap : 0;
    c0 = split_res_bytes(c0);
    c1 = split_res_bytes(c1);
    if (split_grow(&sp.d_res, &c0, split_res_bytes(want)) || split_grow(&sp.h_res, &c1, split_res_bytes(want), true)) {
        sp.tab_cap = 0;
        return FERHIP_E_HIP;
    }
    sp.tab_cap = want;
    return 0;
}

int fer_split_run(FerSplit &sp, hipStream_t st, const uint8_t *const *ptrs, const size_t *lens, int n, uint8_t *dst, size_t cap, int length_size)
{
    if (n <= 0 || n > 65535 || (length_size != 0 && length_size != 1 && length_size != 2 && length_size != 4)) return FERHIP_E_ARG;
    const bool avcc = length_size != 0;
    if (!sp.ev0) CK(hipEventCreate(&sp.ev0));
    if (!sp.ev1) CK(hipEventCreate(&sp.ev1));
    if (sp.rng_cap < (size_t)n) {
        const size_t want = (size_t)n;
        size_t c0 = sp.d_rng ? sp.rng_cap : 0, c1 = sp.h_rng ? sp.rng_cap : 0, c2 = sp.d_rtot ? sp.rng_cap : 0, c3 = sp.d_rbase ? sp.rng_cap : 0;
        if (split_grow(&sp.d_rng, &c0, want) || split_grow(&sp.h_rng, &c1, want, true) || split_grow(&sp.d_rtot, &c2, want) ||
            split_grow(&sp.d_rbase, &c3, want)) {
            sp.rng_cap = 0;
            return FERHIP_E_HIP;
        }
        sp.rng_cap = want;
    }
    if (avcc && sp.fault_cap < (size_t)n) {
        size_t c0 = sp.d_fault ? sp.fault_cap : 0, c1 = sp.h_fault ? sp.fault_cap : 0;
        if (split_grow(&sp.d_fault, &c0, sp.rng_cap) || split_grow(&sp.h_fault, &c1, sp.rng_cap, true)) {
            sp.fault_cap = 0;
            return FERHIP_E_HIP;
        }
        sp.fault_cap = sp.rng_cap;
    }
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
    if (int rc = split_grow_table(sp, std::max<size_t>(sp.tab_cap, std::max<size_t>(64, 4 * (size_t)n)))) return rc;
    // length-prefixed: a unit's payload is chunked on an image of its own, which costs a unit up to two chunk slots more than
    // its bytes alone; the slots are 32-bit counts in the arrays of the chunk functions (four to an element)
    auto avcc_slots = [&]() { return (in_bytes / SPL_CHUNK + 2 * sp.tab_cap + 4) / 4 + 1; };
    if (avcc) nchunks = avcc_slots();
    if (sp.ch_cap < nchunks) {
        const size_t want = nchunks + nchunks / 4 + 64;
        size_t c0 = sp.d_summ ? sp.ch_cap : 0, c1 = sp.d_cin ? sp.ch_cap : 0;
        if (split_grow(&sp.d_summ, &c0, want) || split_grow(&sp.d_cin, &c1, want)) {
            sp.ch_cap = 0;
            return FERHIP_E_HIP;
        }
        sp.ch_cap = want;
    }
    // a unit's RBSP is shorter than its bytes in the range, but every unit is rounded up to 16: the store holds the ranges'
    // lengths, which is enough unless units of a few bytes abound; the true total tells, and the emit launch is repeated.
    // k_dec_parse reads whole dwords up to 4 bytes behind a unit: 64 spare bytes like the host path's buffer
    if (!dst && sp.store_cap < need + 64) {
        size_t c = sp.d_store ? sp.store_cap : 0;
        if (split_grow(&sp.d_store, &c, need + need / 4 + 4096)) {
            sp.store_cap = 0;
            return FERHIP_E_HIP;
        }
        sp.store_cap = c;
    }
    const unsigned gx = (unsigned)std::min<size_t>(nchmax, 64);  // a range of more chunks walks them with that stride
    FerSplitJob j;
    auto bind = [&]() {
        j.rng = sp.d_rng;
        j.n = n;
        j.summ = sp.d_summ;
        j.cin = sp.d_cin;
        j.rtot = sp.d_rtot;
        j.rbase = sp.d_rbase;
        j.head = (FerSplitHead *)sp.d_res;
        j.tab = (ferhip_nal_unit *)(sp.d_res + sizeof(FerSplitHead));
        j.tab_cap = (uint32_t)sp.tab_cap;
        j.dst = dst ? dst : sp.d_store;
        j.cap = dst ? cap : sp.store_cap - 64;
        j.pref = dst ? nullptr : sp.d_res + sizeof(FerSplitHead) + sp.tab_cap * sizeof(ferhip_nal_unit);
        j.lsize = length_size;
        j.aunit = sp.d_aunit;
        j.acnt = (uint32_t *)sp.d_summ;
        j.acin = (uint32_t *)sp.d_cin;
        j.fault = sp.d_fault;
    };
    auto grow_units = [&]() -> int {  // length-prefixed: one record per table entry
        if (!avcc || (sp.aunit_cap >= sp.tab_cap && sp.d_aunit)) return 0;
        size_t c = sp.d_aunit ? sp.aunit_cap : 0;
        if (split_grow(&sp.d_aunit, &c, sp.tab_cap)) {
            sp.aunit_cap = 0;
            return FERHIP_E_HIP;
        }
        sp.aunit_cap = c;
        return 0;
    };
    if (int rc = grow_units()) return rc;
    auto fetch = [&]() -> int {  // the totals, the table and (the decoder's jobs) the prefixes in one copy
        const size_t nb = dst ? sizeof(FerSplitHead) + sp.tab_cap * sizeof(ferhip_nal_unit) : split_res_bytes(sp.tab_cap);
        CK(hipMemcpyAsync(sp.h_res, sp.d_res, nb, hipMemcpyDeviceToHost, st));
        if (avcc) CK(hipMemcpyAsync(sp.h_fault, sp.d_fault, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        CK(hipStreamSynchronize(st));
        return 0;
    };
    bind();
    CK(hipMemcpyAsync(sp.d_rng, sp.h_rng, sizeof(FerSplitRange) * n, hipMemcpyHostToDevice, st));
    CK(hipEventRecord(sp.ev0, st));
    if (avcc) {
        avcc_launch(j, gx, st);
    } else {
        split_launch_plan(j, gx, st);
        split_launch_emit(j, gx, st);
    }
    CK(hipEventRecord(sp.ev1, st));
    CK(hipGetLastError());
    if (int rc = fetch()) return rc;
    float ms = 0;
    if (hipEventElapsedTime(&ms, sp.ev0, sp.ev1) == hipSuccess) sp.ms += ms;
    sp.in_bytes += in_bytes;
    const size_t units = sp.head()->units, total = (size_t)sp.head()->bytes;
    const bool more_units = units > sp.tab_cap, more_store = !dst && total > sp.store_cap - 64;
    if (more_units || more_store) {  // the plan stands (chunk functions, range bases): only the emit is repeated
        if (more_units)
            if (int rc = split_grow_table(sp, units + units / 4 + 64)) return rc;
        auto grow_store = [&](size_t bytes) -> int {
            size_t c = sp.store_cap;
            if (split_grow(&sp.d_store, &c, bytes + bytes / 4 + 4096)) {
                sp.store_cap = 0;
                return FERHIP_E_HIP;
            }
            sp.store_cap = c;
            return 0;
        };
        if (more_store)
            if (int rc = grow_store(total)) return rc;
        if (avcc && more_units) {  // the records and the chunk slots follow the table
            if (int rc = grow_units()) return rc;
            if (sp.ch_cap < avcc_slots()) {
                const size_t want = avcc_slots();
                size_t c0 = sp.d_summ ? sp.ch_cap : 0, c1 = sp.d_cin ? sp.ch_cap : 0;
                if (split_grow(&sp.d_summ, &c0, want) || split_grow(&sp.d_cin, &c1, want)) {
                    sp.ch_cap = 0;
                    return FERHIP_E_HIP;
                }
                sp.ch_cap = want;
            }
        }
        bind();
        if (avcc) {
            avcc_launch(j, gx, st);  // the whole job: it is a handful of small launches
        } else {
            hipLaunchKernelGGL(k_split_index, dim3(1), dim3(64), 0, st, j);  // a new table has no totals yet
            split_launch_emit(j, gx, st);
        }
        CK(hipGetLastError());
        if (int rc = fetch()) return rc;
        // length-prefixed: the first total covered the units of the old table only, so the store is looked at once more
        if (avcc && more_units && !dst && (size_t)sp.head()->bytes > sp.store_cap - 64) {
            if (int rc = grow_store((size_t)sp.head()->bytes)) return rc;
            bind();
            avcc_launch(j, gx, st);
            CK(hipGetLastError());
            if (int rc = fetch()) return rc;
        }
    }
    return 0;
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
    std::vector<uint8_t *> alloc(n, nullptr);
    std::vector<const uint8_t *> ptrs(n, nullptr);
    std::vector<size_t> ln(n, 0);
    uint8_t *dst = nullptr;
    FerSplit sp;
    auto body = [&]() -> int {
        for (size_t i = 0; i < n; i++) {
            if (!lens[i]) continue;
            CK(hipMalloc((void **)&alloc[i], (size_t)misalign + lens[i]));
            CK(hipMemcpy(alloc[i] + misalign, ranges + i * stride, lens[i], hipMemcpyHostToDevice));
            ptrs[i] = alloc[i] + misalign;
            ln[i] = lens[i];
        }
        CK(hipMalloc((void **)&dst, std::max<size_t>(cap, 16)));
        if (cap) CK(hipMemcpy(dst, out, cap, hipMemcpyHostToDevice));
        if (int rc = fer_split_run(sp, nullptr, ptrs.data(), ln.data(), (int)n, dst, cap, length_size)) return rc;
        if (cap) CK(hipMemcpy(out, dst, cap, hipMemcpyDeviceToHost));
        return 0;
    };
    int rc = body();
    if (!rc) {
        // the empty-payload cut of split_stream: a unit without payload ends its range
        const ferhip_nal_unit *t = sp.table();
        const size_t nt = sp.head()->units;
        size_t k = 0;
        uint32_t cut = ~0u;
        for (size_t i = 0; i < nt; i++) {
            if (t[i].range == cut) continue;
            if (t[i].bytes == 0) {
                cut = t[i].range;
                continue;
            }
            if (k < units_cap) units[k] = t[i];
            k++;
        }
        *nunits = k;
        if (range_fault)
            for (size_t i = 0; i < n; i++) range_fault[i] = length_size ? sp.h_fault[i] : 0;
        if (k > units_cap || (size_t)sp.head()->bytes > cap) rc = FERHIP_E_ARG;
    }
    for (uint8_t *p : alloc)
        if (p) hipFree(p);
    if (dst) hipFree(dst);
    fer_split_free(sp);
    return rc;
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
