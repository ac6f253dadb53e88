// fer_nalpack.hip -- Annex-B framing of the coded pictures on the device (ferhip_pack_nal, ferhip_fetch_nal,
// ferhip_frame_nal_blocks): start code, header byte and emulation prevention of writeNAL (F/nal.cpp:261-299) for many
// payloads at once, written 16-byte aligned into one buffer with an index of (offset, bytes, NAL type).
//
// writeNAL's counter takes the values 0, 1 and 2 only and an insertion resets it, so a run of payload bytes is a function
// on three states: for each incoming counter value, how many 03 bytes it inserts and which value it leaves.  These
// functions compose, and composition is associative: a scan.  In closed form, inside a maximal zero run z_0 .. z_{L-1} that
// starts from counter 0 an 03 goes before z_k exactly when k >= 2 and k is even, and before the non-zero byte b that ends
// it exactly when b <= 3, L >= 2 and L is even; tests/nal_model.py states that form and is pinned to the byte loop.
//
//   k_nal_count  grid (chunk, payload): a lane takes 16 payload bytes (masked past the payload's length) and reduces them
//                to their function; the 256 lanes of a workgroup compose theirs in order (wavefront scan by shuffles, the
//                four wavefronts through LDS); one function per 4096-byte chunk goes to HBM.
//   k_nal_plan   one wavefront per payload composes the chunk functions in order into each chunk's incoming counter and
//                the number of 03 bytes in front of it, and the size of the payload's entry.
//   k_nal_index  one wavefront: the exclusive sum over the payloads of the 16-rounded entry sizes = the index.
//   k_nal_emit   grid (chunk, payload): every lane recomputes its function, the same scan gives its incoming counter and
//                output position, the bytes and the inserted 03s are placed in output order in LDS, and the chunk's
//                output span is stored with 16-byte stores; the ragged bytes at its two ends share a 16-byte word with the
//                neighbouring chunk and are stored byte-wise.  Chunk 0 also places the parameter sets (where asked for),
//                the start code and the header byte.  An entry is written only if its 16-byte slots end within `cap`.
// No workgroup waits for another one: the phases are separate launches on one stream.
#include "../../include/ferhip.h"
#include "fer_internal.h"

#define NAL_THREADS 256
#define NAL_CHUNK (NAL_THREADS * 16)
// LDS image of one chunk's output: up to 15 bytes of misalignment, the parameter sets, five prefix bytes, the chunk and
// one 03 for every two of its bytes (+ 1 when the incoming counter is 2), rounded up to 16
#define NAL_IMG ((15 + FER_NAL_PS_ROW + 5 + NAL_CHUNK + NAL_CHUNK / 2 + 1 + 15) & ~15)

// A function on the counter's three states as a uint4: x, y, z = the 03 bytes inserted from incoming counter 0, 1, 2;
// w = the outgoing counters, two bits each.
__device__ __forceinline__ uint4 nal_identity() { return make_uint4(0u, 0u, 0u, 0u | 1u << 2 | 2u << 4); }
__device__ __forceinline__ uint32_t nal_cnt(const uint4 &g, uint32_t z) { return z == 0u ? g.x : (z == 1u ? g.y : g.z); }
__device__ __forceinline__ uint32_t nal_out(const uint4 &g, uint32_t z) { return (g.w >> (2u * z)) & 3u; }

// f first, then g
__device__ __forceinline__ uint4 nal_compose(const uint4 &f, const uint4 &g)
{
    const uint32_t o0 = f.w & 3u, o1 = (f.w >> 2) & 3u, o2 = (f.w >> 4) & 3u;
    uint4 r;
    r.x = f.x + nal_cnt(g, o0);
    r.y = f.y + nal_cnt(g, o1);
    r.z = f.z + nal_cnt(g, o2);
    r.w = nal_out(g, o0) | nal_out(g, o1) << 2 | nal_out(g, o2) << 4;
    return r;
}

// one byte of writeNAL's loop: returns 1 when an 03 goes in front of b
__device__ __forceinline__ uint32_t nal_step(uint32_t b, uint32_t &z)
{
    const uint32_t ins = (z >= 2u) & (b <= 3u);
    z = ins ? 0u : z;
    z = b == 0u ? z + 1u : 0u;
    return ins;
}

// the function of the first nvalid of the 16 bytes in v (memory order: byte 0 is the low byte of v.x)
__device__ __forceinline__ uint4 nal_piece(const uint4 &v, int nvalid)
{
    uint32_t z0 = 0u, z1 = 1u, z2 = 2u, c0 = 0u, c1 = 0u, c2 = 0u;
#define NAL_DWORD(w, k)                                   \
    _Pragma("unroll") for (int j = 0; j < 4; j++)         \
    {                                                     \
        if (4 * (k) + j < nvalid) {                       \
            const uint32_t b = ((w) >> (8 * j)) & 0xffu;  \
            c0 += nal_step(b, z0);                        \
            c1 += nal_step(b, z1);                        \
            c2 += nal_step(b, z2);                        \
        }                                                 \
    }
    NAL_DWORD(v.x, 0)
    NAL_DWORD(v.y, 1)
    NAL_DWORD(v.z, 2)
    NAL_DWORD(v.w, 3)
#undef NAL_DWORD
    return make_uint4(c0, c1, c2, z0 | z1 << 2 | z2 << 4);
}

__device__ __forceinline__ uint4 nal_shfl_up(const uint4 &f, int m)
{
    return make_uint4(__shfl_up(f.x, m), __shfl_up(f.y, m), __shfl_up(f.z, m), __shfl_up(f.w, m));
}

// inclusive scan over the wavefront, lane order
__device__ __forceinline__ uint4 nal_wave_scan(uint4 f, int lane)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint4 t = nal_shfl_up(f, m);
        if (lane >= m) f = nal_compose(t, f);
    }
    return f;
}

// length of payload s; never more than its slot holds (a picture that overflowed its RBSP buffer has FER_ERR bit 2 set and
// a length beyond the slot)
__device__ __forceinline__ uint32_t nal_len(const FerNalJob &j, int s) { return min(j.lens[s], (uint32_t)j.src_stride); }

// the 16 bytes of lane tid of chunk `chunk` of payload s, and how many of them belong to the payload
__device__ __forceinline__ uint4 nal_load(const FerNalJob &j, int s, uint32_t len, uint32_t chunk, int tid, int &nvalid)
{
    const uint32_t pos = chunk * NAL_CHUNK + (uint32_t)tid * 16u;
    nvalid = pos < len ? (int)min(16u, len - pos) : 0;
    // a word that starts inside the payload ends inside its 16-byte-rounded slot; bytes past the length are masked
    return nvalid ? *(const uint4 *)(j.src + (size_t)s * j.src_stride + pos) : make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(NAL_THREADS) void k_nal_count(FerNalJob j)
{
    const int s = blockIdx.y;
    const uint32_t len = nal_len(j, s);  // 0 for a stream without a picture: its workgroups leave here
    const uint32_t nch = (len + NAL_CHUNK - 1) / NAL_CHUNK;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint4 wtot[NAL_THREADS / 64];
    for (uint32_t chunk = blockIdx.x; chunk < nch; chunk += gridDim.x) {
        int nvalid;
        const uint4 v = nal_load(j, s, len, chunk, tid, nvalid);
        const uint4 incl = nal_wave_scan(nal_piece(v, nvalid), lane);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        if (tid == 0) j.summ[(size_t)s * j.nchmax + chunk] = nal_compose(nal_compose(wtot[0], wtot[1]), nal_compose(wtot[2], wtot[3]));
        __syncthreads();
    }
}

// is payload s there, and with which NAL unit type: an encoder context tells both by the device's own slice headers
__device__ __forceinline__ bool nal_present(const FerNalJob &j, int s, uint32_t len, int &type)
{
    if (j.hdr) {
        const uint32_t t = j.hdr[s * 4 + 3];
        type = t == 2u ? FERHIP_NAL_IDR : FERHIP_NAL_SLICE;
        return t != FER_PIC_ABSENT && len != 0u;
    }
    type = j.types[s] & 31;
    return true;
}

__global__ __launch_bounds__(64) void k_nal_plan(FerNalJob j)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const uint32_t len = nal_len(j, s);
    int type;
    if (!nal_present(j, s, len, type)) {
        if (lane == 0) j.ent[s] = make_uint2(0u, 0u);
        return;
    }
    const uint32_t nch = (len + NAL_CHUNK - 1) / NAL_CHUNK;
    uint32_t z = 0u, base = 0u;  // the counter and the 03 bytes in front of the block of 64 chunks
    for (uint32_t i0 = 0; i0 < nch; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint4 f = i < nch ? j.summ[(size_t)s * j.nchmax + i] : nal_identity();
        const uint4 incl = nal_wave_scan(f, lane);
        uint4 excl = nal_shfl_up(incl, 1);
        if (lane == 0) excl = nal_identity();
        if (i < nch) j.cin[(size_t)s * j.nchmax + i] = make_uint2(nal_out(excl, z), base + nal_cnt(excl, z));
        const uint4 tot = make_uint4(__shfl(incl.x, 63), __shfl(incl.y, 63), __shfl(incl.z, 63), __shfl(incl.w, 63));
        base += nal_cnt(tot, z);
        z = nal_out(tot, z);
    }
    if (lane == 0) {
        const uint32_t ps = (j.ps && type == FERHIP_NAL_IDR) ? j.ps[(size_t)s * FER_NAL_PS_ROW + FER_NAL_PS_ROW - 1] : 0u;
        j.ent[s] = make_uint2(ps + 5u + len + base, (uint32_t)type);
    }
}

__global__ __launch_bounds__(64) void k_nal_index(FerNalJob j)
{
    const int lane = threadIdx.x;
    unsigned long long run = 0;
    uint32_t written = 0;
    for (int s0 = 0; s0 < j.n; s0 += 64) {
        const int s = s0 + lane;
        const uint2 e = s < j.n ? j.ent[s] : make_uint2(0u, 0u);
        const unsigned long long r = ((unsigned long long)e.x + 15ull) & ~15ull;
        unsigned long long incl = r;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned long long t = __shfl_up(incl, m);
            if (lane >= m) incl += t;
        }
        const unsigned long long off = run + incl - r;
        if (s < j.n) {
            ferhip_au a;
            a.offset = off;
            a.bytes = e.x;
            a.nal_type = e.x ? (int32_t)e.y : 0;
            j.index[s] = a;
        }
        written += (uint32_t)__popcll(__ballot(e.x != 0u && off + r <= j.cap));
        run += __shfl(incl, 63);
    }
    if (lane == 0) {
        ferhip_au a;
        a.offset = run;
        a.bytes = written;
        a.nal_type = 0;
        j.index[j.n] = a;
    }
}

__global__ __launch_bounds__(NAL_THREADS) void k_nal_emit(FerNalJob j)
{
    const int s = blockIdx.y;
    const ferhip_au au = j.index[s];
    // no entry, or one whose 16-byte slots do not end within cap
    if (au.bytes == 0u || au.offset + (((unsigned long long)au.bytes + 15ull) & ~15ull) > j.cap) return;
    const uint32_t len = nal_len(j, s);
    const uint32_t nch = max((len + NAL_CHUNK - 1) / NAL_CHUNK, 1u);  // an empty payload still has its five prefix bytes
    const uint32_t pslen = (j.ps && au.nal_type == FERHIP_NAL_IDR) ? j.ps[(size_t)s * FER_NAL_PS_ROW + FER_NAL_PS_ROW - 1] : 0u;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint4 wtot[NAL_THREADS / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[NAL_IMG];
    for (uint32_t chunk = blockIdx.x; chunk < nch; chunk += gridDim.x) {
        int nvalid;
        const uint4 v = nal_load(j, s, len, chunk, tid, nvalid);
        const uint4 incl = nal_wave_scan(nal_piece(v, nvalid), lane);
        if (lane == 63) wtot[wave] = incl;
        uint4 excl = nal_shfl_up(incl, 1);
        if (lane == 0) excl = nal_identity();
        // chunk 0 starts from counter 0 with nothing inserted in front of it
        const uint2 cin = chunk ? j.cin[(size_t)s * j.nchmax + chunk] : make_uint2(0u, 0u);
        __syncthreads();
        uint4 pre = nal_identity();
        for (int w = 0; w < wave; w++) pre = nal_compose(pre, wtot[w]);
        excl = nal_compose(pre, excl);
        const uint4 tot = nal_compose(nal_compose(wtot[0], wtot[1]), nal_compose(wtot[2], wtot[3]));
        // the chunk's span of the output: [a, a + n), staged in img at [sh, sh + n) so that 16-byte words line up
        const uint32_t head = chunk ? 0u : pslen + 5u;
        const unsigned long long a = au.offset + (chunk ? (unsigned long long)pslen + 5ull + (unsigned long long)chunk * NAL_CHUNK + cin.y : 0ull);
        const uint32_t sh = (uint32_t)a & 15u;
        const uint32_t nin = len > chunk * NAL_CHUNK ? min((uint32_t)NAL_CHUNK, len - chunk * NAL_CHUNK) : 0u;
        const uint32_t n = head + nin + nal_cnt(tot, cin.x);
        if (!chunk) {
            if ((uint32_t)tid < pslen) img[tid] = j.ps[(size_t)s * FER_NAL_PS_ROW + tid];
            if ((uint32_t)tid >= pslen && (uint32_t)tid < pslen + 5u) {
                const uint32_t k = (uint32_t)tid - pslen;
                img[tid] = k < 3u ? 0u : (k == 3u ? 1u : (uint8_t)(1u << 5 | ((uint32_t)au.nal_type & 31u)));
            }
        }
        {
            uint32_t z = nal_out(excl, cin.x);
            uint32_t p = sh + head + (uint32_t)tid * 16u + nal_cnt(excl, cin.x);
#define NAL_DWORD(w, k)                                    \
    _Pragma("unroll") for (int q = 0; q < 4; q++)          \
    {                                                      \
        if (4 * (k) + q < nvalid) {                        \
            const uint32_t b = ((w) >> (8 * q)) & 0xffu;   \
            if (nal_step(b, z)) img[p++] = 3;              \
            img[p++] = (uint8_t)b;                         \
        }                                                  \
    }
            NAL_DWORD(v.x, 0)
            NAL_DWORD(v.y, 1)
            NAL_DWORD(v.z, 2)
            NAL_DWORD(v.w, 3)
#undef NAL_DWORD
        }
        __syncthreads();
        uint8_t *dst = j.dst + (a - sh);  // 16-byte aligned
        const uint32_t nwords = (sh + n + 15u) >> 4;
        for (uint32_t w = tid; w < nwords; w += NAL_THREADS) {
            const uint32_t lo = w << 4, hi = lo + 16u;
            if (lo >= sh && hi <= sh + n) {
                *(uint4 *)(dst + lo) = *(const uint4 *)(img + lo);
            } else {
                for (uint32_t k = max(lo, sh); k < min(hi, sh + n); k++) dst[k] = img[k];
            }
        }
        __syncthreads();
    }
}

static unsigned nal_grid_x(const FerNalJob &j)
{
    // at most 64 workgroups per payload; one that is longer walks its chunks with that stride
    return (unsigned)(j.nchmax < 1 ? 1 : (j.nchmax > 64 ? 64 : j.nchmax));
}

// count + plan: fills j.index (device) for the payloads of j; nothing of dst is touched
void fer_launch_nal_plan(const FerNalJob &j, hipStream_t st)
{
    hipLaunchKernelGGL(k_nal_count, dim3(nal_grid_x(j), j.n), dim3(NAL_THREADS), 0, st, j);
    hipLaunchKernelGGL(k_nal_plan, dim3(j.n), dim3(64), 0, st, j);
    hipLaunchKernelGGL(k_nal_index, dim3(1), dim3(64), 0, st, j);
}

// writes every entry of j.index whose 16-byte slots end within j.cap
void fer_launch_nal_emit(const FerNalJob &j, hipStream_t st)
{
    hipLaunchKernelGGL(k_nal_emit, dim3(nal_grid_x(j), j.n), dim3(NAL_THREADS), 0, st, j);
}
