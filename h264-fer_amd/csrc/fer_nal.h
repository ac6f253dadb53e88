// fer_nal.h -- what the framings of the coded pictures share (fer_nalpack.hip: Annex-B and length-prefixed units;
// fer_rtp.hip: RTP packets; fer_ts.hip: transport stream packets): the framing job, writeNAL's counter as a function that composes (NalCompose), the function of
// 16 payload bytes (nal_piece) and their load (nal_load).  The kernels that scan it (k_nal_count, k_nal_plan) live in
// fer_nalpack.hip; fer_launch_nal_count launches them for every framing.
#pragma once
#include "fer_ctx.h"
#include "fer_scan.h"

#pragma GCC visibility push(hidden)

// One framing job: n payloads, payload s = lens[s] bytes at src + s * src_stride (16-byte
// aligned, every slot readable up to its length rounded up to 16).  hdr != null: an encoder context's slice headers say
// which payloads are there and give the NAL unit type; else types[n] does and every payload is there.  ps (optional):
// [n][FER_NAL_PS_ROW] framed SPS + PPS of every payload, the row's last byte = their length; they go in front of IDR units.
// A row of at most FER_NAL_PS_ROW - 2 bytes also records where its second prefix (the PPS's) sits, in the byte in front of
// the last one: the length-prefixed form of the row is the row itself with its two prefixes rewritten as it is placed.
#define FER_NAL_PS_ROW 64
struct FerNalJob {
    const uint8_t *src;
    size_t src_stride;
    const uint32_t *lens;
    const uint32_t *hdr;
    const int32_t *types;
    const uint8_t *ps;
    int avcc;            // the 4-byte prefix of every unit is its length (FERHIP_AU_AVCC), not the start code
    int n, nchmax;       // payloads; 4096-byte chunks a payload can have (the pitch of summ and cin)
    uint4 *summ;         // [n][nchmax] what each chunk does to writeNAL's counter (k_nal_count)
    uint2 *cin;          // [n][nchmax] each chunk's incoming counter and the 03 bytes in front of it (k_nal_plan)
    uint2 *ent;          // [n] entry size, NAL unit type
    ferhip_au *index;    // [n + 1] device
    uint8_t *dst;
    unsigned long long cap;
};

#define NAL_THREADS 256
#define NAL_CHUNK (NAL_THREADS * 16)

// A function on the counter's three states as a uint4: x, y, z = the 03 bytes inserted from incoming counter 0, 1, 2;
// w = the outgoing counters, two bits each.
__device__ __forceinline__ uint4 nal_identity() { return make_uint4(0u, 0u, 0u, 0u | 1u << 2 | 2u << 4); }
__device__ __forceinline__ uint32_t nal_cnt(const uint4 &g, uint32_t z) { return z == 0u ? g.x : (z == 1u ? g.y : g.z); }
__device__ __forceinline__ uint32_t nal_out(const uint4 &g, uint32_t z) { return (g.w >> (2u * z)) & 3u; }

// f first, then g
struct NalCompose {
    __device__ __forceinline__ uint4 operator()(const uint4 &f, const uint4 &g) const
    {
        const uint32_t o0 = f.w & 3u, o1 = (f.w >> 2) & 3u, o2 = (f.w >> 4) & 3u;
        uint4 r;
        r.x = f.x + nal_cnt(g, o0);
        r.y = f.y + nal_cnt(g, o1);
        r.z = f.z + nal_cnt(g, o2);
        r.w = nal_out(g, o0) | nal_out(g, o1) << 2 | nal_out(g, o2) << 4;
        return r;
    }
};

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

// at most 64 workgroups per payload; one that is longer walks its chunks with that stride
static inline unsigned nal_grid_x(const FerNalJob &j) { return (unsigned)(j.nchmax < 1 ? 1 : (j.nchmax > 64 ? 64 : j.nchmax)); }

// ---- host side, fer_nalpack.hip
// k_nal_count + k_nal_plan: fills j.summ, j.cin and j.ent; neither j.index nor j.dst is touched
void fer_launch_nal_count(const FerNalJob &j, hipStream_t st);
// the framing job of a context's last picture (buffers on first use; FERHIP_AU_PARAM_SETS: the parameter set table is
// brought up to date, and with FERHIP_AU_AVCC a row without its PPS position is refused); j.index, j.dst and j.cap are the caller's
int fer_nal_prepare(ferhip_ctx *c, int flags, FerNalJob &j);

#pragma GCC visibility pop
