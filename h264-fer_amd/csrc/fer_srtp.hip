// fer_srtp.hip -- SRTP (RFC 3711, AES-128 counter mode and HMAC-SHA1 with an 80-bit tag) on the device: ferhip_srtp_protect
// turns the datagrams ferhip_pack_rtp left in device memory into SRTP packets, ferhip_srtp_unprotect checks and decrypts
// received ones into the packets ferhip_decs_decode_rtp takes, ferhip_srtp_blocks is the known-answer surface of both.  The
// definition stands in include/ferhip.h, the host half (key schedule, derivation, midstates, header rule, index estimate,
// argument checks) in fer_srtp_host.h.
//
// The passes, separate launches on one stream (no workgroup waits for another one):
//   k_srtp_parse   one lane per row: the header rule (fer_srtp_header, shared with the host), seq and ssrc, and an atomicMin
//                  on first[stream], the stream's first well-formed row -- what a state with set == 0 takes s_l from.
//   k_srtp_plan    one lane per row: the index estimate against the state the call started with (nothing has written the
//                  state yet), on the way in the HMAC over the packet and v and the comparison with its tag, which gives
//                  the status; the row's output size goes into the output table.  The workgroup then sums its 256 rows'
//                  sizes rounded up to 16 (wave_scan, wg_put / wg_front / wg_total of fer_scan.h): every row gets its offset
//                  within the workgroup, and the workgroup's sum goes to bsum[].
//   k_srtp_scan    one wavefront: the exclusive sums of the workgroups' sums (carry_scan), in place, and row npkts.
//   k_srtp_place   one lane per row: the workgroup's base onto the row's offset; the packets that end within cap are
//                  counted into row npkts, one atomicAdd per wavefront.
//   k_srtp_cipher  one wavefront per packet, four to a workgroup, one lane per 16-byte keystream block.  The workgroup stages
//                  Te0 (1 KB) and the S-box (256 bytes) in LDS once; the other three round tables are rotations of Te0.  The
//                  round keys are the same for the whole wavefront (one stream), so they are loaded through the scalar unit
//                  and stay in scalar registers.  Input at any alignment: a whole block is read as the aligned dwords that
//                  cover it and shifted into place, the ragged last block byte by byte.  hl is a multiple of 4 and a packet
//                  starts on 16 in the output, so a whole block leaves as four dword stores; the last block's bytes and
//                  nothing behind them are stored byte-wise.  The header's dwords are copied by the same lanes first.
//                  Lane 0 then raises the stream's state word with a 64-bit atomicMax.
//   k_srtp_tag     (the way out only) one lane per packet: SHA-1 from the inner midstate over the packet as it now stands in
//                  the output (dword loads, it starts on 16) and v, the outer compression, ten tag bytes behind the packet.
// One lane per packet for the hash, not one wavefront: SHA-1 is a serial chain of 80 rounds per 64 bytes with nothing for
// 64 lanes to share, and a picture of 256 streams has thousands of packets.  The 80 rounds are unrolled so that the 16-word
// schedule ring is indexed by constants only and stays in registers: no kernel here uses scratch memory.
// The slot offsets are a scan in two levels because one wavefront over all rows, 64 a step, was measured at 1.6 ms for the
// 211 267 packets of an I picture of 256 1080p streams -- more than half of a protect call.
#include "fer_ctx.h"
#include "fer_scan.h"
#include "fer_srtp_host.h"
#include <string.h>
#include <algorithm>
#include <vector>

#pragma GCC visibility push(hidden)

ferhip_ctx *fer_decs_ctx(ferhip_decs *d);  // fer_decode_live.hip: the live decoder's context, for its device and stream

struct FerSrtpJob {
    const uint8_t *base;          // the packets in
    const ferhip_rtp_pkt *pkts;   // [npk] device
    uint32_t npk, S;
    int unprotect;
    const uint32_t *rows;         // [S][FER_SRTP_ROW] the session table
    unsigned long long *state;    // [S] FER_SRTP_STATE words
    const uint32_t *tab;          // [FER_SRTP_TAB]
    uint32_t *first;              // [S] the stream's first well-formed row, preset to ~0
    uint4 *rec;                   // [npk] hl (0 = not to be written), v, seq, ssrc
    unsigned long long *bsum;     // [ceil(npk / 256)] the slot bytes of every 256 rows, then what stands in front of them
    uint8_t *dst;
    unsigned long long cap;
    ferhip_rtp_pkt *out;          // [npk + 1] device
    int32_t *status;              // [npk] device, the way in only
};

__device__ __forceinline__ uint32_t srtp_rotl(uint32_t v, int n) { return v << n | v >> (32 - n); }
__device__ __forceinline__ uint32_t srtp_ror(uint32_t v, int n) { return v >> n | v << (32 - n); }

__global__ __launch_bounds__(256) void k_srtp_parse(FerSrtpJob j)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= j.npk) return;
    const ferhip_rtp_pkt row = j.pkts[k];
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (row.stream < j.S && j.rows[(size_t)row.stream * FER_SRTP_ROW + FER_SRTP_ROW_KEYED]) {
        const uint32_t L = j.unprotect ? (row.bytes >= FER_SRTP_TAG ? row.bytes - FER_SRTP_TAG : 0u) : row.bytes;
        const uint8_t *p = j.base + row.offset;
        const uint32_t hl = fer_srtp_header(p, L);
        if (hl) {
            r.x = hl;
            r.z = (uint32_t)p[2] << 8 | p[3];
            r.w = (uint32_t)p[8] << 24 | (uint32_t)p[9] << 16 | (uint32_t)p[10] << 8 | p[11];
            atomicMin(&j.first[row.stream], k);
        }
    }
    j.rec[k] = r;
}

// ---- SHA-1, 80 rounds unrolled over a ring of 16 words that only constants index
#define SRTP_SHA_ROUND(t, f, kk)                                                                                   \
    {                                                                                                              \
        uint32_t wt;                                                                                               \
        if ((t) < 16)                                                                                              \
            wt = w[(t) & 15];                                                                                      \
        else                                                                                                       \
            wt = w[(t) & 15] = srtp_rotl(w[((t) + 13) & 15] ^ w[((t) + 8) & 15] ^ w[((t) + 2) & 15] ^ w[(t) & 15], 1); \
        const uint32_t x = srtp_rotl(a, 5) + (f) + e + (kk) + wt;                                                  \
        e = d, d = c, c = srtp_rotl(b, 30), b = a, a = x;                                                          \
    }
__device__ __forceinline__ void srtp_sha1_compress(uint32_t (&h)[5], uint32_t (&w)[16])
{
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
    for (int t = 0; t < 20; t++) SRTP_SHA_ROUND(t, (b & c) | (~b & d), 0x5A827999u)
#pragma unroll
    for (int t = 20; t < 40; t++) SRTP_SHA_ROUND(t, b ^ c ^ d, 0x6ED9EBA1u)
#pragma unroll
    for (int t = 40; t < 60; t++) SRTP_SHA_ROUND(t, (b & c) | (b & d) | (c & d), 0x8F1BBCDCu)
#pragma unroll
    for (int t = 60; t < 80; t++) SRTP_SHA_ROUND(t, b ^ c ^ d, 0xCA62C1D6u)
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e;
}
#undef SRTP_SHA_ROUND

// The big-endian word at byte `off` (a multiple of 4) of the padded message p[0, L) || v || 80 00 ..; ALIGNED: p is a
// multiple of 4.  Reads inside [p, p + L) only.
template <bool ALIGNED>
__device__ __forceinline__ uint32_t srtp_msg_word(const uint8_t *p, uint32_t L, uint32_t v, uint32_t off)
{
    if (off + 4u <= L) {
        if (ALIGNED) return __builtin_bswap32(*(const uint32_t *)(p + off));
        return (uint32_t)p[off] << 24 | (uint32_t)p[off + 1u] << 16 | (uint32_t)p[off + 2u] << 8 | p[off + 3u];
    }
    uint32_t w = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
        const uint32_t o = off + i;
        const uint32_t b = o < L ? p[o] : o < L + 4u ? (v >> (8u * (3u - (o - L)))) & 255u : o == L + 4u ? 0x80u : 0u;
        w = w << 8 | b;
    }
    return w;
}

// HMAC-SHA1 from the row's two midstates over p[0, L) || v: the first 80 bits as t0, t1 and the upper half of t2
template <bool ALIGNED>
__device__ __forceinline__ void srtp_hmac(const uint32_t *row, const uint8_t *p, uint32_t L, uint32_t v, uint32_t &t0, uint32_t &t1, uint32_t &t2)
{
    uint32_t h[5], w[16];
#pragma unroll
    for (int i = 0; i < 5; i++) h[i] = row[FER_SRTP_ROW_MID_I + i];
    const uint32_t n = L + 4u, nblk = (n + 9u + 63u) >> 6;
    for (uint32_t blk = 0; blk < nblk; blk++) {
#pragma unroll
        for (int q = 0; q < 16; q++) w[q] = srtp_msg_word<ALIGNED>(p, L, v, blk * 64u + 4u * (uint32_t)q);
        if (blk == nblk - 1u) w[15] = (64u + n) * 8u;  // the length in bits, the key block included; its upper word is 0
        srtp_sha1_compress(h, w);
    }
#pragma unroll
    for (int i = 0; i < 5; i++) w[i] = h[i];
    w[5] = 0x80000000u;
#pragma unroll
    for (int i = 6; i < 15; i++) w[i] = 0u;
    w[15] = (64u + 20u) * 8u;
#pragma unroll
    for (int i = 0; i < 5; i++) h[i] = row[FER_SRTP_ROW_MID_O + i];
    srtp_sha1_compress(h, w);
    t0 = h[0], t1 = h[1], t2 = h[2];
}

__device__ __forceinline__ uint32_t srtp_tag_byte(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t i)
{
    const uint32_t w = i < 4u ? t0 : i < 8u ? t1 : t2;
    return (w >> (8u * (3u - (i & 3u)))) & 255u;
}

__global__ __launch_bounds__(256) void k_srtp_plan(FerSrtpJob j)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const bool there = k < j.npk;  // every lane stays for the workgroup's sum
    uint4 r = there ? j.rec[k] : make_uint4(0u, 0u, 0u, 0u);
    ferhip_rtp_pkt row;
    row.offset = 0ull, row.bytes = 0u, row.stream = 0u;
    if (there) row = j.pkts[k];
    uint32_t bytes = 0u;
    int32_t status = 2;
    if (r.x) {
        const unsigned long long st = j.state[row.stream];
        const uint32_t roc = (uint32_t)(st >> 16);
        const uint32_t s_l = (st >> 48) & 1ull ? (uint32_t)st & 0xffffu : j.rec[j.first[row.stream]].z;
        r.y = fer_srtp_estimate(roc, s_l, r.z);
        if (!j.unprotect) {
            bytes = row.bytes + FER_SRTP_TAG;
            status = 0;
        } else {
            const uint8_t *p = j.base + row.offset;
            const uint32_t L = row.bytes - FER_SRTP_TAG;
            uint32_t t0, t1, t2;
            srtp_hmac<false>(j.rows + (size_t)row.stream * FER_SRTP_ROW, p, L, r.y, t0, t1, t2);
            uint32_t diff = 0u;
            for (uint32_t i = 0; i < FER_SRTP_TAG; i++) diff |= srtp_tag_byte(t0, t1, t2, i) ^ p[L + i];
            status = diff ? 1 : 0;
            if (diff)
                r.x = 0u;  // nothing of it is decrypted, and the state does not see it
            else
                bytes = L;
        }
        j.rec[k] = r;
    }
    // the slot's offset within the workgroup's 256 rows, and the workgroup's sum for k_srtp_scan
    __shared__ unsigned long long wtot[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long slot = (bytes + 15u) & ~15u;
    const unsigned long long incl = wave_scan(slot, lane, ScanAdd());
    wg_put(wtot, incl, wave, lane);
    __syncthreads();
    if (threadIdx.x == 0) j.bsum[blockIdx.x] = wg_total(wtot, ScanAdd());
    if (!there) return;
    ferhip_rtp_pkt o;
    o.offset = wg_front(wtot, wave, 0ull, ScanAdd()) + incl - slot;
    o.bytes = bytes;
    o.stream = row.stream;
    j.out[k] = o;
    if (j.status) j.status[k] = status;
}

// one wavefront over the workgroups' sums: every workgroup's base in place of its sum, and row npkts with no packet counted yet
__global__ __launch_bounds__(64) void k_srtp_scan(FerSrtpJob j)
{
    const int lane = threadIdx.x;
    unsigned long long *bsum = j.bsum;
    const unsigned long long total = carry_scan(
        (j.npk + 255u) >> 8, lane, 0ull, ScanAdd(), [&](uint32_t i) { return bsum[i]; }, [&](uint32_t i, unsigned long long base) { bsum[i] = base; });
    if (lane == 0) {
        ferhip_rtp_pkt o;
        o.offset = total;
        o.bytes = 0u;
        o.stream = 0u;
        j.out[j.npk] = o;
    }
}

// one lane per row: the workgroup's base onto the slot's offset; the packets that end within cap are counted into row npkts,
// one atomic per wavefront
__global__ __launch_bounds__(256) void k_srtp_place(FerSrtpJob j)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    bool fits = false;
    if (k < j.npk) {
        const unsigned long long off = j.out[k].offset + j.bsum[blockIdx.x];
        const uint32_t bytes = j.out[k].bytes;
        j.out[k].offset = off;
        fits = bytes != 0u && off + bytes <= j.cap;
    }
    const uint32_t n = (uint32_t)__popcll(__ballot(fits));
    if ((threadIdx.x & 63u) == 0u && n) atomicAdd(&j.out[j.npk].bytes, n);
}

// ---- AES-128: Te0 and the S-box in LDS, the round keys in registers
#define SRTP_TE(x, n) srtp_ror(te[(x)], n)
#define SRTP_AES_ROUND(r)                                                                                                             \
    {                                                                                                                                 \
        const uint32_t u0 = te[s0 >> 24] ^ SRTP_TE((s1 >> 16) & 255u, 8) ^ SRTP_TE((s2 >> 8) & 255u, 16) ^ SRTP_TE(s3 & 255u, 24) ^ rk[4 * (r)];     \
        const uint32_t u1 = te[s1 >> 24] ^ SRTP_TE((s2 >> 16) & 255u, 8) ^ SRTP_TE((s3 >> 8) & 255u, 16) ^ SRTP_TE(s0 & 255u, 24) ^ rk[4 * (r) + 1]; \
        const uint32_t u2 = te[s2 >> 24] ^ SRTP_TE((s3 >> 16) & 255u, 8) ^ SRTP_TE((s0 >> 8) & 255u, 16) ^ SRTP_TE(s1 & 255u, 24) ^ rk[4 * (r) + 2]; \
        const uint32_t u3 = te[s3 >> 24] ^ SRTP_TE((s0 >> 16) & 255u, 8) ^ SRTP_TE((s1 >> 8) & 255u, 16) ^ SRTP_TE(s2 & 255u, 24) ^ rk[4 * (r) + 3]; \
        s0 = u0, s1 = u1, s2 = u2, s3 = u3;                                                                                           \
    }
#define SRTP_SB(x) ((uint32_t)sb[(x)])
__device__ __forceinline__ void srtp_aes(const uint32_t *te, const uint8_t *sb, const uint32_t (&rk)[44], uint32_t &s0, uint32_t &s1, uint32_t &s2,
                                         uint32_t &s3)
{
    s0 ^= rk[0], s1 ^= rk[1], s2 ^= rk[2], s3 ^= rk[3];
#pragma unroll
    for (int r = 1; r < 10; r++) SRTP_AES_ROUND(r)
    const uint32_t u0 = (SRTP_SB(s0 >> 24) << 24 | SRTP_SB((s1 >> 16) & 255u) << 16 | SRTP_SB((s2 >> 8) & 255u) << 8 | SRTP_SB(s3 & 255u)) ^ rk[40];
    const uint32_t u1 = (SRTP_SB(s1 >> 24) << 24 | SRTP_SB((s2 >> 16) & 255u) << 16 | SRTP_SB((s3 >> 8) & 255u) << 8 | SRTP_SB(s0 & 255u)) ^ rk[41];
    const uint32_t u2 = (SRTP_SB(s2 >> 24) << 24 | SRTP_SB((s3 >> 16) & 255u) << 16 | SRTP_SB((s0 >> 8) & 255u) << 8 | SRTP_SB(s1 & 255u)) ^ rk[42];
    const uint32_t u3 = (SRTP_SB(s3 >> 24) << 24 | SRTP_SB((s0 >> 16) & 255u) << 16 | SRTP_SB((s1 >> 8) & 255u) << 8 | SRTP_SB(s2 & 255u)) ^ rk[43];
    s0 = u0, s1 = u1, s2 = u2, s3 = u3;
}
#undef SRTP_SB
#undef SRTP_AES_ROUND
#undef SRTP_TE

__device__ __forceinline__ uint32_t srtp_load_le32(const uint8_t *p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

__global__ __launch_bounds__(256) void k_srtp_cipher(FerSrtpJob j)
{
    __shared__ uint32_t te[256];
    __shared__ __attribute__((aligned(4))) uint8_t sb[256];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    te[tid] = j.tab[tid];
    if (tid < 64u) ((uint32_t *)sb)[tid] = j.tab[256u + tid];
    __syncthreads();
    const uint32_t k = blockIdx.x * 4u + wave;
    if (k >= j.npk) return;
    const uint4 r = j.rec[k];
    if (!r.x) return;
    const ferhip_rtp_pkt o = j.out[k];
    const uint32_t stream = o.stream;
    if (o.offset + o.bytes <= j.cap) {
        const uint32_t hl = r.x, L = j.unprotect ? o.bytes : o.bytes - FER_SRTP_TAG;  // the packet without a tag
        const uint8_t *src = j.base + j.pkts[k].offset;
        uint8_t *dst = j.dst + o.offset;
        for (uint32_t i = lane; i < hl >> 2; i += 64u) ((uint32_t *)dst)[i] = srtp_load_le32(src + 4u * i);
        const uint32_t *row = j.rows + (size_t)stream * FER_SRTP_ROW;
        uint32_t rk[44];
#pragma unroll
        for (int i = 0; i < 44; i++) rk[i] = row[i];
        const uint32_t iv0 = row[FER_SRTP_ROW_KS], iv1 = row[FER_SRTP_ROW_KS + 1] ^ r.w, iv2 = row[FER_SRTP_ROW_KS + 2] ^ r.y,
                       iv3 = row[FER_SRTP_ROW_KS + 3] ^ (r.z << 16);
        const uint32_t nblk = (L - hl + 15u) >> 4;
        for (uint32_t b = lane; b < nblk; b += 64u) {
            uint32_t s0 = iv0, s1 = iv1, s2 = iv2, s3 = iv3 | b;  // the IV's last two bytes are 0 and b < 65536
            srtp_aes(te, sb, rk, s0, s1, s2, s3);
            const uint32_t pos = hl + 16u * b;
            const uint8_t *sp = src + pos;
            if (pos + 16u <= L) {
                const uint32_t sh = ((uint32_t)(uintptr_t)sp & 3u) * 8u;
                const uint32_t *a = (const uint32_t *)((uintptr_t)sp & ~(uintptr_t)3);
                uint32_t x0 = a[0], x1 = a[1], x2 = a[2], x3 = a[3];
                if (sh) {  // the fifth dword holds the block's last bytes only then
                    const uint32_t x4 = a[4];
                    x0 = x0 >> sh | x1 << (32u - sh);
                    x1 = x1 >> sh | x2 << (32u - sh);
                    x2 = x2 >> sh | x3 << (32u - sh);
                    x3 = x3 >> sh | x4 << (32u - sh);
                }
                uint32_t *dp = (uint32_t *)(dst + pos);
                dp[0] = x0 ^ __builtin_bswap32(s0);
                dp[1] = x1 ^ __builtin_bswap32(s1);
                dp[2] = x2 ^ __builtin_bswap32(s2);
                dp[3] = x3 ^ __builtin_bswap32(s3);
            } else {
                for (uint32_t i = 0; pos + i < L; i++) {
                    const uint32_t w = i < 4u ? s0 : i < 8u ? s1 : i < 12u ? s2 : s3;
                    dst[pos + i] = (uint8_t)(sp[i] ^ (w >> (8u * (3u - (i & 3u)))));
                }
            }
        }
    }
    if (lane == 0u) atomicMax(&j.state[stream], FER_SRTP_STATE(1, r.y, r.z));
}

__global__ __launch_bounds__(256) void k_srtp_tag(FerSrtpJob j)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= j.npk) return;
    const uint4 r = j.rec[k];
    const ferhip_rtp_pkt o = j.out[k];
    if (!r.x || o.offset + o.bytes > j.cap) return;
    uint8_t *p = j.dst + o.offset;
    const uint32_t L = o.bytes - FER_SRTP_TAG;
    uint32_t t0, t1, t2;
    srtp_hmac<true>(j.rows + (size_t)o.stream * FER_SRTP_ROW, p, L, r.y, t0, t1, t2);
    for (uint32_t i = 0; i < FER_SRTP_TAG; i++) p[L + i] = (uint8_t)srtp_tag_byte(t0, t1, t2, i);
}

// ---- host side
#define FER_SRTP_SLOTS 4
struct SrtpCore {  // what a session and a ferhip_srtp_blocks call own on the device
    int S = 0;
    DevBuf<uint32_t> d_rows, d_tab, d_first;
    DevBuf<unsigned long long> d_state, d_bsum;
    DevBuf<uint4> d_rec;
    std::vector<uint8_t> keyed;
    int create(int nstreams, const uint32_t *tab)
    {
        S = nstreams;
        keyed.assign((size_t)S, 0);
        if (d_rows.reserve((size_t)S * FER_SRTP_ROW) || d_tab.reserve(FER_SRTP_TAB) || d_first.reserve((size_t)S) || d_state.reserve((size_t)S))
            return FERHIP_E_HIP;
        CK(hipMemset(d_rows, 0, (size_t)S * FER_SRTP_ROW * sizeof(uint32_t)));
        CK(hipMemset(d_state, 0, (size_t)S * sizeof(unsigned long long)));
        CK(hipMemcpy(d_tab, tab, FER_SRTP_TAB * sizeof(uint32_t), hipMemcpyHostToDevice));
        return 0;
    }
};

static const uint32_t *srtp_tables()
{
    static const struct Tab {
        uint32_t w[FER_SRTP_TAB];
        Tab() { fer_aes_tables(w); }
    } t;
    return t.w;
}

// the passes of one call on stream st; d_status = null: the way out
static int srtp_launch(SrtpCore &c, hipStream_t st, const uint8_t *d_base, const ferhip_rtp_pkt *d_pkts, size_t npk, uint8_t *d_dst, size_t cap,
                       ferhip_rtp_pkt *d_out, int32_t *d_status, bool unprotect)
{
    if (c.d_rec.reserve(npk, npk + npk / 4 + 256) || c.d_bsum.reserve(npk / 256 + 1, npk / 200 + 64)) return FERHIP_E_HIP;
    FerSrtpJob j;
    j.base = d_base;
    j.pkts = d_pkts;
    j.npk = (uint32_t)npk;
    j.S = (uint32_t)c.S;
    j.unprotect = unprotect ? 1 : 0;
    j.rows = c.d_rows;
    j.state = c.d_state;
    j.tab = c.d_tab;
    j.first = c.d_first;
    j.rec = c.d_rec;
    j.bsum = c.d_bsum;
    j.dst = d_dst;
    j.cap = cap;
    j.out = d_out;
    j.status = d_status;
    const unsigned g256 = (unsigned)((npk + 255) / 256);
    if (npk) {
        CK(hipMemsetAsync(c.d_first, 0xff, (size_t)c.S * sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_srtp_parse, dim3(g256), dim3(256), 0, st, j);
        hipLaunchKernelGGL(k_srtp_plan, dim3(g256), dim3(256), 0, st, j);
    }
    hipLaunchKernelGGL(k_srtp_scan, dim3(1), dim3(64), 0, st, j);
    if (npk) {
        hipLaunchKernelGGL(k_srtp_place, dim3(g256), dim3(256), 0, st, j);
        hipLaunchKernelGGL(k_srtp_cipher, dim3((unsigned)((npk + 3) / 4)), dim3(256), 0, st, j);
        if (!unprotect) hipLaunchKernelGGL(k_srtp_tag, dim3(g256), dim3(256), 0, st, j);
    }
    CK(hipGetLastError());
    return 0;
}

#pragma GCC visibility pop

struct ferhip_srtp {
    SrtpCore core;
    int device = 0;
    // a host table on its way to the device: pinned slots, each rewritten only after the copy that last used it has run
    PinBuf<ferhip_rtp_pkt> h_slot[FER_SRTP_SLOTS];
    hipEvent_t ev[FER_SRTP_SLOTS] = {};
    int slot = 0;
    DevBuf<ferhip_rtp_pkt> d_pkts;   // the table in
    DevBuf<ferhip_rtp_pkt> d_out;    // ferhip_srtp_unprotect: the table out ...
    DevBuf<int32_t> d_status;        // ... and the status, and what the host reads of both
    PinBuf<ferhip_rtp_pkt> h_out;
    PinBuf<int32_t> h_status;
    DevBuf<uint8_t> d_stage;         // ferhip_srtp_unprotect(base_on_device = 0): the packets, copied up once
};

static_assert(sizeof(FerSrtpRow) == sizeof(ferhip_rtp_pkt) && sizeof(ferhip_srtp_key) == 32 && sizeof(ferhip_srtp_index) == 8, "ABI");

extern "C" int ferhip_srtp_derive(const uint8_t *master_key, const uint8_t *master_salt, uint8_t *out)
{
    if (!master_key || !master_salt || !out) return FERHIP_E_ARG;
    fer_srtp_derive(srtp_tables(), master_key, master_salt, out);
    return 0;
}

extern "C" int ferhip_srtp_create(ferhip_srtp **out, int nstreams)
{
    if (!out) return FERHIP_E_ARG;
    *out = nullptr;
    if (nstreams <= 0 || nstreams > 65535) return FERHIP_E_ARG;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        fprintf(stderr, "ferhip: no HIP device; SRTP has no CPU fallback\n");
        return FERHIP_E_HIP;
    }
    ferhip_srtp *h = new ferhip_srtp();
    h->device = dev;
    int rc = h->core.create(nstreams, srtp_tables());
    for (int i = 0; i < FER_SRTP_SLOTS && !rc; i++)
        if (hipEventCreateWithFlags(&h->ev[i], hipEventDisableTiming) != hipSuccess) rc = FERHIP_E_HIP;
    if (rc) {
        (void)hipGetLastError();
        ferhip_srtp_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" void ferhip_srtp_destroy(ferhip_srtp *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;  // the buffers go with it, on the device selected above
}

extern "C" int ferhip_srtp_set_key(ferhip_srtp *h, int s, const uint8_t *master_key, const uint8_t *master_salt)
{
    if (!h || s < 0 || s >= h->core.S || !master_key || !master_salt) return FERHIP_E_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FERHIP_E_HIP;
    uint32_t row[FER_SRTP_ROW];
    fer_srtp_row(srtp_tables(), master_key, master_salt, row);
    const unsigned long long zero = 0ull;
    CK(hipDeviceSynchronize());  // a call in flight keeps the key it started with
    CK(hipMemcpy(h->core.d_rows + (size_t)s * FER_SRTP_ROW, row, sizeof row, hipMemcpyHostToDevice));
    CK(hipMemcpy(h->core.d_state + s, &zero, sizeof zero, hipMemcpyHostToDevice));
    h->core.keyed[s] = 1;
    return 0;
}

extern "C" int ferhip_srtp_get_index(ferhip_srtp *h, int s, uint32_t *roc, uint32_t *s_l, int *set)
{
    if (!h || s < 0 || s >= h->core.S || !roc || !s_l || !set) return FERHIP_E_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FERHIP_E_HIP;
    unsigned long long w = 0;
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(&w, h->core.d_state + s, sizeof w, hipMemcpyDeviceToHost));
    *roc = (uint32_t)(w >> 16);
    *s_l = (uint32_t)w & 0xffffu;
    *set = (int)((w >> 48) & 1ull);
    return 0;
}

extern "C" int ferhip_srtp_set_index(ferhip_srtp *h, int s, uint32_t roc, uint32_t s_l, int set)
{
    if (!h || s < 0 || s >= h->core.S || s_l > 65535u || (set != 0 && set != 1)) return FERHIP_E_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FERHIP_E_HIP;
    const unsigned long long w = FER_SRTP_STATE(set, roc, s_l);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h->core.d_state + s, &w, sizeof w, hipMemcpyHostToDevice));
    return 0;
}

// the caller's table -> the device through the next pinned slot, offsets less `rebase`
static int srtp_send_table(ferhip_srtp *h, hipStream_t st, const ferhip_rtp_pkt *pkts, size_t npk, uint64_t rebase)
{
    if (!npk) return 0;
    const int i = h->slot;
    h->slot = (i + 1) % FER_SRTP_SLOTS;
    CK(hipEventSynchronize(h->ev[i]));
    if (h->h_slot[i].reserve(npk, npk + npk / 4 + 256) || h->d_pkts.reserve(npk, npk + npk / 4 + 256)) return FERHIP_E_HIP;
    ferhip_rtp_pkt *w = h->h_slot[i];
    for (size_t k = 0; k < npk; k++) {
        w[k] = pkts[k];
        w[k].offset -= rebase;
    }
    CK(hipMemcpyAsync(h->d_pkts, w, npk * sizeof(ferhip_rtp_pkt), hipMemcpyHostToDevice, st));
    CK(hipEventRecord(h->ev[i], st));
    return 0;
}

static int srtp_protect_args(ferhip_srtp *h, ferhip_ctx *c, const void *d_src, const void *pkts, size_t npkts, void *d_dst, size_t cap, void *d_out_pkts)
{
    if (!h || !c || c->device != h->device || (npkts && (!d_src || !pkts)) || npkts > 0x7fffffffu) return FERHIP_E_ARG;
    return fer_srtp_check_out(d_dst, cap, d_out_pkts, 16, 8);
}

extern "C" int ferhip_srtp_protect(ferhip_srtp *h, ferhip_ctx *c, const void *d_src, const ferhip_rtp_pkt *src_pkts, size_t npkts, void *d_dst,
                                   size_t cap, ferhip_rtp_pkt *d_out_pkts)
{
    if (int rc = srtp_protect_args(h, c, d_src, src_pkts, npkts, d_dst, cap, d_out_pkts)) return rc;
    if (int rc = fer_srtp_check_rows((const FerSrtpRow *)src_pkts, npkts, (size_t)h->core.S, h->core.keyed.data(), ~0ull)) return rc;
    if (hipSetDevice(h->device) != hipSuccess) return FERHIP_E_HIP;
    if (int rc = srtp_send_table(h, c->st, src_pkts, npkts, 0)) return rc;
    return srtp_launch(h->core, c->st, (const uint8_t *)d_src, h->d_pkts, npkts, (uint8_t *)d_dst, cap, d_out_pkts, nullptr, false);
}

extern "C" int ferhip_srtp_protect_dev(ferhip_srtp *h, ferhip_ctx *c, const void *d_src, const ferhip_rtp_pkt *d_src_pkts, size_t npkts,
                                       void *d_dst, size_t cap, ferhip_rtp_pkt *d_out_pkts)
{
    if (int rc = srtp_protect_args(h, c, d_src, d_src_pkts, npkts, d_dst, cap, d_out_pkts)) return rc;
    if ((uintptr_t)d_src_pkts & 7) return FERHIP_E_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FERHIP_E_HIP;
    return srtp_launch(h->core, c->st, (const uint8_t *)d_src, d_src_pkts, npkts, (uint8_t *)d_dst, cap, d_out_pkts, nullptr, false);
}

extern "C" int ferhip_srtp_unprotect(ferhip_srtp *h, ferhip_decs *d, const void *base, int base_on_device, const ferhip_rtp_pkt *pkts, size_t npkts,
                                     void *d_dst, size_t cap, ferhip_rtp_pkt *h_out_pkts, int32_t *h_status)
{
    if (!h || !d || (npkts && (!base || !pkts || !h_status)) || npkts > 0x7fffffffu || (base_on_device != 0 && base_on_device != 1))
        return FERHIP_E_ARG;
    if (int rc = fer_srtp_check_out(d_dst, cap, h_out_pkts, 16, 1)) return rc;
    if (int rc = fer_srtp_check_rows((const FerSrtpRow *)pkts, npkts, (size_t)h->core.S, h->core.keyed.data(), ~0ull)) return rc;
    ferhip_ctx *c = fer_decs_ctx(d);
    if (c->device != h->device) return FERHIP_E_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FERHIP_E_HIP;
    const uint8_t *d_base = (const uint8_t *)base;
    uint64_t lo = 0;
    if (!base_on_device && npkts) {  // one staging copy of the range the rows span
        uint64_t hi = 0;
        lo = ~0ull;
        for (size_t k = 0; k < npkts; k++) {
            lo = std::min<uint64_t>(lo, pkts[k].offset);
            hi = std::max<uint64_t>(hi, pkts[k].offset + pkts[k].bytes);
        }
        const size_t n = (size_t)(hi - lo);
        if (h->d_stage.reserve(n + 16, n + n / 4 + 4096)) return FERHIP_E_HIP;  // the cipher pass reads whole dwords
        if (n) CK(hipMemcpyAsync(h->d_stage, (const uint8_t *)base + lo, n, hipMemcpyHostToDevice, c->st));
        d_base = h->d_stage;
    }
    if (int rc = srtp_send_table(h, c->st, pkts, npkts, lo)) return rc;
    if (h->d_out.reserve(npkts + 1, npkts + npkts / 4 + 256) || h->h_out.reserve(npkts + 1, npkts + npkts / 4 + 256) ||
        h->d_status.reserve(std::max<size_t>(npkts, 1), npkts + npkts / 4 + 256) || h->h_status.reserve(std::max<size_t>(npkts, 1), npkts + npkts / 4 + 256))
        return FERHIP_E_HIP;
    if (int rc = srtp_launch(h->core, c->st, d_base, h->d_pkts, npkts, (uint8_t *)d_dst, cap, h->d_out, h->d_status, true)) return rc;
    CK(hipMemcpyAsync(h->h_out, h->d_out, (npkts + 1) * sizeof(ferhip_rtp_pkt), hipMemcpyDeviceToHost, c->st));
    if (npkts) CK(hipMemcpyAsync(h->h_status, h->d_status, npkts * sizeof(int32_t), hipMemcpyDeviceToHost, c->st));
    CK(hipStreamSynchronize(c->st));
    memcpy(h_out_pkts, h->h_out, (npkts + 1) * sizeof(ferhip_rtp_pkt));
    if (npkts) memcpy(h_status, h->h_status, npkts * sizeof(int32_t));
    return 0;
}

// known-answer surface: host memory in and out through the same kernels, on the null stream with buffers of its own
extern "C" int ferhip_srtp_blocks(int op, const ferhip_srtp_key *keys, const ferhip_srtp_index *state_in, int nstreams, const uint8_t *base,
                                  size_t base_bytes, const ferhip_rtp_pkt *pkts, size_t npkts, int misalign, uint8_t *out, size_t cap,
                                  ferhip_rtp_pkt *out_pkts, int32_t *status, ferhip_srtp_index *state_out)
{
    if ((op != FERHIP_SRTP_PROTECT && op != FERHIP_SRTP_UNPROTECT) || !keys || !state_in || !state_out || nstreams <= 0 || nstreams > 65535 ||
        misalign < 0 || misalign > 15 || (npkts && (!base || !pkts)) || (op == FERHIP_SRTP_UNPROTECT && npkts && !status))
        return FERHIP_E_ARG;
    if (int rc = fer_srtp_check_out(out, cap, out_pkts, 1, 1)) return rc;
    std::vector<uint8_t> keyed((size_t)nstreams);
    for (int s = 0; s < nstreams; s++) {
        if (keys[s].set > 1 || keys[s].reserved || state_in[s].set > 1) return FERHIP_E_ARG;
        keyed[s] = keys[s].set;
    }
    if (int rc = fer_srtp_check_rows((const FerSrtpRow *)pkts, npkts, (size_t)nstreams, keyed.data(), base_bytes)) return rc;
    SrtpCore c;
    if (int rc = c.create(nstreams, srtp_tables())) return rc;
    std::vector<uint32_t> rows((size_t)nstreams * FER_SRTP_ROW, 0u);
    std::vector<unsigned long long> st((size_t)nstreams);
    for (int s = 0; s < nstreams; s++) {
        if (keyed[s]) fer_srtp_row(srtp_tables(), keys[s].master_key, keys[s].master_salt, rows.data() + (size_t)s * FER_SRTP_ROW);
        st[s] = FER_SRTP_STATE(state_in[s].set, state_in[s].roc, state_in[s].s_l);
    }
    DevBuf<uint8_t> dbase, dst;
    DevBuf<ferhip_rtp_pkt> dp, dout;
    DevBuf<int32_t> dstat;
    if (dbase.reserve((size_t)misalign + base_bytes + 16) || dst.reserve(std::max<size_t>(cap, 16)) || dp.reserve(std::max<size_t>(npkts, 1)) ||
        dout.reserve(npkts + 1) || dstat.reserve(std::max<size_t>(npkts, 1)))
        return FERHIP_E_HIP;
    CK(hipMemcpy(c.d_rows, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    CK(hipMemcpy(c.d_state, st.data(), st.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    if (base_bytes) CK(hipMemcpy(dbase + misalign, base, base_bytes, hipMemcpyHostToDevice));
    if (npkts) CK(hipMemcpy(dp, pkts, npkts * sizeof(ferhip_rtp_pkt), hipMemcpyHostToDevice));
    if (cap) CK(hipMemcpy(dst, out, cap, hipMemcpyHostToDevice));
    const bool un = op == FERHIP_SRTP_UNPROTECT;
    if (int rc = srtp_launch(c, nullptr, dbase + misalign, dp, npkts, dst, cap, dout, un ? dstat.p : nullptr, un)) return rc;
    CK(hipDeviceSynchronize());
    if (cap) CK(hipMemcpy(out, dst, cap, hipMemcpyDeviceToHost));
    CK(hipMemcpy(out_pkts, dout, (npkts + 1) * sizeof(ferhip_rtp_pkt), hipMemcpyDeviceToHost));
    if (un && npkts) CK(hipMemcpy(status, dstat, npkts * sizeof(int32_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(st.data(), c.d_state, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int s = 0; s < nstreams; s++) {
        state_out[s].roc = (uint32_t)(st[s] >> 16);
        state_out[s].s_l = (uint16_t)st[s];
        state_out[s].set = (uint16_t)((st[s] >> 48) & 1ull);
    }
    return 0;  // the temporaries go with their owners
}
