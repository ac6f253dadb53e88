// fer_srtp_host.h -- the host half of SRTP (fer_srtp.hip; the definition stands in include/ferhip.h): the AES-128 key
// expansion and the single block the key derivation needs, the derivation of RFC 3711 section 4.3 at rate 0, SHA-1 for the two
// HMAC midstates, the session row that ferhip_srtp_set_key uploads, the header rule, the index estimate and the argument
// checks.  Plain C++ without the HIP runtime, so that it can be compiled into a stand-alone host program and run under a
// sanitizer (tools/srtp_host_check.cpp); under hipcc the header rule and the index estimate are also device code, so the
// kernels and that program run the same.  The kernels restate AES and SHA-1 (tables in LDS, rounds unrolled); what they
// give is compared with these functions through ferhip_srtp_blocks.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define FER_SRTP_HD __host__ __device__ inline
#else
#define FER_SRTP_HD inline
#endif

#define FER_SRTP_TAG 10u                  // bytes of the authentication tag
#define FER_SRTP_MAX_PAYLOAD (1u << 20)   // 65536 keystream blocks: the counter lives in the last two bytes of the IV
// One stream's row of the session table, 64 words: the 44 round key words (big-endian words of the key schedule), k_s || 00 00
// as four big-endian words, the SHA-1 state behind k_a ^ 36.. and behind k_a ^ 5c.., then 1 = the row holds a key.
#define FER_SRTP_ROW 64u
#define FER_SRTP_ROW_KS 44u
#define FER_SRTP_ROW_MID_I 48u
#define FER_SRTP_ROW_MID_O 53u
#define FER_SRTP_ROW_KEYED 58u
// The AES tables as the cipher pass stages them: Te0[x] = (2 s, s, s, 3 s) with s = S[x], most significant byte first, then
// the S-box as 64 little-endian words.
#define FER_SRTP_TAB 320u
// the packet index state of a stream as one word the device takes the maximum of: set << 48 | roc << 16 | s_l
#define FER_SRTP_STATE(set, roc, s_l) ((unsigned long long)((set) ? 1u : 0u) << 48 | (unsigned long long)(uint32_t)(roc) << 16 | ((s_l) & 0xffffu))

// ---- AES-128 (FIPS-197)
// The S-box from its definition: the inverse in GF(2^8) and the affine map; p runs through the powers of 3, q through those
// of its inverse.
inline void fer_aes_sbox(uint8_t sb[256])
{
    uint8_t p = 1, q = 1;
    do {
        p = (uint8_t)(p ^ (p << 1) ^ ((p & 0x80) ? 0x1B : 0));
        q ^= (uint8_t)(q << 1);
        q ^= (uint8_t)(q << 2);
        q ^= (uint8_t)(q << 4);
        if (q & 0x80) q ^= 0x09;
        const uint32_t x = q;
        const uint32_t r = x ^ (x << 1 | x >> 7) ^ (x << 2 | x >> 6) ^ (x << 3 | x >> 5) ^ (x << 4 | x >> 4);
        sb[p] = (uint8_t)((r & 0xff) ^ 0x63);
    } while (p != 1);
    sb[0] = 0x63;
}

inline uint32_t fer_aes_xtime(uint32_t s) { return ((s << 1) ^ ((s & 0x80u) ? 0x1Bu : 0u)) & 0xffu; }

inline void fer_aes_tables(uint32_t tab[FER_SRTP_TAB])
{
    uint8_t sb[256];
    fer_aes_sbox(sb);
    for (uint32_t x = 0; x < 256; x++) {
        const uint32_t s = sb[x], s2 = fer_aes_xtime(s);
        tab[x] = s2 << 24 | s << 16 | s << 8 | (s2 ^ s);
    }
    for (uint32_t w = 0; w < 64; w++)
        tab[256 + w] = (uint32_t)sb[4 * w] | (uint32_t)sb[4 * w + 1] << 8 | (uint32_t)sb[4 * w + 2] << 16 | (uint32_t)sb[4 * w + 3] << 24;
}
inline uint32_t fer_aes_sb(const uint32_t *tab, uint32_t x) { return (tab[256 + (x >> 2)] >> (8 * (x & 3))) & 0xffu; }

inline uint32_t fer_be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
inline void fer_put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }

// the key schedule as 44 big-endian words
inline void fer_aes_expand(const uint32_t *tab, const uint8_t key[16], uint32_t rk[44])
{
    for (int i = 0; i < 4; i++) rk[i] = fer_be32(key + 4 * i);
    uint32_t rcon = 1;
    for (int i = 4; i < 44; i++) {
        uint32_t t = rk[i - 1];
        if (i % 4 == 0) {
            t = t << 8 | t >> 24;
            t = fer_aes_sb(tab, t >> 24) << 24 | fer_aes_sb(tab, (t >> 16) & 255) << 16 | fer_aes_sb(tab, (t >> 8) & 255) << 8 | fer_aes_sb(tab, t & 255);
            t ^= rcon << 24;
            rcon = fer_aes_xtime(rcon);
        }
        rk[i] = rk[i - 4] ^ t;
    }
}

inline uint32_t fer_ror(uint32_t v, int n) { return v >> n | v << (32 - n); }

// one block: the state as four big-endian words, a column each
inline void fer_aes_block(const uint32_t *tab, const uint32_t rk[44], const uint32_t in[4], uint32_t out[4])
{
    uint32_t s[4], t[4];
    for (int c = 0; c < 4; c++) s[c] = in[c] ^ rk[c];
    for (int r = 1; r < 10; r++) {
        for (int c = 0; c < 4; c++)
            t[c] = tab[s[c] >> 24] ^ fer_ror(tab[(s[(c + 1) & 3] >> 16) & 255], 8) ^ fer_ror(tab[(s[(c + 2) & 3] >> 8) & 255], 16) ^
                   fer_ror(tab[s[(c + 3) & 3] & 255], 24) ^ rk[4 * r + c];
        for (int c = 0; c < 4; c++) s[c] = t[c];
    }
    for (int c = 0; c < 4; c++)
        out[c] = (fer_aes_sb(tab, s[c] >> 24) << 24 | fer_aes_sb(tab, (s[(c + 1) & 3] >> 16) & 255) << 16 |
                  fer_aes_sb(tab, (s[(c + 2) & 3] >> 8) & 255) << 8 | fer_aes_sb(tab, s[(c + 3) & 3] & 255)) ^
                 rk[40 + c];
}
inline void fer_aes_block_bytes(const uint32_t *tab, const uint32_t rk[44], const uint8_t in[16], uint8_t out[16])
{
    uint32_t a[4], b[4];
    for (int c = 0; c < 4; c++) a[c] = fer_be32(in + 4 * c);
    fer_aes_block(tab, rk, a, b);
    for (int c = 0; c < 4; c++) fer_put_be32(out + 4 * c, b[c]);
}

// n bytes of the counter mode keystream of RFC 3711 section 4.1.1: block b is AES(iv + b), the sum in the last two bytes
inline void fer_aes_cm(const uint32_t *tab, const uint32_t rk[44], const uint8_t iv[16], uint8_t *out, size_t n)
{
    uint8_t ctr[16], ks[16];
    memcpy(ctr, iv, 16);
    const uint32_t c0 = (uint32_t)iv[14] << 8 | iv[15];
    for (size_t b = 0; 16 * b < n; b++) {
        const uint32_t c = (c0 + (uint32_t)b) & 0xffffu;
        ctr[14] = (uint8_t)(c >> 8), ctr[15] = (uint8_t)c;
        fer_aes_block_bytes(tab, rk, ctr, ks);
        memcpy(out + 16 * b, ks, n - 16 * b < 16 ? n - 16 * b : 16);
    }
}

// ---- the key derivation at rate 0 (r = 0): out = k_e [16] | k_a [20] | k_s [14]
inline void fer_srtp_derive(const uint32_t *tab, const uint8_t master_key[16], const uint8_t master_salt[14], uint8_t out[50])
{
    uint32_t rk[44];
    fer_aes_expand(tab, master_key, rk);
    static const struct { uint8_t label; uint8_t at, n; } part[3] = {{0, 0, 16}, {1, 16, 20}, {2, 36, 14}};
    for (int k = 0; k < 3; k++) {
        uint8_t iv[16] = {0};
        memcpy(iv, master_salt, 14);
        iv[7] ^= part[k].label;
        fer_aes_cm(tab, rk, iv, out + part[k].at, part[k].n);
    }
}

// ---- SHA-1 (FIPS 180), one compression
inline void fer_sha1_compress(uint32_t h[5], const uint8_t block[64])
{
    uint32_t w[80];
    for (int t = 0; t < 16; t++) w[t] = fer_be32(block + 4 * t);
    for (int t = 16; t < 80; t++) {
        const uint32_t x = w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16];
        w[t] = x << 1 | x >> 31;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
    for (int t = 0; t < 80; t++) {
        const uint32_t f = t < 20 ? ((b & c) | (~b & d)) : t < 40 ? (b ^ c ^ d) : t < 60 ? ((b & c) | (b & d) | (c & d)) : (b ^ c ^ d);
        const uint32_t k = t < 20 ? 0x5A827999u : t < 40 ? 0x6ED9EBA1u : t < 60 ? 0x8F1BBCDCu : 0xCA62C1D6u;
        const uint32_t x = (a << 5 | a >> 27) + f + e + k + w[t];
        e = d, d = c, c = b << 30 | b >> 2, b = a, a = x;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e;
}
inline void fer_sha1_init(uint32_t h[5]) { h[0] = 0x67452301u, h[1] = 0xEFCDAB89u, h[2] = 0x98BADCFEu, h[3] = 0x10325476u, h[4] = 0xC3D2E1F0u; }

// the SHA-1 state behind the block k_a ^ pad.. (pad = 0x36 inner, 0x5c outer) of HMAC with a 20-byte key
inline void fer_hmac_midstate(const uint8_t k_a[20], uint8_t pad, uint32_t h[5])
{
    uint8_t block[64];
    memset(block, pad, 64);
    for (int i = 0; i < 20; i++) block[i] ^= k_a[i];
    fer_sha1_init(h);
    fer_sha1_compress(h, block);
}

// HMAC-SHA1 from the two midstates over msg[0, n), whole (20 bytes): the reference of the tag pass
inline void fer_hmac_sha1(const uint32_t mid_i[5], const uint32_t mid_o[5], const uint8_t *msg, size_t n, uint8_t out[20])
{
    uint32_t h[5];
    uint8_t block[64];
    memcpy(h, mid_i, 20);
    size_t at = 0;
    for (; at + 64 <= n; at += 64) fer_sha1_compress(h, msg + at);
    const size_t rest = n - at;
    memset(block, 0, 64);
    if (rest) memcpy(block, msg + at, rest);
    block[rest] = 0x80;
    if (rest >= 56) {
        fer_sha1_compress(h, block);
        memset(block, 0, 64);
    }
    const uint64_t bits = (uint64_t)(64 + n) * 8;
    fer_put_be32(block + 56, (uint32_t)(bits >> 32));
    fer_put_be32(block + 60, (uint32_t)bits);
    fer_sha1_compress(h, block);
    memset(block, 0, 64);
    for (int i = 0; i < 5; i++) fer_put_be32(block + 4 * i, h[i]);
    block[20] = 0x80;
    fer_put_be32(block + 60, (64 + 20) * 8);
    memcpy(h, mid_o, 20);
    fer_sha1_compress(h, block);
    for (int i = 0; i < 5; i++) fer_put_be32(out + 4 * i, h[i]);
}

// the row of the session table that ferhip_srtp_set_key uploads
inline void fer_srtp_row(const uint32_t *tab, const uint8_t master_key[16], const uint8_t master_salt[14], uint32_t row[FER_SRTP_ROW])
{
    uint8_t k[50], ks[16] = {0};
    fer_srtp_derive(tab, master_key, master_salt, k);
    memset(row, 0, FER_SRTP_ROW * sizeof(uint32_t));
    fer_aes_expand(tab, k, row);
    memcpy(ks, k + 36, 14);
    for (int i = 0; i < 4; i++) row[FER_SRTP_ROW_KS + i] = fer_be32(ks + 4 * i);
    fer_hmac_midstate(k + 16, 0x36, row + FER_SRTP_ROW_MID_I);
    fer_hmac_midstate(k + 16, 0x5c, row + FER_SRTP_ROW_MID_O);
    row[FER_SRTP_ROW_KEYED] = 1u;
}

// ---- the packet rules
// The header rule: the bytes in front of the payload of the L bytes at p, 0 = malformed.  Reads inside [p, p + L) only.
FER_SRTP_HD uint32_t fer_srtp_header(const uint8_t *p, uint32_t L)
{
    if (L < 12u || p[0] >> 6 != 2u) return 0u;
    uint32_t hl = 12u + 4u * (p[0] & 15u);
    if (p[0] & 0x10u) {
        if (hl + 4u > L) return 0u;
        hl += 4u + 4u * ((uint32_t)p[hl + 2u] << 8 | p[hl + 3u]);
    }
    if (hl > L || L - hl > FER_SRTP_MAX_PAYLOAD) return 0u;
    return hl;
}

// The index estimate of RFC 3711 section 3.3.1: v for seq against (roc, s_l), modulo 2^32
FER_SRTP_HD uint32_t fer_srtp_estimate(uint32_t roc, uint32_t s_l, uint32_t seq)
{
    if (s_l < 32768u) return (seq > s_l && seq - s_l > 32768u) ? roc - 1u : roc;
    return s_l - 32768u > seq ? roc + 1u : roc;
}

// ---- the argument checks that need no device: 0, -1 (FERHIP_E_ARG) or -3 (FERHIP_E_STATE).  Rows as (offset, bytes,
// stream) of 16 bytes; keyed[s] != 0 = stream s has a key; base_bytes = ~0 where the packets' range is not known.
struct FerSrtpRow { uint64_t offset; uint32_t bytes, stream; };
inline int fer_srtp_check_rows(const FerSrtpRow *pkts, size_t npkts, size_t S, const uint8_t *keyed, uint64_t base_bytes)
{
    if (npkts && !pkts) return -1;
    if (npkts > 0x7fffffffu) return -1;
    for (size_t k = 0; k < npkts; k++) {
        if (pkts[k].stream >= S) return -1;
        if (base_bytes != ~0ull && (pkts[k].offset > base_bytes || pkts[k].bytes > base_bytes - pkts[k].offset)) return -1;
    }
    for (size_t k = 0; k < npkts; k++)
        if (!keyed[pkts[k].stream]) return -3;
    return 0;
}
inline int fer_srtp_check_out(const void *dst, uint64_t cap, const void *out_pkts, unsigned dst_align, unsigned tab_align)
{
    if (!out_pkts || (!dst && cap)) return -1;
    if (((uintptr_t)dst & (dst_align - 1u)) || ((uintptr_t)out_pkts & (tab_align - 1u))) return -1;
    return 0;
}
