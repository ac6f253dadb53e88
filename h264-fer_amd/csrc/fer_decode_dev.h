// fer_decode_dev.h -- device bit reader, decode tables, CAVLC block parser and Intra4x4 mode derivation shared by the decode
// twin (fer_decode.hip) and the per-macroblock seams (k_cavlc_parse_blocks, k_residual_mbs, k_seam_i4_modes in
// fer_mbunit.hip): residual_block_cavlc and the decoder's form of nC (F/residual.cpp:1069-1386, :424-538),
// getIntra4x4PredMode (F/intra.cpp:77-136).  The tables are built once per device by dec_luts()
// (fer_decode.hip, declared in fer_internal.h).
#pragma once
#include "fer_dev.h"

// Bit reader over one slice: a 64-bit window of the stream starting at the 32-bit aligned position wbase (big-endian),
// refilled 32 bits at a time.  The stream itself comes in through a 512-byte ring in LDS, one coalesced 256-byte load of
// the whole wavefront per 2 048 bits: a refill is then a DS read, not a trip to memory (a dword requested from memory
// one refill ahead was waited for on the spot all the same -- the copy into the loop-carried register needs the data).
// Position, window and everything derived from them are wave-uniform (scalar registers).
struct DecBits {
    const uint8_t *buf;  // 4-byte aligned; the slice buffers are padded by 16 bytes
    unsigned size;  // bytes
    unsigned pos;   // bit position
    unsigned long long win;  // stream bits [wbase, wbase + 64)
    unsigned wbase;          // multiple of 32, pos - wbase < 32
    uint32_t *ring;          // [128] dwords of this wavefront in LDS: stream bytes [256 c, 256 c + 256) in half c & 1
};

// chunk c of the stream into its half of the ring (addresses clamped into the padded buffer)
__device__ __forceinline__ void db_chunk(const DecBits &b, unsigned c)
{
    const unsigned lane = threadIdx.x & 63;
    const unsigned a = min(c * 256u + lane * 4u, (b.size + 3u) & ~3u);
    const uint32_t v = *(const uint32_t *)(b.buf + a);
    b.ring[((c & 1u) << 6) + lane] = v;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// the dword at byte offset `byte` (a multiple of 4) as big-endian stream bits, zero past the end of the slice
__device__ __forceinline__ unsigned db_dword(const DecBits &b, unsigned byte)
{
    unsigned v = __builtin_bswap32((unsigned)__builtin_amdgcn_readfirstlane((int)b.ring[(byte >> 2) & 127u]));
    if (byte + 4 > b.size) v = byte >= b.size ? 0u : (v & ~(0xffffffffu >> (8 * (b.size - byte))));
    return v;
}
__device__ __forceinline__ void db_open(DecBits &b, const uint8_t *buf, unsigned size, unsigned pos, uint32_t *ring)
{
    b.buf = buf;
    b.size = size;
    b.pos = pos;
    b.ring = ring;
    b.wbase = pos & ~31u;
    const unsigned by = b.wbase >> 3;
    db_chunk(b, by >> 8);
    if (((by + 4) >> 8) != (by >> 8)) db_chunk(b, (by + 4) >> 8);
    b.win = ((unsigned long long)db_dword(b, by) << 32) | db_dword(b, by + 4);
}
__device__ __forceinline__ void db_skip(DecBits &b, unsigned n)  // n <= 32
{
    b.pos += n;
    if (__builtin_expect(b.pos - b.wbase >= 32, 0)) {  // (a lone wavefront pays ~20 cycles per taken branch: the common case falls through)
        const unsigned by = (b.wbase >> 3) + 8;
        if (__builtin_expect((by & 255u) == 0, 0)) db_chunk(b, by >> 8);
        b.win = (b.win << 32) | db_dword(b, by);
        b.wbase += 32;
    }
}
__device__ __forceinline__ unsigned db_peek(const DecBits &b, int n)  // 1 <= n <= 32
{
    return (unsigned)((b.win << (b.pos - b.wbase)) >> (64 - n));
}
__device__ __forceinline__ unsigned db_bits(DecBits &b, int n)
{
    if (n == 0) return 0;
    unsigned v = db_peek(b, n);
    db_skip(b, (unsigned)n);
    return v;
}
__device__ __forceinline__ unsigned db_bit(DecBits &b) { return db_bits(b, 1); }
__device__ __forceinline__ unsigned db_ue(DecBits &b)  // F/expgolomb.cpp:122-140
{
    unsigned w = db_peek(b, 24);
    int z = w ? __clz((int)w) - 8 : 24;
    db_skip(b, (unsigned)(z + 1));
    unsigned s = db_bits(b, z);
    return (1u << z) - 1u + s;
}
__device__ __forceinline__ int db_se(DecBits &b)
{
    int v = (int)db_ue(b);
    return (v & 1) ? (v + 1) / 2 : -v / 2;
}
// te(v) as the reference reads it, whatever the range (F/expgolomb.cpp:156-178): an Exp-Golomb prefix and suffix;
// a code number above 2 is returned as is, anything else (other than the single bit "1" = 0) is followed by one
// more bit whose inverse is the value.  The bits consumed are what matters here -- the value is never used.
__device__ __forceinline__ unsigned db_te(DecBits &b)
{
    unsigned w = db_peek(b, 24);
    int z = w ? __clz((int)w) - 8 : 24;
    db_skip(b, (unsigned)(z + 1));
    if (z == 0) return 0;
    unsigned x = db_bits(b, z);
    if (x > 1) return (1u << z) - 1u + x;
    return db_bit(b) ? 0u : 1u;
}
__device__ __forceinline__ bool db_more(const DecBits &b) { return (b.pos >> 3) + 1 < b.size; }

// ---- decode tables: the code tables of F/residual_tables.cpp inverted once per process into direct
// look-ups by the next bits of the stream (coeff_token: 16 bits, total_zeros: 9, run_before: 3).
// entry = len << 8 | value, 0 = no code matches; coeff_token value = TotalCoeff << 2 | TrailingOnes.
#define DEC_CT_SUBS 48
// One coefficient level per look-up (level_prefix + level_suffix, F/residual.cpp:1183-1262) by the next DEC_LEV_BITS bits
// of the stream and the decoder state: states 0..6 = suffixLength, 7 / 8 = suffixLength 0 / 1 at the first level after
// fewer than three trailing ones (levelCode + 2).  entry = bits | next suffixLength << 4 | level << 7 (signed 9 bits),
// 0 = the code does not fit the window (long prefixes, escapes): the arithmetic path decodes it.
#define DEC_LEV_BITS 11
#define DEC_LEV_STATES 9
struct DecLuts {
    uint16_t ct[4][65536];   // class 0..2 by nC, 3 = chroma DC: the full 16-bit look-up (build step only)
    // what the parse kernel keeps in LDS: coeff_token in two levels of 8 bits
    uint16_t ct1[4][256];    // len <= 8: the entry; longer codes: 0x8000 | sub-table
    uint16_t ct2[DEC_CT_SUBS][256];
    uint16_t tz[15][512];    // by TotalCoeff - 1
    uint16_t tzdc[3][8];
    uint16_t rb[6][8];       // by zerosLeft - 1 (zerosLeft <= 6)
    uint16_t lev[DEC_LEV_STATES][1 << DEC_LEV_BITS];
    int nsub;
};
struct DecLutsLds {  // the same tables, resident in LDS for one parse wavefront
    uint16_t ct1[4][256];
    uint16_t ct2[DEC_CT_SUBS][256];
    uint16_t tz[15][512];
    uint16_t tzdc[3][8];
    uint16_t rb[6][8];
    uint16_t lev[DEC_LEV_STATES][1 << DEC_LEV_BITS];
};

// residual_block_cavlc, F/residual.cpp:1069-1386.  coef: int16 destination (maxNumCoeff entries, already zero).
// The levels of the block live in one vector register (lane i = level i), the runs in a scalar 64-bit word.  Returns TotalCoeff, or -1 on a malformed block.
__device__ int dec_block(DecBits &b, const DecLutsLds *L, int16_t *coef, int maxNumCoeff, int nC)
{
    int TotalCoeff, TrailingOnes = 0;
    if (nC >= 8) {
        unsigned v = db_bits(b, 6);
        if (v == 3) {
            TotalCoeff = 0;
        } else {
            TotalCoeff = (int)(v >> 2) + 1;
            TrailingOnes = (int)(v & 3);
        }
    } else {
        const int cls = nC == -1 ? 3 : (nC <= 1 ? 0 : (nC <= 3 ? 1 : 2));
        const unsigned w16 = db_peek(b, 16);
        unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)L->ct1[cls][w16 >> 8]);
        if (e & 0x8000) e = (unsigned)__builtin_amdgcn_readfirstlane((int)L->ct2[e & 0x7fff][w16 & 0xff]);
        if (e == 0) return -1;
        db_skip(b, e >> 8);
        TotalCoeff = (int)((e >> 2) & 31);
        TrailingOnes = (int)(e & 3);
    }
    if (TotalCoeff == 0) return 0;
    if (TotalCoeff > maxNumCoeff) return -1;
    const int lane = (int)(threadIdx.x & 63);
    int lvv = 0;
    // the sign bits of the trailing ones, first coefficient first.  The 6-bit coeff_token of nC >= 8 can name more trailing
    // ones than coefficients; the reference reads one sign per coefficient then (F/residual.cpp:1249-1254), so does this
    const int nsign = min(TrailingOnes, TotalCoeff);
    if (nsign) {
        const unsigned sg = db_bits(b, nsign);
        lvv = 1 - 2 * (int)((sg >> ((nsign - 1 - lane) & 31)) & 1u);
    }
    int suffixLength = (TotalCoeff > 10 && TrailingOnes < 3) ? 1 : 0;
    int st = TrailingOnes < 3 ? 7 + suffixLength : suffixLength;
    for (int i = TrailingOnes; i < TotalCoeff; i++) {
        int lev;
        const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)L->lev[st][db_peek(b, DEC_LEV_BITS)]);
        if (__builtin_expect(e != 0, 1)) {
            db_skip(b, e & 15u);
            lev = ((int)(e << 16)) >> 23;
            suffixLength = (int)((e >> 4) & 7u);
        } else {
            const unsigned w = db_peek(b, 32);
            if (w == 0) return -1;  // level_prefix beyond 31
            const int prefix = __clz((int)w);
            db_skip(b, (unsigned)(prefix + 1));
            int size = (prefix == 14 && suffixLength == 0) ? 4 : (prefix >= 15 ? prefix - 3 : suffixLength);
            unsigned suffix = (size > 0 || prefix >= 14) ? db_bits(b, size) : 0;
            int levelCode = (min(prefix, 15) << suffixLength);
            if (size > 0 || prefix >= 14) levelCode += (int)suffix;
            if (prefix >= 15 && suffixLength == 0) levelCode += 15;
            if (st >= 7) levelCode += 2;
            lev = (levelCode & 1) == 0 ? (levelCode + 2) >> 1 : (-levelCode - 1) >> 1;
            if (suffixLength == 0) suffixLength = 1;
            if (iabs(lev) > (3 << (suffixLength - 1)) && suffixLength < 6) suffixLength++;
        }
        st = suffixLength;
        lvv = lane == i ? lev : lvv;
    }
    int zerosLeft = 0;
    if (TotalCoeff < maxNumCoeff) {
        const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane(
            (int)(nC == -1 ? L->tzdc[TotalCoeff - 1][db_peek(b, 3)] : L->tz[TotalCoeff - 1][db_peek(b, 9)]));
        if (e == 0) return -1;
        db_skip(b, e >> 8);
        zerosLeft = (int)(e & 0xff);
        // (the 4x4 total_zeros tables serve the 15-coefficient blocks too and can name one zero too many for them)
        if (TotalCoeff + zerosLeft > maxNumCoeff) return -1;
    }
    unsigned long long runs = 0;  // run_before of coefficient j in bits 4j..4j+3 (scalar registers, no LDS round trips)
    int j = 0;
    for (; j < TotalCoeff - 1 && zerosLeft > 0; j++) {  // (no zeros left: every further run is 0)
        int rb;
        if (zerosLeft > 6) {
            rb = 7 - (int)db_bits(b, 3);
            if (rb == 7) {
                const unsigned w = db_peek(b, 32);
                if (w == 0) return -1;
                const int z = __clz((int)w);
                db_skip(b, (unsigned)(z + 1));
                rb += z;
            }
        } else {
            const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)L->rb[zerosLeft - 1][db_peek(b, 3)]);
            if (e == 0) return -1;
            db_skip(b, e >> 8);
            rb = (int)(e & 0xff);
        }
        // a run_before above zerosLeft (only the escape above can code one): the reference lets zerosLeft go negative and
        // stores the levels in front of the block, into a neighbouring block of its level array or outside it.  Refused, like
        // the other blocks whose coefficients do not fit them (TotalCoeff or total_zeros too large, above).
        if (rb > zerosLeft) return -1;
        runs |= (unsigned long long)(rb & 15) << (4 * j);
        zerosLeft -= rb;
    }
    runs |= (unsigned long long)(max(zerosLeft, 0) & 15) << (4 * (TotalCoeff - 1));
    {  // placement, one coefficient per lane: position of coefficient i = sum over k >= i of (run_k + 1), minus 1
        const int i = lane;
        if (i < TotalCoeff) {
            unsigned long long x = runs >> (4 * i);
            unsigned long long sm = (x & 0x0f0f0f0f0f0f0f0full) + ((x >> 4) & 0x0f0f0f0f0f0f0f0full);
            unsigned s32 = (unsigned)sm + (unsigned)(sm >> 32);
            int pos = (TotalCoeff - i) - 1 + (int)((s32 * 0x01010101u) >> 24);
            if (pos < maxNumCoeff) coef[pos] = (int16_t)lvv;
        }
    }
    return TotalCoeff;
}

// getIntra4x4PredMode, F/intra.cpp:77-136, for the sixteen blocks of the Intra4x4 macroblock at (mbx, mby): the modes, 4
// bits per block, from i4flags (prev_intra4x4_pred_mode_flag << 3 | rem_intra4x4_pred_mode, 4 bits per block) and the
// neighbours' side: left_i4 / above_i4 = the macroblock to the left / above is Intra4x4, left_modes = its sixteen modes,
// above_modes = the modes of its blocks 10, 11, 14, 15.  Everything is wave-uniform (scalar registers); shared by
// k_dec_parse and the neighbourhood seam (k_seam_i4_modes, fer_mbunit.hip).
__device__ __forceinline__ unsigned long long dec_i4_modes(unsigned long long i4flags, int mbx, int mby, bool constrained_intra, bool left_i4,
                                                           unsigned long long left_modes, bool above_i4, unsigned above_modes)
{
    unsigned long long cm = 0;
    for (int blk = 0; blk < 16; blk++) {
        bool edgeA = blk == 0 || blk == 2 || blk == 8 || blk == 10;
        bool edgeB = blk == 0 || blk == 1 || blk == 4 || blk == 5;
        bool okA = !(edgeA && mbx == 0), okB = !(edgeB && mby == 0);
        int mA = 2, mB = 2;
        if (okA && okB && !constrained_intra) {
            // c_nbA / c_nbB (the neighbouring block to the left / above), 4 bits per block: no table load in the chain
            const int nA = (int)((0xebc9af8d63412705ull >> (4 * blk)) & 15), nB = (int)((0xdc76983254fe10baull >> (4 * blk)) & 15);
            if (edgeA)
                mA = left_i4 ? (int)((left_modes >> (4 * nA)) & 15) : 2;
            else
                mA = (int)((cm >> (4 * nA)) & 15);
            if (edgeB)
                mB = above_i4 ? (int)((above_modes >> (4 * ((nB & 1) | ((nB >> 1) & 2)))) & 15) : 2;  // 10, 11, 14, 15 -> 0 .. 3
            else
                mB = (int)((cm >> (4 * nB)) & 15);
        }
        int pm = mA <= mB ? mA : mB;
        int f = (int)((i4flags >> (4 * blk)) & 15);
        int mode = (f & 8) ? pm : ((f & 7) < pm ? (f & 7) : (f & 7) + 1);
        cm |= (unsigned long long)mode << (4 * blk);
    }
    return cm;
}

// What the total-coefficient prediction needs from a decoded neighbour, kept in LDS: one entry per macroblock
// column holds the macroblock above until the current one replaces it (so entry x - 1 is the left neighbour).
struct DecNb {
    uint8_t tc[24];
    uint8_t cbpL, cbpC, skip, i4;  // i4: an Intra4x4 macroblock (its bottom-row prediction modes are in the i4row entry)
};
// nC of F/residual.cpp:424-538 (wave-uniform)
__device__ int dec_nC(const DecNb *row, int x, int y, bool luma, int blk, int plane, const uint8_t *tcur, int cbpL, int cbpC)
{
    bool edgeA, edgeB;
    int bA, bB;
    if (luma) {
        edgeA = blk == 0 || blk == 2 || blk == 8 || blk == 10;
        edgeB = blk == 0 || blk == 1 || blk == 4 || blk == 5;
        bA = c_nbA[blk];
        bB = c_nbB[blk];
    } else {
        edgeA = blk == 0 || blk == 2;
        edgeB = blk < 2;
        bA = c_nbcA[blk];
        bB = c_nbcB[blk];
    }
    bool availA = true, availB = true;
    int nA = 0, nB = 0;
    if (edgeA) {
        if (x == 0)
            availA = false;
        else {
            const DecNb &m = row[x - 1];
            bool zero = luma ? ((m.cbpL & (1 << (bA / 4))) == 0) : ((m.cbpC & 2) == 0);
            if (!(m.skip || zero)) nA = luma ? m.tc[bA] : m.tc[16 + plane * 4 + bA];
        }
    } else {
        bool zero = luma ? ((cbpL & (1 << (bA / 4))) == 0) : ((cbpC & 2) == 0);
        if (!zero) nA = luma ? tcur[bA] : tcur[16 + plane * 4 + bA];
    }
    if (edgeB) {
        if (y == 0)
            availB = false;
        else {
            const DecNb &m = row[x];
            bool zero = luma ? ((m.cbpL & (1 << (bB / 4))) == 0) : ((m.cbpC & 2) == 0);
            if (!(m.skip || zero)) nB = luma ? m.tc[bB] : m.tc[16 + plane * 4 + bB];
        }
    } else {
        bool zero = luma ? ((cbpL & (1 << (bB / 4))) == 0) : ((cbpC & 2) == 0);
        if (!zero) nB = luma ? tcur[bB] : tcur[16 + plane * 4 + bB];
    }
    int r = 0;
    if (availA && availB)
        r = (nA + nB + 1) >> 1;
    else if (availA)
        r = nA;
    else if (availB)
        r = nB;
    return __builtin_amdgcn_readfirstlane(r);
}
