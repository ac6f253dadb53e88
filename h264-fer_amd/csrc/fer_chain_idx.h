// fer_chain_idx.h -- where a step of the motion chain (k_me_resolve, fer_me.hip) finds what the guessed search left for it.
// The chain requests the lists of step gx + RES_AHEAD while it works on step gx, so the step it asks for has to be clamped
// to the row: the last row of the last stream ends where the arrays end.  Plain C++ without the HIP runtime, so that the
// arithmetic can be swept on the host (tools/chain_idx_host_check.cpp); under hipcc it is device code as well, and the
// kernel uses these functions and nothing else to address the lists.
#pragma once

#ifdef __HIPCC__
#define FER_CHAIN_HD __host__ __device__ inline
#else
#define FER_CHAIN_HD inline
#endif

#ifndef RES_AHEAD
#define RES_AHEAD 1  // steps between the request of a step's lists and their use (1 or 2)
#endif

#define FER_CHAIN_L1 17u  // entries of a partition in spec_l1
#define FER_CHAIN_L2 33u  // ... in spec_l2, and survivors of a partition in st3 (three ints each)

// Offsets of one lane's operands of one step, in elements, from the entry of the row's first partition (0, gy): the
// arrays are laid out [macroblock][quadrant], a row of partitions owns the quadrants (gy & 1) * 2 + {0, 1} of a row of
// macroblocks.
struct ChainIdx {
    unsigned rp;   // spec_hdr (int4) and st3n (int)
    unsigned l1;   // spec_l1 (int2)
    unsigned l2;   // spec_l2 (int2)
    unsigned st3;  // st3 (int): x, then y and SAD at + 1, + 2
};

// the step whose lists are requested `ahead` steps early at step gx of a row of gw partitions
FER_CHAIN_HD int chain_ahead_step(int gx, int ahead, int gw)
{
    const int g = gx + ahead;
    return g < gw - 1 ? g : gw - 1;
}

// partition g of the row, relative to the row's first partition
FER_CHAIN_HD unsigned chain_rel_part(int g) { return (unsigned)((g >> 1) * 4 + (g & 1)); }

// lanes beyond a list's length read its last entry (they are masked when the lists are priced)
FER_CHAIN_HD ChainIdx chain_idx(unsigned rp, int lane)
{
    const unsigned a1 = (unsigned)(lane < 16 ? lane : 16), a2 = (unsigned)(lane < 32 ? lane : 32);
    ChainIdx o;
    o.rp = rp;
    o.l1 = rp * FER_CHAIN_L1 + a1;
    o.l2 = rp * FER_CHAIN_L2 + a2;
    o.st3 = (rp * FER_CHAIN_L2 + a2) * 3u;
    return o;
}

FER_CHAIN_HD ChainIdx chain_idx_ahead(int gx, int ahead, int gw, int lane) { return chain_idx(chain_rel_part(chain_ahead_step(gx, ahead, gw)), lane); }
