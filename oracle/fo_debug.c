/*
 * fo_debug.c -- ORACLE (test infrastructure): accessors used by tests/ to
 * compare intermediate state (planes, features, sort, MVs, levels) of the HIP
 * path with the CPU restatement through ctypes.
 */
#include "fo.h"
#include <stdlib.h>
#include <string.h>

uint8_t *fo_dbg_plane(fo_ctx *c, int which) /* 0..2 frame, 3..5 dpb */
{
    switch (which) {
    case 0: return c->L;
    case 1: return c->C[0];
    case 2: return c->C[1];
    case 3: return c->dL;
    case 4: return c->dC[0];
    default: return c->dC[1];
    }
}
uint8_t *fo_dbg_interp(fo_ctx *c, int f) { return c->interp[f]; }
int *fo_dbg_kar(fo_ctx *c, int k, int f) { return c->kar[k][f]; }
int *fo_dbg_sorted(fo_ctx *c, int k) { return c->sorted[k]; }
int *fo_dbg_koliko(fo_ctx *c) { return c->koliko; }
int *fo_dbg_mb_type(fo_ctx *c) { return c->mb_type; }
int *fo_dbg_cbp(fo_ctx *c, int chroma) { return chroma ? c->cbp_c : c->cbp_l; }
int *fo_dbg_mv(fo_ctx *c, int y) { return y ? &c->dbg_mvy[0][0][0] : &c->dbg_mvx[0][0][0]; }
/* the decoder's (and encoder's) live vector field mvx / mvy [nmb][4][4]; entries of macroblocks that are not inter are stale */
int *fo_dbg_dec_mv(fo_ctx *c, int y) { return y ? &c->mvy[0][0][0] : &c->mvx[0][0][0]; }
int *fo_dbg_chroma_mode(fo_ctx *c) { return c->chroma_pred_mode; }
int fo_dbg_block_overrun(fo_ctx *c) { return c->block_overrun; } /* blocks so far whose coefficients did not fit them */
int fo_dbg_refusals(fo_ctx *c) { return c->refusals; }           /* FO_REFUSE_* met so far */
int fo_dbg_slice_type(fo_ctx *c) { return c->slice_type; } /* of the last slice: 0 = P, 2 = I */
int *fo_dbg_tc_l(fo_ctx *c) { return &c->tc_l[0][0]; }
int *fo_dbg_tc_c(fo_ctx *c) { return &c->tc_c[0][0][0]; }
int *fo_dbg_i4mode(fo_ctx *c) { return c->i4mode; }
int *fo_dbg_type_count(fo_ctx *c) { return c->type_count; } /* brojTipova */
void fo_dbg_set_dpb(fo_ctx *c, const uint8_t *y, const uint8_t *u, const uint8_t *v)
{
    memcpy(c->dL, y, (size_t)c->W * c->H);
    memcpy(c->dC[0], u, (size_t)c->Wc * c->Hc);
    memcpy(c->dC[1], v, (size_t)c->Wc * c->Hc);
    c->have_dpb = 1;
}
void fo_dbg_set_frame(fo_ctx *c, const uint8_t *y, const uint8_t *u, const uint8_t *v)
{
    memcpy(c->L, y, (size_t)c->W * c->H);
    memcpy(c->C[0], u, (size_t)c->Wc * c->Hc);
    memcpy(c->C[1], v, (size_t)c->Wc * c->Hc);
}

/* coded_mb_size of the Intra16x16 / Intra4x4 alternative of every macroblock of the last I picture */
int *fo_dbg_mbsize(fo_ctx *c) { return &c->dbg_mbsize[0][0]; }
/* context-free pieces for the per-macroblock KATs: one macroblock of a W x H context */
void fo_dbg_set_mb(fo_ctx *c, int cur, int mb_type, int slice_type, int qp)
{
    c->cur = cur;
    c->cur_mb_type = mb_type;
    c->mb_type[cur] = mb_type;
    c->slice_type = slice_type;
    c->QPy = qp;
}
int *fo_dbg_levels(fo_ctx *c) { return &c->lv.Lumalevel[0][0]; } /* fo_levels: Lumalevel[16][16], DC16[16], AC16[16][16], CDC[2][4], CAC[2][4][16] */
void fo_dbg_set_mv(fo_ctx *c, int mb, int sub, int part, int mvx, int mvy)
{
    c->mvx[mb][sub][part] = mvx;
    c->mvy[mb][sub][part] = mvy;
}
uint8_t *fo_dbg_dpb(fo_ctx *c, int k) { return k == 0 ? c->dL : c->dC[k - 1]; }

/* candidate lists of fo_interEncoding: on != 0 starts recording (records zeroed), 0 stops it; returns the records,
 * [nmb][4] fo_me_rec (FO_ME_REC_INTS ints each), or NULL when recording is off.  Recording changes no output. */
int *fo_dbg_me_record(fo_ctx *c, int on)
{
    if (!on) {
        free(c->me_rec);
        c->me_rec = NULL;
        return NULL;
    }
    if (!c->me_rec) c->me_rec = (fo_me_rec *)malloc((size_t)c->nmb * 4 * sizeof(fo_me_rec));
    if (!c->me_rec) return NULL; /* out of memory: recording stays off */
    memset(c->me_rec, 0, (size_t)c->nmb * 4 * sizeof(fo_me_rec));
    return (int *)c->me_rec;
}
int *fo_dbg_me_lists(fo_ctx *c) { return (int *)c->me_rec; }

/* The largest |level| fo_encode_slice produced in the last picture, over the level arrays that the macroblock's
 * mb_type and CBP cause to be written (the block list of residual_blocks, fo_cavlc.c).  Above 2063 a level does not fit
 * the 12-bit escape suffix at suffixLength 0 and the reference's writer is not pinned.  Changes no output. */
int fo_pred_class(const fo_ctx *c, int mb_type);
static void note(fo_ctx *c, const int *lv, int n)
{
    for (int i = 0; i < n; i++) {
        int a = lv[i] < 0 ? -lv[i] : lv[i];
        if (a > c->dbg_max_level) c->dbg_max_level = a;
    }
}
void fo_dbg_note_levels(fo_ctx *c)
{
    int i16 = fo_pred_class(c, c->cur_mb_type) == 1;
    if (i16) note(c, c->lv.DC16, 16);
    for (int blk = 0; blk < 16; blk++)
        if (c->cbpL & (1 << (blk >> 2))) {
            if (i16)
                note(c, c->lv.AC16[blk], 15);
            else
                note(c, c->lv.Lumalevel[blk], 16);
        }
    for (int k = 0; k < 2; k++) {
        if (c->cbpC & 3) note(c, c->lv.CDC[k], 4);
        if (c->cbpC & 2)
            for (int b = 0; b < 4; b++) note(c, c->lv.CAC[k][b], 15);
    }
}
int fo_dbg_max_level(fo_ctx *c) { return c->dbg_max_level; }
