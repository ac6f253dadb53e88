/*
 * ferhip_legacy.h -- the reference's own global-state seam, exported by libferhip with C linkage.
 *
 * A maintainer of fer_h264 who wants the GPU path behind the existing NAL/slice driver
 * (encode()/NastaviEncode(), F/fer_h264.cpp:55-134) links libferhip instead of compiling
 * rbsp_encoding.cpp, intra.cpp, moestimation.cpp, mocomp.cpp, mode_pred.cpp,
 * quantizationTransform.cpp, scaleTransform.cpp, inttransform.cpp, residual.cpp and ref_frames.cpp.
 * Names, argument meaning and side effects are the reference's:
 *
 *   reference (C++ linkage)                          here (C linkage)
 *   void RBSP_encode(NALunit &nal_unit)              void RBSP_encode(NALunit *nal_unit)     F/rbsp_encoding.h:3
 *   int  selectNALUnitType()                         int  selectNALUnitType(void)            F/ref_frames.cpp:185
 *   frame_type frame                                 frame_type frame                        F/h264_globals.h:152-158
 *   int _qParameter, BasicInterEncoding, WindowSize, MAXDIFF_SET, IntraEvery, currFrameCount
 *                                                                                            F/h264_globals.h:168-176,193
 *   int brojTipova[5], vrijeme                                                               F/h264_globals.h:166-167
 *   void RBSP_decode(NALunit nal_unit)               void RBSP_decode(NALunit nal_unit)      F/rbsp_decoding.h:3
 *   LoadY4MHeader / ReadFromY4M / writeToY4M / writeToYUV, FILE *yuvinput, *yuvoutput        F/fileIO.h
 *   forwardResidual, transformScan, forwardDCLumaIntra, forwardDCChroma                      F/quantizationTransform.h
 *   transformInverseScan, inverseResidual, InverseDCLumaIntra, InverseDCChroma               F/scaleTransform.h
 *   the per-macroblock functions (quantizationTransform ... residual_write, intraPredictionEncoding, intraPrediction,
 *   DeriveMVs): see "per-macroblock entry points" below
 *
 * Contract kept from F/rbsp_encoding.cpp:119-326: nal_unit_type 7 / 8 write SPS / PPS (the SPS
 * call also sizes the encoder from frame.Lwidth x frame.Lheight); 5 / 1 encode the picture in
 * `frame` (tightly packed planes), overwrite `frame` with the reconstruction and make it the
 * reference picture; rbsp_byte is caller-allocated and NumBytesInRBSP is the out-length.
 * Errors cannot be returned through this signature (the reference returns void): on failure
 * NumBytesInRBSP is set to 0 and a message goes to stderr.  One stream per process, like the
 * reference.
 */
#ifndef FERHIP_LEGACY_H
#define FERHIP_LEGACY_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    unsigned char forbidden_zero_bit; /* bool in the reference (F/nal.h:8-14) */
    unsigned int nal_ref_idc, nal_unit_type, NumBytesInRBSP;
    unsigned char *rbsp_byte;
} NALunit;

typedef struct {
    int Lwidth, Lheight;
    int Cwidth, Cheight;
    unsigned char *L, *C[2];
} frame_type;

extern frame_type frame;
extern int _qParameter, BasicInterEncoding, WindowSize, MAXDIFF_SET, IntraEvery, currFrameCount;
extern int brojTipova[5];
extern int vrijeme; /* clock() ticks spent in the last picture */

void RBSP_encode(NALunit *nal_unit);
int selectNALUnitType(void);

/* void RBSP_decode(NALunit nal_unit), F/rbsp_decoding.h:3 (by value, as in the reference): the callee of decode()'s
 * getNAL loop (F/fer_h264.cpp:37-47).  nal_unit_type 7 sizes and allocates `frame`, 8 takes the PPS, 5 / 1 decode one
 * picture into `frame` (it becomes the reference picture) and append it to `yuvoutput` when that file is open. */
void RBSP_decode(NALunit nal_unit);

/* Y4M ingest / emit of F/fileIO.h, through `frame`, `yuvinput` and `yuvoutput` (F/fileIO.cpp:10-11,100-176,228-346) */
#include <stdio.h>
extern FILE *yuvinput, *yuvoutput;
extern int inputWidth, inputHeight;
void LoadY4MHeader(void);
int ReadFromY4M(void);
void writeToY4M(void);
void writeToYUV(void);

/* The block-level entry points of F/quantizationTransform.h and F/scaleTransform.h under their own names (the unit-parity
 * surface of SURVEY 8b): one block per call through the same device functions the encode / decode kernels use -- a seam
 * for the maintainer's unit tests, not a fast path (the batched forms are ferhip_forward_residual ... in ferhip.h).
 * `unsigned char` stands for the reference's bool.  On a device error the output is left unchanged and a message goes
 * to stderr (the reference returns void). */
void forwardResidual(int qP, int c[4][4], int r[4][4], unsigned char Intra, unsigned char Intra16x16OrChroma); /* F/quantizationTransform.cpp:284 */
void transformScan(int c[4][4], int list[16], unsigned char Intra16x16AC);                                     /* :310 */
void forwardDCLumaIntra(int qP, int dcY[4][4], int c[4][4]);                                                   /* :293 */
void forwardDCChroma(int qP, int dcC[2][2], int c[2][2], unsigned char Intra);                                 /* :302 */
void transformInverseScan(int list[16], int c[4][4]);                                                          /* F/scaleTransform.cpp:454 */
void inverseResidual(int bitDepth, int qP, int c[4][4], int r[4][4], unsigned char intra16x16OrChroma);        /* F/scaleTransform.h */
void InverseDCLumaIntra(int bitDepth, int qP, int c[4][4], int dcY[4][4]);
void InverseDCChroma(int bitDepth, int qP, int c[2][2], int dcC[2][2]);

/* ---- per-macroblock entry points (the "per-MB" row of SURVEY.md 8b): one macroblock per call, through the same device
 * functions the kernels use (ferhip_mb_unit, ferhip_cavlc_blocks, ferhip_mc_sub_mb_parts of ferhip.h).  They work on the
 * reference's own globals: the macroblock CurrMbAddr of `frame` (F/h264_globals.h:181), QPy (:179), mb_type (:106), the
 * level arrays of F/residual.h, the vector arrays of F/mode_pred.h. */
extern int CurrMbAddr, QPy, mb_type;
extern int LumaLevel[16][16], Intra16x16DCLevel[16], Intra16x16ACLevel[16][16];
extern int ChromaDCLevel[2][4], ChromaACLevel[2][4][16];
extern int ***mvL0x, ***mvL0y; /* [macroblock][subMbIdx][subMbPartIdx], quarter samples (F/mode_pred.h) */
extern frame_type dpb;         /* the reference picture Decode() predicts from (RefPicList0[0].frame, F/ref_frames.cpp) */
void AllocateMemory(void);     /* F/mode_pred.cpp:22: sizes mvL0x / mvL0y from `frame` */
/* what the reference keeps where a caller of the bare functions cannot reach it:
 * ferhip_legacy_slice_type = shd.slice_type (MbPartPredMode reads it, F/h264_globals.h:123; RBSP_encode sets it);
 * ferhip_legacy_nC = the nC residual_block_cavlc_write / _size use (the reference derives it from file-statics that only
 * its residual_write() sets, F/residual.cpp:433-538; -1 = chroma DC); ferhip_legacy_bits / _nbits = where
 * residual_block_cavlc_write appends (the bit writer F/rbsp_IO.cpp is a leaf file the maintainer keeps) */
extern int ferhip_legacy_slice_type, ferhip_legacy_nC;
extern unsigned char ferhip_legacy_bits[1 << 16];
extern unsigned int ferhip_legacy_nbits;
void quantizationTransform(int predL[16][16], int predCb[8][8], int predCr[8][8], unsigned char reconstruct);              /* F/quantizationTransform.cpp:349 */
void transformDecoding4x4LumaResidual(int LumaLevel[16][16], int predL[16][16], int luma4x4BlkIdx, int QPy);               /* F/inttransform.cpp:133 */
void transformDecodingIntra_16x16Luma(int Intra16x16DCLevel[16], int Intra16x16ACLevel[16][16], int predL[16][16], int QPy); /* :157 */
void transformDecodingP_Skip(int predL[16][16], int predCb[8][8], int predCr[8][8], int QPy);                              /* :215 */
void transformDecodingChroma(int ChromaDCLevel[4], int ChromaACLevel[4][16], int predC[8][8], int QPy, unsigned char Cb);  /* :237 */
void residual_block_cavlc_write(int coeffLevel[16], int startIdx, int endIdx, int maxNumCoeff);                            /* F/residual.cpp:374 */
unsigned int residual_block_cavlc_size(int coeffLevel[16], int startIdx, int endIdx, int maxNumCoeff);                     /* :673 */
void MotionCompensateSubMBPart(int predL[16][16], int predCr[8][8], int predCb[8][8], frame_type *refPic, int mbPartIdx, int subMbIdx,
                               int subMbPartIdx);                                                                         /* F/mocomp.cpp:152 */
void Decode(int predL[16][16], int predCr[8][8], int predCb[8][8]);                                                        /* :200 */
/* ---- the CAVLC seam in both directions, macroblock layer included (ferhip_cavlc_parse_blocks, ferhip_residual_mbs of
 * ferhip.h).  The block parser reads the ferhip_legacy_nbits bits of ferhip_legacy_bits at the cursor ferhip_legacy_bitpos
 * and advances it, with nC stated in ferhip_legacy_nC like the writer's; a malformed block (one that runs past the written
 * bits included) leaves the cursor alone, zeroes the block and prints the message.
 * residual_write() and residual(0, 15) derive nC themselves, from where the reference keeps the neighbours' state:
 * mb_type_array, CodedBlockPatternLumaArray / ChromaArray, totalcoeff_array_luma / _chroma (F/h264_globals.h:102-109,
 * 187-188), for macroblock CurrMbAddr of a picture `frame`.Lwidth wide, with CodedBlockPatternLuma / Chroma as its own
 * pattern.  As in the reference, the caller (setCodedBlockPattern, the macroblock-layer parser) stores mb_type and the
 * pattern of the macroblock in the arrays as well; the shims store its TotalCoeff.  AllocateMemory sizes the pattern
 * arrays from `frame`; the fixed-size arrays hold FERHIP_LEGACY_MAX_MBS macroblocks, as the reference's do.
 * TotalCoeff_luma_array / TotalCoeff_chroma_array of F/residual.h are not exported: the reference reads them in get_nC
 * (F/residual.cpp:111) alone, by sample position, and nothing calls that; what residual_write() and residual() read and
 * write is totalcoeff_array_*.  Only (0, 15) is supported by residual(); anything else prints the message and returns. */
#define FERHIP_LEGACY_MAX_MBS 10000
extern unsigned int ferhip_legacy_bitpos;
extern int CodedBlockPatternLuma, CodedBlockPatternChroma;                  /* F/h264_globals.cpp:171-172 */
extern int *CodedBlockPatternLumaArray, *CodedBlockPatternChromaArray;      /* [macroblock] */
extern int mb_type_array[FERHIP_LEGACY_MAX_MBS];
extern int totalcoeff_array_luma[FERHIP_LEGACY_MAX_MBS][16], totalcoeff_array_chroma[2][FERHIP_LEGACY_MAX_MBS][4];
void residual_block_cavlc(int coeffLevel[16], int startIdx, int endIdx, int maxNumCoeff); /* F/residual.cpp:1069 */
void residual_write(void);                                                                 /* :300 */
void residual(int startIdx, int endIdx);                                                   /* :959 */
/* ---- intra prediction and motion-vector derivation of one macroblock among its neighbours (ferhip_intra_mbs,
 * ferhip_mv_mbs of ferhip.h).  The shims cut the 3 x 2-macroblock neighbourhood of CurrMbAddr out of `frame` and of the
 * state arrays -- mb_type_array, CodedBlockPatternLumaArray / ChromaArray, totalcoeff_array_*, Intra4x4PredMode, mvL0x /
 * mvL0y -- and place the macroblock where it has exactly the neighbours it has in `frame`.  AllocateMemory sizes
 * Intra4x4PredMode ([macroblock << 4 | luma4x4BlkIdx]) and refIdxL0 ([macroblock]) from `frame` as well.
 * `unsigned char` stands for the reference's bool; ferhip_legacy_constrained_intra_pred = pps.constrained_intra_pred_flag.
 *   intraPredictionEncoding (F/intra.cpp:949), an I slice: `frame` holds the source at CurrMbAddr and the reconstruction
 *     around it, QPy the QP, mb_type_array[CurrMbAddr] the entry of the previous picture (the first coded_mb_size reads it).
 *     Returns the Intra16x16 mode or -1 (Intra4x4) and sets Intra4x4PredMode, intra_chroma_pred_mode, the flags and rem
 *     modes, the predictions and mb_type_array[CurrMbAddr] = 0; for -1 the luma of `frame` is the reconstruction and LumaLevel
 *     holds its levels.  ferhip_legacy_mbsize[2] = the two coded_mb_size values (F/rbsp_encoding.cpp:330) the function asked
 *     for: of the Intra16x16 and of the Intra4x4 alternative.
 *   intraPrediction (F/intra.cpp:770) with getIntra4x4PredMode, an I or P slice (ferhip_legacy_slice_type): mb_type, the
 *     flags and rem modes, intra_chroma_pred_mode, for Intra4x4 LumaLevel and QPy in; the predictions and, for Intra4x4,
 *     Intra4x4PredMode and the luma of `frame` out.  A mode that reads a neighbour the macroblock does not have is refused.
 *   DeriveMVs (F/mode_pred.cpp:428): mb_type (0..4, 31), sub_mb_type, mvd_l0[mbPartIdx][0] in; mvL0x / mvL0y [CurrMbAddr]
 *     and refIdxL0[CurrMbAddr] = 0 out.  A vector that leaves 16 bits is refused (the device keeps 16 bits).
 *   ClearMVD (F/mode_pred.cpp:41): mvd_l0 = 0.
 * For a `frame` one macroblock wide -- B without C and D, first and last column at once: no macroblock of a 3 x 2
 * neighbourhood is like that -- the three shims print the message and return (intraPredictionEncoding: 0). */
extern int *Intra4x4PredMode, *refIdxL0;
extern int intra_chroma_pred_mode;
extern unsigned char prev_intra4x4_pred_mode_flag[16];
extern int rem_intra4x4_pred_mode[16];
extern int mvd_l0[4][4][2];
extern int sub_mb_type[4];
extern int ferhip_legacy_constrained_intra_pred;
extern int ferhip_legacy_mbsize[2];
int intraPredictionEncoding(int predL[16][16], int predCr[8][8], int predCb[8][8]); /* F/intra.cpp:949 */
void intraPrediction(int predL[16][16], int predCr[8][8], int predCb[8][8]);        /* :770 */
void DeriveMVs(void);                                                               /* F/mode_pred.cpp:428 */
void ClearMVD(void);                                                                /* :41 */
/* Every shim above that takes CurrMbAddr checks it first: against the macroblocks of `frame`, or, where it indexes what
 * AllocateMemory sized, against the macroblock count of the last AllocateMemory.
 * What has no stand-alone shim, and why:
 *   - coded_mb_size (F/rbsp_encoding.cpp:330) under its own name: its value for arbitrary caller-made predictions is not
 *     something any kernel computes.  The two values the reference ever asks for -- inside intraPredictionEncoding -- are
 *     ferhip_legacy_mbsize[2] (mbsize[2] of ferhip_intra_result).
 *   - per-macroblock interEncoding: the serial chain k_me_resolve is not given a second entry; the lists it searches are
 *     pinned against the reference's, one 8x8 partition at a time, by tests/test_gpu_me_lists.py. */

#ifdef __cplusplus
}
#endif
#endif
