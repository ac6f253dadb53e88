// fer_pic_host.h -- host-side arithmetic of the picture descriptors (ferhip_set_pictures, ferhip_get_recon_pictures,
// ferhip_decs_set_layout): validation and slot sizes.  Plain C++ without the HIP runtime, so that it can be compiled
// into a stand-alone host program and run under a sanitizer (tools/pic_host_check.cpp, and tools/csc_host_check.cpp for the
// packed formats).
#pragma once
#include "../../include/ferhip.h"
#include <stddef.h>
#include <stdint.h>

// the packed formats: one plane of 2 (4:2:2) or 4 (RGB) bytes per pixel, converted on the way in and out
static inline bool fer_pic_packed422(int format) { return format == FERHIP_FMT_YUY2 || format == FERHIP_FMT_UYVY; }
static inline bool fer_pic_packed_rgb(int format) { return format == FERHIP_FMT_BGRA || format == FERHIP_FMT_RGBA; }
static inline bool fer_pic_packed(int format) { return fer_pic_packed422(format) || fer_pic_packed_rgb(format); }

// bytes of one row of plane[0] of a picture dw samples wide (dw is below 2^24, so 4 * dw fits)
static inline uint32_t fer_pic_row_bytes(int format, uint32_t dw) { return fer_pic_packed_rgb(format) ? 4u * dw : fer_pic_packed422(format) ? 2u * dw : dw; }

// bytes of one chroma row of a picture dw samples wide; a packed format has no chroma plane
static inline uint32_t fer_pic_chroma_row(int format, uint32_t dw) { return fer_pic_packed(format) ? 0u : format == FERHIP_FMT_NV12 ? dw : dw / 2u; }

// a packed picture: plane[0] and pitch[0] alone, both multiples of 4, the pitch not below the row's bytes
static inline int fer_pic_check_packed(const ferhip_pic *pics, int S, int format, uint32_t dw)
{
    const uint32_t row = fer_pic_row_bytes(format, dw);
    for (int s = 0; s < S; s++) {
        const ferhip_pic &p = pics[s];
        if (!p.plane[0]) continue;
        if (p.reserved != 0 || ((uintptr_t)p.plane[0] & 3u) || (p.pitch[0] & 3u) || p.pitch[0] < row) return FERHIP_E_ARG;
    }
    return 0;
}

// [S] descriptors of pictures dw samples wide: 0, or FERHIP_E_ARG for an unknown format, and in a present stream
// (plane[0] != NULL) a pitch below the row's bytes, a NULL chroma plane or reserved != 0; in a packed format a plane[0] or
// pitch[0] that is no multiple of 4.  Nothing but plane[0] of an absent stream is looked at.
static inline int fer_pic_check(const ferhip_pic *pics, int S, int format, uint32_t dw)
{
    if (pics && fer_pic_packed(format)) return fer_pic_check_packed(pics, S, format, dw);
    if (!pics || (format != FERHIP_FMT_I420 && format != FERHIP_FMT_NV12)) return FERHIP_E_ARG;
    const int nplanes = format == FERHIP_FMT_NV12 ? 2 : 3;
    const uint32_t crow = fer_pic_chroma_row(format, dw);
    for (int s = 0; s < S; s++) {
        const ferhip_pic &p = pics[s];
        if (!p.plane[0]) continue;
        if (p.reserved != 0 || p.pitch[0] < dw) return FERHIP_E_ARG;
        for (int k = 1; k < nplanes; k++)
            if (!p.plane[k] || p.pitch[k] < crow) return FERHIP_E_ARG;
    }
    return 0;
}

// the layout of the live decoder's output slots: 0 when the pitches hold a row of a window dw wide
static inline int fer_pic_layout_check(int format, uint32_t pitch_y, uint32_t pitch_c, uint32_t dw)
{
    if (fer_pic_packed(format)) return (pitch_y & 3u) == 0u && pitch_y >= fer_pic_row_bytes(format, dw) ? 0 : FERHIP_E_ARG;  // pitch_c is ignored
    if (format != FERHIP_FMT_I420 && format != FERHIP_FMT_NV12) return FERHIP_E_ARG;
    return pitch_y >= dw && pitch_c >= fer_pic_chroma_row(format, dw) ? 0 : FERHIP_E_ARG;
}

// bytes of one slot: Y takes pitch_y * dh, each chroma plane pitch_c * dh / 2 (I420 has two of them, NV12 one); a packed
// format has its one plane of pitch_y * dh
static inline size_t fer_pic_slot_bytes(int format, uint32_t pitch_y, uint32_t pitch_c, uint32_t dh)
{
    if (fer_pic_packed(format)) return (size_t)pitch_y * dh;
    return (size_t)pitch_y * dh + (size_t)(format == FERHIP_FMT_NV12 ? 1 : 2) * pitch_c * (dh / 2u);
}
