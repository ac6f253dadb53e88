// Host-side arithmetic of the packed picture formats (h264-fer_amd/csrc/fer_pic_host.h: FERHIP_FMT_YUY2, UYVY, BGRA, RGBA)
// as a stand-alone program, for a run under a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/csc_host_check.cpp -o csc_host_check && ./csc_host_check
// It checks the row bytes, the alignment rule and the other refusals of ferhip_set_pictures in a packed format, that nothing
// but plane[0] of an absent stream and nothing but plane[0] and pitch[0] of a present one is looked at, the layout rule of
// ferhip_decs_set_layout, and the slot sizes up to pitches and heights whose product passes 2^32.
// (tools/pic_host_check.cpp does the same for the planar formats.)
#include "../h264-fer_amd/csrc/fer_pic_host.h"
#include <stdio.h>
#include <vector>

static int fails = 0;
#define EXPECT(x)                                              \
    do {                                                       \
        if (!(x)) {                                            \
            printf("line %d: %s\n", __LINE__, #x);             \
            fails++;                                           \
        }                                                      \
    } while (0)

int main()
{
    alignas(16) static uint8_t mem[64];
    const int S = 3;
    for (int fmt : {FERHIP_FMT_YUY2, FERHIP_FMT_UYVY, FERHIP_FMT_BGRA, FERHIP_FMT_RGBA}) {
        const bool rgb = fmt == FERHIP_FMT_BGRA || fmt == FERHIP_FMT_RGBA;
        const uint32_t dw = 46, row = rgb ? 4 * dw : 2 * dw;
        EXPECT(fer_pic_packed(fmt) && fer_pic_packed_rgb(fmt) == rgb && fer_pic_packed422(fmt) == !rgb);
        EXPECT(fer_pic_row_bytes(fmt, dw) == row);
        EXPECT(fer_pic_row_bytes(fmt, 16384) == (rgb ? 65536u : 32768u));
        EXPECT(fer_pic_chroma_row(fmt, dw) == 0);  // one plane
        std::vector<ferhip_pic> p(S);  // exactly S descriptors on the heap: a read past them is an error
        // a present stream: the other planes and pitches are garbage that a planar format would refuse
        for (int s = 0; s < S; s++) p[s] = ferhip_pic{{mem + 4 * s, nullptr, (const void *)3}, {row + 4u * s, 1, 0}, 0};
        p[1] = ferhip_pic{{nullptr, (const void *)17, nullptr}, {3, 1, 0xffffffffu}, 77};  // absent: the rest is garbage
        EXPECT(fer_pic_check(p.data(), S, fmt, dw) == 0);
        EXPECT(fer_pic_check(nullptr, S, fmt, dw) == FERHIP_E_ARG);
        for (int bad : {2, 3, 6, 7, 10, -1}) EXPECT(fer_pic_check(p.data(), S, bad, dw) == FERHIP_E_ARG);
        std::vector<ferhip_pic> q;
        for (int o = 1; o < 4; o++) {
            q = p, q[2].plane[0] = mem + o;
            EXPECT(fer_pic_check(q.data(), S, fmt, dw) == FERHIP_E_ARG);
            q = p, q[0].pitch[0] = row + 4 + o;
            EXPECT(fer_pic_check(q.data(), S, fmt, dw) == FERHIP_E_ARG);
            EXPECT(fer_pic_layout_check(fmt, row + 4 + o, 0, dw) == FERHIP_E_ARG);
        }
        q = p, q[0].pitch[0] = row - 4;
        EXPECT(fer_pic_check(q.data(), S, fmt, dw) == FERHIP_E_ARG);
        q = p, q[2].reserved = 1;
        EXPECT(fer_pic_check(q.data(), S, fmt, dw) == FERHIP_E_ARG);
        q = p, q[0].pitch[0] = 0xfffffffcu;  // any larger multiple of 4
        EXPECT(fer_pic_check(q.data(), S, fmt, dw) == 0);
        EXPECT(fer_pic_layout_check(fmt, row, 0, dw) == 0);           // pitch_c is ignored
        EXPECT(fer_pic_layout_check(fmt, row, 0xffffffffu, dw) == 0);
        EXPECT(fer_pic_layout_check(fmt, row + 256, 3, dw) == 0);
        EXPECT(fer_pic_layout_check(fmt, row - 4, row, dw) == FERHIP_E_ARG);
        EXPECT(fer_pic_slot_bytes(fmt, row, 0, 38) == (size_t)row * 38);
        EXPECT(fer_pic_slot_bytes(fmt, row + 4, 0xffffffffu, 38) == (size_t)(row + 4) * 38);  // pitch_c is ignored
        EXPECT(fer_pic_slot_bytes(fmt, 0xfffffffcu, 0xfffffffcu, 16384) == (size_t)0xfffffffcu * 16384);
    }
    for (int bad : {2, 3, 6, 7, 10, -1}) {
        EXPECT(!fer_pic_packed(bad));
        EXPECT(fer_pic_layout_check(bad, 1024, 1024, 46) == FERHIP_E_ARG);
    }
    // the planar formats are as they were
    EXPECT(!fer_pic_packed(FERHIP_FMT_I420) && !fer_pic_packed(FERHIP_FMT_NV12));
    EXPECT(fer_pic_row_bytes(FERHIP_FMT_I420, 46) == 46 && fer_pic_row_bytes(FERHIP_FMT_NV12, 46) == 46);
    EXPECT(fer_pic_chroma_row(FERHIP_FMT_I420, 46) == 23 && fer_pic_chroma_row(FERHIP_FMT_NV12, 46) == 46);
    EXPECT(fer_pic_layout_check(FERHIP_FMT_I420, 47, 23, 46) == 0);  // odd pitches
    EXPECT(fer_pic_slot_bytes(FERHIP_FMT_NV12, 53, 51, 2) == 53u * 2 + 51);
    printf(fails ? "%d checks failed\n" : "csc_host_check ok\n", fails);
    return fails != 0;
}
