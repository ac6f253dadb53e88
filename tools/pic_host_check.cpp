// Host-side arithmetic of the picture descriptors (h264-fer_amd/csrc/fer_pic_host.h) as a stand-alone program, for a run
// under a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/pic_host_check.cpp -o pic_host_check && ./pic_host_check
// It checks the four refusals of ferhip_set_pictures, that nothing but plane[0] of an absent stream is looked at, and the
// slot sizes of ferhip_decs_set_layout up to pitches and heights whose product passes 2^32.
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
    static uint8_t mem[64];
    const int S = 3;
    for (int fmt : {FERHIP_FMT_I420, FERHIP_FMT_NV12}) {
        const uint32_t dw = 46, crow = fmt == FERHIP_FMT_NV12 ? dw : dw / 2;
        std::vector<ferhip_pic> p(S);  // exactly S descriptors on the heap: a read past them is an error
        for (int s = 0; s < S; s++) p[s] = ferhip_pic{{mem, mem + 1, mem + 2}, {dw, crow, crow}, 0};
        p[1] = ferhip_pic{{nullptr, (const void *)16, nullptr}, {0, 1, 0xffffffffu}, 77};  // absent: the rest is garbage
        EXPECT(fer_pic_check(p.data(), S, fmt, dw) == 0);
        EXPECT(fer_pic_check(p.data(), S, 2, dw) == FERHIP_E_ARG);
        EXPECT(fer_pic_check(p.data(), S, -1, dw) == FERHIP_E_ARG);
        EXPECT(fer_pic_check(nullptr, S, fmt, dw) == FERHIP_E_ARG);
        std::vector<ferhip_pic> q = p;
        q[2].reserved = 1;
        EXPECT(fer_pic_check(q.data(), S, fmt, dw) == FERHIP_E_ARG);
        q = p, q[0].pitch[0] = dw - 1;
        EXPECT(fer_pic_check(q.data(), S, fmt, dw) == FERHIP_E_ARG);
        q = p, q[2].pitch[1] = crow - 1;
        EXPECT(fer_pic_check(q.data(), S, fmt, dw) == FERHIP_E_ARG);
        q = p, q[2].plane[1] = nullptr;
        EXPECT(fer_pic_check(q.data(), S, fmt, dw) == FERHIP_E_ARG);
        q = p, q[0].plane[2] = nullptr, q[0].pitch[2] = 0;  // the third plane matters for I420 only
        EXPECT(fer_pic_check(q.data(), S, fmt, dw) == (fmt == FERHIP_FMT_I420 ? FERHIP_E_ARG : 0));
        q = p, q[0].pitch[0] = 0xffffffffu, q[0].pitch[1] = 0xfffffffdu;  // any larger pitch, odd included
        EXPECT(fer_pic_check(q.data(), S, fmt, dw) == 0);
        EXPECT(fer_pic_layout_check(fmt, dw, crow, dw) == 0);
        EXPECT(fer_pic_layout_check(fmt, dw - 1, crow, dw) == FERHIP_E_ARG);
        EXPECT(fer_pic_layout_check(fmt, dw, crow - 1, dw) == FERHIP_E_ARG);
        EXPECT(fer_pic_layout_check(7, dw, crow, dw) == FERHIP_E_ARG);
    }
    EXPECT(fer_pic_slot_bytes(FERHIP_FMT_I420, 50, 25, 38) == 50u * 38 * 3 / 2);
    EXPECT(fer_pic_slot_bytes(FERHIP_FMT_NV12, 50, 50, 38) == 50u * 38 * 3 / 2);
    EXPECT(fer_pic_slot_bytes(FERHIP_FMT_I420, 256, 256, 38) == 256u * 38 + 2u * 256 * 19);
    EXPECT(fer_pic_slot_bytes(FERHIP_FMT_NV12, 53, 51, 2) == 53u * 2 + 51);
    EXPECT(fer_pic_slot_bytes(FERHIP_FMT_I420, 0xffffffffu, 0xffffffffu, 16384) == (size_t)0xffffffffu * 16384 * 2);
    EXPECT(fer_pic_slot_bytes(FERHIP_FMT_NV12, 0xffffffffu, 0xffffffffu, 16384) == (size_t)0xffffffffu * 16384 * 3 / 2);
    printf(fails ? "%d checks failed\n" : "pic_host_check ok\n", fails);
    return fails != 0;
}
