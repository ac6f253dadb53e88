// ref_decode_main.cpp -- TEST INFRASTRUCTURE: a driver of our own around the reference's decoder translation units
// (linked where they lie by the `ref` target of oracle/Makefile into oracle/_ref/ref_decode; nothing of the reference is
// copied).  ref_decode IN.264 OUT.y4m decodes an Annex-B stream the way the reference's decode() does -- getNAL,
// RBSP_decode until a NAL unit comes back empty -- and leaves the Y4M file RBSP_decode writes.  The OpenCL symbols the
// decoder units name are stubbed: the CPU path (OpenCLEnabled == false) never calls them.
#include <stdio.h>
#include <stdlib.h>

#include "nal.h"
#include "fileIO.h"
#include "rbsp_decoding.h"
#include "residual_tables.h"

bool OpenCLEnabled = false;
int *predModes16x16 = 0, *predModes4x4 = 0;
static void never(const char *what)
{
    fprintf(stderr, "ref_decode: %s called on the CPU path\n", what);
    abort();
}
void AllocateFrameBuffersCL() {}
void IntraCL() { never("IntraCL"); }
void WaitIntraCL(int) { never("WaitIntraCL"); }
void subtractFramesCL(unsigned char *, unsigned char *) { never("subtractFramesCL"); }

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: ref_decode IN.264 OUT.y4m\n");
        return 2;
    }
    stream = fopen(argv[1], "rb");
    yuvoutput = fopen(argv[2], "wb");
    if (!stream || !yuvoutput) {
        perror("ref_decode");
        return 2;
    }
    generate_residual_level_tables();
    InitNAL();
    NALunit nu;
    nu.rbsp_byte = new unsigned char[500000];
    unsigned long ptr = 0;
    for (;;) {
        getNAL(&ptr, nu);
        if (nu.NumBytesInRBSP == 0) break;
        RBSP_decode(nu);
    }
    fclose(stream);
    fclose(yuvoutput);
    return 0;
}
