// fer_levels.h -- the level record of one macroblock (FerDev.levels), for device code (fer_dev.h) and for host code that
// packs it without the HIP runtime (fer_seam_pack_host.h).
#pragma once
#define FER_LEVELS 400   // int16 per MB: luma 16x16, dc16 16, cdc 2x4, cac 2x4x15
#define FER_LV_DC16 256
#define FER_LV_CDC 272
#define FER_LV_CAC 280
