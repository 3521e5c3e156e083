// rt_camera_move.h -- what rt_api.cpp hands to the resident camera build (rt_camera_move.hip).  Every pointer is device memory of the
// scene; `pixels` = tileCount * 128 * 128 tile-major pixels.
#ifndef RT_CAMERA_MOVE_H
#define RT_CAMERA_MOVE_H

#include <stddef.h>
#include <stdint.h>

#define RTC_NO_SLOT 0xffffffffu

struct RtCamMoveCtl { unsigned long long total; uint32_t bigCount, pad; }; // entries of the view; triangles handed to workgroups

struct RtCamMoveArgs {
    float eye[3], topLeft[3], lr[3], tb[3], pixelSizeInv;
    uint32_t width, height, tilesX, triangleCount, pixels;
    const float *triRec, *triShade;
    const uint32_t *slotOf;    // [tilesX * tilesY] tile id -> the instance's slot, or RTC_NO_SLOT
    const uint32_t *firstSlot; // [tileCount] the first slot with the same tile id; NULL when no tile id repeats
    void *pos;                 // [3 * triangleCount] projected vertices (rtbuild::F2)
    uint32_t *count;           // [pixels] entries per pixel, then the fill cursor
    uint32_t *bigList;         // [triangleCount]
    RtCamMoveCtl *ctl;
    void *scanTmp;
    size_t scanBytes;
    uint32_t *start, *end, *list; // the storage being built (not the one the scene renders from)
};

#endif
