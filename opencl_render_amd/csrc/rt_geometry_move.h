// rt_geometry_move.h -- what rt_api.cpp hands to the device side of a geometry update (rtHipSceneSetGeometry): the grid build's core
// (rt_build_device.hip), which takes DEVICE vertex and index arrays and leaves planes, starts and list on the device, and the one kernel
// that is new (rt_geometry_move.hip): triangle records from new vertices with the words no update touches carried over.
#ifndef RT_GEOMETRY_MOVE_H
#define RT_GEOMETRY_MOVE_H

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime_api.h>

// Device storage of a grid build.  It belongs to whoever made it (zero-initialised; rt_grid_space_free releases it) and only ever grows:
// a buffer that is too small for a build is replaced by a larger one -- of needed + needed / 8 elements when `headroom` is set -- so that
// a later build that needs no more allocates nothing.  `allocated` is raised by every allocation (the owner clears it); `bytes` is what
// the space holds.
struct RtGridSpace {
    uint32_t fillGroups;   // big triangles filled at a time (bitmaps, test maps and queues of the workgroup fill), 1 .. 64
    int headroom;
    // fixed sizes
    float *bm;             // [257][4] split planes, lane 3 zero
    char *ctl;             // key cursor u64 | big-triangle bound u64 | big count u32 | overflow u32
    uint32_t *count;       // [256^3] entries per cell
    void *scanTmp; size_t scanBytes;
    uint32_t *bitmaps, *passmaps, *queues; // made when the first big triangle shows up
    uint64_t bitmapCap, passmapCap, queueCap; // in words
    int mapsDirty;         // a build failed between the big fills: the maps are cleared before the next one
    // by vertex count
    float *vals, *sorted; void *vSortTmp; size_t vSortBytes; uint64_t vCap;
    // by triangle count
    uint32_t *bigList; uint64_t tCap;
    // by pair count
    unsigned long long *keys, *keysSorted; void *kSortTmp; size_t kSortBytes; uint64_t keyCap;
    uint64_t bytes;
    int allocated;
};

// Return codes of the core: 0, -2 a HIP failure, -3 more pairs than listLimit, -4 no device memory, -7 a single fill outgrew its workgroup
// queue or the second fill overflowed too.
// The storage a build of V vertices and T triangles starts with (stage 1 calls it itself; a caller that times the build calls it first).
int rt_grid_space_reserve(RtGridSpace *space, uint32_t V, uint32_t T, uint64_t tunedKeyCap);
// Stage 1: planes, the fill of every triangle, leaving `*pairs` keys in the space.  log: RT_BUILD_LOG_* fields of the grid (raytrace_hip.h).
int rt_grid_core_fill(RtGridSpace *space, uint32_t V, uint32_t T, const void *dVertex, const void *dIndex, uint64_t tunedKeyCap, uint64_t listLimit,
                      hipStream_t stream, uint64_t *pairs, uint64_t *log);
// Stage 2: the keys sorted, starts [256^3 + 1] and list [pairs] written to the caller's device arrays.
int rt_grid_core_lists(RtGridSpace *space, uint64_t pairs, uint32_t *dStart, uint32_t *dList, hipStream_t stream);
void rt_grid_space_free(RtGridSpace *space);

// rt_geometry_move.hip: triRec / triShade rows of T triangles from new vertices -- rt_prepare_triangles' operations in its order -- with the
// UV and material words of the rows the scene holds (oldShade), and its corner normals too when triNormal is NULL.
extern "C" hipError_t rtg_launch_records(uint32_t T, const void *vertex, const void *triIndex, const void *triNormal, const float *oldShade,
                                         float *triRec, float *triShade, hipStream_t stream);

#endif
