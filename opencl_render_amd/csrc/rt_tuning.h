// rt_tuning.h -- the tuning values and test hooks of libraytrace_hip.so.  No HIP header: the frame planner (rt_frame_plan.h) and its
// stand-alone test (tests/frame_plan_host.cpp) read them too.
#pragma once
#include "raytrace_hip.h"

#include <stdint.h>

namespace rthost {

// Tuning values and test hooks.  The library reads NO environment variables: a plugin host's environment must not be able to
// make frames slower, redo themselves or fail.  Everything here is set through rtHipTune() (include/raytrace_hip.h, test / tuning
// entry point; the Python stub maps RT_* variables of ITS process onto it for the sweep scripts) and applies to scenes built
// afterwards.
struct Tuning {
    uint32_t stageMb = 32;          // size of each of the two pinned staging buffers of an upload
    uint32_t extraFactor = 6;       // region B of the entry arrays (further segments of cut rays), in units of the path capacity
    uint64_t stateMb = 0;           // path-state budget per sample batch (0 = 24 GB, never more than a third of free memory); tests force several batches
    uint32_t groups = 1;            // concurrent tile groups per instance (measured: no gain once rays are cut into segments)
    uint32_t lookAhead = 1;         // 0: one ray in flight per path
    uint32_t segLen[5] = { 4096u, 384u, 96u, 64u, 16u }; // aimed-at cell visits per segment for rounds with >= segRays[0] | [1] | [2] | [3] | fewer rays
    uint32_t segRays[4] = { 700000u, 300000u, 100000u, 30000u };
    uint32_t fastQuotient = 1;
    uint32_t spinLimit = 16384;     // a ray makes at most 766 cell visits = 154 walk phases; lowered by the test of the guard's error path
    uint32_t appendRays = 300000;   // later rounds with fewer rays are not ordered: the trace kernel plans and cuts their rays itself (RtRoundMode)
    uint32_t orderedFirst = 1;      // 0: round 1 follows the same rule (tests: the trace kernel's planning on dense rounds)
    uint32_t sliceRays = 0;         // rounds with fewer rays use smallSlices queue slices per kind instead of RT_WF_SHARDS (off: a round's appends want
                                    // many counters -- 16 slices cost the logic kernel of a 58 k-ray round 17 us -- and the trace kernel packs its pieces anyway)
    uint32_t smallSlices = 16;
    uint32_t groupRays = 0;         // rays per workgroup of the trace kernel in rounds that are not ordered (0 = by segment length)
    uint32_t blocking = 0;          // 1: every frame watches its queue (no launch plan)
    uint32_t planRounds = 0;        // test hook: planned frames issue at most this many rounds, so that the too-short-plan path runs
    uint32_t planGridTiny = 0;      // test hook: planned trace grids of one workgroup, so that the too-small-grid path runs
    uint32_t planShadeSkip = 0;     // test hook: planned frames launch no shade pass (as if the plan's shade lists were empty), so that the listed-but-skipped path runs
    uint32_t visitLog = 0;          // test hook: every frame waits after each round's trace launch and the host reads the round back (rtHipTestRoundVisits)
    uint32_t pipeline = RT_HIP_PIPELINE_WAVEFRONT;
    uint32_t timing = 0;            // 1: where the time of a scene build / a RaytraceAll call goes (stderr)
    uint32_t virtualDevices = 0;    // test hook: the all-GPUs id deals the tiles over this many instances on the devices that are there
    uint32_t cache = 1;             // 0: RaytraceAll builds and frees per call, like the reference
    uint32_t batchPlan = 1;         // 1: the sample batches after a watched frame's first are issued from that batch's launch plan
    uint32_t logicClass = 1;        // 0: every scene's paths run on the general logic kernel; 1: the kernel of the scene's path class (path_class_of)
    uint32_t deadShadow = 1;        // 0: trace every shadow ray, also those whose answer only feeds the face[] entry that is never read
    uint32_t rayClip = 1;           // 1: grid rays without a far end stop where they leave the scene's clip bound (rt_ray_clip.h); 0: at the grid's wall
    uint32_t logicSplit = 1;        // 1: rounds >= 1 of the opaque-diffuse class (look-ahead on) run wf_answer_kernel + wf_shade_kernel; 0: wf_logic_kernel
    uint32_t placeDirect = 1;       // 1: a planned frame's ordered rounds that qualify (rt_frame_plan.h, round_goes_direct) are placed by the logic kernel
                                    // from the round's placement table and run no wf_scatter_kernel; 0: every ordered round is scattered
    uint32_t placeSkew = 0;         // test hook: once per scene, the first placement table a round is about to be placed by is skewed by one entry
                                    // between two cells (wf_place_skew_kernel), so that the guard, the flagged frame and its remedy run
    uint64_t buildKeyCap = 0;      // test hook: first key capacity of the device grid build (0 = max(32 T, 2^22)), so that its grow and refill paths run
    uint64_t buildListLimit = 0xffffffffull; // test hook: most entries a device-built list may hold, so that the refusal above it runs
    uint32_t queryRays = 1u << 20;  // rays per staging chunk of rtHipSceneIntersect (52 bytes each, on the device and pinned on the host)
    uint32_t aoSamples = 1u << 20;  // pixel samples per chunk of the ambient occlusion calls (32 bytes each of scene-owned scratch)
    uint32_t bakeTexels = 1u << 20; // texels per chunk of the ambient occlusion bake (32 bytes each of scene-owned scratch)
    uint32_t matteChunk = 64;       // samples per launch of the matte count kernel (1..65536), read at the entry of every matte call
};

} // namespace rthost
