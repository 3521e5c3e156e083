// rt_host.h -- what the host translation units of libraytrace_hip.so share (rt_api.cpp: scenes, queries; rt_scene_parts.cpp: the builders
// of a scene's parts; rt_frame.cpp: the frame loop; rt_filters.cpp: the image-space filters; rt_matte.cpp: the mattes): the error text, the tuning values
// (rt_tuning.h), upload staging, and the resident scene itself.  Internal: nothing here is part of the C ABI of include/raytrace_hip.h.
#pragma once
#include "raytrace_hip.h"
#include "rt_device.h"
#include "rt_tuning.h"
#include "rt_frame_plan.h"
#include "rt_ray_clip.h"
#include "rt_camera_move.h"
#include "rt_geometry_move.h"
#include "rt_owned.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// Which render pass bits need the surface buffer
#define RT_SURF_BUF_BITS (RT_HIP_PASS_NORMAL | RT_HIP_PASS_ALBEDO)

namespace rthost {

// Internal functions are kept out of the library's exported symbols.
#define RT_INTERNAL __attribute__((visibility("hidden")))

// Sets this thread's error text (rtHipLastError) and returns -1.
RT_INTERNAL int fail(const char *fmt, ...);

#define HIP_OK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return rthost::fail("%s failed: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

// Host-to-device copies go through two pinned buffers (hipHostMalloc once per scene, RT_HIP_STAGE_MB each, default 32): the
// caller's arrays are pageable (new[] in render.cpp:1089-1123), and a pageable hipMemcpy is a synchronous bounce through the
// runtime's own small staging area.  Here the CPU fills one buffer (several threads for big pieces) while the DMA engine
// drains the other; copy() returns when the source has been read completely, so callers may free it at once.
struct Stager {
    hipStream_t stream = nullptr;
    char *buf[2] = { nullptr, nullptr };
    hipEvent_t done[2] = { nullptr, nullptr };
    bool used[2] = { false, false };
    size_t size = 0;
    int next = 0;
    // Pinning 2 x 32 MB costs 15-25 ms, more than the rest of an instance's build when its shared parts are copied from another
    // instance: the buffers are taken when the first host array needs them and go back to a process-wide pool, not to the driver.
    struct Pool {
        std::mutex lock;
        std::vector<std::pair<char *, size_t>> idle;
        char *take(size_t bytes)
        {
            {
                std::lock_guard<std::mutex> g(lock);
                for (size_t i = 0; i < idle.size(); ++i)
                    if (idle[i].second == bytes) { char *p = idle[i].first; idle.erase(idle.begin() + i); return p; }
            }
            char *p = nullptr;
            if (hipHostMalloc((void **)&p, bytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            return p;
        }
        void give(char *p, size_t bytes)
        {
            std::lock_guard<std::mutex> g(lock);
            if (idle.size() < 8) idle.emplace_back(p, bytes);
            else (void)hipHostFree(p);
        }
    };
    static Pool &pool() { static Pool *p = new Pool(); return *p; } // (never destroyed: buffers may come back during process exit)
    int init(hipStream_t st, const Tuning &T)
    {
        stream = st;
        size = (size_t)std::min<uint32_t>(std::max<uint32_t>(T.stageMb, 1u), 4096u) << 20;
        for (int i = 0; i < 2; ++i) HIP_OK(hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
        return 0;
    }
    static void fill(char *dst, const char *src, size_t n)
    {
        const size_t piece = (size_t)4 << 20;
        if (n < 2 * piece) { memcpy(dst, src, n); return; }
        const size_t parts = std::min<size_t>(8, n / piece);
        std::vector<std::thread> pool;
        for (size_t t = 1; t < parts; ++t) pool.emplace_back([=] { memcpy(dst + n * t / parts, src + n * t / parts, n * (t + 1) / parts - n * t / parts); });
        memcpy(dst, src, n / parts);
        for (auto &th : pool) th.join();
    }
    // is `p` device memory (a scene description may hand over arrays that are already on the GPU)?
    static bool on_device(const void *p)
    {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof at);
        if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; } // (plain host memory: "invalid value")
        return at.type == hipMemoryTypeDevice;
    }
    hipError_t copy(void *dst, const void *src, size_t bytes)
    {
        if (bytes && on_device(src)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream); // no staging: HBM to HBM
        for (size_t off = 0; off < bytes;) {
            const size_t n = std::min(size, bytes - off);
            const int i = next;
            next ^= 1;
            if (used[i]) { const hipError_t e = hipEventSynchronize(done[i]); if (e != hipSuccess) return e; }
            if (!buf[i] && !(buf[i] = pool().take(size))) return hipErrorOutOfMemory;
            fill(buf[i], (const char *)src + off, n);
            hipError_t e = hipMemcpyAsync((char *)dst + off, buf[i], n, hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) return e;
            e = hipEventRecord(done[i], stream);
            if (e != hipSuccess) return e;
            used[i] = true;
            off += n;
        }
        return hipSuccess;
    }
    hipError_t drain() // every copy so far has left its staging buffer; the buffers go back to the pool (the next instance's build takes them)
    {
        for (int i = 0; i < 2; ++i) {
            if (used[i]) { const hipError_t e = hipEventSynchronize(done[i]); if (e != hipSuccess) return e; used[i] = false; }
            if (buf[i]) { pool().give(buf[i], size); buf[i] = nullptr; }
        }
        return hipSuccess;
    }
    void destroy()
    {
        for (int i = 0; i < 2; ++i) {
            if (done[i]) { if (used[i]) (void)hipEventSynchronize(done[i]); (void)hipEventDestroy(done[i]); done[i] = nullptr; }
            if (buf[i]) { pool().give(buf[i], size); buf[i] = nullptr; }
        }
    }
};

} // namespace rthost

enum { PART_FIXED = 0, PART_CAMERA, PART_GEOMETRY, PART_GRID, PART_MATERIALS, PART_LIGHTS, PART_WAVEFRONT, PART_COUNT };

struct rtHipScene {
    int device = -1;
    rthost::Stream stream; // (declared before everything issued on it: destroyed last)
    RtDevScene dev{};
    // Device allocations by PART (tiles + outputs | camera lists | geometry | grid | materials | lights | path state): the drop-in
    // layer's cache replaces the parts whose inputs changed between two RaytraceAll calls and keeps the others in HBM.  A part's bytes
    // are counted in `bytes` by install and drop_part below, nowhere else (a peer instance copies the shared parts block by block).
    rthost::DevPart parts[PART_COUNT];
    rthost::Stager stager;
    uint32_t *prepErr = nullptr;   // device word: RT_PREP_ERR_* bits raised by the validation kernels
    uint64_t camListSize = 0;
    uint64_t gridListSize = 0;      // entries of the grid list = pair records of the dense view
    uint32_t gridListSizeHint = 0;  // scene description with device arrays: scenePixelTriangleListStart[256^3], fetched by scene_build
    bool haveGridListSize = false;
    // the clip bound of the grid in effect (rt_ray_clip.h): the planes kept {n.xyz, off}, and what the planes' buffer holds from RT_CLIP_AT
    // on (the count the kernels apply -- 0 with tune.rayClip off -- three pad words, the planes); clipKeys: the supports' read-back
    uint32_t clipCount = 0;
    float clipTail[4 + 4 * RT_CLIP_MAX_PLANES] = {};
    uint32_t clipKeys[RT_CLIP_CANDIDATES] = {};
    bool wfMultiLight = false;     // what the path-state buffers were sized for
    bool classMaterials = false, classLights = false; // the materials part / the lights part admit the opaque-diffuse path class
    uint64_t bytes = 0;
    std::vector<cl_uint> tileIds;
    uint32_t width = 0, height = 0, tilesX = 0;
    // kernel timing: one event pair per launch since the last rtHipKernelTime
    std::vector<std::pair<rthost::Event, rthost::Event>> events;
    size_t eventsUsed = 0;
    // wavefront pipeline (rt_wavefront.hip)
    int pipeline = RT_HIP_PIPELINE_WAVEFRONT;
    // The instance's tile slots are cut into contiguous GROUPS, each a view of `dev` (its own slice of tileIds, camStart/End,
    // tileBuf) with its own path state and stream.  A frame runs the groups concurrently: while one group is in a phase that
    // cannot fill the GPU (a round with few rays, a host read-back), the others' kernels do.  Per pixel nothing changes.
    struct Group {
        RtDevScene dev{};
        RtWavefront wf{};
        RtShadeList shade{};            // the split logic rounds' list of paths to shade (rt_device.h)
        rthost::Stream stream;          // groups 1.. ; group 0 runs on the caller's stream
        rthost::Event done;
        uint32_t logicBlocks = 1, traceBlocks = 1, queueBlocks = 1;
        rthost::Pinned<uint32_t> hostCount;  // pinned: queue length read back between round chunks
        rthost::Pinned<uint32_t> hostStatus; // pinned + mapped: RT_WF_STATUS_* words the kernels write (rt_device.h)
        bool ctlClean = false;          // the batch before was a planned one: wf_status_kernel left the control words zeroed
        uint32_t rounds = 0;
        uint32_t slot0 = 0, slot1 = 0;  // this group's range of the instance's tile slots
        // launch plan (render_wavefront): what the last discovery frame needed
        uint32_t roundsNeeded = 0;
        rthost::Pinned<uint4> hostLog;  // pinned + mapped: RtWavefront::roundLog, written by the kernels, read by the host after a sync
        rthost::RoundPlan plan[RT_WF_ROUND_LOG], planNext[RT_WF_ROUND_LOG]; // (rt_frame_plan.h)
        std::vector<RtRoundMode> modes; // how the rounds of the batch being issued are laid out (modes[r] is decided when logic(r-1) is launched)
        uint64_t guessRays = 0;         // watched batches: what the next round is assumed to hold
        rthost::PlaceStamp place[RT_WF_PLACE_ROUNDS + 1]; // per round: what its placement table on the device was recorded under (rt_frame_plan.h)
    };
    std::vector<Group> groups;
    rthost::Event forkEvent;
    uint32_t samplesPerBatch = 1;
    uint32_t planRounds = 0;   // rounds a planned frame issues per batch; 0 = no plan yet (the next frame is a discovery frame)
    uint64_t splitRoundsLast = 0; // logic rounds the last frame issued as answer + shade launches, over its batches and groups (rtHipTestShadeLog)
    uint32_t directRoundsLast = 0, scatterLaunchesLast = 0; // ordered rounds the last frame placed directly / scatter launches it issued, over its batches and groups (rtHipTestPlaceLog)
    bool placeSkewed = false;  // test hook place_skew: the one skew has been applied
    bool blocking = false;     // every frame watches the queue (no plan)
    rthost::Tuning tune;       // the tuning values this scene was built with (rtHipTune)
    bool unverified = false;   // planned frames were issued since the last frame_finish()
    hipStream_t lastStream = nullptr; // where the last frame was issued
    // sample windows (rtHipSceneSetSampleWindow): the window the next frame issued will use and the one the last issued frame used (all
    // zero before the first frame; a frame that is rendered again renders this one).  `dev` and the groups' views carry the window of the
    // frame issued last, or of the last set.
    rtHipSampleWindow window{}, lastWindow{};
    std::atomic<float> *progress = nullptr; // drop-in layer: where finished sample batches are reported (GetProgress, raytrace.c:566-587)
    float progressBase = 0.f, progressSpan = 0.f;
    // per-stage device time of the frames since the last query: [primary, logic, trace, accum, sort]
    struct StageEvent { int stage; rthost::Event a, b; };
    std::vector<StageEvent> stageEvents;
    size_t stageEventsUsed = 0;
    bool stageTiming = false;
    uint64_t roundsLast = 0;
    // test hook visit_log: per round of the last frame, the fields of rtHipTestRoundVisits (render_wavefront, log_round_visits)
    std::vector<std::array<uint64_t, RT_ROUND_VISIT_FIELDS>> visitLog;
    // render passes (rtHipScenePasses): RT_HIP_PASS_* bits, the pass buffer [slot][RT_PASS_WORDS][128*128] (rt_device.h) while ALPHA,
    // DEPTH or TRIANGLE is on, and the surface buffer [slot][RT_SURF_WORDS][128*128] while NORMAL or ALBEDO is on
    uint32_t passMask = 0;
    rthost::Dev<uint32_t> passBuf;
    rthost::Dev<float> surfBuf;
    // ray queries through host arrays (rtHipSceneIntersect): one chunk of hits | rays | excluded ids on the device and a pinned host buffer
    // of the same layout from the staging pool, both made on first use
    uint32_t queryRays = 0;
    rthost::Dev<> queryDev;
    char *queryHost = nullptr; // (queryDev.size bytes; goes back to the pool)
    // denoiser scratch of rtHipSceneDenoise (gathered inputs, filter scratch, outputs), made on first use while NORMAL and ALBEDO are on
    rthost::Dev<> denoiseBuf;
    // device time of the last rtHipSceneDenoise: events before the gather, after it, after the guides and after the output
    rthost::Event denoiseEv[4];
    float denoiseMs[3] = {};
    // ambient occlusion scratch (rtHipSceneAmbientOcclusion*), made on first use: the pixel counters, then one chunk of primary hits; the
    // event marks the end of the last call that used it, so that a call on another stream waits for it on the device
    rthost::Dev<> aoBuf;
    uint32_t aoChunk = 0;
    rthost::Event aoDone;
    // ambient occlusion bake scratch (rtHipSceneBakeAmbientOcclusion*), made on first use and grown for a larger map: winners, counters
    // and a second value plane for W*H texels, the big list, one chunk of texels; the event as above
    rthost::Dev<> bakeBuf;
    uint64_t bakeTexels = 0;
    uint32_t bakeChunk = 0;
    rthost::Event bakeDone;
    // motion vectors (rtHipSceneMotion*): the reference of the last rtHipSceneMotionMark -- its camera, and a, ab, ac of every triangle in
    // storage of its own (RT_MOTION_REF_ROWS float4 per triangle), made by the first mark -- and the host entry point's staging (tile-major
    // motion | t | prevT | triangle, 20 bytes per tile pixel), made on its first use.  marked: the end of the last mark on the scene's
    // stream; done: the end of the last call that read the reference or used the staging, on whatever stream it ran.
    struct Motion {
        bool have = false;
        rtHipCamera cam{};
        uint32_t triangles = 0;
        rthost::Dev<float4> ref;
        rthost::Dev<> stage;
        rthost::Event marked, done;
    } motion;
    // temporal accumulation (rtHipSceneTemporal), made on its first call in one block: two history sets (colour | count | t | triangle;
    // `cur` is the one the next call reads), this frame's motion and prevT, the gathered colour and the u16 output planes.  valid: the
    // history set `cur` holds a frame (false after a reset: the next call clears its counts first).
    // rtHipSceneTemporalVariance adds a block of its own on its first call: two sets of moments (they change places with the history
    // sets), the variance plane and the filter's il plane.  momentsValid: the moments set `cur` belongs to the history set `cur` (false
    // after an rtHipSceneTemporal, which does not write them).
    struct Temporal {
        rthost::Dev<> buf, momentsBuf;
        int cur = 0;
        bool valid = false, momentsValid = false;
        rthost::Event ev[5];
        float ms[4] = {};
        bool clampOn = false; // rtHipSceneSetTemporalClamp: the accumulation step runs the clamped kernel with `clamp`
        rtHipTemporalClampParams clamp = {};
    } temporal;
    // motion blur (rtHipSceneMotionBlur), made on its first call in one block: this frame's motion and t, the gathered colour, the blurred
    // image, the u16 output planes and the filter's scratch.  ev: before the motion pass, after it, after the gather, after the blur
    // and the output kernel; ms: the three spans of the last call.
    struct MotionBlur {
        rthost::Dev<> buf;
        rthost::Event ev[4];
        float ms[3] = {};
    } motionBlur;
    // depth of field (rtHipSceneDepthOfField), made on its first call in one block: the gathered colour and depth, the blurred image, the
    // u16 output planes and the filter's scratch.  ev: before the gather, after it, after the blur, after the output kernel; ms: the three
    // spans of the last call.
    struct DepthOfField {
        rthost::Dev<> buf;
        rthost::Event ev[4];
        float ms[3] = {};
    } dof;
    // camera moves (rtHipSceneSetCamera), made on the first move: the build scratch (slot tables, projected vertices, counts, big list,
    // control words, scan temporaries) in one block, and TWO sets of ranges + list -- a move builds into the set the frames do not read
    // and the sets change places at its end.  log: triangles per thread, per workgroup, entries of the last move; ms: device time of its
    // count stage and of its fill stage.
    struct CamMove {
        rthost::Dev<> scratch;
        rthost::Dev<uint32_t> start[2], end[2], list[2];
        int live = -1; // the set in use; -1 while the scene still renders from the lists it was created with
        RtCamMoveArgs args{};
        rthost::Event ev[4];
        uint64_t log[3] = {};
        double ms[2] = {};
    } cam;
    // geometry updates (rtHipSceneSetGeometry), made by the first update: TWO sets of everything the kernels read of the shape (triangle
    // records, shading rows, planes, cell table, grid starts and list, occupancy words, block table, pair records) -- an update builds into
    // the set the frames do not read and the sets change places at its end; the parts the scene was created with are freed after the
    // first update.  The rest is build scratch that stays: the grid build's space, staging for host arrays, two index arrays (the retained
    // one and the one being checked), the pair order.
    struct GeoMove {
        struct Set {
            rthost::Dev<float> triRec, triShade, boxMin, pairRec;
            rthost::Dev<uint8_t> cellLut;
            rthost::Dev<uint32_t> gridStart, gridList, sparse;
            rthost::Dev<unsigned long long> gridBits;
        } set[2];
        int live = -1;      // the set in use; -1 while the scene still renders from the parts it was created with
        RtGridSpace space{};
        rthost::Dev<> vertexBuf, normalBuf, index[2], denseTmp;
        rthost::Dev<int> material;
        rthost::Dev<uint32_t> pairOrder, pairInfo;
        int retained = -1;  // which index array the last successful update left; -1: none (creation drops the index array)
        rthost::Event ev[5];
        uint64_t log[6] = {}; // per thread, per workgroup, attempts, pairs, camera entries, allocated
        double ms[4] = {};
    } geo;
    // scene edits (rtHipSceneSetLights, rtHipSceneSetMaterials): staging for material ids that come from the host, made by the first
    // call that brings some; the events around the last edit's stages (light arrays | tables and atlas | id check | id store) and ms:
    // device time of the last successful edit's light arrays, tables and atlas, id check + id store
    struct Edit {
        rthost::Dev<int> ids;
        rthost::Event ev[6];
        double ms[3] = {};
    } edit;
    // mattes (rtHipSceneMattes*, rt_matte.cpp): the group table of rtHipSceneSetMatteGroups (one id per triangle, storage of the scene's
    // own) and the per-pixel state [slot][words][128*128] u32, made by the first call and grown when a call needs more words per pixel.
    // ev: before the last call's first count launch, after its last one, after its finish kernel -- the last one also marks the end of
    // the last call that used the state or read the table, on whatever stream it ran.  issued: the events have been recorded.
    struct Matte {
        rthost::Dev<uint32_t> groups, state;
        uint32_t words = 0;
        rthost::Event ev[3];
        bool issued = false;
    } matte;

    // Only what ordering requires: the device is selected, work on the streams ends, then the grid build's space, the upload staging and
    // the pooled query staging go; every member above, the parts among them, frees itself afterwards.
    ~rtHipScene()
    {
        if (device >= 0) (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (Group &G : groups)
            if (G.stream) (void)hipStreamSynchronize(G.stream);
        rt_grid_space_free(&geo.space);
        stager.destroy();
        if (queryHost) rthost::Stager::pool().give(queryHost, queryDev.size);
    }

    // `count` elements (one at least) as a new block of `part`, a part being built: not the scene's, and not counted, before install
    template <class T> int alloc(rthost::DevPart &part, uint64_t count, T **dst)
    {
        void *p = nullptr;
        const hipError_t e = part.get(&p, (count ? count : 1) * sizeof(T));
        if (e != hipSuccess) return rthost::fail("hipMalloc(&p, n * sizeof(T)) failed: %s", hipGetErrorString(e));
        *dst = (T *)p;
        return 0;
    }
    // ... filled from `src` (host or device memory) through the stager
    template <class T> int upload(rthost::DevPart &part, const T *src, uint64_t count, const T **dst, const char *what)
    {
        T *p = nullptr;
        if (alloc(part, count, &p)) return -1;
        if (count) {
            if (!src) return rthost::fail("%s: null pointer with %llu elements", what, (unsigned long long)count);
            HIP_OK(stager.copy(p, src, count * sizeof(T)));
        }
        *dst = p;
        return 0;
    }
    // The two places a part's bytes enter and leave rtHipSceneBytes.  Work on the scene's stream may still read a part that goes.
    void drop_part(int part)
    {
        if (parts[part].empty()) return;
        if (stream) (void)hipStreamSynchronize(stream);
        bytes -= parts[part].bytes;
        parts[part].clear();
    }
    void install(int part, rthost::DevPart &&fresh)
    {
        drop_part(part);
        bytes += fresh.bytes;
        parts[part] = std::move(fresh);
    }
    // looks at the device-side validation word (after the caller's stream synchronisation)
    int check_prep()
    {
        uint32_t err = 0;
        HIP_OK(hipMemcpy(&err, prepErr, 4, hipMemcpyDeviceToHost));
        if (!err) return 0;
        HIP_OK(hipMemset(prepErr, 0, 4));
        return rthost::fail("scene rejected (0x%x):%s%s%s%s%s%s", err,
                    (err & RT_PREP_ERR_TRI_INDEX) ? " a triangle references a vertex that does not exist;" : "",
                    (err & RT_PREP_ERR_TRI_MATERIAL) ? " a triangle uses a material >= materialCount;" : "",
                    (err & RT_PREP_ERR_CAM_ENTRY) ? " a camera list entry is not a triangle;" : "",
                    (err & RT_PREP_ERR_CAM_RANGE) ? " a camera list range exceeds the list size;" : "",
                    (err & RT_PREP_ERR_GRID_MONOTONE) ? " scenePixelTriangleListStart is not monotone;" : "",
                    (err & RT_PREP_ERR_GRID_ENTRY) ? " a grid list entry is not a triangle;" : "");
    }
};

namespace rthost {

// Scene scratch of `bytes` bytes, counted in rtHipSceneBytes, and an event: made, or fail() in the name of `who`.
inline int scene_block(rtHipScene *sc, DevBlock &b, uint64_t bytes, const char *who)
{
    const hipError_t e = b.make(bytes, sc->bytes);
    return e == hipSuccess ? 0 : fail("%s: hipMalloc(%llu) failed: %s", who, (unsigned long long)bytes, hipGetErrorString(e));
}
inline int scene_event(Event &ev, unsigned flags, const char *who)
{
    const hipError_t e = ev.make(flags);
    return e == hipSuccess ? 0 : fail("%s: hipEventCreate failed: %s", who, hipGetErrorString(e));
}

// Sample windows (include/raytrace_hip.h, "SAMPLE WINDOWS").  The default window of a scene of S samples:
inline rtHipSampleWindow default_window(uint32_t S) { return rtHipSampleWindow{ S, 0u, S, 0u, 0u }; }
inline bool same_window(const rtHipSampleWindow &a, const rtHipSampleWindow &b)
{
    return a.total == b.total && a.first == b.first && a.divisor == b.divisor && a.accumulate == b.accumulate && a.advance == b.advance;
}
// Does a frame under `w` follow on what the tile buffer holds?  (Such a frame cannot be rendered again: it is issued watched.)
inline bool window_continues(const rtHipSampleWindow &w) { return w.accumulate == 1u && w.first > 0u; }
// `w` becomes the window of the scene's device description and of every tile group's copy of it (RtDevScene travels by value): host
// words only, picked up by the next launch.
inline void apply_window(rtHipScene *sc, const rtHipSampleWindow &w)
{
    auto put = [&](RtDevScene &D) {
        D.seedStride = w.total; D.sampleFirst = w.first; D.sampleDivisor = w.divisor;
        D.continuesFrame = window_continues(w) ? 1u : 0u;
        D.directStore = (D.sampleCount == 1u && !D.continuesFrame) ? 1u : 0u;
    };
    put(sc->dev);
    for (auto &G : sc->groups) put(G.dev);
}

// bytes of the fixed-size arrays of a grid (rtHipScene::GeoMove::Set)
constexpr uint64_t GEO_PLANE_BYTES = RT_CLIP_FLOATS * 4 /* (the planes and the clip bound behind them, rt_ray_clip.h) */, GEO_LUT_BYTES = 3 * 256, GEO_START_BYTES = ((uint64_t)RT_GRID_DIV * RT_GRID_DIV * RT_GRID_DIV + 1) * 4,
                   GEO_BITS_BYTES = (uint64_t)(RT_GRID_DIV / 4) * (RT_GRID_DIV / 4) * (RT_GRID_DIV / 4) * 8,
                   GEO_SPARSE_BYTES = (uint64_t)3 * ((63u << 16 | 63u << 8 | 63u) + 1u) * 4;

// rt_scene_parts.cpp: the part builders (0, or -1 with the error text set: the caller destroys the scene), what follows a rebuilt
// part, and the arithmetic a scene build shares with the moves and edits of rt_api.cpp
RT_INTERNAL int build_fixed(rtHipScene *sc, const rtHipSceneDesc *d, const cl_uint *tileIds, cl_uint tileCount);
RT_INTERNAL int build_camera(rtHipScene *sc, const rtHipSceneDesc *d);
RT_INTERNAL int build_geometry(rtHipScene *sc, const rtHipSceneDesc *d);
RT_INTERNAL int build_grid(rtHipScene *sc, const rtHipSceneDesc *d);
RT_INTERNAL int build_materials(rtHipScene *sc, const rtHipSceneDesc *d);
RT_INTERNAL int build_lights(rtHipScene *sc, const rtHipSceneDesc *d);
RT_INTERNAL int build_wavefront(rtHipScene *sc, uint32_t sampleCount);
RT_INTERNAL int clone_part(rtHipScene *dst, const rtHipScene *src, int part);
RT_INTERNAL int scene_build(rtHipScene *sc, const rtHipSceneDesc *d, const cl_uint *tileIds, cl_uint tileCount, const rtHipScene *like, const Tuning &tune);
RT_INTERNAL void refresh_views(rtHipScene *sc);
RT_INTERNAL void derive_path_class(rtHipScene *sc);
RT_INTERNAL bool materials_admit_opaque_diffuse(const rtHipSceneDesc *d);
RT_INTERNAL bool lights_admit_opaque_diffuse(const rtHipSceneDesc *d);
RT_INTERNAL std::vector<uint32_t> material_records(const rtHipSceneDesc *d);
RT_INTERNAL std::vector<float> light_spreads(uint32_t count, const cl_float3 *dir, const cl_float *radius);
RT_INTERNAL void grid_tables(const float *planes, uint8_t *lut, uint32_t *tame);
RT_INTERNAL void clip_buffer_init(const float *planes, float *buffer);
RT_INTERNAL hipError_t clip_bound_issue(rtHipScene *sc, const unsigned long long *words, float *boxMin, hipStream_t st);
RT_INTERNAL hipError_t clip_bound_commit(const rtHipScene *sc, const float *planes, float *boxMin, hipStream_t st, uint32_t *count, float *tail);
// rt_frame.cpp
RT_INTERNAL int render_wavefront(rtHipScene *sc, hipStream_t st, bool forceDiscovery);
RT_INTERNAL int frame_finish(rtHipScene *sc, hipStream_t st, int *redone);
// rt_api.cpp
RT_INTERNAL int query_pointer_ok(int device, const char *whose, const void *p, uint64_t bytes, uint64_t align, const char *what);
RT_INTERNAL int motion_run(rtHipScene *sc, void *motion, void *t, void *prevT, void *triangle, bool rowMajor, hipStream_t st);
RT_INTERNAL Tuning tuning_now(); // a snapshot of the tuning values as rtHipTune left them: an entry point's one look at them

} // namespace rthost
