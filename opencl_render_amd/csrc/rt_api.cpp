// rt_api.cpp -- host side of libraytrace_hip.so: the C ABI of include/raytrace_hip.h.
//
// Replaces the reference's dispatcher (source/opencl/raytrace.c): where that file creates 35 USE_HOST_PTR buffers,
// recompiles the kernel and enqueues tiles x samples NDRanges per call (raytrace.c:330-556), this one uploads the
// scene once into HBM, reshapes it on the device (rt_prepare_triangles) and issues ONE launch per frame and GPU.  The scene's parts are
// built in rt_scene_parts.cpp.
// There is no CPU fallback: without a HIP device every entry point that would compute fails with an error text.
#include "rt_host.h"
#include "rt_launch.h"
#include "rt_build_shared.h"
#include "rt_scene_edit.h"
#include "rt_tile_order.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <chrono>

using namespace rthost;

namespace {
thread_local std::string g_error;
}

int rthost::fail(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
    return -1;
}

namespace {

// Read at the entry points only (scene create, RaytraceAll, the two public device builders): a build works from one snapshot.
Tuning g_tune;
std::mutex g_tuneMutex;
Tuning tuning() { std::lock_guard<std::mutex> lock(g_tuneMutex); return g_tune; }

} // namespace

Tuning rthost::tuning_now() { return tuning(); }
rtbuild::DeviceBuildTuning rtbuild::device_build_tuning() { const Tuning t = tuning(); return { t.buildKeyCap, t.buildListLimit }; }

namespace {

// Scene edits (rtHipSceneSetLights, rtHipSceneSetMaterials below).
// An edit builds its part (PART_LIGHTS, PART_MATERIALS) beside the one in use: a local DevPart, freed when the edit fails, installed in
// the old part's place when it succeeds.  `count` elements (one at least) as a new block of it, filled from the host array `src` through
// the scene's stager: 0, -4 or -2
template <class T> int edit_put(rtHipScene *sc, DevPart &part, const T *src, uint64_t count, const T **dst, const char *who, const char *what)
{
    void *p = nullptr;
    const uint64_t n = (count ? count : 1) * sizeof(T);
    if (const hipError_t e = part.get(&p, n); e != hipSuccess) {
        fail("%s: no device memory for %s (%llu bytes): %s", who, what, (unsigned long long)n, hipGetErrorString(e));
        return -4;
    }
    if (count)
        if (const hipError_t e = sc->stager.copy(p, src, count * sizeof(T)); e != hipSuccess) {
            fail("%s: copying %s to the device failed: %s", who, what, hipGetErrorString(e));
            return -2;
        }
    *dst = (const T *)p;
    return 0;
}

} // namespace

// A device pointer a kernel may read or write `bytes` from: device memory of `device`, 16-byte aligned where the kernel loads 16 bytes at
// a time, and inside one allocation.  A host pointer must never reach a kernel: its fault takes the whole GPU down.
// `whose` names what lives on `device` in the error text ("the scene").  Declared in rt_host.h: the filters (rt_filters.cpp) call it too.
int rthost::query_pointer_ok(int device, const char *whose, const void *p, uint64_t bytes, uint64_t align, const char *what)
{
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return fail("%s %p is not device memory", what, p); }
    if (at.type != hipMemoryTypeDevice) return fail("%s %p is not device memory (memory type %d)", what, p, (int)at.type);
    if (at.device != device) return fail("%s %p is memory of device %d, %s is on device %d", what, p, at.device, whose, device);
    if ((uintptr_t)p % align) return fail("%s %p is not %llu-byte aligned", what, p, (unsigned long long)align);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return fail("%s %p: no allocation found", what, p); }
    if ((uint64_t)((const char *)p - (const char *)base) + bytes > (uint64_t)size)
        return fail("%s %p: %llu bytes reach past the end of its allocation", what, p, (unsigned long long)bytes);
    return 0;
}

// Enqueues the motion pass (rtHipSceneMotion*) on `st`, after the mark and after the last call's use of the reference and the staging.  Declared in rt_host.h: the temporal
// calls of rt_filters.cpp run it too.
int rthost::motion_run(rtHipScene *sc, void *motion, void *t, void *prevT, void *triangle, bool rowMajor, hipStream_t st)
{
    rtHipScene::Motion &M = sc->motion;
    RtMotionArgs A;
    for (int i = 0; i < 3; ++i) { A.eye[i] = M.cam.eye[i]; A.topLeft[i] = M.cam.eyeToTopLeft[i]; A.lr[i] = M.cam.leftToRight[i]; A.tb[i] = M.cam.topToBottom[i]; }
    A.ref = M.ref;
    A.motion = (float *)motion; A.t = (float *)t; A.prevT = (float *)prevT; A.triangle = (uint32_t *)triangle;
    A.rowMajor = rowMajor ? 1u : 0u; A.fastQuotient = sc->tune.fastQuotient ? 1u : 0u;
    if (st != sc->stream) HIP_OK(hipStreamWaitEvent(st, M.marked, 0));
    if (!rowMajor) HIP_OK(hipStreamWaitEvent(st, M.done, 0)); // (the staging)
    HIP_OK(rtw_launch_motion(&sc->dev, &A, st));
    HIP_OK(hipEventRecord(M.done, st));
    return 0;
}

namespace {

rtHipScene *scene_create(int device, const rtHipSceneDesc *desc, const cl_uint *tileIds, cl_uint tileCount, const rtHipScene *like, const Tuning &tune)
{
    g_error.clear();
    const int n = rtHipDeviceCount();
    if (n <= 0) { fail("no HIP device available: libraytrace_hip has no CPU fallback"); return nullptr; }
    if (device < 0 || device >= n) { fail("device %d out of range (%d HIP devices)", device, n); return nullptr; }
    rtHipScene *sc = new rtHipScene();
    sc->device = device;
    if (scene_build(sc, desc, tileIds, tileCount, like, tune) == 0) return sc;
    const std::string keep = g_error;
    rtHipSceneDestroy(sc);
    g_error = keep;
    return nullptr;
}

} // namespace

extern "C" {

int rtHipDeviceCount(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *rtHipLastError(void) { return g_error.c_str(); }

rtHipScene *rtHipSceneCreate(int device, const rtHipSceneDesc *desc, const cl_uint *tileIds, cl_uint tileCount)
{
    return rtHipSceneCreateLike(device, desc, tileIds, tileCount, nullptr);
}

rtHipScene *rtHipSceneCreateLike(int device, const rtHipSceneDesc *desc, const cl_uint *tileIds, cl_uint tileCount, const rtHipScene *like)
{
    return scene_create(device, desc, tileIds, tileCount, like, tuning());
}

void rtHipSceneDestroy(rtHipScene *sc)
{
    if (sc) delete sc;
}

uint64_t rtHipSceneBytes(const rtHipScene *sc) { return sc ? sc->bytes : 0; }

int rtHipSceneGetCamera(const rtHipScene *sc, rtHipCamera *out)
{
    if (!sc || !out) return fail("rtHipSceneGetCamera: null argument");
    const RtDevScene &D = sc->dev;
    memset(out, 0, sizeof *out);
    for (int i = 0; i < 3; ++i) { out->eye[i] = D.eye[i]; out->eyeToTopLeft[i] = D.topLeft[i]; out->leftToRight[i] = D.lr[i]; out->topToBottom[i] = D.tb[i]; }
    out->pixelSizeInv = D.pixelSizeInv;
    return 0;
}

// What changes a resident scene (camera moves, geometry updates, edits) reports a failed runtime call in the name of its entry point,
// `who` in the scope, and returns -2.
#define HIP_WHO(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { fail("%s: %s failed: %s", who, #expr, hipGetErrorString(e_)); return -2; } } while (0)

// What every such change starts with: work already issued reads the old state -- planned frames are verified (and redone, watched, if
// their plan was short) while it is still in effect, then the stream is idle.
static int change_begin(rtHipScene *sc, const char *who)
{
    HIP_WHO(hipSetDevice(sc->device));
    if (sc->unverified && frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, nullptr) != 0) return -2;
    HIP_WHO(hipStreamSynchronize(sc->stream));
    return 0;
}

// The scene-owned storage of camera moves, made by the first move: one scratch block and both sets of ranges.  The lists are sized by
// the move itself.  On failure nothing is kept.
static int cam_move_init(rtHipScene *sc)
{
    rtHipScene::CamMove &C = sc->cam;
    if (C.scratch) return 0;
    const RtDevScene &D = sc->dev;
    const uint32_t tilesX = sc->tilesX, tilesY = (sc->height + RT_TILE - 1) / RT_TILE, nt = (uint32_t)sc->tileIds.size();
    const uint64_t pixels = (uint64_t)nt * RT_TILE_PIXELS, T = D.triangleCount;
    if (pixels > 0x7fffffffull) { fail("rtHipSceneSetCamera: %llu tile pixels are more than the range scan takes", (unsigned long long)pixels); return -2; }
    std::vector<uint32_t> tables((size_t)tilesX * tilesY + nt, RTC_NO_SLOT);
    uint32_t *slotOf = tables.data(), *firstSlot = slotOf + (size_t)tilesX * tilesY;
    bool repeats = false;
    for (uint32_t i = 0; i < nt; ++i) {
        uint32_t &slot = slotOf[sc->tileIds[i]];
        if (slot == RTC_NO_SLOT) slot = i; else repeats = true;
        firstSlot[i] = slot;
    }
    size_t scanBytes = 0;
    if (const hipError_t e = rtc_scan_bytes((uint32_t)pixels, &scanBytes); e != hipSuccess) { fail("rtHipSceneSetCamera: sizing the scan failed: %s", hipGetErrorString(e)); return -2; }
    auto up = [](uint64_t v) { return (v + 255) & ~(uint64_t)255; };
    const uint64_t oTables = 0, oCtl = up(tables.size() * 4), oPos = oCtl + 256, oCount = oPos + up(T * 24), oBig = oCount + up(pixels * 4),
                   oScan = oBig + up(T * 4), total = oScan + up(scanBytes ? scanBytes : 1);
    // made here and handed to the scene -- and counted -- when all of it is there
    Dev<> block;
    Dev<uint32_t> r[4];
    Event ev[4];
    uint64_t uncounted = 0;
    const uint64_t rangeBytes = pixels ? pixels * 4 : 4;
    hipError_t e = block.make(total, uncounted);
    for (int i = 0; e == hipSuccess && i < 4; ++i) e = r[i].make(rangeBytes, uncounted);
    if (e == hipSuccess) e = hipMemcpy(block + oTables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice);
    for (int i = 0; e == hipSuccess && i < 4; ++i) e = ev[i].make();
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fail("rtHipSceneSetCamera: the build storage (%llu bytes) could not be made: %s", (unsigned long long)(total + 4 * rangeBytes), hipGetErrorString(e));
        return -4;
    }
    RtCamMoveArgs &A = C.args;
    A.width = sc->width; A.height = sc->height; A.tilesX = tilesX; A.triangleCount = D.triangleCount; A.pixels = (uint32_t)pixels;
    A.triRec = D.triRec; A.triShade = D.triShade;
    A.slotOf = (const uint32_t *)(block + oTables);
    A.firstSlot = repeats ? A.slotOf + (size_t)tilesX * tilesY : nullptr;
    A.ctl = (RtCamMoveCtl *)(block + oCtl); A.pos = block + oPos; A.count = (uint32_t *)(block + oCount); A.bigList = (uint32_t *)(block + oBig);
    A.scanTmp = block + oScan; A.scanBytes = scanBytes;
    C.scratch.adopt(std::move(block), sc->bytes);
    for (int i = 0; i < 2; ++i) {
        C.start[i].adopt(std::move(r[2 * i]), sc->bytes);
        C.end[i].adopt(std::move(r[2 * i + 1]), sc->bytes);
    }
    for (int i = 0; i < 4; ++i) C.ev[i] = std::move(ev[i]);
    return 0;
}

// One of the two lists made to hold `entries` entries (an eighth more than asked for, at least 1024, at most 2^32 - 1); an existing
// buffer is only ever replaced by a larger one; `exact`: of just `entries` entries (the other set's capacity).  The caller has made sure no work reads set `i`.
static bool cam_move_list(rtHipScene *sc, int i, uint64_t entries, bool exact = false)
{
    const uint64_t cap = exact ? entries : std::min<uint64_t>(std::max<uint64_t>(entries + entries / 8, 1024), 0xffffffffull);
    return sc->cam.list[i].fit(entries * 4, cap * 4, sc->bytes) == hipSuccess;
}

// The lists of camera `cam` over the triangles in triRec / triShade, built into the set the frames do not read (*target) on the idle
// stream of the scene and complete on return; nothing the scene renders from changes.  `who` names the entry point in error texts.
static int cam_move_build(rtHipScene *sc, const rtHipCamera *cam, const float *triRec, const float *triShade, uint64_t listLimit, const char *who,
                          int *target, RtCamMoveCtl *ctl, float ms[2])
{
    if (const int rc = cam_move_init(sc)) return rc;
    rtHipScene::CamMove &C = sc->cam;
    *target = C.live == 0 ? 1 : 0;
    RtCamMoveArgs A = C.args;
    A.triRec = triRec; A.triShade = triShade;
    for (int i = 0; i < 3; ++i) { A.eye[i] = cam->eye[i]; A.topLeft[i] = cam->eyeToTopLeft[i]; A.lr[i] = cam->leftToRight[i]; A.tb[i] = cam->topToBottom[i]; }
    A.pixelSizeInv = cam->pixelSizeInv;
    A.start = C.start[*target]; A.end = C.end[*target]; A.list = nullptr;
    HIP_WHO(hipEventRecord(C.ev[0], sc->stream));
    HIP_WHO(rtc_launch_count(&A, sc->stream));
    HIP_WHO(hipEventRecord(C.ev[1], sc->stream));
    HIP_WHO(hipMemcpyAsync(ctl, A.ctl, sizeof *ctl, hipMemcpyDeviceToHost, sc->stream)); // the only words that come back: 16 bytes
    HIP_WHO(hipStreamSynchronize(sc->stream));
    if (ctl->total > listLimit) {
        fail("%s: the view's lists hold %llu entries, more than the limit of %llu", who, ctl->total, (unsigned long long)listLimit);
        return -3;
    }
    if (!cam_move_list(sc, *target, ctl->total)) {
        fail("%s: no memory for a list of %llu entries", who, ctl->total);
        return -4;
    }
    A.list = C.list[*target];
    HIP_WHO(hipEventRecord(C.ev[2], sc->stream));
    HIP_WHO(rtc_launch_fill(&A, sc->stream));
    HIP_WHO(hipEventRecord(C.ev[3], sc->stream));
    HIP_WHO(hipStreamSynchronize(sc->stream));
    HIP_WHO(hipEventElapsedTime(&ms[0], C.ev[0], C.ev[1]));
    HIP_WHO(hipEventElapsedTime(&ms[1], C.ev[2], C.ev[3]));
    return 0;
}

// The view cam_move_build made takes the old one's place.
static void cam_move_commit(rtHipScene *sc, const rtHipCamera *cam, int target, const RtCamMoveCtl &ctl)
{
    rtHipScene::CamMove &C = sc->cam;
    RtDevScene &D = sc->dev;
    for (int i = 0; i < 3; ++i) { D.eye[i] = cam->eye[i]; D.topLeft[i] = cam->eyeToTopLeft[i]; D.lr[i] = cam->leftToRight[i]; D.tb[i] = cam->topToBottom[i]; }
    D.pixelSizeInv = cam->pixelSizeInv;
    D.camStart = C.start[target]; D.camEnd = C.end[target]; D.camList = C.list[target];
    sc->camListSize = ctl.total;
    C.live = target;
    sc->planRounds = 0; // other rays: the next frame watches its queue again
    refresh_views(sc);
    sc->drop_part(PART_CAMERA); // the lists the scene was created with (the first move only)
    // the other list is made as large as this one now, so that the next move to a view of no more entries allocates nothing; if that
    // fails the move has succeeded all the same and the next one tries again
    (void)cam_move_list(sc, target ^ 1, C.list[target].size / 4, true);
}

int rtHipSceneSetCamera(rtHipScene *sc, const rtHipCamera *cam)
{
    if (!sc || !cam) return fail("rtHipSceneSetCamera: null argument");
    const uint64_t listLimit = std::min<uint64_t>(tuning().buildListLimit, 0xffffffffull); // this entry point's one look at the tuning values
    if (const int rc = change_begin(sc, "rtHipSceneSetCamera")) return rc;
    int target = 0;
    RtCamMoveCtl ctl{};
    float ms[2] = { 0.f, 0.f };
    if (const int rc = cam_move_build(sc, cam, sc->dev.triRec, sc->dev.triShade, listLimit, "rtHipSceneSetCamera", &target, &ctl, ms)) return rc;
    // the new view is complete: it takes the old one's place
    cam_move_commit(sc, cam, target, ctl);
    rtHipScene::CamMove &C = sc->cam;
    C.log[0] = sc->dev.triangleCount - ctl.bigCount; C.log[1] = ctl.bigCount; C.log[2] = ctl.total;
    C.ms[0] = ms[0]; C.ms[1] = ms[1];
    return 0;
}

int rtHipTestSceneCameraList(const rtHipScene *sc, uint64_t first, uint64_t count, cl_uint *out)
{
    if (!sc) return fail("rtHipTestSceneCameraList: null scene");
    if (sc->camListSize > 0x7fffffffull) return fail("rtHipTestSceneCameraList: the list has %llu entries", (unsigned long long)sc->camListSize);
    if (!out) return (int)sc->camListSize;
    if (first > sc->camListSize || count > sc->camListSize - first)
        return fail("rtHipTestSceneCameraList: entries %llu + %llu reach past the %llu of the list", (unsigned long long)first, (unsigned long long)count,
                    (unsigned long long)sc->camListSize);
    if (!count) return 0;
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipStreamSynchronize(sc->stream));
    HIP_OK(hipMemcpy(out, sc->dev.camList + first, count * 4, hipMemcpyDeviceToHost));
    return 0;
}

int rtHipTestScenePointers(const rtHipScene *sc, const void *out[6])
{
    if (!sc || !out) return fail("rtHipTestScenePointers: null argument");
    const RtDevScene &D = sc->dev;
    out[0] = D.triRec; out[1] = D.triShade; out[2] = D.gridBlockSparse; out[3] = D.pairRec; out[4] = D.matRec; out[5] = D.lightPos;
    return 0;
}

int rtHipTestSceneCameraLog(const rtHipScene *sc, uint64_t out[3])
{
    if (!sc || !out) return fail("rtHipTestSceneCameraLog: null argument");
    for (int i = 0; i < 3; ++i) out[i] = sc->cam.log[i];
    return 0;
}

int rtHipTestSceneCameraTimes(const rtHipScene *sc, double out[2])
{
    if (!sc || !out) return fail("rtHipTestSceneCameraTimes: null argument");
    out[0] = sc->cam.ms[0]; out[1] = sc->cam.ms[1];
    return 0;
}

int rtHipRenderTiles(rtHipScene *sc, void *stream)
{
    if (!sc) return fail("null scene");
    HIP_OK(hipSetDevice(sc->device));
    hipStream_t st = stream ? (hipStream_t)stream : sc->stream;
    // The frame's sample window.  A frame that continues from the tile buffer adds into the planes and cannot be rendered again: the
    // frames before it are verified first (and redone while their own window is still the last one), and it is issued watched.
    const rtHipSampleWindow w = sc->window;
    const bool continues = window_continues(w);
    if (continues && sc->unverified && frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, nullptr) != 0) return -1;
    apply_window(sc, w);
    sc->lastStream = st;
    auto issue = [&]() -> int {
        if (sc->eventsUsed == sc->events.size()) {
            Event a, b;
            HIP_OK(a.make()); HIP_OK(b.make());
            sc->events.emplace_back(std::move(a), std::move(b));
        }
        auto &ev = sc->events[sc->eventsUsed++];
        HIP_OK(hipEventRecord(ev.first, st));
        if (sc->pipeline == RT_HIP_PIPELINE_WAVEFRONT) {
            if (render_wavefront(sc, st, continues) != 0) return -1;
        } else {
            HIP_OK(rtk_launch_trace(&sc->dev, 0, st));
        }
        HIP_OK(hipEventRecord(ev.second, st));
        return 0;
    };
    // a frame that could not be issued leaves the windows alone: `last` keeps naming the last frame that was issued, `next` has not moved
    if (issue() != 0) return -1;
    sc->lastWindow = w;
    if (w.advance) sc->window.first = (uint32_t)(((uint64_t)w.first + sc->dev.sampleCount) % w.total);
    return 0;
}

int rtHipSampleWindowCheck(cl_uint sampleCount, const rtHipSampleWindow *w)
{
    if (!w) return fail("sample window: null argument");
    const uint64_t S = sampleCount, N = w->total, f = w->first;
    if (S == 0) return fail("sample window: sampleCount must be >= 1");
    if (N == 0) return fail("sample window: total must be >= 1");
    if (w->divisor == 0) return fail("sample window: divisor must be >= 1");
    if (f + S > N) return fail("sample window: first + sampleCount = %llu + %llu reaches past total = %llu", (unsigned long long)f, (unsigned long long)S, (unsigned long long)N);
    if (w->accumulate > 1u) return fail("sample window: accumulate must be 0 or 1, not %u", w->accumulate);
    if (w->advance > 1u) return fail("sample window: advance must be 0 or 1, not %u", w->advance);
    if (w->advance && N % S != 0) return fail("sample window: advance needs total = %llu to be a multiple of sampleCount = %llu", (unsigned long long)N, (unsigned long long)S);
    if (w->advance && f % S != 0) return fail("sample window: advance needs first = %llu to be a multiple of sampleCount = %llu", (unsigned long long)f, (unsigned long long)S);
    return 0;
}

int rtHipSceneSetSampleWindow(rtHipScene *sc, const rtHipSampleWindow *w)
{
    if (!sc) return fail("rtHipSceneSetSampleWindow: null scene");
    const rtHipSampleWindow def = default_window(sc->dev.sampleCount);
    if (!w) w = &def;
    if (rtHipSampleWindowCheck(sc->dev.sampleCount, w) != 0) return -1;
    // (the launch plan stays: other sample ids of the same pixels need statistically the same rounds, see render_wavefront's batches)
    sc->window = *w;
    apply_window(sc, sc->window);
    return 0;
}

int rtHipSceneGetSampleWindow(const rtHipScene *sc, rtHipSampleWindow *next, rtHipSampleWindow *last)
{
    if (!sc) return fail("rtHipSceneGetSampleWindow: null scene");
    if (next) *next = sc->window;
    if (last) *last = sc->lastWindow;
    return 0;
}

int rtHipSetPipeline(rtHipScene *sc, int pipeline)
{
    if (!sc) return fail("null scene");
    if (pipeline != RT_HIP_PIPELINE_MEGAKERNEL && pipeline != RT_HIP_PIPELINE_WAVEFRONT) return fail("unknown pipeline %d", pipeline);
    if (pipeline == RT_HIP_PIPELINE_MEGAKERNEL && sc->passMask)
        return fail("render passes are on: the megakernel pipeline does not produce them (rtHipScenePasses(scene, 0) first)");
    sc->pipeline = pipeline;
    return 0;
}

// Which render pass bits need the pass buffer (RT_SURF_BUF_BITS: rt_host.h)
#define RT_PASS_BUF_BITS (RT_HIP_PASS_ALPHA | RT_HIP_PASS_DEPTH | RT_HIP_PASS_TRIANGLE)

// One of the two pass buffers: made (zeroed) when `want` and absent, freed when not `want` -- after a sync, frames in flight may still
// write it.  Counted in rtHipSceneBytes.
static int keep_pass_buffer(rtHipScene *sc, bool want, DevBlock &buf, uint32_t words)
{
    if (!want && buf.p) {
        HIP_OK(hipDeviceSynchronize());
        buf.drop(sc->bytes);
    } else if (want && !buf.p) {
        const uint64_t n = std::max<uint64_t>((uint64_t)sc->tileIds.size() * words * RT_TILE_PIXELS * 4, 4);
        HIP_OK(buf.make(n, sc->bytes));
        HIP_OK(hipMemset(buf.p, 0, n));
    }
    return 0;
}

int rtHipScenePasses(rtHipScene *sc, cl_uint mask)
{
    if (!sc) return fail("null scene");
    if (mask & ~(cl_uint)(RT_PASS_BUF_BITS | RT_SURF_BUF_BITS)) return fail("unknown render pass bits 0x%x", mask);
    if (mask && sc->pipeline == RT_HIP_PIPELINE_MEGAKERNEL) return fail("render passes need the wavefront pipeline (the scene is on the megakernel)");
    HIP_OK(hipSetDevice(sc->device));
    if (keep_pass_buffer(sc, (mask & RT_PASS_BUF_BITS) != 0, sc->passBuf, RT_PASS_WORDS) != 0) return -1;
    if (keep_pass_buffer(sc, (mask & RT_SURF_BUF_BITS) != 0, sc->surfBuf, RT_SURF_WORDS) != 0) return -1;
    if ((mask & RT_SURF_BUF_BITS) != RT_SURF_BUF_BITS && sc->denoiseBuf) { // the denoiser needs both surface passes
        HIP_OK(hipDeviceSynchronize());
        sc->denoiseBuf.drop(sc->bytes);
    }
    sc->passMask = mask;
    return 0;
}

void *rtHipPassBuffer(rtHipScene *sc) { return sc ? sc->passBuf.p : nullptr; }
uint64_t rtHipPassBufferBytes(const rtHipScene *sc) { return sc && sc->passBuf ? (uint64_t)sc->tileIds.size() * RT_PASS_WORDS * RT_TILE_PIXELS * 4 : 0; }
void *rtHipSurfaceBuffer(rtHipScene *sc) { return sc ? sc->surfBuf.p : nullptr; }
uint64_t rtHipSurfaceBufferBytes(const rtHipScene *sc) { return sc && sc->surfBuf ? (uint64_t)sc->tileIds.size() * RT_SURF_WORDS * RT_TILE_PIXELS * 4 : 0; }

// Diagnostic: raw copy of the 8 device-side debug counters (work counters of the counted kernel, or the cycle sums of
// an RT_DIAG_STAMPS build).  clear != 0 zeroes them afterwards.
int rtHipDebugCounters(rtHipScene *sc, unsigned long long out[8], int clear)
{
    if (!sc || !out) return fail("null argument");
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, sc->dev.stats, 64, hipMemcpyDeviceToHost));
    if (clear) HIP_OK(hipMemset(sc->dev.stats, 0, 64));
    return 0;
}

int rtHipStageTiming(rtHipScene *sc, int enable)
{
    if (!sc) return fail("null scene");
    sc->stageTiming = enable != 0;
    sc->stageEventsUsed = 0;
    return 0;
}

int rtHipStageTimes(rtHipScene *sc, double ms[5], uint64_t *rounds)
{
    if (!sc || !ms) return fail("null argument");
    HIP_OK(hipSetDevice(sc->device));
    for (int i = 0; i < 5; ++i) ms[i] = 0.0;
    for (size_t i = 0; i < sc->stageEventsUsed; ++i) {
        HIP_OK(hipEventSynchronize(sc->stageEvents[i].b));
        float t = 0.f;
        HIP_OK(hipEventElapsedTime(&t, sc->stageEvents[i].a, sc->stageEvents[i].b));
        ms[sc->stageEvents[i].stage] += t;
    }
    sc->stageEventsUsed = 0;
    if (rounds) *rounds = sc->roundsLast;
    return 0;
}

int rtHipRenderTilesCounted(rtHipScene *sc, rtHipStats *stats)
{
    if (!sc || !stats) return fail("null argument");
    if (!same_window(sc->window, default_window(sc->dev.sampleCount)))
        return fail("rtHipRenderTilesCounted: a sample window is in effect (the work counters describe the default frame; rtHipSceneSetSampleWindow(scene, NULL) first)");
    HIP_OK(hipSetDevice(sc->device));
    apply_window(sc, sc->window);
    HIP_OK(hipMemsetAsync(sc->dev.stats, 0, 64, sc->stream));
    HIP_OK(rtk_launch_trace(&sc->dev, 1, sc->stream));
    unsigned long long host[8] = { 0 };
    HIP_OK(hipMemcpyAsync(host, sc->dev.stats, 64, hipMemcpyDeviceToHost, sc->stream));
    HIP_OK(hipStreamSynchronize(sc->stream));
    stats->primarySamples = host[0]; stats->primaryCandidates = host[1]; stats->gridRays = host[2]; stats->gridCells = host[3];
    stats->gridCandidates = host[4]; stats->shadedHits = host[5]; stats->texelFetches = host[6];
    return 0;
}

void *rtHipTileBuffer(rtHipScene *sc) { return sc ? (void *)sc->dev.tileBuf : nullptr; }
uint64_t rtHipTileBufferBytes(const rtHipScene *sc) { return sc ? (uint64_t)sc->tileIds.size() * 3 * RT_TILE_PIXELS * 2 : 0; }

int rtHipDetile(int device, const void *tileBuffer, const cl_uint *tileIdsDevice, cl_uint tileCount, cl_uint width, cl_uint height,
                void *planeR, void *planeG, void *planeB, void *stream)
{
    if (!tileBuffer || !tileIdsDevice || !planeR || !planeG || !planeB) return fail("null argument");
    if (width == 0 || height == 0) return fail("empty image");
    HIP_OK(hipSetDevice(device));
    const uint32_t tilesX = (width + RT_TILE - 1) / RT_TILE;
    HIP_OK(rtk_launch_detile(tileBuffer, tileIdsDevice, tileCount, width, height, tilesX, planeR, planeG, planeB, 1, (hipStream_t)stream));
    return 0;
}

int rtHipDetileStore(int device, const void *tileBuffer, const cl_uint *tileIdsDevice, cl_uint tileCount, cl_uint width, cl_uint height,
                     void *planeR, void *planeG, void *planeB, void *stream)
{
    if (!tileBuffer || !tileIdsDevice || !planeR || !planeG || !planeB) return fail("null argument");
    if (width == 0 || height == 0) return fail("empty image");
    HIP_OK(hipSetDevice(device));
    const uint32_t tilesX = (width + RT_TILE - 1) / RT_TILE;
    HIP_OK(rtk_launch_detile(tileBuffer, tileIdsDevice, tileCount, width, height, tilesX, planeR, planeG, planeB, 0, (hipStream_t)stream));
    return 0;
}

// Plain device memory for hosts that do not include HIP headers (a gather root's planes, test buffers).
void *rtHipDeviceAlloc(int device, uint64_t bytes)
{
    void *p = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { fail("rtHipDeviceAlloc(%d, %llu) failed", device, (unsigned long long)bytes); return nullptr; }
    return p;
}
void rtHipDeviceFree(int device, void *p)
{
    if (p && hipSetDevice(device) == hipSuccess) (void)hipFree(p);
}
int rtHipDeviceCopy(int device, void *dst, const void *src, uint64_t bytes, int toDevice)
{
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(dst, src, bytes, toDevice ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return 0;
}

int rtHipSync(rtHipScene *sc, void *stream)
{
    if (!sc) return fail("null scene");
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipStreamSynchronize(stream ? (hipStream_t)stream : sc->stream));
    return frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, nullptr);
}

int rtHipFrameFinish(rtHipScene *sc, int *redone)
{
    if (!sc) return fail("null scene");
    HIP_OK(hipSetDevice(sc->device));
    return frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, redone);
}

int rtHipReadback(rtHipScene *sc, cl_ushort *outR, cl_ushort *outG, cl_ushort *outB)
{
    if (!sc || !outR || !outG || !outB) return fail("null argument");
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipDeviceSynchronize());
    if (frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, nullptr) != 0) return -1;
    const size_t nt = sc->tileIds.size();
    std::vector<uint16_t> host(nt * 3 * RT_TILE_PIXELS);
    HIP_OK(hipMemcpy(host.data(), sc->dev.tileBuf, host.size() * 2, hipMemcpyDeviceToHost));
    cl_ushort *planes[3] = { outR, outG, outB };
    rt_tile_walk_rows(sc->tileIds.data(), nt, sc->tilesX, sc->width, sc->height, [&](size_t s, uint32_t ly, size_t at, uint32_t n) {
        for (int c = 0; c < 3; ++c) {
            const uint16_t *src = host.data() + (s * 3 + c) * RT_TILE_PIXELS + ly * RT_TILE;
            cl_ushort *dst = planes[c] + at;
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t v = (uint32_t)dst[i] + src[i]; // saturating accumulate (raytrace_opencl.c:729-740)
                dst[i] = (cl_ushort)(v > 0xFFFFu ? 0xFFFFu : v);
            }
        }
    });
    return 0;
}

int rtHipReadbackPasses(rtHipScene *sc, cl_ushort *alpha, cl_float *depth, cl_uint *triangle)
{
    if (!sc) return fail("null scene");
    const struct { const void *out; cl_uint bit; const char *name; } want[3] = {
        { alpha, RT_HIP_PASS_ALPHA, "alpha" }, { depth, RT_HIP_PASS_DEPTH, "depth" }, { triangle, RT_HIP_PASS_TRIANGLE, "triangle" } };
    for (const auto &w : want)
        if (w.out && !(sc->passMask & w.bit)) return fail("the %s pass is not on for this scene (rtHipScenePasses)", w.name);
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipDeviceSynchronize());
    if (frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, nullptr) != 0) return -1;
    if (!alpha && !depth && !triangle) return 0;
    const size_t nt = sc->tileIds.size();
    std::vector<uint32_t> host(nt * RT_PASS_WORDS * RT_TILE_PIXELS);
    HIP_OK(hipMemcpy(host.data(), sc->passBuf, host.size() * 4, hipMemcpyDeviceToHost));
    const uint64_t S = sc->dev.sampleCount;
    rt_tile_walk_rows(sc->tileIds.data(), nt, sc->tilesX, sc->width, sc->height, [&](size_t s, uint32_t ly, size_t at, uint32_t n) {
        const uint32_t *src = host.data() + s * RT_PASS_WORDS * RT_TILE_PIXELS + ly * RT_TILE;
        for (uint32_t i = 0; i < n; ++i) {
            if (alpha) alpha[at + i] = (cl_ushort)((uint64_t)src[RT_PASS_HITS * RT_TILE_PIXELS + i] * 65535u / S);
            if (depth) memcpy(&depth[at + i], &src[RT_PASS_DEPTH * RT_TILE_PIXELS + i], 4);
            if (triangle) triangle[at + i] = src[RT_PASS_TRIANGLE * RT_TILE_PIXELS + i];
        }
    });
    return 0;
}

int rtHipReadbackSurfacePasses(rtHipScene *sc, cl_float *normal, cl_float *albedo)
{
    if (!sc) return fail("null scene");
    if (normal && !(sc->passMask & RT_HIP_PASS_NORMAL)) return fail("the normal pass is not on for this scene (rtHipScenePasses)");
    if (albedo && !(sc->passMask & RT_HIP_PASS_ALBEDO)) return fail("the albedo pass is not on for this scene (rtHipScenePasses)");
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipDeviceSynchronize());
    if (frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, nullptr) != 0) return -1;
    if (!normal && !albedo) return 0;
    const size_t nt = sc->tileIds.size();
    std::vector<float> host(nt * RT_SURF_WORDS * RT_TILE_PIXELS);
    HIP_OK(hipMemcpy(host.data(), sc->surfBuf, host.size() * 4, hipMemcpyDeviceToHost));
    const float S = (float)sc->dev.sampleCount; // the buffer holds sums in sample order; the means are taken here, in fp32
    rt_tile_walk_rows(sc->tileIds.data(), nt, sc->tilesX, sc->width, sc->height, [&](size_t s, uint32_t ly, size_t at, uint32_t n) {
        const float *src = host.data() + s * RT_SURF_WORDS * RT_TILE_PIXELS + ly * RT_TILE;
        for (uint32_t i = 0; i < n; ++i)
            for (int c = 0; c < 3; ++c) {
                if (normal) normal[3 * (at + i) + c] = src[(RT_SURF_NORMAL + c) * RT_TILE_PIXELS + i] / S;
                if (albedo) albedo[3 * (at + i) + c] = src[(RT_SURF_ALBEDO + c) * RT_TILE_PIXELS + i] / S;
            }
    });
    return 0;
}

int rtHipSceneIntersectDevice(rtHipScene *sc, const void *rays, const void *excluded, cl_uint count, void *hits, void *stream)
{
    if (!sc) return fail("null scene");
    if (count == 0) return 0;
    if (!rays || !hits) return fail("null rays or hits with %u rays", count);
    HIP_OK(hipSetDevice(sc->device));
    if (query_pointer_ok(sc->device, "the scene", rays, (uint64_t)count * sizeof(rtHipRay), 16, "rays") != 0) return -1;
    if (excluded && query_pointer_ok(sc->device, "the scene", excluded, (uint64_t)count * 4, 4, "excluded") != 0) return -1;
    if (query_pointer_ok(sc->device, "the scene", hits, (uint64_t)count * sizeof(rtHipHit), 16, "hits") != 0) return -1;
    HIP_OK(rtw_launch_query(&sc->dev, rays, (const uint32_t *)excluded, count, hits, sc->tune.fastQuotient ? 1u : 0u,
                            stream ? (hipStream_t)stream : sc->stream));
    return 0;
}

int rtHipSceneIntersect(rtHipScene *sc, const rtHipRay *rays, const cl_uint *excluded, cl_uint count, rtHipHit *hits)
{
    if (!sc) return fail("null scene");
    if (count == 0) return 0;
    if (!rays || !hits) return fail("null rays or hits with %u rays", count);
    HIP_OK(hipSetDevice(sc->device));
    if (!sc->queryDev) {
        const uint32_t chunk = std::max<uint32_t>(sc->tune.queryRays, 1u);
        const uint64_t bytes = (uint64_t)chunk * (sizeof(rtHipRay) + 4 + sizeof(rtHipHit));
        char *host = Stager::pool().take(bytes);
        if (!host) return fail("rtHipSceneIntersect: no pinned staging buffer of %llu bytes", (unsigned long long)bytes);
        if (scene_block(sc, sc->queryDev, bytes, "rtHipSceneIntersect") != 0) { Stager::pool().give(host, bytes); return -1; }
        sc->queryRays = chunk; sc->queryHost = host;
    }
    const uint64_t chunk = sc->queryRays;
    // hits | rays | excluded ids: the two 16-byte records stay 16-byte aligned whatever the chunk
    char *hostHits = sc->queryHost, *hostRays = hostHits + chunk * sizeof(rtHipHit), *hostExcl = hostRays + chunk * sizeof(rtHipRay);
    char *devHits = sc->queryDev, *devRays = devHits + chunk * sizeof(rtHipHit), *devExcl = devRays + chunk * sizeof(rtHipRay);
    for (uint64_t off = 0; off < count; off += chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, count - off);
        memcpy(hostRays, rays + off, (size_t)n * sizeof(rtHipRay));
        HIP_OK(hipMemcpyAsync(devRays, hostRays, (size_t)n * sizeof(rtHipRay), hipMemcpyHostToDevice, sc->stream));
        if (excluded) {
            memcpy(hostExcl, excluded + off, (size_t)n * 4);
            HIP_OK(hipMemcpyAsync(devExcl, hostExcl, (size_t)n * 4, hipMemcpyHostToDevice, sc->stream));
        }
        HIP_OK(rtw_launch_query(&sc->dev, devRays, excluded ? (const uint32_t *)devExcl : nullptr, n, devHits, sc->tune.fastQuotient ? 1u : 0u, sc->stream));
        HIP_OK(hipMemcpyAsync(hostHits, devHits, (size_t)n * sizeof(rtHipHit), hipMemcpyDeviceToHost, sc->stream));
        HIP_OK(hipStreamSynchronize(sc->stream));
        memcpy(hits + off, hostHits, (size_t)n * sizeof(rtHipHit));
    }
    return 0;
}

// ---- ambient occlusion (include/raytrace_hip.h, "AMBIENT OCCLUSION"; kernels in rt_scene_passes.hip, rt_ao_*) ------------------------
void rtHipAoDefaults(rtHipAoParams *p)
{
    if (!p) return;
    p->raysPerHit = 16;
    p->pixelSamples = 1;
    p->radius = HUGE_VALF;
    p->seed = 0;
}

static int ao_check(const rtHipScene *sc, const rtHipAoParams *p, const void *out)
{
    if (!sc || !p || !out) return fail("ambient occlusion: null scene, parameters or output");
    if (p->raysPerHit < 1 || p->raysPerHit > 256) return fail("ambient occlusion: raysPerHit %u is not in 1..256", p->raysPerHit);
    if (p->pixelSamples < 1 || p->pixelSamples > 64) return fail("ambient occlusion: pixelSamples %u is not in 1..64", p->pixelSamples);
    if (!(p->radius > 0.f)) return fail("ambient occlusion: radius %g is not > 0", (double)p->radius);
    if ((uint64_t)sc->width * sc->height >= (1ull << 32)) return fail("ambient occlusion: %u x %u is 2^32 pixels or more", sc->width, sc->height);
    return 0;
}

// Enqueues the whole pass on `st`: counters zeroed, the chunks' primary and AO launches, the finish kernel into `out` (row-major W x H), or --
// rowMajor false -- over the counters themselves, in AO order.
static int ao_run(rtHipScene *sc, const rtHipAoParams *p, float *out, bool rowMajor, hipStream_t st)
{
    const uint64_t pixels = (uint64_t)sc->tileIds.size() * RT_TILE_PIXELS, counterBytes = (pixels * 4 + 255) & ~255ull;
    if (!sc->aoBuf) {
        const uint32_t chunk = std::max<uint32_t>(sc->tune.aoSamples, 1u);
        const uint64_t bytes = counterBytes + 256 + (uint64_t)chunk * 32; // counters | hit list length | hit list
        // (the event first: one that is left without its scratch is harmless and is found again by the next call)
        if (scene_event(sc->aoDone, hipEventDisableTiming, "ambient occlusion") != 0 || scene_block(sc, sc->aoBuf, bytes, "ambient occlusion") != 0) return -1;
        sc->aoChunk = chunk;
    } else HIP_OK(hipStreamWaitEvent(st, sc->aoDone, 0)); // the last call's use of the scratch, on whatever stream it ran
    uint32_t *counter = sc->aoBuf.as<uint32_t>();
    HIP_OK(hipMemsetAsync(counter, 0, pixels * 4, st));
    RtAoArgs A;
    A.raysPerHit = p->raysPerHit; A.pixelSamples = p->pixelSamples; A.seed = p->seed; A.fastQuotient = sc->tune.fastQuotient ? 1u : 0u;
    A.radius = p->radius; A.hits = (uint32_t *)(sc->aoBuf + counterBytes); A.rec = (float4 *)(sc->aoBuf + counterBytes + 256); A.counter = counter;
    const uint64_t total = pixels * p->pixelSamples;
    for (uint64_t base = 0; base < total; base += sc->aoChunk) {
        A.base = base;
        A.count = (uint32_t)std::min<uint64_t>(sc->aoChunk, total - base);
        HIP_OK(hipMemsetAsync(A.hits, 0, 4, st));
        HIP_OK(rtw_launch_ao(&sc->dev, &A, st));
    }
    HIP_OK(rtw_launch_ao_finish(&sc->dev, counter, p->pixelSamples * p->raysPerHit, rowMajor ? out : (float *)counter, rowMajor ? 1u : 0u, st));
    HIP_OK(hipEventRecord(sc->aoDone, st));
    return 0;
}

int rtHipSceneAmbientOcclusionDevice(rtHipScene *sc, const rtHipAoParams *p, void *out, void *stream)
{
    if (ao_check(sc, p, out) != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    if (query_pointer_ok(sc->device, "the scene", out, (uint64_t)sc->width * sc->height * 4, 4, "out") != 0) return -1;
    return ao_run(sc, p, (float *)out, true, stream ? (hipStream_t)stream : sc->stream);
}

int rtHipSceneAmbientOcclusion(rtHipScene *sc, const rtHipAoParams *p, cl_float *out)
{
    if (ao_check(sc, p, out) != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    // the finished values overwrite the counters in AO order; the host stores the scene's pixels
    if (ao_run(sc, p, nullptr, false, sc->stream) != 0) return -1;
    const size_t n = sc->tileIds.size() * (size_t)RT_TILE_PIXELS;
    std::vector<float> host(n);
    HIP_OK(hipMemcpyAsync(host.data(), sc->aoBuf, n * 4, hipMemcpyDeviceToHost, sc->stream));
    HIP_OK(hipStreamSynchronize(sc->stream));
    rt_tile_walk_block_pixels(sc->tileIds.data(), sc->tileIds.size(), sc->tilesX, sc->width, sc->height, [&](size_t lp, size_t at) { out[at] = host[lp]; });
    return 0;
}

// ---- motion vectors (include/raytrace_hip.h, "MOTION VECTORS"; kernels in rt_scene_passes.hip, rt_motion_*) ---------------------------
int rtHipSceneMotionMark(rtHipScene *sc)
{
    if (!sc) return fail("rtHipSceneMotionMark: null scene");
    rtHipScene::Motion &M = sc->motion;
    HIP_OK(hipSetDevice(sc->device));
    const uint32_t T = sc->dev.triangleCount;
    if (!M.ref) {
        const uint64_t bytes = std::max<uint64_t>((uint64_t)T * RT_MOTION_REF_ROWS * 16, 16);
        static const char who[] = "rtHipSceneMotionMark"; // (the events first, as in ao_run)
        if (scene_event(M.marked, hipEventDisableTiming, who) != 0 || scene_event(M.done, hipEventDisableTiming, who) != 0 || scene_block(sc, M.ref, bytes, who) != 0)
            return -1;
        M.triangles = T;
    } else {
        if (T != M.triangles) return fail("rtHipSceneMotionMark: the scene has %u triangles, the reference was made for %u", T, M.triangles);
        HIP_OK(hipStreamWaitEvent(sc->stream, M.done, 0)); // calls on other streams that still read the old reference
    }
    HIP_OK(rtw_launch_motion_mark(sc->dev.triRec, M.ref, T, sc->stream));
    HIP_OK(hipEventRecord(M.marked, sc->stream));
    rtHipSceneGetCamera(sc, &M.cam);
    M.have = true;
    return 0;
}

int rtHipSceneMotionReferenceCamera(const rtHipScene *sc, rtHipCamera *out)
{
    if (!sc || !out) return fail("rtHipSceneMotionReferenceCamera: null argument");
    if (!sc->motion.have) return fail("rtHipSceneMotionReferenceCamera: no motion reference (rtHipSceneMotionMark)");
    *out = sc->motion.cam;
    return 0;
}

static int motion_check(const rtHipScene *sc, const void *motion, const void *t, const void *prevT, const void *triangle)
{
    if (!sc) return fail("motion vectors: null scene");
    if (!motion && !t && !prevT && !triangle) return fail("motion vectors: every output is null");
    if (!sc->motion.have) return fail("motion vectors: no motion reference (rtHipSceneMotionMark)");
    if (sc->dev.triangleCount != sc->motion.triangles)
        return fail("motion vectors: the scene has %u triangles, the reference was made for %u", sc->dev.triangleCount, sc->motion.triangles);
    if ((uint64_t)sc->width * sc->height >= (1ull << 32)) return fail("motion vectors: %u x %u is 2^32 pixels or more", sc->width, sc->height);
    return 0;
}

int rtHipSceneMotionDevice(rtHipScene *sc, void *motion, void *t, void *prevT, void *triangle, void *stream)
{
    if (motion_check(sc, motion, t, prevT, triangle) != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    const uint64_t pixels = (uint64_t)sc->width * sc->height;
    if (motion && query_pointer_ok(sc->device, "the scene", motion, pixels * 8, 4, "motion") != 0) return -1;
    if (t && query_pointer_ok(sc->device, "the scene", t, pixels * 4, 4, "t") != 0) return -1;
    if (prevT && query_pointer_ok(sc->device, "the scene", prevT, pixels * 4, 4, "prevT") != 0) return -1;
    if (triangle && query_pointer_ok(sc->device, "the scene", triangle, pixels * 4, 4, "triangle") != 0) return -1;
    return motion_run(sc, motion, t, prevT, triangle, true, stream ? (hipStream_t)stream : sc->stream);
}

int rtHipSceneMotion(rtHipScene *sc, cl_float *motion, cl_float *t, cl_float *prevT, cl_uint *triangle)
{
    if (motion_check(sc, motion, t, prevT, triangle) != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    rtHipScene::Motion &M = sc->motion;
    const size_t n = sc->tileIds.size() * (size_t)RT_TILE_PIXELS;
    if (!M.stage) {
        const uint64_t bytes = std::max<uint64_t>((uint64_t)n * 20, 16);
        if (scene_block(sc, M.stage, bytes, "motion vectors") != 0) return -1;
    }
    // tile-major planes in AO order: motion | t | prevT | triangle; the host stores the scene's pixels
    char *dMotion = M.stage, *dT = M.stage + n * 8, *dPrev = M.stage + n * 12, *dTri = M.stage + n * 16;
    if (motion_run(sc, motion ? dMotion : nullptr, t ? dT : nullptr, prevT ? dPrev : nullptr, triangle ? dTri : nullptr, false, sc->stream) != 0) return -1;
    std::vector<uint32_t> host(n * 5);
    uint32_t *hMotion = host.data(), *hT = hMotion + n * 2, *hPrev = hT + n, *hTri = hPrev + n;
    if (motion) HIP_OK(hipMemcpyAsync(hMotion, dMotion, n * 8, hipMemcpyDeviceToHost, sc->stream));
    if (t) HIP_OK(hipMemcpyAsync(hT, dT, n * 4, hipMemcpyDeviceToHost, sc->stream));
    if (prevT) HIP_OK(hipMemcpyAsync(hPrev, dPrev, n * 4, hipMemcpyDeviceToHost, sc->stream));
    if (triangle) HIP_OK(hipMemcpyAsync(hTri, dTri, n * 4, hipMemcpyDeviceToHost, sc->stream));
    HIP_OK(hipStreamSynchronize(sc->stream));
    rt_tile_walk_block_pixels(sc->tileIds.data(), sc->tileIds.size(), sc->tilesX, sc->width, sc->height, [&](size_t lp, size_t at) {
        if (motion) memcpy(motion + 2 * at, hMotion + 2 * lp, 8);
        if (t) memcpy(t + at, hT + lp, 4);
        if (prevT) memcpy(prevT + at, hPrev + lp, 4);
        if (triangle) triangle[at] = hTri[lp];
    });
    return 0;
}

// ---- ambient occlusion bake (include/raytrace_hip.h, "AMBIENT OCCLUSION BAKE"; kernels in rt_scene_passes.hip, rt_bake_*) -------------
void rtHipBakeDefaults(rtHipBakeParams *p)
{
    if (!p) return;
    p->width = 0; p->height = 0;
    p->raysPerTexel = 16;
    p->radius = HUGE_VALF;
    p->seed = 0;
    p->dilate = 2;
    p->firstTriangle = 0; p->triangleCount = 0xffffffffu;
    p->material = 0; p->matchMaterial = 0;
}

static int bake_check(const rtHipScene *sc, const rtHipBakeParams *p, const void *ao)
{
    if (!sc || !p || !ao) return fail("ambient occlusion bake: null scene, parameters or ao");
    if (p->width < 1 || p->height < 1 || (uint64_t)p->width * p->height > (1ull << 26))
        return fail("ambient occlusion bake: a %u x %u map is not 1 .. 2^26 texels", p->width, p->height);
    if (p->raysPerTexel < 1 || p->raysPerTexel > 256) return fail("ambient occlusion bake: raysPerTexel %u is not in 1..256", p->raysPerTexel);
    if (!(p->radius > 0.f)) return fail("ambient occlusion bake: radius %g is not > 0", (double)p->radius);
    if (p->dilate > 64) return fail("ambient occlusion bake: dilate %u is not in 0..64", p->dilate);
    const uint64_t T = sc->dev.triangleCount;
    if (p->triangleCount == 0xffffffffu ? p->firstTriangle > T : (uint64_t)p->firstTriangle + p->triangleCount > T)
        return fail("ambient occlusion bake: triangles %u + %u reach past the scene's %llu", p->firstTriangle, p->triangleCount, (unsigned long long)T);
    return 0;
}

// Enqueues the whole bake on `st`: rasterise, the chunks' points and AO launches, finish and dilation.  The values go to `ao` and the
// winners to `tri` (may be null), both row-major W x H device arrays; null `ao` = into the scratch, whose value plane bake_run returns
// in `result` (the host entry point reads it and the winners from there).
static int bake_run(rtHipScene *sc, const rtHipBakeParams *p, float *ao, uint32_t *tri, hipStream_t st, const char **result = nullptr)
{
    const uint64_t texels = (uint64_t)p->width * p->height;
    const uint32_t T = sc->dev.triangleCount, chunkWant = std::min<uint32_t>(std::max<uint32_t>(sc->tune.bakeTexels, 1u), 1u << 24);
    const uint64_t bigBytes = ((uint64_t)T * 4 + 255) & ~255ull;
    if (!sc->bakeBuf || texels > sc->bakeTexels || chunkWant != sc->bakeChunk) {
        const uint64_t cap = std::max<uint64_t>(texels, sc->bakeTexels), capPlane = (cap * 4 + 255) & ~255ull;
        if (sc->bakeBuf) { // a larger map: the last call's use of the old scratch ends first, and the scratch goes before the larger one is made
            HIP_OK(hipEventSynchronize(sc->bakeDone));
            sc->bakeBuf.drop(sc->bytes);
            sc->bakeTexels = 0;
        }
        const uint64_t bytes = 3 * capPlane + bigBytes + 256 + (uint64_t)chunkWant * 32; // win | counter | values | big list | lengths | hit list
        static const char who[] = "ambient occlusion bake"; // (the event first, as in ao_run)
        if (scene_event(sc->bakeDone, hipEventDisableTiming, who) != 0 || scene_block(sc, sc->bakeBuf, bytes, who) != 0) return -1;
        sc->bakeTexels = cap; sc->bakeChunk = chunkWant;
    } else HIP_OK(hipStreamWaitEvent(st, sc->bakeDone, 0)); // the last call's use of the scratch, on whatever stream it ran
    const uint64_t capPlane = (sc->bakeTexels * 4 + 255) & ~255ull;
    uint32_t *win = sc->bakeBuf.as<uint32_t>(), *counter = (uint32_t *)(sc->bakeBuf + capPlane);
    float *values = (float *)(sc->bakeBuf + 2 * capPlane);
    char *tail = sc->bakeBuf + 3 * capPlane;
    RtBakeArgs A;
    A.width = p->width; A.height = p->height; A.raysPerTexel = p->raysPerTexel; A.seed = p->seed; A.fastQuotient = sc->tune.fastQuotient ? 1u : 0u;
    A.radius = p->radius; A.material = p->material; A.matchMaterial = p->matchMaterial ? 1u : 0u;
    A.win = win; A.counter = counter; A.bigList = (uint32_t *)tail; A.bigCount = (uint32_t *)(tail + bigBytes); A.hits = A.bigCount + 1;
    A.rec = (float4 *)(tail + bigBytes + 256);
    HIP_OK(hipMemsetAsync(win, 0xff, texels * 4, st));
    HIP_OK(hipMemsetAsync(A.bigCount, 0, 4, st));
    A.first = p->firstTriangle; A.count = p->triangleCount == 0xffffffffu ? T - p->firstTriangle : p->triangleCount; A.base = 0;
    HIP_OK(rtw_launch_bake_raster(&sc->dev, &A, st));
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(sc->bakeChunk, (1ull << 31) / p->raysPerTexel); // (chunk x R <= 2^31)
    for (uint64_t base = 0; base < texels; base += chunk) {
        A.base = base;
        A.count = (uint32_t)std::min<uint64_t>(chunk, texels - base);
        HIP_OK(hipMemsetAsync(A.hits, 0, 4, st));
        HIP_OK(rtw_launch_bake_points(&sc->dev, &A, st));
        HIP_OK(rtw_launch_bake_ao(&sc->dev, &A, st));
    }
    // values: counter's plane (in place) and `values` in turn, the last pass into `ao` -- or, for the host, the plane it would read next
    float *planes[2] = { (float *)counter, values };
    const uint32_t G = p->dilate;
    float *dst = ao ? ao : planes[G & 1u];
    HIP_OK(rtw_launch_bake_finish((uint32_t)texels, win, counter, p->raysPerTexel, G ? -1.f : 0.f, G ? planes[0] : dst, tri, st));
    for (uint32_t g = 1; g <= G; ++g)
        HIP_OK(rtw_launch_bake_dilate(p->width, p->height, planes[(g - 1) & 1u], g == G ? dst : planes[g & 1u], g == G ? 1u : 0u, st));
    HIP_OK(hipEventRecord(sc->bakeDone, st));
    if (result) *result = (const char *)dst;
    return 0;
}

int rtHipSceneBakeAmbientOcclusionDevice(rtHipScene *sc, const rtHipBakeParams *p, void *ao, void *triangle, void *stream)
{
    if (bake_check(sc, p, ao) != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    const uint64_t bytes = (uint64_t)p->width * p->height * 4;
    if (query_pointer_ok(sc->device, "the scene", ao, bytes, 4, "ao") != 0) return -1;
    if (triangle && query_pointer_ok(sc->device, "the scene", triangle, bytes, 4, "triangle") != 0) return -1;
    return bake_run(sc, p, (float *)ao, (uint32_t *)triangle, stream ? (hipStream_t)stream : sc->stream);
}

int rtHipSceneBakeAmbientOcclusion(rtHipScene *sc, const rtHipBakeParams *p, cl_float *ao, cl_uint *triangle)
{
    if (bake_check(sc, p, ao) != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    const char *values = nullptr;
    if (bake_run(sc, p, nullptr, nullptr, sc->stream, &values) != 0) return -1;
    const size_t bytes = (size_t)p->width * p->height * 4;
    HIP_OK(hipMemcpyAsync(ao, values, bytes, hipMemcpyDeviceToHost, sc->stream));
    if (triangle) HIP_OK(hipMemcpyAsync(triangle, sc->bakeBuf, bytes, hipMemcpyDeviceToHost, sc->stream)); // (the winners' plane)
    HIP_OK(hipStreamSynchronize(sc->stream));
    return 0;
}

// ---- geometry updates ------------------------------------------------------------------------------------------------------------
// A scene-owned device buffer of at least `need` bytes: kept when it is large enough, otherwise replaced by one of need + need / 8 bytes
// (`exact`: of just `need`); contents are not carried over.  The caller has made sure no work reads it.
static bool geo_fit(rtHipScene *sc, DevBlock &buf, uint64_t need, bool exact, bool *allocated)
{
    const void *before = buf.p;
    if (buf.fit(need, std::max<uint64_t>(exact ? need : need + need / 8, 64), sc->bytes) != hipSuccess) return false;
    if (allocated && buf.p != before) *allocated = true;
    return true;
}

// the arrays of set `i` whose size only depends on the triangle count and, with `lists`, its list and pair records for `listBytes` / `pairBytes`
static bool geo_set_fit(rtHipScene *sc, int i, bool lists, uint64_t listBytes, uint64_t pairBytes, bool exact, bool *allocated)
{
    rtHipScene::GeoMove::Set &L = sc->geo.set[i];
    const uint64_t T = sc->dev.triangleCount;
    return geo_fit(sc, L.triRec, T * 64, true, allocated) && geo_fit(sc, L.triShade, T * RT_TRI_SHADE_WORDS * 4, true, allocated) &&
           geo_fit(sc, L.boxMin, GEO_PLANE_BYTES, true, allocated) && geo_fit(sc, L.cellLut, GEO_LUT_BYTES, true, allocated) &&
           geo_fit(sc, L.gridStart, GEO_START_BYTES, true, allocated) && geo_fit(sc, L.gridBits, GEO_BITS_BYTES, true, allocated) &&
           geo_fit(sc, L.sparse, GEO_SPARSE_BYTES, true, allocated) &&
           (!lists || (geo_fit(sc, L.gridList, listBytes, exact, allocated) && geo_fit(sc, L.pairRec, pairBytes, exact, allocated)));
}

int rtHipSceneSetGeometry(rtHipScene *sc, const rtHipGeometryUpdate *up)
{
    static const char who[] = "rtHipSceneSetGeometry";
    if (!sc || !up) return fail("%s: null argument", who);
    rtHipScene::GeoMove &G = sc->geo;
    const uint64_t V = up->vertexCount, T = sc->dev.triangleCount;
    if (V && !up->vertex) return fail("%s: null vertex array with %llu vertices", who, (unsigned long long)V);
    if (!up->triIndex && G.retained < 0) return fail("%s: no index array given and none retained (a scene drops the one it was created with)", who);
    const Tuning tune = tuning(); // this entry point's one look at the tuning values
    const uint64_t listLimit = std::min<uint64_t>(tune.buildListLimit, 0xffffffffull);
#define GEO_MEM(expr, what) do { if (!(expr)) { fail("%s: no device memory for %s", who, what); return -4; } } while (0)
    HIP_WHO(hipSetDevice(sc->device));
    if (up->arraysOnDevice) {
        if (V && query_pointer_ok(sc->device, "the scene", up->vertex, V * 16, 16, "vertex") != 0) return -1;
        if (up->triIndex && T && query_pointer_ok(sc->device, "the scene", up->triIndex, T * 16, 16, "triIndex") != 0) return -1;
        if (up->triNormal && T && query_pointer_ok(sc->device, "the scene", up->triNormal, T * 48, 16, "triNormal") != 0) return -1;
    }
    if (const int rc = change_begin(sc, who)) return rc;
    hipStream_t st = sc->stream;
    bool allocated = false;
    const uint64_t camCapBefore[2] = { sc->cam.list[0].size, sc->cam.list[1].size };
    const bool camMade = !sc->cam.scratch;
    for (Event &e : G.ev) HIP_WHO(e.make());
    if (!G.space.fillGroups) { G.space.fillGroups = 8; G.space.headroom = 1; }
    const int target = G.live == 0 ? 1 : 0, spareIndex = G.retained == 0 ? 1 : 0;
    rtHipScene::GeoMove::Set &N = G.set[target];
    GEO_MEM(geo_set_fit(sc, target, false, 0, 0, true, &allocated), "the spare set of records and grid arrays");
    GEO_MEM(geo_fit(sc, G.material, T * 4, true, &allocated), "the build scratch");
    if (allocated) HIP_WHO(hipMemsetAsync(G.material, 0xff, (size_t)G.material.size, st)); // every id -1: rtp_validate reads a material per triangle

    // 1. the caller's arrays on the device
    const void *dVertex = up->vertex, *dIndex = up->triIndex, *dNormal = up->triNormal;
    if (!up->arraysOnDevice) {
        GEO_MEM(geo_fit(sc, G.vertexBuf, V * 16, false, &allocated), "the vertices");
        HIP_WHO(sc->stager.copy(G.vertexBuf, up->vertex, V * 16));
        dVertex = G.vertexBuf;
        // (the normals' staging is made with the vertices', whether this update brings normals or not: a later one that does allocates nothing)
        GEO_MEM(geo_fit(sc, G.normalBuf, T * 48, true, &allocated), "the corner normals");
        if (up->triNormal) {
            HIP_WHO(sc->stager.copy(G.normalBuf, up->triNormal, T * 48));
            dNormal = G.normalBuf;
        }
    }
    // both index arrays are made by the first update: the retained one and the one a later update is checked in
    GEO_MEM(geo_fit(sc, G.index[0], T * 16, true, &allocated) && geo_fit(sc, G.index[1], T * 16, true, &allocated), "the index arrays");
    if (up->triIndex) { // host or device: the scene keeps a copy of its own
        HIP_WHO(sc->stager.copy(G.index[spareIndex], up->triIndex, T * 16));
        dIndex = G.index[spareIndex];
    } else dIndex = G.index[G.retained];
    HIP_WHO(sc->stager.drain());
    HIP_WHO(hipEventRecord(G.ev[0], st));

    // 2. ids are checked before anything gathers through them (the retained array too: V may have shrunk)
    HIP_WHO(rtp_validate((uint32_t)T, (uint32_t)V, 0x7fffffffu, dIndex, G.material, 0, nullptr, nullptr, 0, nullptr, sc->prepErr, st));
    HIP_WHO(hipStreamSynchronize(st));
    if (sc->check_prep() != 0) return -5;

    // 3. records
    HIP_WHO(rtg_launch_records((uint32_t)T, dVertex, dIndex, dNormal, sc->dev.triShade, N.triRec, N.triShade, st));
    HIP_WHO(hipEventRecord(G.ev[1], st));

    // 4. the grid, device arrays in, device arrays out
    uint64_t pairs = 0, glog[RT_BUILD_LOG_FIELDS] = {};
    G.space.allocated = 0;
    const uint64_t spaceBefore = G.space.bytes;
    const int grc = rt_grid_core_fill(&G.space, (uint32_t)V, (uint32_t)T, dVertex, dIndex, tune.buildKeyCap, listLimit, st, &pairs, glog);
    sc->bytes += G.space.bytes - spaceBefore;
    allocated = allocated || G.space.allocated;
    if (grc == -3) { fail("%s: the grid holds %llu pairs, more than the limit of %llu", who, (unsigned long long)glog[RT_BUILD_LOG_PAIRS], (unsigned long long)listLimit); return -3; }
    if (grc == -7) { fail("%s: a single triangle's fill outgrew its workgroup queue, or the second fill overflowed", who); return -7; }
    if (grc == -4) { fail("%s: no device memory for the grid build", who); return -4; }
    if (grc) { fail("%s: the grid build failed on the device", who); return -2; }
    if (pairs >= RT_PAIR_LIMIT) { fail("%s: the grid holds 2^28 pairs or more: pair indices would not fit the trace kernel's records", who); return -3; }
    GEO_MEM(geo_set_fit(sc, target, true, pairs * 4, pairs * 64, false, &allocated), "the grid list and pair records");
    GEO_MEM(geo_fit(sc, G.pairOrder, pairs * 4, false, &allocated) && geo_fit(sc, G.pairInfo, pairs * 4, false, &allocated), "the pair order");
    if (rt_grid_core_lists(&G.space, pairs, N.gridStart, N.gridList, st) != 0) { fail("%s: sorting the grid's pairs failed on the device", who); return -2; }
    float bm[4 * (RT_GRID_DIV + 1)];
    HIP_WHO(hipMemcpyAsync(bm, G.space.bm, sizeof bm, hipMemcpyDeviceToHost, st)); // 4 KB: the planes, for the tables the host derives
    HIP_WHO(hipStreamSynchronize(st));
    float planes[3 * (RT_GRID_DIV + 1)];
    uint8_t lut[3 * 256];
    uint32_t tame = 0;
    for (int w = 0; w < 3; ++w)
        for (int i = 0; i <= RT_GRID_DIV; ++i) planes[w * (RT_GRID_DIV + 1) + i] = bm[4 * i + w];
    grid_tables(planes, lut, &tame);
    float planeBuffer[RT_CLIP_FLOATS];
    clip_buffer_init(planes, planeBuffer);
    HIP_WHO(hipMemcpyAsync(N.boxMin, planeBuffer, sizeof planeBuffer, hipMemcpyHostToDevice, st));
    HIP_WHO(hipMemcpyAsync(N.cellLut, lut, sizeof lut, hipMemcpyHostToDevice, st));
    HIP_WHO(hipEventRecord(G.ev[2], st));

    // 5. the dense view and the pair records
    size_t denseBytes = 0;
    HIP_WHO(rtp_dense_grid(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &denseBytes, st));
    GEO_MEM(geo_fit(sc, G.denseTmp, denseBytes, true, &allocated), "the dense view's scratch");
    denseBytes = (size_t)G.denseTmp.size;
    HIP_WHO(hipMemsetAsync(N.sparse, 0, GEO_SPARSE_BYTES, st));
    HIP_WHO(rtp_dense_grid(N.gridStart, N.gridList, N.gridBits, N.sparse, G.pairOrder, G.pairInfo, G.denseTmp, &denseBytes, st));
    HIP_WHO(rtk_launch_gather_pairs((uint32_t)pairs, G.pairOrder, G.pairInfo, N.triRec, N.pairRec, st));
    HIP_WHO(clip_bound_issue(sc, N.gridBits, N.boxMin, st)); // (read back by the synchronisation behind the camera lists)
    HIP_WHO(hipEventRecord(G.ev[3], st));

    // 6. the camera lists of the camera in effect, over the new records
    rtHipCamera cam;
    (void)rtHipSceneGetCamera(sc, &cam);
    int camTarget = 0;
    RtCamMoveCtl ctl{};
    float camMs[2] = { 0.f, 0.f };
    if (const int rc = cam_move_build(sc, &cam, N.triRec, N.triShade, listLimit, who, &camTarget, &ctl, camMs)) return rc;
    HIP_WHO(hipEventRecord(G.ev[4], st));
    HIP_WHO(hipStreamSynchronize(st));
    float ms[4] = {};
    for (int i = 0; i < 4; ++i) HIP_WHO(hipEventElapsedTime(&ms[i], G.ev[i], G.ev[i + 1]));
    uint32_t clipCount = 0;
    float clipTail[4 + 4 * RT_CLIP_MAX_PLANES];
    HIP_WHO(clip_bound_commit(sc, planes, N.boxMin, st, &clipCount, clipTail));
    HIP_WHO(hipStreamSynchronize(st));
#undef GEO_MEM

    // 7. everything is complete: the new shape takes the old one's place
    RtDevScene &D = sc->dev;
    D.triRec = N.triRec; D.triShade = N.triShade;
    D.boxMin = N.boxMin; D.cellLut = N.cellLut; D.planesTame = tame;
    sc->clipCount = clipCount;
    memcpy(sc->clipTail, clipTail, sizeof sc->clipTail);
    D.gridStart = N.gridStart; D.gridList = N.gridList; D.gridBits = N.gridBits; D.gridBlockSparse = N.sparse; D.pairRec = N.pairRec;
    sc->gridListSize = pairs;
    G.live = target;
    if (up->triIndex) G.retained = spareIndex;
    sc->cam.args.triRec = N.triRec; sc->cam.args.triShade = N.triShade;
    cam_move_commit(sc, &cam, camTarget, ctl); // (refreshes the groups' views and drops the launch plan)
    sc->drop_part(PART_GEOMETRY); // what the scene was created with (the first update only)
    sc->drop_part(PART_GRID);
    // the other set is made as large as this one now, so that the next update to a shape of no more pairs allocates nothing; if that fails
    // the update has succeeded all the same and the next one tries again
    (void)geo_set_fit(sc, target ^ 1, true, N.gridList.size, N.pairRec.size, true, &allocated);
    allocated = allocated || camMade || camCapBefore[0] != sc->cam.list[0].size || camCapBefore[1] != sc->cam.list[1].size;
    G.log[0] = glog[RT_BUILD_LOG_GRID_THREAD]; G.log[1] = glog[RT_BUILD_LOG_GRID_GROUP]; G.log[2] = glog[RT_BUILD_LOG_ATTEMPTS];
    G.log[3] = pairs; G.log[4] = ctl.total; G.log[5] = allocated ? 1 : 0;
    for (int i = 0; i < 4; ++i) G.ms[i] = ms[i];
    return 0;
}

int rtHipTestSceneGeometryLog(const rtHipScene *sc, uint64_t *out, cl_uint n)
{
    if (!sc || (n && !out)) return fail("rtHipTestSceneGeometryLog: null argument");
    for (cl_uint i = 0; i < n; ++i) out[i] = i < 6 ? sc->geo.log[i] : 0;
    return 6;
}

int rtHipTestSceneGeometryTimes(const rtHipScene *sc, double ms[4])
{
    if (!sc || !ms) return fail("rtHipTestSceneGeometryTimes: null argument");
    for (int i = 0; i < 4; ++i) ms[i] = sc->geo.ms[i];
    return 0;
}

// ---- scene edits: lights and materials (include/raytrace_hip.h, "SCENE EDITS: LIGHTS AND MATERIALS") ------------------------------------

// What every edit starts with: the scene is idle (change_begin), the edit's events exist.
static int edit_begin(rtHipScene *sc, const char *who)
{
    if (const int rc = change_begin(sc, who)) return rc;
    for (Event &e : sc->edit.ev) HIP_WHO(e.make());
    return 0;
}

// What every edit ends with: other rays, so the next frame watches its queue again; the groups' views follow the description.
static void edit_end(rtHipScene *sc, double lights, double tables, double ids)
{
    derive_path_class(sc);
    sc->planRounds = 0;
    refresh_views(sc);
    sc->edit.ms[0] = lights; sc->edit.ms[1] = tables; sc->edit.ms[2] = ids;
}

int rtHipLightsCheck(const rtHipLights *lights)
{
    char text[256];
    return rtedit::lights_check(lights, text, sizeof text) == 0 ? 0 : fail("lights: %s", text);
}

int rtHipMaterialsCheck(const rtHipMaterialUpdate *update)
{
    char text[256];
    return rtedit::materials_check(update, text, sizeof text) == 0 ? 0 : fail("materials: %s", text);
}

int rtHipSceneSetLights(rtHipScene *sc, const rtHipLights *l)
{
    static const char who[] = "rtHipSceneSetLights";
    if (!sc || !l) return fail("%s: null argument", who);
    if (rtHipLightsCheck(l) != 0) return -1;
    if (const int rc = edit_begin(sc, who)) return rc;
    hipStream_t st = sc->stream;
    rtHipScene::Edit &E = sc->edit;
    const uint32_t L = l->lightCount;
    DevPart part;
    RtDevScene N = sc->dev; // (its light fields are filled here and copied over at the end)
    HIP_WHO(hipEventRecord(E.ev[0], st));
    const std::vector<float> spread = light_spreads(L, l->lightDir, l->lightRadius);
    int rc = 0;
    if ((rc = edit_put(sc, part, l->lightType, L, &N.lightType, who, "lightType")) != 0 ||
        (rc = edit_put(sc, part, (const float *)l->lightPos, (uint64_t)L * 4, &N.lightPos, who, "lightPosition")) != 0 ||
        (rc = edit_put(sc, part, (const float *)l->lightDir, (uint64_t)L * 4, &N.lightDir, who, "lightDirection")) != 0 ||
        (rc = edit_put(sc, part, (const float *)l->lightCol, (uint64_t)L * 4, &N.lightCol, who, "lightColour")) != 0 ||
        (rc = edit_put(sc, part, l->lightRadius, L, &N.lightRadius, who, "lightRadius")) != 0 ||
        (rc = edit_put(sc, part, l->lightHalfAtt, L, &N.lightHalfAtt, who, "lightHalfAttenuationDistance")) != 0 ||
        (rc = edit_put(sc, part, spread.data(), L, &N.lightSpread, who, "lightSpread")) != 0)
        return rc;
    HIP_WHO(sc->stager.drain());
    HIP_WHO(hipEventRecord(E.ev[1], st));
    // The path state only scenes of several lights use (build_wavefront: shN, rngL), made by the first edit that brings a second light
    // and kept from then on: nothing else of the path state depends on the light count, so the sample window, the launch plan's storage
    // and the groups stay as they are.
    const bool grow = L > 1u && !sc->wfMultiLight;
    std::vector<Dev<float4>> shN(grow ? sc->groups.size() : 0);
    std::vector<Dev<unsigned long long>> rngL(shN.size());
    uint64_t uncounted = 0;
    for (size_t g = 0; g < shN.size(); ++g) {
        const uint64_t cap = sc->groups[g].wf.capacity ? sc->groups[g].wf.capacity : 1;
        if (shN[g].make(cap * sizeof(float4), uncounted) != hipSuccess || rngL[g].make(cap * 8, uncounted) != hipSuccess) {
            fail("%s: no device memory for the path state of a scene of several lights", who);
            return -4;
        }
    }
    HIP_WHO(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_WHO(hipEventElapsedTime(&ms, E.ev[0], E.ev[1]));
    // everything is complete: the new lights take the old ones' place
    RtDevScene &D = sc->dev;
    D.lightCount = L;
    D.lightType = N.lightType; D.lightPos = N.lightPos; D.lightDir = N.lightDir; D.lightCol = N.lightCol;
    D.lightRadius = N.lightRadius; D.lightHalfAtt = N.lightHalfAtt; D.lightSpread = N.lightSpread;
    sc->install(PART_LIGHTS, std::move(part));
    for (size_t g = 0; g < shN.size(); ++g) { // (the one-element stand-ins stay in the part until the scene goes)
        sc->groups[g].wf.shN = shN[g]; sc->groups[g].wf.rngL = rngL[g];
        sc->parts[PART_WAVEFRONT].adopt(std::move(shN[g]));
        sc->parts[PART_WAVEFRONT].adopt(std::move(rngL[g]));
    }
    sc->bytes += uncounted; // the path-state part holds them now: what their make() summed up is counted
    if (grow) sc->wfMultiLight = true;
    sc->classLights = L <= 1u;
    edit_end(sc, ms, 0.0, 0.0);
    return 0;
}

int rtHipSceneSetMaterials(rtHipScene *sc, const rtHipMaterialUpdate *u)
{
    static const char who[] = "rtHipSceneSetMaterials";
    if (!sc || !u) return fail("%s: null argument", who);
    if (rtHipMaterialsCheck(u) != 0) return -1;
    const uint64_t T = sc->dev.triangleCount;
    HIP_WHO(hipSetDevice(sc->device));
    if (u->triMaterial && u->triMaterialOnDevice && T && query_pointer_ok(sc->device, "the scene", u->triMaterial, T * 4, 4, "triMaterial") != 0) return -1;
    if (const int rc = edit_begin(sc, who)) return rc;
    hipStream_t st = sc->stream;
    rtHipScene::Edit &E = sc->edit;

    // 1. the ids that will be in effect, checked completely before anything is stored: the new array, or -- tables that shrink under
    // ids that stay -- the resident rows
    const uint32_t M = u->replaceMaterials ? u->materialCount : sc->dev.materialCount;
    const int *ids = nullptr;
    if (u->triMaterial && T) {
        if (u->triMaterialOnDevice) ids = u->triMaterial;
        else {
            if (E.ids.fit(T * 4, T * 4, sc->bytes) != hipSuccess) { fail("%s: no device memory for the ids' staging", who); return -4; }
            HIP_WHO(sc->stager.copy(E.ids, u->triMaterial, T * 4));
            ids = E.ids;
        }
    }
    const bool check = ids || (!u->triMaterial && M < sc->dev.materialCount);
    HIP_WHO(hipEventRecord(E.ev[2], st));
    if (check) HIP_WHO(rte_launch_check_ids((uint32_t)T, M, ids, sc->dev.triShade, sc->prepErr, st));
    HIP_WHO(hipEventRecord(E.ev[3], st));
    HIP_WHO(hipStreamSynchronize(st));
    if (check && sc->check_prep() != 0) return strncmp(rtHipLastError(), "scene rejected", 14) == 0 ? -5 : -2;

    // 2. tables and atlas, beside the ones in use
    DevPart part;
    RtDevScene N = sc->dev;
    bool classMaterials = sc->classMaterials;
    HIP_WHO(hipEventRecord(E.ev[0], st));
    if (u->replaceMaterials) {
        rtHipSceneDesc d;
        memset(&d, 0, sizeof d);
        d.materialCount = u->materialCount; d.matSize = u->matSize; d.matStart = u->matStart; d.texturesSize = u->texturesSize; d.textures = u->textures;
        const std::vector<uint32_t> rec = material_records(&d); // (rtHipMaterialsCheck has checked the channel starts)
        int rc = 0;
        if ((rc = edit_put(sc, part, (const uint32_t *)u->matSize, (uint64_t)u->materialCount * 10, &N.matSize, who, "materialImageSize")) != 0 ||
            (rc = edit_put(sc, part, (const int32_t *)u->matStart, (uint64_t)u->materialCount * 5, &N.matStart, who, "materialImageStart")) != 0 ||
            (rc = edit_put(sc, part, (const uint8_t *)u->textures, (uint64_t)u->texturesSize * 4, &N.textures, who, "textures")) != 0 ||
            (rc = edit_put(sc, part, rec.data(), rec.size(), &N.matRec, who, "matRec")) != 0)
            return rc;
        N.materialCount = u->materialCount;
        N.texelCount = u->texturesSize ? u->texturesSize : 1;
        classMaterials = materials_admit_opaque_diffuse(&d);
    }
    HIP_WHO(sc->stager.drain());
    HIP_WHO(hipEventRecord(E.ev[1], st));

    // 3. the ids into the rows in use: the last thing issued, after everything that can be refused
    HIP_WHO(hipEventRecord(E.ev[4], st));
    if (ids) HIP_WHO(rte_launch_store_ids((uint32_t)T, ids, const_cast<float *>(sc->dev.triShade), st));
    HIP_WHO(hipEventRecord(E.ev[5], st));
    HIP_WHO(hipStreamSynchronize(st));
    float ms[3] = {};
    HIP_WHO(hipEventElapsedTime(&ms[0], E.ev[0], E.ev[1]));
    HIP_WHO(hipEventElapsedTime(&ms[1], E.ev[2], E.ev[3]));
    HIP_WHO(hipEventElapsedTime(&ms[2], E.ev[4], E.ev[5]));

    // 4. the new tables take the old ones' place
    if (u->replaceMaterials) {
        RtDevScene &D = sc->dev;
        D.materialCount = N.materialCount; D.texelCount = N.texelCount;
        D.matSize = N.matSize; D.matStart = N.matStart; D.textures = N.textures; D.matRec = N.matRec;
        sc->install(PART_MATERIALS, std::move(part));
        sc->classMaterials = classMaterials;
    }
    edit_end(sc, 0.0, u->replaceMaterials ? ms[0] : 0.0, check ? (double)ms[1] + ms[2] : 0.0);
    return 0;
}
#undef HIP_WHO

int rtHipSceneEditTimes(const rtHipScene *sc, double ms[3])
{
    if (!sc || !ms) return fail("rtHipSceneEditTimes: null argument");
    for (int i = 0; i < 3; ++i) ms[i] = sc->edit.ms[i];
    return 0;
}

int rtHipKernelTime(rtHipScene *sc, double *avgMs, uint64_t *launches)
{
    if (!sc || !avgMs || !launches) return fail("null argument");
    HIP_OK(hipSetDevice(sc->device));
    double total = 0.0;
    for (size_t i = 0; i < sc->eventsUsed; ++i) {
        HIP_OK(hipEventSynchronize(sc->events[i].second));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, sc->events[i].first, sc->events[i].second));
        total += ms;
    }
    *launches = sc->eventsUsed;
    *avgMs = sc->eventsUsed ? total / (double)sc->eventsUsed : 0.0;
    sc->eventsUsed = 0;
    return 0;
}

// ---- drop-in layer ---------------------------------------------------------------------------------------------

// device table, published last like raytrace.c:117-120
static std::atomic<cl_bool> g_tableReady{ CL_FALSE };
static std::atomic<int> g_deviceCount{ 0 };
static char g_deviceName[256][256];
static std::mutex g_tableMutex;

void InitOpenCL(void)
{
    std::lock_guard<std::mutex> lock(g_tableMutex);
    char names[256][256];
    int n = rtHipDeviceCount();
    if (n > 254) n = 254;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t prop;
        memset(&prop, 0, sizeof prop);
        if (hipGetDeviceProperties(&prop, i) != hipSuccess) strcpy(prop.name, "unknown");
        snprintf(names[i], 256, "AMD HIP %.200s #%d", prop.name, i);
    }
    int entries = n;
    if (n > 1) snprintf(names[entries++], 256, "AMD HIP all %d GPUs (tiled)", n);
    memcpy(g_deviceName, names, sizeof(names[0]) * (size_t)entries);
    g_deviceCount.store(entries, std::memory_order_relaxed);
    g_tableReady.store(CL_TRUE, std::memory_order_release);
}

void ResetComputationType(void)
{
    if (g_tableReady.load(std::memory_order_acquire)) {
        g_tableReady.store(CL_FALSE, std::memory_order_relaxed);
        g_deviceCount.store(0, std::memory_order_relaxed);
    }
}

cl_bool GetIsComputationTypeUpdated(void) { return g_tableReady.load(std::memory_order_acquire); }

size_t GetComputationTypeCount(void) { return 1 + (size_t)g_deviceCount.load(std::memory_order_relaxed); }

cl_bool GetComputationTypeName(size_t id, size_t strLen, cl_char *str)
{
    if (!str) return CL_FALSE;
    if (0 == id--) {
        static const char cpu[] = "Local CPU single thread"; // raytrace.c:138
        if (strlen(cpu) <= strLen) { strcpy((char *)str, cpu); return CL_TRUE; }
    } else if (id < (size_t)g_deviceCount.load(std::memory_order_relaxed)) {
        if (strlen(g_deviceName[id]) <= strLen) {
            memcpy(str, g_deviceName[id], std::min<size_t>(256, strLen)); // raytrace.c:147
            return CL_TRUE;
        }
    }
    return CL_FALSE;
}

static std::atomic<float> g_progress{ 0.f };
static std::atomic<long> g_startTime{ 0 }, g_endTime{ 0 };

cl_float GetProgress(void) { return g_progress.load(std::memory_order_relaxed); }
void SetProgress(cl_float p) { g_progress.store(p, std::memory_order_relaxed); }
clock_t GetStartTime(void) { return (clock_t)g_startTime.load(std::memory_order_relaxed); }
clock_t GetEndTime(void) { return (clock_t)g_endTime.load(std::memory_order_relaxed); }
void ResetTime(void) { g_startTime.store(0, std::memory_order_relaxed); g_endTime.store(0, std::memory_order_relaxed); }

} // extern "C"

// ---- the drop-in layer's scene cache ("next" row 2) ---------------------------------------------------------
// The reference rebuilds everything on every call: program, 35 buffers, tiles x samples launches (raytrace.c:330-489).  A second
// Render click usually changes the camera, sometimes the sample count, rarely the scene.  The scenes of the last call stay in
// HBM; the next call hashes its input arrays (all host threads, a few ms for a 1 M-triangle scene) and rebuilds only the parts
// whose hash changed: geometry + grid + materials are the expensive ones (upload, triangle records, dense grid view), the
// camera lists, the lights and the path-state buffers are cheap.  RT_HIP_CACHE=0 switches the cache off (every call builds and
// frees, like the reference); rtHipCacheClear() frees what is held.
namespace {

inline uint64_t mix64(uint64_t v)
{
    v ^= v >> 32; v *= 0xd6e8feb86659fd93ull; v ^= v >> 32; v *= 0xd6e8feb86659fd93ull; v ^= v >> 32;
    return v;
}

// content hash of one chunk: four independent multiply-rotate lanes over 32-byte blocks, then the tail
uint64_t hash_chunk(const unsigned char *p, size_t n)
{
    uint64_t a = 0x9e3779b97f4a7c15ull, b = 0xc2b2ae3d27d4eb4full, c = 0x165667b19e3779f9ull, d = 0x27d4eb2f165667c5ull;
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        uint64_t w[4];
        memcpy(w, p + i, 32);
        a = (a ^ w[0]) * 0x9fb21c651e98df25ull; a = (a << 29) | (a >> 35);
        b = (b ^ w[1]) * 0x9fb21c651e98df25ull; b = (b << 29) | (b >> 35);
        c = (c ^ w[2]) * 0x9fb21c651e98df25ull; c = (c << 29) | (c >> 35);
        d = (d ^ w[3]) * 0x9fb21c651e98df25ull; d = (d << 29) | (d >> 35);
    }
    // the tail (< 32 bytes): whole 8-byte words folded one by one, then the last partial word -- each assembled in a zeroed word
    // of its own, so that no byte is ever ORed over another one's bits
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        memcpy(&w, p + i, 8);
        a = mix64(a ^ w);
    }
    uint64_t tail = 0;
    if (i < n) memcpy(&tail, p + i, n - i);
    return mix64(a ^ mix64(b ^ mix64(c ^ mix64(d ^ tail ^ (uint64_t)n))));
}

struct HashJob { const void *ptr; size_t bytes; int group; };

// hashes of the five input groups (geometry, grid, materials, lights, camera), computed chunk-parallel
void hash_inputs(const std::vector<HashJob> &jobs, uint64_t out[5])
{
    struct Chunk { const unsigned char *p; size_t n; uint64_t h; int group; };
    std::vector<Chunk> chunks;
    const size_t piece = (size_t)2 << 20;
    for (const HashJob &j : jobs) {
        const unsigned char *p = (const unsigned char *)j.ptr;
        size_t left = p ? j.bytes : 0;
        chunks.push_back(Chunk{ nullptr, j.bytes, 0, j.group }); // the length always counts, also for an empty array
        while (left) { const size_t n = std::min(piece, left); chunks.push_back(Chunk{ p, n, 0, j.group }); p += n; left -= n; }
    }
    unsigned threads = std::thread::hardware_concurrency();
    threads = std::max(1u, std::min(threads ? threads : 1u, 16u));
    std::atomic<size_t> next{ 0 };
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < chunks.size();)
            chunks[i].h = chunks[i].p ? hash_chunk(chunks[i].p, chunks[i].n) : mix64(chunks[i].n + 0x51ull);
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    for (int g = 0; g < 5; ++g) out[g] = 0x12345678u + g;
    for (const Chunk &c : chunks) out[c.group] = mix64(out[c.group] * 0x100000001b3ull ^ c.h);
}

struct SceneCache {
    std::vector<rtHipScene *> scenes;
    std::vector<std::vector<cl_uint>> tiles; // per scene: its tile ids (empty = all)
    int first = 0, count = 0, devices = 0;
    Tuning tune;               // the tuning values the scenes were built with: other values, other scenes
    uint32_t width = 0, height = 0, sampleCount = 0;
    uint64_t hash[5] = { 0 };
    bool valid = false;
    // gather root (device `first`): row-major planes and, for several scenes, the peers' tile buffers
    Dev<uint16_t> planes, gather;
    Dev<uint32_t> gatherIds;
    uint64_t bytes = 0; // (of these three; no scene counts them)
    size_t gatherTiles = 0;
    void clear()
    {
        for (rtHipScene *s : scenes) rtHipSceneDestroy(s);
        scenes.clear(); tiles.clear();
        if (valid || planes || gather || gatherIds) {
            if (devices > 0) (void)hipSetDevice(first % devices);
            planes.drop(bytes); gather.drop(bytes); gatherIds.drop(bytes);
        }
        gatherTiles = 0;
        valid = false;
    }
};
SceneCache &g_cache = *new SceneCache(); // (never destroyed: nothing is freed on the device during process exit)
std::mutex g_cacheMutex;

} // namespace

extern "C" {

int rtHipTune(const char *key, double value)
{
    if (!key) return fail("rtHipTune: null key");
    std::lock_guard<std::mutex> lock(g_tuneMutex);
    Tuning &T = g_tune;
    const std::string k = key;
    if (k == "reset") { T = Tuning(); return 0; }
    if (k == "matte_chunk") { // (the one key with a smallest legal value: a chunk of no samples would never end)
        if (!(value >= 1.0 && value <= 65536.0)) return fail("rtHipTune: matte_chunk %g is not in 1..65536", value);
        T.matteChunk = (uint32_t)value;
        return 0;
    }
    // every key's field, 32 or 64 bits wide, and the most it takes: negative values become 0, larger ones saturate at `most`
    struct Key { const char *name; uint32_t *f32; uint64_t *f64 = nullptr; double most = 4294967295.0; } table[] = {
        { "stage_mb", &T.stageMb }, { "extra_factor", &T.extraFactor }, { "groups", &T.groups }, { "lookahead", &T.lookAhead },
        { "seg0", &T.segLen[0] }, { "seg1", &T.segLen[1] }, { "seg2", &T.segLen[2] }, { "seg3", &T.segLen[3] }, { "seg4", &T.segLen[4] },
        { "seg_rays0", &T.segRays[0] }, { "seg_rays1", &T.segRays[1] }, { "seg_rays2", &T.segRays[2] }, { "seg_rays3", &T.segRays[3] },
        { "fast_quotient", &T.fastQuotient }, { "spin_limit", &T.spinLimit }, { "append_rays", &T.appendRays }, { "ordered_first", &T.orderedFirst }, { "slice_rays", &T.sliceRays },
        { "small_slices", &T.smallSlices }, { "group_rays", &T.groupRays }, { "blocking", &T.blocking }, { "plan_rounds", &T.planRounds }, { "plan_grid_tiny", &T.planGridTiny }, { "plan_shade_skip", &T.planShadeSkip }, { "visit_log", &T.visitLog },
        { "pipeline", &T.pipeline }, { "timing", &T.timing }, { "virtual_devices", &T.virtualDevices }, { "cache", &T.cache }, { "batch_plan", &T.batchPlan },
        { "logic_class", &T.logicClass }, { "dead_shadow", &T.deadShadow }, { "ray_clip", &T.rayClip }, { "logic_split", &T.logicSplit }, { "place_direct", &T.placeDirect }, { "place_skew", &T.placeSkew }, { "query_rays", &T.queryRays, nullptr, 1u << 26 },
        { "ao_samples", &T.aoSamples, nullptr, 1u << 22 }, { "bake_texels", &T.bakeTexels, nullptr, 1u << 24 },
        { "state_mb", nullptr, &T.stateMb, HUGE_VAL }, { "build_key_cap", nullptr, &T.buildKeyCap, 1e18 }, { "build_list_limit", nullptr, &T.buildListLimit },
    };
    for (const Key &e : table) {
        if (k != e.name) continue;
        const double v = value < 0 ? 0 : std::min(value, e.most);
        if (e.f64) *e.f64 = (uint64_t)v; else *e.f32 = (uint32_t)v;
        return 0;
    }
    return fail("rtHipTune: unknown key '%s'", key);
}

int rtHipTestCachePointers(const void *out[6])
{
    if (!out) return -1;
    std::lock_guard<std::mutex> lock(g_cacheMutex);
    if (!g_cache.valid || g_cache.scenes.empty() || !g_cache.scenes[0]) return -2;
    const RtDevScene &D = g_cache.scenes[0]->dev;
    out[0] = D.triRec; out[1] = D.triShade; out[2] = D.pairRec; out[3] = D.matRec; out[4] = D.textures; out[5] = D.camList;
    return 0;
}

int rtHipTestPathClass(const rtHipScene *scene)
{
    if (!scene) return -1;
    return (int)scene->dev.pathClass;
}

int rtHipTestShadeKat(const rtHipScene *scene, int op, uint32_t count, const void *in, void *out)
{
    if (!scene || (count && (!in || !out))) return -1;
    const RtDevScene &D = scene->dev;
    // every index the kernel reads through is checked here: the kernel trusts its items
    for (uint32_t i = 0; i < count; ++i) {
        if (op == RT_SHADE_KAT_TEXEL) {
            const int32_t *item = reinterpret_cast<const int32_t *>(in) + 10 * (size_t)i;
            if (D.texelCount == 0u || item[0] < 0 || (uint32_t)item[0] >= D.materialCount || item[1] < 0 || item[1] >= 5) return -1;
        } else if (op == RT_SHADE_KAT_NORMAL) {
            if (reinterpret_cast<const uint32_t *>(in)[12 * (size_t)i] >= D.triangleCount) return -1;
        } else return -1;
    }
    if (op == RT_SHADE_KAT_NORMAL && count && D.texelCount == 0u && D.materialCount) return -1; // (a height map fetch needs an atlas)
    if (hipSetDevice(scene->device) != hipSuccess || hipStreamSynchronize(scene->stream) != hipSuccess) return -3;
    return rt_shade_kat_run(&D, op, count, in, out);
}

int rtHipTestRoundLog(const rtHipScene *scene, uint32_t *rays, uint32_t n)
{
    if (!scene || (n && !rays)) return -1;
    const uint32_t rounds = (uint32_t)std::min<uint64_t>(scene->roundsLast, RT_WF_ROUND_LOG);
    for (uint32_t r = 0; r < n; ++r) {
        uint64_t sum = 0;
        if (r < rounds)
            for (const auto &G : scene->groups) sum += G.hostLog[r].x; // (mapped host memory, written by the logic kernels)
        rays[r] = (uint32_t)std::min<uint64_t>(sum, 0xffffffffu);
    }
    return (int)scene->roundsLast;
}

int rtHipTestRoundVisits(const rtHipScene *scene, uint64_t *out, uint32_t rounds)
{
    if (!scene || (rounds && !out)) return fail("rtHipTestRoundVisits: null argument");
    if (!scene->tune.visitLog) return fail("rtHipTestRoundVisits: the scene was built without the test hook visit_log");
    for (uint32_t r = 0; r < rounds; ++r)
        for (uint32_t f = 0; f < RT_ROUND_VISIT_FIELDS; ++f) out[(size_t)RT_ROUND_VISIT_FIELDS * r + f] = r < scene->visitLog.size() ? scene->visitLog[r][f] : 0;
    return (int)std::min<uint64_t>(scene->roundsLast, 0x7fffffffu);
}

int rtHipTestShadeLog(const rtHipScene *scene, uint32_t *listed, uint32_t n)
{
    if (!scene || (n && !listed)) return -1;
    const uint32_t rounds = (uint32_t)std::min<uint64_t>(scene->roundsLast, RT_WF_ROUND_LOG);
    for (uint32_t r = 0; r < n; ++r) {
        uint64_t sum = 0;
        if (r < rounds)
            for (const auto &G : scene->groups) sum += G.hostLog[r].w; // (mapped host memory, written by the shade passes)
        listed[r] = (uint32_t)std::min<uint64_t>(sum, 0xffffffffu);
    }
    return (int)std::min<uint64_t>(scene->splitRoundsLast, 0x7fffffffu);
}

int rtHipTestPlaceLog(const rtHipScene *scene, uint32_t out[2])
{
    if (!scene || !out) return -1;
    out[0] = scene->directRoundsLast;
    out[1] = scene->scatterLaunchesLast;
    return 0;
}

int rtHipTestPlaceView(const rtHipScene *scene, uint32_t round, uint32_t *table, uint32_t *entries, uint32_t positions)
{
    static_assert(RT_PLACE_TABLE_ROUNDS == RT_WF_PLACE_ROUNDS && RT_PLACE_TABLE_WORDS == RT_WF_PLACE_WORDS, "the header's figures are the device's");
    if (!scene || scene->groups.empty() || round < 1u || round > RT_WF_PLACE_ROUNDS) return fail("rtHipTestPlaceView: invalid argument");
    const RtWavefront &W = scene->groups[0].wf;
    if ((uint64_t)positions > 2ull * W.capacity + W.extraCap) return fail("rtHipTestPlaceView: %u positions reach past the entry array", positions);
    HIP_OK(hipSetDevice(scene->device));
    HIP_OK(hipStreamSynchronize(scene->stream));
    if (table) HIP_OK(hipMemcpy(table, W.ctl + RT_WF_PLACE_AT(round), sizeof(uint32_t) * RT_WF_PLACE_WORDS, hipMemcpyDeviceToHost));
    if (entries && positions) HIP_OK(hipMemcpy(entries, W.ent[round & 1u], (size_t)64 * positions, hipMemcpyDeviceToHost));
    return 0;
}

int rtHipTestSceneView(const rtHipScene *scene, int what, uint64_t firstElement, uint64_t count, void *out)
{
    if (!scene) return fail("rtHipTestSceneView: null scene");
    const RtDevScene &D = scene->dev;
    const uint32_t header[5] = { D.planesTame, D.tileCount, D.tilesX, D.triangleCount, (uint32_t)scene->gridListSize };
    const uint64_t tilePixels = (uint64_t)D.tileCount * RT_TILE_PIXELS, blocks = (uint64_t)(RT_GRID_DIV / 4) * (RT_GRID_DIV / 4) * (RT_GRID_DIV / 4);
    struct View { const void *ptr; uint64_t elements, elementBytes; bool host; } v;
    uint64_t pitch = 0; // bytes from one element to the next on the device, where that is more than the view's elementBytes
    switch (what) {
    case RT_SCENE_VIEW_HEADER: v = { header, 5, 4, true }; break;
    case RT_SCENE_VIEW_CAM_START: v = { D.camStart, tilePixels, 4, false }; break;
    case RT_SCENE_VIEW_CAM_END: v = { D.camEnd, tilePixels, 4, false }; break;
    case RT_SCENE_VIEW_TRI_REC: v = { D.triRec, D.triangleCount, 64, false }; break;
    case RT_SCENE_VIEW_TRI_SHADE: v = { D.triShade, D.triangleCount, 96, false }; pitch = RT_TRI_SHADE_WORDS * 4; break; // the packed words of each row
    case RT_SCENE_VIEW_TRI_SHADE_ROW: v = { D.triShade, D.triangleCount, RT_TRI_SHADE_WORDS * 4, false }; break;
    case RT_SCENE_VIEW_GRID_BITS: v = { D.gridBits, blocks, 8, false }; break;
    case RT_SCENE_VIEW_BLOCK_SPARSE: v = { D.gridBlockSparse, (uint64_t)3 * ((63u << 16 | 63u << 8 | 63u) + 1u), 4, false }; break;
    case RT_SCENE_VIEW_PAIR_REC: v = { D.pairRec, scene->gridListSize, 64, false }; break;
    case RT_SCENE_VIEW_CELL_LUT: v = { D.cellLut, 3 * 256, 1, false }; break;
    // (what the planning kernels read, behind the planes on the device -- not the host's copy)
    case RT_SCENE_VIEW_CLIP_PLANES: v = { D.boxMin ? D.boxMin + RT_CLIP_AT + 4 : nullptr, scene->clipCount, 16, false }; break;
    case RT_SCENE_VIEW_CLIP_APPLIED: v = { D.boxMin ? D.boxMin + RT_CLIP_AT : nullptr, 1, 4, false }; break;
    default: return fail("rtHipTestSceneView: unknown array %d", what);
    }
    if (v.elements > 0x7fffffffull) return fail("rtHipTestSceneView: array %d has %llu elements", what, (unsigned long long)v.elements);
    if (!out) return (int)v.elements;
    if (firstElement > v.elements || count > v.elements - firstElement)
        return fail("rtHipTestSceneView: elements %llu + %llu reach past the %llu of array %d", (unsigned long long)firstElement,
                    (unsigned long long)count, (unsigned long long)v.elements, what);
    if (!count) return 0;
    if (v.host) { memcpy(out, (const char *)v.ptr + firstElement * v.elementBytes, count * v.elementBytes); return 0; }
    if (!v.ptr) return fail("rtHipTestSceneView: the scene does not hold array %d", what);
    HIP_OK(hipSetDevice(scene->device));
    HIP_OK(hipStreamSynchronize(scene->stream));
    if (pitch) { HIP_OK(hipMemcpy2D(out, v.elementBytes, (const char *)v.ptr + firstElement * pitch, pitch, v.elementBytes, count, hipMemcpyDeviceToHost)); }
    else { HIP_OK(hipMemcpy(out, (const char *)v.ptr + firstElement * v.elementBytes, count * v.elementBytes, hipMemcpyDeviceToHost)); }
    return 0;
}

int rtHipScenePathClass(const rtHipSceneDesc *desc)
{
    if (!desc) return fail("rtHipScenePathClass: null scene description");
    if (desc->arraysOnDevice) return fail("rtHipScenePathClass: the description's arrays are device memory");
    if (desc->materialCount && (!desc->matSize || !desc->matStart || !desc->textures)) return fail("rtHipScenePathClass: null material array");
    for (uint32_t i = 0; i < desc->materialCount * 5; ++i)
        if (desc->matSize[i].s[0] == 1u && desc->matSize[i].s[1] == 1u && ((int64_t)desc->matStart[i] < 0 || (uint64_t)desc->matStart[i] >= desc->texturesSize))
            return fail("rtHipScenePathClass: material channel %u starts outside the atlas", i);
    return (materials_admit_opaque_diffuse(desc) && lights_admit_opaque_diffuse(desc)) ? RT_PATH_CLASS_OPAQUE_DIFFUSE : RT_PATH_CLASS_GENERAL;
}

uint64_t rtHipTestHashBytes(const void *bytes, uint64_t count) { return hash_chunk((const unsigned char *)bytes, (size_t)count); }

void rtHipCacheClear(void)
{
    std::lock_guard<std::mutex> lock(g_cacheMutex);
    const std::string keep = g_error;
    g_cache.clear();
    g_error = keep;
}

cl_bool RaytraceAll(cl_uint computationType, cl_uint2 cameraImageDimension, cl_float3 cameraEye, cl_float3 cameraEyeToTopLeftVector,
                    cl_float3 cameraLeftToRightPixelSizeVector, cl_float3 cameraTopToBottomPixelSizeVector, cl_float cameraPixelSizeInv,
                    cl_uint *cameraPixelTriangleListStart, cl_uint *cameraPixelTriangleListEnd, cl_uint *cameraPixelTriangleList,
                    ptrdiff_t cameraPixelTriangleListSize, cl_uint sampleCount, cl_uint vertexCount, cl_float3 *vertex,
                    cl_uint triangleCount, cl_int3 *triangleVertexIndex, cl_int *triangleMaterialId, cl_float2 *triangleUv,
                    cl_float3 *triangleNormal, cl_int axesDivCount, cl_float3 *sceneBoxMin, cl_uint *scenePixelTriangleListStart,
                    cl_uint *scenePixelTriangleList, cl_uint materialCount, cl_uint2 *materialImageSize, cl_int *materialImageStart,
                    cl_uint texturesSize, cl_uchar3 *textures, cl_uint lightCount, cl_int *lightType, cl_float3 *lightPosition,
                    cl_float3 *lightDirection, cl_float3 *lightColour, cl_float *lightRadius, cl_float *lightHalfAttenuationDistance,
                    cl_ushort *outputRed, cl_ushort *outputGreen, cl_ushort *outputBlue)
{
    g_error.clear();
    auto refuse = [&](const char *why) -> cl_bool {
        fprintf(stderr, "libraytrace_hip: %s\n", why);
        return CL_FALSE;
    };
    if (computationType == 0) {
        // The reference's id 0 is its own in-thread C loop (raytrace.c:604-655).  This library is the device path
        // only; falling back to a CPU here would hide a missing GPU.  Fail loudly.
        fail("RaytraceAll: computationType 0 (\"Local CPU single thread\") is the reference's own C path and is not "
             "provided by libraytrace_hip; pick a HIP device (computationType >= 1)");
        return refuse(g_error.c_str());
    }
    const int n = rtHipDeviceCount();
    // "All GPUs": one scene per device with the tiles dealt round-robin, one host thread per device while the scenes are built
    // and the first frame watches its ray queue.  RT_HIP_VIRTUAL_DEVICES=k (test hook): the all-GPUs id deals the tiles over k
    // instances that share the real devices, so the path runs on a one-GPU box.
    const Tuning tune = tuning();
    const int virt = (int)tune.virtualDevices;
    const bool all = (n > 1 && computationType == (cl_uint)n + 1);
    const bool allVirtual = n > 0 && virt > 1 && computationType == (cl_uint)n + 1;
    if (n <= 0 || (!all && !allVirtual && computationType > (cl_uint)n)) {
        fail("RaytraceAll: computationType %u but %d HIP device(s) present", computationType, n);
        return refuse(g_error.c_str());
    }
    if (!outputRed || !outputGreen || !outputBlue) { fail("RaytraceAll: null output plane"); return CL_FALSE; }

    rtHipSceneDesc d;
    memset(&d, 0, sizeof d);
    d.width = cameraImageDimension.s[0]; d.height = cameraImageDimension.s[1];
    for (int i = 0; i < 3; ++i) {
        d.eye[i] = cameraEye.s[i]; d.eyeToTopLeft[i] = cameraEyeToTopLeftVector.s[i];
        d.leftToRight[i] = cameraLeftToRightPixelSizeVector.s[i]; d.topToBottom[i] = cameraTopToBottomPixelSizeVector.s[i];
    }
    d.pixelSizeInv = cameraPixelSizeInv;
    d.camStart = cameraPixelTriangleListStart; d.camEnd = cameraPixelTriangleListEnd; d.camList = cameraPixelTriangleList;
    d.camListSize = cameraPixelTriangleListSize < 0 ? 0 : (uint64_t)cameraPixelTriangleListSize;
    d.sampleCount = sampleCount;
    d.vertexCount = vertexCount; d.vertex = vertex;
    d.triangleCount = triangleCount; d.triIndex = triangleVertexIndex; d.triMaterial = triangleMaterialId;
    d.triUv = triangleUv; d.triNormal = triangleNormal;
    d.axesDiv = axesDivCount; d.boxMin = sceneBoxMin; d.gridStart = scenePixelTriangleListStart; d.gridList = scenePixelTriangleList;
    d.materialCount = materialCount; d.matSize = materialImageSize; d.matStart = materialImageStart;
    d.texturesSize = texturesSize; d.textures = textures;
    d.lightCount = lightCount; d.lightType = lightType; d.lightPos = lightPosition; d.lightDir = lightDirection;
    d.lightCol = lightColour; d.lightRadius = lightRadius; d.lightHalfAtt = lightHalfAttenuationDistance;
    if (d.width == 0 || d.height == 0 || (uint64_t)d.width * d.height > 0xffffffffull) { fail("RaytraceAll: bad image size %ux%u", d.width, d.height); return refuse(g_error.c_str()); }
    if (d.axesDiv != RT_GRID_DIV || !d.gridStart) { fail("RaytraceAll: axesDivCount %d / null grid (the reference builds %d, trianglelist.h:110)", d.axesDiv, RT_GRID_DIV); return refuse(g_error.c_str()); }

    const size_t P = (size_t)d.width * d.height;
    const bool every = all || allVirtual;
    const int first = every ? 0 : (int)computationType - 1, count = allVirtual ? virt : (all ? n : 1);
    const uint32_t tilesTotal = ((d.width + RT_TILE - 1) / RT_TILE) * ((d.height + RT_TILE - 1) / RT_TILE);
    g_progress.store(0.f, std::memory_order_relaxed);
    const long t0 = (long)clock();
    g_startTime.store(t0 ? t0 : 1, std::memory_order_relaxed); // must read non-zero once the kernel phase begins
    g_endTime.store(t0 ? t0 : 1, std::memory_order_relaxed);

    // ---- what changed since the last call? ---------------------------------------------------------------------------------
    const uint64_t cells = (uint64_t)RT_GRID_DIV * RT_GRID_DIV * RT_GRID_DIV;
    const uint64_t gridListSize = d.gridStart[cells];
    uint64_t h[5];
    const auto tCall = std::chrono::steady_clock::now();
    {
        const uint32_t scalars[4] = { d.vertexCount, d.triangleCount, d.materialCount, d.texturesSize }; // (light count and image size have their own groups / keys)
        std::vector<HashJob> jobs = {
            { d.vertex, (size_t)d.vertexCount * 16, 0 }, { d.triIndex, (size_t)d.triangleCount * 16, 0 }, { d.triMaterial, (size_t)d.triangleCount * 4, 0 },
            { d.triUv, (size_t)d.triangleCount * 24, 0 }, { d.triNormal, (size_t)d.triangleCount * 48, 0 }, { scalars, sizeof scalars, 0 },
            { d.boxMin, (size_t)(RT_GRID_DIV + 1) * 16, 1 }, { d.gridStart, (size_t)(cells + 1) * 4, 1 }, { d.gridList, (size_t)gridListSize * 4, 1 },
            { d.matSize, (size_t)d.materialCount * 40, 2 }, { d.matStart, (size_t)d.materialCount * 20, 2 }, { d.textures, (size_t)d.texturesSize * 4, 2 },
            { d.lightType, (size_t)d.lightCount * 4, 3 }, { d.lightPos, (size_t)d.lightCount * 16, 3 }, { d.lightDir, (size_t)d.lightCount * 16, 3 },
            { d.lightCol, (size_t)d.lightCount * 16, 3 }, { d.lightRadius, (size_t)d.lightCount * 4, 3 }, { d.lightHalfAtt, (size_t)d.lightCount * 4, 3 },
            { d.camStart, P * 4, 4 }, { d.camEnd, P * 4, 4 }, { d.camList, (size_t)d.camListSize * 4, 4 }, { d.eye, 4 * 17, 4 },
        };
        hash_inputs(jobs, h);
    }
    const bool timing = tune.timing != 0;
    const auto tHash = std::chrono::steady_clock::now();

    std::lock_guard<std::mutex> lock(g_cacheMutex);
    SceneCache &C = g_cache;
    const bool useCache = tune.cache != 0;
    const bool sameSet = useCache && C.valid && C.first == first && C.count == count && C.devices == n && C.width == d.width && C.height == d.height &&
                         (int)C.scenes.size() == count && memcmp(&C.tune, &tune, sizeof tune) == 0;
    // What is rebuilt.  Geometry (triangle records), grid (its dense view holds copies of triangle records: it follows the geometry),
    // materials, lights, camera lists and the path-state buffers are separate parts of a resident scene, each behind its own gate: a
    // changed texel re-bakes the materials and leaves the 260 MB of geometry and grid of a 1 M-triangle scene where they are.
    const bool geometryChanged = !sameSet || C.hash[0] != h[0];
    const bool gridChanged = geometryChanged || C.hash[1] != h[1];
    const bool materialsChanged = !sameSet || C.hash[2] != h[2];
    const bool lightsChanged = !sameSet || C.hash[3] != h[3];
    const bool cameraChanged = !sameSet || C.hash[4] != h[4];
    const bool samplesChanged = !sameSet || C.sampleCount != d.sampleCount;
    const bool reuse = sameSet;
    if (!sameSet) {
        C.clear();
        C.first = first; C.count = count; C.devices = n; C.width = d.width; C.height = d.height; C.tune = tune;
        C.scenes.assign((size_t)count, nullptr);
        C.tiles.assign((size_t)count, std::vector<cl_uint>());
        if (count > 1)
            for (int g = 0; g < count; ++g)
                for (uint32_t t = (uint32_t)g; t < tilesTotal; t += (uint32_t)count) C.tiles[g].push_back(t); // round-robin tile deal
    }
    std::vector<std::string> errors((size_t)count);
    std::vector<char> failed((size_t)count, 0);
    // build or update one device's scene; errors are thread-local, so they are carried out by hand.  Instance 0 goes first: the others
    // copy the parts all instances hold alike from it, device to device (clone_part), instead of uploading and reshaping them again
    auto build = [&](int g) -> bool {
        if (count > 1 && C.tiles[g].empty()) return true; // more instances than tiles
        bool ok = true;
        const rtHipScene *root = g > 0 ? C.scenes[0] : nullptr;
        if (!C.scenes[g]) {
            C.scenes[g] = scene_create((first + g) % n, &d, C.tiles[g].empty() ? nullptr : C.tiles[g].data(), (cl_uint)C.tiles[g].size(), root, tune);
            ok = C.scenes[g] != nullptr;
        } else {
            rtHipScene *sc = C.scenes[g];
            ok = hipSetDevice(sc->device) == hipSuccess;
            if (ok && geometryChanged) ok = (root ? clone_part(sc, root, PART_GEOMETRY) : build_geometry(sc, &d)) == 0;
            if (ok && gridChanged) ok = (root ? clone_part(sc, root, PART_GRID) : build_grid(sc, &d)) == 0;
            if (ok && materialsChanged) ok = (root ? clone_part(sc, root, PART_MATERIALS) : build_materials(sc, &d)) == 0;
            if (ok && lightsChanged) ok = (root ? clone_part(sc, root, PART_LIGHTS) : build_lights(sc, &d)) == 0;
            if (ok && cameraChanged) ok = build_camera(sc, &d) == 0;
            if (ok && (cameraChanged || geometryChanged)) // ids inside the list against the triangles there are now: one look at the validation word
                ok = rtp_validate(sc->dev.triangleCount, 0, 0, nullptr, nullptr, sc->camListSize, sc->dev.camList, nullptr, 0, nullptr, sc->prepErr, sc->stream) == hipSuccess &&
                     hipStreamSynchronize(sc->stream) == hipSuccess && sc->check_prep() == 0;
            if (ok && (samplesChanged || (sc->dev.lightCount > 1) != sc->wfMultiLight)) ok = build_wavefront(sc, d.sampleCount) == 0;
            if (ok && (lightsChanged || cameraChanged || gridChanged || materialsChanged)) sc->planRounds = 0; // other rays: the next frame watches its queue again
            if (ok) refresh_views(sc);
        }
        if (!ok) { failed[g] = 1; errors[g] = g_error; }
        return ok;
    };
    auto work = [&](int g, bool built) { // (instance 0 is built before the threads start), then render the instance's share
        if (count > 1 && C.tiles[g].empty()) return;
        bool ok = built || build(g);
        if (failed[g]) return;
        if (ok) {
            rtHipScene *sc = C.scenes[g];
            sc->progress = &g_progress;
            sc->progressBase = 0.999f * (float)g / (float)count;
            sc->progressSpan = 0.999f / (float)count;
            sc->eventsUsed = 0; // one event pair per call: nobody asks the drop-in layer for kernel times, and a cached scene lives on
            ok = rtHipRenderTiles(sc, nullptr) == 0;
            if (ok && sc->unverified) { // a planned frame runs without the host: follow the batch counter its kernels bump
                const uint32_t batches = (d.sampleCount + sc->samplesPerBatch - 1) / sc->samplesPerBatch * (uint32_t)sc->groups.size();
                uint32_t before = 0;
                for (auto &G : sc->groups) before += G.hostStatus[RT_WF_STATUS_BATCHES];
                while (hipStreamQuery(sc->stream) == hipErrorNotReady) {
                    uint32_t now = 0;
                    for (auto &G : sc->groups) now += G.hostStatus[RT_WF_STATUS_BATCHES];
                    g_progress.store(sc->progressBase + sc->progressSpan * (float)std::min(now - before, batches) / (float)batches, std::memory_order_relaxed);
                    std::this_thread::sleep_for(std::chrono::microseconds(200));
                }
            }
            ok = ok && rtHipSync(sc, nullptr) == 0;
            sc->progress = nullptr;
        }
        if (!ok) { failed[g] = 1; errors[g] = g_error; }
    };
    const bool rootBuilt = build(0);
    if (count == 1) { if (rootBuilt) work(0, true); }
    else if (rootBuilt) {
        std::vector<std::thread> pool;
        for (int g = 0; g < count; ++g) pool.emplace_back(work, g, g == 0);
        for (auto &t : pool) t.join();
    }
    bool ok = true;
    for (int g = 0; g < count; ++g)
        if (failed[g]) { ok = false; g_error = errors[g]; }
    const auto tRender = std::chrono::steady_clock::now();

    // ---- gather on the root device: peers' tile buffers over the fabric, one de-tiling launch, one copy per plane to the caller -----
    if (ok) {
        auto gather = [&]() -> int {
            rtHipScene *root = nullptr;
            for (rtHipScene *s : C.scenes) if (s) { root = s; break; }
            if (!root) return fail("RaytraceAll: nothing to render");
            HIP_OK(hipSetDevice(root->device));
            if (!C.planes) HIP_OK(C.planes.make(3 * P * sizeof(uint16_t), C.bytes));
            // (the ABI's planes are zeroed first, raytrace.c:476,481,486, and every pixel belongs to exactly one tile of the deal:
            // the de-tiling launch simply writes them)
            const void *tileBuf = root->dev.tileBuf;
            const cl_uint *ids = root->dev.tileIds;
            size_t tiles = root->tileIds.size();
            if (count > 1) {
                // [scene][slot] tile buffers next to each other on the root, ids alongside; a peer's buffer travels device to device
                size_t total = 0;
                for (rtHipScene *s : C.scenes) if (s) total += s->tileIds.size();
                if (C.gatherTiles != total) {
                    C.gather.drop(C.bytes); C.gatherIds.drop(C.bytes);
                    HIP_OK(C.gather.make(total * 3 * RT_TILE_PIXELS * sizeof(uint16_t), C.bytes));
                    HIP_OK(C.gatherIds.make(total * sizeof(uint32_t), C.bytes));
                    std::vector<uint32_t> allIds;
                    for (rtHipScene *s : C.scenes) if (s) allIds.insert(allIds.end(), s->tileIds.begin(), s->tileIds.end());
                    HIP_OK(hipMemcpy(C.gatherIds, allIds.data(), total * sizeof(uint32_t), hipMemcpyHostToDevice));
                    C.gatherTiles = total;
                }
                size_t at = 0;
                for (rtHipScene *s : C.scenes) {
                    if (!s) continue;
                    const size_t bytes = s->tileIds.size() * 3 * RT_TILE_PIXELS * sizeof(uint16_t);
                    HIP_OK(hipMemcpyPeerAsync(C.gather.as<char>() + at, root->device, s->dev.tileBuf, s->device, bytes, root->stream)); // (the scenes were synchronised above)
                    at += bytes;
                }
                tileBuf = C.gather; ids = C.gatherIds; tiles = total;
            }
            HIP_OK(rtk_launch_detile(tileBuf, ids, (uint32_t)tiles, d.width, d.height, root->tilesX, C.planes, C.planes + P, C.planes + 2 * P, 0, root->stream));
            HIP_OK(hipStreamSynchronize(root->stream));
            HIP_OK(hipMemcpy(outputRed, C.planes, P * sizeof(uint16_t), hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(outputGreen, C.planes + P, P * sizeof(uint16_t), hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(outputBlue, C.planes + 2 * P, P * sizeof(uint16_t), hipMemcpyDeviceToHost));
            return 0;
        };
        ok = gather() == 0;
    }
    if (ok) {
        for (int i = 0; i < 5; ++i) C.hash[i] = h[i];
        C.sampleCount = d.sampleCount;
        C.valid = true;
        g_progress.store(0.999f, std::memory_order_relaxed); // capped like raytrace.c:580; the caller sets 1.0 (render.cpp:1397)
    }
    if (timing) {
        const auto tEnd = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "libraytrace_hip: RaytraceAll: %s; hashing %.1f ms, build/update + render %.1f ms, gather + copy out %.1f ms\n",
                reuse ? (cameraChanged || lightsChanged || samplesChanged || gridChanged || materialsChanged ? "scene reused, parts rebuilt" : "scene reused as it is") : "scene built",
                ms(tCall, tHash), ms(tHash, tRender), ms(tRender, tEnd));
    }
    if (!ok || !useCache) {
        const std::string keep = g_error;
        C.clear();
        g_error = keep;
    }
    g_endTime.store((long)clock(), std::memory_order_relaxed);
    if (!ok) fprintf(stderr, "libraytrace_hip: RaytraceAll failed: %s\n", g_error.c_str());
    return ok ? CL_TRUE : CL_FALSE;
}

} // extern "C"

