// rt_filters.cpp -- the image-space filters of libraytrace_hip.so (include/raytrace_hip.h: "DENOISER", "TEMPORAL ACCUMULATION",
// "VARIANCE-GUIDED FILTER", "TEMPORAL CLAMP", "MOTION BLUR", "DEPTH OF FIELD"): parameter checks, the device and host entry points, and the resident scene's calls with their buffers.
// The kernels are in rt_denoise.hip, rt_temporal.hip, rt_variance.hip, rt_motion_blur.hip and rt_dof.hip; the scene and what else the host side shares, in rt_host.h.
#include "rt_host.h"
#include "rt_launch.h"
#include "rt_overlap.h"

#include <cmath>

using namespace rthost;

// ---- what the filters share ------------------------------------------------------------------------------------------------------
// The arrays of a device entry point, in the order its refusals name them: no written array overlaps another, `stream` (or the null
// stream) is one of `device`, which becomes the current device, and every array that was given is memory of it (query_pointer_ok).
// The caller has refused null arrays it needs and a scratch that is too small.
static int checked_device_arrays(const char *who, int device, void *stream, const RtArray *arr, int n)
{
    int i = 0, k = 0;
    if (rt_first_overlap(arr, n, &i, &k)) return fail("%s: %s overlaps %s", who, arr[k].what, arr[i].what);
    HIP_OK(hipSetDevice(device));
    if (stream) { // (the null stream is the current device's, set above)
        hipDevice_t sd = -1;
        if (hipStreamGetDevice((hipStream_t)stream, &sd) != hipSuccess) { (void)hipGetLastError(); return fail("%s: stream %p is not a stream", who, stream); }
        if (sd != device) return fail("%s: stream %p belongs to device %d, the call is for device %d", who, stream, (int)sd, device);
    }
    for (i = 0; i < n; ++i)
        if (arr[i].p && query_pointer_ok(device, "the call", arr[i].p, arr[i].bytes, arr[i].align, arr[i].what) != 0) return -1;
    return 0;
}

// The device side of a host entry point's arrays, freed when the scope ends: up() gives a device copy of a host array (null for a null
// one), out() a device array to copy back from.  After a failure both give null and `status` says what failed.
struct HostStage {
    DevPart mem;
    hipError_t status = hipSuccess;
    int failed() const { return fail("device staging failed: %s", hipGetErrorString(status)); }
    template <class T> T *out(size_t bytes)
    {
        void *d = nullptr;
        if (status == hipSuccess) status = mem.get(&d, bytes);
        return status == hipSuccess ? (T *)d : nullptr;
    }
    template <class T> T *up(const T *host, size_t bytes)
    {
        T *d = host ? out<T>(bytes) : nullptr;
        if (d) status = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        return status == hipSuccess ? d : nullptr;
    }
};

// u16 output planes: all three or none
struct Planes { uint16_t *r = nullptr, *g = nullptr, *b = nullptr; };

// `who` needs every tile of the image once in the instance's tile set (it works on the whole row-major image).
static int whole_image_tiles(const rtHipScene *sc, const char *who)
{
    const uint32_t tiles = sc->tilesX * ((sc->height + RT_TILE - 1) / RT_TILE);
    std::vector<char> seen(tiles, 0);
    for (cl_uint t : sc->tileIds)
        if (t >= tiles || seen[t]++) return fail("%s needs a tile set that holds every tile of the image once (tile %u)", who, t);
    if (sc->tileIds.size() != tiles) return fail("%s needs a tile set that holds every tile of the image (%zu of %u)", who, sc->tileIds.size(), tiles);
    return 0;
}

// The end of a scene call, after its synchronisation: the image of n pixels and the planes, each where the caller asked for it.
static int scene_outputs_to_host(size_t n, const float *rgb, const Planes &planes, cl_float *outRgb, cl_ushort *outR, cl_ushort *outG, cl_ushort *outB)
{
    if (outRgb) HIP_OK(hipMemcpy(outRgb, rgb, n * 12, hipMemcpyDeviceToHost));
    if (outR) HIP_OK(hipMemcpy(outR, planes.r, n * 2, hipMemcpyDeviceToHost));
    if (outG) HIP_OK(hipMemcpy(outG, planes.g, n * 2, hipMemcpyDeviceToHost));
    if (outB) HIP_OK(hipMemcpy(outB, planes.b, n * 2, hipMemcpyDeviceToHost));
    return 0;
}

// ---- denoiser (include/raytrace_hip.h, "DENOISER"; kernels in rt_denoise.hip) ------------------------------------------------
// Filter scratch of a W x H image: C^i and C^(i+1) as float4 (ping-pong), then the guides G0 = (n^, z) and G1 = (albedo, 0) as float4.
#define RT_DENOISE_MAX_PIXELS (1ull << 27)
#define RT_DENOISE_SCRATCH_PER_PIXEL 64ull

void rtHipDenoiseDefaults(rtHipDenoiseParams *p)
{
    if (!p) return;
    p->iterations = 4;
    p->colourInvSigma2 = 4.0f;
    p->albedoInvSigma2 = 100.0f;
    p->normalPowerLog2 = 7;
}

static int denoise_params_ok(const rtHipDenoiseParams *p)
{
    if (!p) return fail("denoise: null parameters");
    if (p->iterations > 12) return fail("denoise: iterations %u is not in 0..12", p->iterations);
    if (!(std::isfinite(p->colourInvSigma2) && p->colourInvSigma2 >= 0.f))
        return fail("denoise: colourInvSigma2 %g is not finite and >= 0", (double)p->colourInvSigma2);
    if (!(std::isfinite(p->albedoInvSigma2) && p->albedoInvSigma2 >= 0.f))
        return fail("denoise: albedoInvSigma2 %g is not finite and >= 0", (double)p->albedoInvSigma2);
    if (p->normalPowerLog2 > 10) return fail("denoise: normalPowerLog2 %u is not in 0..10", p->normalPowerLog2);
    float ic = p->colourInvSigma2; // what the last iteration uses: ic multiplied by 4.0f K-1 times in fp32
    for (uint32_t i = 1; i < p->iterations; ++i) ic = ic * 4.0f;
    if (!std::isfinite(ic)) return fail("denoise: colourInvSigma2 * 4^(iterations-1) overflows fp32");
    return 0;
}

static int denoise_size_ok(uint32_t W, uint32_t H)
{
    if (W == 0 || H == 0 || (uint64_t)W * H > RT_DENOISE_MAX_PIXELS) return fail("denoise: a %u x %u image is not 1..2^27 pixels", W, H);
    return 0;
}

uint64_t rtHipDenoiseScratchBytes(cl_uint width, cl_uint height)
{
    if (width == 0 || height == 0 || (uint64_t)width * height > RT_DENOISE_MAX_PIXELS) return 0;
    return (uint64_t)width * height * RT_DENOISE_SCRATCH_PER_PIXEL;
}

// Issues the filter on `st`: guides, K iterations, output, and `afterGuides` (if any) between the guides and the first iteration.
// Arguments were checked by the caller.
static int denoise_issue(uint32_t W, uint32_t H, const float *colour, const float *normal, const float *albedo, float *out, Planes planes,
                         char *scratch, const rtHipDenoiseParams *p, hipStream_t st, hipEvent_t afterGuides = nullptr)
{
    const size_t n = (size_t)W * H;
    char *c[2] = { scratch, scratch + 16 * n };
    char *g0 = scratch + 32 * n, *g1 = scratch + 48 * n;
    HIP_OK(rtd_launch_guides((uint32_t)n, colour, normal, albedo, c[0], g0, g1, st));
    if (afterGuides) HIP_OK(hipEventRecord(afterGuides, st));
    float ic = p->colourInvSigma2;
    for (uint32_t i = 0; i < p->iterations; ++i) {
        HIP_OK(rtd_launch_iteration(W, H, 1 << i, ic, p->albedoInvSigma2, p->normalPowerLog2, c[i & 1], g0, g1, c[(i + 1) & 1], st));
        ic = ic * 4.0f;
    }
    HIP_OK(rtd_launch_output((uint32_t)n, c[p->iterations & 1], out, planes.r, planes.g, planes.b, st));
    return 0;
}

int rtHipDenoiseDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *normal, const void *albedo, void *out,
                       void *scratch, uint64_t scratchBytes, const rtHipDenoiseParams *params, void *stream)
{
    if (denoise_params_ok(params) != 0 || denoise_size_ok(width, height) != 0) return -1;
    if (!colour || !normal || !albedo || !out || !scratch) return fail("denoise: null array");
    const uint64_t img = (uint64_t)width * height * 12, need = rtHipDenoiseScratchBytes(width, height);
    if (scratchBytes < need) return fail("denoise: scratch of %llu bytes, %llu needed", (unsigned long long)scratchBytes, (unsigned long long)need);
    const RtArray arr[5] = { { colour, img, 4, "colour" }, { normal, img, 4, "normal" }, { albedo, img, 4, "albedo" },
                             { out, img, 4, "out", true }, { scratch, need, 16, "scratch", true } };
    if (checked_device_arrays("denoise", device, stream, arr, 5) != 0) return -1;
    return denoise_issue(width, height, (const float *)colour, (const float *)normal, (const float *)albedo, (float *)out, Planes{},
                         (char *)scratch, params, (hipStream_t)stream);
}

int rtHipDenoise(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *normal, const cl_float *albedo,
                 cl_float *out, const rtHipDenoiseParams *params)
{
    if (denoise_params_ok(params) != 0 || denoise_size_ok(width, height) != 0) return -1;
    if (!colour || !normal || !albedo || !out) return fail("denoise: null array");
    HIP_OK(hipSetDevice(device));
    const size_t img = (size_t)width * height * 12;
    HostStage dev;
    const float *c = dev.up(colour, img), *n = dev.up(normal, img), *a = dev.up(albedo, img);
    float *dout = dev.out<float>(img);
    char *scratch = dev.out<char>(rtHipDenoiseScratchBytes(width, height));
    if (dev.status != hipSuccess) return dev.failed();
    if (denoise_issue(width, height, c, n, a, dout, Planes{}, scratch, params, nullptr) != 0) return -1;
    HIP_OK(hipMemcpy(out, dout, img, hipMemcpyDeviceToHost));
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

// The scene's denoiser scratch, made on first use: [colour | normal | albedo | out] W x H x 3 f32, [R | G | B] u16, filter scratch; every
// part 256-byte aligned.
struct DenoiseBuffer {
    size_t n;
    float *colour, *normal, *albedo, *out;
    Planes planes;
    char *scratch;
};
static int denoise_buffer(rtHipScene *sc, DenoiseBuffer &D)
{
    const uint32_t W = sc->width, H = sc->height;
    const size_t n = (size_t)W * H, img = (n * 12 + 255) & ~(size_t)255, plane = (n * 2 + 255) & ~(size_t)255;
    const uint64_t bytes = 4 * img + 3 * plane + rtHipDenoiseScratchBytes(W, H);
    if (!sc->denoiseBuf) HIP_OK(sc->denoiseBuf.make(bytes, sc->bytes));
    char *b = sc->denoiseBuf;
    D.n = n;
    D.colour = (float *)b; D.normal = (float *)(b + img); D.albedo = (float *)(b + 2 * img); D.out = (float *)(b + 3 * img);
    D.planes = { (uint16_t *)(b + 4 * img), (uint16_t *)(b + 4 * img + plane), (uint16_t *)(b + 4 * img + 2 * plane) };
    D.scratch = b + 4 * img + 3 * plane;
    return 0;
}

int rtHipSceneDenoise(rtHipScene *sc, const rtHipDenoiseParams *params, cl_float *outRgb, cl_ushort *outR, cl_ushort *outG, cl_ushort *outB)
{
    if (!sc) return fail("null scene");
    if (denoise_params_ok(params) != 0 || denoise_size_ok(sc->width, sc->height) != 0) return -1;
    if ((sc->passMask & RT_SURF_BUF_BITS) != RT_SURF_BUF_BITS)
        return fail("denoise needs the normal and the albedo pass on for this scene (rtHipScenePasses)");
    if (whole_image_tiles(sc, "denoise") != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipDeviceSynchronize());
    if (frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, nullptr) != 0) return -1;
    const uint32_t W = sc->width, H = sc->height;
    DenoiseBuffer D;
    if (denoise_buffer(sc, D) != 0) return -1;
    for (Event &e : sc->denoiseEv) HIP_OK(e.make());
    const bool wantPlanes = outR || outG || outB;
    hipStream_t st = sc->stream;
    Event *ev = sc->denoiseEv;
    HIP_OK(hipEventRecord(ev[0], st));
    HIP_OK(rtd_launch_gather(W, H, sc->tilesX, sc->dev.tileIds, (uint32_t)sc->tileIds.size(), sc->dev.tileBuf, sc->surfBuf,
                             (float)sc->dev.sampleCount, D.colour, D.normal, D.albedo, st));
    HIP_OK(hipEventRecord(ev[1], st));
    if (denoise_issue(W, H, D.colour, D.normal, D.albedo, outRgb ? D.out : nullptr, wantPlanes ? D.planes : Planes{}, D.scratch, params, st,
                      ev[2]) != 0)
        return -1;
    HIP_OK(hipEventRecord(ev[3], st));
    HIP_OK(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) HIP_OK(hipEventElapsedTime(&sc->denoiseMs[i], ev[i], ev[i + 1]));
    return scene_outputs_to_host(D.n, D.out, D.planes, outRgb, outR, outG, outB);
}

int rtHipSceneDenoiseTimes(const rtHipScene *sc, cl_float *ms)
{
    if (!sc || !ms) return fail("null argument");
    for (int i = 0; i < 3; ++i) ms[i] = sc->denoiseMs[i];
    return 0;
}

// ---- temporal accumulation (include/raytrace_hip.h, "TEMPORAL ACCUMULATION"; kernels in rt_temporal.hip) ---------------------------
#define RT_TEMPORAL_MAX_SIDE 16384u

void rtHipTemporalDefaults(rtHipTemporalParams *p)
{
    if (!p) return;
    p->maxHistory = 32.0f;
    p->depthTolerance = 0.05f;
}

static int temporal_params_ok(const rtHipTemporalParams *p)
{
    if (!p) return fail("temporal: null parameters");
    if (!(std::isfinite(p->maxHistory) && p->maxHistory >= 1.0f && p->maxHistory <= 65536.0f))
        return fail("temporal: maxHistory %g is not finite and in 1..65536", (double)p->maxHistory);
    if (!(std::isfinite(p->depthTolerance) && p->depthTolerance >= 0.f))
        return fail("temporal: depthTolerance %g is not finite and >= 0", (double)p->depthTolerance);
    return 0;
}

static int temporal_size_ok(uint32_t W, uint32_t H)
{
    if (W == 0 || H == 0 || W > RT_TEMPORAL_MAX_SIDE || H > RT_TEMPORAL_MAX_SIDE || (uint64_t)W * H > RT_DENOISE_MAX_PIXELS)
        return fail("temporal: a %u x %u image is not 1..16384 pixels wide and high and 1..2^27 pixels", W, H);
    return 0;
}

// ---- temporal clamp (include/raytrace_hip.h, "TEMPORAL CLAMP"; rtt_clamp_kernel in rt_temporal.hip) ------------------------------
void rtHipTemporalClampDefaults(rtHipTemporalClampParams *p)
{
    if (!p) return;
    p->mode = RT_HIP_CLAMP_MINMAX | RT_HIP_CLAMP_VARIANCE;
    p->gamma = 1.0f;
}

int rtHipTemporalClampCheck(const rtHipTemporalClampParams *p)
{
    if (!p) return fail("temporal clamp: null parameters");
    if (p->mode < 1 || p->mode > 3) return fail("temporal clamp: mode %u is not 1 (min/max), 2 (variance) or 3 (both)", p->mode);
    if (!(std::isfinite(p->gamma) && p->gamma >= 0.f)) return fail("temporal clamp: gamma %g is not finite and >= 0", (double)p->gamma);
    return 0;
}

// The accumulation on checked device arrays: with `clamp` (checked) the clamped kernel, with or without moments; without, the kernel
// each call has always issued.
static int accumulate_issue(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *prevT, const uint32_t *triangle,
                            const float *histColour, const float *histCount, const float *histT, const uint32_t *histTriangle,
                            const float *histMoments, float *outColour, float *outCount, float *outMoments, float *outVariance,
                            const rtHipTemporalParams *p, const rtHipTemporalClampParams *clamp, hipStream_t st)
{
    if (clamp)
        HIP_OK(rtt_launch_accumulate_clamp(W, H, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, histMoments,
                                           outColour, outCount, outMoments, outVariance, p->maxHistory, p->depthTolerance, clamp->mode,
                                           clamp->gamma, st));
    else if (histMoments)
        HIP_OK(rtv_launch_moments(W, H, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, histMoments, outColour,
                                  outCount, outMoments, outVariance, p->maxHistory, p->depthTolerance, st));
    else
        HIP_OK(rtt_launch_accumulate(W, H, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, outColour, outCount,
                                     p->maxHistory, p->depthTolerance, st));
    return 0;
}

// rtHipTemporalDevice (clamp null) and rtHipTemporalClampDevice (clamp checked by the caller)
static int temporal_device(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *prevT,
                           const void *triangle, const void *histColour, const void *histCount, const void *histT, const void *histTriangle,
                           void *outColour, void *outCount, const rtHipTemporalParams *params, const rtHipTemporalClampParams *clamp,
                           void *stream)
{
    if (temporal_params_ok(params) != 0 || temporal_size_ok(width, height) != 0) return -1;
    if (!colour || !motion || !prevT || !triangle || !histColour || !histCount || !histT || !histTriangle || !outColour)
        return fail("temporal: null array");
    const uint64_t n = (uint64_t)width * height;
    const RtArray arr[10] = {
        { colour, n * 12, 4, "colour" }, { motion, n * 8, 4, "motion" }, { prevT, n * 4, 4, "prevT" }, { triangle, n * 4, 4, "triangle" },
        { histColour, n * 12, 4, "histColour" }, { histCount, n * 4, 4, "histCount" }, { histT, n * 4, 4, "histT" },
        { histTriangle, n * 4, 4, "histTriangle" }, { outColour, n * 12, 4, "outColour", true }, { outCount, n * 4, 4, "outCount", true } };
    if (checked_device_arrays("temporal", device, stream, arr, 10) != 0) return -1;
    return accumulate_issue(width, height, (const float *)colour, (const float *)motion, (const float *)prevT, (const uint32_t *)triangle,
                            (const float *)histColour, (const float *)histCount, (const float *)histT, (const uint32_t *)histTriangle, nullptr,
                            (float *)outColour, (float *)outCount, nullptr, nullptr, params, clamp, (hipStream_t)stream);
}

int rtHipTemporalDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *prevT,
                        const void *triangle, const void *histColour, const void *histCount, const void *histT, const void *histTriangle,
                        void *outColour, void *outCount, const rtHipTemporalParams *params, void *stream)
{
    return temporal_device(device, width, height, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, outColour,
                           outCount, params, nullptr, stream);
}

int rtHipTemporalClampDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *prevT,
                             const void *triangle, const void *histColour, const void *histCount, const void *histT,
                             const void *histTriangle, void *outColour, void *outCount, const rtHipTemporalParams *params,
                             const rtHipTemporalClampParams *clamp, void *stream)
{
    if (rtHipTemporalClampCheck(clamp) != 0) return -1;
    return temporal_device(device, width, height, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, outColour,
                           outCount, params, clamp, stream);
}

// rtHipTemporal (clamp null) and rtHipTemporalClamp (clamp checked by the caller)
static int temporal_host(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *prevT,
                         const cl_uint *triangle, const cl_float *histColour, const cl_float *histCount, const cl_float *histT,
                         const cl_uint *histTriangle, cl_float *outColour, cl_float *outCount, const rtHipTemporalParams *params,
                         const rtHipTemporalClampParams *clamp)
{
    if (temporal_params_ok(params) != 0 || temporal_size_ok(width, height) != 0) return -1;
    if (!colour || !motion || !prevT || !triangle || !histColour || !histCount || !histT || !histTriangle || !outColour)
        return fail("temporal: null array");
    HIP_OK(hipSetDevice(device));
    const size_t n = (size_t)width * height;
    HostStage dev;
    const float *c = dev.up(colour, n * 12), *m = dev.up(motion, n * 8), *pt = dev.up(prevT, n * 4);
    const cl_uint *tri = dev.up(triangle, n * 4);
    const float *hc = dev.up(histColour, n * 12), *hn = dev.up(histCount, n * 4), *ht = dev.up(histT, n * 4);
    const cl_uint *htri = dev.up(histTriangle, n * 4);
    float *dColour = dev.out<float>(n * 12), *dCount = outCount ? dev.out<float>(n * 4) : nullptr;
    if (dev.status != hipSuccess) return dev.failed();
    if (accumulate_issue(width, height, c, m, pt, tri, hc, hn, ht, htri, nullptr, dColour, dCount, nullptr, nullptr, params, clamp, nullptr) != 0)
        return -1;
    HIP_OK(hipMemcpy(outColour, dColour, n * 12, hipMemcpyDeviceToHost));
    if (outCount) HIP_OK(hipMemcpy(outCount, dCount, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

int rtHipTemporal(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *prevT,
                  const cl_uint *triangle, const cl_float *histColour, const cl_float *histCount, const cl_float *histT,
                  const cl_uint *histTriangle, cl_float *outColour, cl_float *outCount, const rtHipTemporalParams *params)
{
    return temporal_host(device, width, height, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, outColour, outCount,
                         params, nullptr);
}

int rtHipTemporalClamp(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *prevT,
                       const cl_uint *triangle, const cl_float *histColour, const cl_float *histCount, const cl_float *histT,
                       const cl_uint *histTriangle, cl_float *outColour, cl_float *outCount, const rtHipTemporalParams *params,
                       const rtHipTemporalClampParams *clamp)
{
    if (rtHipTemporalClampCheck(clamp) != 0) return -1;
    return temporal_host(device, width, height, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, outColour, outCount,
                         params, clamp);
}

// ---- variance-guided filter (include/raytrace_hip.h, "VARIANCE-GUIDED FILTER"; kernels in rt_variance.hip) ------------------------
// Filter scratch of a W x H image: the states S^i and S^(i+1) = (C.rgb, V) as float4 (ping-pong), the guides G0 and G1 as float4 (the
// denoiser's 64 B per pixel), then il as f32.
#define RT_VARIANCE_SCRATCH_PER_PIXEL 68ull

void rtHipVarianceDefaults(rtHipVarianceParams *p)
{
    if (!p) return;
    p->iterations = 4;
    p->luminanceSigma2 = 4.0f;
    p->varianceFloor = 1e-8f;
    p->albedoInvSigma2 = 100.0f;
    p->normalPowerLog2 = 7;
    p->spatialBelow = 4.0f;
}

static int variance_params_ok(const rtHipVarianceParams *p)
{
    if (!p) return fail("variance: null parameters");
    if (p->iterations > 12) return fail("variance: iterations %u is not in 0..12", p->iterations);
    if (!(std::isfinite(p->luminanceSigma2) && p->luminanceSigma2 >= 0.f))
        return fail("variance: luminanceSigma2 %g is not finite and >= 0", (double)p->luminanceSigma2);
    if (!(std::isfinite(p->varianceFloor) && p->varianceFloor >= 0x1p-100f))
        return fail("variance: varianceFloor %g is not finite and >= 2^-100", (double)p->varianceFloor);
    if (!(std::isfinite(p->albedoInvSigma2) && p->albedoInvSigma2 >= 0.f))
        return fail("variance: albedoInvSigma2 %g is not finite and >= 0", (double)p->albedoInvSigma2);
    if (p->normalPowerLog2 > 10) return fail("variance: normalPowerLog2 %u is not in 0..10", p->normalPowerLog2);
    if (!(std::isfinite(p->spatialBelow) && p->spatialBelow >= 0.f && p->spatialBelow <= 65537.0f))
        return fail("variance: spatialBelow %g is not finite and in 0..65537", (double)p->spatialBelow);
    return 0;
}

uint64_t rtHipVarianceScratchBytes(cl_uint width, cl_uint height)
{
    if (width == 0 || height == 0 || (uint64_t)width * height > RT_DENOISE_MAX_PIXELS) return 0;
    return (uint64_t)width * height * RT_VARIANCE_SCRATCH_PER_PIXEL;
}

// Issues the filter on `st`: guides and estimate, K iterations, output.  scratch: the first 64 B per pixel of the layout above; il: n f32.
// Arguments were checked by the caller.
static int variance_issue(uint32_t W, uint32_t H, const float *colour, const float *normal, const float *albedo, const float *moments,
                          const float *count, float *out, float *outVariance, Planes planes, char *scratch, char *il,
                          const rtHipVarianceParams *p, hipStream_t st)
{
    const size_t n = (size_t)W * H;
    char *s[2] = { scratch, scratch + 16 * n };
    char *g0 = scratch + 32 * n, *g1 = scratch + 48 * n;
    HIP_OK(rtv_launch_estimate(W, H, colour, normal, albedo, moments, count, p->spatialBelow, p->albedoInvSigma2, p->normalPowerLog2, s[0], g0,
                               g1, st));
    for (uint32_t i = 0; i < p->iterations; ++i)
        HIP_OK(rtv_launch_iteration(W, H, 1 << i, p->luminanceSigma2, p->varianceFloor, p->albedoInvSigma2, p->normalPowerLog2, s[i & 1], il,
                                    g0, g1, s[(i + 1) & 1], st));
    HIP_OK(rtv_launch_output((uint32_t)n, s[p->iterations & 1], out, outVariance, planes.r, planes.g, planes.b, st));
    return 0;
}

int rtHipDenoiseVarianceDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *normal, const void *albedo,
                               const void *moments, const void *count, void *out, void *outVariance, void *scratch, uint64_t scratchBytes,
                               const rtHipVarianceParams *params, void *stream)
{
    if (variance_params_ok(params) != 0 || denoise_size_ok(width, height) != 0) return -1;
    if (!colour || !normal || !albedo || !out || !scratch) return fail("variance: null array");
    if ((moments == nullptr) != (count == nullptr)) return fail("variance: moments and count are both NULL or both given");
    const uint64_t n = (uint64_t)width * height, img = n * 12, need = rtHipVarianceScratchBytes(width, height);
    if (scratchBytes < need) return fail("variance: scratch of %llu bytes, %llu needed", (unsigned long long)scratchBytes, (unsigned long long)need);
    const RtArray arr[8] = { { colour, img, 4, "colour" }, { normal, img, 4, "normal" }, { albedo, img, 4, "albedo" },
                             { moments, n * 8, 4, "moments" }, { count, n * 4, 4, "count" }, { out, img, 4, "out", true },
                             { scratch, need, 16, "scratch", true }, { outVariance, n * 4, 4, "outVariance", true } };
    if (checked_device_arrays("variance", device, stream, arr, 8) != 0) return -1;
    return variance_issue(width, height, (const float *)colour, (const float *)normal, (const float *)albedo, (const float *)moments,
                          (const float *)count, (float *)out, (float *)outVariance, Planes{}, (char *)scratch, (char *)scratch + 64 * n, params,
                          (hipStream_t)stream);
}

int rtHipDenoiseVariance(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *normal, const cl_float *albedo,
                         const cl_float *moments, const cl_float *count, cl_float *out, cl_float *outVariance, const rtHipVarianceParams *params)
{
    if (variance_params_ok(params) != 0 || denoise_size_ok(width, height) != 0) return -1;
    if (!colour || !normal || !albedo || !out) return fail("variance: null array");
    if ((moments == nullptr) != (count == nullptr)) return fail("variance: moments and count are both NULL or both given");
    HIP_OK(hipSetDevice(device));
    const size_t n = (size_t)width * height, img = n * 12;
    HostStage dev;
    const float *c = dev.up(colour, img), *nrm = dev.up(normal, img), *a = dev.up(albedo, img);
    const float *m = dev.up(moments, n * 8), *cnt = dev.up(count, n * 4);
    float *dout = dev.out<float>(img), *dvar = dev.out<float>(n * 4);
    char *scratch = dev.out<char>(rtHipVarianceScratchBytes(width, height));
    if (dev.status != hipSuccess) return dev.failed();
    if (variance_issue(width, height, c, nrm, a, m, cnt, dout, dvar, Planes{}, scratch, scratch + 64 * n, params, nullptr) != 0) return -1;
    HIP_OK(hipMemcpy(out, dout, img, hipMemcpyDeviceToHost));
    if (outVariance) HIP_OK(hipMemcpy(outVariance, dvar, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

// rtHipTemporalMomentsDevice (clamp null) and rtHipTemporalMomentsClampDevice (clamp checked by the caller)
static int moments_device(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *prevT,
                          const void *triangle, const void *histColour, const void *histCount, const void *histT, const void *histTriangle,
                          const void *histMoments, void *outColour, void *outCount, void *outMoments, void *outVariance,
                          const rtHipTemporalParams *params, const rtHipTemporalClampParams *clamp, void *stream)
{
    if (temporal_params_ok(params) != 0 || temporal_size_ok(width, height) != 0) return -1;
    if (!colour || !motion || !prevT || !triangle || !histColour || !histCount || !histT || !histTriangle || !histMoments || !outColour ||
        !outMoments)
        return fail("temporal: null array");
    const uint64_t n = (uint64_t)width * height;
    const RtArray arr[13] = {
        { colour, n * 12, 4, "colour" }, { motion, n * 8, 4, "motion" }, { prevT, n * 4, 4, "prevT" }, { triangle, n * 4, 4, "triangle" },
        { histColour, n * 12, 4, "histColour" }, { histCount, n * 4, 4, "histCount" }, { histT, n * 4, 4, "histT" },
        { histTriangle, n * 4, 4, "histTriangle" }, { histMoments, n * 8, 4, "histMoments" }, { outColour, n * 12, 4, "outColour", true },
        { outMoments, n * 8, 4, "outMoments", true }, { outCount, n * 4, 4, "outCount", true }, { outVariance, n * 4, 4, "outVariance", true } };
    if (checked_device_arrays("temporal", device, stream, arr, 13) != 0) return -1;
    return accumulate_issue(width, height, (const float *)colour, (const float *)motion, (const float *)prevT, (const uint32_t *)triangle,
                            (const float *)histColour, (const float *)histCount, (const float *)histT, (const uint32_t *)histTriangle,
                            (const float *)histMoments, (float *)outColour, (float *)outCount, (float *)outMoments, (float *)outVariance, params,
                            clamp, (hipStream_t)stream);
}

int rtHipTemporalMomentsDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *prevT,
                               const void *triangle, const void *histColour, const void *histCount, const void *histT, const void *histTriangle,
                               const void *histMoments, void *outColour, void *outCount, void *outMoments, void *outVariance,
                               const rtHipTemporalParams *params, void *stream)
{
    return moments_device(device, width, height, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, histMoments,
                          outColour, outCount, outMoments, outVariance, params, nullptr, stream);
}

int rtHipTemporalMomentsClampDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *prevT,
                                    const void *triangle, const void *histColour, const void *histCount, const void *histT,
                                    const void *histTriangle, const void *histMoments, void *outColour, void *outCount, void *outMoments,
                                    void *outVariance, const rtHipTemporalParams *params, const rtHipTemporalClampParams *clamp, void *stream)
{
    if (rtHipTemporalClampCheck(clamp) != 0) return -1;
    return moments_device(device, width, height, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, histMoments,
                          outColour, outCount, outMoments, outVariance, params, clamp, stream);
}

// rtHipTemporalMoments (clamp null) and rtHipTemporalMomentsClamp (clamp checked by the caller)
static int moments_host(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *prevT,
                        const cl_uint *triangle, const cl_float *histColour, const cl_float *histCount, const cl_float *histT,
                        const cl_uint *histTriangle, const cl_float *histMoments, cl_float *outColour, cl_float *outCount, cl_float *outMoments,
                        cl_float *outVariance, const rtHipTemporalParams *params, const rtHipTemporalClampParams *clamp)
{
    if (temporal_params_ok(params) != 0 || temporal_size_ok(width, height) != 0) return -1;
    if (!colour || !motion || !prevT || !triangle || !histColour || !histCount || !histT || !histTriangle || !histMoments || !outColour ||
        !outMoments)
        return fail("temporal: null array");
    HIP_OK(hipSetDevice(device));
    const size_t n = (size_t)width * height;
    HostStage dev;
    const float *c = dev.up(colour, n * 12), *m = dev.up(motion, n * 8), *pt = dev.up(prevT, n * 4);
    const cl_uint *tri = dev.up(triangle, n * 4);
    const float *hc = dev.up(histColour, n * 12), *hn = dev.up(histCount, n * 4), *ht = dev.up(histT, n * 4);
    const cl_uint *htri = dev.up(histTriangle, n * 4);
    const float *hm = dev.up(histMoments, n * 8);
    float *dColour = dev.out<float>(n * 12), *dMoments = dev.out<float>(n * 8);
    float *dCount = outCount ? dev.out<float>(n * 4) : nullptr, *dVariance = outVariance ? dev.out<float>(n * 4) : nullptr;
    if (dev.status != hipSuccess) return dev.failed();
    if (accumulate_issue(width, height, c, m, pt, tri, hc, hn, ht, htri, hm, dColour, dCount, dMoments, dVariance, params, clamp, nullptr) != 0)
        return -1;
    HIP_OK(hipMemcpy(outColour, dColour, n * 12, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(outMoments, dMoments, n * 8, hipMemcpyDeviceToHost));
    if (outCount) HIP_OK(hipMemcpy(outCount, dCount, n * 4, hipMemcpyDeviceToHost));
    if (outVariance) HIP_OK(hipMemcpy(outVariance, dVariance, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

int rtHipTemporalMoments(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *prevT,
                         const cl_uint *triangle, const cl_float *histColour, const cl_float *histCount, const cl_float *histT,
                         const cl_uint *histTriangle, const cl_float *histMoments, cl_float *outColour, cl_float *outCount, cl_float *outMoments,
                         cl_float *outVariance, const rtHipTemporalParams *params)
{
    return moments_host(device, width, height, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, histMoments,
                        outColour, outCount, outMoments, outVariance, params, nullptr);
}

int rtHipTemporalMomentsClamp(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *prevT,
                              const cl_uint *triangle, const cl_float *histColour, const cl_float *histCount, const cl_float *histT,
                              const cl_uint *histTriangle, const cl_float *histMoments, cl_float *outColour, cl_float *outCount,
                              cl_float *outMoments, cl_float *outVariance, const rtHipTemporalParams *params,
                              const rtHipTemporalClampParams *clamp)
{
    if (rtHipTemporalClampCheck(clamp) != 0) return -1;
    return moments_host(device, width, height, colour, motion, prevT, triangle, histColour, histCount, histT, histTriangle, histMoments,
                        outColour, outCount, outMoments, outVariance, params, clamp);
}

// ---- the resident scene's temporal calls -------------------------------------------------------------------------------------------
// rtHipSceneTemporal (withMoments false: `denoise` or no filter) and rtHipSceneTemporalVariance (withMoments true: `variance` or no filter)
// are one sequence; the second carries the moments along and has a variance to output.
static int scene_temporal(rtHipScene *sc, const rtHipTemporalParams *params, const rtHipDenoiseParams *denoise, bool withMoments,
                          const rtHipVarianceParams *variance, cl_float *outRgb, cl_ushort *outR, cl_ushort *outG, cl_ushort *outB,
                          cl_float *outCount, cl_float *outVariance)
{
    if (!sc) return fail("temporal: null scene");
    if (temporal_params_ok(params) != 0 || temporal_size_ok(sc->width, sc->height) != 0) return -1;
    if (denoise) {
        if (denoise_params_ok(denoise) != 0) return -1;
        if ((sc->passMask & RT_SURF_BUF_BITS) != RT_SURF_BUF_BITS)
            return fail("temporal: denoise needs the normal and the albedo pass on for this scene (rtHipScenePasses)");
    }
    if (variance) {
        if (variance_params_ok(variance) != 0) return -1;
        if ((sc->passMask & RT_SURF_BUF_BITS) != RT_SURF_BUF_BITS)
            return fail("temporal: the variance-guided filter needs the normal and the albedo pass on for this scene (rtHipScenePasses)");
    }
    if (whole_image_tiles(sc, "temporal accumulation") != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipDeviceSynchronize());
    if (frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, nullptr) != 0) return -1;
    if (!sc->motion.have && rtHipSceneMotionMark(sc) != 0) return -1;
    if (sc->dev.triangleCount != sc->motion.triangles)
        return fail("temporal: the scene has %u triangles, the motion reference was made for %u", sc->dev.triangleCount, sc->motion.triangles);
    rtHipScene::Temporal &T = sc->temporal;
    const uint32_t W = sc->width, H = sc->height;
    const size_t n = (size_t)W * H;
    const auto part = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t set = part(n * 12) + 3 * part(n * 4); // a history set: colour | count | t | triangle
    if (!T.buf) {
        const uint64_t bytes = 2 * set + part(n * 8) + part(n * 4) + part(n * 12) + 3 * part(n * 2);
        if (scene_block(sc, T.buf, bytes, "temporal") != 0) return -1;
        T.cur = 0; T.valid = false;
    }
    if (withMoments && !T.momentsBuf) { // two sets of moments | the variance | the filter's il
        const uint64_t bytes = 2 * part(n * 8) + 2 * part(n * 4);
        if (scene_block(sc, T.momentsBuf, bytes, "temporal") != 0) return -1;
        T.momentsValid = false;
    }
    if (withMoments && !T.momentsValid) T.valid = false; // a live history whose moments are stale starts again, as after a reset
    for (Event &e : T.ev) HIP_OK(e.make());
    struct Set { float *colour, *count, *t; uint32_t *triangle; } hs[2];
    for (int i = 0; i < 2; ++i) {
        char *b = T.buf + i * set;
        hs[i].colour = (float *)b; hs[i].count = (float *)(b + part(n * 12)); hs[i].t = (float *)(b + part(n * 12) + part(n * 4));
        hs[i].triangle = (uint32_t *)(b + part(n * 12) + 2 * part(n * 4));
    }
    char *rest = T.buf + 2 * set;
    float *motion = (float *)rest, *prevT = (float *)(rest + part(n * 8)), *colour = (float *)(rest + part(n * 8) + part(n * 4));
    char *plane = rest + part(n * 8) + part(n * 4) + part(n * 12);
    const Planes planes = { (uint16_t *)plane, (uint16_t *)(plane + part(n * 2)), (uint16_t *)(plane + 2 * part(n * 2)) };
    const Set &hist = hs[T.cur], &next = hs[T.cur ^ 1];
    float *moments[2] = {}, *varianceOut = nullptr;
    char *il = nullptr;
    if (withMoments) {
        moments[0] = T.momentsBuf.as<float>(); moments[1] = (float *)(T.momentsBuf + part(n * 8));
        varianceOut = (float *)(T.momentsBuf + 2 * part(n * 8));
        il = T.momentsBuf + 2 * part(n * 8) + part(n * 4);
    }
    const bool surfaces = denoise || variance; // the filters take the gathered normal and albedo
    DenoiseBuffer D{};
    if (surfaces && denoise_buffer(sc, D) != 0) return -1;
    hipStream_t st = sc->stream;
    if (!T.valid) HIP_OK(hipMemsetAsync(hist.count, 0, n * 4, st)); // no history: every tap is refused, whatever the rest of the set holds
    HIP_OK(hipEventRecord(T.ev[0], st));
    if (motion_run(sc, motion, next.t, prevT, next.triangle, true, st) != 0) return -1; // this frame's guides are the next call's history
    HIP_OK(hipEventRecord(T.ev[1], st));
    if (surfaces) {
        HIP_OK(rtd_launch_gather(W, H, sc->tilesX, sc->dev.tileIds, (uint32_t)sc->tileIds.size(), sc->dev.tileBuf, sc->surfBuf,
                                 (float)sc->dev.sampleCount, D.colour, D.normal, D.albedo, st));
        colour = D.colour;
    } else {
        HIP_OK(rtt_launch_gather(W, H, sc->tilesX, sc->dev.tileIds, (uint32_t)sc->tileIds.size(), sc->dev.tileBuf, colour, st));
    }
    HIP_OK(hipEventRecord(T.ev[2], st));
    if (accumulate_issue(W, H, colour, motion, prevT, next.triangle, hist.colour, hist.count, hist.t, hist.triangle,
                         withMoments ? moments[T.cur] : nullptr, next.colour, next.count, withMoments ? moments[T.cur ^ 1] : nullptr,
                         withMoments && !variance ? varianceOut : nullptr, params, T.clampOn ? &T.clamp : nullptr, st) != 0)
        return -1;
    HIP_OK(hipEventRecord(T.ev[3], st));
    // From here until the new mark stands, a failure leaves the scene without history: set `next` is half a step ahead of the reference.
    T.valid = false;
    T.momentsValid = false;
    const bool wantPlanes = outR || outG || outB;
    const float *result = next.colour;
    Planes resultPlanes = planes;
    if (variance) { // temporal, then spatial with the moments' variance; the history keeps the unfiltered accumulation
        if (variance_issue(W, H, next.colour, D.normal, D.albedo, moments[T.cur ^ 1], next.count, outRgb ? D.out : nullptr, varianceOut,
                           wantPlanes ? D.planes : Planes{}, D.scratch, il, variance, st) != 0)
            return -1;
        result = D.out;
        resultPlanes = D.planes;
    } else if (denoise) { // temporal, then spatial; the history keeps the unfiltered accumulation
        if (denoise_issue(W, H, next.colour, D.normal, D.albedo, outRgb ? D.out : nullptr, wantPlanes ? D.planes : Planes{}, D.scratch, denoise,
                          st) != 0)
            return -1;
        result = D.out;
        resultPlanes = D.planes;
    } else if (wantPlanes) {
        HIP_OK(rtt_launch_quantise((uint32_t)n, next.colour, planes.r, planes.g, planes.b, st));
    }
    HIP_OK(hipEventRecord(T.ev[4], st));
    if (rtHipSceneMotionMark(sc) != 0) return -1; // the reference becomes the state this frame was rendered from
    HIP_OK(hipStreamSynchronize(st));
    T.cur ^= 1; // the sets change places only now: history and reference advance together
    T.valid = true;
    T.momentsValid = withMoments;
    for (int i = 0; i < 4; ++i) HIP_OK(hipEventElapsedTime(&T.ms[i], T.ev[i], T.ev[i + 1]));
    if (scene_outputs_to_host(n, result, resultPlanes, outRgb, outR, outG, outB) != 0) return -1;
    if (outCount) HIP_OK(hipMemcpy(outCount, next.count, n * 4, hipMemcpyDeviceToHost));
    if (outVariance) HIP_OK(hipMemcpy(outVariance, varianceOut, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int rtHipSceneTemporal(rtHipScene *sc, const rtHipTemporalParams *params, const rtHipDenoiseParams *denoise, cl_float *outRgb,
                       cl_ushort *outR, cl_ushort *outG, cl_ushort *outB, cl_float *outCount)
{
    return scene_temporal(sc, params, denoise, false, nullptr, outRgb, outR, outG, outB, outCount, nullptr);
}

int rtHipSceneTemporalVariance(rtHipScene *sc, const rtHipTemporalParams *params, const rtHipVarianceParams *variance, cl_float *outRgb,
                               cl_ushort *outR, cl_ushort *outG, cl_ushort *outB, cl_float *outCount, cl_float *outVariance)
{
    return scene_temporal(sc, params, nullptr, true, variance, outRgb, outR, outG, outB, outCount, outVariance);
}

int rtHipSceneTemporalReset(rtHipScene *sc)
{
    if (!sc) return fail("temporal: null scene");
    sc->temporal.valid = false;
    return 0;
}

int rtHipSceneSetTemporalClamp(rtHipScene *sc, const rtHipTemporalClampParams *clamp)
{
    if (!sc) return fail("temporal clamp: null scene");
    if (clamp && rtHipTemporalClampCheck(clamp) != 0) return -1;
    sc->temporal.clampOn = clamp != nullptr;
    sc->temporal.clamp = clamp ? *clamp : rtHipTemporalClampParams{};
    return 0;
}

int rtHipSceneGetTemporalClamp(const rtHipScene *sc, rtHipTemporalClampParams *out)
{
    if (!sc || !out) return fail("null argument");
    *out = sc->temporal.clamp; // (zeroed while off)
    return sc->temporal.clampOn ? 1 : 0;
}

int rtHipSceneTemporalTimes(const rtHipScene *sc, cl_float *ms)
{
    if (!sc || !ms) return fail("null argument");
    for (int i = 0; i < 4; ++i) ms[i] = sc->temporal.ms[i];
    return 0;
}

// ---- motion blur (include/raytrace_hip.h, "MOTION BLUR"; kernels in rt_motion_blur.hip) ---------------------------------------------
// Filter scratch of a W x H image: lz = (l, depth) per pixel as 2 f32, rounded up to 16 bytes, then tileMax and nbMax as float4 per
// 32 x 32 tile.
void rtHipMotionBlurDefaults(rtHipMotionBlurParams *p)
{
    if (!p) return;
    p->shutter = 0.5f;
    p->maxBlur = 16.0f;
    p->taps = 15;
    p->depthSoftness = 0.05f;
}

int rtHipMotionBlurCheck(const rtHipMotionBlurParams *p)
{
    if (!p) return fail("motion blur: null parameters");
    if (!(std::isfinite(p->shutter) && p->shutter >= 0.f && p->shutter <= 4.0f))
        return fail("motion blur: shutter %g is not finite and in 0..4", (double)p->shutter);
    if (!(std::isfinite(p->maxBlur) && p->maxBlur >= 1.0f && p->maxBlur <= 32.0f))
        return fail("motion blur: maxBlur %g is not finite and in 1..32", (double)p->maxBlur);
    if (p->taps < 1 || p->taps > 64) return fail("motion blur: taps %u is not in 1..64", p->taps);
    if (!(std::isfinite(p->depthSoftness) && p->depthSoftness >= 0.f))
        return fail("motion blur: depthSoftness %g is not finite and >= 0", (double)p->depthSoftness);
    return 0;
}

static bool motion_blur_size_legal(uint32_t W, uint32_t H)
{
    return W != 0 && H != 0 && W <= RT_TEMPORAL_MAX_SIDE && H <= RT_TEMPORAL_MAX_SIDE && (uint64_t)W * H <= RT_DENOISE_MAX_PIXELS;
}

static int motion_blur_size_ok(uint32_t W, uint32_t H)
{
    if (!motion_blur_size_legal(W, H))
        return fail("motion blur: a %u x %u image is not 1..16384 pixels wide and high and 1..2^27 pixels", W, H);
    return 0;
}

static uint64_t motion_blur_tiles(uint32_t W, uint32_t H) { return (uint64_t)((W + 31u) / 32u) * ((H + 31u) / 32u); }
static uint64_t motion_blur_lz_bytes(uint32_t W, uint32_t H) { return ((uint64_t)W * H * 8 + 15) & ~15ull; }

uint64_t rtHipMotionBlurScratchBytes(cl_uint width, cl_uint height)
{
    if (!motion_blur_size_legal(width, height)) return 0;
    return motion_blur_lz_bytes(width, height) + 2 * motion_blur_tiles(width, height) * 16;
}

// Issues the filter on `st`; arguments were checked by the caller.
static int motion_blur_issue(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *depth, float *out, char *scratch,
                             const rtHipMotionBlurParams *p, hipStream_t st)
{
    char *tileMax = scratch + motion_blur_lz_bytes(W, H), *nbMax = tileMax + motion_blur_tiles(W, H) * 16;
    HIP_OK(rmb_launch(W, H, colour, motion, depth, out, (float *)scratch, (float *)tileMax, (float *)nbMax, p->shutter, p->maxBlur, p->taps,
                      p->depthSoftness, st));
    return 0;
}

int rtHipMotionBlurDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *depth, void *out,
                          void *scratch, uint64_t scratchBytes, const rtHipMotionBlurParams *params, void *stream)
{
    if (rtHipMotionBlurCheck(params) != 0 || motion_blur_size_ok(width, height) != 0) return -1;
    if (!colour || !motion || !depth || !out || !scratch) return fail("motion blur: null array");
    const uint64_t n = (uint64_t)width * height, need = rtHipMotionBlurScratchBytes(width, height);
    if (scratchBytes < need)
        return fail("motion blur: scratch of %llu bytes, %llu needed", (unsigned long long)scratchBytes, (unsigned long long)need);
    const RtArray arr[5] = { { colour, n * 12, 4, "colour" }, { motion, n * 8, 4, "motion" }, { depth, n * 4, 4, "depth" },
                             { out, n * 12, 4, "out", true }, { scratch, need, 16, "scratch", true } };
    if (checked_device_arrays("motion blur", device, stream, arr, 5) != 0) return -1;
    return motion_blur_issue(width, height, (const float *)colour, (const float *)motion, (const float *)depth, (float *)out, (char *)scratch,
                             params, (hipStream_t)stream);
}

int rtHipMotionBlur(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *depth,
                    cl_float *out, const rtHipMotionBlurParams *params)
{
    if (rtHipMotionBlurCheck(params) != 0 || motion_blur_size_ok(width, height) != 0) return -1;
    if (!colour || !motion || !depth || !out) return fail("motion blur: null array");
    HIP_OK(hipSetDevice(device));
    const size_t n = (size_t)width * height;
    HostStage dev;
    const float *c = dev.up(colour, n * 12), *m = dev.up(motion, n * 8), *z = dev.up(depth, n * 4);
    float *dout = dev.out<float>(n * 12);
    char *scratch = dev.out<char>(rtHipMotionBlurScratchBytes(width, height));
    if (dev.status != hipSuccess) return dev.failed();
    if (motion_blur_issue(width, height, c, m, z, dout, scratch, params, nullptr) != 0) return -1;
    HIP_OK(hipMemcpy(out, dout, n * 12, hipMemcpyDeviceToHost));
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

int rtHipSceneMotionBlur(rtHipScene *sc, const rtHipMotionBlurParams *params, cl_float *outRgb, cl_ushort *outR, cl_ushort *outG,
                         cl_ushort *outB)
{
    if (!sc) return fail("motion blur: null scene");
    if (rtHipMotionBlurCheck(params) != 0 || motion_blur_size_ok(sc->width, sc->height) != 0) return -1;
    if (whole_image_tiles(sc, "motion blur") != 0) return -1;
    if (!sc->motion.have) return fail("motion blur: no motion reference (rtHipSceneMotionMark)");
    if (sc->dev.triangleCount != sc->motion.triangles)
        return fail("motion blur: the scene has %u triangles, the motion reference was made for %u", sc->dev.triangleCount, sc->motion.triangles);
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipDeviceSynchronize());
    if (frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, nullptr) != 0) return -1;
    rtHipScene::MotionBlur &B = sc->motionBlur;
    const uint32_t W = sc->width, H = sc->height;
    const size_t n = (size_t)W * H;
    const auto part = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    if (!B.buf) { // motion | t | colour | out | R | G | B | scratch
        const uint64_t bytes = part(n * 8) + part(n * 4) + 2 * part(n * 12) + 3 * part(n * 2) + part(rtHipMotionBlurScratchBytes(W, H));
        if (scene_block(sc, B.buf, bytes, "motion blur") != 0) return -1;
    }
    for (Event &e : B.ev) HIP_OK(e.make());
    char *b = B.buf;
    float *motion = (float *)b, *t = (float *)(b + part(n * 8)), *colour = (float *)(b + part(n * 8) + part(n * 4));
    float *out = (float *)((char *)colour + part(n * 12));
    char *plane = (char *)out + part(n * 12);
    const Planes planes = { (uint16_t *)plane, (uint16_t *)(plane + part(n * 2)), (uint16_t *)(plane + 2 * part(n * 2)) };
    char *scratch = plane + 3 * part(n * 2);
    hipStream_t st = sc->stream;
    HIP_OK(hipEventRecord(B.ev[0], st));
    if (motion_run(sc, motion, t, nullptr, nullptr, true, st) != 0) return -1;
    HIP_OK(hipEventRecord(B.ev[1], st));
    HIP_OK(rtt_launch_gather(W, H, sc->tilesX, sc->dev.tileIds, (uint32_t)sc->tileIds.size(), sc->dev.tileBuf, colour, st));
    HIP_OK(hipEventRecord(B.ev[2], st));
    if (motion_blur_issue(W, H, colour, motion, t, out, scratch, params, st) != 0) return -1;
    if (outR || outG || outB) HIP_OK(rtt_launch_quantise((uint32_t)n, out, planes.r, planes.g, planes.b, st));
    HIP_OK(hipEventRecord(B.ev[3], st));
    HIP_OK(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) HIP_OK(hipEventElapsedTime(&B.ms[i], B.ev[i], B.ev[i + 1]));
    return scene_outputs_to_host(n, out, planes, outRgb, outR, outG, outB);
}

int rtHipSceneMotionBlurTimes(const rtHipScene *sc, cl_float *ms)
{
    if (!sc || !ms) return fail("null argument");
    for (int i = 0; i < 3; ++i) ms[i] = sc->motionBlur.ms[i];
    return 0;
}

// ---- depth of field (include/raytrace_hip.h, "DEPTH OF FIELD"; kernels in rt_dof.hip) ------------------------------------------------
// Filter scratch of a W x H image: rz = (r, depth) per pixel as 2 f32, rounded up to 16 bytes, then tileMax and nbMax as one float per
// 32 x 32 tile, each rounded up to 16 bytes.
void rtHipDepthOfFieldDefaults(rtHipDepthOfFieldParams *p)
{
    if (!p) return;
    p->focus = 1.0f;
    p->cocScale = 8.0f;
    p->maxCoc = 16.0f;
    p->rings = 3;
    p->depthSoftness = 0.05f;
}

static int dof_focus_ok(float focus)
{
    if (!(std::isfinite(focus) && focus > 0.f)) return fail("depth of field: focus %g is not finite and > 0", (double)focus);
    return 0;
}

static int dof_coc_scale_ok(float cocScale)
{
    if (!(std::isfinite(cocScale) && cocScale >= 0.f && cocScale <= 4096.0f))
        return fail("depth of field: cocScale %g is not finite and in 0..4096", (double)cocScale);
    return 0;
}

int rtHipDepthOfFieldCheck(const rtHipDepthOfFieldParams *p)
{
    if (!p) return fail("depth of field: null parameters");
    if (dof_focus_ok(p->focus) != 0 || dof_coc_scale_ok(p->cocScale) != 0) return -1;
    if (!(std::isfinite(p->maxCoc) && p->maxCoc >= 1.0f && p->maxCoc <= 32.0f))
        return fail("depth of field: maxCoc %g is not finite and in 1..32", (double)p->maxCoc);
    if (p->rings < 1 || p->rings > 6) return fail("depth of field: rings %u is not in 1..6", p->rings);
    if (!(std::isfinite(p->depthSoftness) && p->depthSoftness >= 0.f))
        return fail("depth of field: depthSoftness %g is not finite and >= 0", (double)p->depthSoftness);
    return 0;
}

static bool dof_size_legal(uint32_t W, uint32_t H)
{
    return W != 0 && H != 0 && W <= RT_TEMPORAL_MAX_SIDE && H <= RT_TEMPORAL_MAX_SIDE && (uint64_t)W * H <= RT_DENOISE_MAX_PIXELS;
}

static int dof_size_ok(uint32_t W, uint32_t H)
{
    if (!dof_size_legal(W, H))
        return fail("depth of field: a %u x %u image is not 1..16384 pixels wide and high and 1..2^27 pixels", W, H);
    return 0;
}

static uint64_t dof_rz_bytes(uint32_t W, uint32_t H) { return ((uint64_t)W * H * 8 + 15) & ~15ull; }
static uint64_t dof_tile_bytes(uint32_t W, uint32_t H) { return ((uint64_t)((W + 31u) / 32u) * ((H + 31u) / 32u) * 4 + 15) & ~15ull; }

uint64_t rtHipDepthOfFieldScratchBytes(cl_uint width, cl_uint height)
{
    if (!dof_size_legal(width, height)) return 0;
    return dof_rz_bytes(width, height) + 2 * dof_tile_bytes(width, height);
}

// Issues the filter on `st`; arguments were checked by the caller.
static int dof_issue(uint32_t W, uint32_t H, const float *colour, const float *depth, float *out, char *scratch,
                     const rtHipDepthOfFieldParams *p, hipStream_t st)
{
    char *tileMax = scratch + dof_rz_bytes(W, H), *nbMax = tileMax + dof_tile_bytes(W, H);
    HIP_OK(rdf_launch(W, H, colour, depth, out, (float *)scratch, (float *)tileMax, (float *)nbMax, p->focus, p->cocScale, p->maxCoc, p->rings,
                      p->depthSoftness, st));
    return 0;
}

int rtHipDepthOfFieldDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *depth, void *out, void *scratch,
                            uint64_t scratchBytes, const rtHipDepthOfFieldParams *params, void *stream)
{
    if (rtHipDepthOfFieldCheck(params) != 0 || dof_size_ok(width, height) != 0) return -1;
    if (!colour || !depth || !out || !scratch) return fail("depth of field: null array");
    const uint64_t n = (uint64_t)width * height, need = rtHipDepthOfFieldScratchBytes(width, height);
    if (scratchBytes < need)
        return fail("depth of field: scratch of %llu bytes, %llu needed", (unsigned long long)scratchBytes, (unsigned long long)need);
    const RtArray arr[4] = { { colour, n * 12, 4, "colour" }, { depth, n * 4, 4, "depth" }, { out, n * 12, 4, "out", true },
                             { scratch, need, 16, "scratch", true } };
    if (checked_device_arrays("depth of field", device, stream, arr, 4) != 0) return -1;
    return dof_issue(width, height, (const float *)colour, (const float *)depth, (float *)out, (char *)scratch, params, (hipStream_t)stream);
}

int rtHipDepthOfField(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *depth, cl_float *out,
                      const rtHipDepthOfFieldParams *params)
{
    if (rtHipDepthOfFieldCheck(params) != 0 || dof_size_ok(width, height) != 0) return -1;
    if (!colour || !depth || !out) return fail("depth of field: null array");
    HIP_OK(hipSetDevice(device));
    const size_t n = (size_t)width * height;
    HostStage dev;
    const float *c = dev.up(colour, n * 12), *z = dev.up(depth, n * 4);
    float *dout = dev.out<float>(n * 12);
    char *scratch = dev.out<char>(rtHipDepthOfFieldScratchBytes(width, height));
    if (dev.status != hipSuccess) return dev.failed();
    if (dof_issue(width, height, c, z, dout, scratch, params, nullptr) != 0) return -1;
    HIP_OK(hipMemcpy(out, dout, n * 12, hipMemcpyDeviceToHost));
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

int rtHipSceneDepthOfField(rtHipScene *sc, const rtHipDepthOfFieldParams *params, cl_float *outRgb, cl_ushort *outR, cl_ushort *outG,
                           cl_ushort *outB)
{
    if (!sc) return fail("depth of field: null scene");
    if (rtHipDepthOfFieldCheck(params) != 0 || dof_size_ok(sc->width, sc->height) != 0) return -1;
    if (!(sc->passMask & RT_HIP_PASS_DEPTH) || !sc->passBuf)
        return fail("depth of field needs the depth pass on for this scene (rtHipScenePasses)");
    if (whole_image_tiles(sc, "depth of field") != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipDeviceSynchronize());
    if (frame_finish(sc, sc->lastStream ? sc->lastStream : sc->stream, nullptr) != 0) return -1;
    rtHipScene::DepthOfField &D = sc->dof;
    const uint32_t W = sc->width, H = sc->height;
    const size_t n = (size_t)W * H;
    const auto part = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    if (!D.buf) { // colour | depth | out | R | G | B | scratch
        const uint64_t bytes = 2 * part(n * 12) + part(n * 4) + 3 * part(n * 2) + part(rtHipDepthOfFieldScratchBytes(W, H));
        if (scene_block(sc, D.buf, bytes, "depth of field") != 0) return -1;
    }
    for (Event &e : D.ev) HIP_OK(e.make());
    char *b = D.buf;
    float *colour = (float *)b, *depth = (float *)(b + part(n * 12)), *out = (float *)(b + part(n * 12) + part(n * 4));
    char *plane = (char *)out + part(n * 12);
    const Planes planes = { (uint16_t *)plane, (uint16_t *)(plane + part(n * 2)), (uint16_t *)(plane + 2 * part(n * 2)) };
    char *scratch = plane + 3 * part(n * 2);
    hipStream_t st = sc->stream;
    HIP_OK(hipEventRecord(D.ev[0], st));
    HIP_OK(rdf_launch_scene_gather(W, H, sc->tilesX, sc->dev.tileIds, (uint32_t)sc->tileIds.size(), sc->dev.tileBuf, sc->passBuf, colour, depth,
                                   st));
    HIP_OK(hipEventRecord(D.ev[1], st));
    if (dof_issue(W, H, colour, depth, out, scratch, params, st) != 0) return -1;
    HIP_OK(hipEventRecord(D.ev[2], st));
    if (outR || outG || outB) HIP_OK(rtt_launch_quantise((uint32_t)n, out, planes.r, planes.g, planes.b, st));
    HIP_OK(hipEventRecord(D.ev[3], st));
    HIP_OK(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) HIP_OK(hipEventElapsedTime(&D.ms[i], D.ev[i], D.ev[i + 1]));
    return scene_outputs_to_host(n, out, planes, outRgb, outR, outG, outB);
}

int rtHipSceneDepthOfFieldTimes(const rtHipScene *sc, cl_float *ms)
{
    if (!sc || !ms) return fail("null argument");
    for (int i = 0; i < 3; ++i) ms[i] = sc->dof.ms[i];
    return 0;
}

// The thin lens of the header, in double with + - * / and sqrt, each result rounded once to float (tests/dof_oracle.py: lens).
int rtHipDepthOfFieldLens(const rtHipCamera *cam, cl_float apertureRadius, cl_float focus, rtHipDepthOfFieldParams *inout)
{
    if (!cam || !inout) return fail("depth of field: null argument");
    const double tl[3] = { cam->eyeToTopLeft[0], cam->eyeToTopLeft[1], cam->eyeToTopLeft[2] };
    const double lr[3] = { cam->leftToRight[0], cam->leftToRight[1], cam->leftToRight[2] };
    const double tb[3] = { cam->topToBottom[0], cam->topToBottom[1], cam->topToBottom[2] };
    const double nv[3] = { lr[1] * tb[2] - lr[2] * tb[1], lr[2] * tb[0] - lr[0] * tb[2], lr[0] * tb[1] - lr[1] * tb[0] };
    const auto dot = [](const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
    double h = dot(tl, nv);
    if (h < 0) h = -h;
    const double plane = h / std::sqrt(dot(nv, nv)), pitch = std::sqrt(dot(lr, lr));
    if (!(std::isfinite(plane) && plane > 0 && std::isfinite(pitch) && pitch > 0))
        return fail("depth of field: the camera's plane distance %g or pixel pitch %g is zero or not finite", plane, pitch);
    const double focalPixels = plane / pitch;
    const float cocScale = (float)(((double)apertureRadius * focalPixels) / (double)focus);
    if (dof_focus_ok(focus) != 0 || dof_coc_scale_ok(cocScale) != 0) return -1;
    inout->focus = focus;
    inout->cocScale = cocScale;
    return 0;
}
