// rt_matte.cpp -- the mattes of libraytrace_hip.so (include/raytrace_hip.h, "MATTES"): the parameter check and defaults, the scene's group
// table, the device and host entry points with the scene-owned state between a call's launches, and the last call's device times.  The
// kernels are in rt_scene_passes.hip (rt_matte_*); the scene and what else the host side shares, in rt_host.h.
#include "rt_host.h"
#include "rt_launch.h"
#include "rt_tile_order.h"

using namespace rthost;

static_assert(RT_HIP_MATTE_MAX_SELECT == RT_MATTE_MAX_SELECT && RT_HIP_MATTE_MAX_LAYERS == RT_MATTE_MAX_LAYERS, "the ABI's bounds are the kernels'");
static_assert(RT_HIP_MATTE_TRIANGLE == RT_MATTE_TRIANGLE && RT_HIP_MATTE_MATERIAL == RT_MATTE_MATERIAL && RT_HIP_MATTE_GROUP == RT_MATTE_GROUP,
              "the ABI's kinds are the kernels'");
#define RT_MATTE_MAX_SAMPLES 65536u

int rtHipMatteCheck(const rtHipMatteParams *p)
{
    if (!p) return fail("mattes: null parameters");
    if (p->kind > RT_HIP_MATTE_GROUP) return fail("mattes: kind %u is not RT_HIP_MATTE_TRIANGLE, _MATERIAL or _GROUP", p->kind);
    if (p->total == 0) return fail("mattes: total must be >= 1");
    if (p->samples == 0 || p->samples > RT_MATTE_MAX_SAMPLES) return fail("mattes: samples %u is not in 1..%u", p->samples, RT_MATTE_MAX_SAMPLES);
    if ((uint64_t)p->first + p->samples > p->total)
        return fail("mattes: first + samples = %u + %u reaches past total = %u", p->first, p->samples, p->total);
    if (p->selectCount > RT_HIP_MATTE_MAX_SELECT) return fail("mattes: selectCount %u is more than %d", p->selectCount, RT_HIP_MATTE_MAX_SELECT);
    if (p->layers > RT_HIP_MATTE_MAX_LAYERS) return fail("mattes: layers %u is more than %d", p->layers, RT_HIP_MATTE_MAX_LAYERS);
    if (p->selectCount == 0 && p->layers == 0) return fail("mattes: neither a selected id nor a layer is asked for");
    for (uint32_t m = 0; m < p->selectCount; ++m)
        if (p->select[m] == RT_HIP_MATTE_NONE) return fail("mattes: select[%u] is 0xffffffff, the id of no sample", m);
    return 0;
}

int rtHipMatteDefaults(const rtHipScene *sc, rtHipMatteParams *p)
{
    if (!sc || !p) return fail("rtHipMatteDefaults: null argument");
    memset(p, 0, sizeof *p);
    const uint32_t S = sc->dev.sampleCount;
    const bool rendered = sc->lastWindow.total != 0u; // (all zero before the first frame)
    p->kind = RT_HIP_MATTE_TRIANGLE;
    p->total = rendered ? sc->lastWindow.total : S;
    p->first = rendered ? sc->lastWindow.first : 0u;
    p->samples = S;
    p->selectCount = 0;
    p->layers = 4;
    return 0;
}

int rtHipSceneSetMatteGroups(rtHipScene *sc, const cl_uint *groups, cl_int onDevice)
{
    const char *who = "rtHipSceneSetMatteGroups";
    if (!sc) return fail("%s: null scene", who);
    HIP_OK(hipSetDevice(sc->device));
    rtHipScene::Matte &M = sc->matte;
    if (M.issued) HIP_OK(hipEventSynchronize(M.ev[2])); // the last call that read the table, on whatever stream it ran
    if (!groups) {
        M.groups.drop(sc->bytes);
        return 0;
    }
    const uint64_t T = sc->dev.triangleCount;
    if (onDevice && T && query_pointer_ok(sc->device, "the scene", groups, T * 4, 4, "groups") != 0) return -1;
    if (!M.groups && scene_block(sc, M.groups, (T ? T : 1) * 4, who) != 0) return -1;
    if (T) HIP_OK(sc->stager.copy(M.groups, groups, T * 4));
    HIP_OK(sc->stager.drain());
    HIP_OK(hipStreamSynchronize(sc->stream));
    return 0;
}

// What both entry points refuse before anything is touched.
static int matte_check(const rtHipScene *sc, const rtHipMatteParams *p, const void *select, const void *layerId, const void *layerCoverage,
                       const void *rest)
{
    if (!sc || !p) return fail("mattes: null scene or parameters");
    if (rtHipMatteCheck(p) != 0) return -1;
    if (!select && !layerId && !layerCoverage && !rest) return fail("mattes: every output is null");
    if (select && p->selectCount == 0) return fail("mattes: a select output with selectCount 0");
    if ((layerId || layerCoverage) && p->layers == 0) return fail("mattes: a layer output with layers 0");
    if (p->kind == RT_HIP_MATTE_GROUP && !sc->matte.groups) return fail("mattes: kind GROUP needs a group table (rtHipSceneSetMatteGroups)");
    if ((uint64_t)sc->width * sc->height >= (1ull << 32)) return fail("mattes: %u x %u is 2^32 pixels or more", sc->width, sc->height);
    return 0;
}

// Enqueues the whole pass on `st`: the chunks' count launches one after the other, then the finish kernel -- into the four row-major
// arrays, or (rowMajor false) over the state itself, tile by tile.
static int matte_run(rtHipScene *sc, const rtHipMatteParams *p, void *select, void *layerId, void *layerCoverage, void *rest, bool rowMajor,
                     hipStream_t st)
{
    const uint32_t chunk = std::min<uint32_t>(std::max<uint32_t>(tuning_now().matteChunk, 1u), RT_MATTE_MAX_SAMPLES); // this call's one look
    rtHipScene::Matte &M = sc->matte;
    const uint32_t words = p->selectCount + 2u * p->layers + 1u;
    const uint64_t need = std::max<uint64_t>((uint64_t)sc->tileIds.size() * words * RT_TILE_PIXELS * 4, 256);
    for (Event &e : M.ev)
        if (scene_event(e, hipEventDefault, "mattes") != 0) return -1;
    if (M.issued) {
        // the last call's use of the state, on whatever stream it ran: before this call's launches, and before a block that grows is freed
        if (M.state.size < need) HIP_OK(hipEventSynchronize(M.ev[2]));
        else HIP_OK(hipStreamWaitEvent(st, M.ev[2], 0));
    }
    if (M.state.fit(need, need, sc->bytes) != hipSuccess) return fail("mattes: hipMalloc(%llu) failed", (unsigned long long)need);
    M.words = words;

    RtMatteArgs A;
    memset(&A, 0, sizeof A);
    A.kind = p->kind; A.seedStride = p->total;
    A.selectCount = p->selectCount; A.layers = p->layers; A.words = words;
    for (uint32_t m = 0; m < RT_MATTE_MAX_SELECT; ++m) A.select[m] = m < p->selectCount ? p->select[m] : RT_HIP_MATTE_NONE;
    A.groups = M.groups; A.state = M.state;
    A.den = (float)p->samples; A.rowMajor = rowMajor ? 1u : 0u;
    A.outSelect = (float *)select; A.outLayerId = (uint32_t *)layerId; A.outLayerCoverage = (float *)layerCoverage; A.outRest = (float *)rest;
    HIP_OK(hipEventRecord(M.ev[0], st));
    for (uint32_t done = 0; done < p->samples; done += chunk) {
        A.sampleFirst = p->first + done; A.samples = std::min(chunk, p->samples - done); A.first = done == 0u ? 1u : 0u;
        HIP_OK(rtw_launch_matte_count(&sc->dev, &A, st));
    }
    HIP_OK(hipEventRecord(M.ev[1], st));
    HIP_OK(rtw_launch_matte_finish(&sc->dev, &A, st));
    HIP_OK(hipEventRecord(M.ev[2], st));
    M.issued = true;
    return 0;
}

int rtHipSceneMattesDevice(rtHipScene *sc, const rtHipMatteParams *p, void *select, void *layerId, void *layerCoverage, void *rest, void *stream)
{
    if (matte_check(sc, p, select, layerId, layerCoverage, rest) != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    const uint64_t plane = (uint64_t)sc->width * sc->height * 4;
    if ((select && query_pointer_ok(sc->device, "the scene", select, plane * p->selectCount, 4, "select") != 0) ||
        (layerId && query_pointer_ok(sc->device, "the scene", layerId, plane * p->layers, 4, "layerId") != 0) ||
        (layerCoverage && query_pointer_ok(sc->device, "the scene", layerCoverage, plane * p->layers, 4, "layerCoverage") != 0) ||
        (rest && query_pointer_ok(sc->device, "the scene", rest, plane, 4, "rest") != 0))
        return -1;
    return matte_run(sc, p, select, layerId, layerCoverage, rest, true, stream ? (hipStream_t)stream : sc->stream);
}

int rtHipSceneMattes(rtHipScene *sc, const rtHipMatteParams *p, cl_float *select, cl_uint *layerId, cl_float *layerCoverage, cl_float *rest)
{
    if (matte_check(sc, p, select, layerId, layerCoverage, rest) != 0) return -1;
    HIP_OK(hipSetDevice(sc->device));
    // the finished values overwrite the state tile by tile, select | layer ids | layer coverages | rest; the host stores the scene's pixels
    if (matte_run(sc, p, nullptr, nullptr, nullptr, nullptr, false, sc->stream) != 0) return -1;
    const uint32_t M = p->selectCount, K = p->layers, words = M + 2u * K + 1u;
    const size_t nt = sc->tileIds.size();
    std::vector<uint32_t> host(nt * words * RT_TILE_PIXELS);
    if (!host.empty()) HIP_OK(hipMemcpyAsync(host.data(), sc->matte.state, host.size() * 4, hipMemcpyDeviceToHost, sc->stream));
    HIP_OK(hipStreamSynchronize(sc->stream));
    const size_t plane = (size_t)sc->width * sc->height;
    rt_tile_walk_rows(sc->tileIds.data(), nt, sc->tilesX, sc->width, sc->height, [&](size_t s, uint32_t ly, size_t at, uint32_t n) {
        // word w of the state is plane `k` of the caller's array `dst` (32-bit words either way)
        auto row = [&](uint32_t w, void *dst, uint32_t k) {
            memcpy((uint32_t *)dst + k * plane + at, host.data() + (s * words + w) * RT_TILE_PIXELS + (size_t)ly * RT_TILE, (size_t)n * 4);
        };
        for (uint32_t m = 0; select && m < M; ++m) row(m, select, m);
        for (uint32_t k = 0; layerId && k < K; ++k) row(M + k, layerId, k);
        for (uint32_t k = 0; layerCoverage && k < K; ++k) row(M + K + k, layerCoverage, k);
        if (rest) row(M + 2u * K, rest, 0);
    });
    return 0;
}

int rtHipSceneMatteTimes(rtHipScene *sc, double ms[2])
{
    if (!sc || !ms) return fail("rtHipSceneMatteTimes: null argument");
    ms[0] = ms[1] = 0.0;
    rtHipScene::Matte &M = sc->matte;
    if (!M.issued) return 0;
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(hipEventSynchronize(M.ev[2]));
    float t[2] = {};
    HIP_OK(hipEventElapsedTime(&t[0], M.ev[0], M.ev[1]));
    HIP_OK(hipEventElapsedTime(&t[1], M.ev[1], M.ev[2]));
    ms[0] = t[0]; ms[1] = t[1];
    return 0;
}
