// rt_scene_passes.hip -- what is traced against a resident scene outside the frame, for gfx950 (MI355X): the mattes, ray queries, ambient
// occlusion, motion vectors and the ambient occlusion bake, each section with its kernels and their launch wrappers (declared in
// rt_launch.h).  No frame launches any of these.  They read the scene the way the frame's kernels do (rt_wavefront.hip) -- the camera
// scan, the dense grid view, the trace entries' plane search -- through the helpers of rt_wf_shared.h; the host side is in rt_api.cpp
// and rt_matte.cpp.
// A translation unit of its own: a change to a pass recompiles no frame kernel, and a change to the frame none of these.
#include "rt_devfuncs.h"
#include "rt_launch.h"
#include "rt_tile_order.h"
#include "rt_wf_shared.h"

// ---- mattes: id coverage over a pixel's samples (rtHipSceneMattes*; include/raytrace_hip.h, "MATTES"; rt_device.h, RtMatteArgs) -------
// The mapping of wf_surface_passes_kernel (ONE thread per pixel, a wave an 8x8 quadrant whose lanes scan overlapping camera lists), and
// its way of deriving each sample's primary hit again; what is summed is an indicator.  The M selected counts, the K layer slots and
// rest stay in registers across the chunk's samples: every loop below runs to a compile-time bound and indexes its array with the loop
// variable, so the arrays are registers, and the bounds that are the call's (M, K) and the id's kind are uniform kernel arguments.
// Chunks of one call follow one another on one stream: the table is built in sample order without atomics.
__global__ __launch_bounds__(256) void rt_matte_count_kernel(const RtDevScene S, const RtMatteArgs A)
{
    const uint32_t slot = blockIdx.x >> 6, patch = blockIdx.x & 63;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t lx = (patch & 7) * RT_PATCH + (wave & 1) * 8 + (lane & 7);
    const uint32_t ly = (patch >> 3) * RT_PATCH + (wave >> 1) * 8 + (lane >> 3);
    const uint32_t tile = S.tileIds[slot];
    const uint32_t gx = (tile % S.tilesX) * RT_TILE + lx;
    const uint32_t gy = (tile / S.tilesX) * RT_TILE + ly;
    if (gx >= S.width || gy >= S.height) return;

    const uint32_t localPixel = slot * RT_TILE_PIXELS + ly * RT_TILE + lx;
    uint32_t *state = A.state + (size_t)slot * A.words * RT_TILE_PIXELS + ly * RT_TILE + lx;
    const uint32_t M = A.selectCount, K = A.layers;
    uint32_t sel[RT_MATTE_MAX_SELECT], id[RT_MATTE_MAX_LAYERS], cnt[RT_MATTE_MAX_LAYERS], rest = 0u;
#pragma unroll
    for (int m = 0; m < RT_MATTE_MAX_SELECT; ++m) sel[m] = 0u;
#pragma unroll
    for (int k = 0; k < RT_MATTE_MAX_LAYERS; ++k) { id[k] = RT_NONE; cnt[k] = 0u; }
    if (!A.first) {
#pragma unroll
        for (int m = 0; m < RT_MATTE_MAX_SELECT; ++m)
            if ((uint32_t)m < M) sel[m] = state[(size_t)m * RT_TILE_PIXELS];
#pragma unroll
        for (int k = 0; k < RT_MATTE_MAX_LAYERS; ++k)
            if ((uint32_t)k < K) {
                id[k] = state[(size_t)(M + k) * RT_TILE_PIXELS];
                cnt[k] = state[(size_t)(M + K + k) * RT_TILE_PIXELS];
            }
        rest = state[(size_t)(M + 2u * K) * RT_TILE_PIXELS];
    }
    const uint32_t pixel = gy * S.width + gx;
    const V3 eye = ld3(S.eye), lr = ld3(S.lr), tb = ld3(S.tb), topLeft = ld3(S.topLeft);
    for (uint32_t j = 0; j < A.samples; ++j) {
        uint64_t rng = (uint64_t)pixel * (uint64_t)A.seedStride + ((uint64_t)A.sampleFirst + j + 1u); // :481
        V3 dir = topLeft;
        float k = (float)gx + rand01(rng); // LR jitter first, then TB (:496-503)
        dir.x += lr.x * k; dir.y += lr.y * k; dir.z += lr.z * k;
        k = (float)gy + rand01(rng);
        dir.x += tb.x * k; dir.y += tb.y * k; dir.z += tb.z * k;
        float hit_t = 0.f, hit_l1 = 0.f, hit_l2 = 0.f;
        const uint32_t tri = camera_scan(S, localPixel, eye, dir, 0.f, RT_INF, RT_NONE, hit_t, hit_l1, hit_l2);
        uint32_t g = tri;
        if (tri != RT_NONE) {
            if (A.kind == RT_MATTE_MATERIAL) {
                const int m = __float_as_int(S.triShade[RT_TRI_SHADE_WORDS * (size_t)tri + 21]);
                g = m < 0 ? RT_NONE : (uint32_t)m;
            } else if (A.kind == RT_MATTE_GROUP) g = A.groups[tri];
        }
        if (g == RT_NONE) continue;
#pragma unroll
        for (int m = 0; m < RT_MATTE_MAX_SELECT; ++m) sel[m] += (g == A.select[m]) ? 1u : 0u; // (entries from M on are NONE)
        // find or insert: the used slots are a prefix, so whether g was found is settled before the first free slot is reached
        bool settled = false;
#pragma unroll
        for (int s = 0; s < RT_MATTE_MAX_LAYERS; ++s) {
            const bool open = (uint32_t)s < K && !settled;
            const bool used = cnt[s] != 0u;
            const bool match = open && used && id[s] == g, take = open && !used;
            id[s] = take ? g : id[s];
            cnt[s] += (match || take) ? 1u : 0u;
            settled = settled || match || take;
        }
        rest += settled ? 0u : 1u;
    }
#pragma unroll
    for (int m = 0; m < RT_MATTE_MAX_SELECT; ++m)
        if ((uint32_t)m < M) state[(size_t)m * RT_TILE_PIXELS] = sel[m];
#pragma unroll
    for (int k = 0; k < RT_MATTE_MAX_LAYERS; ++k)
        if ((uint32_t)k < K) {
            state[(size_t)(M + k) * RT_TILE_PIXELS] = id[k];
            state[(size_t)(M + K + k) * RT_TILE_PIXELS] = cnt[k];
        }
    state[(size_t)(M + 2u * K) * RT_TILE_PIXELS] = rest;
}

// One compare-exchange of the finish kernel's network.  A slot's key is ~count << 32 | id: ascending keys are counts descending, equal
// counts by id ascending, and a free slot (count 0, id NONE) is the largest key there is.
__device__ __forceinline__ void matte_exchange(unsigned long long &a, unsigned long long &b)
{
    const unsigned long long lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo; b = hi;
}

// One thread per pixel of the scene's tiles, row by row of its tile (the state is read, and the caller's arrays are written, in whole
// lines): the K slots ordered by Batcher's odd-even merge network for 8 keys (19 exchanges, fixed indices: registers), the quotients,
// and the stores -- row-major into the caller's arrays, or over the pixel's own state words for the host entry point, which walks them
// in the row order of rt_tile_order.h.
__global__ __launch_bounds__(256) void rt_matte_finish_kernel(const RtDevScene S, const RtMatteArgs A)
{
    const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
    if (lp >= S.tileCount * RT_TILE_PIXELS) return;
    const uint32_t slot = lp >> 14, q = lp & (RT_TILE_PIXELS - 1u);
    uint32_t x0, y0;
    rt_tile_origin(S.tileIds[slot], S.tilesX, x0, y0);
    const uint32_t gx = x0 + (q & (RT_TILE - 1u)), gy = y0 + (q >> 7);
    if (gx >= S.width || gy >= S.height) return;
    uint32_t *state = A.state + (size_t)slot * A.words * RT_TILE_PIXELS + q;
    const uint32_t M = A.selectCount, K = A.layers;
    uint32_t sel[RT_MATTE_MAX_SELECT];
    unsigned long long key[RT_MATTE_MAX_LAYERS];
#pragma unroll
    for (int m = 0; m < RT_MATTE_MAX_SELECT; ++m) sel[m] = (uint32_t)m < M ? state[(size_t)m * RT_TILE_PIXELS] : 0u;
#pragma unroll
    for (int k = 0; k < RT_MATTE_MAX_LAYERS; ++k) {
        const uint32_t c = (uint32_t)k < K ? state[(size_t)(M + K + k) * RT_TILE_PIXELS] : 0u;
        const uint32_t i = c != 0u ? state[(size_t)(M + k) * RT_TILE_PIXELS] : RT_NONE;
        key[k] = (unsigned long long)~c << 32 | i;
    }
    const uint32_t rest = state[(size_t)(M + 2u * K) * RT_TILE_PIXELS];
    matte_exchange(key[0], key[1]); matte_exchange(key[2], key[3]); matte_exchange(key[4], key[5]); matte_exchange(key[6], key[7]);
    matte_exchange(key[0], key[2]); matte_exchange(key[1], key[3]); matte_exchange(key[4], key[6]); matte_exchange(key[5], key[7]);
    matte_exchange(key[1], key[2]); matte_exchange(key[5], key[6]);
    matte_exchange(key[0], key[4]); matte_exchange(key[1], key[5]); matte_exchange(key[2], key[6]); matte_exchange(key[3], key[7]);
    matte_exchange(key[2], key[4]); matte_exchange(key[3], key[5]);
    matte_exchange(key[1], key[2]); matte_exchange(key[3], key[4]); matte_exchange(key[5], key[6]);
    const size_t plane = A.rowMajor ? (size_t)S.width * S.height : (size_t)RT_TILE_PIXELS;
    const size_t at = A.rowMajor ? (size_t)gy * S.width + gx : 0;
    // (every store is a 32-bit word store, the quotients as their bits: over the state they follow this thread's own loads of the same type)
    uint32_t *outSelect = A.rowMajor ? reinterpret_cast<uint32_t *>(A.outSelect) : state;
    uint32_t *outId = A.rowMajor ? A.outLayerId : state + (size_t)M * RT_TILE_PIXELS;
    uint32_t *outCov = A.rowMajor ? reinterpret_cast<uint32_t *>(A.outLayerCoverage) : state + (size_t)(M + K) * RT_TILE_PIXELS;
    uint32_t *outRest = A.rowMajor ? reinterpret_cast<uint32_t *>(A.outRest) : state + (size_t)(M + 2u * K) * RT_TILE_PIXELS;
    if (outSelect) {
#pragma unroll
        for (int m = 0; m < RT_MATTE_MAX_SELECT; ++m)
            if ((uint32_t)m < M) outSelect[(size_t)m * plane + at] = __float_as_uint((float)sel[m] / A.den);
    }
#pragma unroll
    for (int k = 0; k < RT_MATTE_MAX_LAYERS; ++k)
        if ((uint32_t)k < K) {
            if (outId) outId[(size_t)k * plane + at] = (uint32_t)key[k];
            if (outCov) outCov[(size_t)k * plane + at] = __float_as_uint((float)~(uint32_t)(key[k] >> 32) / A.den);
        }
    if (outRest) outRest[at] = __float_as_uint((float)rest / A.den);
}

// mattes: one chunk of samples counted into the state ...
extern "C" hipError_t rtw_launch_matte_count(const RtDevScene *scene, const RtMatteArgs *args, hipStream_t stream)
{
    if (scene->tileCount == 0 || args->samples == 0) return hipSuccess;
    if (args->kind > RT_MATTE_GROUP || args->selectCount > RT_MATTE_MAX_SELECT || args->layers > RT_MATTE_MAX_LAYERS || !args->state ||
        args->words != args->selectCount + 2u * args->layers + 1u || (args->kind == RT_MATTE_GROUP && !args->groups))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_matte_count_kernel, dim3(scene->tileCount * 64), dim3(256), 0, stream, *scene, *args);
    return hipGetLastError();
}

// ... and the finished values stored
extern "C" hipError_t rtw_launch_matte_finish(const RtDevScene *scene, const RtMatteArgs *args, hipStream_t stream)
{
    const uint32_t n = scene->tileCount * RT_TILE_PIXELS;
    if (n == 0) return hipSuccess;
    if (args->selectCount > RT_MATTE_MAX_SELECT || args->layers > RT_MATTE_MAX_LAYERS || !args->state ||
        args->words != args->selectCount + 2u * args->layers + 1u)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_matte_finish_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, *scene, *args);
    return hipGetLastError();
}

// ---- ray queries (rtHipSceneIntersect*): caller-supplied rays against the resident grid -------------------------------------
// One lane per ray: RayIntersectsTriangles (raytrace_opencl.c:324-401) over the dense view wf_trace_kernel reads (rt_device.h,
// gridBlockSparse / pairRec): one block-table look-up per 4x4x4 block the walk enters, one 64-byte gather per occupied cell (its
// first candidate and its count), the further candidates at `rest` in list order.  The running maximum is reset per cell (:366), a
// candidate replaces it only with a strictly smaller t (ties keep the earlier candidate), and the walk ends at the first cell with a
// hit, at the end cell, or where a step would leave the grid (:380-398).  Rays are {o.xyz, tmin} {d.xyz, tmax}; hits {t, triangle,
// abL, acL}, abL = acL = 0 and t = tmax on a miss.  Every input has a bounded walk that reads inside the grid arrays: cell_of is a
// binary search (coordinates in [0, 255] whatever the point, NaN included), and each step moves one axis one cell in the direction
// fixed by the sign of d, so a walk leaves the grid after at most 3 x 255 steps -- the loop bound only states that.
template <bool FAST>
__device__ __forceinline__ uint32_t query_walk(const RtDevScene &S, const float *planes, V3 o, V3 d, float tmin, float tmax, uint32_t excluded,
                                               float &hitT, float &hitL1, float &hitL2)
{
    const V3 lo = mk(planes[0], planes[RT_GRID_DIV + 1], planes[2 * (RT_GRID_DIV + 1)]);
    const V3 hi = mk(planes[RT_GRID_DIV], planes[2 * RT_GRID_DIV + 1], planes[3 * RT_GRID_DIV + 2]);
    V3 from = along(o, tmin, d);
    bind_in_cube(from, d, lo, hi);
    uint32_t cell = cell_of(planes, from), endCell = 0xffffffffu;
    if (tmax < RT_INF) {
        V3 to = along(o, tmax, d);
        bind_in_cube(to, d, lo, hi);
        endCell = cell_of(planes, to);
    }
    const bool px = (0.f <= d.x), py = (0.f <= d.y), pz = (0.f <= d.z);
    const float *planesY = planes + (RT_GRID_DIV + 1), *planesZ = planes + 2 * (RT_GRID_DIV + 1);
    uint32_t cx = cell & 255u, cy = (cell >> 8) & 255u, cz = cell >> 16;
    // distances from the ray ORIGIN to the next plane of each axis (:383-385); a step re-divides only the axis it moved
    float dx = (planes[cx + (px ? 1 : 0)] - o.x) / d.x;
    float dy = (planesY[cy + (py ? 1 : 0)] - o.y) / d.y;
    float dz = (planesZ[cz + (pz ? 1 : 0)] - o.z) / d.z;
    const float rx = FAST ? refined_rcp(d.x) : 0.f, ry = FAST ? refined_rcp(d.y) : 0.f, rz = FAST ? refined_rcp(d.z) : 0.f;
    const char *__restrict__ blockTable = reinterpret_cast<const char *>(S.gridBlockSparse);
    const float4 *__restrict__ recs = reinterpret_cast<const float4 *>(S.pairRec);
    uint32_t wordKey = 0xffffffffu, wordLo = 0, wordHi = 0, wordRank = 0;
    uint32_t best = RT_NONE;
    hitT = tmax;
#pragma unroll 1
    for (uint32_t visit = 0; visit < 3u * RT_GRID_DIV; ++visit) {
        cell = cx | (cy << 8) | (cz << 16);
        const uint32_t key = cell & 0xFCFCFCu;
        if (key != wordKey) {
            const uint3 w = *reinterpret_cast<const uint3 *>(blockTable + (size_t)key * 3u);
            wordKey = key; wordLo = w.x; wordHi = w.y; wordRank = w.z;
        }
        const uint32_t bit = (cx & 3u) | ((cy & 3u) << 2) | ((cz & 3u) << 4);
        const uint32_t below = (1u << (bit & 31u)) - 1u;
        const uint32_t half = (bit & 32u) ? wordHi : wordLo;
        if ((half >> (bit & 31u)) & 1u) {
            const uint32_t dense = wordRank + ((bit & 32u) ? __popc(wordLo) + __popc(wordHi & below) : __popc(wordLo & below));
            float tbest = tmax; // reset per cell (:366)
            const float4 *rec = recs + 4 * (size_t)dense;
            float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
            const uint32_t info = __float_as_uint(r1.w);
            float t, l1, l2;
            if (pair_test_flat(r0, r1, r2, r3, o, d, tmin, tbest, excluded, t, l1, l2)) {
                best = __float_as_uint(r0.w); tbest = t; hitL1 = l1; hitL2 = l2;
            }
            uint32_t n = info & 15u;
            if (n > 1u) {
                rec = recs + 4 * (size_t)(info >> 4);
                r0 = rec[0]; r1 = rec[1]; r2 = rec[2]; r3 = rec[3];
                if (n == RT_PAIR_MANY) n = __float_as_uint(r1.w); // (the first further record has the exact count)
#pragma unroll 1
                for (uint32_t i = 1;;) {
                    if (pair_test_flat(r0, r1, r2, r3, o, d, tmin, tbest, excluded, t, l1, l2)) {
                        best = __float_as_uint(r0.w); tbest = t; hitL1 = l1; hitL2 = l2;
                    }
                    if (++i >= n) break;
                    rec += 4;
                    r0 = rec[0]; r1 = rec[1]; r2 = rec[2]; r3 = rec[3];
                }
            }
            hitT = tbest;
            if (best != RT_NONE) break;
        }
        if (cell == endCell) break;
        // axis choice (:387-398): x only if strictly smallest, else y if smaller than z, else z; a step off the grid ends the walk
        if ((dx < dy) & (dx < dz)) {
            if (cx == (px ? 255u : 0u)) break;
            cx = px ? cx + 1u : cx - 1u;
            const float num = planes[cx + (px ? 1 : 0)] - o.x;
            dx = FAST ? tame_quotient(num, d.x, rx) : num / d.x;
        } else if (dy < dz) {
            if (cy == (py ? 255u : 0u)) break;
            cy = py ? cy + 1u : cy - 1u;
            const float num = planesY[cy + (py ? 1 : 0)] - o.y;
            dy = FAST ? tame_quotient(num, d.y, ry) : num / d.y;
        } else {
            if (cz == (pz ? 255u : 0u)) break;
            cz = pz ? cz + 1u : cz - 1u;
            const float num = planesZ[cz + (pz ? 1 : 0)] - o.z;
            dz = FAST ? tame_quotient(num, d.z, rz) : num / d.z;
        }
    }
    return best;
}

// rays [count][2] float4, excluded [count] (nullptr: none), hits [count] float4.  fastQuotient: the walk's quotient without scaling
// and fix-up for waves whose rays are all tame, under the same guard as wf_trace_kernel.
__global__ __launch_bounds__(256) void rt_query_kernel(const RtDevScene S, const float4 *__restrict__ rays, const uint32_t *__restrict__ excludedIds,
                                                       const uint32_t count, float4 *__restrict__ hits, const uint32_t fastQuotient)
{
    __shared__ float planes[3 * (RT_GRID_DIV + 1)];
    for (int i = threadIdx.x; i < 3 * (RT_GRID_DIV + 1); i += 256) planes[i] = S.boxMin[i];
    __syncthreads();
    const size_t at = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (at >= count) return;
    const float4 a = rays[2 * at], b = rays[2 * at + 1];
    const uint32_t excluded = excludedIds ? excludedIds[at] : RT_NONE;
    const V3 o = xyz(a), d = xyz(b);
    float t, l1 = 0.f, l2 = 0.f;
    uint32_t tri;
    const bool tame = tame_origin(o.x) && tame_origin(o.y) && tame_origin(o.z) && tame_direction(d.x) && tame_direction(d.y) && tame_direction(d.z);
    if (S.planesTame && fastQuotient && __ballot(!tame) == 0ull) tri = query_walk<true>(S, planes, o, d, a.w, b.w, excluded, t, l1, l2);
    else tri = query_walk<false>(S, planes, o, d, a.w, b.w, excluded, t, l1, l2);
    if (tri == RT_NONE) { l1 = 0.f; l2 = 0.f; }
    hits[at] = make_float4(t, __uint_as_float(tri), l1, l2);
}

extern "C" hipError_t rtw_launch_query(const RtDevScene *scene, const void *rays, const uint32_t *excluded, uint32_t count, void *hits,
                                       uint32_t fastQuotient, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_query_kernel, dim3((uint32_t)(((uint64_t)count + 255u) / 256u)), dim3(256), 0, stream, *scene,
                       reinterpret_cast<const float4 *>(rays), excluded, count, reinterpret_cast<float4 *>(hits), fastQuotient);
    return hipGetLastError();
}

// ---- ambient occlusion (rtHipSceneAmbientOcclusion*; include/raytrace_hip.h, "AMBIENT OCCLUSION"; buffers in rt_device.h, RtAoArgs) -------
// Both walks are query_walk, under rt_query_kernel's tame guard: each ray gets exactly the answer rtHipSceneIntersect gives it.
__device__ __forceinline__ uint64_t ao_mix(uint64_t z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// U(c) for base state s0 = mix(seed): the top 24 bits of h(c), exact in fp32
__device__ __forceinline__ float ao_uniform(uint64_t s0, uint64_t c)
{
    return (float)(uint32_t)(ao_mix(s0 + (c + 1ull) * 0x9E3779B97F4A7C15ull) >> 40) * 0x1p-24f;
}
// the image pixel of AO-order index lp (may lie outside the image in a tile at its right or bottom edge): rt_tile_origin + rt_tile_block_xy
// of rt_tile_order.h, which the host's read-backs walk -- in the kernel's own text, because calling them changed its instructions
__device__ __forceinline__ void ao_pixel(const RtDevScene &S, uint32_t lp, uint32_t &gx, uint32_t &gy)
{
    const uint32_t tile = S.tileIds[lp >> 14], q = lp & (RT_TILE_PIXELS - 1u), blk = q >> 6, in = q & 63u;
    gx = (tile % S.tilesX) * RT_TILE + (blk & 15u) * 8u + (in & 7u);
    gy = (tile / S.tilesX) * RT_TILE + (blk >> 4) * 8u + (in >> 3);
}
__device__ __forceinline__ uint32_t ao_walk(const RtDevScene &S, const float *planes, uint32_t fastQuotient, V3 o, V3 d, float tmax, uint32_t excluded,
                                            float &t)
{
    float l1, l2;
    const bool tame = tame_origin(o.x) && tame_origin(o.y) && tame_origin(o.z) && tame_direction(d.x) && tame_direction(d.y) && tame_direction(d.z);
    if (S.planesTame && fastQuotient && __ballot(!tame) == 0ull) return query_walk<true>(S, planes, o, d, 0.f, tmax, excluded, t, l1, l2);
    return query_walk<false>(S, planes, o, d, 0.f, tmax, excluded, t, l1, l2);
}

// One lane per pixel sample: the primary ray, its walk, the hit point and the oriented unit normal.  A sample with something to trace is
// appended to the chunk's hit list (one atomic per wave); a miss or a normal of length 0 adds its R open rays to the pixel at once, so the
// AO kernel's waves hold only rays that are traced.
__global__ __launch_bounds__(256) void rt_ao_primary_kernel(const RtDevScene S, const RtAoArgs A)
{
    __shared__ float planes[3 * (RT_GRID_DIV + 1)];
    for (int i = threadIdx.x; i < 3 * (RT_GRID_DIV + 1); i += 256) planes[i] = S.boxMin[i];
    __syncthreads();
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    if (at >= A.count) return;
    const uint64_t g = A.base + at;
    const uint32_t Sp = A.pixelSamples, lp = (uint32_t)(g / Sp), j = (uint32_t)(g - (uint64_t)lp * Sp);
    uint32_t gx, gy;
    ao_pixel(S, lp, gx, gy);
    if (gx >= S.width || gy >= S.height) return; // (its counter is never read)
    const uint32_t p = gy * S.width + gx;
    float u = 0.5f, v = 0.5f;
    if (Sp > 1u) {
        const uint64_t s0 = ao_mix(A.seed), c = ((uint64_t)p * Sp + j) * (A.raysPerHit + 1u) * 32ull;
        u = ao_uniform(s0, c);
        v = ao_uniform(s0, c + 1u);
    }
    const float fx = (float)gx + u, fy = (float)gy + v;
    const V3 o = mk(S.eye[0], S.eye[1], S.eye[2]);
    const V3 d = mk((S.topLeft[0] + S.lr[0] * fx) + S.tb[0] * fy, (S.topLeft[1] + S.lr[1] * fx) + S.tb[1] * fy,
                    (S.topLeft[2] + S.lr[2] * fx) + S.tb[2] * fy);
    float t;
    const uint32_t tri = ao_walk(S, planes, A.fastQuotient, o, d, RT_INF, RT_NONE, t);
    V3 P = mk(0.f, 0.f, 0.f), n = P;
    bool trace = false;
    if (tri != RT_NONE) {
        P = along(o, t, d);
        const float4 r2 = reinterpret_cast<const float4 *>(S.triRec)[4 * (size_t)tri + 2]; // {ac.z, n = cross(ac, ab)}
        n = mk(r2.y, r2.z, r2.w);
        if (dot3(n, d) > 0.f) n = mk(-n.x, -n.y, -n.z);
        const float m = dot3(n, n);
        if (m > 0.f) {
            const float r = sqrt_rn(m);
            n = mk(n.x / r, n.y / r, n.z / r);
            trace = true;
        }
    }
    const uint32_t slot = wave_append(A.hits, trace);
    if (trace) {
        A.rec[2 * (size_t)slot] = make_float4(P.x, P.y, P.z, __uint_as_float(tri));
        A.rec[2 * (size_t)slot + 1] = make_float4(n.x, n.y, n.z, __uint_as_float(at));
    } else atomicAdd(A.counter + lp, A.raysPerHit);
}

// One lane per AO ray of the chunk's hit list, the R rays of a pixel sample on consecutive lanes (the grid is sized for every sample of
// the chunk hitting; workgroups past the list exit at once).  The unoccluded rays of a wave are counted per pixel with a ballot: each
// pixel's lanes are one run of the wave, its first lane adds the run's popcount to the pixel's counter (integer sums: the result does
// not depend on the order of the atomics, nor on the order of the hit list).
__global__ __launch_bounds__(256) void rt_ao_kernel(const RtDevScene S, const RtAoArgs A)
{
    const uint32_t R = A.raysPerHit, Sp = A.pixelSamples, listed = *A.hits;
    if ((uint64_t)blockIdx.x * 256u >= (uint64_t)listed * R) return;
    __shared__ float planes[3 * (RT_GRID_DIV + 1)];
    for (int i = threadIdx.x; i < 3 * (RT_GRID_DIV + 1); i += 256) planes[i] = S.boxMin[i];
    __syncthreads();
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, s = k / R, r = k - s * R;
    const bool live = s < listed;
    bool open = false;
    uint32_t lp = 0xffffffffu;
    if (live) {
        const float4 a = A.rec[2 * (size_t)s], b = A.rec[2 * (size_t)s + 1];
        const uint64_t g = A.base + __float_as_uint(b.w);
        lp = (uint32_t)(g / Sp);
        const uint32_t j = (uint32_t)(g - (uint64_t)lp * Sp), tri = __float_as_uint(a.w);
        uint32_t gx, gy;
        ao_pixel(S, lp, gx, gy);
        const V3 n = xyz(b);
        const float sg = (n.z >= 0.f) ? 1.f : -1.f, fa = -1.f / (sg + n.z), fb = (n.x * n.y) * fa;
        const V3 t1 = mk(1.f + ((sg * n.x) * n.x) * fa, sg * fb, -(sg * n.x));
        const V3 t2 = mk(fb, sg + (n.y * n.y) * fa, -n.y);
        const uint64_t s0 = ao_mix(A.seed), c = (((uint64_t)(gy * S.width + gx) * Sp + j) * (R + 1u) + 1u + r) * 32ull;
        float xd = 0.f, yd = 0.f, r2 = 0.f;
#pragma unroll 1
        for (uint32_t att = 0; att < 16u; ++att) {
            const float x = 2.f * ao_uniform(s0, c + 2u * att) - 1.f, y = 2.f * ao_uniform(s0, c + 2u * att + 1u) - 1.f;
            const float q = x * x + y * y;
            if (q < 1.f) { xd = x; yd = y; r2 = q; break; }
        }
        const float z = sqrt_rn(1.f - r2);
        const V3 d = mk((xd * t1.x + yd * t2.x) + z * n.x, (xd * t1.y + yd * t2.y) + z * n.y, (xd * t1.z + yd * t2.z) + z * n.z);
        float t;
        open = ao_walk(S, planes, A.fastQuotient, xyz(a), d, A.radius, tri, t) == RT_NONE;
    }
    const uint64_t openMask = __ballot(open);
    const uint32_t lane = __lane_id();
    const uint32_t before = __shfl_up(lp, 1, 64);
    const bool first = live && (lane == 0u || before != lp);
    const uint64_t firsts = __ballot(first);
    if (first) {
        const uint64_t later = firsts & ~((2ull << lane) - 1ull);           // first lanes of the runs after this one
        const uint64_t run = (later ? (later & (0ull - later)) - 1ull : ~0ull) & ~((1ull << lane) - 1ull);
        const uint32_t n = (uint32_t)__popcll(openMask & run);
        if (n) atomicAdd(A.counter + lp, n);
    }
}

// One lane per pixel of the scene's tiles: value = (float)U / (float)(Sp*R) into row-major W x H `out` (rowMajor) or at index lp
// (the host entry point's staging, de-tiled on the host; `out` may then be `counter` itself).
__global__ __launch_bounds__(256) void rt_ao_finish_kernel(const RtDevScene S, const uint32_t *counter, float den, float *out, uint32_t rowMajor)
{
    const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
    if (lp >= S.tileCount * RT_TILE_PIXELS) return;
    uint32_t gx, gy;
    ao_pixel(S, lp, gx, gy);
    if (gx >= S.width || gy >= S.height) return;
    const float v = (float)counter[lp] / den;
    if (rowMajor) out[(size_t)gy * S.width + gx] = v;
    else out[lp] = v;
}

extern "C" hipError_t rtw_launch_ao(const RtDevScene *scene, const RtAoArgs *args, hipStream_t stream)
{
    if (args->count == 0) return hipSuccess;
    const uint64_t rays = (uint64_t)args->count * args->raysPerHit;
    if (rays > (1ull << 31)) return hipErrorInvalidValue; // (the AO kernel's lane index is 32-bit)
    hipLaunchKernelGGL(rt_ao_primary_kernel, dim3((args->count + 255u) / 256u), dim3(256), 0, stream, *scene, *args);
    hipLaunchKernelGGL(rt_ao_kernel, dim3((uint32_t)((rays + 255u) / 256u)), dim3(256), 0, stream, *scene, *args);
    return hipGetLastError();
}

extern "C" hipError_t rtw_launch_ao_finish(const RtDevScene *scene, const uint32_t *counter, uint32_t samplesTimesRays, float *out, uint32_t rowMajor,
                                           hipStream_t stream)
{
    const uint32_t n = scene->tileCount * RT_TILE_PIXELS;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_ao_finish_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, *scene, counter, (float)samplesTimesRays, out, rowMajor);
    return hipGetLastError();
}

// ---- motion vectors (rtHipSceneMotion*; include/raytrace_hip.h, "MOTION VECTORS"; buffers in rt_device.h, RtMotionArgs) -------------------
// One lane per triangle: the rows of its triRec line that hold a, ab, ac become its reference record (16-byte loads and stores).
__global__ __launch_bounds__(256) void rt_motion_mark_kernel(const float4 *__restrict__ triRec, float4 *__restrict__ ref, const uint32_t triangles)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= triangles) return;
    const float4 *src = triRec + 4 * (size_t)i;
    const float4 r0 = src[0], r1 = src[1], r2 = src[2];
    float4 *dst = ref + RT_MOTION_REF_ROWS * (size_t)i;
    dst[0] = r0;
    dst[1] = r1;
    dst[2] = make_float4(r2.x, 0.f, 0.f, 0.f); // (the rest of the row is the normal)
}

// One lane per pixel of the scene's tiles in AO order (a wave is one 8x8 block of the screen): the centre ray, its walk -- query_walk
// under rt_query_kernel's tame guard, the answer rtHipSceneIntersect gives --, one gather of the hit triangle's reference record, the
// projection through the reference camera and up to four stores.
__global__ __launch_bounds__(256) void rt_motion_kernel(const RtDevScene S, const RtMotionArgs A)
{
    __shared__ float planes[3 * (RT_GRID_DIV + 1)];
    for (int i = threadIdx.x; i < 3 * (RT_GRID_DIV + 1); i += 256) planes[i] = S.boxMin[i];
    __syncthreads();
    const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
    if (lp >= S.tileCount * RT_TILE_PIXELS) return;
    uint32_t gx, gy;
    ao_pixel(S, lp, gx, gy);
    if (gx >= S.width || gy >= S.height) return;
    const float fx = (float)gx + 0.5f, fy = (float)gy + 0.5f;
    const V3 o = mk(S.eye[0], S.eye[1], S.eye[2]);
    const V3 d = mk((S.topLeft[0] + S.lr[0] * fx) + S.tb[0] * fy, (S.topLeft[1] + S.lr[1] * fx) + S.tb[1] * fy,
                    (S.topLeft[2] + S.lr[2] * fx) + S.tb[2] * fy);
    float t, l1 = 0.f, l2 = 0.f;
    uint32_t tri;
    const bool tame = tame_origin(o.x) && tame_origin(o.y) && tame_origin(o.z) && tame_direction(d.x) && tame_direction(d.y) && tame_direction(d.z);
    if (S.planesTame && A.fastQuotient && __ballot(!tame) == 0ull) tri = query_walk<true>(S, planes, o, d, 0.f, RT_INF, RT_NONE, t, l1, l2);
    else tri = query_walk<false>(S, planes, o, d, 0.f, RT_INF, RT_NONE, t, l1, l2);
    const bool hit = tri != RT_NONE;
    const V3 E = mk(A.eye[0], A.eye[1], A.eye[2]), TL = mk(A.topLeft[0], A.topLeft[1], A.topLeft[2]);
    const V3 lr = mk(A.lr[0], A.lr[1], A.lr[2]), tb = mk(A.tb[0], A.tb[1], A.tb[2]);
    V3 w = d; // a miss: the background is a point at infinity
    if (hit) {
        const float4 *rec = A.ref + RT_MOTION_REF_ROWS * (size_t)tri;
        const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
        const V3 P = mk((r0.x + l1 * r0.w) + l2 * r1.z, (r0.y + l1 * r1.x) + l2 * r1.w, (r0.z + l1 * r1.y) + l2 * r2.x);
        w = sub3(P, E);
    }
    const V3 n = cross3(lr, tb);
    const float den = dot3(w, n);
    const size_t at = A.rowMajor ? (size_t)gy * S.width + gx : (size_t)lp;
    if (A.motion) {
        const float px = dot3(TL, cross3(w, tb)) / den, py = dot3(TL, cross3(lr, w)) / den;
        A.motion[2 * at] = px - fx; // (two 4-byte stores: the caller's array need not be 8-byte aligned)
        A.motion[2 * at + 1] = py - fy;
    }
    if (A.t) A.t[at] = hit ? t : RT_INF;
    if (A.prevT) A.prevT[at] = hit ? den / dot3(TL, n) : RT_INF;
    if (A.triangle) A.triangle[at] = tri;
}

extern "C" hipError_t rtw_launch_motion_mark(const float *triRec, void *ref, uint32_t triangles, hipStream_t stream)
{
    if (triangles == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_motion_mark_kernel, dim3((triangles + 255u) / 256u), dim3(256), 0, stream, reinterpret_cast<const float4 *>(triRec),
                       reinterpret_cast<float4 *>(ref), triangles);
    return hipGetLastError();
}

extern "C" hipError_t rtw_launch_motion(const RtDevScene *scene, const RtMotionArgs *args, hipStream_t stream)
{
    const uint32_t n = scene->tileCount * RT_TILE_PIXELS;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_motion_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, *scene, *args);
    return hipGetLastError();
}

// ---- ambient occlusion bake (rtHipSceneBakeAmbientOcclusion*; include/raytrace_hip.h, "AMBIENT OCCLUSION BAKE"; buffers in rt_device.h,
// RtBakeArgs) ------------------------------------------------------------------------------------------------------------------------
// The AO rays are the AO block's (ao_mix, ao_uniform, ao_walk): each gets exactly the answer rtHipSceneIntersect gives it.
#define RT_BAKE_BIG_RECT 1024u // texel rectangles larger than this are rasterised by every workgroup of rt_bake_raster_big_kernel
#define RT_BAKE_BIG_BLOCKS 1024u

// The coverage test of texel centre (cu, cv) against UV corners uv[0..5] = uvA, uvB, uvC, and its barycentrics (l1 weighs b, l2 c).
__device__ __forceinline__ bool bake_cover(const float *uv, float cu, float cv, float &l1, float &l2)
{
    const float e1x = uv[2] - uv[0], e1y = uv[3] - uv[1], e2x = uv[4] - uv[0], e2y = uv[5] - uv[1], qx = cu - uv[0], qy = cv - uv[1];
    const float den = e1x * e2y - e1y * e2x;
    l1 = (qx * e2y - qy * e2x) / den;
    l2 = (e1x * qy - e1y * qx) / den;
    return l1 >= 0.f && l2 >= 0.f && l1 + l2 <= 1.f;
}
__device__ __forceinline__ float bake_centre(uint32_t i, uint32_t n) { return ((float)i + 0.5f) / (float)n; }

// The texel rectangle outside which bake_cover provably fails for UV corners uv[0..5]; false if no texel can pass.  A den that is 0 or
// NaN (a NaN UV gives one) covers nothing.  Otherwise the UV bounding box is grown by a bound on the test's rounding (in double):
// with E the largest |e| component, Q = 1 + max|uvA|, u = 2^-24, the computed den is within 8uE^2 of the exact D of the rounded edges,
// and a texel that passes has exact barycentrics within delta = 4(u + 8u(QE + 2E^2)/D) of [0, 1], so its centre lies within 6 delta E
// (+ 4uQ for the centre's own rounding) of the box, plus one texel.  An infinite UV, or D <= 32uE^2 (den may be rounding noise), gets
// the whole map.
__device__ __forceinline__ bool bake_rect(const float *uv, uint32_t W, uint32_t H, uint32_t &x0, uint32_t &x1, uint32_t &y0, uint32_t &y1)
{
    const float e1x = uv[2] - uv[0], e1y = uv[3] - uv[1], e2x = uv[4] - uv[0], e2y = uv[5] - uv[1];
    const float den = e1x * e2y - e1y * e2x;
    if (den == 0.f || den != den) return false;
    x0 = 0; x1 = W - 1; y0 = 0; y1 = H - 1;
    bool finite = fabsf(den) < RT_INF;
    for (int k = 0; k < 6; ++k) finite = finite && fabsf(uv[k]) < RT_INF;
    if (!finite) return true;
    const double u = 0x1p-24, E = fmax(fmax(fabs((double)e1x), fabs((double)e1y)), fmax(fabs((double)e2x), fabs((double)e2y)));
    const double D = fabs((double)e1x * (double)e2y - (double)e1y * (double)e2x);
    if (!(D > 32.0 * u * E * E)) return true;
    const double Q = 1.0 + fmax(fabs((double)uv[0]), fabs((double)uv[1]));
    const double delta = 4.0 * (u + 8.0 * u * (Q * E + 2.0 * E * E) / D), m = 6.0 * delta * E + 4.0 * u * Q;
    const double umin = fmin(fmin((double)uv[0], (double)uv[2]), (double)uv[4]) - m, umax = fmax(fmax((double)uv[0], (double)uv[2]), (double)uv[4]) + m;
    const double vmin = fmin(fmin((double)uv[1], (double)uv[3]), (double)uv[5]) - m, vmax = fmax(fmax((double)uv[1], (double)uv[3]), (double)uv[5]) + m;
    const double lx = floor(umin * W - 0.5) - 1.0, hx = ceil(umax * W - 0.5) + 1.0, ly = floor(vmin * H - 0.5) - 1.0, hy = ceil(vmax * H - 0.5) + 1.0;
    if (hx < 0.0 || hy < 0.0 || lx > (double)(W - 1) || ly > (double)(H - 1)) return false;
    x0 = lx > 0.0 ? (uint32_t)lx : 0u; y0 = ly > 0.0 ? (uint32_t)ly : 0u;
    x1 = hx < (double)(W - 1) ? (uint32_t)hx : W - 1; y1 = hy < (double)(H - 1) ? (uint32_t)hy : H - 1;
    return true;
}
__device__ __forceinline__ void bake_texel(const float *uv, uint32_t W, uint32_t H, uint32_t x, uint32_t y, uint32_t tri, uint32_t *win)
{
    float l1, l2;
    if (bake_cover(uv, bake_centre(x, W), bake_centre(y, H), l1, l2)) atomicMin(win + (size_t)y * W + x, tri);
}

// One thread per triangle of the range A.first .. A.first + A.count - 1 that passes the material filter: the texels of its rectangle,
// or -- a rectangle of more than RT_BAKE_BIG_RECT texels -- an entry of the big list.  atomicMin: the smallest covering id wins
// whatever the order.
__global__ __launch_bounds__(256) void rt_bake_raster_kernel(const RtDevScene S, const RtBakeArgs A)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.count) return;
    const uint32_t tri = A.first + i;
    const float *sh = S.triShade + RT_TRI_SHADE_WORDS * (size_t)tri;
    if (A.matchMaterial && __float_as_int(sh[21]) != A.material) return;
    float uv[6];
    for (int k = 0; k < 6; ++k) uv[k] = sh[15 + k];
    uint32_t x0, x1, y0, y1;
    if (!bake_rect(uv, A.width, A.height, x0, x1, y0, y1)) return;
    if ((uint64_t)(x1 - x0 + 1) * (uint64_t)(y1 - y0 + 1) > RT_BAKE_BIG_RECT) {
        A.bigList[atomicAdd(A.bigCount, 1u)] = tri;
        return;
    }
    for (uint32_t y = y0; y <= y1; ++y)
        for (uint32_t x = x0; x <= x1; ++x) bake_texel(uv, A.width, A.height, x, y, tri, A.win);
}

// The big list's triangles in turn, the texels of each one's rectangle dealt over every thread of the launch (one quad can cover the
// whole map: a workgroup per triangle would leave the chip idle).
__global__ __launch_bounds__(256) void rt_bake_raster_big_kernel(const RtDevScene S, const RtBakeArgs A)
{
    const uint32_t n = *A.bigCount;
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t b = 0; b < n; ++b) {
        const uint32_t tri = A.bigList[b];
        const float *sh = S.triShade + RT_TRI_SHADE_WORDS * (size_t)tri;
        float uv[6];
        for (int k = 0; k < 6; ++k) uv[k] = sh[15 + k];
        uint32_t x0, x1, y0, y1;
        bake_rect(uv, A.width, A.height, x0, x1, y0, y1); // (true: it was listed)
        const uint32_t w = x1 - x0 + 1, area = w * (y1 - y0 + 1); // (at most W*H <= 2^26)
        for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < area; k += stride) {
            const uint32_t ky = k / w;
            bake_texel(uv, A.width, A.height, x0 + (k - ky * w), y0 + ky, tri, A.win);
        }
    }
}

// One lane per texel of the chunk: its winner, the surface point and the oriented unit normal.  An uncovered texel's counter is set to
// 0 and a zero-normal texel's to R here; the others' to 0, and they are appended to the hit list (one atomic per wave).
__global__ __launch_bounds__(256) void rt_bake_points_kernel(const RtDevScene S, const RtBakeArgs A)
{
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    if (at >= A.count) return;
    const uint32_t t = (uint32_t)(A.base + at), tri = A.win[t];
    V3 P = mk(0.f, 0.f, 0.f), n = P;
    bool trace = false;
    uint32_t open = 0;
    if (tri != RT_NONE) {
        const float *sh = S.triShade + RT_TRI_SHADE_WORDS * (size_t)tri;
        float uv[6];
        for (int k = 0; k < 6; ++k) uv[k] = sh[15 + k];
        const uint32_t y = t / A.width, x = t - y * A.width;
        float l1, l2;
        bake_cover(uv, bake_centre(x, A.width), bake_centre(y, A.height), l1, l2); // (true: it won)
        const float4 *rec = reinterpret_cast<const float4 *>(S.triRec) + 4 * (size_t)tri;
        const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2]; // a.xyz ab.x | ab.yz ac.xy | ac.z n.xyz
        P = mk((r0.x + l1 * r0.w) + l2 * r1.z, (r0.y + l1 * r1.x) + l2 * r1.w, (r0.z + l1 * r1.y) + l2 * r2.x);
        n = mk(r2.y, r2.z, r2.w);
        const V3 s = mk((sh[6] + sh[9]) + sh[12], (sh[7] + sh[10]) + sh[13], (sh[8] + sh[11]) + sh[14]);
        if (dot3(n, s) < 0.f) n = mk(-n.x, -n.y, -n.z);
        const float m = dot3(n, n);
        if (m > 0.f) {
            const float r = sqrt_rn(m);
            n = mk(n.x / r, n.y / r, n.z / r);
            trace = true;
        } else open = A.raysPerTexel;
    }
    A.counter[t] = open;
    const uint32_t slot = wave_append(A.hits, trace);
    if (trace) {
        A.rec[2 * (size_t)slot] = make_float4(P.x, P.y, P.z, __uint_as_float(tri));
        A.rec[2 * (size_t)slot + 1] = make_float4(n.x, n.y, n.z, __uint_as_float(at));
    }
}

// One lane per AO ray of the chunk's hit list, a texel's R rays on consecutive lanes; open rays are counted per texel with
// rt_ao_kernel's ballot and one atomic per run of a wave.
__global__ __launch_bounds__(256) void rt_bake_ao_kernel(const RtDevScene S, const RtBakeArgs A)
{
    const uint32_t R = A.raysPerTexel, listed = *A.hits;
    if ((uint64_t)blockIdx.x * 256u >= (uint64_t)listed * R) return;
    __shared__ float planes[3 * (RT_GRID_DIV + 1)];
    for (int i = threadIdx.x; i < 3 * (RT_GRID_DIV + 1); i += 256) planes[i] = S.boxMin[i];
    __syncthreads();
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, s = k / R, r = k - s * R;
    const bool live = s < listed;
    bool open = false;
    uint32_t t = 0xffffffffu;
    if (live) {
        const float4 a = A.rec[2 * (size_t)s], b = A.rec[2 * (size_t)s + 1];
        t = (uint32_t)(A.base + __float_as_uint(b.w));
        const uint32_t tri = __float_as_uint(a.w);
        const V3 n = xyz(b);
        const float sg = (n.z >= 0.f) ? 1.f : -1.f, fa = -1.f / (sg + n.z), fb = (n.x * n.y) * fa;
        const V3 t1 = mk(1.f + ((sg * n.x) * n.x) * fa, sg * fb, -(sg * n.x));
        const V3 t2 = mk(fb, sg + (n.y * n.y) * fa, -n.y);
        const uint64_t s0 = ao_mix(A.seed), c = ((uint64_t)t * (R + 1u) + 1u + r) * 32ull;
        float xd = 0.f, yd = 0.f, r2 = 0.f;
#pragma unroll 1
        for (uint32_t att = 0; att < 16u; ++att) {
            const float x = 2.f * ao_uniform(s0, c + 2u * att) - 1.f, y = 2.f * ao_uniform(s0, c + 2u * att + 1u) - 1.f;
            const float q = x * x + y * y;
            if (q < 1.f) { xd = x; yd = y; r2 = q; break; }
        }
        const float z = sqrt_rn(1.f - r2);
        const V3 d = mk((xd * t1.x + yd * t2.x) + z * n.x, (xd * t1.y + yd * t2.y) + z * n.y, (xd * t1.z + yd * t2.z) + z * n.z);
        float th;
        open = ao_walk(S, planes, A.fastQuotient, xyz(a), d, A.radius, tri, th) == RT_NONE;
    }
    const uint64_t openMask = __ballot(open);
    const uint32_t lane = __lane_id();
    const uint32_t before = __shfl_up(t, 1, 64);
    const bool first = live && (lane == 0u || before != t);
    const uint64_t firsts = __ballot(first);
    if (first) {
        const uint64_t later = firsts & ~((2ull << lane) - 1ull);
        const uint64_t run = (later ? (later & (0ull - later)) - 1ull : ~0ull) & ~((1ull << lane) - 1ull);
        const uint32_t cnt = (uint32_t)__popcll(openMask & run);
        if (cnt) atomicAdd(A.counter + t, cnt);
    }
}

// One lane per texel: the value (float)U / (float)R, or `fill` where nothing covers the texel (0, or -1 = invalid when dilation
// follows), into `out` (which may be `counter` itself), and the winner into `tri` (if not null).
__global__ __launch_bounds__(256) void rt_bake_finish_kernel(uint32_t texels, const uint32_t *win, const uint32_t *counter, float rays, float fill,
                                                             float *out, uint32_t *tri)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= texels) return;
    const uint32_t w = win[t];
    const float v = (w == RT_NONE) ? fill : (float)counter[t] / rays;
    out[t] = v;
    if (tri) tri[t] = w;
}

// One dilation pass (Jacobi): values >= 0 are valid, -1 is not.  `last`: a texel still invalid is written as 0.
__global__ __launch_bounds__(256) void rt_bake_dilate_kernel(uint32_t W, uint32_t H, const float *src, float *dst, uint32_t last)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= W * H) return;
    const float v = src[t];
    if (v >= 0.f) { dst[t] = v; return; }
    const int y = (int)(t / W), x = (int)(t - (uint32_t)y * W);
    float sum = 0.f;
    uint32_t k = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int nx = x + dx, ny = y + dy;
            if ((dx == 0 && dy == 0) || nx < 0 || ny < 0 || nx >= (int)W || ny >= (int)H) continue;
            const float w = src[(size_t)ny * W + nx];
            if (w >= 0.f) { sum += w; ++k; }
        }
    dst[t] = k ? sum / (float)k : (last ? 0.f : -1.f);
}

extern "C" hipError_t rtw_launch_bake_raster(const RtDevScene *scene, const RtBakeArgs *args, hipStream_t stream)
{
    if (args->count == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_bake_raster_kernel, dim3((args->count + 255u) / 256u), dim3(256), 0, stream, *scene, *args);
    hipLaunchKernelGGL(rt_bake_raster_big_kernel, dim3(RT_BAKE_BIG_BLOCKS), dim3(256), 0, stream, *scene, *args);
    return hipGetLastError();
}

extern "C" hipError_t rtw_launch_bake_points(const RtDevScene *scene, const RtBakeArgs *args, hipStream_t stream)
{
    if (args->count == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_bake_points_kernel, dim3((args->count + 255u) / 256u), dim3(256), 0, stream, *scene, *args);
    return hipGetLastError();
}

extern "C" hipError_t rtw_launch_bake_ao(const RtDevScene *scene, const RtBakeArgs *args, hipStream_t stream)
{
    if (args->count == 0) return hipSuccess;
    const uint64_t rays = (uint64_t)args->count * args->raysPerTexel;
    if (rays > (1ull << 31)) return hipErrorInvalidValue; // (the AO kernel's lane index is 32-bit)
    hipLaunchKernelGGL(rt_bake_ao_kernel, dim3((uint32_t)((rays + 255u) / 256u)), dim3(256), 0, stream, *scene, *args);
    return hipGetLastError();
}

extern "C" hipError_t rtw_launch_bake_finish(uint32_t texels, const uint32_t *win, const uint32_t *counter, uint32_t rays, float fill, float *out,
                                             uint32_t *tri, hipStream_t stream)
{
    hipLaunchKernelGGL(rt_bake_finish_kernel, dim3((texels + 255u) / 256u), dim3(256), 0, stream, texels, win, counter, (float)rays, fill, out, tri);
    return hipGetLastError();
}

extern "C" hipError_t rtw_launch_bake_dilate(uint32_t W, uint32_t H, const float *src, float *dst, uint32_t last, hipStream_t stream)
{
    hipLaunchKernelGGL(rt_bake_dilate_kernel, dim3((W * H + 255u) / 256u), dim3(256), 0, stream, W, H, src, dst, last);
    return hipGetLastError();
}
