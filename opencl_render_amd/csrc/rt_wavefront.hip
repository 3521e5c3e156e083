// rt_wavefront.hip -- the hot path as a staged wavefront pipeline for gfx950 (MI355X).
//
// Why: in a one-thread-per-pixel kernel only the pixels whose primary ray hit something (28 % in the headline scene)
// do any secondary work, and their grid walks differ in length by 10x, so a wave averages 4-5 busy lanes of 64
// (rocprofv3 PMC, profiles/r01_v1_*).  Here every ray that needs the grid becomes a queue entry.
//
//   wf_primary  one thread per (pixel, sample): jittered camera ray + per-pixel candidate list (raytrace_opencl.c:470-528).
//               Hits become PATHS: dense id from a wave-aggregated atomic, state written to HBM (rt_device.h).
//   wf_logic    one thread per waiting path: resumes the per-sample state machine of raytrace_opencl.c:532-724 where it
//               stopped, runs it until the next grid ray (shadow ray :611, or a queued ray :530) and appends that ray
//               to the next round's queue as a self-contained TRACE ENTRY (the ray + its DDA start state; a long ray of
//               a small round is cut into exact segments); paths with an empty ring retire their colour.
//   wf_scatter  big rounds only: orders the entries by predicted walk length (the logic kernel counted the classes).
//   wf_trace    one entry per lane: walks the non-uniform grid (:324-401) in blind phases, tests the occupied cells it
//               passed wave-cooperatively; a hit is published as (segment, pair) in hitKey and resolved by wf_logic.
//   wf_accum    frames with several samples: per pixel, samples in order, truncated saturating u16 accumulate into the
//               tile buffer (:726-741); a one-sample frame's pixels are written by wf_primary / wf_logic directly (unless the
//               frame continues a sample window's sequence from the tile buffer: rt_device.h, directStore).
//
// Per path everything happens in the reference's order (RNG draws, ring FIFO, light loop), and paths never interact,
// so the planes are bit-identical to the single-launch kernel (rt_kernels.hip) and to the oracle.
//
// This file holds the kernels a frame launches and their launch wrappers, nothing else.  The helpers it shares with the passes traced
// against a resident scene outside the frame (rt_scene_passes.hip: mattes, ray queries, ambient occlusion, motion vectors, the bake) are
// in rt_wf_shared.h, the trace entries among them.
#include "rt_devfuncs.h"
#include "rt_launch.h"
#include "rt_path_state.h"
#include "rt_ray_clip.h"
#include "rt_wf_shared.h"

namespace {

enum { WS_RAY = 0, WS_SHADOW = 1 };
static_assert(RT_PATH_RING_SLOTS == RT_RING, "rt_path_state.h addresses the ring allocation");

} // namespace

// ---- stage 1: primary rays ---------------------------------------------------------------------------------------
// grid = (tileCount*64, samplesInBatch); workgroup = 16x16 pixel patch, wave = 8x8 quadrant.
// PASSES (rtHipScenePasses): the primary hit also feeds the render passes, laid out like tileBuf ([slot][RT_PASS_*][128*128] 32-bit
// words): every hitting sample adds 1 to its pixel's hit counter (zeroed by the host before the frame's first batch; a one-sample frame
// stores it instead), and sample 1 writes the eye-to-hit distance and the triangle.  Without PASSES the body is the plain primary stage.
template <bool PASSES>
__device__ __forceinline__ void wf_primary_body(const RtDevScene &S, const RtWavefront &W, uint32_t *passBuf)
{
    const uint32_t slot = blockIdx.x >> 6, patch = blockIdx.x & 63;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t lx = (patch & 7) * RT_PATCH + (wave & 1) * 8 + (lane & 7);
    const uint32_t ly = (patch >> 3) * RT_PATCH + (wave >> 1) * 8 + (lane >> 3);
    const uint32_t tile = S.tileIds[slot];
    const uint32_t gx = (tile % S.tilesX) * RT_TILE + lx;
    const uint32_t gy = (tile / S.tilesX) * RT_TILE + ly;
    const uint32_t sb = blockIdx.y;
    const bool valid = gx < S.width && gy < S.height;

    uint32_t hit_tri = RT_NONE;
    float hit_t = 0.f, hit_l1 = 0.f, hit_l2 = 0.f;
    uint64_t rng = 0;
    V3 dir = mk(0.f, 0.f, 0.f);
    const uint32_t localPixel = slot * RT_TILE_PIXELS + ly * RT_TILE + lx;
    const uint32_t outSlot = localPixel * W.samplesInBatch + sb;
    if (valid) {
        const uint32_t pixel = gy * S.width + gx;
        rng = (uint64_t)pixel * (uint64_t)S.seedStride + (uint64_t)(S.sampleFirst + W.sampleBase + sb + 1); // :481
        const V3 lr = ld3(S.lr), tb = ld3(S.tb);
        dir = ld3(S.topLeft);
        float k = (float)gx + rand01(rng); // LR jitter first, then TB (:496-503)
        dir.x += lr.x * k; dir.y += lr.y * k; dir.z += lr.z * k;
        k = (float)gy + rand01(rng);
        dir.x += tb.x * k; dir.y += tb.y * k; dir.z += tb.z * k;
        hit_tri = camera_scan(S, localPixel, ld3(S.eye), dir, 0.f, RT_INF, RT_NONE, hit_t, hit_l1, hit_l2);
        if (hit_tri == RT_NONE) {
            if (S.directStore == 1u) store_single_sample(S, localPixel, mk(0.f, 0.f, 0.f));
            else W.sampleOut[outSlot] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const bool born = valid && hit_tri != RT_NONE;
    // workgroups are dealt to the shards round-robin: concurrently running groups append to different counters
    const uint32_t shard = (blockIdx.x + blockIdx.y * gridDim.x) % RT_WF_SHARDS;
    // the path id doubles as the index of its round-0 queue entry: the primary hit plays the answered request
    const uint32_t a = shard * W.shardCap + wave_append(&W.ctl[RT_WF_CTL_COUNTS + shard], born);
    if (born) {
        W.rng[a] = rng;
        W.meta[a] = make_uint4(outSlot, localPixel, 0u | (1u << 4) | ((uint32_t)WS_RAY << 8), hit_tri);
        // ring slot 0 = the camera ray (:490-508).  Only its direction is stored: round 0 of wf_logic_kernel, the slot's one
        // reader, knows the rest (origin = eye, weight 1, maxBounces 12, fromCamera), as it knows that nothing is collected yet.
        // Where the slot lives depends on the scene's path class (rt_path_state.h; the same choice in every lane): in the opaque-diffuse
        // class the directions are a dense plane, a wave's store is whole lines.
        const size_t dirAt = S.pathClass == RT_PATH_CLASS_OPAQUE_DIFFUSE ? rt_path_class_quad(W.capacity, a, 0u, 1u) : rt_path_ring_quad(a, 0u, 1u);
        W.ring[dirAt] = pack4(dir, __uint_as_float(RT_NONE));
        W.res[a] = make_uint4(hit_tri, __float_as_uint(hit_t), __float_as_uint(hit_l1), __float_as_uint(hit_l2));
    }
    if (PASSES && valid) {
        uint32_t *pass = passBuf + (size_t)slot * RT_PASS_WORDS * RT_TILE_PIXELS + ly * RT_TILE + lx;
        // one sample per pixel: this thread is the pixel's only sample and stores its count (no zeroing, no atomic); otherwise the
        // samples of a pixel sit in different workgroups and batches and add into the counter the host zeroed
        if (S.sampleCount == 1u) pass[RT_PASS_HITS * RT_TILE_PIXELS] = born ? 1u : 0u;
        else if (born) __hip_atomic_fetch_add(pass + RT_PASS_HITS * RT_TILE_PIXELS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (result unused: no-return atomic)
        if (W.sampleBase + sb == 0u) {
            const float depth = born ? hit_t * sqrt_rn(dot3(dir, dir)) : RT_INF; // dir is not normalised: t * |dir| is the distance
            pass[RT_PASS_DEPTH * RT_TILE_PIXELS] = __float_as_uint(depth);
            pass[RT_PASS_TRIANGLE * RT_TILE_PIXELS] = hit_tri;
        }
    }
}

__global__ __launch_bounds__(256) void wf_primary_kernel(const RtDevScene S, const RtWavefront W) { wf_primary_body<false>(S, W, nullptr); }
__global__ __launch_bounds__(256) void wf_primary_passes_kernel(const RtDevScene S, const RtWavefront W, uint32_t *passBuf)
{
    wf_primary_body<true>(S, W, passBuf);
}

// ---- surface passes: shading normal and albedo, summed over a pixel's samples (RT_HIP_PASS_NORMAL | RT_HIP_PASS_ALBEDO) -------------
// grid = tileCount*64; workgroup = 16x16 pixel patch, wave = 8x8 quadrant, as wf_primary -- but ONE thread per pixel, which walks the
// batch's samples in order.  Each sample's primary hit is derived again (generator, direction and camera scan of wf_primary_body) and
// shaded as SHADE_BEGIN shades it (raytrace_opencl.c:548, :554): n = shading_normal, albedo = the colour channel's texel, both zero on a
// miss or for material -1.  They are added into the pixel's six f32 sums (rt_device.h, surfBuf).  The batch with sampleBase 0 starts
// from +0 instead of reading the buffer; later batches of the frame follow on the same stream, so every sum is taken in sample order
// s = 1..S without atomics.  (The samples of a pixel sit in different workgroups of wf_primary and in different paths of the logic
// kernel: summing them in order there would need per-sample staging.)
__global__ __launch_bounds__(256) void wf_surface_passes_kernel(const RtDevScene S, const RtWavefront W, float *surfBuf)
{
    __shared__ Shared sh; // as every kernel that shades sets it up
    for (int i = threadIdx.x; i < 3 * (RT_GRID_DIV + 1); i += 256) (&sh.planes[0][0])[i] = S.boxMin[i];
    sh.unit255[threadIdx.x] = (float)threadIdx.x / 255.f;
    __syncthreads();
    const uint32_t slot = blockIdx.x >> 6, patch = blockIdx.x & 63;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t lx = (patch & 7) * RT_PATCH + (wave & 1) * 8 + (lane & 7);
    const uint32_t ly = (patch >> 3) * RT_PATCH + (wave >> 1) * 8 + (lane >> 3);
    const uint32_t tile = S.tileIds[slot];
    const uint32_t gx = (tile % S.tilesX) * RT_TILE + lx;
    const uint32_t gy = (tile / S.tilesX) * RT_TILE + ly;
    if (gx >= S.width || gy >= S.height) return;

    const uint32_t localPixel = slot * RT_TILE_PIXELS + ly * RT_TILE + lx;
    float *sums = surfBuf + (size_t)slot * RT_SURF_WORDS * RT_TILE_PIXELS + ly * RT_TILE + lx;
    float acc[RT_SURF_WORDS];
#pragma unroll
    for (int k = 0; k < RT_SURF_WORDS; ++k) acc[k] = W.sampleBase == 0u ? 0.f : sums[k * RT_TILE_PIXELS];
    const uint32_t pixel = gy * S.width + gx;
    const V3 eye = ld3(S.eye), lr = ld3(S.lr), tb = ld3(S.tb), topLeft = ld3(S.topLeft);
    Counters cn; // unused (COUNT=false)
    for (uint32_t sb = 0; sb < W.samplesInBatch; ++sb) {
        uint64_t rng = (uint64_t)pixel * (uint64_t)S.seedStride + (uint64_t)(S.sampleFirst + W.sampleBase + sb + 1); // :481
        V3 dir = topLeft;
        float k = (float)gx + rand01(rng); // LR jitter first, then TB (:496-503)
        dir.x += lr.x * k; dir.y += lr.y * k; dir.z += lr.z * k;
        k = (float)gy + rand01(rng);
        dir.x += tb.x * k; dir.y += tb.y * k; dir.z += tb.z * k;
        float hit_t = 0.f, hit_l1 = 0.f, hit_l2 = 0.f;
        const uint32_t hit_tri = camera_scan(S, localPixel, eye, dir, 0.f, RT_INF, RT_NONE, hit_t, hit_l1, hit_l2);
        V3 n = mk(0.f, 0.f, 0.f), albedo = mk(0.f, 0.f, 0.f);
        if (hit_tri != RT_NONE) {
            const float *shade = S.triShade + RT_TRI_SHADE_WORDS * (size_t)hit_tri;
            const int m = __float_as_int(shade[21]);
            const V3 where = along(eye, hit_t, dir);
            MatRec mat;
            mat.desc[0] = mat.desc[1] = mat.desc[2] = mat.desc[3] = mat.desc[4] = 0u; mat.m = m;
            if (0 <= m) mat = load_mat(S, m);
            n = shading_normal<false>(S, sh, where, eye, dir, hit_tri, hit_l1, hit_l2, shade, m, cn, &mat);
            uint32_t raw;
            if (0 <= m && mat.desc[CH_COLOR]) albedo = texel_rec<false>(S, sh, mat, CH_COLOR, shade + 15, hit_l1, hit_l2, raw, cn);
        }
        acc[RT_SURF_NORMAL + 0] += n.x; acc[RT_SURF_NORMAL + 1] += n.y; acc[RT_SURF_NORMAL + 2] += n.z;
        acc[RT_SURF_ALBEDO + 0] += albedo.x; acc[RT_SURF_ALBEDO + 1] += albedo.y; acc[RT_SURF_ALBEDO + 2] += albedo.z;
    }
#pragma unroll
    for (int k = 0; k < RT_SURF_WORDS; ++k) sums[k * RT_TILE_PIXELS] = acc[k];
}

// ---- stage 2: per-path state machine ---------------------------------------------------------------------------------
// Two rays of a path may be in flight at once: the current hit's shadow ray (or the ring ray being traced) and a
// LOOK-AHEAD trace of the next ring entry.  That is legal because nothing about a spawned ray depends on the shadow
// rays of the hit that spawned it -- only the ORDER in which colour is accumulated does, and that order is kept: the
// machine below is still strictly sequential per path, it merely finds some answers already there.  To know the spawned
// rays before the light loop has run, a hit's spawns are computed when it is shaded: the generator is moved past the light
// loop's draws first (their count depends on the generator alone, :30-45), the diffuse direction is drawn (:671), and the
// lights are set up later from the draws made on the way (light 0) or from a second cursor into the stream (rngL, further
// lights).  The draw order of raytrace_opencl.c is unchanged, so are the results.
//
// What a hit keeps while its shadow rays are out is folded to two vectors: `out` already holds the luminance term (:642-644,
// nothing touches `out` between a hit's shading and its :647-651), P is the product (1-out)*weight*(1-transparency)*texture
// of :649-651 in the reference's order, and of face[2] only the entry :647 will pick is tracked.
#ifndef RT_WF_LOGIC_WAVES
#define RT_WF_LOGIC_WAVES 3
#endif
#ifndef RT_WF_LOGIC_WAVES_FIRST
#define RT_WF_LOGIC_WAVES_FIRST 3
#endif
#ifndef RT_WF_LOGIC_WAVES_FIRST_ORDERED
#define RT_WF_LOGIC_WAVES_FIRST_ORDERED 3
#endif
#ifndef RT_WF_LOGIC_WAVES_LEAN_FIRST
#define RT_WF_LOGIC_WAVES_LEAN_FIRST 4
#endif
#ifndef RT_WF_LOGIC_WAVES_LEAN
#define RT_WF_LOGIC_WAVES_LEAN 4
#endif
#define RT_WF_LIGHTS_LDS 64
#ifdef RT_DIAG_LOGIC // diagnostic build: where a wave is at which time, round RT_DIAG_LOGIC (no waits added; scripts/diag_logic.py)
#define DG(i) dg[i] = diag_stamp()
#else
#define DG(i)
#endif
// PC_LIGHT_ACCUM (:628-636) and PC_SHADE_END (:647-651) of the opaque-diffuse class for wf_answer_kernel: the operations of the class path's
// light_accum and shade_end (rt_wf_logic_body.h) in their order; lc = the light's colour and half-attenuation distance.  (Those stay written
// out where they are: calling these from there moved instructions in the round-0 kernels, which this split leaves as they were.)
__device__ __forceinline__ void class_light_accum(V3 &face, float ndl, bool front, float lmax, float4 lc, V3 atten)
{
    const float mag = __builtin_fabsf(ndl);
    const float x = lmax / lc.w;
    const float e = mag * half_falloff(x);
    if ((0.f <= ndl) == front) {
        face.x += (1.f - face.x) * atten.x * e * lc.x;
        face.y += (1.f - face.y) * atten.y * e * lc.y;
        face.z += (1.f - face.z) * atten.z * e * lc.z;
    }
}
__device__ __forceinline__ void class_shade_end(V3 &out, V3 P, V3 face)
{
    out.x += P.x * face.x;
    out.y += P.y * face.y;
    out.z += P.z * face.z;
}

// For the launch plan: a round's rays and its longest queue slice, as the logic kernel logs them (rt_wf_logic_body.h), for wf_answer_kernel.
// One whole workgroup adds up the RT_WF_QSHARDS queue lengths.
__device__ __forceinline__ void log_round_rays(const RtWavefront &W, const uint32_t *ctlIn, uint32_t round, uint32_t lane, uint32_t wave)
{
    __shared__ uint32_t sumWave[4], maxWave[4];
    static_assert(RT_WF_QSHARDS == 512, "two queue lengths per thread");
    const uint32_t c0 = ctlIn[RT_WF_CTL_COUNTS + threadIdx.x], c1 = ctlIn[RT_WF_CTL_COUNTS + 256 + threadIdx.x];
    uint32_t n = c0 + c1, m = max(c0, c1);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { n += __shfl_xor(n, off, 64); m = max(m, (uint32_t)__shfl_xor((int)m, off, 64)); }
    if (lane == 0) { sumWave[wave] = n; maxWave[wave] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t *log = reinterpret_cast<uint32_t *>(W.roundLog + round);
        log[0] = sumWave[0] + sumWave[1] + sumWave[2] + sumWave[3];
        log[1] = max(max(maxWave[0], maxWave[1]), max(maxWave[2], maxWave[3]));
    }
}

// What shading a hit reads of its triangle, fetched in one batch from ONE 128-byte line: the shading row's 24 packed floats and its copy
// of the first vertex (rt_device.h, triShade: quad 6 = triRec quad 0).
struct TriRow { float v[24]; float4 a; uint32_t tri; };
__device__ __forceinline__ void load_tri_row(const RtDevScene &S, uint32_t tri, TriRow &row)
{
    const float4 *sp = reinterpret_cast<const float4 *>(S.triShade + RT_TRI_SHADE_WORDS * (size_t)tri);
    const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3], s4 = sp[4], s5 = sp[5];
    row.a = sp[6];
    row.v[0] = s0.x; row.v[1] = s0.y; row.v[2] = s0.z; row.v[3] = s0.w; row.v[4] = s1.x; row.v[5] = s1.y; row.v[6] = s1.z; row.v[7] = s1.w;
    row.v[8] = s2.x; row.v[9] = s2.y; row.v[10] = s2.z; row.v[11] = s2.w; row.v[12] = s3.x; row.v[13] = s3.y; row.v[14] = s3.z; row.v[15] = s3.w;
    row.v[16] = s4.x; row.v[17] = s4.y; row.v[18] = s4.z; row.v[19] = s4.w; row.v[20] = s5.x; row.v[21] = s5.y; row.v[22] = s5.z; row.v[23] = s5.w;
    row.tri = tri;
}
// Where a later round's hit reads vertex a: quad 6 of the triangle's own row (the line its other shading words come from, not triRec).  The
// address is made from the triangle on its own, as the record's address was: derived from the row pointer, the load joined the row's other
// loads and the ordered later-round kernels spilled more registers.
__device__ __forceinline__ const float4 *tri_row_a(const RtDevScene &S, uint32_t tri)
{
    asm volatile("" : "+v"(tri));
    return reinterpret_cast<const float4 *>(S.triShade + RT_TRI_SHADE_WORDS * (size_t)tri) + 6;
}

// FIRST = round 0: every entry is a primary hit (stage, ring positions and the colour so far are known), a path's id is its queue index.
// ORDERED = the round this launch spawns is an ordered one (next.ordered): its entries are planned and classed here; the other
// instantiation carries none of that code (its registers are the state machine's).
// slicesIn = queue slices per kind of THIS round (what logic(round - 1) was told), next = how the round this launch spawns is laid out.
// LEAN = the scene is in the opaque-diffuse path class (RtDevScene::pathClass, rt_api.cpp): the path is written out as its fixed shape
// instead of the general state machine below, in fewer registers.
// SHADE = the dense shade pass of a split round (class only, rounds >= 1; wf_shade_kernel): one lane per entry of the round's shade list
// (wf_answer_kernel, below) instead of per queue entry.  An entry is a path whose bounce ray hit something; the answer kernel has folded
// what came before (the shadow answer) into the stored `out` and left the rest of the state alone, so the lane takes the class path up at
// "a ray's answer" with the listed key.  The housekeeping is the answer kernel's; this pass logs the list's length.
// The kernel's body is in rt_wf_logic_body.h: wf_shade_kernel (below) is the same text with SHADE on, and a kernel whose body is a function
// shared through a call compiled to other instructions than the one that holds it.
template <bool FIRST, bool ORDERED, bool LEAN>
__global__ __launch_bounds__(256, LEAN ? (FIRST ? RT_WF_LOGIC_WAVES_LEAN_FIRST : RT_WF_LOGIC_WAVES_LEAN)
                                       : (FIRST ? (ORDERED ? RT_WF_LOGIC_WAVES_FIRST_ORDERED : RT_WF_LOGIC_WAVES_FIRST) : RT_WF_LOGIC_WAVES)) void wf_logic_kernel(const RtDevScene S, const RtWavefront W, const uint32_t round,
                                                                                                             const uint32_t slicesIn, const RtRoundMode next)
{
    constexpr bool SHADE = false;
    const RtShadeList L{ nullptr, nullptr }; // (named in SHADE branches only)
#include "rt_wf_logic_body.h"
}

// ---- stage 2, split (opaque-diffuse class with look-ahead, rounds >= 1): answers streamed, bounce hits shaded densely ----------------
// Of such a round's paths one in nine has anything to shade -- its bounce ray hit something.  The others read two answers, fold the
// shadow answer into `out` and store their pixel: a stream, for which the logic kernel's registers (4 waves per SIMD) and its chain of
// dependent loads are not needed.  So the round is two launches.  wf_answer_kernel, one lane per main entry in the logic kernel's
// addressing, does what needs no shading, with the logic kernel's operations in its order:
//   a shadow answer:  atten = 1, times zero when the ray was answered, light_accum, shade_end; then the next ring entry -- none: the pixel
//                     is stored; the bounce, whose look-ahead answer is a miss: the ring is empty, the pixel is stored;
//   a ray's answer (the bounce became the main ray because the camera hit's shadow ray was dead): a miss stores the pixel.
// A path whose bounce answer is a hit is appended to the round's shade list (RtShadeList) with the winning key; of its state only `out`
// is rewritten.  wf_shade_kernel (wf_logic_body<.., SHADE>) then runs the class code from the hit on with one lane per listed path.
// The in-stream housekeeping of the round (control words two rounds ahead, round log) is done here.  shadeFollows = 0: the host's plan
// says nothing will be listed and no shade pass is launched -- a wave that lists a path all the same raises RT_WF_ERR_GRID.
#ifndef RT_WF_ANSWER_WAVES
#define RT_WF_ANSWER_WAVES 8
#endif
__global__ __launch_bounds__(256, RT_WF_ANSWER_WAVES) void wf_answer_kernel(const RtDevScene S, const RtWavefront W, const uint32_t round, const uint32_t slicesIn,
                                                                            const RtShadeList L, const uint32_t shadeFollows)
{
    const uint32_t in = round & 1;
    const uint32_t *ctlIn = W.ctl + (round % 3) * RT_WF_CTL_WORDS;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t waveId = (blockIdx.x * 256 + threadIdx.x) >> 6, waves = (gridDim.x * 256) >> 6;
    {
        const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
        if (gid < RT_WF_CTL_WORDS) W.ctl[((round + 2) % 3) * RT_WF_CTL_WORDS + gid] = 0u;
        if (gid < RT_WF_SHARDS) L.count[((round + 2) % 3) * RT_WF_SHARDS + gid] = 0u;
    }
    if (blockIdx.x == gridDim.x - 1 && round < RT_WF_ROUND_LOG) log_round_rays(W, ctlIn, round, lane, wave);
    const uint32_t shard = __builtin_amdgcn_readfirstlane(waveId % slicesIn);
    const uint32_t total = __builtin_amdgcn_readfirstlane(ctlIn[RT_WF_CTL_COUNTS + shard]);
    const uint32_t sliceCapIn = W.capacity / slicesIn;
    uint32_t *listCount = L.count + (round % 3) * RT_WF_SHARDS + shard;
    const float4 lc = S.lightCount != 0u ? make_float4(S.lightCol[0], S.lightCol[1], S.lightCol[2], S.lightHalfAtt[0]) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t localChunk = __builtin_amdgcn_readfirstlane(waveId / slicesIn); localChunk * 64 < total; localChunk += waves / slicesIn) {
        const uint32_t local = localChunk * 64 + lane;
        const uint32_t q = shard * sliceCapIn + local;
        bool list = false, odd = false;
        uint32_t a = 0;
        unsigned long long listKey = ~0ull;
        if (local < total) {
            const uint2 who = W.pathOf[in][q];
            a = who.x;
            const unsigned long long key = W.hitKey[in][q];
            unsigned long long laKey = ~0ull;
            if (who.y != 0xffffffffu) laKey = W.hitKey[in][who.y];
            const uint4 meta = W.meta[a];
            const float4 oc = W.outc[a]; // xyz: the colour so far; w: the far end of the shadow ray the path is parked on (rt_wf_logic_body.h)
            V3 out = xyz(oc);
            int head = (int)(meta.z & 15u);
            const int tail = (int)((meta.z >> 4) & 15u);
            const uint32_t stage = (meta.z >> 8) & 1u, laState = (meta.z >> 10) & 3u;
            const int laIndex = (int)((meta.z >> 12) & 15u);
            if (laState == 2u) laKey = W.laKey[a]; // (an answer kept from an earlier round)
            bool finished = false;
            if (stage == WS_SHADOW) { // PC_SHADOW_RESULT (:612-626) of light 0
                const float4 sp = W.shP[a];
                const float lmax = oc.w;
                const V3 zero = mk(0.f, 0.f, 0.f);
                // (the parked face entry is always SHADE_BEGIN's 0.1, and `front` is a bit of the flags word: rt_wf_logic_body.h)
                V3 face = mk(0.1f, 0.1f, 0.1f), atten = mk(1.f, 1.f, 1.f);
                if (key != ~0ull) { atten.x *= zero.x; atten.y *= zero.y; atten.z *= zero.z; }
                class_light_accum(face, sp.w, (meta.z & RT_WF_META_CLASS_FRONT) != 0u, lmax, lc, atten);
                class_shade_end(out, xyz(sp), face);
                head = (head + 1) % RT_RING; // PC_NEXT_RAY (:509)
                if (head == tail) finished = true;
                else if (laState != 0u && laIndex == head) { // the bounce, traced ahead of time
                    if (laKey != ~0ull) { list = true; listKey = laKey; W.outc[a] = pack4(out, 0.f); }
                    else if ((head + 1) % RT_RING == tail) finished = true; // (a bounce spawns nothing: the ring is empty)
                    else odd = true;
                } else odd = true;
            } else if (laState != 0u) odd = true;
            else if (key != ~0ull) { list = true; listKey = key; } // the bounce as the main ray: `out` is as it was
            else if ((head + 1) % RT_RING == tail) finished = true;
            else odd = true;
            if (finished) {
                if (S.directStore == 1u) store_single_sample(S, meta.y, out);
                else W.sampleOut[meta.x] = pack4(out, 0.f);
            }
        }
        if (__ballot(odd) != 0ull && lane == 0u) atomicOr(W.hostStatus + RT_WF_STATUS_ERROR, RT_WF_ERR_SPLIT);
        if (!shadeFollows && __ballot(list) != 0ull && lane == 0u) atomicOr(W.hostStatus + RT_WF_STATUS_ERROR, RT_WF_ERR_GRID);
        const uint32_t at = wave_append(listCount, list);
        if (list) L.list[shard * sliceCapIn + at] = make_uint4(a, (uint32_t)listKey, (uint32_t)(listKey >> 32), 0u);
    }
}

template <bool ORDERED>
__global__ __launch_bounds__(256, RT_WF_LOGIC_WAVES_LEAN) void wf_shade_kernel(const RtDevScene S, const RtWavefront W, const uint32_t round, const uint32_t slicesIn,
                                                                              const RtRoundMode next, const RtShadeList L)
{
    constexpr bool FIRST = false, LEAN = true, SHADE = true;
#include "rt_wf_logic_body.h"
}

// ---- stage 2b: an ordered round's entries, longest predicted walk first ------------------------------------------------------
// Queue slice s of a round (s < slices: main entries, s >= slices: look-ahead entries): where it starts and how long it is.
__device__ __forceinline__ uint32_t slice_first(const RtWavefront &W, uint32_t slices, uint32_t s)
{
    const uint32_t kind = (s >= slices) ? 1u : 0u, shard = s - kind * slices;
    return kind * W.capacity + shard * (W.capacity / slices);
}
__device__ __forceinline__ uint32_t slice_count(const uint32_t *ctl, uint32_t slices, uint32_t s)
{
    const uint32_t kind = (s >= slices) ? 1u : 0u, shard = s - kind * slices;
    return ctl[RT_WF_CTL_COUNTS + kind * RT_WF_SHARDS + shard];
}

// Work items: the used 256-entry blocks of the queue slices (region A: segment 0 of every ray, in queue order), then the blocks of
// region B (further segments, densely packed); a fixed grid takes them in turn.  The logic kernel left a rank inside its (class,
// copy) and the class itself per entry; the classes' sizes are in the round's histogram.
// The launch also RECORDS what it worked out -- every cell's first position and size, the total, the round's layout -- in the round's
// placement table (rt_device.h, RT_WF_PLACE_*; rounds 1 .. RT_WF_PLACE_ROUNDS): the frames of an unchanged scene fill the cells alike, so a
// later planned frame's logic kernel places the entries itself (RT_ROUND_DIRECT) and this kernel is not launched for the round.
__global__ __launch_bounds__(256) void wf_scatter_kernel(const RtWavefront W, const uint32_t round, const uint32_t slices, const uint32_t segLen)
{
    __shared__ uint32_t base[RT_WF_SORT_BINS * RT_WF_SORT_COPIES];
    __shared__ uint32_t longWave[4];
    uint32_t *ctl = W.ctl + (round % 3) * RT_WF_CTL_WORDS;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        const uint32_t c0 = ctl[RT_WF_CTL_COUNTS + threadIdx.x], c1 = ctl[RT_WF_CTL_COUNTS + 256 + threadIdx.x];
        uint32_t m = max(c0, c1);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
        if (lane == 0) longWave[wave] = m;
    }
    if (threadIdx.x < RT_WF_SORT_BINS) { // one wave: exclusive prefix over (bin, copy), bin-major
        uint32_t sum = 0;
        for (int c = 0; c < RT_WF_SORT_COPIES; ++c) sum += ctl[RT_WF_CTL_HIST + c * RT_WF_SORT_BINS + threadIdx.x];
        uint32_t incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, 64);
            if ((int)threadIdx.x >= off) incl += up;
        }
        uint32_t at = incl - sum;
        for (int c = 0; c < RT_WF_SORT_COPIES; ++c) { base[threadIdx.x * RT_WF_SORT_COPIES + c] = at; at += ctl[RT_WF_CTL_HIST + c * RT_WF_SORT_BINS + threadIdx.x]; }
        if (blockIdx.x == 0 && threadIdx.x == RT_WF_SORT_BINS - 1) {
            ctl[RT_WF_CTL_TOTAL] = incl; // all entries are in [0, total)
            if (round >= 1u && round <= RT_WF_PLACE_ROUNDS) W.ctl[RT_WF_PLACE_AT(round) + RT_WF_PLACE_TOTAL] = incl;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && round >= 1u && round <= RT_WF_PLACE_ROUNDS) {
        uint32_t *place = W.ctl + RT_WF_PLACE_AT(round);
        for (uint32_t i = threadIdx.x; i < RT_WF_PLACE_CELLS; i += 256) // i = bin * copies + copy
            reinterpret_cast<uint2 *>(place)[i] = make_uint2(base[i], ctl[RT_WF_CTL_HIST + (i % RT_WF_SORT_COPIES) * RT_WF_SORT_BINS + i / RT_WF_SORT_COPIES]);
        if (threadIdx.x == 0) { place[RT_WF_PLACE_SLICES] = slices; place[RT_WF_PLACE_SEGLEN] = segLen; }
    }
    const uint32_t usedBlocks = (max(max(longWave[0], longWave[1]), max(longWave[2], longWave[3])) + 255u) >> 8;
    const uint32_t itemsA = 2u * slices * usedBlocks;
    const uint32_t extra = min(ctl[RT_WF_CTL_EXTRA], W.extraCap); // the count runs past the capacity when region B filled up (wf_logic_kernel)
    const uint32_t itemsB = (extra + 255u) >> 8;
    for (uint32_t item = blockIdx.x; item < itemsA + itemsB; item += gridDim.x) {
        uint32_t mine = 0;
        bool valid = false;
        if (item < itemsA) {
            const uint32_t sl = item % (2u * slices);
            const uint32_t local = (item / (2u * slices)) * 256 + threadIdx.x;
            valid = local < slice_count(ctl, slices, sl);
            mine = slice_first(W, slices, sl) + local;
        } else {
            const uint32_t local = (item - itemsA) * 256 + threadIdx.x;
            valid = local < extra;
            mine = 2u * W.capacity + local;
        }
        if (valid) {
            // only the ORDER is written: the trace kernel gathers its 64-byte entries through it
            const uint32_t rank = W.sortRank[mine];
            if (rank != 0xffffffffu) { // not an unused reservation
                const uint32_t tag = W.sortTag[mine]; // bin | copy << 6
                W.sortedIdx[base[(tag & 63u) * RT_WF_SORT_COPIES + (tag >> 6)] + rank] = mine;
            }
        }
    }
}

__global__ void wf_place_skew_kernel(const RtWavefront W, const uint32_t round)
{
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    uint2 *cell = reinterpret_cast<uint2 *>(W.ctl + RT_WF_PLACE_AT(round));
    for (uint32_t i = 0; i + 1u < RT_WF_PLACE_CELLS; ++i)
        if (cell[i].y != 0u) { cell[i].y -= 1u; cell[i + 1].x -= 1u; cell[i + 1].y += 1u; return; }
}

// ---- stage 3: grid traversal (raytrace_opencl.c:324-401) ------------------------------------------------------------------
// One sorted entry per lane.  WALK, THEN TEST: where a ray walks does not depend on what it hits -- only where it stops does:
// the reference resets its running maximum in every cell (:366) and ends at the first cell that produced any hit (:380).  So a
// lane walks freely and only RECORDS the occupied cells it passes in a small per-lane list in LDS; when lists fill up, or
// nobody can walk any further, the wave tests the recorded cells cooperatively (the items of all lanes are flattened, a lane
// takes one cell per round whoever recorded it, ray data comes from the owner lane by ds_bpermute); the first cell with a hit
// ends the ray, a ray without a hit carries on walking from where it stands.  Results do not depend on where a walk is cut.
// Waves of a workgroup never synchronise after the plane table is staged.  The walk is VALU-issue bound (a round's waves outnumber the
// wave slots), so the step is built to cost as few vector instructions as possible:
//   * per-ray constants of the step are precomputed per axis (signed cell increment, plane-table offset, exit coordinate);
//   * the occupancy word of a 4x4x4 block is found at byte offset 3*(cell & 0xFCFCFC) of a sparsely indexed copy of the
//     block table (two instructions instead of six: rt_device.h, gridBlockSparse), its bit with one multiply (bit-gather) and one bit-field extract;
//   * an occupied cell is recorded as its DENSE id (rank of its block, which arrives with the occupancy word, + occupied cells below
//     it): the index the test phase gathers the cell's record by.  Working it out in the test phase, where all 64 lanes have an item,
//     costs fewer instructions (6 of 64 lanes are on an occupied cell in the walk) but a second dependent gather of the block word
//     per item: one round trip per item instead of two was worth 5 % of the kernel (round 3).
#ifndef RT_WF_LEAN_WAVES
#define RT_WF_LEAN_WAVES 5
#endif
#ifndef RT_WF_LEAN_LIST
#define RT_WF_LEAN_LIST 16            // per-lane LDS slots: recorded occupied cells + the cells logged by the current blind phase
#endif
#ifndef RT_WF_BLIND
#define RT_WF_BLIND 5                 // cell visits per blind phase (4-7 are within 0.5 % of each other, 8 and 10 are 1 % and 3 % slower)
#endif
#ifndef RT_WF_MORE_ITEMS
#define RT_WF_MORE_ITEMS 128          // per-wave list of further candidates (beyond a cell's first) awaiting their test
#endif
#ifndef RT_WF_LEAN_STALL
#define RT_WF_LEAN_STALL 64           // test once (lanes without room for another phase) x this exceeds the lanes still walking
#endif
#define RT_WF_GROUP_RAYS 128          // rays a workgroup of wf_trace_kernel<false> plans at most (RtRoundMode::groupRays): its first two waves
template <bool ORDERED>
__global__ __launch_bounds__(256, RT_WF_LEAN_WAVES) void wf_trace_kernel(const RtDevScene S, const RtWavefront W, const uint32_t round, const RtRoundMode mode)
{
    __shared__ float planes[3 * (RT_GRID_DIV + 1)];
    __shared__ uint32_t cellList[RT_WF_LEAN_LIST][256];                 // [entry][thread] packed cells cx | cy<<8 | cz<<16
    __shared__ uint8_t ownerOf[4][RT_WF_LEAN_LIST * 64];                // per wave: lane that recorded item c
    __shared__ unsigned long long keyOf[4][64];                         // per wave and lane: (cell order, t, pair index) of the earliest hit
    __shared__ uint32_t moreOf[4][2][RT_WF_MORE_ITEMS];                 // per wave: further candidates under test {owner | cell order << 6}, {pair}
    __shared__ uint32_t moreCount[4];
    static_assert(RT_WF_LEAN_LIST <= 16, "hit_key: 4 bits of cell order");
    // <false> only: the workgroup's rays as planned by its first lanes {o,tmin} {d,tmax} {excluded, q, start cell, end cell} {dx,dy,dz,te},
    // the first segment of every ray in the workgroup's list of segments, and whose ray a segment is.  They live in the cell
    // lists' memory: the planning is over before the walk begins, and 5 KB more of LDS would cost the kernel its fifth workgroup per CU.
    static_assert(sizeof(float4) * 4 * RT_WF_GROUP_RAYS + 4 * (RT_WF_GROUP_RAYS + 1) + 256 <= sizeof(cellList) && RT_WF_GROUP_RAYS == 128, "the plan tables fit the cell lists; waves 0 and 1 plan");
    float4 *rayO = reinterpret_cast<float4 *>(&cellList[0][0]), *rayD = rayO + RT_WF_GROUP_RAYS, *rayT = rayD + RT_WF_GROUP_RAYS;
    uint4 *rayX = reinterpret_cast<uint4 *>(rayT + RT_WF_GROUP_RAYS);
    uint32_t *segFirst = reinterpret_cast<uint32_t *>(rayX + RT_WF_GROUP_RAYS);
    uint8_t *segOwner = reinterpret_cast<uint8_t *>(segFirst + RT_WF_GROUP_RAYS + 1); // [256]: a workgroup's segments are one per lane at most

    // Which rays this workgroup takes.
    //   ordered round:  256 entries, block i of the sorted order, through sortedIdx -- the hardware dispatches workgroups in order, so
    //                   the longest walks start first and a free slot always gets the longest work left;
    //   other rounds:   mode.groupRays rays of one queue slice, slice-minor (piece b of every slice before piece b + 1 of any: slices
    //                   fill evenly); the workgroup plans them, cuts them, and deals the segments to its lanes 256 at a time.
    // A planned frame's grid is sized from the same frame's previous rendering (rt_api.cpp); should it be too small the host is told
    // and renders the frame again with the worst-case grid (a loop that strides over the rest measured 4 % slower).
    const uint32_t *ctl = W.ctl + (round % 3) * RT_WF_CTL_WORDS;
    const uint32_t par = round & 1;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#ifdef RT_DIAG_STAMPS
    const unsigned long long dgK0 = diag_stamp();
#endif
    uint32_t mine = 0, segments = 0;
    bool active = false;
    if (ORDERED) {
        // (a round placed directly, RT_ROUND_DIRECT: no scatter launch wrote the total or an order -- the total is the placement table's and
        // the entries stand in sorted order, so the workgroup's 256 are one 16 KB block and nothing is looked up on the way to them)
        const bool direct = (mode.ordered & RT_ROUND_DIRECT) != 0u;
        const uint32_t total = direct ? W.ctl[RT_WF_PLACE_AT(round) + RT_WF_PLACE_TOTAL] : ctl[RT_WF_CTL_TOTAL];
        const uint32_t blocksUsed = (total + 255u) >> 8;
        if (direct && blockIdx.x + 1u == blocksUsed && wave == 0u) {
            // No cell took more than its run (the logic kernel's guard), so the cells are exactly full if the round made as many entries as
            // the table places; fewer, and some position still holds an entry of an earlier frame: the frame is invalid
            uint32_t n = 0;
#pragma unroll
            for (int i = 0; i < RT_WF_QSHARDS / 64; ++i) n += ctl[RT_WF_CTL_COUNTS + i * 64 + lane];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, 64);
            if (lane == 0u && n != total) atomicOr(W.hostStatus + RT_WF_STATUS_ERROR, RT_WF_ERR_GRID);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (round < RT_WF_ROUND_LOG) reinterpret_cast<uint32_t *>(W.roundLog + round)[2] = min(ctl[RT_WF_CTL_EXTRA], W.extraCap);
            if (blocksUsed > gridDim.x) atomicOr(W.hostStatus + RT_WF_STATUS_ERROR, RT_WF_ERR_GRID);
        }
        if (blockIdx.x >= blocksUsed) return; // whole workgroup beyond the entries
        const uint32_t at = blockIdx.x * 256 + threadIdx.x;
        active = at < total;
        if (active) mine = direct ? at : W.sortedIdx[at];
        for (int i = threadIdx.x; i < 3 * (RT_GRID_DIV + 1); i += 256) planes[i] = S.boxMin[i];
        __syncthreads();
    } else {
        // Workgroup i takes piece `row` of queue slice `sl`, pieces numbered through the slices in turn -- found by adding up the
        // slices' piece counts, not by arithmetic on i: a grid striped "slice = i % slices" puts the workgroups of the empty slices (a
        // late round has no look-ahead rays) at a fixed stride, the hardware deals workgroups to XCDs and CUs round-robin, and half
        // of the CUs ended up with all of the round's work (measured: 64 -> 130 us).
        const uint32_t group = min(mode.groupRays, (uint32_t)RT_WF_GROUP_RAYS);
        __shared__ uint32_t pieceWave[4], pieceAt[2];
        uint32_t sl = 0, row = 0, count = 0;
        {
            static_assert(2 * RT_WF_SHARDS == 512, "two queue slices per thread");
            const uint32_t s0 = threadIdx.x, s1 = 256u + threadIdx.x;
            const uint32_t c0 = s0 < 2u * mode.slices ? slice_count(ctl, mode.slices, s0) : 0u, c1 = s1 < 2u * mode.slices ? slice_count(ctl, mode.slices, s1) : 0u;
            const uint32_t p0 = (c0 + group - 1u) / group, p1 = (c1 + group - 1u) / group;
            // pieces before slice s0 (slices 0..255 first, then 256..511): scan of p0 over the workgroup, then of p1 behind it
            uint32_t i0 = p0, i1 = p1;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t u0 = __shfl_up(i0, off, 64), u1 = __shfl_up(i1, off, 64);
                if ((int)lane >= off) { i0 += u0; i1 += u1; }
            }
            if (lane == 63) { pieceWave[wave] = i0; }
            __syncthreads();
            uint32_t before0 = 0, all0 = 0;
            for (uint32_t w = 0; w < 4; ++w) { if (w < wave) before0 += pieceWave[w]; all0 += pieceWave[w]; }
            __syncthreads();
            if (lane == 63) { pieceWave[wave] = i1; }
            __syncthreads();
            uint32_t before1 = all0, all1 = all0;
            for (uint32_t w = 0; w < 4; ++w) { if (w < wave) before1 += pieceWave[w]; all1 += pieceWave[w]; }
            const uint32_t first0 = before0 + i0 - p0, first1 = before1 + i1 - p1;
            if (blockIdx.x == 0 && threadIdx.x == 0 && all1 > gridDim.x) atomicOr(W.hostStatus + RT_WF_STATUS_ERROR, RT_WF_ERR_GRID);
            if (blockIdx.x >= all1) return; // whole workgroup beyond the round's pieces
            if (first0 <= blockIdx.x && blockIdx.x < first0 + p0) { pieceAt[0] = s0; pieceAt[1] = blockIdx.x - first0; }
            if (first1 <= blockIdx.x && blockIdx.x < first1 + p1) { pieceAt[0] = s1; pieceAt[1] = blockIdx.x - first1; }
            __syncthreads();
            sl = pieceAt[0]; row = pieceAt[1];
            count = slice_count(ctl, mode.slices, sl);
        }
        for (int i = threadIdx.x; i < 3 * (RT_GRID_DIV + 1); i += 256) planes[i] = S.boxMin[i];
        __syncthreads();
        // The first lanes plan the workgroup's rays: every lane busy, where the logic kernel would have planned one ray in ten lanes.
        // A workgroup takes every rowsUsed-th ray of its slice, not a stretch of it: neighbours in the queue are neighbours in the
        // image, their rays are alike, and a stretch of long rays made one workgroup's list of segments two or three times the
        // others' (the round lasts as long as its slowest workgroup: 64 -> 160 us).
        const uint32_t rowsUsed = (count + group - 1u) / group;
        __shared__ uint32_t planWave[2];
        uint32_t n = 0;
        const uint32_t local = row + threadIdx.x * rowsUsed;
        const bool planner = threadIdx.x < group && local < count; // (group <= 128: waves 0 and 1)
        if (planner) {
            const uint32_t q = slice_first(W, mode.slices, sl) + local;
            const uint4 *e = W.ent[par] + 4 * (size_t)q;
            const uint32_t excl = reinterpret_cast<const uint32_t *>(e)[3];
            const float tmin = __uint_as_float(reinterpret_cast<const uint32_t *>(e)[7]);
            const uint4 c2 = e[2], c3 = e[3];
            const V3 o = mk(__uint_as_float(c2.x), __uint_as_float(c2.y), __uint_as_float(c2.z)), d = mk(__uint_as_float(c3.x), __uint_as_float(c3.y), __uint_as_float(c3.z));
            const float tmax = __uint_as_float(c2.w);
            const EntryPlan plan = plan_ray(planes, o, d, tmin, tmax, false, 0u, nullptr, nullptr, S.boxMin + RT_CLIP_AT);
            n = segments_of(plan, d, tmax, mode.segLen);
            rayO[threadIdx.x] = pack4(o, tmin); rayD[threadIdx.x] = pack4(d, tmax);
            rayX[threadIdx.x] = make_uint4(excl, q, plan.start.cell, plan.endCell);
            rayT[threadIdx.x] = make_float4(plan.start.dx, plan.start.dy, plan.start.dz, plan.te);
        }
        // one pass of 256 lanes must do: a workgroup whose rays would make more segments cuts them coarser
        if (wave < 2) {
            uint32_t sum = n;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
            if (lane == 0) planWave[wave] = sum;
        }
        __syncthreads();
        const uint32_t all = planWave[0] + planWave[1];
        __syncthreads();
        if (wave < 2) {
            // (every ray keeps one segment at least: what is left of the 256 lanes is shared out in proportion)
            const uint32_t raysHere = min(group, (count - row + rowsUsed - 1u) / rowsUsed);
            if (all > 256u && n > 1u) n = max(1u, n * (256u - raysHere) / all);
            uint32_t incl = n;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t up = __shfl_up(incl, off, 64);
                if ((int)lane >= off) incl += up;
            }
            if (lane == 63) planWave[wave] = incl;
            n = incl - n; // (this lane's first segment, inside its wave)
        }
        __syncthreads();
        if (wave < 2) {
            const uint32_t nextFirst = (uint32_t)__shfl_down((int)n, 1, 64); // (by every lane: a shuffle reads nothing from a lane that sits it out)
            const uint32_t first = n + (wave == 1 ? planWave[0] : 0u), mineN = (lane == 63 ? planWave[wave] : nextFirst) - n;
            segFirst[threadIdx.x] = first;
            if (threadIdx.x == 127) segFirst[128] = planWave[0] + planWave[1];
            for (uint32_t k = 0; k < mineN; ++k) segOwner[first + k] = (uint8_t)threadIdx.x;
        }
        __syncthreads();
        segments = segFirst[128];
    }

    // an ordered round: the workgroup's 256 entries; any other round: the workgroup's segments (256 at most, see above)
    for (uint32_t pass = 0; pass < 1u; ++pass) {
    uint32_t q = 0, excluded = RT_NONE, cell = 0, endCell = 0xffffffffu, seg = 0;
    V3 o = mk(0, 0, 0), d = mk(1, 1, 1);
    float tmin = 0.f, tmax = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    if (ORDERED) {
        if (active) {
            const uint4 *e = W.ent[par] + 4 * (size_t)mine;
            const uint4 c0 = e[0], c1 = e[1], c2 = e[2], c3 = e[3];
            q = c0.x; cell = c0.y & 0xffffffu; endCell = c0.z; excluded = c0.w;
            dx = __uint_as_float(c1.x); dy = __uint_as_float(c1.y); dz = __uint_as_float(c1.z); tmin = __uint_as_float(c1.w);
            o = mk(__uint_as_float(c2.x), __uint_as_float(c2.y), __uint_as_float(c2.z)); tmax = __uint_as_float(c2.w);
            d = mk(__uint_as_float(c3.x), __uint_as_float(c3.y), __uint_as_float(c3.z));
            seg = c3.w >> 24;
            // (a position that this frame did not fill -- a round placed directly whose table was not the frame's, flagged where it is found
            // out -- holds whatever was there: the answer goes to hitKey[q], so a q that is no queue slot is not walked)
            active = q < 2u * W.capacity;
        }
    } else {
        const uint32_t i = threadIdx.x;
        active = i < segments;
        if (active) {
            const uint32_t owner = segOwner[i];
            const uint32_t k = i - segFirst[owner], n = segFirst[owner + 1] - segFirst[owner];
            const float4 ro = rayO[owner], rd = rayD[owner], rt = rayT[owner];
            const uint4 rx = rayX[owner];
            o = xyz(ro); tmin = ro.w; d = xyz(rd); tmax = rd.w; excluded = rx.x; q = rx.y; seg = k;
            // segment k goes from the walk's state at tau_k (tau_0: the ray's own start) to the start cell of segment k + 1
            const float ta = fminf(rt.x, fminf(rt.y, rt.z)), te = rt.w;
            float tau;
            cell = rx.z; dx = rt.x; dy = rt.y; dz = rt.z;
            if (k > 0u) {
                if (cut_at(ta, te, k, n, tau)) {
                    // (counting the crossings with T <= tau from the ray's start cell: the state does not depend on where counting begins)
                    const uint32_t nx = axis_state_at(planes, rx.z & 255u, o.x, d.x, tau, dx);
                    const uint32_t ny = axis_state_at(planes + (RT_GRID_DIV + 1), (rx.z >> 8) & 255u, o.y, d.y, tau, dy);
                    const uint32_t nz = axis_state_at(planes + 2 * (RT_GRID_DIV + 1), rx.z >> 16, o.z, d.z, tau, dz);
                    cell = nx | (ny << 8) | (nz << 16);
                } else active = false; // rounding left no room for this cut: the segment before runs to the ray's end
            }
            endCell = rx.w;
            if (active && k + 1u < n && cut_at(ta, te, k + 1u, n, tau)) {
                float unused;
                const uint32_t nx = axis_state_at(planes, rx.z & 255u, o.x, d.x, tau, unused);
                const uint32_t ny = axis_state_at(planes + (RT_GRID_DIV + 1), (rx.z >> 8) & 255u, o.y, d.y, tau, unused);
                const uint32_t nz = axis_state_at(planes + 2 * (RT_GRID_DIV + 1), rx.z >> 16, o.z, d.z, tau, unused);
                endCell = nx | (ny << 8) | (nz << 16);
            }
        }
        __syncthreads(); // the plan tables become the cell lists
    }
    const bool fastWave = S.planesTame && W.fastQuotient && __ballot(active && !(tame_origin(o.x) && tame_origin(o.y) && tame_origin(o.z) &&
                                                                               tame_direction(d.x) && tame_direction(d.y) && tame_direction(d.z))) == 0ull;
    // per-axis step constants (:387-398): direction of travel is fixed per ray
    const bool px = (0.f <= d.x), py = (0.f <= d.y), pz = (0.f <= d.z);
    const uint32_t stepX = px ? 1u : (uint32_t)-1, stepY = py ? (1u << 8) : (uint32_t)-(1 << 8), stepZ = pz ? (1u << 16) : (uint32_t)-(1 << 16);
    // byte offset into `planes` of the plane that bounds the NEW cell ahead, counted from the OLD cell's coordinate c (which the exit test
    // has just extracted): the new cell is c +- 1 and its far plane c + 2 going up, c - 1 going down -> 4*(axisBase + (positive ? 2 : -1)),
    // in wrapping 32-bit arithmetic (c >= 1 when going down: c == 0 ended the walk)
    const uint32_t offX = 4u * (px ? 2u : (uint32_t)-1), offY = 4u * ((RT_GRID_DIV + 1) + (py ? 2u : (uint32_t)-1)),
                   offZ = 4u * (2 * (RT_GRID_DIV + 1) + (pz ? 2u : (uint32_t)-1));
    const char *__restrict__ blockTable = reinterpret_cast<const char *>(S.gridBlockSparse);
    const char *planeBytes = reinterpret_cast<const char *>(planes);

    uint32_t wordKey = 0xffffffffu, wordLo = 0, wordHi = 0, wordRank = 0; // occupancy word + rank of the last block looked up (key = cell & 0xFCFCFC)
    uint32_t listed = 0;
    bool walkEnded = !active;
    uint32_t spins = 0;
#ifdef RT_DIAG_STAMPS
    unsigned long long dgWalk = 0, dgTest = 0, dgWalkIters = 0, dgBatches = 0, dgSteps = 0, dgItems = 0;
    const unsigned long long dgStart = diag_stamp();
#endif

#pragma unroll 1
    for (;;) {
        // ---- walk: BLIND phases of RT_WF_BLIND cell visits (pure DDA stepping, every visited cell logged in LDS), each
        // followed by ONE batched look-up of the logged cells' occupancy words.  The look-ups of a phase are independent
        // loads, so a wave waits for memory once per phase instead of once per visit.
#ifdef RT_DIAG_STAMPS
        const unsigned long long dgW0 = diag_stamp();
#endif
#pragma unroll 1
        for (;;) {
            const bool canWalk = !walkEnded && listed + RT_WF_BLIND <= RT_WF_LEAN_LIST;
            const unsigned long long walkers = __ballot(canWalk);
            if (walkers == 0ull) break;
            const int stalled = __popcll(__ballot(!walkEnded && !canWalk));
            if (stalled * RT_WF_LEAN_STALL > __popcll(walkers)) break;
            if (++spins > W.spinLimit) break; // cannot happen (a ray makes at most 766 visits); keeps a logic error from hanging the GPU
#ifdef RT_DIAG_STAMPS
            dgWalkIters++;
#endif
            uint32_t logged = 0;
            // The quotient (plane - o) / d is the correctly rounded one, as the compiler expands it: v_div_scale x2, v_rcp, two
            // refinements of the reciprocal, q0 = n*r, two corrections, v_div_fmas, v_div_fixup.  When the exponents of n and d
            // are tame (tame_ray below) the scale instructions return their operands, v_div_fmas is a plain fma and the fix-up
            // returns its input: what is left is q0 = n*r1, e1 = fma(-d,q0,n), q1 = fma(e1,r1,q0), e2 = fma(-d,q1,n),
            // q2 = fma(e2,r1,q1) with r1 = the refined reciprocal, which depends on the axis only -- the same operations on the
            // same operands, bit for bit, in 5 issue slots instead of 14 (v_rcp_f32 is quarter rate).  A wave takes this path
            // when all of its rays are tame; the reciprocals live in registers only while the wave walks.
#define RT_WALK_STEP(FAST)                                                                                                          \
                if (canWalk && !walkEnded) {                                                                                        \
                    cellList[listed + u][threadIdx.x] = cell; /* (a lane that walks step u has walked every step before it: logged == u) */ \
                    ++logged;                                                                                                       \
                    /* axis choice (:387-398): x only if strictly smallest, else y if smaller than z, else z */                     \
                    const bool sxm = (dx < dy) & (dx < dz);                                                                         \
                    const bool sym = !sxm & (dy < dz);                                                                              \
                    const uint32_t shift = sxm ? 0u : (sym ? 8u : 16u);                                                             \
                    const uint32_t stepSel = sxm ? stepX : (sym ? stepY : stepZ);                                                   \
                    const uint32_t coord = (cell >> shift) & 255u;                                                                  \
                    /* the end cell ends the walk after it has been visited (:380-381); so does a step that would leave the grid  */ \
                    /* (:389,:393,:397): coordinate 255 going up, 0 going down.  ONE condition, one branch: nested, the compiler   */ \
                    /* carried "cell is the end cell" through three register moves per step                                         */ \
                    const bool done = (cell == endCell) | (coord == (((int32_t)stepSel > 0) ? 255u : 0u));                          \
                    if (!done) {                                                                                                    \
                        cell += stepSel;                                                                                            \
                        const uint32_t off = sxm ? offX : (sym ? offY : offZ);                                                      \
                        const float plane = *reinterpret_cast<const float *>(planeBytes + (uint32_t)((coord << 2) + off));          \
                        const float dd = sxm ? d.x : (sym ? d.y : d.z);                                                             \
                        const float oo = sxm ? o.x : (sym ? o.y : o.z);                                                             \
                        float nd;                                                                                                   \
                        if (FAST) {                                                                                                 \
                            const float rr = sxm ? rx : (sym ? ry : rz);                                                            \
                            nd = tame_quotient(plane - oo, dd, rr);                                                                 \
                        } else nd = (plane - oo) / dd;                                                                              \
                        dx = sxm ? nd : dx; dy = sym ? nd : dy; dz = (sxm | sym) ? dz : nd;                                         \
                    }                                                                                                               \
                    walkEnded = done;                                                                                               \
                }
            if (fastWave) {
                const float rx = refined_rcp(d.x), ry = refined_rcp(d.y), rz = refined_rcp(d.z);
#pragma unroll
                for (int u = 0; u < RT_WF_BLIND; ++u) { RT_WALK_STEP(true) }
            } else {
                const float rx = 0.f, ry = 0.f, rz = 0.f;
#pragma unroll
                for (int u = 0; u < RT_WF_BLIND; ++u) { RT_WALK_STEP(false) }
            }
#undef RT_WALK_STEP
            // look-up: which of the logged cells are occupied?  Keep those -- as their DENSE ids, which is what the test phase gathers
            // records by -- in path order, at the front of the list.  Only the
            // requested words stay in registers across the wait; the logged cells are read back from LDS on both sides of it
            // (what a word is needed for -- "the block differs from the one before" -- is recomputed the same way).
            uint3 lw[RT_WF_BLIND];
            {
                uint32_t prev = wordKey;
#pragma unroll
                for (int i = 0; i < RT_WF_BLIND; ++i) {
                    // EVERY lane loads: a lane that needs no word (its block is the one it has, or it logged fewer cells) reads the table's
                    // first entry -- one address for all of them, one access -- instead of sitting a branch out: no branch, and no
                    // registers to zero for the lanes that skipped it (six moves per slot; -2 % of the kernel)
                    const uint32_t key = cellList[listed + i][threadIdx.x] & 0xFCFCFCu;
                    const bool need = ((uint32_t)i < logged) & (key != prev);
                    lw[i] = *reinterpret_cast<const uint3 *>(blockTable + (size_t)(need ? key * 3u : 0u));
                    prev = need ? key : prev;
                }
            }
            const uint32_t listedBefore = listed;
#pragma unroll
            for (int i = 0; i < RT_WF_BLIND; ++i) {
                if ((uint32_t)i < logged) {
                    const uint32_t c = cellList[listedBefore + i][threadIdx.x]; // slot listedBefore + i >= listed: not overwritten yet
                    const uint32_t key = c & 0xFCFCFCu;
                    if (key != wordKey) { wordKey = key; wordLo = lw[i].x; wordHi = lw[i].y; wordRank = lw[i].z; }
                    // bit (cx&3) | (cy&3)<<2 | (cz&3)<<4 : gather the three 2-bit fields with one multiply
                    const uint32_t bit = (((c & 0x030303u) * 0x1041u) >> 12) & 63u;
                    const uint32_t half = (c & 0x20000u) ? wordHi : wordLo; // bit 5 of `bit` is bit 1 of cz
                    if (__builtin_amdgcn_ubfe(half, bit & 31u, 1u)) {
                        // the cell's dense id = rank of its block + occupied cells below it in the block: what the test phase gathers by
                        const uint32_t below = (1u << (bit & 31u)) - 1u;
                        const uint32_t inLo = __popc(wordLo & ((c & 0x20000u) ? 0xffffffffu : below));
                        cellList[listed][threadIdx.x] = wordRank + inLo + ((c & 0x20000u) ? __popc(wordHi & below) : 0u);
                        ++listed;
                    }
                }
            }
        }

#ifdef RT_DIAG_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long dgT0 = diag_stamp();
        dgWalk += dgT0 - dgW0;
        dgBatches++;
#endif
        // ---- test, wave-cooperative: items = recorded cells of the whole wave, one per lane and round.  The reference tests a
        // cell's candidates in list order against a running maximum that is reset per cell (:366-379) and takes the hit of the
        // EARLIEST cell that has one (:380).  A candidate's own t, l1, l2 do not depend on the running maximum -- it only picks
        // the smallest t, the earlier candidate on a tie -- so candidates are tested independently and an LDS atomicMin on
        // (cell order | t | pair index) finds the same winner (t > tmin >= 0: its bits order like the value; pair indices grow
        // in list order inside a cell).  Round one tests every cell's FIRST candidate (it sits at the cell's dense id and says
        // how many more there are and where), the further candidates of all cells are flattened into a second list and tested
        // one per lane afterwards (7 % of the cells of a fine scene have any: looping over them cell by cell ran 64-lane
        // instructions for a handful of lanes, behind two more dependent gathers).  The owner re-evaluates the winning pair.
        {
            // (the cached block entry stays across the test phase: a register or two more at the kernel's peak, one gather fewer per batch and lane)
            const uint32_t mineN = listed;
            uint32_t incl = mineN;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t up = __shfl_up(incl, off, 64);
                if ((int)lane >= off) incl += up;
            }
            const uint32_t myBase = incl - mineN;
            const uint32_t items = __shfl(incl, 63, 64);
#ifdef RT_DIAG_STAMPS
            dgItems += items;
#endif
            if (items) { // wave-uniform
                // (the lists are addressed as the __shared__ arrays they are: through a generic `volatile` pointer every access became
                // a system-coherent FLAT instruction with a wait behind it.  One wave, in-order LDS: a wavefront-scope fence is all the
                // ordering the exchange between lanes needs, and it costs no instruction.)
                uint8_t (&owners)[RT_WF_LEAN_LIST * 64] = ownerOf[wave];
                unsigned long long (&keys)[64] = keyOf[wave];
                uint32_t (&moreWho)[RT_WF_MORE_ITEMS] = moreOf[wave][0], (&morePair)[RT_WF_MORE_ITEMS] = moreOf[wave][1];
                for (uint32_t j = 0; j < mineN; ++j) owners[myBase + j] = (uint8_t)lane;
                {   // (made here, not kept in a register pair across the walk: the compiler spilled the hoisted constant to scratch)
                    unsigned long long none = ~0ull;
                    asm volatile("" : "+v"(none));
                    keys[lane] = none;
                }
                if (lane == 0) moreCount[wave] = 0u;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier(); // one wave: its LDS operations retire in order
                for (uint32_t c0 = 0; c0 < items; c0 += 64) {
                    const uint32_t c = c0 + lane;
                    const bool has = c < items;
                    const uint32_t owner = has ? owners[c] : 0u;
                    const uint32_t ownerBase = __shfl(myBase, owner, 64);
                    const V3 po = mk(__shfl(o.x, owner, 64), __shfl(o.y, owner, 64), __shfl(o.z, owner, 64));
                    const V3 pd = mk(__shfl(d.x, owner, 64), __shfl(d.y, owner, 64), __shfl(d.z, owner, 64));
                    const float ptmin = __shfl(tmin, owner, 64), ptmax = __shfl(tmax, owner, 64);
                    const uint32_t pexcl = __shfl(excluded, owner, 64);
                    if (has) {
                        const uint32_t j = c - ownerBase;
                        const uint32_t pc = cellList[j][(wave << 6) + owner];
                        const uint32_t dense = pc; // (made by the look-up that found the cell occupied)
                        const float4 *rec = reinterpret_cast<const float4 *>(S.pairRec) + 4 * (size_t)dense;
                        float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                        const uint32_t info = __float_as_uint(r1.w);
                        unsigned long long best = ~0ull;
                        float t, l1, l2;
                        if (pair_test_flat(r0, r1, r2, r3, po, pd, ptmin, ptmax, pexcl, t, l1, l2)) best = hit_key(j, t, dense);
                        uint32_t n = info & 15u;
                        if (n > 1u) { // further candidates: onto the second list; a crowded cell, or one the list has no room for, in place
                            uint32_t restAt = info >> 4, i = 0;
                            if (n < RT_PAIR_MANY) {
                                const uint32_t at = atomicAdd(&moreCount[wave], n - 1u);
                                for (; i + 1 < n && at + i < RT_WF_MORE_ITEMS; ++i) { moreWho[at + i] = owner | (j << 6); morePair[at + i] = restAt + i; }
                            }
                            if (i + 1 < n) {
                                rec = reinterpret_cast<const float4 *>(S.pairRec) + 4 * (size_t)(restAt + i);
                                r0 = rec[0]; r1 = rec[1]; r2 = rec[2]; r3 = rec[3];
                                if (n == RT_PAIR_MANY) n = __float_as_uint(r1.w); // (i == 0 here: the first further record has the exact count)
#pragma unroll 1
                                for (;;) {
                                    if (pair_test_flat(r0, r1, r2, r3, po, pd, ptmin, ptmax, pexcl, t, l1, l2)) best = min(best, hit_key(j, t, restAt + i));
                                    if (++i + 1 >= n) break;
                                    rec += 4;
                                    r0 = rec[0]; r1 = rec[1]; r2 = rec[2]; r3 = rec[3];
                                }
                            }
                        }
                        if (best != ~0ull) atomicMin(&keys[owner], best);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const uint32_t more = min(moreCount[wave], (uint32_t)RT_WF_MORE_ITEMS);
                for (uint32_t e0 = 0; e0 < more; e0 += 64) {
                    const uint32_t e = e0 + lane;
                    const bool has = e < more;
                    const uint32_t who = has ? moreWho[e] : 0u;
                    const uint32_t owner = who & 63u;
                    const V3 po = mk(__shfl(o.x, owner, 64), __shfl(o.y, owner, 64), __shfl(o.z, owner, 64));
                    const V3 pd = mk(__shfl(d.x, owner, 64), __shfl(d.y, owner, 64), __shfl(d.z, owner, 64));
                    const float ptmin = __shfl(tmin, owner, 64), ptmax = __shfl(tmax, owner, 64);
                    const uint32_t pexcl = __shfl(excluded, owner, 64);
                    if (has) {
                        const uint32_t pair = morePair[e];
                        const float4 *rec = reinterpret_cast<const float4 *>(S.pairRec) + 4 * (size_t)pair;
                        const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                        float t, l1, l2;
                        if (pair_test_flat(r0, r1, r2, r3, po, pd, ptmin, ptmax, pexcl, t, l1, l2))
                            atomicMin(&keys[owner], hit_key(who >> 6, t, pair));
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (mineN) {
                    const unsigned long long key = keys[lane];
                    if (key != ~0ull) { // this segment's hit: the ray's answer is that of its lowest segment with one
                        atomicMin(&W.hitKey[par][q], ((unsigned long long)seg << 32) | (key & (unsigned long long)(2u * RT_PAIR_LIMIT - 1u)));
                        active = false;
                        walkEnded = true;
                    }
                }
            }
            listed = 0;
        }
#ifdef RT_DIAG_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        dgTest += diag_stamp() - dgT0;
#endif
        if (active && walkEnded) active = false; // walked to the end without a hit: hitKey[q] stays as it is
        if (spins > W.spinLimit || __ballot(active) == 0ull) break;
    }
    if (spins > W.spinLimit) { // the guard tripped: rays of this wave were abandoned -- tell the host, which fails the frame
        if (lane == 0) atomicOr(W.hostStatus + RT_WF_STATUS_ERROR, RT_WF_ERR_SPIN);
        break;
    }
#ifdef RT_DIAG_STAMPS
    if (lane == 0 && round == RT_DIAG_STAMPS) { // cycle anatomy of this wave in round RT_DIAG_STAMPS (scripts/diag_stamps.py); [5] = before the walk
        atomicAdd(&S.stats[0], diag_stamp() - dgStart); atomicAdd(&S.stats[1], dgWalk); atomicAdd(&S.stats[2], dgTest);
        atomicAdd(&S.stats[3], dgWalkIters); atomicAdd(&S.stats[4], dgBatches); atomicAdd(&S.stats[5], dgStart - dgK0);
        atomicAdd(&S.stats[6], 1ull); atomicAdd(&S.stats[7], dgItems);
    }
#endif
    } // passes
}

// ---- stage 4: samples -> u16 planes -----------------------------------------------------------------------------------
// One thread per pixel of the instance's tiles, row-major inside the tile (coalesced 2-byte stores).  Samples are added
// in order, each addend truncated on its own, saturating (raytrace_opencl.c:726-741); `first` starts from zero, later
// sample batches continue from the tile buffer.
__global__ __launch_bounds__(256) void wf_accum_kernel(const RtDevScene S, const RtWavefront W, const int first)
{
    const uint32_t localPixel = blockIdx.x * 256 + threadIdx.x;
    if (localPixel >= S.tileCount * RT_TILE_PIXELS) return;
    const uint32_t slot = localPixel / RT_TILE_PIXELS, inTile = localPixel % RT_TILE_PIXELS;
    const uint32_t tile = S.tileIds[slot];
    const uint32_t gx = (tile % S.tilesX) * RT_TILE + (inTile % RT_TILE), gy = (tile / S.tilesX) * RT_TILE + (inTile / RT_TILE);
    if (gx >= S.width || gy >= S.height) return;
    uint16_t *planes = S.tileBuf + (size_t)slot * 3 * RT_TILE_PIXELS + inTile;
    int r = 0, g = 0, b = 0;
    if (!first) { r = planes[0]; g = planes[RT_TILE_PIXELS]; b = planes[2 * RT_TILE_PIXELS]; }
    const float scale = (float)(0xFFFF) / (float)S.sampleDivisor; // :728
    for (uint32_t sb = 0; sb < W.samplesInBatch; ++sb) {
        const float4 c = W.sampleOut[localPixel * W.samplesInBatch + sb];
        r = sat_add_u16(r, c.x, scale);
        g = sat_add_u16(g, c.y, scale);
        b = sat_add_u16(b, c.z, scale);
    }
    planes[0] = (uint16_t)r;
    planes[RT_TILE_PIXELS] = (uint16_t)g;
    planes[2 * RT_TILE_PIXELS] = (uint16_t)b;
}

// ---- end of a batch's issued rounds: tell the host whether anybody is still waiting ------------------------------------------
// One workgroup.  The main queue slices of round `round` (what logic(round - 1) appended) hold one request per path that is not
// finished; their sum goes to the mapped host word, so the host can issue a frame's rounds without looking at the queue in
// between and check afterwards (rt_frame.cpp).
__global__ __launch_bounds__(256) void wf_status_kernel(const RtWavefront W, const uint32_t round, uint32_t *shadeCount)
{
    __shared__ uint32_t part[4];
    uint32_t n = W.ctl[(round % 3) * RT_WF_CTL_WORDS + RT_WF_CTL_COUNTS + threadIdx.x]; // RT_WF_SHARDS == 256 main slices
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t waiting = part[0] + part[1] + part[2] + part[3];
        if (waiting) atomicAdd(W.hostStatus + RT_WF_STATUS_WAITING, waiting);
        atomicAdd(W.hostStatus + RT_WF_STATUS_BATCHES, 1u);
    }
    // nothing of the batch is in flight any more: leave all three sets of control words zeroed for the next one (the host skips its memset --
    // a launch of the runtime's fill kernel with ~6 us of idle time in front of it -- when the batch before ended here)
    for (uint32_t i = threadIdx.x; i < 3u * RT_WF_CTL_WORDS; i += 256u) W.ctl[i] = 0u;
    if (shadeCount) // (the split rounds' list lengths, RtShadeList::count, likewise)
        for (uint32_t i = threadIdx.x; i < 3u * RT_WF_SHARDS; i += 256u) shadeCount[i] = 0u;
}

// ---- launch wrappers of the frame's kernels (rt_launch.h; those of the scene passes are in rt_scene_passes.hip) -------------------
extern "C" hipError_t rtw_launch_primary(const RtDevScene *scene, const RtWavefront *wf, hipStream_t stream)
{
    if (scene->tileCount == 0) return hipSuccess;
    hipLaunchKernelGGL(wf_primary_kernel, dim3(scene->tileCount * 64, wf->samplesInBatch), dim3(256), 0, stream, *scene, *wf);
    return hipGetLastError();
}

// passBuf: this tile group's slice of the pass buffer (rt_device.h, RT_PASS_*), its hit counters zeroed before the frame's first batch
extern "C" hipError_t rtw_launch_primary_passes(const RtDevScene *scene, const RtWavefront *wf, uint32_t *passBuf, hipStream_t stream)
{
    if (scene->tileCount == 0) return hipSuccess;
    hipLaunchKernelGGL(wf_primary_passes_kernel, dim3(scene->tileCount * 64, wf->samplesInBatch), dim3(256), 0, stream, *scene, *wf, passBuf);
    return hipGetLastError();
}

// surfBuf: this tile group's slice of the surface buffer (rt_device.h, RT_SURF_*); the batch with sampleBase 0 overwrites it
extern "C" hipError_t rtw_launch_surface_passes(const RtDevScene *scene, const RtWavefront *wf, float *surfBuf, hipStream_t stream)
{
    if (scene->tileCount == 0) return hipSuccess;
    hipLaunchKernelGGL(wf_surface_passes_kernel, dim3(scene->tileCount * 64), dim3(256), 0, stream, *scene, *wf, surfBuf);
    return hipGetLastError();
}

static bool mode_ok(const RtRoundMode &m)
{
    return m.slices >= 1u && m.slices <= RT_WF_SHARDS && (m.slices & (m.slices - 1u)) == 0u && m.segLen >= 1u && m.groupRays >= 1u && m.groupRays <= RT_WF_GROUP_RAYS;
}

// slicesIn: the queue slices of the round this launch consumes; next: the layout of the round it spawns (next.slices <= slicesIn)
extern "C" hipError_t rtw_launch_logic(const RtDevScene *scene, const RtWavefront *wf, uint32_t round, uint32_t blocks, uint32_t slicesIn, const RtRoundMode *next, hipStream_t stream)
{
    if (blocks % (RT_WF_SHARDS / 4) != 0) return hipErrorInvalidValue; // a whole number of waves per queue slice (wf_logic_kernel)
    if (!mode_ok(*next) || slicesIn < next->slices || slicesIn > RT_WF_SHARDS || (slicesIn & (slicesIn - 1u)) != 0u) return hipErrorInvalidValue;
    if ((next->ordered & RT_ROUND_DIRECT) && (round >= RT_WF_PLACE_ROUNDS || scene->pathClass != RT_PATH_CLASS_OPAQUE_DIFFUSE)) return hipErrorInvalidValue;
    if (scene->pathClass == RT_PATH_CLASS_OPAQUE_DIFFUSE) {
        if (round == 0u && next->ordered) hipLaunchKernelGGL((wf_logic_kernel<true, true, true>), dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *next);
        else if (round == 0u) hipLaunchKernelGGL((wf_logic_kernel<true, false, true>), dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *next);
        else if (next->ordered) hipLaunchKernelGGL((wf_logic_kernel<false, true, true>), dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *next);
        else hipLaunchKernelGGL((wf_logic_kernel<false, false, true>), dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *next);
    } else if (scene->pathClass == RT_PATH_CLASS_GENERAL) {
        if (round == 0u && next->ordered) hipLaunchKernelGGL((wf_logic_kernel<true, true, false>), dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *next);
        else if (round == 0u) hipLaunchKernelGGL((wf_logic_kernel<true, false, false>), dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *next);
        else if (next->ordered) hipLaunchKernelGGL((wf_logic_kernel<false, true, false>), dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *next);
        else hipLaunchKernelGGL((wf_logic_kernel<false, false, false>), dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *next);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}

// A split logic round (opaque-diffuse class, look-ahead on, round >= 1): the answers of every main entry ...
extern "C" hipError_t rtw_launch_answer(const RtDevScene *scene, const RtWavefront *wf, uint32_t round, uint32_t blocks, uint32_t slicesIn, const RtShadeList *list,
                                        uint32_t shadeFollows, hipStream_t stream)
{
    if (blocks % (RT_WF_SHARDS / 4) != 0 || blocks * 256ull < RT_WF_CTL_WORDS) return hipErrorInvalidValue; // whole waves per queue slice; the housekeeping's threads
    if (scene->pathClass != RT_PATH_CLASS_OPAQUE_DIFFUSE || !wf->lookAhead || round == 0u || !list->list || !list->count) return hipErrorInvalidValue;
    if (slicesIn < 1u || slicesIn > RT_WF_SHARDS || (slicesIn & (slicesIn - 1u)) != 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wf_answer_kernel, dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *list, shadeFollows);
    return hipGetLastError();
}

// ... then the listed paths' hits, shaded by dense waves (any whole number of waves per slice will do: they stride over the list)
extern "C" hipError_t rtw_launch_shade(const RtDevScene *scene, const RtWavefront *wf, uint32_t round, uint32_t blocks, uint32_t slicesIn, const RtRoundMode *next,
                                       const RtShadeList *list, hipStream_t stream)
{
    if (blocks == 0u || blocks % (RT_WF_SHARDS / 4) != 0) return hipErrorInvalidValue;
    if (!mode_ok(*next) || slicesIn < next->slices || slicesIn > RT_WF_SHARDS || (slicesIn & (slicesIn - 1u)) != 0u) return hipErrorInvalidValue;
    if (scene->pathClass != RT_PATH_CLASS_OPAQUE_DIFFUSE || !wf->lookAhead || round == 0u || !list->list || !list->count) return hipErrorInvalidValue;
    if ((next->ordered & RT_ROUND_DIRECT) && round >= RT_WF_PLACE_ROUNDS) return hipErrorInvalidValue;
    if (next->ordered) hipLaunchKernelGGL(wf_shade_kernel<true>, dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *next, *list);
    else hipLaunchKernelGGL(wf_shade_kernel<false>, dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, slicesIn, *next, *list);
    return hipGetLastError();
}

// an ordered round: ranks -> positions (fixed grid, the kernel strides over the blocks that are in use)
extern "C" hipError_t rtw_launch_scatter(const RtWavefront *wf, uint32_t round, uint32_t blocks, const RtRoundMode *mode, hipStream_t stream)
{
    if (!mode_ok(*mode)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wf_scatter_kernel, dim3(blocks), dim3(256), 0, stream, *wf, round, mode->slices, mode->segLen);
    return hipGetLastError();
}

// TEST ONLY (tuning key place_skew): the round's recorded placement table with one entry moved from its first cell that holds any to the
// cell behind it -- still a partition of [0, total), but not the one the frame's entries want: a frame placed by it runs one cell over
// (the guard's path) and leaves the other a stale entry.
extern "C" hipError_t rtw_launch_place_skew(const RtWavefront *wf, uint32_t round, hipStream_t stream)
{
    if (round < 1u || round > RT_WF_PLACE_ROUNDS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wf_place_skew_kernel, dim3(1), dim3(64), 0, stream, *wf, round);
    return hipGetLastError();
}

// one workgroup per 256 entries (a watched frame's grid is sized for the worst case; surplus workgroups exit at once)
extern "C" hipError_t rtw_launch_trace(const RtDevScene *scene, const RtWavefront *wf, uint32_t round, uint32_t blocks, const RtRoundMode *mode, hipStream_t stream)
{
    if (!mode_ok(*mode)) return hipErrorInvalidValue;
    if ((mode->ordered & RT_ROUND_DIRECT) && (round < 1u || round > RT_WF_PLACE_ROUNDS)) return hipErrorInvalidValue;
    if (mode->ordered) hipLaunchKernelGGL(wf_trace_kernel<true>, dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, *mode);
    else hipLaunchKernelGGL(wf_trace_kernel<false>, dim3(blocks), dim3(256), 0, stream, *scene, *wf, round, *mode);
    return hipGetLastError();
}

extern "C" hipError_t rtw_launch_status(const RtWavefront *wf, uint32_t round, uint32_t *shadeCount, hipStream_t stream)
{
    static_assert(RT_WF_SHARDS == 256, "wf_status_kernel sums one main queue slice per thread");
    hipLaunchKernelGGL(wf_status_kernel, dim3(1), dim3(256), 0, stream, *wf, round, shadeCount);
    return hipGetLastError();
}

extern "C" hipError_t rtw_launch_accum(const RtDevScene *scene, const RtWavefront *wf, int first, hipStream_t stream)
{
    const uint32_t n = scene->tileCount * RT_TILE_PIXELS;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(wf_accum_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *scene, *wf, first);
    return hipGetLastError();
}
