// rt_wf_shared.h -- the device helpers that the frame's kernels (rt_wavefront.hip) and the scene passes (rt_scene_passes.hip) both read:
// the wave-aggregated appends, the flattened camera scan and pair test, hit resolution, and the trace entries (the DDA start state of a
// ray and its exact segments).  Each translation unit compiles its own copy; everything here is inlined into the kernels that use it.
#pragma once
#include "rt_devfuncs.h"
#include "rt_ray_clip.h"

namespace {

__device__ __forceinline__ float4 pack4(V3 v, float w) { return make_float4(v.x, v.y, v.z, w); }
__device__ __forceinline__ V3 xyz(float4 v) { return mk(v.x, v.y, v.z); }

// A frame with ONE sample per pixel needs no ordered accumulate (raytrace_opencl.c:726-741 adds to zeroed planes once): the
// kernel that finishes a pixel writes its three u16 values itself, wf_accum_kernel is not launched.  (S.directStore; a one-sample frame
// that continues a sample window's sequence from the tile buffer goes through sampleOut and wf_accum_kernel like any other.)
__device__ __forceinline__ void store_single_sample(const RtDevScene &S, uint32_t localPixel, V3 c)
{
    const uint32_t slot = localPixel / RT_TILE_PIXELS, inTile = localPixel % RT_TILE_PIXELS;
    uint16_t *planes = S.tileBuf + (size_t)slot * 3 * RT_TILE_PIXELS + inTile;
    uint32_t samples = S.sampleDivisor; // :728 (the window's divisor; 1 by default here).  Opaque, so that the quotient is made where it is used: hoisted to the top of the
    asm volatile("" : "+s"(samples)); // logic kernel it lived in a vector register across the state machine and was spilled
    const float scale = (float)(0xFFFF) / (float)samples;
    planes[0] = (uint16_t)sat_add_u16(0, c.x, scale);
    planes[RT_TILE_PIXELS] = (uint16_t)sat_add_u16(0, c.y, scale);
    planes[2 * RT_TILE_PIXELS] = (uint16_t)sat_add_u16(0, c.z, scale);
}

// Wave-aggregated queue append: one atomic per wave for all lanes that `want` a slot.  Must be reached by the lanes
// together (it ballots over the lanes that execute it).
__device__ __forceinline__ uint32_t wave_append(uint32_t *counter, bool want)
{
    const unsigned long long mask = __ballot(want);
    if (mask == 0) return 0;
    const uint32_t lane = __lane_id();
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, leader, 64);
    return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// Two appends in one round trip: lanes 0 and 1 carry the two atomics of the wave in the same instruction.
__device__ __forceinline__ void wave_append2(uint32_t *counterA, bool wantA, uint32_t *counterB, bool wantB, uint32_t &posA, uint32_t &posB)
{
    const unsigned long long maskA = __ballot(wantA), maskB = __ballot(wantB);
    const uint32_t lane = __lane_id();
    uint32_t base = 0;
    const uint32_t n = (lane == 0u) ? (uint32_t)__popcll(maskA) : (uint32_t)__popcll(maskB);
    if (lane < 2u && n != 0u) base = atomicAdd(lane == 0u ? counterA : counterB, n);
    const unsigned long long below = (1ull << lane) - 1ull;
    posA = (uint32_t)__shfl((int)base, 0, 64) + (uint32_t)__popcll(maskA & below);
    posB = (uint32_t)__shfl((int)base, 1, 64) + (uint32_t)__popcll(maskB & below);
}

// Triangle test on a per-triangle record that is already in registers (rt_device.h: a | ab | ac | n | abab abac acac inv),
// branch-free like pair_test_flat below: same operations and operands as tri_test for every lane whose plane distance is in
// range, the others discard the second half.
__device__ __forceinline__ bool tri_rec_test_flat(const float4 r0, const float4 r1, const float4 r2, const float4 r3, V3 o, V3 d, float tmin,
                                                  float tmax, float &t, float &l1, float &l2)
{
    const V3 a = mk(r0.x, r0.y, r0.z), ab = mk(r0.w, r1.x, r1.y), ac = mk(r1.z, r1.w, r2.x), n = mk(r2.y, r2.z, r2.w);
    const V3 ao = sub3(o, a);
    t = -dot3(n, ao) / dot3(n, d);
    const V3 ap = sub3(along(o, t, d), a);
    const float ap_ab = dot3(ap, ab);
    const float ap_ac = dot3(ap, ac);
    l1 = (r3.y * ap_ac - r3.z * ap_ab) * r3.w;
    l2 = (r3.y * ap_ab - r3.x * ap_ac) * r3.w;
    return (tmin < t) & (t < tmax) & (0 <= l1) & (0 <= l2) & (l1 + l2 <= 1.f);
}

// Nearest hit among the pixel's candidate list (raytrace_opencl.c:514-528): running maximum, ties keep the earliest.
// Two candidates per step: their list entries were requested a step ahead, their records are requested together, so a
// pixel with one or two candidates (the common case) costs three dependent round trips: range, list, records.
__device__ __forceinline__ uint32_t camera_scan(const RtDevScene &S, uint32_t localPixel, V3 o, V3 d, float tmin, float tmax,
                                                uint32_t excluded, float &hit_t, float &hit_l1, float &hit_l2)
{
    uint32_t hit_tri = RT_NONE;
    hit_t = tmax;
    const uint32_t first = S.camStart[localPixel], last = S.camEnd[localPixel];
    const float4 *recs = reinterpret_cast<const float4 *>(S.triRec);
    uint32_t t0 = (first < last) ? S.camList[first] : RT_NONE;
    uint32_t t1 = (first + 1 < last) ? S.camList[first + 1] : RT_NONE;
    for (uint32_t i = first; i < last; i += 2) {
        const bool two = i + 1 < last;
        const float4 *ra = recs + 4 * (size_t)t0, *rb = recs + 4 * (size_t)(two ? t1 : t0);
        const float4 a0 = ra[0], a1 = ra[1], a2 = ra[2], a3 = ra[3];
        const float4 b0 = rb[0], b1 = rb[1], b2 = rb[2], b3 = rb[3];
        const uint32_t n0 = (i + 2 < last) ? S.camList[i + 2] : RT_NONE;
        const uint32_t n1 = (i + 3 < last) ? S.camList[i + 3] : RT_NONE;
        float t, l1, l2;
        if (tri_rec_test_flat(a0, a1, a2, a3, o, d, tmin, hit_t, t, l1, l2) & (excluded != t0)) {
            hit_t = t; hit_tri = t0; hit_l1 = l1; hit_l2 = l2;
        }
        if (tri_rec_test_flat(b0, b1, b2, b3, o, d, tmin, hit_t, t, l1, l2) & (excluded != t1) & two) {
            hit_t = t; hit_tri = t1; hit_l1 = l1; hit_l2 = l2;
        }
        t0 = n0; t1 = n1;
    }
    return hit_tri;
}

// The same scan without the pipelining, for the logic kernel's rare camera-type continuation rays (:707-722), where
// registers matter more than round trips.
__device__ __forceinline__ uint32_t camera_scan_compact(const RtDevScene &S, uint32_t localPixel, V3 o, V3 d, float tmin, float tmax,
                                                     uint32_t excluded, float &hit_t, float &hit_l1, float &hit_l2)
{
    uint32_t hit_tri = RT_NONE;
    hit_t = tmax;
    const uint32_t first = S.camStart[localPixel], last = S.camEnd[localPixel];
    for (uint32_t i = first; i < last; ++i) {
        const uint32_t tri = S.camList[i];
        if (excluded != tri) {
            float t, l1, l2;
            if (tri_test(S.triRec, tri, o, d, tmin, hit_t, t, l1, l2)) {
                hit_t = t; hit_tri = tri; hit_l1 = l1; hit_l2 = l2;
            }
        }
    }
    return hit_tri;
}

// Triangle test against a (cell, triangle) pair record (rt_device.h: {a,id}{n,-}{ab,abab}{ac,acac}), the arithmetic of
// tri_test / the reference (raytrace_opencl.c:124-172).
// The record is already in registers and the test is BRANCH-FREE: every lane computes both halves, and whether the
// plane distance was in range only enters the final predicate.  Lanes for which the reference would not have computed the
// second half (raytrace_opencl.c:143) discard it; for the others every operation and operand is the same, so t, l1, l2
// are bit-identical.  With no branch between the four 16-byte loads and their uses the compiler issues them together
// (one round trip per candidate instead of three dependent ones).
__device__ __forceinline__ bool pair_test_flat(const float4 r0, const float4 r1, const float4 r2, const float4 r3, V3 o, V3 d, float tmin,
                                               float tmax, uint32_t excluded, float &t, float &l1, float &l2)
{
    const uint32_t tri = __float_as_uint(r0.w);
    const V3 a = mk(r0.x, r0.y, r0.z), n = mk(r1.x, r1.y, r1.z);
    const V3 ao = sub3(o, a);
    t = -dot3(n, ao) / dot3(n, d);
    const V3 ab = mk(r2.x, r2.y, r2.z), ac = mk(r3.x, r3.y, r3.z);
    // The record's two spare words carry dot(ab,ac) and 1/(abac^2 - abab*acac) as rt_prepare_triangles worked them out (:147-149, the same
    // correctly rounded division); the two squared lengths are worked out here from the same operands.  (The other way round -- lengths
    // stored, the quotient taken here -- was a second full division per candidate: ~13 issue slots against 10 plain ones.)
    const float abab = dot3(ab, ab), abac = r2.w, acac = dot3(ac, ac);
    const float inv = r3.w;
    const V3 ap = sub3(along(o, t, d), a);
    const float ap_ab = dot3(ap, ab);
    const float ap_ac = dot3(ap, ac);
    l1 = (abac * ap_ac - acac * ap_ab) * inv;
    l2 = (abac * ap_ab - abab * ap_ac) * inv;
    return (tri != excluded) & (tmin < t) & (t < tmax) & (0 <= l1) & (0 <= l2) & (l1 + l2 <= 1.f);
}

// The answer of a traced ray from its hitKey: the winning (cell, triangle) pair is evaluated once more with the ray's own
// limits, which reproduces t, l1, l2 bit for bit (the running maximum of :366-379 only ever rejected other candidates).
__device__ __forceinline__ uint32_t resolve_hit(const RtDevScene &S, unsigned long long key, V3 o, V3 d, float tmin, float tmax,
                                                uint32_t excluded, float &t, float &l1, float &l2)
{
    if (key == ~0ull) return RT_NONE;
    const float4 *rec = reinterpret_cast<const float4 *>(S.pairRec) + 4 * (size_t)(uint32_t)key;
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    pair_test_flat(r0, r1, r2, r3, o, d, tmin, tmax, excluded, t, l1, l2);
    return __float_as_uint(r0.w);
}

// Order of the hits of one ray inside a test phase: earlier recorded cell, then smaller t, then earlier candidate.
__device__ __forceinline__ unsigned long long hit_key(uint32_t cellOrder, float t, uint32_t pair)
{
    return ((unsigned long long)cellOrder << 60) | ((unsigned long long)__float_as_uint(t) << 29) | (unsigned long long)pair;
}

#if defined(RT_DIAG_STAMPS) || defined(RT_DIAG_LOGIC)
// Diagnostic build only (never shipped, outputs untouched): shader-clock stamps, summed per wave into S.stats.
__device__ __forceinline__ unsigned long long diag_stamp()
{
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
#endif

} // namespace

// ---- trace entries: the DDA start state of a ray, and exact segments ------------------------------------------------
// A round lasts as long as its longest dependent chain: a ray that crosses the whole grid makes 766 cell visits one after
// the other, and measured round times are ~0.4 ms + 0.32 ms per million rays -- the constant is that chain.  The walk is a
// 3-way merge: per axis, the parameters T_a(i) = (plane_a[i] - o_a) / d_a at which the ray crosses successive planes form a
// non-decreasing sequence (the same rounded quotients the reference computes, :383-385), and every step takes the smallest
// head (:387-398).  So the state of the walk after all crossings with T <= tau is, per axis, simply the NUMBER of such
// crossings -- it can be computed without walking (a plane search plus two exact divides per axis), for any tau.  A long
// ray is therefore cut into up to RT_WF_MAXSEG SEGMENTS at parameters tau_k: segment k starts in the state at tau_k and ends
// when it has visited the start cell of segment k+1 (the existing end-cell rule, :380).  Segments are traced by different
// lanes; the ray's answer is the hit of its lowest segment that has one (atomicMin on hitKey), exactly the first cell
// with a hit in path order.  Segments after a hit are wasted work; the chain per lane is ~8x shorter.
//
// Who makes the DDA start state of a ray (no kernel of its own: a set-up kernel between logic and trace cost a launch, a second
// round trip of every ray through HBM and 30-50 us per round of a frame whose rounds are 60-600 us):
//   * an ORDERED round (many rays: bound by total work, never cut) -- wf_logic_kernel, where the ray is in registers and nearly
//     every lane spawns one; the entry carries the start state, and its walk-length class (predicted cell visits, exact for a
//     ray that hits nothing) is counted on the way (per wave in LDS, one global atomic instruction per wave); wf_scatter_kernel
//     turns ranks into positions, longest class first;
//   * any other round (few rays: bound by its longest chain, cut finely enough to occupy every SIMD) -- wf_trace_kernel<false>,
//     whose workgroups take a few rays each, plan them with every lane busy, and deal the segments to their lanes.  In a late
//     round only every tenth path spawns a ray: planning those in the logic kernel ran its whole tail at a tenth of the lanes
//     (measured: logic round 1 84 -> 167 us).
// Only the ORDER and GROUPING in which cells are visited changes.  Cutting costs work (every segment has a start-up and a test
// batch of its own, segments behind a hit are wasted), so the aimed-at cell visits per segment depend on how many rays the
// round has (RtRoundMode::segLen, chosen by the host from the launch plan).
#ifndef RT_WF_MAXSEG
#define RT_WF_MAXSEG 12
#endif
struct DdaState { uint32_t cell; float dx, dy, dz; };

// One axis of the state at parameter tau: c0 = cell coordinate of the walk's start, returns the coordinate after all
// crossings with T <= tau and, in `head`, the parameter of the next crossing.  `limit` = crossings that stay inside the grid.
// `lut` / `lutScale` (optional): this axis' 256 cell estimates and 256 / box width (RtDevScene::cellLut) -- the guess then costs one
// table read instead of the eight dependent reads of a plane search, unless the table is coarse where the point lies.
__device__ __forceinline__ uint32_t axis_state_at(const float *planes, uint32_t c0, float oa, float da, float tau, float &head,
                                                  const uint8_t *lut = nullptr, float lutScale = 0.f)
{
    const bool pos = (0.f <= da);
    const int limit = pos ? (int)(RT_GRID_DIV - 1 - c0) : (int)c0; // the crossing after these leaves the grid (tau is before it)
    // guess from the position (the plane search of GetBoxAddress), then settle it with the exact quotients
    const float p = oa + tau * da;
    int g = 0;
    bool search = true;
    if (lut) {
        const int i = min(255, max(0, (int)((p - planes[0]) * lutScale)));
        const int a = lut[max(i - 1, 0)], b = lut[min(i + 1, 255)];
        g = lut[i];
        search = b - a > 4; // (more than a few cells in three table steps: the settling loops below would walk them one by one)
    }
    if (search) {
        g = 0;
#pragma unroll
        for (int div = RT_GRID_DIV / 2; div >= 1; div /= 2)
            if (planes[g + div] < p) g += div;
    }
    int m = pos ? g - (int)c0 : (int)c0 - g;
    m = m < 0 ? 0 : (m > limit ? limit : m);
    // crossing number k (1-based) is plane c0+k going up, c0-k+1 going down
    while (m >= 1 && !((planes[pos ? (int)c0 + m : (int)c0 - m + 1] - oa) / da <= tau)) --m;
    float next = (planes[pos ? (int)c0 + m + 1 : (int)c0 - m] - oa) / da;
    while (m < limit && next <= tau) {
        ++m;
        next = (planes[pos ? (int)c0 + m + 1 : (int)c0 - m] - oa) / da;
    }
    head = next;
    return pos ? c0 + (uint32_t)m : c0 - (uint32_t)m;
}

// GetBoxAddress (:174-193) on the LDS planes: strict '<'; packed cx | cy << 8 | cz << 16
__device__ __forceinline__ uint32_t cell_of(const float *planes, V3 p)
{
    int cx = 0, cy = 0, cz = 0;
#pragma unroll
    for (int div = RT_GRID_DIV / 2; div >= 1; div /= 2) {
        if (planes[cx + div] < p.x) cx += div;
        if (planes[(RT_GRID_DIV + 1) + cy + div] < p.y) cy += div;
        if (planes[2 * (RT_GRID_DIV + 1) + cz + div] < p.z) cz += div;
    }
    return (uint32_t)cx | ((uint32_t)cy << 8) | ((uint32_t)cz << 16);
}

// What a ray's walk is made from: its DDA start state (:351-362, :383-385), where it ends (a ray with a finite range: the cell of
// its far end, :356-362), how many cells it will visit if it hits nothing, and where it leaves the grid (te).
struct EntryPlan { DdaState start; uint32_t endCell, visits; float te; };

// `haveStart`: the caller knows the start cell (a hit's shadow ray and its bounce ray start at the same point).  `lut` (optional; LDS
// copy of RtDevScene::cellLut followed by the three scales 256 / box width): where a ray WITHOUT an end cell leaves the grid -- which
// only predicts the length of its walk -- is estimated with one table read per axis instead of a plane search.
// `clip` (optional; RtDevScene::boxMin + RT_CLIP_AT, the same address in every lane): the scene's clip planes (rt_ray_clip.h), read with scalar
// loads.  A plain ray's te is lowered to where it leaves their bound, and it ends in the cell of that point like a finite ray.
typedef const __attribute__((address_space(4))) float *ClipPlanes;
__device__ __forceinline__ EntryPlan plan_ray(const float *planes, V3 o, V3 d, float tmin, float tmax, bool haveStart = false, uint32_t startCell = 0u,
                                              const uint8_t *lut = nullptr, const float *lutScale = nullptr, const float *clip = nullptr)
{
    EntryPlan p;
    const V3 lo = mk(planes[0], planes[RT_GRID_DIV + 1], planes[2 * (RT_GRID_DIV + 1)]);
    const V3 hi = mk(planes[RT_GRID_DIV], planes[2 * RT_GRID_DIV + 1], planes[3 * RT_GRID_DIV + 2]);
    // start / end cells (:351-362)
    V3 from = along(o, tmin, d);
    const bool startInside = lo.x <= from.x && from.x <= hi.x && lo.y <= from.y && from.y <= hi.y && lo.z <= from.z && from.z <= hi.z;
    bind_in_cube(from, d, lo, hi);
    p.start.cell = startCell;
    if (!haveStart) p.start.cell = cell_of(planes, from);
    p.te = RT_INF;
    V3 to;
    if (tmax < RT_INF) {
        to = along(o, tmax, d);
        bind_in_cube(to, d, lo, hi);
    } else {
        // where the ray leaves the grid: the smallest of the three boundary crossings (same quotients as the walk's)
        if (d.x != 0.f) { const float t = (((0.f <= d.x) ? hi.x : lo.x) - o.x) / d.x; if (t < p.te) p.te = t; }
        if (d.y != 0.f) { const float t = (((0.f <= d.y) ? hi.y : lo.y) - o.y) / d.y; if (t < p.te) p.te = t; }
        if (d.z != 0.f) { const float t = (((0.f <= d.z) ? hi.z : lo.z) - o.z) / d.z; if (t < p.te) p.te = t; }
        to = (p.te < RT_INF) ? along(o, p.te, d) : from;
    }
    const int cx = (int)(p.start.cell & 255u), cy = (int)((p.start.cell >> 8) & 255u), cz = (int)(p.start.cell >> 16);
    // distances from the ray ORIGIN to the next plane of each axis (:383-385)
    p.start.dx = (planes[cx + ((0 <= d.x) ? 1 : 0)] - o.x) / d.x;
    p.start.dy = (planes[(RT_GRID_DIV + 1) + cy + ((0 <= d.y) ? 1 : 0)] - o.y) / d.y;
    p.start.dz = (planes[2 * (RT_GRID_DIV + 1) + cz + ((0 <= d.z) ? 1 : 0)] - o.z) / d.z;
    // the clip (rt_ray_clip.h has the argument): the walk ends once it has visited the cell of o + te d, beyond which every cell is empty
    bool clipped = false;
    if (clip) {
        const ClipPlanes cp = (ClipPlanes)(uintptr_t)clip;
        const uint32_t count = __float_as_uint(cp[0]);
        clipped = rt_clip_ray(cp, count, tmax < RT_INF, startInside, o.x, o.y, o.z, d.x, d.y, d.z, tmin, p.start.dx, p.start.dy, p.start.dz, p.te);
        if (clipped) to = along(o, p.te, d);
    }
    uint32_t last; // (where a ray without an end cell leaves the grid is a scheduling matter only)
    if (lut && !(tmax < RT_INF) && !clipped) {
        const float fx = (to.x - lo.x) * lutScale[0], fy = (to.y - lo.y) * lutScale[1], fz = (to.z - lo.z) * lutScale[2];
        const int ix = min(255, max(0, (int)fx)), iy = min(255, max(0, (int)fy)), iz = min(255, max(0, (int)fz)); // (a NaN converts to 0)
        last = (uint32_t)lut[ix] | ((uint32_t)lut[256 + iy] << 8) | ((uint32_t)lut[512 + iz] << 16);
    } else last = cell_of(planes, to);
    p.endCell = (tmax < RT_INF || clipped) ? last : 0xffffffffu;
    // every step moves one axis by one cell in a fixed direction: visits = Manhattan distance + 1
    p.visits = (uint32_t)(abs((int)(last & 255u) - cx) + abs((int)((last >> 8) & 255u) - cy) + abs((int)(last >> 16) - cz)) + 1u;
    return p;
}

// Into how many segments a planned ray is cut when a segment should make about segLen cell visits.  Only rays without an end
// cell are cut, and only where every quotient involved is an ordinary number (a zero direction component makes heads infinite
// or NaN and the merge argument is not worth stretching to them); a ray only slightly over the aim is left whole.
__device__ __forceinline__ uint32_t segments_of(const EntryPlan &p, V3 d, float tmax, uint32_t segLen)
{
    const bool plain = rt_clip_plain(tmax < RT_INF, d.x, d.y, d.z, p.te, p.start.dx, p.start.dy, p.start.dz);
    if (!plain || p.visits <= segLen + segLen / 4) return 1u;
    const uint32_t n = (p.visits + segLen - 1) / segLen;
    return n > RT_WF_MAXSEG ? (uint32_t)RT_WF_MAXSEG : n;
}

// Cut k (1 <= k < n) of a ray: tau_k = ta + (te - ta) * k / n is non-decreasing in k, and a cut only exists where ta <= tau_k < te,
// so the cuts that exist are a prefix of 1 .. n - 1: whether cut k and cut k + 1 exist can be told from k alone.
__device__ __forceinline__ bool cut_at(float ta, float te, uint32_t k, uint32_t n, float &tau)
{
    tau = ta + (te - ta) * ((float)k / (float)n);
    return ta <= tau && tau < te;
}
