// rt_ray_clip.h -- the arithmetic of the ray clip ("Round 7"), with no HIP in it: the kernels of rt_wavefront.hip and
// rt_scene_prep.hip, the host side of rt_api.cpp and tests/ray_clip_host.cpp (which compiles it for the host on its own) all use these
// functions, so that what the test walks is what the device plans.
//
// THE BOUND.  A scene keeps up to RT_CLIP_MAX_PLANES half-spaces n.x <= off that hold every corner of every OCCUPIED cell of its grid
// (unit normals from a fixed candidate set, offsets = the support of the occupied cells' boxes, inflated by rt_clip_inflation).
//
// THE CLIP.  A grid ray without a far end (tmax = inf) walks until it leaves the grid's box; te is the parameter of that exit.  For such
// a ray, where every quotient is an ordinary number (rt_clip_plain), te is lowered to where the ray crosses a kept plane outwards, pushed
// out by a slack, and the walk ends in the cell E that holds P = o + te * d (exact plane search), like a finite ray ends in the cell of
// its far end.
//
// WHY NO RESULT CHANGES.  The walk moves one axis by one cell per step, always in the direction of d, so a cell C visited after E has,
// per axis, the index of E or one further along d.  Let T be the (rounded) head at which the walk entered C.
//   * T >= te: the point o + T d lies in C up to the rounding of the heads (a few ulps of |o_a| + |plane| + |T d_a| per axis) and
//     n.(o + T d) >= n.(o + te d), because n.d > 0.
//   * T < te: every axis on which C lies beyond E was crossed at a head below te, yet P = o + te d, evaluated in the same arithmetic, lies
//     in E: P is within the heads' rounding of C's near face on those axes, and in C's slab on the others.
// Either way C holds, up to a few ulps of max(|o_a|, |plane|) per axis, a point X with n.X >= n.P - (the same few ulps).  The slacks make
// n.P exceed the raw support by far more than that: the offsets are inflated by 3e-4 of the box diagonal + 2e-5 of the largest plane
// magnitude (thousands of ulps; a cell of an even 256-grid is 2e-3 of the diagonal wide), the numerator of t by 2e-5 of the magnitudes
// that went into it (|off|, |n_a o_a|: 300 ulps, against the 4 roundings of the dot product and the reciprocal's 1 ulp), and t itself by
// 2e-5 of |t|.  A cell with a point outside a kept half-space has a corner outside it, so it is not occupied: it holds no candidates,
// whatever a trace would have done there.  If E is not on the walk's path (a corner graze) the walk runs to the box wall as before.
#ifndef RT_RAY_CLIP_H
#define RT_RAY_CLIP_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_CLIP_HD __host__ __device__ __forceinline__
#else
#define RT_CLIP_HD inline
#endif

#define RT_CLIP_MAX_PLANES 8
#define RT_CLIP_CANDIDATES 290 // primitive integer vectors with components in -3..3
#define RT_CLIP_LATTICE 32     // the greedy choice scores planes on the centres of every 8th cell per axis

// The planes' buffer (RtDevScene::boxMin) behind its 3 x 257 planes, in floats: the number of planes the kernels apply (a uint32's bits;
// 0 with tuning key ray_clip = 0), the kept planes {n.xyz, off}, the support keys the bound kernel reduces into and the candidate normals
// {n.xyz, 0} it reads.  Every field starts on a 16-byte boundary.
#define RT_CLIP_AT 772
#define RT_CLIP_PLANES_AT 776
#define RT_CLIP_KEYS_AT (RT_CLIP_PLANES_AT + 4 * RT_CLIP_MAX_PLANES)
#define RT_CLIP_NORMALS_AT (RT_CLIP_KEYS_AT + (RT_CLIP_CANDIDATES + 3) / 4 * 4) // (one key per candidate, rounded up to 16 bytes)
#define RT_CLIP_FLOATS (RT_CLIP_NORMALS_AT + 4 * RT_CLIP_CANDIDATES)

#define RT_CLIP_SLACK_REL 2e-5f
#define RT_CLIP_SLACK_ABS 2e-5f

// The candidate normals in their fixed order (x fastest), unit length; returns their number (RT_CLIP_CANDIDATES).
inline int rt_clip_candidates(float (*out)[4])
{
    auto gcd = [](int a, int b) { a = a < 0 ? -a : a; b = b < 0 ? -b : b; while (b) { const int t = a % b; a = b; b = t; } return a; };
    int n = 0;
    for (int z = -3; z <= 3; ++z)
        for (int y = -3; y <= 3; ++y)
            for (int x = -3; x <= 3; ++x) {
                if (gcd(gcd(x, y), z) != 1) continue;
                const double len = __builtin_sqrt((double)(x * x + y * y + z * z));
                if (out) { out[n][0] = (float)(x / len); out[n][1] = (float)(y / len); out[n][2] = (float)(z / len); out[n][3] = 0.f; }
                ++n;
            }
    return n;
}

// order-preserving key of a float for an unsigned atomicMax (0 = below every float), and back
RT_CLIP_HD uint32_t rt_clip_key(float f)
{
    union { float f; uint32_t u; } v; v.f = f;
    return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}
RT_CLIP_HD float rt_clip_unkey(uint32_t k)
{
    union { float f; uint32_t u; } v; v.u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return v.f;
}

// n . (the corner of the box [lo, hi] that lies furthest along n)
RT_CLIP_HD float rt_clip_support(float nx, float ny, float nz, float lox, float loy, float loz, float hix, float hiy, float hiz)
{
    return nx * (0.f <= nx ? hix : lox) + ny * (0.f <= ny ? hiy : loy) + nz * (0.f <= nz ? hiz : loz);
}

// by how much a support offset is inflated: planes = the [3][div + 1] plane table of a grid of div cells per axis (the scenes': 256)
inline float rt_clip_inflation(const float *planes, int div = 256)
{
    float diag2 = 0.f, big = 0.f;
    for (int w = 0; w < 3; ++w) {
        const float lo = planes[w * (div + 1)], hi = planes[w * (div + 1) + div];
        diag2 += (hi - lo) * (hi - lo);
        const float a = lo < 0.f ? -lo : lo, b = hi < 0.f ? -hi : hi;
        if (a > big) big = a;
        if (b > big) big = b;
    }
    return 3e-4f * __builtin_sqrtf(diag2) + 2e-5f * big;
}

// Which of the candidates are kept: greedily, the plane that cuts off most lattice points (centres of cells 4, 12, .. 252 per axis of a
// 256-grid, in cell-index space) no earlier pick cuts off, until a pick adds nothing or RT_CLIP_MAX_PLANES are kept; none if all picks together cut off
// less than 5 % of the lattice.  `off` = the inflated offsets (a candidate with a non-finite offset is never kept; ties go to the lower
// index).  Returns the number kept, their indices in `kept`, and in `cut` (optional) the lattice points cut off.
inline int rt_clip_choose(const float *planes, const float (*normal)[4], const float *off, int candidates, int *kept, int *cut, int div = 256)
{
    constexpr int L = RT_CLIP_LATTICE, WORDS = L * L; // one 32-bit word per (j, k): bit i
    static_assert(L == 32, "one word per lattice row");
    float centre[3][L];
    for (int w = 0; w < 3; ++w)
        for (int i = 0; i < L; ++i) { const int c = (2 * i + 1) * div / (2 * L); centre[w][i] = 0.5f * (planes[w * (div + 1) + c] + planes[w * (div + 1) + c + 1]); }
    uint32_t *mask = new uint32_t[(size_t)candidates * WORDS];
    for (int c = 0; c < candidates; ++c) {
        uint32_t *m = mask + (size_t)c * WORDS;
        float ax[L];
        for (int i = 0; i < L; ++i) ax[i] = normal[c][0] * centre[0][i];
        const bool usable = off[c] == off[c] && off[c] - off[c] == 0.f;
        for (int k = 0; k < L; ++k)
            for (int j = 0; j < L; ++j) {
                const float rest = off[c] - (normal[c][1] * centre[1][j] + normal[c][2] * centre[2][k]);
                // (the centres ascend, so ax is monotone: the points with ax[i] > rest are the top or the bottom `count` of the row)
                uint32_t word = 0;
                if (usable) {
                    int count = 0;
                    if (normal[c][0] > 0.f) { int lo = 0, hi = L; while (lo < hi) { const int mid = (lo + hi) / 2; if (ax[mid] > rest) hi = mid; else lo = mid + 1; } count = L - lo; }
                    else if (normal[c][0] < 0.f) { int lo = 0, hi = L; while (lo < hi) { const int mid = (lo + hi) / 2; if (ax[mid] > rest) lo = mid + 1; else hi = mid; } count = lo; }
                    else count = ax[0] > rest ? L : 0;
                    if (count) word = normal[c][0] > 0.f ? ~0u << (L - count) : ~0u >> (L - count);
                }
                m[k * L + j] = word;
            }
    }
    uint32_t gone[WORDS] = {};
    int *bound = new int[candidates]; // a candidate's gain at its last count: gains only fall as picks are made
    for (int c = 0; c < candidates; ++c) bound[c] = L * L * L;
    int n = 0, total = 0;
    while (n < RT_CLIP_MAX_PLANES) {
        int best = -1, bestGain = 0;
        for (int c = 0; c < candidates; ++c) {
            if (bound[c] <= bestGain) continue; // (cannot beat the best so far, which wins ties)
            const uint32_t *m = mask + (size_t)c * WORDS;
            int gain = 0;
            for (int i = 0; i < WORDS; ++i) gain += __builtin_popcount(m[i] & ~gone[i]);
            bound[c] = gain;
            if (gain > bestGain) { bestGain = gain; best = c; }
        }
        if (best < 0) break;
        const uint32_t *m = mask + (size_t)best * WORDS;
        for (int i = 0; i < WORDS; ++i) gone[i] |= m[i];
        kept[n++] = best;
        total += bestGain;
    }
    delete[] mask;
    delete[] bound;
    if (total * 20 < L * L * L) n = 0, total = 0;
    if (cut) *cut = total;
    return n;
}

// The `plain` ray of segments_of and of the clip: no far end, no zero direction component, an exit te and first heads hx, hy, hz that are
// all ordinary numbers, the first crossing before the exit.
RT_CLIP_HD bool rt_clip_plain(bool farEnd, float dx, float dy, float dz, float te, float hx, float hy, float hz)
{
    const float inf = __builtin_inff();
    const float ta = __builtin_fminf(hx, __builtin_fminf(hy, hz));
    return !farEnd && dx != 0.f && dy != 0.f && dz != 0.f && te < inf && -inf < ta && ta < te && hx == hx && hy == hy && hz == hz && hx < inf &&
           hy < inf && hz < inf;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define RT_CLIP_RCP(x) __builtin_amdgcn_rcpf(x)
#else
#define RT_CLIP_RCP(x) (1.f / (x))
#endif

// One kept plane {nx, ny, nz, off} against the ray o + t d of range (tmin, te): the lowered te, or te itself.  A plane the ray does not
// cross outwards (n.d <= 0), crosses at or before tmin (an origin beyond it), or crosses behind te leaves te alone; so does every NaN.
RT_CLIP_HD float rt_clip_plane(float nx, float ny, float nz, float off, float ox, float oy, float oz, float dx, float dy, float dz, float tmin, float te)
{
    const float nd = nx * dx + ny * dy + nz * dz;
    if (!(nd > 0.f)) return te;
    const float ax = nx * ox, ay = ny * oy, az = nz * oz;
    float num = off - (ax + ay + az);
    num += RT_CLIP_SLACK_ABS * (__builtin_fabsf(off) + __builtin_fabsf(ax) + __builtin_fabsf(ay) + __builtin_fabsf(az));
    float t = num * RT_CLIP_RCP(nd);
    t += RT_CLIP_SLACK_REL * __builtin_fabsf(t);
    return (tmin < t && t < te) ? t : te;
}

// every plane of `clip` (the buffer's fields from RT_CLIP_AT on: count, pad, planes): P = a pointer type that reads floats
template <class P> RT_CLIP_HD float rt_clip_te(P clip, uint32_t count, float ox, float oy, float oz, float dx, float dy, float dz, float tmin, float te)
{
    for (uint32_t k = 0; k < count; ++k) {
        const int at = (RT_CLIP_PLANES_AT - RT_CLIP_AT) + 4 * (int)k;
        te = rt_clip_plane(clip[at], clip[at + 1], clip[at + 2], clip[at + 3], ox, oy, oz, dx, dy, dz, tmin, te);
    }
    return te;
}

// The clip of one planned ray: hx, hy, hz = its first heads, te = its exit from the grid's box, startInside = its start point o + tmin d lies
// in the grid's box (a ray that starts outside is moved onto the box, or misses it and walks a path of its own: the argument above wants the
// walk's cells to lie on the ray).  Lowers te and returns true when the ray is plain and a plane applies; the walk then ends in the cell of
// o + te d.
template <class P> RT_CLIP_HD bool rt_clip_ray(P clip, uint32_t count, bool farEnd, bool startInside, float ox, float oy, float oz, float dx, float dy, float dz,
                                               float tmin, float hx, float hy, float hz, float &te)
{
    if (count == 0u || !startInside || !rt_clip_plain(farEnd, dx, dy, dz, te, hx, hy, hz)) return false;
    const float lowered = rt_clip_te(clip, count, ox, oy, oz, dx, dy, dz, tmin, te);
    if (!(lowered < te)) return false;
    te = lowered;
    return true;
}

#endif
