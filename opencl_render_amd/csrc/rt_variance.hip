// rt_variance.hip -- the variance-guided filter of include/raytrace_hip.h ("VARIANCE-GUIDED FILTER"): luminance moments accumulated along
// the temporal reprojection, a per-pixel variance estimate from them, and an a-trous filter whose luminance edge-stop is scaled by the
// local variance and which carries the variance through its iterations (Schied et al. 2017), in the exact fp32 arithmetic the header
// fixes (tests/variance_oracle.py is the same definition in numpy).  The per-pixel arithmetic is rt_variance_pixel.h's.
//
// Kernels, in launch order (rt_filters.cpp issues them on one stream):
//   rtv_moments_kernel    rtt_accumulate_kernel's layout (a wave is one 8x8 block of the screen), with the two moments on the same taps
//   rtv_guide_kernel      row-major normal and albedo -> the packed guides G0 = (n^.xyz, z ? 1 : 0), G1 = (albedo.rgb, 0)
//   rtv_estimate_kernel   colour, moments, count and guides -> the state S^0 = (C^0.rgb, V^0) as float4.  A 16x16 workgroup stages the 22x22
//                         patch its 7x7 windows reach (both guides and the moments, 40 B each, 19.4 KB) in LDS; a workgroup whose pixels
//                         are all on the temporal arm stages nothing
//   rtv_il_kernel         per iteration: il = 1 / (ls * (3x3 Gaussian of V^i) + floor) per pixel; the 3x3 lies off the iteration's
//                         residue lattice for h > 1, so it is a pass of its own (9 neighbouring loads, 4 B written per pixel)
//   rtv_iter_lds_kernel   one iteration S^i -> S^(i+1), 25 taps at spacing h = 2^i <= 64: rtd_iter_lds_kernel's residue-lattice scheme, a
//                         20x20 patch of one lattice in LDS; V rides in the colour's .w, so the patch is no larger than the denoiser's
//   rtv_iter_kernel       the same for h > 64: every tap a global load
//   rtv_output_kernel     S^K -> row-major f32 colour, the variance and, optionally, the quantised u16 planes
// Nothing here may change a bit: no fast math, no reciprocal-multiply, no contraction (the Makefile's exactness flags apply).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rt_launch.h"
#include "rt_variance_pixel.h"

namespace {

constexpr uint32_t PATCH = 16;    // 16x16 pixels per workgroup of the estimate and iteration kernels
constexpr int RTV_LDS_MAX_H = 64; // up to this dilation the iterations stage a lattice patch in LDS
constexpr int LAT = PATCH + 4;    // the iteration's patch: two lattice points on every side
constexpr int WIN = PATCH + 6;    // the estimate's patch: three pixels on every side

__global__ __launch_bounds__(256) void rtv_moments_kernel(const RtvMomentArgs A)
{
    const uint32_t bx = blockIdx.x % A.blocksX, by = blockIdx.x / A.blocksX;
    const uint32_t wave = threadIdx.x >> 6, in = threadIdx.x & 63u;
    const uint32_t x = bx * 32u + wave * 8u + (in & 7u), y = by * 8u + (in >> 3);
    if (x >= A.W || y >= A.H) return;
    rtv_moments_pixel(A, x, y);
}

__global__ __launch_bounds__(256) void rtv_guide_kernel(uint32_t n, const float *__restrict__ normal, const float *__restrict__ albedo,
                                                        float4 *__restrict__ g0, float4 *__restrict__ g1)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const size_t b = (size_t)i * 3;
    g0[i] = rtv_guide_normal(normal[b], normal[b + 1], normal[b + 2]);
    g1[i] = make_float4(albedo[b], albedo[b + 1], albedo[b + 2], 0.f);
}

// The moments and count of pixel q: the given arrays, or (both null) the single frame's (lum, lum*lum) and 1.
__device__ __forceinline__ void rtv_load_moments(const float *__restrict__ colour, const float *__restrict__ moments, uint32_t q, float &m1,
                                                 float &m2)
{
    if (moments) {
        m1 = moments[2 * (size_t)q];
        m2 = moments[2 * (size_t)q + 1];
    } else {
        const size_t b = (size_t)q * 3;
        const float l = rtv_lum(colour[b], colour[b + 1], colour[b + 2]);
        m1 = l;
        m2 = l * l;
    }
}

__global__ __launch_bounds__(256) void rtv_estimate_kernel(uint32_t W, uint32_t H, uint32_t patchesX, float spatialBelow, float ia, uint32_t E,
                                                           const float *__restrict__ colour, const float *__restrict__ moments,
                                                           const float *__restrict__ count, const float4 *__restrict__ g0,
                                                           const float4 *__restrict__ g1, float4 *__restrict__ s0)
{
    __shared__ float4 sn[WIN * WIN], sa[WIN * WIN];
    __shared__ float2 sm[WIN * WIN];
    const int x0 = (int)((blockIdx.x % patchesX) * PATCH), y0 = (int)((blockIdx.x / patchesX) * PATCH);
    const int tx = threadIdx.x % PATCH, ty = threadIdx.x / PATCH;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < (int)W && y < (int)H;
    const uint32_t p = inside ? (uint32_t)y * W + (uint32_t)x : 0u;
    float m1 = 0.f, m2 = 0.f, cnt = 1.0f;
    if (inside) {
        rtv_load_moments(colour, moments, p, m1, m2);
        if (count) cnt = count[p];
    }
    const bool spatial = inside && !(cnt >= spatialBelow);
    float v = 0.f;
    if (__syncthreads_or(spatial)) { // (every thread of the workgroup comes here)
        for (int i = threadIdx.x; i < WIN * WIN; i += 256) {
            const int qx = x0 + i % WIN - 3, qy = y0 + i / WIN - 3;
            if (qx >= 0 && qx < (int)W && qy >= 0 && qy < (int)H) { // points outside the image are never read: their taps are skipped
                const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
                sn[i] = g0[q];
                sa[i] = g1[q];
                float q1, q2;
                rtv_load_moments(colour, moments, q, q1, q2);
                sm[i] = make_float2(q1, q2);
            }
        }
        __syncthreads();
        if (inside) {
            const int l = (ty + 3) * WIN + tx + 3;
            v = rtv_estimate_pixel(W, H, x, y, m1, m2, cnt, spatialBelow, ia, E, sn[l], sa[l],
                                   [&](int dx, int dy, float4 &nq, float4 &aq, float &q1, float &q2) {
                                       const int lq = l + dy * WIN + dx;
                                       nq = sn[lq];
                                       aq = sa[lq];
                                       const float2 m = sm[lq];
                                       q1 = m.x;
                                       q2 = m.y;
                                   });
        }
    } else if (inside) {
        v = rtv_variance(m1, m2);
    }
    if (inside) {
        const size_t b = (size_t)p * 3;
        s0[p] = make_float4(colour[b], colour[b + 1], colour[b + 2], v);
    }
}

__global__ __launch_bounds__(256) void rtv_il_kernel(uint32_t W, uint32_t H, uint32_t patchesX, float ls, float floor_,
                                                     const float4 *__restrict__ sin, float *__restrict__ il)
{
    const int x = (int)((blockIdx.x % patchesX) * PATCH + threadIdx.x % PATCH), y = (int)((blockIdx.x / patchesX) * PATCH + threadIdx.x / PATCH);
    if (x >= (int)W || y >= (int)H) return;
    const uint32_t p = (uint32_t)y * W + (uint32_t)x;
    il[p] = rtv_il_pixel(W, H, x, y, ls, floor_, [&](int dx, int dy) { return sin[(uint32_t)(y + dy) * W + (uint32_t)(x + dx)].w; });
}

// Large h: one thread per pixel of a 16x16 patch, every tap a 16-byte load from global memory (L2 / Infinity Cache).
__global__ __launch_bounds__(256) void rtv_iter_kernel(uint32_t W, uint32_t H, uint32_t patchesX, int h, float ia, uint32_t E,
                                                       const float4 *__restrict__ sin, const float *__restrict__ il,
                                                       const float4 *__restrict__ g0, const float4 *__restrict__ g1, float4 *__restrict__ sout)
{
    const uint32_t px = blockIdx.x % patchesX, py = blockIdx.x / patchesX;
    const int x = (int)(px * PATCH + (threadIdx.x % PATCH)), y = (int)(py * PATCH + (threadIdx.x / PATCH));
    if (x >= (int)W || y >= (int)H) return;
    const uint32_t p = (uint32_t)y * W + (uint32_t)x;
    sout[p] = rtv_iter_pixel(W, H, x, y, h, il[p], ia, E, sin[p], g0[p], g1[p], [&](int j, int k, float4 &cq, float4 &nq, float4 &aq) {
        const uint32_t q = (uint32_t)(y + (j - 2) * h) * W + (uint32_t)(x + (k - 2) * h);
        cq = sin[q];
        nq = g0[q];
        aq = g1[q];
    });
}

// Small h (<= RTV_LDS_MAX_H): the taps of pixel (x, y) lie on its residue lattice {(x + a h, y + b h)}, so a workgroup takes a 16x16
// patch of ONE lattice -- pixels (x0 + tx h, y0 + ty h) -- and stages the 20x20 lattice points its taps reach (state and both guides,
// 48 B each, 19.2 KB) in LDS once.  Workgroup b: residue (rx, ry) = b % (resX * resY), super-tile (sx, sy) = b / (resX * resY) of
// 16h x 16h pixels.
__global__ __launch_bounds__(256) void rtv_iter_lds_kernel(uint32_t W, uint32_t H, uint32_t superX, uint32_t resX, uint32_t resY, int h,
                                                           float ia, uint32_t E, const float4 *__restrict__ sin, const float *__restrict__ il,
                                                           const float4 *__restrict__ g0, const float4 *__restrict__ g1,
                                                           float4 *__restrict__ sout)
{
    __shared__ float4 sc[LAT * LAT], sn[LAT * LAT], sa[LAT * LAT];
    const uint32_t r = blockIdx.x % (resX * resY), s = blockIdx.x / (resX * resY);
    const int x0 = (int)((s % superX) * PATCH * (uint32_t)h + r % resX), y0 = (int)((s / superX) * PATCH * (uint32_t)h + r / resX);
    for (int i = threadIdx.x; i < LAT * LAT; i += 256) {
        const int qx = x0 + (i % LAT - 2) * h, qy = y0 + (i / LAT - 2) * h;
        if (qx >= 0 && qx < (int)W && qy >= 0 && qy < (int)H) { // points outside the image are never read: their taps are skipped
            const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
            sc[i] = sin[q];
            sn[i] = g0[q];
            sa[i] = g1[q];
        }
    }
    __syncthreads();
    const int tx = threadIdx.x % PATCH, ty = threadIdx.x / PATCH;
    const int x = x0 + tx * h, y = y0 + ty * h;
    if (x >= (int)W || y >= (int)H) return;
    const int l = (ty + 2) * LAT + tx + 2;
    const uint32_t p = (uint32_t)y * W + (uint32_t)x;
    sout[p] = rtv_iter_pixel(W, H, x, y, h, il[p], ia, E, sc[l], sn[l], sa[l], [&](int j, int k, float4 &cq, float4 &nq, float4 &aq) {
        const int lq = (ty + j) * LAT + tx + k;
        cq = sc[lq];
        nq = sn[lq];
        aq = sa[lq];
    });
}

__global__ __launch_bounds__(256) void rtv_output_kernel(uint32_t n, const float4 *__restrict__ s, float *__restrict__ out,
                                                         float *__restrict__ outVariance, uint16_t *__restrict__ outR,
                                                         uint16_t *__restrict__ outG, uint16_t *__restrict__ outB)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 v = s[i];
    if (out) {
        const size_t b = (size_t)i * 3;
        out[b] = v.x;
        out[b + 1] = v.y;
        out[b + 2] = v.z;
    }
    if (outVariance) outVariance[i] = v.w;
    if (outR) {
        const float q[3] = { v.x * 65535.0f, v.y * 65535.0f, v.z * 65535.0f };
        uint16_t u[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            u[ch] = !(q[ch] > 0.f) ? (uint16_t)0 : (q[ch] >= 65534.5f ? (uint16_t)65535 : (uint16_t)(q[ch] + 0.5f));
        outR[i] = u[0];
        outG[i] = u[1];
        outB[i] = u[2];
    }
}

} // namespace

// The arrays were checked by the caller (rt_filters.cpp): W x H each, W, H in 1..16384, W*H <= 2^27, the outputs overlap nothing.
extern "C" hipError_t rtv_launch_moments(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *prevT,
                                         const uint32_t *triangle, const float *histColour, const float *histCount, const float *histT,
                                         const uint32_t *histTriangle, const float *histMoments, float *outColour, float *outCount,
                                         float *outMoments, float *outVariance, float maxHistory, float depthTolerance, hipStream_t stream)
{
    RtvMomentArgs A;
    A.W = W; A.H = H; A.blocksX = (W + 31u) / 32u;
    A.maxHistory = maxHistory; A.depthTolerance = depthTolerance;
    A.colour = colour; A.motion = motion; A.prevT = prevT; A.triangle = triangle;
    A.histColour = histColour; A.histCount = histCount; A.histT = histT; A.histTriangle = histTriangle; A.histMoments = histMoments;
    A.outColour = outColour; A.outCount = outCount; A.outMoments = outMoments; A.outVariance = outVariance;
    hipLaunchKernelGGL(rtv_moments_kernel, dim3(A.blocksX * ((H + 7u) / 8u)), dim3(256), 0, stream, A);
    return hipGetLastError();
}

// Guides and S^0.  moments and count: both given or both null (the single-frame use).
extern "C" hipError_t rtv_launch_estimate(uint32_t W, uint32_t H, const float *colour, const float *normal, const float *albedo,
                                          const float *moments, const float *count, float spatialBelow, float ia, uint32_t E, void *s0,
                                          void *g0, void *g1, hipStream_t stream)
{
    const uint32_t n = W * H;
    hipLaunchKernelGGL(rtv_guide_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, normal, albedo, reinterpret_cast<float4 *>(g0),
                       reinterpret_cast<float4 *>(g1));
    const uint32_t patchesX = (W + PATCH - 1) / PATCH, patchesY = (H + PATCH - 1) / PATCH;
    hipLaunchKernelGGL(rtv_estimate_kernel, dim3(patchesX * patchesY), dim3(256), 0, stream, W, H, patchesX, spatialBelow, ia, E, colour, moments,
                       count, reinterpret_cast<const float4 *>(g0), reinterpret_cast<const float4 *>(g1), reinterpret_cast<float4 *>(s0));
    return hipGetLastError();
}

extern "C" hipError_t rtv_launch_iteration(uint32_t W, uint32_t H, int h, float ls, float floor_, float ia, uint32_t E, const void *sin,
                                           void *il, const void *g0, const void *g1, void *sout, hipStream_t stream)
{
    const float4 *c = reinterpret_cast<const float4 *>(sin), *n = reinterpret_cast<const float4 *>(g0), *a = reinterpret_cast<const float4 *>(g1);
    float4 *o = reinterpret_cast<float4 *>(sout);
    float *l = reinterpret_cast<float *>(il);
    const uint32_t patchesX = (W + PATCH - 1) / PATCH, patchesY = (H + PATCH - 1) / PATCH;
    hipLaunchKernelGGL(rtv_il_kernel, dim3(patchesX * patchesY), dim3(256), 0, stream, W, H, patchesX, ls, floor_, c, l);
    if (h <= RTV_LDS_MAX_H) {
        const uint32_t span = PATCH * (uint32_t)h;
        const uint32_t superX = (W + span - 1) / span, superY = (H + span - 1) / span;
        const uint32_t resX = W < (uint32_t)h ? W : (uint32_t)h, resY = H < (uint32_t)h ? H : (uint32_t)h;
        hipLaunchKernelGGL(rtv_iter_lds_kernel, dim3(superX * superY * resX * resY), dim3(256), 0, stream, W, H, superX, resX, resY, h, ia, E, c, l,
                           n, a, o);
    } else {
        hipLaunchKernelGGL(rtv_iter_kernel, dim3(patchesX * patchesY), dim3(256), 0, stream, W, H, patchesX, h, ia, E, c, l, n, a, o);
    }
    return hipGetLastError();
}

extern "C" hipError_t rtv_launch_output(uint32_t n, const void *s, float *out, float *outVariance, uint16_t *outR, uint16_t *outG,
                                        uint16_t *outB, hipStream_t stream)
{
    hipLaunchKernelGGL(rtv_output_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, reinterpret_cast<const float4 *>(s), out, outVariance,
                       outR, outG, outB);
    return hipGetLastError();
}
