// rt_denoise.hip -- the denoiser of include/raytrace_hip.h ("DENOISER"): an edge-avoiding a-trous wavelet filter guided by the normal
// and albedo passes, in the exact fp32 arithmetic the header fixes (tests/denoise_oracle.py is the same definition in numpy).
//
// Kernels, in launch order (rt_filters.cpp issues them on one stream):
//   rtd_gather_kernel    scene path only: the [slot][R,G,B][128*128] u16 tile buffer and the [slot][nx ny nz ar ag ab][128*128] surface
//                        sums -> row-major W x H x 3 f32 colour (u16 / 65535), normal and albedo (sum / S)
//   rtd_guide_kernel     row-major inputs -> C^0 as float4 (padded, so every later colour load is one 16-byte load) and the packed
//                        guides G0 = (n^.xyz, z ? 1 : 0), G1 = (albedo.rgb, 0)
//   rtd_iter_lds_kernel  one a-trous iteration, C^i -> C^(i+1), 25 taps at spacing h = 2^i, for h <= 64: a workgroup stages a 20x20
//                        patch of one residue lattice in LDS (below)
//   rtd_iter_kernel      the same for h > 64: every tap a global load
//   rtd_output_kernel    C^K -> row-major f32 and, optionally, the quantised u16 planes
// Nothing here may change a bit: no fast math, no reciprocal-multiply, no contraction (the Makefile's exactness flags apply).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rt_launch.h"

namespace {

constexpr uint32_t PATCH = 16; // 16x16 pixels per workgroup of the iteration kernels
constexpr int RTD_LDS_MAX_H = 64; // up to this dilation the iterations stage a lattice patch in LDS (rtd_iter_lds_kernel)

__global__ __launch_bounds__(256) void rtd_guide_kernel(uint32_t n, const float *__restrict__ colour, const float *__restrict__ normal,
                                                        const float *__restrict__ albedo, float4 *__restrict__ c0,
                                                        float4 *__restrict__ g0, float4 *__restrict__ g1)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const size_t b = (size_t)i * 3;
    c0[i] = make_float4(colour[b], colour[b + 1], colour[b + 2], 0.f);
    const float nx = normal[b], ny = normal[b + 1], nz = normal[b + 2];
    const float m = (nx * nx + ny * ny) + nz * nz;
    if (m > 0.f) {
        const float r = sqrtf(m);
        g0[i] = make_float4(nx / r, ny / r, nz / r, 0.f);
    } else {
        g0[i] = make_float4(0.f, 0.f, 0.f, 1.f);
    }
    g1[i] = make_float4(albedo[b], albedo[b + 1], albedo[b + 2], 0.f);
}

// One tap of the header's loop, in its order of operations (both iteration kernels call this, so they compute the same bits).
__device__ __forceinline__ void rtd_tap(const float4 cp, const float4 np_, const float4 ap, bool zp, const float4 cq, const float4 nq,
                                        const float4 aq, float bb, float ic, float ia, uint32_t E, float &sw, float &sr, float &sg, float &sb)
{
    const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
    const float dc = (dr * dr + dg * dg) + db * db;
    const float er = ap.x - aq.x, eg = ap.y - aq.y, eb = ap.z - aq.z;
    const float da = (er * er + eg * eg) + eb * eb;
    float wn;
    if (zp && nq.w != 0.f) {
        wn = 1.f;
    } else {
        float d = (np_.x * nq.x + np_.y * nq.y) + np_.z * nq.z;
        d = d > 0.f ? d : 0.f;
        for (uint32_t e = 0; e < E; ++e) d = d * d;
        wn = d;
    }
    const float w = (bb * wn) / ((1.f + dc * ic) * (1.f + da * ia));
    sw = sw + w;
    sr = sr + w * cq.x;
    sg = sg + w * cq.y;
    sb = sb + w * cq.z;
}

// Large h: one thread per pixel of a 16x16 patch, every tap a 16-byte load from global memory (L2 / Infinity Cache).
__global__ __launch_bounds__(256) void rtd_iter_kernel(uint32_t W, uint32_t H, uint32_t patchesX, int h, float ic, float ia, uint32_t E,
                                                       const float4 *__restrict__ cin, const float4 *__restrict__ g0,
                                                       const float4 *__restrict__ g1, float4 *__restrict__ cout)
{
    const uint32_t px = blockIdx.x % patchesX, py = blockIdx.x / patchesX;
    const int x = (int)(px * PATCH + (threadIdx.x % PATCH)), y = (int)(py * PATCH + (threadIdx.x / PATCH));
    if (x >= (int)W || y >= (int)H) return;
    const uint32_t p = (uint32_t)y * W + (uint32_t)x;
    const float4 cp = cin[p], np_ = g0[p], ap = g1[p];
    const bool zp = np_.w != 0.f;
    const float B[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int qy = y + (j - 2) * h;
        if (qy < 0 || qy >= (int)H) continue;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int qx = x + (k - 2) * h;
            if (qx < 0 || qx >= (int)W) continue;
            const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
            rtd_tap(cp, np_, ap, zp, cin[q], g0[q], g1[q], B[j] * B[k], ic, ia, E, sw, sr, sg, sb);
        }
    }
    cout[p] = sw > 0.f ? make_float4(sr / sw, sg / sw, sb / sw, 0.f) : cp;
}

// Small h (<= RTD_LDS_MAX_H): the taps of pixel (x, y) lie on its residue lattice {(x + a h, y + b h)}, so a workgroup takes a 16x16
// patch of ONE lattice -- pixels (x0 + tx h, y0 + ty h) -- and stages the 20x20 lattice points its taps reach (colour and both guides,
// 48 B each, 19.2 KB) in LDS once: 1.56 global loads per pixel and array instead of 25.  Workgroup b: residue (rx, ry) = b % (resX *
// resY), super-tile (sx, sy) = b / (resX * resY) of 16h x 16h pixels.
constexpr int LAT = PATCH + 4;
__global__ __launch_bounds__(256) void rtd_iter_lds_kernel(uint32_t W, uint32_t H, uint32_t superX, uint32_t resX, uint32_t resY, int h,
                                                           float ic, float ia, uint32_t E, const float4 *__restrict__ cin,
                                                           const float4 *__restrict__ g0, const float4 *__restrict__ g1,
                                                           float4 *__restrict__ cout)
{
    __shared__ float4 sc[LAT * LAT], sn[LAT * LAT], sa[LAT * LAT];
    const uint32_t r = blockIdx.x % (resX * resY), s = blockIdx.x / (resX * resY);
    const int x0 = (int)((s % superX) * PATCH * (uint32_t)h + r % resX), y0 = (int)((s / superX) * PATCH * (uint32_t)h + r / resX);
    for (int i = threadIdx.x; i < LAT * LAT; i += 256) {
        const int qx = x0 + (i % LAT - 2) * h, qy = y0 + (i / LAT - 2) * h;
        if (qx >= 0 && qx < (int)W && qy >= 0 && qy < (int)H) { // points outside the image are never read: their taps are skipped
            const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
            sc[i] = cin[q];
            sn[i] = g0[q];
            sa[i] = g1[q];
        }
    }
    __syncthreads();
    const int tx = threadIdx.x % PATCH, ty = threadIdx.x / PATCH;
    const int x = x0 + tx * h, y = y0 + ty * h;
    if (x >= (int)W || y >= (int)H) return;
    const int l = (ty + 2) * LAT + tx + 2;
    const float4 cp = sc[l], np_ = sn[l], ap = sa[l];
    const bool zp = np_.w != 0.f;
    const float B[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int qy = y + (j - 2) * h;
        if (qy < 0 || qy >= (int)H) continue;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int qx = x + (k - 2) * h;
            if (qx < 0 || qx >= (int)W) continue;
            const int lq = (ty + j) * LAT + tx + k;
            rtd_tap(cp, np_, ap, zp, sc[lq], sn[lq], sa[lq], B[j] * B[k], ic, ia, E, sw, sr, sg, sb);
        }
    }
    cout[(uint32_t)y * W + (uint32_t)x] = sw > 0.f ? make_float4(sr / sw, sg / sw, sb / sw, 0.f) : cp;
}

__global__ __launch_bounds__(256) void rtd_output_kernel(uint32_t n, const float4 *__restrict__ c, float *__restrict__ out,
                                                         uint16_t *__restrict__ outR, uint16_t *__restrict__ outG, uint16_t *__restrict__ outB)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 v = c[i];
    if (out) {
        const size_t b = (size_t)i * 3;
        out[b] = v.x;
        out[b + 1] = v.y;
        out[b + 2] = v.z;
    }
    if (outR) {
        const float s[3] = { v.x * 65535.0f, v.y * 65535.0f, v.z * 65535.0f };
        uint16_t u[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            u[ch] = !(s[ch] > 0.f) ? (uint16_t)0 : (s[ch] >= 65534.5f ? (uint16_t)65535 : (uint16_t)(s[ch] + 0.5f));
        outR[i] = u[0];
        outG[i] = u[1];
        outB[i] = u[2];
    }
}

// One thread per pixel slot of the instance's tiles (tile-major, like tileBuf); slots past the image's edge write nothing.  tileIds were
// checked against the tile count when the scene was built.
__global__ __launch_bounds__(256) void rtd_gather_kernel(uint32_t W, uint32_t H, uint32_t tilesX, const uint32_t *__restrict__ tileIds,
                                                         const uint16_t *__restrict__ tileBuf, const float *__restrict__ surf, float S,
                                                         float *__restrict__ colour, float *__restrict__ normal, float *__restrict__ albedo)
{
    const uint32_t slot = blockIdx.x / 64u, l = (blockIdx.x % 64u) * 256u + threadIdx.x;
    const uint32_t t = tileIds[slot];
    const uint32_t gx = (t % tilesX) * 128u + (l % 128u), gy = (t / tilesX) * 128u + (l / 128u);
    if (gx >= W || gy >= H) return;
    const size_t o = ((size_t)gy * W + gx) * 3;
    const uint16_t *tb = tileBuf + (size_t)slot * 3 * 16384u + l;
    const float *sf = surf + (size_t)slot * 6 * 16384u + l;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        colour[o + c] = (float)tb[c * 16384u] / 65535.0f;
        normal[o + c] = sf[c * 16384u] / S;
        albedo[o + c] = sf[(3 + c) * 16384u] / S;
    }
}

} // namespace

extern "C" hipError_t rtd_launch_guides(uint32_t n, const float *colour, const float *normal, const float *albedo, void *c0, void *g0, void *g1,
                                        hipStream_t stream)
{
    hipLaunchKernelGGL(rtd_guide_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, colour, normal, albedo,
                       reinterpret_cast<float4 *>(c0), reinterpret_cast<float4 *>(g0), reinterpret_cast<float4 *>(g1));
    return hipGetLastError();
}

extern "C" hipError_t rtd_launch_iteration(uint32_t W, uint32_t H, int h, float ic, float ia, uint32_t E, const void *cin, const void *g0,
                                           const void *g1, void *cout, hipStream_t stream)
{
    const float4 *c = reinterpret_cast<const float4 *>(cin), *n = reinterpret_cast<const float4 *>(g0), *a = reinterpret_cast<const float4 *>(g1);
    float4 *o = reinterpret_cast<float4 *>(cout);
    if (h <= RTD_LDS_MAX_H) {
        const uint32_t span = PATCH * (uint32_t)h;
        const uint32_t superX = (W + span - 1) / span, superY = (H + span - 1) / span;
        const uint32_t resX = W < (uint32_t)h ? W : (uint32_t)h, resY = H < (uint32_t)h ? H : (uint32_t)h;
        hipLaunchKernelGGL(rtd_iter_lds_kernel, dim3(superX * superY * resX * resY), dim3(256), 0, stream, W, H, superX, resX, resY, h, ic, ia, E,
                           c, n, a, o);
    } else {
        const uint32_t patchesX = (W + PATCH - 1) / PATCH, patchesY = (H + PATCH - 1) / PATCH;
        hipLaunchKernelGGL(rtd_iter_kernel, dim3(patchesX * patchesY), dim3(256), 0, stream, W, H, patchesX, h, ic, ia, E, c, n, a, o);
    }
    return hipGetLastError();
}

extern "C" hipError_t rtd_launch_output(uint32_t n, const void *c, float *out, uint16_t *outR, uint16_t *outG, uint16_t *outB, hipStream_t stream)
{
    hipLaunchKernelGGL(rtd_output_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, reinterpret_cast<const float4 *>(c), out, outR,
                       outG, outB);
    return hipGetLastError();
}

extern "C" hipError_t rtd_launch_gather(uint32_t W, uint32_t H, uint32_t tilesX, const uint32_t *tileIds, uint32_t tileCount, const uint16_t *tileBuf,
                                        const float *surf, float S, float *colour, float *normal, float *albedo, hipStream_t stream)
{
    if (tileCount == 0) return hipSuccess;
    hipLaunchKernelGGL(rtd_gather_kernel, dim3(tileCount * 64u), dim3(256), 0, stream, W, H, tilesX, tileIds, tileBuf, surf, S, colour, normal,
                       albedo);
    return hipGetLastError();
}
