// rt_variance_pixel.h -- one pixel of each stage of the variance-guided filter (include/raytrace_hip.h, "VARIANCE-GUIDED FILTER"), in the
// header's order of operations: (a) the moments accumulation, (b) the variance estimate, (c) the prefilter and the guided iteration.
// The kernels of rt_variance.hip run these per lane; where a neighbour comes from (LDS or global memory) is the caller's `fetch`, so both
// of a stage's kernels compute the same bits.  tests/variance_host.cpp compiles the same text for the host with the same exactness flags,
// so that the definition is checked against tests/variance_oracle.py where there is no GPU.
#ifndef RT_VARIANCE_PIXEL_H
#define RT_VARIANCE_PIXEL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RTV_FN __device__ __forceinline__
typedef float4 rtv_f4;
#else
#define RTV_FN static inline
struct alignas(16) rtv_f4 {
    float x, y, z, w;
};
#endif

RTV_FN rtv_f4 rtv_make4(float x, float y, float z, float w)
{
    rtv_f4 v;
    v.x = x; v.y = y; v.z = z; v.w = w;
    return v;
}

RTV_FN float rtv_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// max(m2 - m1*m1, 0); a NaN gives 0
RTV_FN float rtv_variance(float m1, float m2)
{
    const float v = m2 - m1 * m1;
    return v > 0.f ? v : 0.f;
}

// ---- (a) moments accumulation: TEMPORAL ACCUMULATION's pixel (rt_temporal_pixel.h, restated: that kernel's instructions stay as they
// are) with the two luminance moments carried along the same taps ------------------------------------------------------------------
struct RtvMomentArgs {
    uint32_t W, H, blocksX;
    float maxHistory, depthTolerance;
    const float *colour, *motion, *prevT;
    const uint32_t *triangle;
    const float *histColour, *histCount, *histT;
    const uint32_t *histTriangle;
    const float *histMoments;
    float *outColour, *outCount, *outMoments, *outVariance; // outCount and outVariance may be null
};

// Pixel (x, y) of a W x H image, x < W and y < H.
RTV_FN void rtv_moments_pixel(const RtvMomentArgs &A, const uint32_t x, const uint32_t y)
{
    const uint32_t W = A.W, H = A.H;
    const size_t p = (size_t)y * W + x;
    const float cr = A.colour[3 * p], cg = A.colour[3 * p + 1], cb = A.colour[3 * p + 2];
    const float mx = A.motion[2 * p], my = A.motion[2 * p + 1];
    const float prevT = A.prevT[p];
    const uint32_t tri = A.triangle[p];
    const float l = rtv_lum(cr, cg, cb), l2 = l * l;
    const float gx = (((float)x + 0.5f) + mx) - 0.5f, gy = (((float)y + 0.5f) + my) - 0.5f;
    const bool ok = prevT > 0.f && gx >= -1.0f && gx < (float)W && gy >= -1.0f && gy < (float)H; // (NaN compares false)
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sn = 0.f, s1 = 0.f, s2 = 0.f;
    if (ok) {
        const float x0f = floorf(gx), y0f = floorf(gy), ax = gx - x0f, ay = gy - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f; // in [-1, W-1] x [-1, H-1]: converted after the range test
        const float tol = A.depthTolerance * prevT;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int qy = y0 + j;
            if (qy < 0 || qy >= (int)H) continue;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int qx = x0 + k;
                if (qx < 0 || qx >= (int)W) continue;
                const size_t q = (size_t)qy * W + (size_t)qx;
                const float b = (k ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                const float hn = A.histCount[q], ht = A.histT[q];
                if (hn >= 1.0f && A.histTriangle[q] == tri && (ht == prevT || fabsf(ht - prevT) <= tol)) {
                    sw = sw + b;
                    sr = sr + b * A.histColour[3 * q];
                    sg = sg + b * A.histColour[3 * q + 1];
                    sb = sb + b * A.histColour[3 * q + 2];
                    sn = sn + b * hn;
                    s1 = s1 + b * A.histMoments[2 * q];
                    s2 = s2 + b * A.histMoments[2 * q + 1];
                }
            }
        }
    }
    float orr = cr, og = cg, ob = cb, n = 1.0f, m1 = l, m2 = l2;
    if (ok && sw > 0.f) {
        const float hr = sr / sw, hg = sg / sw, hb = sb / sw, hn = sn / sw, h1 = s1 / sw, h2 = s2 / sw;
        n = hn + 1.0f;
        if (n > A.maxHistory) n = A.maxHistory;
        if (n != 1.0f) {
            const float a = 1.0f / n;
            orr = hr + (cr - hr) * a;
            og = hg + (cg - hg) * a;
            ob = hb + (cb - hb) * a;
            m1 = h1 + (l - h1) * a;
            m2 = h2 + (l2 - h2) * a;
        }
    }
    A.outColour[3 * p] = orr;
    A.outColour[3 * p + 1] = og;
    A.outColour[3 * p + 2] = ob;
    if (A.outCount) A.outCount[p] = n;
    A.outMoments[2 * p] = m1;
    A.outMoments[2 * p + 1] = m2;
    if (A.outVariance) A.outVariance[p] = rtv_variance(m1, m2);
}

// ---- the guides, exactly the DENOISER block's ----------------------------------------------------------------------------------------
// G0 = (n^.xyz, z ? 1 : 0)
RTV_FN rtv_f4 rtv_guide_normal(float nx, float ny, float nz)
{
    const float m = (nx * nx + ny * ny) + nz * nz;
    if (m > 0.f) {
        const float r = sqrtf(m);
        return rtv_make4(nx / r, ny / r, nz / r, 0.f);
    }
    return rtv_make4(0.f, 0.f, 0.f, 1.f);
}

RTV_FN float rtv_wn(const rtv_f4 np_, bool zp, const rtv_f4 nq, uint32_t E)
{
    if (zp && nq.w != 0.f) return 1.f;
    float d = (np_.x * nq.x + np_.y * nq.y) + np_.z * nq.z;
    d = d > 0.f ? d : 0.f;
    for (uint32_t e = 0; e < E; ++e) d = d * d;
    return d;
}

RTV_FN float rtv_da(const rtv_f4 ap, const rtv_f4 aq)
{
    const float er = ap.x - aq.x, eg = ap.y - aq.y, eb = ap.z - aq.z;
    return (er * er + eg * eg) + eb * eb;
}

// ---- (b) the variance estimate V^0 of pixel (x, y) ---------------------------------------------------------------------------------------
// m1, m2, count: the pixel's own.  fetch(dx, dy, nq, aq, q1, q2) gives the guides and moments of the pixel at (x + dx, y + dy), which lies
// inside the image; it is called only on the spatial arm.
template <class Fetch>
RTV_FN float rtv_estimate_pixel(uint32_t W, uint32_t H, int x, int y, float m1, float m2, float count, float spatialBelow, float ia,
                                uint32_t E, const rtv_f4 np_, const rtv_f4 ap, const Fetch &fetch)
{
    if (count >= spatialBelow) return rtv_variance(m1, m2); // (a NaN count goes on)
    const bool zp = np_.w != 0.f;
    float sw = 0.f, s1 = 0.f, s2 = 0.f;
    for (int dy = -3; dy <= 3; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)H) continue;
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)W) continue;
            rtv_f4 nq, aq;
            float q1, q2;
            fetch(dx, dy, nq, aq, q1, q2);
            const float w = rtv_wn(np_, zp, nq, E) / (1.f + rtv_da(ap, aq) * ia);
            sw = sw + w;
            s1 = s1 + w * q1;
            s2 = s2 + w * q2;
        }
    }
    if (!(sw > 0.f)) return 0.f;
    const float M1 = s1 / sw, M2 = s2 / sw;
    const float v = rtv_variance(M1, M2);
    return v * (count >= 1.0f ? 4.0f / count : 4.0f);
}

// ---- (c) the prefilter: il of pixel (x, y) from the 3x3 Gaussian of V at spacing 1 -------------------------------------------------------
// fetchV(dx, dy) gives V of the pixel at (x + dx, y + dy), which lies inside the image.
template <class FetchV>
RTV_FN float rtv_il_pixel(uint32_t W, uint32_t H, int x, int y, float ls, float floor_, const FetchV &fetchV)
{
    const float G[3] = { 0.25f, 0.5f, 0.25f };
    float gs = 0.f, gw = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int qy = y + j - 1;
        if (qy < 0 || qy >= (int)H) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int qx = x + k - 1;
            if (qx < 0 || qx >= (int)W) continue;
            gs = gs + (G[j] * G[k]) * fetchV(k - 1, j - 1);
            gw = gw + G[j] * G[k];
        }
    }
    const float g = gs / gw; // (the centre tap is always inside: gw >= 1/4)
    return 1.0f / (ls * g + floor_);
}

// ---- (c) one guided iteration of pixel (x, y) at spacing h: (C, V)^i -> (C, V)^(i+1), V in .w ------------------------------------------
// fetch(j, k, cq, nq, aq) gives colour and guides of tap (j, k), the pixel at (x + (k-2)h, y + (j-2)h), which lies inside the image.
template <class Fetch>
RTV_FN rtv_f4 rtv_iter_pixel(uint32_t W, uint32_t H, int x, int y, int h, float il, float ia, uint32_t E, const rtv_f4 cp, const rtv_f4 np_,
                             const rtv_f4 ap, const Fetch &fetch)
{
    const bool zp = np_.w != 0.f;
    const float B[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    const float lp = rtv_lum(cp.x, cp.y, cp.z);
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int qy = y + (j - 2) * h;
        if (qy < 0 || qy >= (int)H) continue;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int qx = x + (k - 2) * h;
            if (qx < 0 || qx >= (int)W) continue;
            rtv_f4 cq, nq, aq;
            fetch(j, k, cq, nq, aq);
            const float dl = lp - rtv_lum(cq.x, cq.y, cq.z);
            const float w = ((B[j] * B[k]) * rtv_wn(np_, zp, nq, E)) / ((1.f + (dl * dl) * il) * (1.f + rtv_da(ap, aq) * ia));
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
            sv = sv + (w * w) * cq.w;
        }
    }
    return sw > 0.f ? rtv_make4(sr / sw, sg / sw, sb / sw, sv / (sw * sw)) : cp;
}

#endif
