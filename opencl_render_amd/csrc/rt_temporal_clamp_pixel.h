// rt_temporal_clamp_pixel.h -- one pixel of the clamped temporal accumulation (include/raytrace_hip.h, "TEMPORAL CLAMP"), in the header's
// order of operations: TEMPORAL ACCUMULATION's pixel (rt_temporal_pixel.h) and, with Moments, the moments accumulation's
// (rt_variance_pixel.h, (a)), both restated -- those kernels' instructions stay as they are -- with one insertion: before the blend the
// reprojected history colour is pulled into the colour box of the frame's 3x3 neighbourhood.  Where a neighbour's colour comes from (LDS
// or global memory) is the caller's `fetch`.  rtt_clamp_kernel (rt_temporal.hip) runs this per lane; tests/temporal_clamp_host.cpp compiles
// the same text for the host with the same exactness flags, so that the definition is checked against tests/temporal_clamp_oracle.py
// where there is no GPU.
#ifndef RT_TEMPORAL_CLAMP_PIXEL_H
#define RT_TEMPORAL_CLAMP_PIXEL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RTC_FN __device__ __forceinline__
#else
#define RTC_FN static inline
#endif

#define RTC_MINMAX 1u   // RT_HIP_CLAMP_MINMAX
#define RTC_VARIANCE 2u // RT_HIP_CLAMP_VARIANCE

struct RtcArgs {
    uint32_t W, H, blocksX;
    uint32_t mode; // 1, 2 or 3
    float gamma;
    float maxHistory, depthTolerance;
    const float *colour, *motion, *prevT;
    const uint32_t *triangle;
    const float *histColour, *histCount, *histT;
    const uint32_t *histTriangle;
    const float *histMoments;                               // Moments only
    float *outColour, *outCount, *outMoments, *outVariance; // outCount may be null; outMoments (Moments only), outVariance may be null
};

// The box [lo, hi] of one channel of pixel (x, y): the 3x3 taps in the header's order.  cnt: the number of taps inside the image.
// fetch(dx, dy, ch) gives channel ch of the frame's colour at (x + dx, y + dy), which lies inside the image.
template <class Fetch>
RTC_FN void rtc_box(uint32_t W, uint32_t H, uint32_t x, uint32_t y, int ch, float cnt, uint32_t mode, float gamma, const Fetch &fetch,
                    float &lo, float &hi)
{
    float s1 = 0.f, s2 = 0.f, mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = (int)y + dy;
        if (qy < 0 || qy >= (int)H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = (int)x + dx;
            if (qx < 0 || qx >= (int)W) continue;
            const float v = fetch(dx, dy, ch);
            s1 = s1 + v;
            s2 = s2 + v * v;
            if (v < mn) mn = v;
            if (v > mx) mx = v;
        }
    }
    const float mu = s1 / cnt, ex2 = s2 / cnt;
    float var = ex2 - mu * mu;
    var = var > 0.f ? var : 0.f;
    const float e = gamma * sqrtf(var);
    if (mode == RTC_MINMAX) {
        lo = mn;
        hi = mx;
    } else if (mode == RTC_VARIANCE) {
        lo = mu - e;
        hi = mu + e;
    } else {
        lo = mu - e > mn ? mu - e : mn;
        hi = mu + e < mx ? mu + e : mx;
    }
}

// Pixel (x, y) of a W x H image, x < W and y < H.
template <bool Moments, class Fetch>
RTC_FN void rtc_pixel(const RtcArgs &A, const uint32_t x, const uint32_t y, const Fetch &fetch)
{
    const uint32_t W = A.W, H = A.H;
    const size_t p = (size_t)y * W + x;
    const float c[3] = { fetch(0, 0, 0), fetch(0, 0, 1), fetch(0, 0, 2) };
    const float mx = A.motion[2 * p], my = A.motion[2 * p + 1]; // (two 4-byte loads: the array need not be 8-byte aligned)
    const float prevT = A.prevT[p];
    const uint32_t tri = A.triangle[p];
    const float l = (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2], l2 = l * l; // rtv_lum
    const float gx = (((float)x + 0.5f) + mx) - 0.5f, gy = (((float)y + 0.5f) + my) - 0.5f;
    const bool ok = prevT > 0.f && gx >= -1.0f && gx < (float)W && gy >= -1.0f && gy < (float)H; // (NaN compares false)
    float sw = 0.f, s[3] = { 0.f, 0.f, 0.f }, sn = 0.f, s1 = 0.f, s2 = 0.f;
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
                    s[0] = s[0] + b * A.histColour[3 * q];
                    s[1] = s[1] + b * A.histColour[3 * q + 1];
                    s[2] = s[2] + b * A.histColour[3 * q + 2];
                    sn = sn + b * hn;
                    if (Moments) {
                        s1 = s1 + b * A.histMoments[2 * q];
                        s2 = s2 + b * A.histMoments[2 * q + 1];
                    }
                }
            }
        }
    }
    float o[3] = { c[0], c[1], c[2] }, n = 1.0f, m1 = l, m2 = l2;
    if (ok && sw > 0.f) {
        const float hn = sn / sw;
        n = hn + 1.0f;
        if (n > A.maxHistory) n = A.maxHistory;
        if (n != 1.0f) { // (n = 1, which only maxHistory = 1 gives, keeps the frame: hc + (c - hc) rounds twice and need not return c)
            const float a = 1.0f / n;
            const float cnt = (float)((1u + (x > 0u) + (x + 1u < W)) * (1u + (y > 0u) + (y + 1u < H))); // 1, 2, 3, 4, 6 or 9
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float lo, hi;
                rtc_box(W, H, x, y, ch, cnt, A.mode, A.gamma, fetch, lo, hi);
                float h = s[ch] / sw;
                if (h < lo) h = lo; // the clamp: a NaN history colour passes both compares and stays
                if (h > hi) h = hi;
                o[ch] = h + (c[ch] - h) * a;
            }
            if (Moments) { // the moments are not clamped
                const float h1 = s1 / sw, h2 = s2 / sw;
                m1 = h1 + (l - h1) * a;
                m2 = h2 + (l2 - h2) * a;
            }
        }
    }
    A.outColour[3 * p] = o[0];
    A.outColour[3 * p + 1] = o[1];
    A.outColour[3 * p + 2] = o[2];
    if (A.outCount) A.outCount[p] = n;
    if (Moments) {
        A.outMoments[2 * p] = m1;
        A.outMoments[2 * p + 1] = m2;
        if (A.outVariance) {
            const float v = m2 - m1 * m1; // rtv_variance
            A.outVariance[p] = v > 0.f ? v : 0.f;
        }
    }
}

#endif
