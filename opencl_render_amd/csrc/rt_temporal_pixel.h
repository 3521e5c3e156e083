// rt_temporal_pixel.h -- one pixel of the temporal accumulation (include/raytrace_hip.h, "TEMPORAL ACCUMULATION"), in the header's order of
// operations.  rtt_accumulate_kernel (rt_temporal.hip) runs it per lane; tests/temporal_host.cpp compiles the same text for the host with
// the same exactness flags, so that the definition is checked against tests/temporal_oracle.py where there is no GPU.
#ifndef RT_TEMPORAL_PIXEL_H
#define RT_TEMPORAL_PIXEL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RTT_FN __device__ __forceinline__
#else
#define RTT_FN static inline
#endif

struct RttArgs {
    uint32_t W, H, blocksX;
    float maxHistory, depthTolerance;
    const float *colour, *motion, *prevT;
    const uint32_t *triangle;
    const float *histColour, *histCount, *histT;
    const uint32_t *histTriangle;
    float *outColour, *outCount; // outCount may be null
};

// Pixel (x, y) of a W x H image, x < W and y < H.
RTT_FN void rtt_pixel(const RttArgs &A, const uint32_t x, const uint32_t y)
{
    const uint32_t W = A.W, H = A.H;
    const size_t p = (size_t)y * W + x;
    const float cr = A.colour[3 * p], cg = A.colour[3 * p + 1], cb = A.colour[3 * p + 2];
    const float mx = A.motion[2 * p], my = A.motion[2 * p + 1]; // (two 4-byte loads: the array need not be 8-byte aligned)
    const float prevT = A.prevT[p];
    const uint32_t tri = A.triangle[p];
    const float gx = (((float)x + 0.5f) + mx) - 0.5f, gy = (((float)y + 0.5f) + my) - 0.5f;
    const bool ok = prevT > 0.f && gx >= -1.0f && gx < (float)W && gy >= -1.0f && gy < (float)H; // (NaN compares false)
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sn = 0.f;
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
                }
            }
        }
    }
    float orr = cr, og = cg, ob = cb, n = 1.0f;
    if (ok && sw > 0.f) {
        const float hr = sr / sw, hg = sg / sw, hb = sb / sw, hn = sn / sw;
        n = hn + 1.0f;
        if (n > A.maxHistory) n = A.maxHistory;
        if (n != 1.0f) { // (n = 1, which only maxHistory = 1 gives, keeps the frame: hc + (c - hc) rounds twice and need not return c)
            const float a = 1.0f / n;
            orr = hr + (cr - hr) * a;
            og = hg + (cg - hg) * a;
            ob = hb + (cb - hb) * a;
        }
    }
    A.outColour[3 * p] = orr;
    A.outColour[3 * p + 1] = og;
    A.outColour[3 * p + 2] = ob;
    if (A.outCount) A.outCount[p] = n;
}

#endif
