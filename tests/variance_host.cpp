// The variance-guided filter's per-pixel code (opencl_render_amd/csrc/rt_variance_pixel.h, what the kernels of rt_variance.hip run per
// lane) compiled for the host: tests/test_variance.py builds this with the exactness flags of csrc/Makefile and compares it with
// variance_oracle.py.  Every neighbour comes from the row-major arrays, as in the kernels' global-memory paths.
#include "rt_variance_pixel.h"

#include <vector>

extern "C" void variance_host_moments(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *prevT,
                                      const uint32_t *triangle, const float *histColour, const float *histCount, const float *histT,
                                      const uint32_t *histTriangle, const float *histMoments, float *outColour, float *outCount,
                                      float *outMoments, float *outVariance, float maxHistory, float depthTolerance)
{
    RtvMomentArgs A;
    A.W = W; A.H = H; A.blocksX = 0;
    A.maxHistory = maxHistory; A.depthTolerance = depthTolerance;
    A.colour = colour; A.motion = motion; A.prevT = prevT; A.triangle = triangle;
    A.histColour = histColour; A.histCount = histCount; A.histT = histT; A.histTriangle = histTriangle; A.histMoments = histMoments;
    A.outColour = outColour; A.outCount = outCount; A.outMoments = outMoments; A.outVariance = outVariance;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) rtv_moments_pixel(A, x, y);
}

// moments and count: both given or both null.  out W x H x 3, outVariance W x H (V^K; with iterations = 0, V^0).
extern "C" void variance_host_filter(uint32_t W, uint32_t H, const float *colour, const float *normal, const float *albedo, const float *moments,
                                     const float *count, float *out, float *outVariance, uint32_t iterations, float ls, float floor_, float ia,
                                     uint32_t E, float spatialBelow)
{
    const size_t n = (size_t)W * H;
    std::vector<rtv_f4> g0(n), g1(n), s[2] = { std::vector<rtv_f4>(n), std::vector<rtv_f4>(n) };
    std::vector<float> m(2 * n), il(n);
    for (size_t p = 0; p < n; ++p) {
        g0[p] = rtv_guide_normal(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]);
        g1[p] = rtv_make4(albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2], 0.f);
        if (moments) {
            m[2 * p] = moments[2 * p];
            m[2 * p + 1] = moments[2 * p + 1];
        } else {
            const float l = rtv_lum(colour[3 * p], colour[3 * p + 1], colour[3 * p + 2]);
            m[2 * p] = l;
            m[2 * p + 1] = l * l;
        }
    }
    for (int y = 0; y < (int)H; ++y)
        for (int x = 0; x < (int)W; ++x) {
            const size_t p = (size_t)y * W + x;
            const float v = rtv_estimate_pixel(W, H, x, y, m[2 * p], m[2 * p + 1], count ? count[p] : 1.0f, spatialBelow, ia, E, g0[p], g1[p],
                                               [&](int dx, int dy, rtv_f4 &nq, rtv_f4 &aq, float &q1, float &q2) {
                                                   const size_t q = (size_t)(y + dy) * W + (x + dx);
                                                   nq = g0[q];
                                                   aq = g1[q];
                                                   q1 = m[2 * q];
                                                   q2 = m[2 * q + 1];
                                               });
            s[0][p] = rtv_make4(colour[3 * p], colour[3 * p + 1], colour[3 * p + 2], v);
        }
    for (uint32_t i = 0; i < iterations; ++i) {
        const std::vector<rtv_f4> &in = s[i & 1];
        std::vector<rtv_f4> &o = s[(i + 1) & 1];
        const int h = 1 << i;
        for (int y = 0; y < (int)H; ++y)
            for (int x = 0; x < (int)W; ++x)
                il[(size_t)y * W + x] = rtv_il_pixel(W, H, x, y, ls, floor_, [&](int dx, int dy) { return in[(size_t)(y + dy) * W + (x + dx)].w; });
        for (int y = 0; y < (int)H; ++y)
            for (int x = 0; x < (int)W; ++x) {
                const size_t p = (size_t)y * W + x;
                o[p] = rtv_iter_pixel(W, H, x, y, h, il[p], ia, E, in[p], g0[p], g1[p], [&](int j, int k, rtv_f4 &cq, rtv_f4 &nq, rtv_f4 &aq) {
                    const size_t q = (size_t)(y + (j - 2) * h) * W + (x + (k - 2) * h);
                    cq = in[q];
                    nq = g0[q];
                    aq = g1[q];
                });
            }
    }
    const std::vector<rtv_f4> &r = s[iterations & 1];
    for (size_t p = 0; p < n; ++p) {
        out[3 * p] = r[p].x;
        out[3 * p + 1] = r[p].y;
        out[3 * p + 2] = r[p].z;
        outVariance[p] = r[p].w;
    }
}
