// The clamped accumulation's per-pixel code (opencl_render_amd/csrc/rt_temporal_clamp_pixel.h, what rtt_clamp_kernel runs per lane)
// compiled for the host, the neighbourhood fetched from the array instead of LDS: tests/test_temporal_clamp.py builds this with the
// exactness flags of csrc/Makefile and compares it with temporal_clamp_oracle.py.  histMoments null: without moments.
#include "rt_temporal_clamp_pixel.h"

template <bool Moments>
static void run(const RtcArgs &A)
{
    for (uint32_t y = 0; y < A.H; ++y)
        for (uint32_t x = 0; x < A.W; ++x)
            rtc_pixel<Moments>(A, x, y, [&](int dx, int dy, int ch) {
                return A.colour[((size_t)((int)y + dy) * A.W + (size_t)((int)x + dx)) * 3 + (size_t)ch];
            });
}

extern "C" void temporal_clamp_host(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *prevT,
                                    const uint32_t *triangle, const float *histColour, const float *histCount, const float *histT,
                                    const uint32_t *histTriangle, const float *histMoments, float *outColour, float *outCount,
                                    float *outMoments, float *outVariance, float maxHistory, float depthTolerance, uint32_t mode, float gamma)
{
    RtcArgs A;
    A.W = W; A.H = H; A.blocksX = 0;
    A.mode = mode; A.gamma = gamma;
    A.maxHistory = maxHistory; A.depthTolerance = depthTolerance;
    A.colour = colour; A.motion = motion; A.prevT = prevT; A.triangle = triangle;
    A.histColour = histColour; A.histCount = histCount; A.histT = histT; A.histTriangle = histTriangle; A.histMoments = histMoments;
    A.outColour = outColour; A.outCount = outCount; A.outMoments = outMoments; A.outVariance = outVariance;
    if (histMoments)
        run<true>(A);
    else
        run<false>(A);
}
