// The accumulation's per-pixel code (opencl_render_amd/csrc/rt_temporal_pixel.h, what rtt_accumulate_kernel runs per lane) compiled for
// the host: tests/test_temporal.py builds this with the exactness flags of csrc/Makefile and compares it with temporal_oracle.py.
#include "rt_temporal_pixel.h"

extern "C" void temporal_host(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *prevT, const uint32_t *triangle,
                              const float *histColour, const float *histCount, const float *histT, const uint32_t *histTriangle,
                              float *outColour, float *outCount, float maxHistory, float depthTolerance)
{
    RttArgs A;
    A.W = W; A.H = H; A.blocksX = 0;
    A.maxHistory = maxHistory; A.depthTolerance = depthTolerance;
    A.colour = colour; A.motion = motion; A.prevT = prevT; A.triangle = triangle;
    A.histColour = histColour; A.histCount = histCount; A.histT = histT; A.histTriangle = histTriangle;
    A.outColour = outColour; A.outCount = outCount;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) rtt_pixel(A, x, y);
}
