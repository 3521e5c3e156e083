// rt_temporal.hip -- the temporal accumulation of include/raytrace_hip.h ("TEMPORAL ACCUMULATION"): the history of the previous frame is
// fetched bilinearly where the motion vectors point, tap by tap validated against the triangle id and prevT, and blended with the new
// frame, in the exact fp32 arithmetic the header fixes (tests/temporal_oracle.py is the same definition in numpy).
//
// Kernels (rt_filters.cpp issues them on one stream):
//   rtt_gather_kernel      scene path only: the [slot][R,G,B][128*128] u16 tile buffer -> row-major W x H x 3 f32 colour (u16 / 65535);
//                          rtd_gather_kernel without the surface sums, for scenes that have no surface passes on
//   rtt_accumulate_kernel  one lane per pixel, a wave is one 8x8 block of the screen (a workgroup is four of them side by side), so under
//                          a smooth flow the four taps of neighbouring lanes fall into the same cache lines; no LDS: the flow is arbitrary
//   rtt_clamp_kernel       "TEMPORAL CLAMP": the same mapping with the frame's 3x3 colour boxes taken from a 34 x 10 tile in LDS, with or
//                          without the luminance moments (rt_temporal_clamp_pixel.h); issued in place of rtt_accumulate_kernel or
//                          rtv_moments_kernel when a clamp is asked for
//   rtt_quantise_kernel    scene path only: W x H x 3 f32 -> the quantised u16 planes, as rtd_output_kernel writes them
// Nothing here may change a bit: no fast math, no reciprocal-multiply, no contraction (the Makefile's exactness flags apply).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rt_launch.h"
#include "rt_temporal_clamp_pixel.h"
#include "rt_temporal_pixel.h"

namespace {

__global__ __launch_bounds__(256) void rtt_accumulate_kernel(const RttArgs A)
{
    const uint32_t bx = blockIdx.x % A.blocksX, by = blockIdx.x / A.blocksX;
    const uint32_t wave = threadIdx.x >> 6, in = threadIdx.x & 63u;
    const uint32_t x = bx * 32u + wave * 8u + (in & 7u), y = by * 8u + (in >> 3);
    if (x >= A.W || y >= A.H) return;
    rtt_pixel(A, x, y);
}

// The clamped accumulation ("TEMPORAL CLAMP"): rtt_accumulate_kernel's mapping, and the frame's colour of the 34 x 10 texels the
// workgroup's 3x3 boxes reach staged in LDS, planar per channel.  The load walks the tile's rows as the 102 consecutive floats they
// are in memory; a texel outside the image is not loaded and never read (rtc_box skips its tap by the same coordinate test).  Row stride
// 40 floats: a ds_read_b32 is served per 32-lane half, which is 4 rows x 8 columns of a wave's 8x8 block -- words 40 r + c + const, banks
// 8 r + c + const, all 32 distinct for every (dx, dy).  Plane stride 405 = 21 mod 32: the 32 consecutive floats a half-wave stores are
// 10 or 11 texels x 3 channels and land on banks t, t + 21, t + 10.  4860 bytes, so the LDS does not limit the occupancy.
// Lanes past the image's edge help to load and reach the barrier; only the pixel's own work is skipped.  History taps stay global loads.
constexpr int RTC_TILE_W = 34, RTC_TILE_H = 10, RTC_ROW = 40, RTC_PLANE = RTC_TILE_H * RTC_ROW + 5;

template <bool Moments>
__global__ __launch_bounds__(256) void rtt_clamp_kernel(const RtcArgs A)
{
    __shared__ float tile[3 * RTC_PLANE];
    const uint32_t bx = blockIdx.x % A.blocksX, by = blockIdx.x / A.blocksX;
    const int tx0 = (int)(bx * 32u) - 1, ty0 = (int)(by * 8u) - 1; // the tile's top-left texel
    for (int i = threadIdx.x; i < RTC_TILE_H * RTC_TILE_W * 3; i += 256) {
        const int r = i / (RTC_TILE_W * 3), e = i % (RTC_TILE_W * 3), t = e / 3, ch = e % 3;
        const int qx = tx0 + t, qy = ty0 + r;
        if (qx >= 0 && qx < (int)A.W && qy >= 0 && qy < (int)A.H)
            tile[ch * RTC_PLANE + r * RTC_ROW + t] = A.colour[((size_t)qy * A.W + (size_t)qx) * 3 + ch];
    }
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, in = threadIdx.x & 63u;
    const uint32_t lx = wave * 8u + (in & 7u), ly = in >> 3;
    const uint32_t x = bx * 32u + lx, y = by * 8u + ly;
    if (x >= A.W || y >= A.H) return; // (after the barrier)
    const float *centre = tile + (ly + 1u) * RTC_ROW + lx + 1u;
    rtc_pixel<Moments>(A, x, y, [&](int dx, int dy, int ch) { return centre[ch * RTC_PLANE + dy * RTC_ROW + dx]; });
}

// One thread per pixel slot of the instance's tiles (tile-major, like tileBuf); slots past the image's edge write nothing.  tileIds were
// checked against the tile count when the scene was built.
__global__ __launch_bounds__(256) void rtt_gather_kernel(uint32_t W, uint32_t H, uint32_t tilesX, const uint32_t *__restrict__ tileIds,
                                                         const uint16_t *__restrict__ tileBuf, float *__restrict__ colour)
{
    const uint32_t slot = blockIdx.x / 64u, l = (blockIdx.x % 64u) * 256u + threadIdx.x;
    const uint32_t t = tileIds[slot];
    const uint32_t gx = (t % tilesX) * 128u + (l % 128u), gy = (t / tilesX) * 128u + (l / 128u);
    if (gx >= W || gy >= H) return;
    const size_t o = ((size_t)gy * W + gx) * 3;
    const uint16_t *tb = tileBuf + (size_t)slot * 3 * 16384u + l;
#pragma unroll
    for (int c = 0; c < 3; ++c) colour[o + c] = (float)tb[c * 16384u] / 65535.0f;
}

__global__ __launch_bounds__(256) void rtt_quantise_kernel(uint32_t n, const float *__restrict__ colour, uint16_t *__restrict__ outR,
                                                           uint16_t *__restrict__ outG, uint16_t *__restrict__ outB)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const size_t b = (size_t)i * 3;
    const float s[3] = { colour[b] * 65535.0f, colour[b + 1] * 65535.0f, colour[b + 2] * 65535.0f };
    uint16_t u[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        u[ch] = !(s[ch] > 0.f) ? (uint16_t)0 : (s[ch] >= 65534.5f ? (uint16_t)65535 : (uint16_t)(s[ch] + 0.5f));
    outR[i] = u[0];
    outG[i] = u[1];
    outB[i] = u[2];
}

} // namespace

// The arrays were checked by the caller (rt_filters.cpp): W x H each, W, H in 1..16384, W*H <= 2^27, the outputs overlap nothing.
extern "C" hipError_t rtt_launch_accumulate(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *prevT,
                                            const uint32_t *triangle, const float *histColour, const float *histCount, const float *histT,
                                            const uint32_t *histTriangle, float *outColour, float *outCount, float maxHistory,
                                            float depthTolerance, hipStream_t stream)
{
    RttArgs A;
    A.W = W; A.H = H; A.blocksX = (W + 31u) / 32u;
    A.maxHistory = maxHistory; A.depthTolerance = depthTolerance;
    A.colour = colour; A.motion = motion; A.prevT = prevT; A.triangle = triangle;
    A.histColour = histColour; A.histCount = histCount; A.histT = histT; A.histTriangle = histTriangle;
    A.outColour = outColour; A.outCount = outCount;
    hipLaunchKernelGGL(rtt_accumulate_kernel, dim3(A.blocksX * ((H + 7u) / 8u)), dim3(256), 0, stream, A);
    return hipGetLastError();
}

// The clamped accumulation; mode and gamma were checked too.  histMoments null: colour and count alone (outMoments and outVariance are
// not written); given: the moments ride along, outMoments is needed and outVariance may be null.
extern "C" hipError_t rtt_launch_accumulate_clamp(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *prevT,
                                                  const uint32_t *triangle, const float *histColour, const float *histCount,
                                                  const float *histT, const uint32_t *histTriangle, const float *histMoments,
                                                  float *outColour, float *outCount, float *outMoments, float *outVariance, float maxHistory,
                                                  float depthTolerance, uint32_t mode, float gamma, hipStream_t stream)
{
    RtcArgs A;
    A.W = W; A.H = H; A.blocksX = (W + 31u) / 32u;
    A.mode = mode; A.gamma = gamma;
    A.maxHistory = maxHistory; A.depthTolerance = depthTolerance;
    A.colour = colour; A.motion = motion; A.prevT = prevT; A.triangle = triangle;
    A.histColour = histColour; A.histCount = histCount; A.histT = histT; A.histTriangle = histTriangle; A.histMoments = histMoments;
    A.outColour = outColour; A.outCount = outCount; A.outMoments = outMoments; A.outVariance = outVariance;
    const dim3 grid(A.blocksX * ((H + 7u) / 8u));
    if (histMoments)
        hipLaunchKernelGGL(rtt_clamp_kernel<true>, grid, dim3(256), 0, stream, A);
    else
        hipLaunchKernelGGL(rtt_clamp_kernel<false>, grid, dim3(256), 0, stream, A);
    return hipGetLastError();
}

extern "C" hipError_t rtt_launch_gather(uint32_t W, uint32_t H, uint32_t tilesX, const uint32_t *tileIds, uint32_t tileCount,
                                        const uint16_t *tileBuf, float *colour, hipStream_t stream)
{
    if (tileCount == 0) return hipSuccess;
    hipLaunchKernelGGL(rtt_gather_kernel, dim3(tileCount * 64u), dim3(256), 0, stream, W, H, tilesX, tileIds, tileBuf, colour);
    return hipGetLastError();
}

extern "C" hipError_t rtt_launch_quantise(uint32_t n, const float *colour, uint16_t *outR, uint16_t *outG, uint16_t *outB, hipStream_t stream)
{
    hipLaunchKernelGGL(rtt_quantise_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, colour, outR, outG, outB);
    return hipGetLastError();
}
