// rt_camera_move.hip -- the camera candidate lists of a RESIDENT scene rebuilt on the device for a new camera
// (rtHipSceneSetCamera; SURVEY.md section 8f row 2: "camera-only changes reuse geometry + grid").
//
// The resident variant of rt_build_device.hip's camera build.  Membership is decided by the same shared header
// (rt_build_shared.h: camera_position, rect_setup, rect_pixel_test), compiled without fp contraction, so a pixel reads the
// triangles the host builder gives it, in ascending order.  What differs:
//   * the vertices come from the scene's own records (a = triRec[t][0..2], b and c = triShade[t][0..5], stored verbatim by
//     rt_prepare_triangles): nothing is uploaded, there is no index gather;
//   * a member pixel (x, y) is written at its TILE-MAJOR index slot*128*128 + (y&127)*128 + (x&127), slot = slotOf[tile of the pixel];
//     pixels of tiles this instance does not own are dropped before their membership test;
//   * no neighbour de-duplication: ranges of different pixels never share storage (what a pixel reads is the same either way);
//   * every buffer belongs to the scene and the launches go to the scene's stream.
//   rtc_project         one thread per triangle: the three projected vertices
//   rtc_rasterize       one thread per triangle (COUNT or FILL pass); a triangle whose clipped rectangle has more than RT_BIG_RECT
//                       pixels goes on a list instead (a function of the triangle alone, so both passes agree) ...
//   rtc_rasterize_big   ... and is rasterised by one workgroup, the rectangle's pixels dealt to its threads row by row
//   rtc_total           the entries in 64 bits, before anything is sized by them
//   rtc_sort_pixels     one thread per pixel: ends, and an insertion sort of its (short) list
//   rtc_alias_slots     only when a tile id occurs twice in the instance's tile list: the later slots take the first one's ranges
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "rt_build_shared.h"
#include "rt_camera_move.h"
#include "rt_launch.h"

using rtbuild::Camera;
using rtbuild::F2;
using rtbuild::F3;
using rtbuild::RectSetup;

#define RT_BIG_RECT 1024u // as in rt_build_device.hip
#define RT_CM_TILE 128u
#define RT_CM_TILE_PIXELS (RT_CM_TILE * RT_CM_TILE)

namespace {

__global__ __launch_bounds__(256) void rtc_project(const Camera cam, uint32_t T, const float4 *__restrict__ triRec, const float *__restrict__ triShade,
                                                   F2 *__restrict__ pos)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const float4 a = triRec[4 * (size_t)t]; // {a.xyz, ab.x}
    const float2 *sh = reinterpret_cast<const float2 *>(triShade + RT_TRI_SHADE_WORDS * (size_t)t); // {b.xyz, c.xyz}
    const float2 s0 = sh[0], s1 = sh[1], s2 = sh[2];
    pos[3 * (size_t)t] = rtbuild::camera_position(cam, F3{ a.x, a.y, a.z });
    pos[3 * (size_t)t + 1] = rtbuild::camera_position(cam, F3{ s0.x, s0.y, s1.x });
    pos[3 * (size_t)t + 2] = rtbuild::camera_position(cam, F3{ s1.y, s2.x, s2.y });
}

// tile-major index of pixel (x, y), or RTC_NO_SLOT when the instance does not own its tile (or the pixel is outside the image)
__device__ __forceinline__ uint32_t tile_major(const RtCamMoveArgs &A, uint32_t x, uint32_t y)
{
    if (x >= A.width || y >= A.height) return RTC_NO_SLOT;
    const uint32_t slot = A.slotOf[(y / RT_CM_TILE) * A.tilesX + x / RT_CM_TILE];
    if (slot == RTC_NO_SLOT) return RTC_NO_SLOT;
    return slot * RT_CM_TILE_PIXELS + (y % RT_CM_TILE) * RT_CM_TILE + x % RT_CM_TILE;
}

// FILL = false: count[pixel] += 1 (no value comes back);  FILL = true: list[start[pixel] + cursor[pixel]++] = triangle
template <bool FILL> __device__ __forceinline__ void emit_pixel(const RtCamMoveArgs &A, uint32_t px, uint32_t tri)
{
    if (!FILL) { atomicAdd(&A.count[px], 1u); return; }
    const uint32_t at = atomicAdd(&A.count[px], 1u);
    A.list[A.start[px] + at] = tri;
}

template <bool FILL> __global__ __launch_bounds__(256) void rtc_rasterize(const RtCamMoveArgs A)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= A.triangleCount) return;
    const F2 *pos = (const F2 *)A.pos;
    const RectSetup s = rtbuild::rect_setup(A.width, A.height, pos[3 * (size_t)t], pos[3 * (size_t)t + 1], pos[3 * (size_t)t + 2]);
    const uint64_t area = (s.x1 >= s.x0 && s.y1 >= s.y0) ? (uint64_t)(s.x1 - s.x0 + 1) * (uint64_t)(s.y1 - s.y0 + 1) : 0;
    if (area > RT_BIG_RECT) {
        if (!FILL) A.bigList[atomicAdd(&A.ctl->bigCount, 1u)] = t;
        return;
    }
    if (s.aOnScreen) {
        const uint32_t px = tile_major(A, s.ax, s.ay);
        if (px != RTC_NO_SLOT) emit_pixel<FILL>(A, px, t);
    }
    for (uint32_t y = s.y0; y <= s.y1; ++y)
        for (uint32_t x = s.x0; x <= s.x1; ++x) {
            if (x == s.ax && y == s.ay) continue;
            const uint32_t px = tile_major(A, x, y);
            if (px != RTC_NO_SLOT && rtbuild::rect_pixel_test(s, x, y)) emit_pixel<FILL>(A, px, t);
        }
}

template <bool FILL> __global__ __launch_bounds__(256) void rtc_rasterize_big(const RtCamMoveArgs A)
{
    const uint32_t bigCount = A.ctl->bigCount < A.triangleCount ? A.ctl->bigCount : A.triangleCount;
    for (uint32_t b = blockIdx.x; b < bigCount; b += gridDim.x) {
        const uint32_t t = A.bigList[b];
        const F2 *pos = (const F2 *)A.pos;
        const RectSetup s = rtbuild::rect_setup(A.width, A.height, pos[3 * (size_t)t], pos[3 * (size_t)t + 1], pos[3 * (size_t)t + 2]);
        if (threadIdx.x == 0 && s.aOnScreen) {
            const uint32_t px = tile_major(A, s.ax, s.ay);
            if (px != RTC_NO_SLOT) emit_pixel<FILL>(A, px, t);
        }
        const uint64_t w = (uint64_t)(s.x1 - s.x0 + 1), h = (uint64_t)(s.y1 - s.y0 + 1);
        for (uint64_t i = threadIdx.x; i < w * h; i += 256) { // consecutive lanes: consecutive pixels of a row (runs of at most 128 in one tile)
            const uint32_t x = s.x0 + (uint32_t)(i % w), y = s.y0 + (uint32_t)(i / w);
            if (x == s.ax && y == s.ay) continue;
            const uint32_t px = tile_major(A, x, y);
            if (px != RTC_NO_SLOT && rtbuild::rect_pixel_test(s, x, y)) emit_pixel<FILL>(A, px, t);
        }
    }
}

// Sum of the per-pixel counts in 64 bits: the exclusive scan that gives the starts runs in 32 bits and would wrap unnoticed.
__global__ __launch_bounds__(256) void rtc_total(uint32_t n, const uint32_t *__restrict__ count, RtCamMoveCtl *ctl)
{
    unsigned long long sum = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) sum += count[p];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&ctl->total, sum);
}

__global__ __launch_bounds__(256) void rtc_sort_pixels(uint32_t n, const uint32_t *__restrict__ start, const uint32_t *__restrict__ count, uint32_t *list,
                                                       uint32_t *__restrict__ end)
{
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t first = start[p], m = count[p];
    end[p] = first + m;
    uint32_t *l = list + first;
    for (uint32_t i = 1; i < m; ++i) { // lists are short (a few entries); entries are distinct triangles
        const uint32_t v = l[i];
        uint32_t j = i;
        while (j > 0 && l[j - 1] > v) { l[j] = l[j - 1]; --j; }
        l[j] = v;
    }
}

__global__ __launch_bounds__(256) void rtc_alias_slots(uint32_t n, const uint32_t *__restrict__ firstSlot, uint32_t *start, uint32_t *end)
{
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t slot = p / RT_CM_TILE_PIXELS, from = firstSlot[slot];
    if (from == slot) return;
    const uint32_t q = from * RT_CM_TILE_PIXELS + p % RT_CM_TILE_PIXELS;
    start[p] = start[q]; end[p] = end[q];
}

Camera camera_of(const RtCamMoveArgs &A)
{
    return Camera{ F3{ A.eye[0], A.eye[1], A.eye[2] }, F3{ A.topLeft[0], A.topLeft[1], A.topLeft[2] }, F3{ A.lr[0], A.lr[1], A.lr[2] },
                   F3{ A.tb[0], A.tb[1], A.tb[2] }, A.pixelSizeInv };
}

constexpr uint32_t BIG_BLOCKS = 1024;

} // namespace

extern "C" hipError_t rtc_scan_bytes(uint32_t n, size_t *bytes)
{
    *bytes = 0;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, nullptr);
}

// Stage 1: projection, the COUNT pass, the 64-bit total.  Leaves ctl = { total, bigCount } for the host to size the list with.
extern "C" hipError_t rtc_launch_count(const RtCamMoveArgs *args, hipStream_t stream)
{
    const RtCamMoveArgs &A = *args;
    hipError_t e = hipMemsetAsync(A.count, 0, (size_t)A.pixels * 4, stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(A.ctl, 0, sizeof(RtCamMoveCtl), stream);
    if (e != hipSuccess) return e;
    const uint32_t T = A.triangleCount, tBlocks = (T + 255) / 256;
    if (T) {
        hipLaunchKernelGGL(rtc_project, dim3(tBlocks), dim3(256), 0, stream, camera_of(A), T, (const float4 *)A.triRec, A.triShade, (F2 *)A.pos);
        hipLaunchKernelGGL(rtc_rasterize<false>, dim3(tBlocks), dim3(256), 0, stream, A);
        hipLaunchKernelGGL(rtc_rasterize_big<false>, dim3(BIG_BLOCKS), dim3(256), 0, stream, A);
    }
    if (A.pixels) hipLaunchKernelGGL(rtc_total, dim3(std::min<uint32_t>((A.pixels + 255) / 256, 1024u)), dim3(256), 0, stream, A.pixels, A.count, A.ctl);
    return hipGetLastError();
}

// Stage 2: exclusive scan of the counts into the starts, the FILL pass (count becomes the cursor), ends and per-pixel order.
extern "C" hipError_t rtc_launch_fill(const RtCamMoveArgs *args, hipStream_t stream)
{
    const RtCamMoveArgs &A = *args;
    if (!A.pixels) return hipSuccess;
    size_t scanBytes = A.scanBytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(A.scanTmp, scanBytes, A.count, A.start, (int)A.pixels, stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(A.count, 0, (size_t)A.pixels * 4, stream);
    if (e != hipSuccess) return e;
    const uint32_t T = A.triangleCount, tBlocks = (T + 255) / 256, pBlocks = (A.pixels + 255) / 256;
    if (T) {
        hipLaunchKernelGGL(rtc_rasterize<true>, dim3(tBlocks), dim3(256), 0, stream, A);
        hipLaunchKernelGGL(rtc_rasterize_big<true>, dim3(BIG_BLOCKS), dim3(256), 0, stream, A);
    }
    hipLaunchKernelGGL(rtc_sort_pixels, dim3(pBlocks), dim3(256), 0, stream, A.pixels, A.start, A.count, A.list, A.end);
    if (A.firstSlot) hipLaunchKernelGGL(rtc_alias_slots, dim3(pBlocks), dim3(256), 0, stream, A.pixels, A.firstSlot, A.start, A.end);
    return hipGetLastError();
}
