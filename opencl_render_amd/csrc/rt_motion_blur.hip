// rt_motion_blur.hip -- the vector motion blur of include/raytrace_hip.h ("MOTION BLUR"): a frame is blurred along its motion vectors,
// every pixel gathering along the dominant velocity of its 32 x 32 tile's neighbourhood (McGuire et al. 2012), in the exact fp32
// arithmetic the header fixes (tests/motion_blur_oracle.py is the same definition in numpy).
//
// Kernels (rt_filters.cpp issues them on one stream, in this order):
//   rmb_velocity_kernel  (a) one lane per pixel: the velocity's length and the depth side by side, lz = (l, z), 8 bytes per pixel -- what a
//                        tap needs of its pixel beside the colour.  (vx, vy) are not stored: only a tile's winner needs them.
//   rmb_tile_max_kernel  (b) one workgroup per tile, four pixels per lane in row-major order; reduced on the pair (l, index) -- greatest
//                        l, then smallest index -- in the wave by shuffles and across the four waves through LDS, so the answer is the
//                        sequential one; the winner's velocity is then computed again from its motion.
//   rmb_nb_max_kernel    (c) one lane per tile over its 3 x 3 neighbourhood.
//   rmb_gather_kernel    (d) rtt_accumulate_kernel's mapping: 32 x 8 workgroups, a wave one 8 x 8 block of the screen.  A workgroup lies
//                        inside one tile, so its neighbourhood maximum is read through a workgroup-uniform address (scalar registers), the
//                        "still tile" copy is a uniform branch and the lanes' taps along the one shared direction fall into the same lines.
// Nothing here may change a bit: no fast math, no reciprocal-multiply, no contraction (the Makefile's exactness flags apply).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rt_launch.h"
#include "rt_motion_blur_pixel.h"

namespace {

__global__ __launch_bounds__(256) void rmb_velocity_kernel(const RmbArgs A, const uint32_t n)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    float vx, vy, l;
    rmb_velocity(A.motion[2 * (size_t)p], A.motion[2 * (size_t)p + 1], A.shutter, A.maxBlur, vx, vy, l);
    A.lz[2 * (size_t)p] = l;
    A.lz[2 * (size_t)p + 1] = A.depth[p];
}

// does (l, i) come before (bl, bi) in the order of (b): a greater length, or the same length at a smaller index
__device__ __forceinline__ bool rmb_before(const float l, const uint32_t i, const float bl, const uint32_t bi)
{
    return l > bl || (l == bl && i < bi);
}

__global__ __launch_bounds__(256) void rmb_tile_max_kernel(const RmbArgs A)
{
    __shared__ float waveL[4];
    __shared__ uint32_t waveI[4];
    const uint32_t tx = blockIdx.x % A.tilesX, ty = blockIdx.x / A.tilesX;
    float bl = 0.f;           // (lengths are never negative and never NaN: rmb_velocity)
    uint32_t bi = 0xffffffffu; // the pixel's row-major index in the tile, 0..1023
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t i = k * 256u + threadIdx.x;
        const uint32_t x = tx * RMB_TILE + (i & 31u), y = ty * RMB_TILE + (i >> 5);
        if (x < A.W && y < A.H) {
            const float l = A.lz[2 * ((size_t)y * A.W + x)];
            if (rmb_before(l, i, bl, bi)) { bl = l; bi = i; }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ol = __shfl_xor(bl, m, 64);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, m, 64);
        if (rmb_before(ol, oi, bl, bi)) { bl = ol; bi = oi; }
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) { waveL[wave] = bl; waveI[wave] = bi; }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    for (uint32_t w = 1; w < 4u; ++w)
        if (rmb_before(waveL[w], waveI[w], bl, bi)) { bl = waveL[w]; bi = waveI[w]; }
    float vx = 0.f, vy = 0.f, l = 0.f;
    if (bl > 0.f) { // (so bi is a pixel of the image: the first one of the greatest length)
        const size_t p = (size_t)(ty * RMB_TILE + (bi >> 5)) * A.W + (tx * RMB_TILE + (bi & 31u));
        rmb_velocity(A.motion[2 * p], A.motion[2 * p + 1], A.shutter, A.maxBlur, vx, vy, l);
    }
    float *t = A.tileMax + (size_t)blockIdx.x * RMB_TILE_FLOATS;
    t[0] = vx; t[1] = vy; t[2] = l; t[3] = 0.f;
}

__global__ __launch_bounds__(256) void rmb_nb_max_kernel(const RmbArgs A)
{
    const uint32_t tile = blockIdx.x * 256u + threadIdx.x;
    if (tile >= A.tilesX * A.tilesY) return;
    const int tx = (int)(tile % A.tilesX), ty = (int)(tile / A.tilesX);
    float vx = 0.f, vy = 0.f, l = 0.f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = ty + dy;
        if (qy < 0 || qy >= (int)A.tilesY) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = tx + dx;
            if (qx < 0 || qx >= (int)A.tilesX) continue;
            const float *t = A.tileMax + ((size_t)qy * A.tilesX + (size_t)qx) * RMB_TILE_FLOATS;
            if (t[2] > l) { vx = t[0]; vy = t[1]; l = t[2]; }
        }
    }
    float *o = A.nbMax + (size_t)tile * RMB_TILE_FLOATS;
    o[0] = vx; o[1] = vy; o[2] = l; o[3] = 0.f;
}

__global__ __launch_bounds__(256) void rmb_gather_kernel(const RmbArgs A)
{
    const uint32_t bx = blockIdx.x % A.tilesX, by = blockIdx.x / A.tilesX; // (a block is as wide as a tile; four 8-row blocks per tile)
    const float *nb = A.nbMax + ((size_t)(by >> 2) * A.tilesX + bx) * RMB_TILE_FLOATS;
    const float nx = nb[0], ny = nb[1], nl = nb[2];
    const uint32_t wave = threadIdx.x >> 6, in = threadIdx.x & 63u;
    const uint32_t x = bx * 32u + wave * 8u + (in & 7u), y = by * 8u + (in >> 3);
    if (x >= A.W || y >= A.H) return;
    rmb_pixel(A, x, y, nx, ny, nl);
}

} // namespace

// The arrays were checked by the caller (rt_filters.cpp): W x H each, W, H in 1..16384, W*H <= 2^27, out overlaps nothing, the scratch
// holds lz, tileMax and nbMax; the parameters were checked too.  Four launches on `stream`.
extern "C" hipError_t rmb_launch(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *depth, float *out, float *lz,
                                 float *tileMax, float *nbMax, float shutter, float maxBlur, uint32_t taps, float depthSoftness,
                                 hipStream_t stream)
{
    RmbArgs A;
    A.W = W; A.H = H;
    A.tilesX = (W + RMB_TILE - 1u) / RMB_TILE; A.tilesY = (H + RMB_TILE - 1u) / RMB_TILE; A.taps = taps;
    A.shutter = shutter; A.maxBlur = maxBlur; A.depthSoftness = depthSoftness;
    A.colour = colour; A.motion = motion; A.depth = depth;
    A.lz = lz; A.tileMax = tileMax; A.nbMax = nbMax;
    A.out = out;
    const uint32_t n = W * H, tiles = A.tilesX * A.tilesY;
    hipLaunchKernelGGL(rmb_velocity_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, A, n);
    hipLaunchKernelGGL(rmb_tile_max_kernel, dim3(tiles), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(rmb_nb_max_kernel, dim3((tiles + 255u) / 256u), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(rmb_gather_kernel, dim3(A.tilesX * ((H + 7u) / 8u)), dim3(256), 0, stream, A);
    return hipGetLastError();
}
