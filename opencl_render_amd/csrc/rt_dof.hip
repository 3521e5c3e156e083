// rt_dof.hip -- the depth of field of include/raytrace_hip.h ("DEPTH OF FIELD"): a frame is blurred by the circle of confusion its depth
// pass gives every pixel, scatter as gather, the gather's extent taken from the greatest radius of the pixel's 32 x 32 tile's
// neighbourhood, in the exact fp32 arithmetic the header fixes (tests/dof_oracle.py is the same definition in numpy).
//
// Kernels (rt_filters.cpp issues them on one stream, in this order):
//   rdf_radius_kernel   (a) one lane per pixel: the radius and the depth side by side, rz = (r, z), 8 bytes per pixel -- what a tap needs
//                       of its pixel beside the colour (one load instead of a load, a division and two multiplies per tap).
//   rdf_tile_max_kernel (b) one workgroup per tile, four pixels per lane; the maximum reduced in the wave by shuffles and across the four
//                       waves through LDS.  Radii are never NaN, so the maximum does not depend on the order.
//   rdf_nb_max_kernel   (c) one lane per tile over its 3 x 3 neighbourhood.
//   rdf_gather_kernel   (d) rtt_accumulate_kernel's mapping: 32 x 8 workgroups, a wave one 8 x 8 block of the screen.  A workgroup lies
//                       inside one tile, so R is read through a workgroup-uniform address (a scalar register) and the "in focus" copy is a
//                       uniform branch.  A tap's (ox, oy, d) depend on R, the tap and the pixel's dither value alone -- four values per
//                       tap and workgroup --: the workgroup computes them once into LDS, [tap][dither] as float4 (at most 10.5 KiB), each
//                       entry by rdf_tap, the function the host build calls per pixel; a lane then reads one entry per tap in
//                       place of an integer division, two float divisions and a square root.  The four addresses of a read are 64
//                       contiguous bytes: no bank conflict.  The pixels' own taps (rz 8 B, colour 12 B) go through the cache: see
//                       DESIGN 5q for why not through an LDS tile.
//   rdf_scene_gather_kernel  scene path only: the [slot][R,G,B][128*128] u16 tile buffer and the depth word of the pass buffer -> row-major
//                       W x H x 3 f32 colour (u16 / 65535) and W x H f32 depth (the word as it is).
// Nothing here may change a bit: no fast math, no reciprocal-multiply, no contraction (the Makefile's exactness flags apply).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rt_device.h"
#include "rt_dof_pixel.h"
#include "rt_launch.h"

namespace {

__global__ __launch_bounds__(256) void rdf_radius_kernel(const RdfArgs A, const uint32_t n)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const float z = A.depth[p];
    A.rz[2 * (size_t)p] = rdf_radius(z, A.focus, A.cocScale, A.maxCoc);
    A.rz[2 * (size_t)p + 1] = z;
}

__global__ __launch_bounds__(256) void rdf_tile_max_kernel(const RdfArgs A)
{
    __shared__ float waveR[4];
    const uint32_t tx = blockIdx.x % A.tilesX, ty = blockIdx.x / A.tilesX;
    float b = 0.f; // (radii are never negative and never NaN: rdf_radius)
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t i = k * 256u + threadIdx.x;
        const uint32_t x = tx * RDF_TILE + (i & 31u), y = ty * RDF_TILE + (i >> 5);
        if (x < A.W && y < A.H) {
            const float r = A.rz[2 * ((size_t)y * A.W + x)];
            if (r > b) b = r;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float o = __shfl_xor(b, m, 64);
        if (o > b) b = o;
    }
    if ((threadIdx.x & 63u) == 0u) waveR[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x != 0u) return;
    for (uint32_t w = 1; w < 4u; ++w)
        if (waveR[w] > b) b = waveR[w];
    A.tileMax[blockIdx.x] = b;
}

__global__ __launch_bounds__(256) void rdf_nb_max_kernel(const RdfArgs A)
{
    const uint32_t tile = blockIdx.x * 256u + threadIdx.x;
    if (tile >= A.tilesX * A.tilesY) return;
    const int tx = (int)(tile % A.tilesX), ty = (int)(tile / A.tilesX);
    float b = 0.f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = ty + dy;
        if (qy < 0 || qy >= (int)A.tilesY) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = tx + dx;
            if (qx < 0 || qx >= (int)A.tilesX) continue;
            const float r = A.tileMax[(size_t)qy * A.tilesX + (size_t)qx];
            if (r > b) b = r;
        }
    }
    A.nbMax[tile] = b;
}

__global__ __launch_bounds__(256) void rdf_gather_kernel(const RdfArgs A)
{
    __shared__ float4 taps[RDF_MAX_TAPS * 4u]; // [tap][dither]: (ox, oy, d, 0)
    const uint32_t bx = blockIdx.x % A.tilesX, by = blockIdx.x / A.tilesX; // (a block is as wide as a tile; four 8-row blocks per tile)
    const float R = A.nbMax[(size_t)(by >> 2) * A.tilesX + bx];
    const uint32_t wave = threadIdx.x >> 6, in = threadIdx.x & 63u;
    const uint32_t x = bx * 32u + wave * 8u + (in & 7u), y = by * 8u + (in >> 3);
    const bool inside = x < A.W && y < A.H;
    if (R >= 0.5f) { // (uniform: every lane of the workgroup reads the same R, so all of them reach the barrier or none does)
        const uint32_t entries = 16u * A.rings * (A.rings + 1u); // 4 dither values x 4 rings (rings + 1) taps, at most 4 RDF_MAX_TAPS
        for (uint32_t i = threadIdx.x; i < entries; i += 256u) {
            const uint32_t t = i >> 2, j = i & 3u;
            uint32_t k = 1;
            while (t >= 4u * k * (k + 1u)) ++k; // ring k holds taps 4 k (k - 1) .. 4 k (k + 1) - 1
            float ox, oy, d;
            rdf_tap(k, t - 4u * k * (k - 1u), A.rings, rdf_jitter(j), R, ox, oy, d);
            taps[i] = make_float4(ox, oy, d, 0.f);
        }
        __syncthreads();
    }
    if (!inside) return; // (after the barrier)
    rdf_pixel(A, x, y, R, [&](uint32_t j, uint32_t t, uint32_t, uint32_t, float &ox, float &oy, float &d) {
        const float4 e = taps[t * 4u + j];
        ox = e.x; oy = e.y; d = e.z;
    });
}

// One thread per pixel slot of the instance's tiles (tile-major, like tileBuf and passBuf); slots past the image's edge write nothing.
// tileIds were checked against the tile count when the scene was built.
__global__ __launch_bounds__(256) void rdf_scene_gather_kernel(uint32_t W, uint32_t H, uint32_t tilesX, const uint32_t *__restrict__ tileIds,
                                                               const uint16_t *__restrict__ tileBuf, const uint32_t *__restrict__ passBuf,
                                                               float *__restrict__ colour, uint32_t *__restrict__ depth)
{
    const uint32_t slot = blockIdx.x / 64u, l = (blockIdx.x % 64u) * 256u + threadIdx.x;
    const uint32_t t = tileIds[slot];
    const uint32_t gx = (t % tilesX) * 128u + (l % 128u), gy = (t / tilesX) * 128u + (l / 128u);
    if (gx >= W || gy >= H) return;
    const size_t o = (size_t)gy * W + gx;
    const uint16_t *tb = tileBuf + (size_t)slot * 3 * RT_TILE_PIXELS + l;
#pragma unroll
    for (int c = 0; c < 3; ++c) colour[3 * o + c] = (float)tb[c * RT_TILE_PIXELS] / 65535.0f;
    depth[o] = passBuf[((size_t)slot * RT_PASS_WORDS + RT_PASS_DEPTH) * RT_TILE_PIXELS + l];
}

} // namespace

// The arrays were checked by the caller (rt_filters.cpp): W x H each, W, H in 1..16384, W*H <= 2^27, out overlaps nothing, the scratch
// holds rz, tileMax and nbMax; the parameters were checked too (rings in 1..RDF_MAX_RINGS: the LDS table holds them).  Four launches
// on `stream`.
extern "C" hipError_t rdf_launch(uint32_t W, uint32_t H, const float *colour, const float *depth, float *out, float *rz, float *tileMax,
                                 float *nbMax, float focus, float cocScale, float maxCoc, uint32_t rings, float depthSoftness,
                                 hipStream_t stream)
{
    if (rings < 1u || rings > RDF_MAX_RINGS) return hipErrorInvalidValue;
    RdfArgs A;
    A.W = W; A.H = H;
    A.tilesX = (W + RDF_TILE - 1u) / RDF_TILE; A.tilesY = (H + RDF_TILE - 1u) / RDF_TILE; A.rings = rings;
    A.focus = focus; A.cocScale = cocScale; A.maxCoc = maxCoc; A.depthSoftness = depthSoftness;
    A.colour = colour; A.depth = depth;
    A.rz = rz; A.tileMax = tileMax; A.nbMax = nbMax;
    A.out = out;
    const uint32_t n = W * H, tiles = A.tilesX * A.tilesY;
    hipLaunchKernelGGL(rdf_radius_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, A, n);
    hipLaunchKernelGGL(rdf_tile_max_kernel, dim3(tiles), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(rdf_nb_max_kernel, dim3((tiles + 255u) / 256u), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(rdf_gather_kernel, dim3(A.tilesX * ((H + 7u) / 8u)), dim3(256), 0, stream, A);
    return hipGetLastError();
}

extern "C" hipError_t rdf_launch_scene_gather(uint32_t W, uint32_t H, uint32_t tilesX, const uint32_t *tileIds, uint32_t tileCount,
                                              const uint16_t *tileBuf, const uint32_t *passBuf, float *colour, float *depth,
                                              hipStream_t stream)
{
    if (tileCount == 0) return hipSuccess;
    hipLaunchKernelGGL(rdf_scene_gather_kernel, dim3(tileCount * 64u), dim3(256), 0, stream, W, H, tilesX, tileIds, tileBuf, passBuf, colour,
                       (uint32_t *)depth);
    return hipGetLastError();
}
