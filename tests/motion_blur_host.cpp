// The motion blur's per-pixel code (opencl_render_amd/csrc/rt_motion_blur_pixel.h, what the kernels of rt_motion_blur.hip run per lane)
// compiled for the host: tests/test_motion_blur.py builds this with the exactness flags of csrc/Makefile and compares it with
// motion_blur_oracle.py.  (b) and (c) are plain sequential loops here, the header's definition word for word; the kernels' parallel
// reduction is checked against the same oracle on the device.
#include "rt_motion_blur_pixel.h"

#include <vector>

extern "C" void motion_blur_host(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *depth, float *out,
                                 float shutter, float maxBlur, uint32_t taps, float depthSoftness)
{
    const uint32_t tilesX = (W + RMB_TILE - 1u) / RMB_TILE, tilesY = (H + RMB_TILE - 1u) / RMB_TILE;
    std::vector<float> lz((size_t)W * H * 2), tileMax((size_t)tilesX * tilesY * RMB_TILE_FLOATS, 0.f),
        nbMax((size_t)tilesX * tilesY * RMB_TILE_FLOATS, 0.f);
    RmbArgs A;
    A.W = W; A.H = H; A.tilesX = tilesX; A.tilesY = tilesY; A.taps = taps;
    A.shutter = shutter; A.maxBlur = maxBlur; A.depthSoftness = depthSoftness;
    A.colour = colour; A.motion = motion; A.depth = depth;
    A.lz = lz.data(); A.tileMax = tileMax.data(); A.nbMax = nbMax.data();
    A.out = out;
    // (a) and (b): the tile's pixels in row-major order, replaced only by a strictly greater length
    for (uint32_t ty = 0; ty < tilesY; ++ty)
        for (uint32_t tx = 0; tx < tilesX; ++tx) {
            float *t = A.tileMax + ((size_t)ty * tilesX + tx) * RMB_TILE_FLOATS;
            for (uint32_t y = ty * RMB_TILE; y < (ty + 1u) * RMB_TILE && y < H; ++y)
                for (uint32_t x = tx * RMB_TILE; x < (tx + 1u) * RMB_TILE && x < W; ++x) {
                    const size_t p = (size_t)y * W + x;
                    float vx, vy, l;
                    rmb_velocity(motion[2 * p], motion[2 * p + 1], shutter, maxBlur, vx, vy, l);
                    A.lz[2 * p] = l;
                    A.lz[2 * p + 1] = depth[p];
                    if (l > t[2]) { t[0] = vx; t[1] = vy; t[2] = l; }
                }
        }
    // (c)
    for (int ty = 0; ty < (int)tilesY; ++ty)
        for (int tx = 0; tx < (int)tilesX; ++tx) {
            float *o = A.nbMax + ((size_t)ty * tilesX + tx) * RMB_TILE_FLOATS;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int qy = ty + dy, qx = tx + dx;
                    if (qy < 0 || qy >= (int)tilesY || qx < 0 || qx >= (int)tilesX) continue;
                    const float *t = A.tileMax + ((size_t)qy * tilesX + qx) * RMB_TILE_FLOATS;
                    if (t[2] > o[2]) { o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; }
                }
        }
    // (d)
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const float *nb = A.nbMax + ((size_t)(y >> 5) * tilesX + (x >> 5)) * RMB_TILE_FLOATS;
            rmb_pixel(A, x, y, nb[0], nb[1], nb[2]);
        }
}
