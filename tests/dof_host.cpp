// The depth of field's per-pixel code (opencl_render_amd/csrc/rt_dof_pixel.h, what the kernels of rt_dof.hip run per lane) compiled for
// the host: tests/test_dof.py builds this with the exactness flags of csrc/Makefile and compares it with dof_oracle.py.  (b) and (c)
// are plain sequential loops here, the header's definition word for word, and every tap's offset is computed where it is used; the
// kernels' parallel reduction and their table of offsets are checked against the same oracle on the device.
#include "rt_dof_pixel.h"

#include <vector>

extern "C" void dof_host(uint32_t W, uint32_t H, const float *colour, const float *depth, float *out, float focus, float cocScale,
                         float maxCoc, uint32_t rings, float depthSoftness)
{
    const uint32_t tilesX = (W + RDF_TILE - 1u) / RDF_TILE, tilesY = (H + RDF_TILE - 1u) / RDF_TILE;
    std::vector<float> rz((size_t)W * H * 2), tileMax((size_t)tilesX * tilesY, 0.f), nbMax((size_t)tilesX * tilesY, 0.f);
    RdfArgs A;
    A.W = W; A.H = H; A.tilesX = tilesX; A.tilesY = tilesY; A.rings = rings;
    A.focus = focus; A.cocScale = cocScale; A.maxCoc = maxCoc; A.depthSoftness = depthSoftness;
    A.colour = colour; A.depth = depth;
    A.rz = rz.data(); A.tileMax = tileMax.data(); A.nbMax = nbMax.data();
    A.out = out;
    // (a) and (b)
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            const float r = rdf_radius(depth[p], focus, cocScale, maxCoc);
            A.rz[2 * p] = r;
            A.rz[2 * p + 1] = depth[p];
            float &t = A.tileMax[(size_t)(y >> 5) * tilesX + (x >> 5)];
            if (r > t) t = r;
        }
    // (c)
    for (int ty = 0; ty < (int)tilesY; ++ty)
        for (int tx = 0; tx < (int)tilesX; ++tx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int qy = ty + dy, qx = tx + dx;
                    if (qy < 0 || qy >= (int)tilesY || qx < 0 || qx >= (int)tilesX) continue;
                    float &o = A.nbMax[(size_t)ty * tilesX + tx];
                    if (A.tileMax[(size_t)qy * tilesX + qx] > o) o = A.tileMax[(size_t)qy * tilesX + qx];
                }
    // (d)
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const float R = A.nbMax[(size_t)(y >> 5) * tilesX + (x >> 5)];
            rdf_pixel(A, x, y, R, [&](uint32_t j, uint32_t, uint32_t k, uint32_t s, float &ox, float &oy, float &d) {
                rdf_tap(k, s, rings, rdf_jitter(j), R, ox, oy, d);
            });
        }
}
