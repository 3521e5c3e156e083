// rt_tile_order.h -- where the pixels of a tile buffer lie in the image, with no HIP in it: the host's read-backs (rt_api.cpp, rt_matte.cpp),
// rt_matte_finish_kernel (rt_scene_passes.hip) and tests/tile_order_host.cpp (which compiles it for the host on its own) use these
// functions, so that what the test walks is what the host stores.  ao_pixel (rt_scene_passes.hip), which the ambient occlusion and motion
// kernels write by, spells the block order out in its own text: calling rt_tile_block_xy there changed those kernels' instructions.
//
// A scene renders a list of tile ids into tile SLOTS: slot s of a buffer holds RT_TILE_PIXELS values per plane for tile tileIds[s], and
// tile `id` of an image tilesX tiles wide covers the pixels from (id % tilesX, id / tilesX) * RT_TILE on.  Tiles at the image's right and
// bottom edge reach past it; those pixels exist in the buffer and not in the image.  Inside a slot there are two orders:
//   ROW order    index q = ly * RT_TILE + lx: the frame's planes, the render passes, the surface passes, the mattes' state;
//   BLOCK order  index q = 64 * block + 8 * (ly % 8) + lx % 8, 8x8 blocks, RT_TILE / 8 = 16 of them per row of blocks: one wave of the
//                ambient occlusion and motion kernels is one block of pixels ("AO order").
#ifndef RT_TILE_ORDER_H
#define RT_TILE_ORDER_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_TILE_HD __host__ __device__ __forceinline__
#else
#define RT_TILE_HD inline
#endif

#ifndef RT_TILE // (rt_device.h's figures, for a program that includes this header alone)
#define RT_TILE 128
#define RT_TILE_PIXELS (RT_TILE * RT_TILE)
#endif
static_assert(RT_TILE == 128 && RT_TILE_PIXELS == 1 << 14, "the block order below is written for 16 x 16 blocks of 8 x 8 pixels");

// The image pixel at which tile `id` starts.
RT_TILE_HD void rt_tile_origin(uint32_t id, uint32_t tilesX, uint32_t &x0, uint32_t &y0)
{
    x0 = (id % tilesX) * RT_TILE;
    y0 = (id / tilesX) * RT_TILE;
}

// Block order: where in its tile the pixel of index q (0 .. RT_TILE_PIXELS - 1) lies.
RT_TILE_HD void rt_tile_block_xy(uint32_t q, uint32_t &lx, uint32_t &ly)
{
    const uint32_t blk = q >> 6, in = q & 63u;
    lx = (blk & 15u) * 8u + (in & 7u);
    ly = (blk >> 4) * 8u + (in >> 3);
}

// The host's two walks over a scene's slots (tileIds[0 .. tileCount - 1]) into an image of width x height pixels, tilesX tiles wide.
// Both rely on every id being a tile of the image, so that its origin lies inside it: build_fixed (rt_scene_parts.cpp) refuses a scene
// with any other id.
//
// Row order: f(slot, ly, at, n) once per row of each slot that the image has -- the n values from index ly * RT_TILE of the slot's plane
// belong at image offset at .. at + n - 1.
template <class F> inline void rt_tile_walk_rows(const uint32_t *tileIds, size_t tileCount, uint32_t tilesX, uint32_t width, uint32_t height, F &&f)
{
    for (size_t s = 0; s < tileCount; ++s) {
        uint32_t x0, y0;
        rt_tile_origin(tileIds[s], tilesX, x0, y0);
        const uint32_t n = width - x0 < RT_TILE ? width - x0 : RT_TILE;
        for (uint32_t ly = 0; ly < RT_TILE && y0 + ly < height; ++ly) f(s, ly, (size_t)(y0 + ly) * width + x0, n);
    }
}

// Block order: f(lp, at) once per pixel that the image has -- value lp = slot * RT_TILE_PIXELS + q of a tile-major plane belongs at image
// offset at.
template <class F> inline void rt_tile_walk_block_pixels(const uint32_t *tileIds, size_t tileCount, uint32_t tilesX, uint32_t width, uint32_t height, F &&f)
{
    for (size_t s = 0; s < tileCount; ++s) {
        uint32_t x0, y0;
        rt_tile_origin(tileIds[s], tilesX, x0, y0);
        for (uint32_t q = 0; q < RT_TILE_PIXELS; ++q) {
            uint32_t lx, ly;
            rt_tile_block_xy(q, lx, ly);
            if (x0 + lx < width && y0 + ly < height) f(s * RT_TILE_PIXELS + q, (size_t)(y0 + ly) * width + x0 + lx);
        }
    }
}

#endif
