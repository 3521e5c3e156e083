// rt_motion_blur_pixel.h -- the per-pixel text of the vector motion blur (include/raytrace_hip.h, "MOTION BLUR"), in the header's order of
// operations: (a) a pixel's velocity and (d) the gather at one pixel.  The kernels of rt_motion_blur.hip run it per lane;
// tests/motion_blur_host.cpp compiles the same text for the host with the same exactness flags, so that the definition is checked against
// tests/motion_blur_oracle.py where there is no GPU.  The reductions (b) and (c) are the kernels' own (and the host build's, sequential).
#ifndef RT_MOTION_BLUR_PIXEL_H
#define RT_MOTION_BLUR_PIXEL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RMB_FN __device__ __forceinline__
#else
#define RMB_FN static inline
#endif

#define RMB_TILE 32u        // (b): tiles of 32 x 32 pixels
#define RMB_TILE_FLOATS 4u  // a tile's (vx, vy, l) and a pad word: 16 bytes, one aligned load

// lz: per pixel (l, depth), what a tap reads of q beside its colour -- 8 bytes where the motion and the depth are 12 and a square root
// and a division more.  tileMax, nbMax: RMB_TILE_FLOATS per tile.  All three lie in the caller's scratch (rtHipMotionBlurScratchBytes).
struct RmbArgs {
    uint32_t W, H, tilesX, tilesY, taps;
    float shutter, maxBlur, depthSoftness;
    const float *colour, *motion, *depth;
    float *lz, *tileMax, *nbMax;
    float *out;
};

// (a) the velocity of a pixel whose motion is (mx, my): half the shutter's share of the flow, capped at maxBlur
RMB_FN void rmb_velocity(const float mx, const float my, const float shutter, const float maxBlur, float &vx, float &vy, float &l)
{
    const float s = shutter * 0.5f;
    vx = mx * s;
    vy = my * s;
    const float l2 = vx * vx + vy * vy;
    if (!(l2 < INFINITY)) { vx = 0.f; vy = 0.f; l = 0.f; } // (a NaN or an overflow: the pixel stands still)
    else l = sqrtf(l2);
    if (l > maxBlur) {
        const float k = maxBlur / l;
        vx = vx * k;
        vy = vy * k;
        l = maxBlur;
    }
}

RMB_FN float rmb_clamp01(const float r) { return !(r > 0.f) ? 0.f : (r > 1.0f ? 1.0f : r); } // (a NaN gives 0)
// is a in front of b, softly: 1 at the same depth, falling to 0 over the extent e
RMB_FN float rmb_sdc(const float a, const float b, const float e) { return a == b ? 1.0f : rmb_clamp01(1.0f - (a - b) / e); }
RMB_FN float rmb_cone(const float d, const float l) { return rmb_clamp01(1.0f - d / l); }
RMB_FN float rmb_cyl(const float d, const float l)
{
    const float r = rmb_clamp01((d - 0.95f * l) / (1.05f * l - 0.95f * l));
    return 1.0f - (r * r) * (3.0f - 2.0f * r);
}

// (d) pixel (x, y) of a W x H image, x < W and y < H, under its tile's neighbourhood maximum (nx, ny, nl)
RMB_FN void rmb_pixel(const RmbArgs &A, const uint32_t x, const uint32_t y, const float nx, const float ny, const float nl)
{
    const uint32_t W = A.W, H = A.H;
    const size_t p = (size_t)y * W + x;
    const float cr = A.colour[3 * p], cg = A.colour[3 * p + 1], cb = A.colour[3 * p + 2];
    if (!(nl >= 0.5f)) { // nothing moves near this tile: a copy
        A.out[3 * p] = cr;
        A.out[3 * p + 1] = cg;
        A.out[3 * p + 2] = cb;
        return;
    }
    const float l_p = A.lz[2 * p], zp = A.lz[2 * p + 1];
    const float lp = l_p < 0.5f ? 0.5f : l_p;
    float wsum = 1.0f / lp;
    float sr = cr * wsum, sg_ = cg * wsum, sb = cb * wsum;
    const uint32_t j = ((x & 1u) * 2u + (y & 1u) * 3u) & 3u;
    const float jit = ((float)j - 1.5f) * 0.25f;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f, ftaps = (float)A.taps, fw = (float)W, fh = (float)H;
    for (uint32_t i = 0; i < A.taps; ++i) {
        const float u = (((float)i + 0.5f) + jit) / ftaps, sg = u * 2.0f - 1.0f;
        const float X = px + nx * sg, Y = py + ny * sg;
        if (!(X >= 0.f && X < fw && Y >= 0.f && Y < fh)) continue; // (NaN compares false; converted only after the range test)
        const size_t q = (size_t)(int)Y * W + (size_t)(int)X;
        const float d = fabsf(sg) * nl;
        const float l_q = A.lz[2 * q], zq = A.lz[2 * q + 1];
        const float lq = l_q < 0.5f ? 0.5f : l_q;
        const float e = A.depthSoftness * (zp < zq ? zp : zq);
        const float f = rmb_sdc(zq, zp, e), bk = rmb_sdc(zp, zq, e);
        const float w = (f * rmb_cone(d, lq) + bk * rmb_cone(d, lp)) + (rmb_cyl(d, lq) * rmb_cyl(d, lp)) * 2.0f;
        wsum = wsum + w;
        sr = sr + A.colour[3 * q] * w;
        sg_ = sg_ + A.colour[3 * q + 1] * w;
        sb = sb + A.colour[3 * q + 2] * w;
    }
    A.out[3 * p] = sr / wsum;
    A.out[3 * p + 1] = sg_ / wsum;
    A.out[3 * p + 2] = sb / wsum;
}

#endif
