// rt_dof_pixel.h -- the per-pixel text of the depth of field (include/raytrace_hip.h, "DEPTH OF FIELD"), in the header's order of
// operations: (a) a pixel's radius, a tap's offset and (d) the gather at one pixel.  The kernels of rt_dof.hip run it per lane;
// tests/dof_host.cpp compiles the same text for the host with the same exactness flags, so that the definition is checked against
// tests/dof_oracle.py where there is no GPU.  The reductions (b) and (c) are the kernels' own (and the host build's, sequential).
#ifndef RT_DOF_PIXEL_H
#define RT_DOF_PIXEL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RDF_FN __device__ __forceinline__
#else
#define RDF_FN static inline
#endif

#define RDF_TILE 32u      // (b): tiles of 32 x 32 pixels
#define RDF_MAX_RINGS 6u  // rtHipDepthOfFieldCheck: rings in 1..6
#define RDF_MAX_TAPS (4u * RDF_MAX_RINGS * (RDF_MAX_RINGS + 1u)) // the taps of the rings, without the centre: 168

// rz: per pixel (r, depth), what a tap reads of q beside its colour.  tileMax, nbMax: one float per tile.  All three lie in the caller's
// scratch (rtHipDepthOfFieldScratchBytes).
struct RdfArgs {
    uint32_t W, H, tilesX, tilesY, rings;
    float focus, cocScale, maxCoc, depthSoftness;
    const float *colour, *depth;
    float *rz, *tileMax, *nbMax;
    float *out;
};

// (a) the radius of the circle of confusion of a pixel at depth z: never negative, never a NaN
RDF_FN float rdf_radius(const float z, const float focus, const float cocScale, const float maxCoc)
{
    float a;
    if (z == INFINITY) a = 1.0f;
    else if (!(z > 0.f)) a = 0.0f; // (a NaN, zero, negative, -inf)
    else a = fabsf(z - focus) / z;
    float r = a * cocScale;
    if (!(r < maxCoc)) r = cocScale > 0.f ? maxCoc : 0.0f; // (also inf * 0)
    return r;
}

RDF_FN uint32_t rdf_dither(const uint32_t x, const uint32_t y) { return ((x & 1u) * 2u + (y & 1u) * 3u) & 3u; }
RDF_FN float rdf_jitter(const uint32_t j) { return ((float)j - 1.5f) * 0.25f; }

// V[v & 7].x, the corners of the unit octagon (1,0), (c,c), (0,1), (-c,c), ...: by compares, so that no table is indexed at run time
RDF_FN float rdf_vx(const uint32_t v)
{
    const float c = 0.70710678f;
    const uint32_t a = v & 7u;
    return a == 0u ? 1.0f : (a == 1u || a == 7u) ? c : (a == 2u || a == 6u) ? 0.0f : a == 4u ? -1.0f : -c;
}

// (d) tap s of ring k under the dither jit and the gather radius R: its offset from the pixel's centre and that offset's length.  The
// same for every pixel of a tile that shares the dither value.
RDF_FN void rdf_tap(const uint32_t k, const uint32_t s, const uint32_t rings, const float jit, const float R, float &ox, float &oy, float &d)
{
    const uint32_t v = s / k, m = s % k;
    const float f = (float)m / (float)k;
    const float ax = rdf_vx(v), ay = rdf_vx(v + 6u), bx = rdf_vx(v + 1u), by = rdf_vx(v + 7u); // V[v], V[v + 1]; V.y(v) = V.x(v - 2)
    const float ux = ax + (bx - ax) * f, uy = ay + (by - ay) * f;
    const float rad = (((float)k + jit) / (float)rings) * R;
    ox = ux * rad;
    oy = uy * rad;
    d = sqrtf(ox * ox + oy * oy);
}

RDF_FN float rdf_clamp01(const float r) { return !(r > 0.f) ? 0.f : (r > 1.0f ? 1.0f : r); } // (a NaN gives 0)
// is a in front of b, softly: 1 at the same depth, falling to 0 over the extent e
RDF_FN float rdf_sdc(const float a, const float b, const float e) { return a == b ? 1.0f : rdf_clamp01(1.0f - (a - b) / e); }

// (d) pixel (x, y) of a W x H image, x < W and y < H, under its tile's neighbourhood maximum R.  tap(j, t, k, s, ox, oy, d) gives tap
// t = 0.. (s of ring k) for the dither value j: rdf_tap's answer, computed (the host build) or looked up (the gather kernel).
template <class Tap>
RDF_FN void rdf_pixel(const RdfArgs &A, const uint32_t x, const uint32_t y, const float R, const Tap tap)
{
    const uint32_t W = A.W, H = A.H;
    const size_t p = (size_t)y * W + x;
    const float cr = A.colour[3 * p], cg = A.colour[3 * p + 1], cb = A.colour[3 * p + 2];
    if (!(R >= 0.5f)) { // nothing near this tile is out of focus: a copy
        A.out[3 * p] = cr;
        A.out[3 * p + 1] = cg;
        A.out[3 * p + 2] = cb;
        return;
    }
    const float r_p = A.rz[2 * p], zp = A.rz[2 * p + 1];
    const float rp = r_p < 0.5f ? 0.5f : r_p;
    const uint32_t j = rdf_dither(x, y);
    float wsum = 1.0f / (rp * rp);
    float sr = cr * wsum, sg = cg * wsum, sb = cb * wsum;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f, fw = (float)W, fh = (float)H;
    uint32_t t = 0;
    for (uint32_t k = 1; k <= A.rings; ++k)
        for (uint32_t s = 0; s < 8u * k; ++s, ++t) {
            float ox, oy, d;
            tap(j, t, k, s, ox, oy, d);
            const float X = px + ox, Y = py + oy;
            if (!(X >= 0.f && X < fw && Y >= 0.f && Y < fh)) continue; // (NaN compares false; converted only after the range test)
            const size_t q = (size_t)(int)Y * W + (size_t)(int)X;
            const float r_q = A.rz[2 * q], zq = A.rz[2 * q + 1];
            const float rq = r_q < 0.5f ? 0.5f : r_q;
            const float e = A.depthSoftness * (zp < zq ? zp : zq);
            const float fr = rdf_sdc(zq, zp, e);
            const float m2 = rq < rp ? rq : rp;
            const float reff = rq * fr + m2 * (1.0f - fr);
            const float w = rdf_clamp01((reff - d) + 0.5f) / (reff * reff);
            wsum = wsum + w;
            sr = sr + A.colour[3 * q] * w;
            sg = sg + A.colour[3 * q + 1] * w;
            sb = sb + A.colour[3 * q + 2] * w;
        }
    A.out[3 * p] = sr / wsum;
    A.out[3 * p + 1] = sg / wsum;
    A.out[3 * p + 2] = sb / wsum;
}

#endif
