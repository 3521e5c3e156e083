// The ray clip's arithmetic (opencl_render_amd/csrc/rt_ray_clip.h) on the host, as a program of its own: random small grids with a random
// occupied set, the bound derived the way the scene build derives it, random rays walked by a plain DDA with the walk's quotients and tie
// rule.  Checks that no occupied cell is visited after a clipped ray's end cell, and that rays the `plain` predicate excludes stay
// unclipped.  Prints one summary line and exits 0, or prints what went wrong and exits 1.
//   ray_clip_host [seed [grids [rays per grid]]]
#include "rt_ray_clip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 32); }
    float unit() { return (float)(next() >> 8) * (1.f / 16777216.f); }         // [0, 1)
    float range(float a, float b) { return a + (b - a) * unit(); }
    uint32_t below(uint32_t n) { return next() % n; }
};

struct Grid {
    int div;
    std::vector<float> planes;   // [3][div + 1]
    std::vector<uint8_t> filled; // [div^3], x fastest
    const float *axis(int w) const { return planes.data() + w * (div + 1); }
    bool at(int x, int y, int z) const { return filled[(size_t)x + (size_t)div * ((size_t)y + (size_t)div * z)] != 0; }
};

// GetBoxAddress on one axis: the last plane strictly below p, found by halving (div need not be a power of two here: a linear search
// with the same strict '<' gives the same cell)
int cell_on(const float *pl, int div, float p)
{
    int c = 0;
    while (c + 1 < div && pl[c + 1] < p) ++c;
    return c;
}

struct Bound { uint32_t count; float tail[4 + 4 * RT_CLIP_MAX_PLANES]; int cut; };

// the scene build's steps: supports over the occupied cells (as keys, like the kernel's atomicMax), inflation, the greedy choice
Bound derive_bound(const Grid &g)
{
    static float normal[RT_CLIP_CANDIDATES][4];
    static const int candidates = rt_clip_candidates(normal);
    std::vector<uint32_t> keys(candidates, 0u);
    for (int z = 0; z < g.div; ++z)
        for (int y = 0; y < g.div; ++y)
            for (int x = 0; x < g.div; ++x) {
                if (!g.at(x, y, z)) continue;
                for (int c = 0; c < candidates; ++c) {
                    const uint32_t k = rt_clip_key(rt_clip_support(normal[c][0], normal[c][1], normal[c][2], g.axis(0)[x], g.axis(1)[y], g.axis(2)[z],
                                                                   g.axis(0)[x + 1], g.axis(1)[y + 1], g.axis(2)[z + 1]));
                    if (k > keys[c]) keys[c] = k;
                }
            }
    const float inflate = rt_clip_inflation(g.planes.data(), g.div);
    std::vector<float> off(candidates);
    for (int c = 0; c < candidates; ++c) off[c] = keys[c] ? rt_clip_unkey(keys[c]) + inflate : std::nanf("");
    int kept[RT_CLIP_MAX_PLANES];
    Bound b{};
    b.count = (uint32_t)rt_clip_choose(g.planes.data(), normal, off.data(), candidates, kept, &b.cut, g.div);
    for (uint32_t k = 0; k < b.count; ++k) {
        float *row = b.tail + 4 + 4 * k;
        row[0] = normal[kept[k]][0]; row[1] = normal[kept[k]][1]; row[2] = normal[kept[k]][2]; row[3] = off[kept[k]];
    }
    return b;
}

int failures = 0;
void complain(const char *what, const Grid &g, const float *o, const float *d, float tmin)
{
    if (++failures <= 10)
        fprintf(stderr, "FAIL %s: grid %d^3, o = (%.9g, %.9g, %.9g), d = (%.9g, %.9g, %.9g), tmin = %.9g\n", what, g.div, o[0], o[1], o[2], d[0], d[1], d[2], tmin);
}

struct Tally { long rays = 0, clipped = 0, reached = 0, visitsFull = 0, visitsClipped = 0, excluded = 0; };

// plan_ray's steps for a ray without a far end (start cell, exit, first heads, clip, end cell), then the walk
void run_ray(const Grid &g, const Bound &b, const float *o, const float *d, float tmin, Tally &tally)
{
    const int div = g.div;
    const float inf = INFINITY;
    // start point (one that lies outside the box is clamped here, where the kernels move it along the ray: such a ray is never clipped)
    int c[3];
    bool startInside = true;
    for (int w = 0; w < 3; ++w) {
        float from = o[w] + tmin * d[w];
        startInside = startInside && g.axis(w)[0] <= from && from <= g.axis(w)[div];
        if (from < g.axis(w)[0]) from = g.axis(w)[0];
        if (from > g.axis(w)[div]) from = g.axis(w)[div];
        c[w] = cell_on(g.axis(w), div, from);
    }
    float te = inf;
    for (int w = 0; w < 3; ++w)
        if (d[w] != 0.f) { const float t = (((0.f <= d[w]) ? g.axis(w)[div] : g.axis(w)[0]) - o[w]) / d[w]; if (t < te) te = t; }
    float head[3];
    for (int w = 0; w < 3; ++w) head[w] = (g.axis(w)[c[w] + ((0.f <= d[w]) ? 1 : 0)] - o[w]) / d[w];
    const float teWall = te;
    const bool plain = rt_clip_plain(false, d[0], d[1], d[2], te, head[0], head[1], head[2]);
    const bool clipped = rt_clip_ray(b.tail, b.count, false, startInside, o[0], o[1], o[2], d[0], d[1], d[2], tmin, head[0], head[1], head[2], te);
    ++tally.rays;
    if (!plain || !startInside) {
        ++tally.excluded;
        if (clipped || te != teWall) complain("a ray the predicate excludes was clipped", g, o, d, tmin);
    }
    if (clipped && !(tmin < te && te < teWall)) complain("the lowered te left (tmin, wall)", g, o, d, tmin);
    int end[3] = { -1, -1, -1 };
    if (clipped)
        for (int w = 0; w < 3; ++w) end[w] = cell_on(g.axis(w), div, o[w] + te * d[w]);
    // the walk (:380-398): the end cell ends it after its visit; x only if strictly smallest, else y if smaller than z, else z
    bool past = false, reached = false;
    long visits = 0, visitsToEnd = 0;
    for (;;) {
        ++visits;
        if (past && g.at(c[0], c[1], c[2])) { complain("an occupied cell is visited after the end cell", g, o, d, tmin); break; }
        if (!past && c[0] == end[0] && c[1] == end[1] && c[2] == end[2]) { past = reached = true; visitsToEnd = visits; }
        const int w = (head[0] < head[1] && head[0] < head[2]) ? 0 : (head[1] < head[2] ? 1 : 2);
        const bool up = 0.f <= d[w];
        if (c[w] == (up ? div - 1 : 0)) break;
        c[w] += up ? 1 : -1;
        head[w] = (g.axis(w)[c[w] + (up ? 1 : 0)] - o[w]) / d[w];
        if (visits > 3L * div + 8) { complain("the walk does not end", g, o, d, tmin); break; }
    }
    tally.visitsFull += visits;
    tally.visitsClipped += reached ? visitsToEnd : visits;
    if (clipped) ++tally.clipped;
    if (reached) ++tally.reached;
}

Grid make_grid(Rng &r, int kind)
{
    Grid g;
    g.div = 16 + (int)r.below(17);
    const int div = g.div;
    g.planes.resize(3 * (div + 1));
    const float centre = (kind & 4) ? r.range(-2000.f, 2000.f) : r.range(-1.f, 1.f); // (some boxes lie far from the origin: coarse ulps)
    for (int w = 0; w < 3; ++w) {
        float p = centre + r.range(-1.f, 0.f), *pl = g.planes.data() + w * (div + 1);
        for (int i = 0; i <= div; ++i) { pl[i] = p; p += r.range(0.01f, 0.3f) * (r.below(8) == 0 ? 0.05f : 1.f); } // non-uniform, some very thin cells
    }
    g.filled.assign((size_t)div * div * div, 0);
    auto set = [&](int x, int y, int z) { g.filled[(size_t)x + (size_t)div * ((size_t)y + (size_t)div * z)] = 1; };
    switch (kind & 3) {
    case 0: { // a frustum-like wedge: the cross-section grows along z
        for (int z = 0; z < div; ++z)
            for (int y = 0; y < div; ++y)
                for (int x = 0; x < div; ++x) {
                    const float half = 0.08f + 0.42f * (float)z / (float)div, fx = (x + 0.5f) / div - 0.5f, fy = (y + 0.5f) / div - 0.5f;
                    if (std::fabs(fx) <= half && std::fabs(fy) <= half && r.below(4) != 0) set(x, y, z);
                }
        break;
    }
    case 1: { // a ball of cells off centre
        const float cx = r.range(0.3f, 0.7f) * div, cy = r.range(0.3f, 0.7f) * div, cz = r.range(0.3f, 0.7f) * div, rad = r.range(0.15f, 0.35f) * div;
        for (int z = 0; z < div; ++z)
            for (int y = 0; y < div; ++y)
                for (int x = 0; x < div; ++x)
                    if ((x - cx) * (x - cx) + (y - cy) * (y - cy) + (z - cz) * (z - cz) <= rad * rad && r.below(3) != 0) set(x, y, z);
        break;
    }
    case 2: { // a slanted slab that touches every wall of the box: its two far corners are empty
        for (int z = 0; z < div; ++z)
            for (int y = 0; y < div; ++y)
                for (int x = 0; x < div; ++x)
                    if (std::abs(x + y - z - div / 2) <= div / 3 && r.below(5) != 0) set(x, y, z);
        for (int i = 0; i < div; ++i) { set(i, 0, 0); set(0, i, div - 1); set(div - 1, div - 1 - i, i); set(i, div - 1, div / 2); set(div / 2, i, 0); }
        break;
    }
    default: // scattered cells, all eight corners among them: nothing to clip
        for (size_t i = 0; i < g.filled.size(); ++i) g.filled[i] = r.below(10) == 0;
        for (int k = 0; k < 8; ++k) set((k & 1) ? div - 1 : 0, (k & 2) ? div - 1 : 0, (k & 4) ? div - 1 : 0);
        break;
    }
    return g;
}

} // namespace

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 0) : 1;
    const int grids = argc > 2 ? atoi(argv[2]) : 48, raysPerGrid = argc > 3 ? atoi(argv[3]) : 4000;
    Rng r{ seed * 0x9E3779B97F4A7C15ull + 0x1234567ull };
    Tally tally;
    int bounded = 0, cornerGridsKept = 0;
    for (int gi = 0; gi < grids; ++gi) {
        const int kind = gi % 8;
        const Grid g = make_grid(r, kind);
        const Bound b = derive_bound(g);
        if (b.count) ++bounded;
        if ((kind & 3) == 3 && b.count) ++cornerGridsKept;
        // the bound is a bound: every corner of every occupied cell satisfies every kept plane
        for (int z = 0; z < g.div; ++z)
            for (int y = 0; y < g.div; ++y)
                for (int x = 0; x < g.div; ++x) {
                    if (!g.at(x, y, z)) continue;
                    for (uint32_t k = 0; k < b.count; ++k) {
                        const float *p = b.tail + 4 + 4 * k;
                        for (int corner = 0; corner < 8; ++corner) {
                            const double v = (double)p[0] * g.axis(0)[x + (corner & 1)] + (double)p[1] * g.axis(1)[y + ((corner >> 1) & 1)] +
                                             (double)p[2] * g.axis(2)[z + (corner >> 2)];
                            if (!(v <= (double)p[3])) { if (++failures <= 10) fprintf(stderr, "FAIL an occupied cell's corner lies beyond a kept plane (grid %d)\n", gi); }
                        }
                    }
                }
        const int div = g.div;
        std::vector<int> occupied;
        for (size_t i = 0; i < g.filled.size(); ++i) if (g.filled[i]) occupied.push_back((int)i);
        for (int ri = 0; ri < raysPerGrid; ++ri) {
            float o[3], d[3], tmin = 0.f;
            const int style = (int)r.below(8);
            // origins: inside an occupied cell (a surface point), anywhere in the box (often beyond the bound), or on a cell face
            int cell[3];
            if (style < 5 && !occupied.empty()) { const int i = occupied[r.below((uint32_t)occupied.size())]; cell[0] = i % div; cell[1] = (i / div) % div; cell[2] = i / (div * div); }
            else for (int w = 0; w < 3; ++w) cell[w] = (int)r.below((uint32_t)div);
            for (int w = 0; w < 3; ++w) o[w] = g.axis(w)[cell[w]] + r.unit() * (g.axis(w)[cell[w] + 1] - g.axis(w)[cell[w]]);
            if (style == 5 || style == 2) { const int w = (int)r.below(3); o[w] = g.axis(w)[cell[w] + (int)r.below(2)]; }            // on a face
            if (style == 6) { const int w = (int)r.below(3); o[w] = g.axis(w)[r.below(2) ? div : 0]; }                                 // on a wall
            for (int w = 0; w < 3; ++w) d[w] = r.range(-1.f, 1.f);
            const int dirStyle = (int)r.below(10);
            if (dirStyle == 0) d[r.below(3)] *= 1e-6f;                                  // nearly parallel to one family of planes
            if (dirStyle == 1) { const int w = (int)r.below(3); d[(w + 1) % 3] *= 1e-7f; d[(w + 2) % 3] *= 1e-5f; } // nearly along an axis
            if (dirStyle == 2) d[r.below(3)] = r.below(2) ? 1e-30f : -1e-38f;           // tiny, denormal: huge or infinite heads
            if (dirStyle == 3) d[r.below(3)] = r.below(2) ? 0.f : -0.f;                 // excluded by the predicate
            if (dirStyle == 4) { d[0] = r.below(2) ? 1.f : -1.f; d[1] = d[0] * (r.below(2) ? 1.f : -1.f); d[2] = d[0]; }            // exact diagonals: tied heads on even grids
            if (r.below(6) == 0) tmin = r.range(0.f, 0.2f);
            if (r.below(40) == 0) o[r.below(3)] += r.range(-3.f, 3.f);                  // an origin outside the box
            run_ray(g, b, o, d, tmin, tally);
        }
    }
    printf("grids %d (with a bound: %d)  rays %ld  clipped %ld  end cell reached %ld  excluded by the predicate %ld  visits to the wall %ld, with the clip %ld  failures %d\n",
           grids, bounded, tally.rays, tally.clipped, tally.reached, tally.excluded, tally.visitsFull, tally.visitsClipped, failures);
    if (cornerGridsKept) { fprintf(stderr, "FAIL %d grids whose occupied cells hold all eight corners kept a plane\n", cornerGridsKept); ++failures; }
    if (!bounded || !tally.clipped || !tally.reached || !tally.excluded) { fprintf(stderr, "FAIL the cases did not exercise the clip\n"); ++failures; }
    return failures ? 1 : 0;
}
