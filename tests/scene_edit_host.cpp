// scene_edit_host.cpp -- the host arithmetic of scene edits (opencl_render_amd/csrc/rt_scene_edit.h) in a program of its own: what
// rtHipLightsCheck and rtHipMaterialsCheck decide, over a table of known answers and over seeded random tables whose expected answer
// is worked out here in 128-bit arithmetic (a channel fits when start >= 0 and start + w * h <= texturesSize, nothing wrapping).
// usage: scene_edit_host SEED COUNT; prints "failures N" and exits with 1 when N > 0.
#include "rt_scene_edit.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static int failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static int lights(const rtHipLights &l, const char *want)
{
    char text[256] = "";
    const int rc = rtedit::lights_check(&l, text, sizeof text);
    if (want) EXPECT(rc == -1 && strstr(text, want), "lights: rc %d, text '%s', expected '%s'", rc, text, want);
    else EXPECT(rc == 0 && !text[0], "lights: rc %d, text '%s', expected 0", rc, text);
    return rc;
}

static int materials(const rtHipMaterialUpdate &u, const char *want)
{
    char text[256] = "";
    const int rc = rtedit::materials_check(&u, text, sizeof text);
    if (want) EXPECT(rc == -1 && strstr(text, want), "materials: rc %d, text '%s', expected '%s'", rc, text, want);
    else EXPECT(rc == 0 && !text[0], "materials: rc %d, text '%s', expected 0", rc, text);
    return rc;
}

// one material whose colour channel is w x h at `start` in an atlas of `texels`
static void one_channel(uint32_t w, uint32_t h, int32_t start, uint32_t texels, const char *want)
{
    cl_uint2 size[5] = {};
    cl_int st[5] = {};
    static cl_uchar3 atlas[1];
    size[0].s[0] = w; size[0].s[1] = h; st[0] = start;
    rtHipMaterialUpdate u = {};
    u.replaceMaterials = 1; u.materialCount = 1; u.matSize = size; u.matStart = st; u.texturesSize = texels; u.textures = atlas; // (never read)
    materials(u, want);
}

static void known_answers()
{
    char text[64];
    EXPECT(rtedit::lights_check(nullptr, text, sizeof text) == -1 && strstr(text, "null"), "null lights");
    EXPECT(rtedit::materials_check(nullptr, text, sizeof text) == -1 && strstr(text, "null"), "null update");
    static cl_int type[1];
    static cl_float3 v[1];
    static cl_float f[1];
    rtHipLights l = { 65535u, type, v, v, v, f, f }; // (the arrays are not read)
    lights(l, nullptr);
    l.lightCount = 65536u; lights(l, "too large");
    l.lightCount = 0xffffffffu; lights(l, "too large");
    l = rtHipLights{}; lights(l, nullptr); // NULL arrays with count 0
    for (int which = 0; which < 6; ++which) {
        l = rtHipLights{ 1u, type, v, v, v, f, f };
        if (which == 0) l.lightType = nullptr;
        if (which == 1) l.lightPos = nullptr;
        if (which == 2) l.lightDir = nullptr;
        if (which == 3) l.lightCol = nullptr;
        if (which == 4) l.lightRadius = nullptr;
        if (which == 5) l.lightHalfAtt = nullptr;
        lights(l, "null light array");
    }
    one_channel(2, 3, -1, 100, "exceed");            // w > 0, start < 0
    one_channel(0, 3, -1, 100, nullptr);             // absent: its start is not read
    one_channel(4, 5, 80, 100, nullptr);             // start + w * h == texturesSize
    one_channel(4, 5, 81, 100, "exceed");            // one more
    one_channel(4, 5, 80, 99, "exceed");
    one_channel(0xffffffffu, 0xffffffffu, 0, 0xffffffffu, "exceed"); // (2^32 - 1)^2: must not wrap to something small
    one_channel(0xffffffffu, 0xffffffffu, 0x7fffffff, 0xffffffffu, "exceed");
    one_channel(0x10000u, 0x10000u, 0, 0xffffffffu, "exceed");       // 2^32 texels: wraps to 0 in 32 bits
    one_channel(0xffffffffu, 1, 0, 0xffffffffu, nullptr);
    one_channel(0xffffffffu, 1, 1, 0xffffffffu, "exceed");
    one_channel(7, 0, 100, 100, nullptr);            // w > 0, h == 0: an image without rows
    one_channel(7, 0, 101, 100, "exceed");
    one_channel(1, 1, 0, 0, "exceed");               // a texel in an empty atlas
    rtHipMaterialUpdate u = {};
    materials(u, "neither");                         // replaceMaterials 0, triMaterial NULL
    static cl_int ids[1];
    u.triMaterial = ids; materials(u, nullptr);      // ids alone; the table fields are ignored
    u.materialCount = 3; materials(u, nullptr);
    u = rtHipMaterialUpdate{}; u.replaceMaterials = 1; materials(u, nullptr); // no materials at all: legal
    u.materialCount = 1; materials(u, "null material table");
    cl_uint2 size[5] = {};
    cl_int st[5] = {};
    u.matSize = size; materials(u, "null material table");
    u.matStart = st; materials(u, nullptr);          // every channel absent, no atlas
    u.texturesSize = 4; materials(u, "null textures");
    // the spread: double sin times double sqrt, one rounding
    const float z[3] = { 0.f, 0.f, 0.f }, e[3] = { 0.f, 0.f, 2.f }, q[3] = { NAN, 0.f, 1.f };
    EXPECT(rtedit::light_spread(0.52f, z) == 0.f, "spread of a zero direction");
    EXPECT(rtedit::light_spread(0.f, e) == 0.f, "spread of radius 0");
    EXPECT(std::fabs(rtedit::light_spread(360.f, e) - 2.f * (float)std::sin(3.14159265f)) < 1e-6f, "spread of radius 360");
    EXPECT(std::fabs(rtedit::light_spread(180.f, e) - 2.f) < 1e-6f, "spread of radius 180: %g", rtedit::light_spread(180.f, e));
    EXPECT(std::isnan(rtedit::light_spread(1.f, q)), "spread of a NaN direction");
}

static void random_tables(uint64_t seed, int count)
{
    std::mt19937_64 rng(seed);
    auto pick = [&](std::initializer_list<uint32_t> v) { return *(v.begin() + rng() % v.size()); };
    static std::vector<cl_uchar3> atlas(1);
    int refused = 0, legal = 0;
    for (int i = 0; i < count; ++i) {
        const uint32_t M = (uint32_t)(rng() % 4);
        const uint32_t texels = rng() % 3 ? (uint32_t)(rng() % 5000) : pick({ 0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu });
        std::vector<cl_uint2> size(M * 5 + 1);
        std::vector<cl_int> start(M * 5 + 1);
        bool fits = true;
        for (uint32_t c = 0; c < M * 5; ++c) {
            const uint32_t w = rng() % 4 ? (uint32_t)(rng() % 40) : pick({ 0u, 1u, 0xffffu, 0x10000u, 0x10001u, 0x80000000u, 0xffffffffu });
            const uint32_t h = rng() % 4 ? (uint32_t)(rng() % 40) : pick({ 0u, 1u, 0xffffu, 0x10000u, 0x10001u, 0x80000000u, 0xffffffffu });
            const unsigned __int128 area = (unsigned __int128)w * h;
            int64_t s;
            switch (rng() % 6) {
            case 0: s = -(int64_t)(rng() % 3) - (rng() % 2 ? 0 : 0x7ffffffd); break;       // negative
            case 1: s = 0x7fffffff - (int64_t)(rng() % 3); break;                           // INT_MAX and just below
            case 2: case 3: s = (int64_t)texels - (int64_t)(area > 0xffffffffu ? 0 : (uint64_t)area) + (int64_t)(rng() % 3) - 1; break; // around the last fit
            default: s = (int64_t)(rng() % (texels ? texels : 1)); break;
            }
            if (s > 0x7fffffff) s = 0x7fffffff;
            if (s < -0x7fffffff - 1) s = -0x7fffffff - 1;
            size[c].s[0] = w; size[c].s[1] = h; start[c] = (cl_int)s;
            if (w && (s < 0 || (unsigned __int128)(uint64_t)s + area > (unsigned __int128)texels)) fits = false;
        }
        rtHipMaterialUpdate u = {};
        u.replaceMaterials = 1; u.materialCount = M; u.matSize = size.data(); u.matStart = start.data();
        u.texturesSize = texels; u.textures = atlas.data(); // (never read by the check)
        char text[256] = "";
        const int rc = rtedit::materials_check(&u, text, sizeof text);
        EXPECT(rc == (fits ? 0 : -1), "random table %d: rc %d, expected %d (%s)", i, rc, fits ? 0 : -1, text);
        EXPECT((rc == 0) == (text[0] == 0), "random table %d: rc %d with text '%s'", i, rc, text);
        (fits ? legal : refused)++;
        // every channel alone against channel_fits
        for (uint32_t c = 0; c < M * 5; ++c) {
            const uint32_t w = size[c].s[0], h = size[c].s[1];
            const bool want = !w || (start[c] >= 0 && (unsigned __int128)(uint64_t)start[c] + (unsigned __int128)w * h <= (unsigned __int128)texels);
            EXPECT(rtedit::channel_fits(w, h, start[c], texels) == want, "channel %ux%u at %d in %u", w, h, start[c], texels);
        }
        // lights: a count around the bound, one array missing now and then
        static cl_int type[1];
        static cl_float3 v[1];
        static cl_float f[1];
        rtHipLights l = { rng() % 2 ? (uint32_t)(rng() % 70000) : pick({ 0u, 1u, 65535u, 65536u, 65537u, 0xffffffffu }), type, v, v, v, f, f };
        const int missing = (int)(rng() % 12);
        if (missing == 0) l.lightType = nullptr;
        if (missing == 1) l.lightPos = nullptr;
        if (missing == 2) l.lightDir = nullptr;
        if (missing == 3) l.lightCol = nullptr;
        if (missing == 4) l.lightRadius = nullptr;
        if (missing == 5) l.lightHalfAtt = nullptr;
        const bool ok = l.lightCount < 65536u && (l.lightCount == 0 || missing > 5);
        const int lrc = rtedit::lights_check(&l, text, sizeof text);
        EXPECT(lrc == (ok ? 0 : -1), "random lights %d: count %u, missing %d: rc %d", i, l.lightCount, missing, lrc);
    }
    EXPECT(count < 100 || (refused > count / 10 && legal > count / 10), "the random tables are one-sided: %d legal, %d refused", legal, refused);
    printf("random tables: %d legal, %d refused\n", legal, refused);
}

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int count = argc > 2 ? atoi(argv[2]) : 4000;
    known_answers();
    random_tables(seed, count);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
