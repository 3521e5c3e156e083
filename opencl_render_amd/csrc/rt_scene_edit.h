// rt_scene_edit.h -- the host arithmetic of scene edits (include/raytrace_hip.h, "SCENE EDITS: LIGHTS AND MATERIALS"): what
// rtHipLightsCheck and rtHipMaterialsCheck decide, and the one value the host derives from a light.  No HIP runtime: rt_api.cpp includes
// it, and tests/scene_edit_host.cpp compiles it into a program of its own.
#pragma once
#include "raytrace_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

namespace rtedit {

// A light's spread, raytrace_opencl.c:594: double sin times double sqrt, then one rounding to float.  A scene build (build_lights) and a
// light edit both call this.
inline float light_spread(float radius, const float dir[3])
{
    const float dd = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
    return (float)(std::sin((double)((radius / 2.f) * 3.14159265f / 180.f)) * std::sqrt((double)dd));
}

// Does a channel of w x h texels that starts at `start` lie inside an atlas of `texels` texels?  w and h are full 32-bit values: their
// product fits 64 bits, and the start is compared against the room that is left instead of added.  w == 0 is an absent channel: nothing
// of it is read.  (w > 0, h == 0: an image without rows, legal wherever it starts inside the atlas.)
inline bool channel_fits(uint32_t w, uint32_t h, int32_t start, uint32_t texels)
{
    if (w == 0u) return true;
    if (start < 0) return false;
    const uint64_t area = (uint64_t)w * (uint64_t)h;
    return area <= (uint64_t)texels && (uint64_t)start <= (uint64_t)texels - area;
}

// 0, or -1 with the reason in text[0 .. n)
inline int lights_check(const rtHipLights *l, char *text, size_t n)
{
    if (!l) { snprintf(text, n, "null argument"); return -1; }
    if (l->lightCount >= 65536u) { snprintf(text, n, "lightCount %u too large", l->lightCount); return -1; }
    if (l->lightCount && (!l->lightType || !l->lightPos || !l->lightDir || !l->lightCol || !l->lightRadius || !l->lightHalfAtt)) {
        snprintf(text, n, "null light array with lightCount %u", l->lightCount);
        return -1;
    }
    return 0;
}

inline int materials_check(const rtHipMaterialUpdate *u, char *text, size_t n)
{
    if (!u) { snprintf(text, n, "null argument"); return -1; }
    if (!u->replaceMaterials) {
        if (!u->triMaterial) { snprintf(text, n, "neither material tables (replaceMaterials) nor triMaterial given"); return -1; }
        return 0;
    }
    if (u->materialCount && (!u->matSize || !u->matStart)) { snprintf(text, n, "null material table with materialCount %u", u->materialCount); return -1; }
    if (u->texturesSize && !u->textures) { snprintf(text, n, "null textures with texturesSize %u", u->texturesSize); return -1; }
    for (uint64_t m = 0; m < (uint64_t)u->materialCount * 5; ++m) {
        const uint32_t w = u->matSize[m].s[0], h = u->matSize[m].s[1];
        if (!channel_fits(w, h, u->matStart[m], u->texturesSize)) {
            snprintf(text, n, "material channel %llu: %ux%u texels at %d exceed the %u-texel atlas", (unsigned long long)m, w, h, u->matStart[m], u->texturesSize);
            return -1;
        }
    }
    return 0;
}

} // namespace rtedit
