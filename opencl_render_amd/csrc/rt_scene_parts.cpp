// rt_scene_parts.cpp -- the PARTS a resident scene is built in, each with its own device allocations (rt_host.h), so that the drop-in
// layer's cache (RaytraceAll, rt_api.cpp) can replace what changed between two calls -- typically the camera -- and keep the rest in
// HBM.  A builder drops the part the scene holds, fills a local DevPart and installs it; after a builder that fails the scene holds
// neither, and its caller destroys the scene.
#include "rt_host.h"
#include "rt_launch.h"
#include "rt_scene_edit.h"

#include <chrono>
#include <cmath>
#include <cstdio>

namespace rthost {

int build_fixed(rtHipScene *sc, const rtHipSceneDesc *d, const cl_uint *tileIds, cl_uint tileCount)
{
    DevPart part;
    const uint32_t tilesX = (d->width + RT_TILE - 1) / RT_TILE, tilesY = (d->height + RT_TILE - 1) / RT_TILE;
    sc->width = d->width; sc->height = d->height; sc->tilesX = tilesX;
    const bool allTiles = (tileIds == nullptr || tileCount == 0);
    if (allTiles) {
        sc->tileIds.resize((size_t)tilesX * tilesY);
        for (uint32_t i = 0; i < tilesX * tilesY; ++i) sc->tileIds[i] = i;
    } else {
        sc->tileIds.assign(tileIds, tileIds + tileCount);
        for (cl_uint t : sc->tileIds)
            if (t >= tilesX * tilesY) return fail("tile id %u out of range (%u tiles)", t, tilesX * tilesY);
    }
    const uint32_t nt = (uint32_t)sc->tileIds.size();
    RtDevScene &D = sc->dev;
    D.width = d->width; D.height = d->height;
    D.tileCount = nt; D.tilesX = tilesX;
    const cl_uint *ids = nullptr;
    if (sc->upload(part, sc->tileIds.data(), nt, &ids, "tileIds")) return -1;
    D.tileIds = ids;
    uint16_t *buf = nullptr;
    if (sc->alloc<uint16_t>(part, (uint64_t)nt * 3 * RT_TILE_PIXELS, &buf)) return -1;
    HIP_OK(hipMemsetAsync(buf, 0, (uint64_t)nt * 3 * RT_TILE_PIXELS * 2, sc->stream));
    D.tileBuf = buf;
    unsigned long long *st = nullptr;
    if (sc->alloc<unsigned long long>(part, 8, &st)) return -1;
    HIP_OK(hipMemsetAsync(st, 0, 64, sc->stream));
    D.stats = st;
    if (sc->alloc<uint32_t>(part, 1, &sc->prepErr)) return -1;
    HIP_OK(hipMemsetAsync(sc->prepErr, 0, 4, sc->stream));
    // bump: xPart/yPart = (float)sin(dh*PI_F/2.f), normalPart factors = (float)cos(...) (raytrace_opencl.c:251-253) with
    // dh = hE/255.f - h0/255.f.  Only 256x256 byte pairs exist: tabulate with the HOST libm -- the library the reference's
    // C path calls -- so the device result is that library's, bit for bit.
    std::vector<float> tsin(65536), tcos(65536);
    for (int e = 0; e < 256; ++e)
        for (int h = 0; h < 256; ++h) {
            const float fe = (float)e / 255.f, fh = (float)h / 255.f;
            const float arg = (fe - fh) * 3.14159265f / 2.f;
            tsin[(e << 8) | h] = (float)std::sin((double)arg);
            tcos[(e << 8) | h] = (float)std::cos((double)arg);
        }
    if (sc->upload(part, tsin.data(), tsin.size(), &D.bumpSin, "bumpSin")) return -1;
    if (sc->upload(part, tcos.data(), tcos.size(), &D.bumpCos, "bumpCos")) return -1;
    HIP_OK(sc->stager.drain());
    sc->install(PART_FIXED, std::move(part));
    return 0;
}

// camera vectors + the per-pixel candidate lists: uploaded as they are, the tile-major view of this instance's tiles is made
// on the device (rt_scene_prep.hip)
int build_camera(rtHipScene *sc, const rtHipSceneDesc *d)
{
    sc->drop_part(PART_CAMERA); // (before the new one is made: the two need not fit side by side)
    DevPart part;
    RtDevScene &D = sc->dev;
    for (int i = 0; i < 3; ++i) { D.eye[i] = d->eye[i]; D.topLeft[i] = d->eyeToTopLeft[i]; D.lr[i] = d->leftToRight[i]; D.tb[i] = d->topToBottom[i]; }
    D.pixelSizeInv = d->pixelSizeInv;
    const uint64_t P = (uint64_t)d->width * d->height;
    if (!d->camStart || !d->camEnd) return fail("null cameraPixelTriangleListStart/End");
    if (d->camListSize && !d->camList) return fail("null cameraPixelTriangleList");
    if (d->camListSize > 0xffffffffull) return fail("camera list too large");
    const cl_uint *srcStart = nullptr, *srcEnd = nullptr;
    DevPart scratch; // the row-major ranges are only needed until the tile-major ones exist
    void *p0 = nullptr, *p1 = nullptr;
    HIP_OK(scratch.get(&p0, P * 4)); HIP_OK(scratch.get(&p1, P * 4));
    HIP_OK(sc->stager.copy(p0, d->camStart, P * 4));
    HIP_OK(sc->stager.copy(p1, d->camEnd, P * 4));
    srcStart = (const cl_uint *)p0; srcEnd = (const cl_uint *)p1;
    if (sc->upload(part, d->camList, d->camListSize, &D.camList, "camList")) return -1;
    sc->camListSize = d->camListSize;
    uint32_t *ts = nullptr, *te = nullptr;
    const uint64_t n = (uint64_t)D.tileCount * RT_TILE_PIXELS;
    if (sc->alloc<uint32_t>(part, n, &ts) || sc->alloc<uint32_t>(part, n, &te)) return -1;
    HIP_OK(rtp_camera_ranges(d->width, d->height, D.tilesX, D.tileIds, D.tileCount, srcStart, srcEnd, d->camListSize, ts, te, sc->prepErr, sc->stream));
    D.camStart = ts; D.camEnd = te;
    HIP_OK(hipStreamSynchronize(sc->stream)); // scratch dies here
    sc->install(PART_CAMERA, std::move(part));
    return 0;
}

// geometry: upload the ABI arrays, reshape on the device (rt_prepare_triangles), drop the originals
int build_geometry(rtHipScene *sc, const rtHipSceneDesc *d)
{
    sc->drop_part(PART_GEOMETRY);
    DevPart part;
    RtDevScene &D = sc->dev;
    D.triangleCount = d->triangleCount;
    if (d->triangleCount && (!d->triIndex || !d->triMaterial || !d->triUv || !d->triNormal)) return fail("null triangle array");
    if (d->vertexCount && !d->vertex) return fail("null vertex array");
    void *dv = nullptr, *di = nullptr, *dm = nullptr, *du = nullptr, *dn = nullptr;
    const uint64_t T = d->triangleCount, V = d->vertexCount;
    DevPart scratch;
    HIP_OK(scratch.get(&dv, V * 16)); HIP_OK(scratch.get(&di, T * 16)); HIP_OK(scratch.get(&dm, T * 4));
    HIP_OK(scratch.get(&du, T * 24)); HIP_OK(scratch.get(&dn, T * 48));
    HIP_OK(sc->stager.copy(dv, d->vertex, V * 16));
    HIP_OK(sc->stager.copy(di, d->triIndex, T * 16));
    HIP_OK(sc->stager.copy(dm, d->triMaterial, T * 4));
    HIP_OK(sc->stager.copy(du, d->triUv, T * 24));
    HIP_OK(sc->stager.copy(dn, d->triNormal, T * 48));
    float *rec = nullptr, *shade = nullptr;
    if (sc->alloc<float>(part, T * 16, &rec) || sc->alloc<float>(part, T * RT_TRI_SHADE_WORDS, &shade)) return -1; // (hipMalloc: each row is one line)
    // ids are checked on the device before anything gathers through them; a scene with a bad id fails at the end of the build
    HIP_OK(rtp_validate(d->triangleCount, d->vertexCount, d->materialCount, di, (const int *)dm, 0, nullptr, nullptr, 0, nullptr, sc->prepErr, sc->stream));
    HIP_OK(hipStreamSynchronize(sc->stream));
    if (sc->check_prep() != 0) return -1; // rt_prepare_triangles would gather out of bounds
    HIP_OK(rtk_launch_prepare(d->triangleCount, dv, di, dm, du, dn, rec, shade, sc->stream));
    D.triRec = rec; D.triShade = shade;
    HIP_OK(hipStreamSynchronize(sc->stream));
    sc->install(PART_GEOMETRY, std::move(part));
    return 0;
}

// What the host derives from the split planes ([3][257], one array per axis): the cell estimate table of rt_device.h (cellLut, [3][256])
// and planesTame.  One arithmetic for a scene build and a geometry update.
void grid_tables(const float *planes, uint8_t *lut, uint32_t *tame)
{
    for (int w = 0; w < 3; ++w) {
        const float *pw = planes + w * (RT_GRID_DIV + 1);
        const float lo = pw[0], step = (pw[RT_GRID_DIV] - pw[0]) / 256.f;
        int c = 0;
        for (int i = 0; i < 256; ++i) {
            const float x = lo + ((float)i + 0.5f) * step;
            while (c < RT_GRID_DIV - 1 && pw[c + 1] < x) ++c; // (planes ascend: the cell index only ever grows with i)
            lut[w * 256 + i] = (uint8_t)c;
        }
    }
    *tame = 1u;
    for (int i = 0; i < 3 * (RT_GRID_DIV + 1); ++i) {
        const float m = std::fabs(planes[i]);
        if (!(m == 0.f || (m >= 0x1p-60f && m <= 0x1p39f))) *tame = 0u;
    }
}

// The planes' buffer as the host makes it (rt_ray_clip.h): the [3][257] planes, no clip plane yet, the candidate normals for the bound kernel.
void clip_buffer_init(const float *planes, float *buffer)
{
    static const std::vector<float> normals = [] { std::vector<float> n(4 * RT_CLIP_CANDIDATES); (void)rt_clip_candidates(reinterpret_cast<float (*)[4]>(n.data())); return n; }();
    memset(buffer, 0, sizeof(float) * RT_CLIP_FLOATS);
    memcpy(buffer, planes, sizeof(float) * 3 * (RT_GRID_DIV + 1));
    memcpy(buffer + RT_CLIP_NORMALS_AT, normals.data(), sizeof(float) * normals.size());
}
// The bound's supports over the occupancy words `words`, into the planes' buffer `boxMin` and back to sc->clipKeys (complete after a
// synchronisation of `st`) ...
hipError_t clip_bound_issue(rtHipScene *sc, const unsigned long long *words, float *boxMin, hipStream_t st)
{
    uint32_t *keys = reinterpret_cast<uint32_t *>(boxMin + RT_CLIP_KEYS_AT);
    const hipError_t e = rtp_clip_support(words, boxMin, boxMin + RT_CLIP_NORMALS_AT, RT_CLIP_CANDIDATES, keys, st);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(sc->clipKeys, keys, sizeof sc->clipKeys, hipMemcpyDeviceToHost, st);
}
// ... and, after that synchronisation, the planes to keep: their number in *count and what the planes' buffer holds from RT_CLIP_AT on in
// `tail` ([4 + 4 * RT_CLIP_MAX_PLANES]), written behind the planes of `boxMin` on `st`.  The scene's own copy (clipCount, clipTail) is the
// caller's to set once the grid they belong to is the scene's: a build or a move that fails after this leaves the scene as it was.
hipError_t clip_bound_commit(const rtHipScene *sc, const float *planes, float *boxMin, hipStream_t st, uint32_t *count, float *tail)
{
    float normal[RT_CLIP_CANDIDATES][4], off[RT_CLIP_CANDIDATES];
    (void)rt_clip_candidates(normal);
    const float inflate = rt_clip_inflation(planes);
    for (int c = 0; c < RT_CLIP_CANDIDATES; ++c) off[c] = sc->clipKeys[c] ? rt_clip_unkey(sc->clipKeys[c]) + inflate : std::nanf(""); // (key 0: no cell is occupied)
    int kept[RT_CLIP_MAX_PLANES];
    const int n = rt_clip_choose(planes, normal, off, RT_CLIP_CANDIDATES, kept, nullptr);
    memset(tail, 0, sizeof sc->clipTail);
    for (int k = 0; k < n; ++k) {
        float *row = tail + 4 + 4 * k;
        row[0] = normal[kept[k]][0]; row[1] = normal[kept[k]][1]; row[2] = normal[kept[k]][2]; row[3] = off[kept[k]];
    }
    *count = (uint32_t)n;
    const uint32_t applied = sc->tune.rayClip ? *count : 0u;
    memcpy(tail, &applied, 4);
    return hipMemcpyAsync(boxMin + RT_CLIP_AT, tail, sizeof sc->clipTail, hipMemcpyHostToDevice, st);
}

// the grid as the ABI hands it over, plus its dense view for the wavefront trace kernel, built on the device
int build_grid(rtHipScene *sc, const rtHipSceneDesc *d)
{
    sc->drop_part(PART_GRID);
    DevPart part;
    RtDevScene &D = sc->dev;
    if (!d->boxMin) return fail("null sceneBoxMin");
    std::vector<float> planes(3 * (RT_GRID_DIV + 1));
    for (int w = 0; w < 3; ++w)
        for (int i = 0; i <= RT_GRID_DIV; ++i) planes[w * (RT_GRID_DIV + 1) + i] = d->boxMin[i].s[w];
    std::vector<float> planeBuffer(RT_CLIP_FLOATS);
    clip_buffer_init(planes.data(), planeBuffer.data());
    if (sc->upload(part, planeBuffer.data(), planeBuffer.size(), &D.boxMin, "boxMin")) return -1;
    std::vector<uint8_t> lut(3 * 256);
    grid_tables(planes.data(), lut.data(), &D.planesTame);
    if (sc->upload(part, lut.data(), lut.size(), &D.cellLut, "cellLut")) return -1;
    const uint64_t cells = (uint64_t)RT_GRID_DIV * RT_GRID_DIV * RT_GRID_DIV;
    if (!d->gridStart) return fail("null scenePixelTriangleListStart");
    const uint64_t listSize = sc->haveGridListSize ? sc->gridListSizeHint : d->gridStart[cells]; // (the last start = the list's length; read from the device by scene_build when the array lives there)
    if (listSize && !d->gridList) return fail("null scenePixelTriangleList");
    if (sc->upload(part, d->gridStart, cells + 1, &D.gridStart, "gridStart")) return -1;
    if (sc->upload(part, d->gridList, listSize, &D.gridList, "gridList")) return -1;
    // (the triangle count the entries are checked against is this scene's: geometry is built before the grid)
    HIP_OK(rtp_validate(D.triangleCount, 0, 0, nullptr, nullptr, 0, nullptr, D.gridStart, listSize, D.gridList, sc->prepErr, sc->stream));
    HIP_OK(hipStreamSynchronize(sc->stream));
    if (sc->check_prep() != 0) return -1; // the dense view walks the lists through the starts
    const size_t blocks = (size_t)(RT_GRID_DIV / 4) * (RT_GRID_DIV / 4) * (RT_GRID_DIV / 4);
    unsigned long long *words = nullptr;
    uint32_t *sparse = nullptr;
    const size_t sparseWords = (size_t)3 * ((63u << 16 | 63u << 8 | 63u) + 1u);
    if (listSize >= RT_PAIR_LIMIT) return fail("scenePixelTriangleList has 2^28 entries or more: pair indices would not fit the trace kernel's records");
    if (sc->alloc<unsigned long long>(part, blocks, &words) || sc->alloc<uint32_t>(part, sparseWords, &sparse)) return -1;
    HIP_OK(hipMemsetAsync(sparse, 0, sparseWords * 4, sc->stream));
    DevPart scratch;
    uint32_t *pairOrder = nullptr, *pairCount = nullptr;
    void *tmp = nullptr;
    size_t tmpBytes = 0;
    HIP_OK(rtp_dense_grid(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &tmpBytes, sc->stream));
    HIP_OK(scratch.get((void **)&pairOrder, (size_t)listSize * 4)); HIP_OK(scratch.get((void **)&pairCount, (size_t)listSize * 4));
    HIP_OK(scratch.get(&tmp, tmpBytes));
    HIP_OK(rtp_dense_grid(D.gridStart, D.gridList, words, sparse, pairOrder, pairCount, tmp, &tmpBytes, sc->stream));
    HIP_OK(clip_bound_issue(sc, words, const_cast<float *>(D.boxMin), sc->stream));
    float *pairRec = nullptr;
    if (sc->alloc<float>(part, (uint64_t)listSize * 16, &pairRec)) return -1;
    HIP_OK(rtk_launch_gather_pairs((uint32_t)listSize, pairOrder, pairCount, D.triRec, pairRec, sc->stream));
    D.gridBits = words; D.gridBlockSparse = sparse; D.pairRec = pairRec;
    sc->gridListSize = listSize;
    D.cellCount = 0; // informational; the kernels find a cell's records through the block table
    HIP_OK(hipStreamSynchronize(sc->stream));
    uint32_t clipCount = 0;
    float clipTail[4 + 4 * RT_CLIP_MAX_PLANES];
    HIP_OK(clip_bound_commit(sc, planes.data(), const_cast<float *>(D.boxMin), sc->stream, &clipCount, clipTail));
    HIP_OK(hipStreamSynchronize(sc->stream));
    sc->clipCount = clipCount;
    memcpy(sc->clipTail, clipTail, sizeof sc->clipTail);
    sc->install(PART_GRID, std::move(part));
    return 0;
}

// The path class (RtDevScene::pathClass) is decided per part: the materials (every reflection, transparency and luminance channel absent or one
// black texel, every height map absent or one texel; the colour channel is free) and the lights (at most one, of any type).
bool materials_admit_opaque_diffuse(const rtHipSceneDesc *d)
{
    for (uint32_t m = 0; m < d->materialCount; ++m)
        for (int c = 1; c < 5; ++c) { // reflection, transparency, bump, luminance (raytrace_opencl.h:14-22)
            const uint32_t w = d->matSize[5 * m + c].s[0], h = d->matSize[5 * m + c].s[1];
            if (w == 0u) continue; // absent (matRec descriptor 0)
            if (w != 1u || h != 1u) return false; // an image
            if (c == 3) continue; // a one-texel height map: any texel
            const cl_uchar *px = d->textures[d->matStart[5 * m + c]].s;
            if (px[0] | px[1] | px[2]) return false; // only 0x80000000, black, reads as 0
        }
    return true;
}
bool lights_admit_opaque_diffuse(const rtHipSceneDesc *d) { return d->lightCount <= 1u; }
void derive_path_class(rtHipScene *sc)
{
    sc->dev.pathClass = (sc->tune.logicClass && sc->classMaterials && sc->classLights) ? RT_PATH_CLASS_OPAQUE_DIFFUSE : RT_PATH_CLASS_GENERAL;
}

// the per-material channel descriptors of rt_device.h (the channel starts have been checked against the atlas): one arithmetic for a
// scene build and a materials edit
std::vector<uint32_t> material_records(const rtHipSceneDesc *d)
{
    std::vector<uint32_t> rec((size_t)d->materialCount * 8, 0u);
    for (uint32_t m = 0; m < d->materialCount; ++m)
        for (int c = 0; c < 5; ++c) {
            const uint32_t w = d->matSize[5 * m + c].s[0], h = d->matSize[5 * m + c].s[1];
            uint32_t desc = 0u;
            if (w == 1u && h == 1u) {
                const cl_uchar *px = d->textures[d->matStart[5 * m + c]].s;
                desc = 0x80000000u | (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
            } else if (w) desc = 0x40000000u; // (w > 0, h == 0: an image without rows -- the general path indexes it as the reference would)
            rec[8 * (size_t)m + c] = desc;
        }
    return rec;
}

// a light's spread per light (rt_scene_edit.h); one element at least
std::vector<float> light_spreads(uint32_t count, const cl_float3 *dir, const cl_float *radius)
{
    std::vector<float> spread(count ? count : 1, 0.f);
    for (uint32_t j = 0; j < count; ++j) spread[j] = rtedit::light_spread(radius[j], dir[j].s);
    return spread;
}

int build_materials(rtHipScene *sc, const rtHipSceneDesc *d)
{
    sc->drop_part(PART_MATERIALS);
    DevPart part;
    RtDevScene &D = sc->dev;
    D.materialCount = d->materialCount;
    D.texelCount = d->texturesSize ? d->texturesSize : 1;
    if (sc->upload(part, (const uint32_t *)d->matSize, (uint64_t)d->materialCount * 10, &D.matSize, "materialImageSize")) return -1;
    if (sc->upload(part, (const int32_t *)d->matStart, (uint64_t)d->materialCount * 5, &D.matStart, "materialImageStart")) return -1;
    if (sc->upload(part, (const uint8_t *)d->textures, (uint64_t)d->texturesSize * 4, &D.textures, "textures")) return -1;
    for (uint32_t m = 0; m < d->materialCount * 5; ++m) {
        const uint64_t w = d->matSize[m].s[0], h = d->matSize[m].s[1];
        if (w && ((int64_t)d->matStart[m] < 0 || (uint64_t)d->matStart[m] + w * h > d->texturesSize))
            return fail("material channel %u: %llux%llu texels at %d exceed the %u-texel atlas", m, (unsigned long long)w, (unsigned long long)h, d->matStart[m], d->texturesSize);
    }
    {
        const std::vector<uint32_t> rec = material_records(d);
        if (sc->upload(part, rec.data(), rec.size(), &D.matRec, "matRec")) return -1;
    }
    sc->classMaterials = materials_admit_opaque_diffuse(d); // (the channel starts were checked above)
    derive_path_class(sc);
    HIP_OK(sc->stager.drain());
    sc->install(PART_MATERIALS, std::move(part));
    return 0;
}

int build_lights(rtHipScene *sc, const rtHipSceneDesc *d)
{
    sc->drop_part(PART_LIGHTS);
    DevPart part;
    RtDevScene &D = sc->dev;
    if (d->lightCount >= 65536u) return fail("lightCount %u too large", d->lightCount);
    D.lightCount = d->lightCount;
    if (d->lightCount && (!d->lightType || !d->lightPos || !d->lightDir || !d->lightCol || !d->lightRadius || !d->lightHalfAtt))
        return fail("null light array with lightCount %u", d->lightCount); // (the spread below reads two of them before upload() would notice)
    const std::vector<float> spread = light_spreads(d->lightCount, d->lightDir, d->lightRadius);
    if (sc->upload(part, d->lightType, d->lightCount, &D.lightType, "lightType")) return -1;
    if (sc->upload(part, (const float *)d->lightPos, (uint64_t)d->lightCount * 4, &D.lightPos, "lightPosition")) return -1;
    if (sc->upload(part, (const float *)d->lightDir, (uint64_t)d->lightCount * 4, &D.lightDir, "lightDirection")) return -1;
    if (sc->upload(part, (const float *)d->lightCol, (uint64_t)d->lightCount * 4, &D.lightCol, "lightColour")) return -1;
    if (sc->upload(part, d->lightRadius, d->lightCount, &D.lightRadius, "lightRadius")) return -1;
    if (sc->upload(part, d->lightHalfAtt, d->lightCount, &D.lightHalfAtt, "lightHalfAttenuationDistance")) return -1;
    if (sc->upload(part, spread.data(), d->lightCount, &D.lightSpread, "lightSpread")) return -1;
    sc->classLights = lights_admit_opaque_diffuse(d);
    derive_path_class(sc);
    HIP_OK(sc->stager.drain());
    sc->install(PART_LIGHTS, std::move(part));
    return 0;
}

// wavefront pipeline buffers: worst case every pixel of every sample in a batch becomes a path
int build_wavefront(rtHipScene *sc, uint32_t sampleCount)
{
    for (auto &G : sc->groups)
        if (G.stream) (void)hipStreamSynchronize(G.stream);
    sc->groups.clear();
    sc->drop_part(PART_WAVEFRONT);
    DevPart part;
    RtDevScene &D = sc->dev;
    D.sampleCount = sampleCount;
    sc->window = default_window(sampleCount); // (a scene starts, and a cached scene whose S changed starts again, with the default window)
    sc->lastWindow = rtHipSampleWindow{};
    apply_window(sc, sc->window);             // (the groups' views follow in refresh_views)
    sc->planRounds = 0; // the next frame watches its queue again
    sc->unverified = false;
    const Tuning &T = sc->tune;
    const uint32_t nt = D.tileCount;
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, sc->device));
    const uint32_t cus = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
    const uint64_t pix = (uint64_t)nt * RT_TILE_PIXELS;
    const uint32_t extraFactor = std::min<uint32_t>(std::max<uint32_t>(T.extraFactor, 1u), 16u);
    // per path: rng, meta, outc, ring, shadow-wait state, look-ahead answer + slot, primary hit, finished colour; per queue entry (two per
    // path): path id and answer per round parity; per entry (2 + extraFactor per path): the 64-byte entry per round parity, rank, class,
    // sorted position
    const uint64_t perPath = 8 + 16 + 16 + (uint64_t)RT_RING * 48 + 3 * 16 + 8 + 4 + 16 + 16 + 2 * 2 * (4 + 8) + (uint64_t)(2 + extraFactor) * (2 * 64 + 4 + 2 + 4);
    // bytes of path state per sample batch: more samples per batch = fewer, fuller rounds (S=4 at 1080p: 5.0 ms with one
    // sample per batch, 4.5 ms with all four); 24 GB of the 288 GB, and never more than a third of what is free
    uint64_t budget = 24ull << 30;
    {
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB / 3 < budget) budget = freeB / 3;
    }
    if (T.stateMb) budget = T.stateMb << 20;
    uint64_t sb = budget / (perPath * (pix ? pix : 1));
    if (sb < 1) sb = 1;
    if (sb > sampleCount) sb = sampleCount;
    if (sb > 65535) sb = 65535; // the primary kernel's gridDim.y
    sc->samplesPerBatch = (uint32_t)sb;
    uint32_t groupCount = std::min<uint32_t>(std::max<uint32_t>(T.groups, 1u), 16u);
    if (groupCount > nt) groupCount = nt ? (uint32_t)nt : 1u;
    const bool multiLight = D.lightCount > 1;
    sc->wfMultiLight = multiLight;
    HIP_OK(sc->forkEvent.make(hipEventDisableTiming));
    sc->groups.resize(groupCount);
    for (uint32_t g = 0; g < groupCount; ++g) {
        rtHipScene::Group &G = sc->groups[g];
        const uint32_t slot0 = (uint32_t)((uint64_t)nt * g / groupCount), slot1 = (uint32_t)((uint64_t)nt * (g + 1) / groupCount);
        G.slot0 = slot0; G.slot1 = slot1;
        if (g > 0) HIP_OK(G.stream.make(hipStreamNonBlocking));
        HIP_OK(G.done.make(hipEventDisableTiming));
        // queue slices: the primary kernel's workgroups are dealt to the shards round-robin, 256 paths each at most
        const uint64_t gpix = (uint64_t)(slot1 - slot0) * RT_TILE_PIXELS;
        const uint64_t primaryBlocks = (uint64_t)(slot1 - slot0) * 64 * sb;
        const uint64_t shardCap = ((primaryBlocks + RT_WF_SHARDS - 1) / RT_WF_SHARDS) * 256;
        const uint64_t cap = shardCap * RT_WF_SHARDS;
        if (cap > 0x7ffffff0ull) return fail("tile set too large for one batch");
        RtWavefront &Wf = G.wf;
        Wf.capacity = (uint32_t)cap;
        Wf.shardCap = (uint32_t)shardCap;
        Wf.lookAhead = T.lookAhead ? 1u : 0u;
        Wf.deadShadow = T.deadShadow ? 1u : 0u;
        const uint64_t qcap = 2 * cap; // queue entries: up to two rays in flight per path
        const uint64_t extraCap = (uint64_t)extraFactor * cap; // room for the further segments of cut rays (a wave that finds it full leaves its rays whole)
        const uint64_t ecap = qcap + extraCap;
        if (ecap > 0xfffffff0ull) return fail("tile set too large for one batch");
        Wf.extraCap = (uint32_t)extraCap;
        Wf.sampleBase = 0; Wf.samplesInBatch = (uint32_t)sb;
        if (sc->alloc<unsigned long long>(part, cap, &Wf.rng) || sc->alloc<uint4>(part, cap, &Wf.meta) || sc->alloc<float4>(part, cap, &Wf.outc) ||
            sc->alloc<float4>(part, cap * RT_RING * 3, &Wf.ring) || sc->alloc<float4>(part, cap, &Wf.shP) || sc->alloc<float4>(part, cap, &Wf.shFace) ||
            sc->alloc<float4>(part, cap, &Wf.shAtt) || sc->alloc<float4>(part, multiLight ? cap : 1, &Wf.shN) ||
            sc->alloc<unsigned long long>(part, multiLight ? cap : 1, &Wf.rngL) || sc->alloc<unsigned long long>(part, cap, &Wf.laKey) ||
            sc->alloc<uint4>(part, ecap * 4, &Wf.ent[0]) || sc->alloc<uint4>(part, ecap * 4, &Wf.ent[1]) || sc->alloc<uint2>(part, cap, &Wf.pathOf[0]) ||
            sc->alloc<uint2>(part, cap, &Wf.pathOf[1]) || sc->alloc<unsigned long long>(part, qcap, &Wf.hitKey[0]) || sc->alloc<unsigned long long>(part, qcap, &Wf.hitKey[1]) ||
            sc->alloc<uint4>(part, cap, &Wf.res) || sc->alloc<float4>(part, gpix * sb, &Wf.sampleOut) ||
            sc->alloc<uint32_t>(part, ecap, &Wf.sortRank) || sc->alloc<uint16_t>(part, ecap, &Wf.sortTag) || sc->alloc<uint32_t>(part, ecap, &Wf.sortedIdx) ||
            sc->alloc<uint32_t>(part, (uint64_t)3 * RT_WF_CTL_WORDS + (uint64_t)RT_WF_PLACE_ROUNDS * RT_WF_PLACE_WORDS, &Wf.ctl) || // (control words, then the placement tables)
            sc->alloc<uint4>(part, cap, &G.shade.list) || sc->alloc<uint32_t>(part, (uint64_t)3 * RT_WF_SHARDS, &G.shade.count)) // (split logic rounds: 16 bytes per path)
            return -1;
        HIP_OK(hipMemsetAsync(Wf.ctl, 0, sizeof(uint32_t) * (3 * RT_WF_CTL_WORDS + RT_WF_PLACE_ROUNDS * RT_WF_PLACE_WORDS), sc->stream));
        HIP_OK(hipMemsetAsync(G.shade.count, 0, sizeof(uint32_t) * 3 * RT_WF_SHARDS, sc->stream));
        HIP_OK(G.hostLog.make(sizeof(uint4) * RT_WF_ROUND_LOG, hipHostMallocMapped));
        memset(G.hostLog, 0, sizeof(uint4) * RT_WF_ROUND_LOG);
        HIP_OK(hipHostGetDevicePointer((void **)&Wf.roundLog, G.hostLog, 0));
        HIP_OK(G.hostCount.make(sizeof(uint32_t) * RT_WF_SHARDS, hipHostMallocDefault));
        HIP_OK(G.hostStatus.make(sizeof(uint32_t) * RT_WF_STATUS_WORDS, hipHostMallocMapped));
        memset(G.hostStatus, 0, sizeof(uint32_t) * RT_WF_STATUS_WORDS);
        HIP_OK(hipHostGetDevicePointer((void **)&Wf.hostStatus, G.hostStatus, 0));
        Wf.spinLimit = T.spinLimit ? T.spinLimit : 16384u;
        Wf.fastQuotient = T.fastQuotient ? 1u : 0u;
        // fixed grids: the kernels stride over the work that is really there (queues are sized for the worst case)
        G.queueBlocks = std::min<uint32_t>(cus * 16, (uint32_t)(qcap / 256)); // scatter: two generations of 8 resident workgroups per CU
        G.traceBlocks = (uint32_t)(ecap / 256); // trace of an ordered round, worst case: one workgroup per 256 entries; surplus groups exit at once
        // (a whole number of waves per queue slice: wf_logic_kernel keeps a wave in one slice)
        G.logicBlocks = std::min<uint32_t>(cus * 8, (uint32_t)((cap + 255) / 256));
        G.logicBlocks = std::max<uint32_t>(RT_WF_SHARDS / 4, (G.logicBlocks + RT_WF_SHARDS / 4 - 1) / (RT_WF_SHARDS / 4) * (RT_WF_SHARDS / 4));
    }
    HIP_OK(hipStreamSynchronize(sc->stream));
    sc->blocking = T.blocking != 0;
    sc->install(PART_WAVEFRONT, std::move(part));
    return 0;
}

// the groups' views of the scene (same scene, a contiguous range of this instance's tile slots): refreshed whenever a part
// was rebuilt
void refresh_views(rtHipScene *sc)
{
    const RtDevScene &D = sc->dev;
    for (auto &G : sc->groups) {
        G.dev = D;
        G.dev.tileIds = D.tileIds + G.slot0;
        G.dev.tileCount = G.slot1 - G.slot0;
        G.dev.camStart = D.camStart + (size_t)G.slot0 * RT_TILE_PIXELS;
        G.dev.camEnd = D.camEnd + (size_t)G.slot0 * RT_TILE_PIXELS;
        G.dev.tileBuf = D.tileBuf + (size_t)G.slot0 * 3 * RT_TILE_PIXELS;
    }
}

// One of the parts every instance of a scene holds alike (geometry, grid, materials, lights), copied from an instance that has it --
// device to device, over xGMI between GPUs -- instead of uploaded and reshaped once more: the "all GPUs" mode builds the scene once
// ("upload once via root then broadcast").  The source's work on the part must be complete (its builders synchronise).
int clone_part(rtHipScene *dst, const rtHipScene *src, int part)
{
    dst->drop_part(part);
    DevPart fresh;
    std::vector<std::pair<const char *, char *>> moved; // (source block, copy)
    std::vector<void *> blocks;
    std::vector<uint64_t> sizes;
    for (const DevBlock &b : src->parts[part].blocks) { blocks.push_back(b.p); sizes.push_back(b.size); }
    if (src->geo.live >= 0 && (part == PART_GEOMETRY || part == PART_GRID)) { // a source whose shape was updated holds it in a set of its own
        const rtHipScene::GeoMove::Set &L = src->geo.set[src->geo.live];
        const uint64_t T = src->dev.triangleCount ? src->dev.triangleCount : 1, n = src->gridListSize ? src->gridListSize : 1;
        if (part == PART_GEOMETRY) { blocks = { L.triRec, L.triShade }; sizes = { T * 64, T * RT_TRI_SHADE_WORDS * 4 }; }
        else {
            blocks = { L.boxMin, L.cellLut, L.gridStart, L.gridList, L.gridBits, L.sparse, L.pairRec };
            sizes = { GEO_PLANE_BYTES, GEO_LUT_BYTES, GEO_START_BYTES, n * 4, GEO_BITS_BYTES, GEO_SPARSE_BYTES, n * 64 };
        }
    }
    for (size_t i = 0; i < blocks.size(); ++i) {
        char *p = nullptr;
        const uint64_t n = sizes[i];
        if (dst->alloc<char>(fresh, n, &p)) return -1;
        HIP_OK(hipMemcpyPeerAsync(p, dst->device, blocks[i], src->device, n, dst->stream));
        moved.emplace_back((const char *)blocks[i], p);
    }
    auto at = [&](const void *old) -> const void * { // the copy of the block `old` points to (the builders hand out block starts only)
        for (auto &m : moved) if (m.first == (const char *)old) return m.second;
        return nullptr;
    };
    const RtDevScene &S = src->dev;
    RtDevScene &D = dst->dev;
#define RT_MOVE(field) D.field = (decltype(D.field))at(S.field)
    if (part == PART_GEOMETRY) { D.triangleCount = S.triangleCount; RT_MOVE(triRec); RT_MOVE(triShade); }
    if (part == PART_GRID) {
        D.planesTame = S.planesTame; D.cellCount = S.cellCount; dst->gridListSize = src->gridListSize;
        RT_MOVE(boxMin); RT_MOVE(cellLut); RT_MOVE(gridStart); RT_MOVE(gridList); RT_MOVE(gridBits); RT_MOVE(gridBlockSparse); RT_MOVE(pairRec);
        // the clip bound came with the planes; how many of its planes the kernels apply is this instance's own tuning
        dst->clipCount = src->clipCount;
        memcpy(dst->clipTail, src->clipTail, sizeof dst->clipTail);
        const uint32_t applied = dst->tune.rayClip ? dst->clipCount : 0u;
        memcpy(dst->clipTail, &applied, 4);
        HIP_OK(hipMemcpyAsync(const_cast<float *>(D.boxMin) + RT_CLIP_AT, dst->clipTail, 4, hipMemcpyHostToDevice, dst->stream));
    }
    if (part == PART_MATERIALS) {
        D.materialCount = S.materialCount; D.texelCount = S.texelCount; RT_MOVE(matSize); RT_MOVE(matStart); RT_MOVE(textures); RT_MOVE(matRec);
        dst->classMaterials = src->classMaterials;
        derive_path_class(dst);
    }
    if (part == PART_LIGHTS) {
        D.lightCount = S.lightCount;
        dst->classLights = src->classLights;
        derive_path_class(dst);
        RT_MOVE(lightType); RT_MOVE(lightPos); RT_MOVE(lightDir); RT_MOVE(lightCol); RT_MOVE(lightRadius); RT_MOVE(lightHalfAtt); RT_MOVE(lightSpread);
    }
#undef RT_MOVE
    HIP_OK(hipStreamSynchronize(dst->stream));
    dst->install(part, std::move(fresh));
    return 0;
}

// `like`: an instance of the same scene (same inputs) on this or another device whose shared parts are copied instead of built;
// `tune`: the caller's one snapshot of the tuning values, kept as sc->tune for the scene's later part rebuilds and frames
int scene_build(rtHipScene *sc, const rtHipSceneDesc *d, const cl_uint *tileIds, cl_uint tileCount, const rtHipScene *like, const Tuning &tune)
{
    if (!d) return fail("null scene description");
    if (d->width == 0 || d->height == 0) return fail("empty image %ux%u", d->width, d->height);
    if (d->sampleCount == 0) return fail("sampleCount must be >= 1");
    if (d->axesDiv != RT_GRID_DIV) return fail("axesDivCount %d unsupported (the reference builds %d, trianglelist.h:110)", d->axesDiv, RT_GRID_DIV);
    if ((uint64_t)d->width * d->height > 0xffffffffull) return fail("image too large");
    HIP_OK(hipSetDevice(sc->device));
    HIP_OK(sc->stream.make(hipStreamNonBlocking));
    sc->tune = tune;
    sc->pipeline = tune.pipeline == RT_HIP_PIPELINE_MEGAKERNEL ? RT_HIP_PIPELINE_MEGAKERNEL : RT_HIP_PIPELINE_WAVEFRONT;
    if (sc->stager.init(sc->stream, tune) != 0) return -1;
    // Tuning::timing: where the time of a scene upload goes (stderr)
    const bool timing = tune.timing != 0;
    auto tLast = std::chrono::steady_clock::now();
    auto mark = [&](const char *what) {
        if (!timing) return;
        (void)hipStreamSynchronize(sc->stream);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "libraytrace_hip: scene build: %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - tLast).count());
        tLast = now;
    };
    // arrays that are already on the device: the few tables the host looks at itself come back to it, the rest is copied HBM to HBM
    rtHipSceneDesc shadowed;
    std::vector<char> hostCopies[10];
    cl_uint gridEnd[1] = { 0 };
    if (d->arraysOnDevice) {
        shadowed = *d;
        auto fetch = [&](int slot, const void *&field, size_t bytes) -> int {
            if (!field || !bytes) return 0;
            hostCopies[slot].resize(bytes);
            HIP_OK(hipMemcpy(hostCopies[slot].data(), field, bytes, hipMemcpyDeviceToHost));
            field = hostCopies[slot].data();
            return 0;
        };
        const uint64_t cells = (uint64_t)RT_GRID_DIV * RT_GRID_DIV * RT_GRID_DIV;
        if (d->gridStart) { HIP_OK(hipMemcpy(gridEnd, d->gridStart + cells, 4, hipMemcpyDeviceToHost)); sc->gridListSizeHint = gridEnd[0]; sc->haveGridListSize = true; }
        if (fetch(0, (const void *&)shadowed.boxMin, (size_t)(RT_GRID_DIV + 1) * 16) || fetch(1, (const void *&)shadowed.matSize, (size_t)d->materialCount * 40) ||
            fetch(2, (const void *&)shadowed.matStart, (size_t)d->materialCount * 20) || fetch(3, (const void *&)shadowed.textures, (size_t)d->texturesSize * 4) ||
            fetch(4, (const void *&)shadowed.lightType, (size_t)d->lightCount * 4) || fetch(5, (const void *&)shadowed.lightPos, (size_t)d->lightCount * 16) ||
            fetch(6, (const void *&)shadowed.lightDir, (size_t)d->lightCount * 16) || fetch(7, (const void *&)shadowed.lightCol, (size_t)d->lightCount * 16) ||
            fetch(8, (const void *&)shadowed.lightRadius, (size_t)d->lightCount * 4) || fetch(9, (const void *&)shadowed.lightHalfAtt, (size_t)d->lightCount * 4))
            return -1;
        d = &shadowed;
    }
    if (build_fixed(sc, d, tileIds, tileCount) != 0) return -1;
    mark("tiles, outputs, bump tables");
    if (like) {
        for (int part : { PART_GEOMETRY, PART_GRID, PART_MATERIALS, PART_LIGHTS })
            if (clone_part(sc, like, part) != 0) return -1;
        mark("geometry, grid, materials, lights (copied from another instance)");
        if (build_camera(sc, d) != 0) return -1;
        mark("camera lists");
    } else {
        if (build_geometry(sc, d) != 0) return -1;
        mark("geometry");
        if (build_grid(sc, d) != 0) return -1;
        mark("grid + dense view");
        if (build_camera(sc, d) != 0) return -1;
        mark("camera lists");
        if (build_materials(sc, d) != 0) return -1;
        if (build_lights(sc, d) != 0) return -1;
        mark("materials + lights");
    }
    // what only a kernel can tell about the inputs (ids inside the lists): one look at the error word
    HIP_OK(rtp_validate(sc->dev.triangleCount, 0, 0, nullptr, nullptr, sc->camListSize, sc->dev.camList, nullptr, 0, nullptr, sc->prepErr, sc->stream));
    HIP_OK(hipStreamSynchronize(sc->stream));
    HIP_OK(sc->stager.drain()); // (the stream is idle: the staging buffers go back to the pool)
    if (sc->check_prep() != 0) return -1;
    if (build_wavefront(sc, d->sampleCount) != 0) return -1;
    refresh_views(sc);
    mark("path state buffers");
    return 0;
}

} // namespace rthost
