// fileio_host.cpp -- the file readers (opencl_render_amd/csrc/rt_fileio.cpp) in a program of its own, so that they can run under the
// address and undefined-behaviour sanitizers without a sanitizer inside Python.  Compiled together with rt_fileio.cpp and rt_frontend.cpp.
// usage: fileio_host DIR; reads every *.obj (rtHipObjRead) and *.ppm / *.bmp (rtHipImageRead) of DIR in the order of their names and
// prints one line per file, fields separated by tabs:
//   obj  rc points polygons materials  fnv(points) fnv(polygons) fnv(normals) fnv(uv) fnv(polygonMaterial) fnv(materials)  name
//   img  rc width height  fnv(texels)  name
// with the 64-bit FNV-1a hash of each returned array's bytes in hexadecimal and "-" for an array that is NULL.  It checks for itself
// that a refused file leaves the outputs zeroed, that an accepted OBJ has every index in range and that rtHipMeshCount / rtHipMeshFill
// return 0 on it; a failed check goes to stderr and makes the exit status 1.
#include "raytrace_hip.h"

#include <dirent.h>

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static std::string fnv(const void *data, size_t bytes)
{
    if (!data) return "-";
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char *p = (const unsigned char *)data;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    char text[24];
    snprintf(text, sizeof text, "%016" PRIx64, h);
    return text;
}

static bool ends_with(const std::string &s, const char *tail)
{
    const size_t n = strlen(tail);
    return s.size() >= n && s.compare(s.size() - n, n, tail) == 0;
}

static void read_obj(const std::string &path, const char *name)
{
    rtHipObjData d;
    memset(&d, 0x5a, sizeof d); // (the reader must not rely on what it is handed)
    const int rc = rtHipObjRead(path.c_str(), &d);
    if (rc != 0) {
        rtHipObjData zero;
        memset(&zero, 0, sizeof zero);
        EXPECT(d.pointCount == 0 && d.polygonCount == 0 && d.materialCount == 0 && !d.points && !d.polygons && !d.cornerNormals && !d.cornerUv &&
               !d.polygonMaterial && !d.materials, "%s: rc %d but *out is not zeroed", name, rc);
        printf("obj\t%d\t0\t0\t0\t-\t-\t-\t-\t-\t-\t%s\n", rc, name);
        return;
    }
    const size_t P = d.pointCount, N = d.polygonCount, M = d.materialCount;
    EXPECT(d.points && d.polygons && d.polygonMaterial && d.materials, "%s: accepted with a NULL array", name);
    for (size_t i = 0; i < 4 * N; ++i) EXPECT(d.polygons[i] >= 0 && (size_t)d.polygons[i] < P, "%s: index %d of %zu points", name, d.polygons[i], P);
    for (size_t i = 0; i < N; ++i) EXPECT(d.polygonMaterial[i] >= -1 && d.polygonMaterial[i] < (cl_int)M, "%s: material %d of %zu", name, d.polygonMaterial[i], M);
    for (size_t i = 0; i < M; ++i) {
        EXPECT(memchr(d.materials[i].name, 0, sizeof d.materials[i].name), "%s: material name without terminator", name);
        for (int c = 0; c < 5; ++c) EXPECT(memchr(d.materials[i].map[c], 0, sizeof d.materials[i].map[c]), "%s: map path without terminator", name);
    }
    // what the front-end does next with it
    rtHipMesh mesh = { d.pointCount, d.points, d.polygonCount, d.polygons, d.cornerNormals, d.cornerUv, d.polygonMaterial };
    cl_uint V = 0, T = 0;
    const int counted = rtHipMeshCount(&mesh, 1, &V, &T);
    EXPECT(counted == 0 && V == d.pointCount && T >= N && T <= 2 * N, "%s: rtHipMeshCount %d, %u vertices, %u triangles", name, counted, V, T);
    if (counted == 0) {
        std::vector<cl_float3> vertex(V ? V : 1), normal(3 * (size_t)T + 1);
        std::vector<cl_int3> index(T ? T : 1);
        std::vector<cl_int> material(T ? T : 1);
        std::vector<cl_float2> uv(3 * (size_t)T + 1);
        const cl_float eye[3] = { 0.25f, 0.5f, -3.f };
        const int filled = rtHipMeshFill(&mesh, 1, eye, vertex.data(), index.data(), material.data(), uv.data(), normal.data());
        EXPECT(filled == 0, "%s: rtHipMeshFill %d", name, filled);
    }
    printf("obj\t0\t%zu\t%zu\t%zu\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", P, N, M, fnv(d.points, 16 * P).c_str(), fnv(d.polygons, 16 * N).c_str(),
           fnv(d.cornerNormals, 64 * N).c_str(), fnv(d.cornerUv, 32 * N).c_str(), fnv(d.polygonMaterial, 4 * N).c_str(),
           fnv(d.materials, sizeof(rtHipObjMaterial) * M).c_str(), name);
    rtHipObjFree(&d);
    EXPECT(!d.points && !d.materials && d.pointCount == 0, "%s: rtHipObjFree left something behind", name);
}

static void read_image(const std::string &path, const char *name)
{
    cl_uint w = 0x5a5a5a5au, h = 0x5a5a5a5au;
    cl_uchar3 *px = (cl_uchar3 *)&w; // (any non-NULL value)
    const int rc = rtHipImageRead(path.c_str(), &w, &h, &px);
    if (rc != 0) {
        EXPECT(!px && w == 0 && h == 0, "%s: rc %d but the outputs are not zeroed", name, rc);
        printf("img\t%d\t0\t0\t-\t%s\n", rc, name);
        return;
    }
    EXPECT(px && w >= 1 && h >= 1, "%s: accepted as %u x %u", name, w, h);
    const cl_uchar *bytes = (const cl_uchar *)px;
    for (size_t i = 0; i < (size_t)w * h; ++i) EXPECT(bytes[4 * i + 3] == 0, "%s: texel %zu has a fourth byte", name, i);
    printf("img\t0\t%u\t%u\t%s\t%s\n", w, h, fnv(px, 4 * (size_t)w * h).c_str(), name);
    free(px); // (rtHipFree is free(); it lives with the builders, which this program does not link)
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: fileio_host DIR\n"); return 2; }
    DIR *dir = opendir(argv[1]);
    if (!dir) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<std::string> names;
    while (const dirent *e = readdir(dir)) names.push_back(e->d_name);
    closedir(dir);
    std::sort(names.begin(), names.end());
    for (const std::string &n : names) {
        const std::string path = std::string(argv[1]) + "/" + n;
        if (ends_with(n, ".obj")) read_obj(path, n.c_str());
        else if (ends_with(n, ".ppm") || ends_with(n, ".bmp")) read_image(path, n.c_str());
    }
    if (failures) fprintf(stderr, "failures %d\n", failures);
    return failures ? 1 : 0;
}
