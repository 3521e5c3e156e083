// rt_kat.hip -- TEST-ONLY entry point: runs the device-side building blocks of rt_devfuncs.h over caller-provided vectors,
// one item per thread, so the function-level known answers minted from the reference kernel (tests/golden/kat.npz) are
// checked on the GPU itself and not only against the CPU oracle.  Nothing here is on the render path.
//
//   op                in (per item)                                   out (per item)
//   RT_KAT_RANDF      u64 seed                                        16 x f32 draws (alternating randF(0,1), randF(-1,1)), 16 x u64 states   (:12-23)
//   RT_KAT_SPHERE     u64 seed, f32 radius, pad                       f32 x,y,z, pad, u64 state                                               (:30-45)
//   RT_KAT_PMODF      f32                                             f32                                                                     (:25-28)
//   RT_KAT_TRI        o3 d3 a3 b3 c3 tmin tmax (17 x f32)             hit (0/1), t, abL, acL (abL/acL 0 when the reference does not write them) (:124-172)
//   RT_KAT_PLINE      origin3 destination3 point3                     f32                                                                     (:83-101)
//   RT_KAT_BOX        p3 (table = split planes, 3 x 257 f32 SoA)      i32 cx, cy, cz                                                          (:174-193)
//   RT_KAT_BIND       p3 d3 lo3 hi3                                   p3 after the clamps                                                     (:265-322)
//   RT_KAT_POW        f32 x                                           (float)pow(0.5f, x), NaN -> 1                                           (:631-632)
//   RT_KAT_QUOTIENT   f32 plane, o, d                                 f32 (plane-o)/d as the compiler divides, f32 the walk's short sequence, u32 tame (:383-385)
//   RT_KAT_SPHERE_SPLIT  u64 seed, f32 radius, pad                    as RT_KAT_SPHERE, through sphere_raw + sphere_scaled (the wavefront kernels' form)
//   RT_KAT_ACCUM      i32 plane, f32 colour, f32 scale                i32 sat_add_u16(plane, colour, scale), i32 trunc_x86(colour * scale)  (:726-741)
//
// rtHipTestShadeKat runs the shading building blocks on a RESIDENT scene (its RtDevScene: triRec, triShade, matRec, matSize,
// matStart, the atlas and the bump tables exactly as the upload built them), with the Shared set-up of the kernels:
//   op                      in (per item, 40 / 48 bytes)                    out (per item, 64 / 96 bytes)
//   RT_SHADE_KAT_TEXEL      i32 material, i32 channel, uv[6], l1, l2        {x,y,z,raw} of texel_rec (zero when the descriptor is 0), of
//                           (Get2dTableValue3, :103-122)                   texel<false> and of texel<true> on matStart/matSize, then the
//                                                                           descriptor word and the texel count of the counted variant
//   RT_SHADE_KAT_NORMAL     u32 triangle, where3, ray o3, ray d3, l1, l2    {x,y,z,ran} of shading_normal<false> with the MatRec,
//                           (GetTriangleNormal, :195-263)                  <true> without one (the megakernel's) and <false, true> (the
//                                                                           opaque-diffuse class form; ran = 0 where the material's height
//                                                                           map is an image), each without and with firstVertex
#include "rt_devfuncs.h"
#include "rt_launch.h"
#include "raytrace_hip.h"

#include <hip/hip_runtime_api.h>

#include <vector>

namespace {

__global__ __launch_bounds__(256) void rt_kat_kernel(int op, uint32_t count, const unsigned char *__restrict__ in, uint32_t inStride,
                                                     unsigned char *__restrict__ out, uint32_t outStride, const float *__restrict__ table)
{
    __shared__ Shared sh;
    if (op == RT_KAT_BOX) {
        for (int i = threadIdx.x; i < 3 * (RT_GRID_DIV + 1); i += 256) (&sh.planes[0][0])[i] = table[i];
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float *fi = reinterpret_cast<const float *>(in + (size_t)i * inStride);
    float *fo = reinterpret_cast<float *>(out + (size_t)i * outStride);
    switch (op) {
    case RT_KAT_RANDF: {
        uint64_t s = *reinterpret_cast<const uint64_t *>(fi);
        uint64_t *states = reinterpret_cast<uint64_t *>(fo + 16);
        for (int j = 0; j < 16; ++j) {
            fo[j] = (j & 1) ? rand11(s) : rand01(s);
            states[j] = s;
        }
        break;
    }
    case RT_KAT_SPHERE: {
        uint64_t s = *reinterpret_cast<const uint64_t *>(fi);
        const V3 p = sphere_point(s, fi[2]);
        fo[0] = p.x; fo[1] = p.y; fo[2] = p.z; fo[3] = 0.f;
        *reinterpret_cast<uint64_t *>(fo + 4) = s;
        break;
    }
    case RT_KAT_PMODF:
        fo[0] = pos_modf(fi[0]);
        break;
    case RT_KAT_TRI: {
        // the record rt_prepare_triangles builds (same operations), then the test the kernels run on it
        const V3 o = ld3(fi), d = ld3(fi + 3), a = ld3(fi + 6), b = ld3(fi + 9), c = ld3(fi + 12);
        const V3 ab = sub3(b, a), ac = sub3(c, a);
        const V3 n = cross3(ac, ab);
        const float abab = dot3(ab, ab), abac = dot3(ab, ac), acac = dot3(ac, ac);
        const float inv = 1.f / (abac * abac - abab * acac);
        __attribute__((aligned(16))) float rec[16] = { a.x, a.y, a.z, ab.x, ab.y, ab.z, ac.x, ac.y, ac.z, n.x, n.y, n.z, abab, abac, acac, inv };
        float t = 0.f, l1 = 0.f, l2 = 0.f;
        const bool hit = tri_test(rec, 0u, o, d, fi[15], fi[16], t, l1, l2);
        fo[0] = hit ? 1.f : 0.f; fo[1] = t; fo[2] = l1; fo[3] = l2;
        // the branch-free variant the wavefront kernels use must agree wherever the reference computes the second half
        float t2, m1, m2;
        const float4 r0 = make_float4(rec[0], rec[1], rec[2], rec[3]), r1 = make_float4(rec[4], rec[5], rec[6], rec[7]);
        const float4 r2 = make_float4(rec[8], rec[9], rec[10], rec[11]), r3 = make_float4(rec[12], rec[13], rec[14], rec[15]);
        const V3 fa = mk(r0.x, r0.y, r0.z), fab = mk(r0.w, r1.x, r1.y), fac = mk(r1.z, r1.w, r2.x), fn = mk(r2.y, r2.z, r2.w);
        t2 = -dot3(fn, sub3(o, fa)) / dot3(fn, d);
        const V3 ap = sub3(along(o, t2, d), fa);
        const float ap_ab = dot3(ap, fab), ap_ac = dot3(ap, fac);
        m1 = (r3.y * ap_ac - r3.z * ap_ab) * r3.w;
        m2 = (r3.y * ap_ab - r3.x * ap_ac) * r3.w;
        const bool hit2 = (fi[15] < t2) & (t2 < fi[16]) & (0 <= m1) & (0 <= m2) & (m1 + m2 <= 1.f);
        const bool inRange = fi[15] < t && t < fi[16];
        const bool same = hit2 == hit && __float_as_uint(t2) == __float_as_uint(t) &&
                          (!inRange || (__float_as_uint(m1) == __float_as_uint(l1) && __float_as_uint(m2) == __float_as_uint(l2)));
        fo[4] = same ? 1.f : 0.f;
        break;
    }
    case RT_KAT_PLINE:
        fo[0] = point_line_sq(ld3(fi), ld3(fi + 3), ld3(fi + 6));
        break;
    case RT_KAT_BOX: {
        int cx, cy, cz;
        box_address(sh, ld3(fi), cx, cy, cz);
        int *io = reinterpret_cast<int *>(fo);
        io[0] = cx; io[1] = cy; io[2] = cz;
        break;
    }
    case RT_KAT_BIND: {
        V3 p = ld3(fi);
        bind_in_cube(p, ld3(fi + 3), ld3(fi + 6), ld3(fi + 9));
        fo[0] = p.x; fo[1] = p.y; fo[2] = p.z;
        break;
    }
    case RT_KAT_POW:
        fo[0] = half_falloff(fi[0]);
        break;
    case RT_KAT_QUOTIENT: { // both ways of wf_trace_kernel's walk; they must agree (up to the sign of zero) whenever `tame` says so
        const float plane = fi[0], o = fi[1], d = fi[2];
        fo[0] = (plane - o) / d;
        fo[1] = tame_quotient(plane - o, d, refined_rcp(d));
        reinterpret_cast<uint32_t *>(fo)[2] = (tame_origin(plane) && tame_origin(o) && tame_direction(d)) ? 1u : 0u;
        break;
    }
    case RT_KAT_SPHERE_SPLIT: {
        uint64_t s = *reinterpret_cast<const uint64_t *>(fi);
        const V3 p = sphere_scaled(sphere_raw(s), fi[2]);
        fo[0] = p.x; fo[1] = p.y; fo[2] = p.z; fo[3] = 0.f;
        *reinterpret_cast<uint64_t *>(fo + 4) = s;
        break;
    }
    case RT_KAT_ACCUM: {
        const int *ii = reinterpret_cast<const int *>(fi);
        int *io = reinterpret_cast<int *>(fo);
        io[0] = sat_add_u16(ii[0], fi[1], fi[2]);
        io[1] = trunc_x86(fi[1] * fi[2]);
        break;
    }
    default:
        break;
    }
}

__device__ __forceinline__ void put4(float *o, V3 v, uint32_t w)
{
    o[0] = v.x; o[1] = v.y; o[2] = v.z; reinterpret_cast<uint32_t *>(o)[3] = w;
}

__global__ __launch_bounds__(256) void rt_shade_kat_kernel(const RtDevScene S, int op, uint32_t count, const unsigned char *__restrict__ in,
                                                           unsigned char *__restrict__ out)
{
    __shared__ Shared sh; // as every kernel that shades sets it up
    for (int i = threadIdx.x; i < 3 * (RT_GRID_DIV + 1); i += 256) (&sh.planes[0][0])[i] = S.boxMin[i];
    sh.unit255[threadIdx.x] = (float)threadIdx.x / 255.f;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    if (op == RT_SHADE_KAT_TEXEL) {
        const int *ii = reinterpret_cast<const int *>(in + (size_t)i * 40);
        const float *fi = reinterpret_cast<const float *>(ii);
        float *fo = reinterpret_cast<float *>(out + (size_t)i * 64);
        const int m = ii[0], ch = ii[1];
        const float *uv = fi + 2;
        const float l1 = fi[8], l2 = fi[9];
        const MatRec M = load_mat(S, m);
        const int at = CH_COUNT * m + ch;
        Counters cn;
        for (int k = 0; k < ST_COUNT; ++k) cn.v[k] = 0;
        uint32_t raw = 0u;
        V3 v = mk(0.f, 0.f, 0.f);
        if (M.desc[ch]) v = texel_rec<false>(S, sh, M, ch, uv, l1, l2, raw, cn);
        put4(fo, v, raw);
        raw = 0u;
        v = texel<false>(S, sh, S.matStart[at], S.matSize[2 * at], S.matSize[2 * at + 1], uv, l1, l2, raw, cn);
        put4(fo + 4, v, raw);
        raw = 0u;
        v = texel<true>(S, sh, S.matStart[at], S.matSize[2 * at], S.matSize[2 * at + 1], uv, l1, l2, raw, cn);
        put4(fo + 8, v, raw);
        reinterpret_cast<uint32_t *>(fo)[12] = M.desc[ch];
        reinterpret_cast<uint32_t *>(fo)[13] = cn.v[ST_TEXELS];
        return;
    }
    // RT_SHADE_KAT_NORMAL
    const float *fi = reinterpret_cast<const float *>(in + (size_t)i * 48);
    float *fo = reinterpret_cast<float *>(out + (size_t)i * 96);
    const uint32_t tri = reinterpret_cast<const uint32_t *>(fi)[0];
    const V3 where = ld3(fi + 1), o = ld3(fi + 4), d = ld3(fi + 7);
    const float l1 = fi[10], l2 = fi[11];
    const float *shade = S.triShade + RT_TRI_SHADE_WORDS * (size_t)tri;
    const int m = __float_as_int(shade[21]);
    const float4 first = reinterpret_cast<const float4 *>(S.triRec)[4 * (size_t)tri]; // the round-0 row's copy (rt_wavefront.hip, TriRow)
    MatRec mat;
    mat.desc[0] = mat.desc[1] = mat.desc[2] = mat.desc[3] = mat.desc[4] = 0u; mat.m = m;
    if (0 <= m) mat = load_mat(S, m);
    Counters cn;
    for (int k = 0; k < ST_COUNT; ++k) cn.v[k] = 0;
    put4(fo + 0, shading_normal<false>(S, sh, where, o, d, tri, l1, l2, shade, m, cn, &mat), 1u);
    put4(fo + 4, shading_normal<false>(S, sh, where, o, d, tri, l1, l2, shade, m, cn, &mat, &first), 1u);
    put4(fo + 8, shading_normal<true>(S, sh, where, o, d, tri, l1, l2, shade, m, cn), 1u);
    put4(fo + 12, shading_normal<true>(S, sh, where, o, d, tri, l1, l2, shade, m, cn, nullptr, &first), 1u);
    const uint32_t bump = mat.desc[CH_BUMP];
    if (m < 0 || bump == 0u || (bump & 0x80000000u)) { // what the class kernel admits: no height map, or one of one texel
        put4(fo + 16, shading_normal<false, true>(S, sh, where, o, d, tri, l1, l2, shade, m, cn, &mat), 1u);
        put4(fo + 20, shading_normal<false, true>(S, sh, where, o, d, tri, l1, l2, shade, m, cn, &mat, &first), 1u);
    } else {
        put4(fo + 16, mk(0.f, 0.f, 0.f), 0u);
        put4(fo + 20, mk(0.f, 0.f, 0.f), 0u);
    }
}

} // namespace

// rtHipTestShadeKat's device part (rt_api.cpp holds the scene): synchronous, on the current device.  0, -1 bad op, -3 HIP failure.
extern "C" __attribute__((visibility("hidden"))) int rt_shade_kat_run(const RtDevScene *scene, int op, uint32_t count, const void *in, void *out)
{
    const RtDevScene &S = *scene;
    if (op != RT_SHADE_KAT_TEXEL && op != RT_SHADE_KAT_NORMAL) return -1;
    if (count == 0) return 0;
    const size_t inStride = op == RT_SHADE_KAT_TEXEL ? 40 : 48, outStride = op == RT_SHADE_KAT_TEXEL ? 64 : 96;
    unsigned char *dIn = nullptr, *dOut = nullptr;
    int rc = -3;
    do {
        if (hipMalloc((void **)&dIn, count * inStride) != hipSuccess) break;
        if (hipMalloc((void **)&dOut, count * outStride) != hipSuccess) break;
        if (hipMemcpy(dIn, in, count * inStride, hipMemcpyHostToDevice) != hipSuccess) break;
        if (hipMemset(dOut, 0, count * outStride) != hipSuccess) break;
        hipLaunchKernelGGL(rt_shade_kat_kernel, dim3((count + 255) / 256), dim3(256), 0, 0, S, op, count, dIn, dOut);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) break;
        if (hipMemcpy(out, dOut, count * outStride, hipMemcpyDeviceToHost) != hipSuccess) break;
        rc = 0;
    } while (0);
    (void)hipFree(dIn); (void)hipFree(dOut);
    return rc;
}

extern "C" int rtHipDeviceKat(int device, int op, cl_uint count, const void *in, cl_uint inStride, void *out, cl_uint outStride, const float *table)
{
    static const uint32_t inNeed[RT_KAT_OPS] = { 8, 16, 4, 68, 36, 12, 48, 4, 12, 16, 12 }, outNeed[RT_KAT_OPS] = { 192, 24, 4, 20, 4, 12, 12, 4, 12, 24, 8 };
    if (op < 0 || op >= RT_KAT_OPS || !in || !out || inStride < inNeed[op] || outStride < outNeed[op] || (inStride & 3u) || (outStride & 3u)) return -1;
    if (op == RT_KAT_BOX && !table) return -1;
    if (count == 0) return 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return -2; // no device: no CPU stand-in
    if (hipSetDevice(device) != hipSuccess) return -2;
    unsigned char *dIn = nullptr, *dOut = nullptr;
    float *dTable = nullptr;
    int rc = -3;
    do {
        if (hipMalloc((void **)&dIn, (size_t)count * inStride) != hipSuccess) break;
        if (hipMalloc((void **)&dOut, (size_t)count * outStride) != hipSuccess) break;
        if (hipMemcpy(dIn, in, (size_t)count * inStride, hipMemcpyHostToDevice) != hipSuccess) break;
        if (hipMemset(dOut, 0, (size_t)count * outStride) != hipSuccess) break;
        if (table) {
            if (hipMalloc((void **)&dTable, sizeof(float) * 3 * (RT_GRID_DIV + 1)) != hipSuccess) break;
            if (hipMemcpy(dTable, table, sizeof(float) * 3 * (RT_GRID_DIV + 1), hipMemcpyHostToDevice) != hipSuccess) break;
        }
        hipLaunchKernelGGL(rt_kat_kernel, dim3((count + 255) / 256), dim3(256), 0, 0, op, count, dIn, inStride, dOut, outStride, dTable);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) break;
        if (hipMemcpy(out, dOut, (size_t)count * outStride, hipMemcpyDeviceToHost) != hipSuccess) break;
        rc = 0;
    } while (0);
    (void)hipFree(dIn); (void)hipFree(dOut); (void)hipFree(dTable);
    return rc;
}
