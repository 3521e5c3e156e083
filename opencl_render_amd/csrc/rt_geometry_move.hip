// rt_geometry_move.hip -- the device side of a geometry update of a RESIDENT scene that is new (rtHipSceneSetGeometry).
//
// An update chains kernels that exist: rtp_validate (rt_scene_prep.hip), the grid build's core (rt_build_device.hip), rtp_dense_grid,
// rt_gather_pair_records (rt_kernels.hip) and the resident camera build (rt_camera_move.hip).  The one thing none of them does is
// make a triangle's records when the scene no longer holds the ABI arrays they were made from:
//   rtg_records   one thread per triangle: triRec and the corner words of triShade from the new vertices -- the operations of
//                 rt_prepare_triangles (rt_kernels.hip) in its order, compiled with the same flags, so every word equals what a scene
//                 created from the new arrays holds -- and the words an update does not touch (UVs, material id, and the corner normals
//                 unless new ones are given) copied from the row the scene renders from.  It writes rows of the SPARE set only.
#include <hip/hip_runtime.h>

#include "rt_devfuncs.h"
#include "rt_geometry_move.h"

namespace {

template <bool NORMALS>
__global__ __launch_bounds__(256) void rtg_records(uint32_t triangleCount, const float4 *__restrict__ vertex, const int4 *__restrict__ triIndex,
                                                   const float4 *__restrict__ triNormal, const float *__restrict__ oldShade,
                                                   float *__restrict__ triRec, float *__restrict__ triShade)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= triangleCount) return;
    const int4 vi = triIndex[t]; // checked by rtp_validate before this launch
    const float4 fa = vertex[vi.x], fb = vertex[vi.y], fc = vertex[vi.z];
    const V3 a = mk(fa.x, fa.y, fa.z), b = mk(fb.x, fb.y, fb.z), c = mk(fc.x, fc.y, fc.z);
    const V3 ab = sub3(b, a), ac = sub3(c, a);
    const V3 n = cross3(ac, ab);
    const float abab = dot3(ab, ab), abac = dot3(ab, ac), acac = dot3(ac, ac);
    const float inv = 1.f / (abac * abac - abab * acac);
    float4 *rec = reinterpret_cast<float4 *>(triRec) + 4 * (size_t)t;
    rec[0] = make_float4(a.x, a.y, a.z, ab.x);
    rec[1] = make_float4(ab.y, ab.z, ac.x, ac.y);
    rec[2] = make_float4(ac.z, n.x, n.y, n.z);
    rec[3] = make_float4(abab, abac, acac, inv);
    // a row is one 128-byte line (rt_device.h): twelve float2 of packed words, then the copy of the record's quad 0 and a zero quad
    float2 *sh = reinterpret_cast<float2 *>(triShade + RT_TRI_SHADE_WORDS * (size_t)t);
    const float2 *old = reinterpret_cast<const float2 *>(oldShade + RT_TRI_SHADE_WORDS * (size_t)t);
    reinterpret_cast<float4 *>(sh)[6] = make_float4(a.x, a.y, a.z, ab.x);
    reinterpret_cast<float4 *>(sh)[7] = make_float4(0.f, 0.f, 0.f, 0.f);
    sh[0] = make_float2(b.x, b.y); sh[1] = make_float2(b.z, c.x); sh[2] = make_float2(c.y, c.z);
    if (NORMALS) {
        const float4 na = triNormal[3 * (size_t)t], nb = triNormal[3 * (size_t)t + 1], nc = triNormal[3 * (size_t)t + 2];
        sh[3] = make_float2(na.x, na.y); sh[4] = make_float2(na.z, nb.x); sh[5] = make_float2(nb.y, nb.z); sh[6] = make_float2(nc.x, nc.y);
        sh[7] = make_float2(nc.z, old[7].y); // word 15 is the first UV word
    } else {
#pragma unroll
        for (int i = 3; i < 8; ++i) sh[i] = old[i];
    }
#pragma unroll
    for (int i = 8; i < 12; ++i) sh[i] = old[i]; // UVs, material id, the two zero words
}

} // namespace

extern "C" hipError_t rtg_launch_records(uint32_t T, const void *vertex, const void *triIndex, const void *triNormal, const float *oldShade,
                                         float *triRec, float *triShade, hipStream_t stream)
{
    if (T == 0) return hipSuccess;
    if (triNormal)
        hipLaunchKernelGGL(rtg_records<true>, dim3((T + 255) / 256), dim3(256), 0, stream, T, (const float4 *)vertex, (const int4 *)triIndex,
                           (const float4 *)triNormal, oldShade, triRec, triShade);
    else
        hipLaunchKernelGGL(rtg_records<false>, dim3((T + 255) / 256), dim3(256), 0, stream, T, (const float4 *)vertex, (const int4 *)triIndex,
                           (const float4 *)nullptr, oldShade, triRec, triShade);
    return hipGetLastError();
}
