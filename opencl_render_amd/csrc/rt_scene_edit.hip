// rt_scene_edit.hip -- the device side of a material id edit of a RESIDENT scene (rtHipSceneSetMaterials).
//
// Lights, material tables and the atlas are tables the host fills and the frame kernels read: replacing them needs no kernel.  The
// material ID of a triangle lives in one place only, word 21 of its triShade row (RT_TRI_SHADE_WORDS floats, rt_device.h; rt_prepare_triangles,
// rt_kernels.hip), beside corner and UV words an edit must not touch.  Two kernels, one thread per triangle:
//   rte_check_ids   reads the ids that will be in effect -- an array of T ids (coalesced), or word 21 of the resident rows when the
//                   tables shrink under ids that stay -- and raises RT_PREP_ERR_TRI_MATERIAL in the scene's validation word for an
//                   id >= M: one ballot per wave, at most one atomic per wave.  Negative ids are legal ("no material").
//   rte_store_ids   launched only after the host has read a clean validation word: word 21 of every row of the set in use, one 4-byte
//                   store per row; the row's other words are neither read nor written.
#include <hip/hip_runtime.h>

#include "rt_device.h"
#include "rt_launch.h"

namespace {

constexpr uint32_t ROW_WORDS = RT_TRI_SHADE_WORDS, ID_WORD = 21;

__global__ __launch_bounds__(256) void rte_check_ids(uint32_t T, uint32_t M, const int *__restrict__ ids, const int *__restrict__ rows, uint32_t *err)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (t < T) { // (no early return: the whole wave meets at the ballot, its tail lanes vote "fine")
        const int id = ids ? ids[t] : rows[(size_t)ROW_WORDS * t + ID_WORD];
        bad = id >= 0 && (uint32_t)id >= M;
    }
    const unsigned long long any = __ballot(bad);
    if (any && (threadIdx.x & 63u) == 0u) atomicOr(err, (uint32_t)RT_PREP_ERR_TRI_MATERIAL);
}

__global__ __launch_bounds__(256) void rte_store_ids(uint32_t T, const int *__restrict__ ids, int *__restrict__ rows)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t < T) rows[(size_t)ROW_WORDS * t + ID_WORD] = ids[t];
}

} // namespace

extern "C" hipError_t rte_launch_check_ids(uint32_t T, uint32_t M, const int *ids, const float *triShade, uint32_t *err, hipStream_t stream)
{
    if (T == 0) return hipSuccess;
    hipLaunchKernelGGL(rte_check_ids, dim3((T + 255) / 256), dim3(256), 0, stream, T, M, ids, reinterpret_cast<const int *>(triShade), err);
    return hipGetLastError();
}

extern "C" hipError_t rte_launch_store_ids(uint32_t T, const int *ids, float *triShade, hipStream_t stream)
{
    if (T == 0) return hipSuccess;
    hipLaunchKernelGGL(rte_store_ids, dim3((T + 255) / 256), dim3(256), 0, stream, T, ids, reinterpret_cast<int *>(triShade));
    return hipGetLastError();
}
