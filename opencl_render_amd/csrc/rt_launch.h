// rt_launch.h -- every host-callable function a .hip file defines, declared ONCE: the .hip that defines one and every .cpp that calls one
// include this header, so a launcher whose parameters change on one side only no longer compiles (with C linkage the linker would not
// notice).  rtg_launch_records and the grid build's core are declared in rt_geometry_move.h, which both of their sides include.
#ifndef RT_LAUNCH_H
#define RT_LAUNCH_H

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime_api.h>

#include "rt_device.h"
#include "rt_camera_move.h"

extern "C" {

// ---- rt_kernels.hip
hipError_t rtk_launch_gather_pairs(uint32_t pairCount, const uint32_t *pairTri, const uint32_t *pairInfo, const float *triRec, float *pairRec, hipStream_t stream);
hipError_t rtk_launch_trace(const RtDevScene *scene, int counted, hipStream_t stream);
hipError_t rtk_launch_prepare(uint32_t triangleCount, const void *vertex, const void *triIndex, const void *triMaterial,
                              const void *triUv, const void *triNormal, float *triRec, float *triShade, hipStream_t stream);
hipError_t rtk_launch_detile(const void *tileBuf, const uint32_t *tileIds, uint32_t tileCount, uint32_t width,
                             uint32_t height, uint32_t tilesX, void *planeR, void *planeG, void *planeB, int accumulate, hipStream_t stream);

// ---- rt_scene_prep.hip
hipError_t rtp_validate(uint32_t T, uint32_t V, uint32_t M, const void *triIndex, const int *triMaterial, uint64_t camListSize,
                        const uint32_t *camList, const uint32_t *gridStart, uint64_t gridListSize, const uint32_t *gridList, uint32_t *err,
                        hipStream_t stream);
hipError_t rtp_camera_ranges(uint32_t W, uint32_t H, uint32_t tilesX, const uint32_t *tileIds, uint32_t tileCount, const uint32_t *camStart,
                             const uint32_t *camEnd, uint64_t camListSize, uint32_t *outStart, uint32_t *outEnd, uint32_t *err, hipStream_t stream);
hipError_t rtp_dense_grid(const uint32_t *gridStart, const uint32_t *gridList, unsigned long long *words, uint32_t *sparse, uint32_t *pairOrder,
                          uint32_t *pairCount, void *scratch, size_t *scratchBytes, hipStream_t stream);
hipError_t rtp_clip_support(const unsigned long long *words, const float *planeTable, const float *normals, uint32_t candidates, uint32_t *keys,
                            hipStream_t stream);

// ---- rt_camera_move.hip
hipError_t rtc_scan_bytes(uint32_t n, size_t *bytes);
hipError_t rtc_launch_count(const RtCamMoveArgs *args, hipStream_t stream);
hipError_t rtc_launch_fill(const RtCamMoveArgs *args, hipStream_t stream);

// ---- rt_scene_edit.hip (ids == NULL: the check reads word 21 of the triShade rows)
hipError_t rte_launch_check_ids(uint32_t T, uint32_t M, const int *ids, const float *triShade, uint32_t *err, hipStream_t stream);
hipError_t rte_launch_store_ids(uint32_t T, const int *ids, float *triShade, hipStream_t stream);

// ---- rt_wavefront.hip (the frame's kernels)
hipError_t rtw_launch_primary(const RtDevScene *scene, const RtWavefront *wf, hipStream_t stream);
hipError_t rtw_launch_primary_passes(const RtDevScene *scene, const RtWavefront *wf, uint32_t *passBuf, hipStream_t stream);
hipError_t rtw_launch_surface_passes(const RtDevScene *scene, const RtWavefront *wf, float *surfBuf, hipStream_t stream);
hipError_t rtw_launch_logic(const RtDevScene *scene, const RtWavefront *wf, uint32_t round, uint32_t blocks, uint32_t slicesIn, const RtRoundMode *next, hipStream_t stream);
hipError_t rtw_launch_answer(const RtDevScene *scene, const RtWavefront *wf, uint32_t round, uint32_t blocks, uint32_t slicesIn, const RtShadeList *list,
                             uint32_t shadeFollows, hipStream_t stream);
hipError_t rtw_launch_shade(const RtDevScene *scene, const RtWavefront *wf, uint32_t round, uint32_t blocks, uint32_t slicesIn, const RtRoundMode *next,
                            const RtShadeList *list, hipStream_t stream);
hipError_t rtw_launch_scatter(const RtWavefront *wf, uint32_t round, uint32_t blocks, const RtRoundMode *mode, hipStream_t stream);
hipError_t rtw_launch_place_skew(const RtWavefront *wf, uint32_t round, hipStream_t stream); // (test hook place_skew)
hipError_t rtw_launch_trace(const RtDevScene *scene, const RtWavefront *wf, uint32_t round, uint32_t blocks, const RtRoundMode *mode, hipStream_t stream);
hipError_t rtw_launch_status(const RtWavefront *wf, uint32_t round, uint32_t *shadeCount, hipStream_t stream);
hipError_t rtw_launch_accum(const RtDevScene *scene, const RtWavefront *wf, int first, hipStream_t stream);

// ---- rt_scene_passes.hip (what is traced against a resident scene outside the frame)
hipError_t rtw_launch_query(const RtDevScene *scene, const void *rays, const uint32_t *excluded, uint32_t count, void *hits,
                            uint32_t fastQuotient, hipStream_t stream);
hipError_t rtw_launch_matte_count(const RtDevScene *scene, const RtMatteArgs *args, hipStream_t stream);
hipError_t rtw_launch_matte_finish(const RtDevScene *scene, const RtMatteArgs *args, hipStream_t stream);
hipError_t rtw_launch_ao(const RtDevScene *scene, const RtAoArgs *args, hipStream_t stream);
hipError_t rtw_launch_ao_finish(const RtDevScene *scene, const uint32_t *counter, uint32_t samplesTimesRays, float *out, uint32_t rowMajor,
                                hipStream_t stream);
hipError_t rtw_launch_motion_mark(const float *triRec, void *ref, uint32_t triangles, hipStream_t stream);
hipError_t rtw_launch_motion(const RtDevScene *scene, const RtMotionArgs *args, hipStream_t stream);
hipError_t rtw_launch_bake_raster(const RtDevScene *scene, const RtBakeArgs *args, hipStream_t stream);
hipError_t rtw_launch_bake_points(const RtDevScene *scene, const RtBakeArgs *args, hipStream_t stream);
hipError_t rtw_launch_bake_ao(const RtDevScene *scene, const RtBakeArgs *args, hipStream_t stream);
hipError_t rtw_launch_bake_finish(uint32_t texels, const uint32_t *win, const uint32_t *counter, uint32_t rays, float fill, float *out,
                                  uint32_t *tri, hipStream_t stream);
hipError_t rtw_launch_bake_dilate(uint32_t W, uint32_t H, const float *src, float *dst, uint32_t last, hipStream_t stream);

// ---- rt_kat.hip (rtHipTestShadeKat's device part; not exported)
__attribute__((visibility("hidden"))) int rt_shade_kat_run(const RtDevScene *scene, int op, uint32_t count, const void *in, void *out);

// ---- rt_denoise.hip
hipError_t rtd_launch_guides(uint32_t n, const float *colour, const float *normal, const float *albedo, void *c0, void *g0, void *g1,
                             hipStream_t stream);
hipError_t rtd_launch_iteration(uint32_t W, uint32_t H, int h, float ic, float ia, uint32_t E, const void *cin, const void *g0,
                                const void *g1, void *cout, hipStream_t stream);
hipError_t rtd_launch_output(uint32_t n, const void *c, float *out, uint16_t *outR, uint16_t *outG, uint16_t *outB, hipStream_t stream);
hipError_t rtd_launch_gather(uint32_t W, uint32_t H, uint32_t tilesX, const uint32_t *tileIds, uint32_t tileCount, const uint16_t *tileBuf,
                             const float *surf, float S, float *colour, float *normal, float *albedo, hipStream_t stream);

// ---- rt_temporal.hip
hipError_t rtt_launch_accumulate(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *prevT,
                                 const uint32_t *triangle, const float *histColour, const float *histCount, const float *histT,
                                 const uint32_t *histTriangle, float *outColour, float *outCount, float maxHistory,
                                 float depthTolerance, hipStream_t stream);
hipError_t rtt_launch_accumulate_clamp(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *prevT,
                                       const uint32_t *triangle, const float *histColour, const float *histCount, const float *histT,
                                       const uint32_t *histTriangle, const float *histMoments, float *outColour, float *outCount,
                                       float *outMoments, float *outVariance, float maxHistory, float depthTolerance, uint32_t mode,
                                       float gamma, hipStream_t stream);
hipError_t rtt_launch_gather(uint32_t W, uint32_t H, uint32_t tilesX, const uint32_t *tileIds, uint32_t tileCount,
                             const uint16_t *tileBuf, float *colour, hipStream_t stream);
hipError_t rtt_launch_quantise(uint32_t n, const float *colour, uint16_t *outR, uint16_t *outG, uint16_t *outB, hipStream_t stream);

// ---- rt_motion_blur.hip (lz: 2 f32 per pixel; tileMax, nbMax: 4 f32 per 32 x 32 tile)
hipError_t rmb_launch(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *depth, float *out, float *lz,
                      float *tileMax, float *nbMax, float shutter, float maxBlur, uint32_t taps, float depthSoftness, hipStream_t stream);

// ---- rt_dof.hip (rz: 2 f32 per pixel; tileMax, nbMax: 1 f32 per 32 x 32 tile)
hipError_t rdf_launch(uint32_t W, uint32_t H, const float *colour, const float *depth, float *out, float *rz, float *tileMax, float *nbMax,
                      float focus, float cocScale, float maxCoc, uint32_t rings, float depthSoftness, hipStream_t stream);
hipError_t rdf_launch_scene_gather(uint32_t W, uint32_t H, uint32_t tilesX, const uint32_t *tileIds, uint32_t tileCount,
                                   const uint16_t *tileBuf, const uint32_t *passBuf, float *colour, float *depth, hipStream_t stream);

// ---- rt_variance.hip
hipError_t rtv_launch_moments(uint32_t W, uint32_t H, const float *colour, const float *motion, const float *prevT,
                              const uint32_t *triangle, const float *histColour, const float *histCount, const float *histT,
                              const uint32_t *histTriangle, const float *histMoments, float *outColour, float *outCount,
                              float *outMoments, float *outVariance, float maxHistory, float depthTolerance, hipStream_t stream);
hipError_t rtv_launch_estimate(uint32_t W, uint32_t H, const float *colour, const float *normal, const float *albedo,
                               const float *moments, const float *count, float spatialBelow, float ia, uint32_t E, void *s0,
                               void *g0, void *g1, hipStream_t stream);
hipError_t rtv_launch_iteration(uint32_t W, uint32_t H, int h, float ls, float floor_, float ia, uint32_t E, const void *sin,
                                void *il, const void *g0, const void *g1, void *sout, hipStream_t stream);
hipError_t rtv_launch_output(uint32_t n, const void *s, float *out, float *outVariance, uint16_t *outR, uint16_t *outG,
                             uint16_t *outB, hipStream_t stream);

} // extern "C"

#endif
