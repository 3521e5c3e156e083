/*
 * raytrace_hip.h -- C ABI of libraytrace_hip.so, the MI355X (gfx950) replacement for the reference's
 * ray-trace + shade hot path (reference: source/opencl/raytrace.c + raytrace_opencl.c, boundary raytrace.h:37-106).
 *
 * Two layers, both extern "C", plain pointers and sizes only (no HIP, torch or C++ types):
 *
 *  (1) DROP-IN layer  -- exactly the symbols the untouched plugin sources (render.cpp, trianglelist.cpp,
 *      writebmp.cpp) link against today, with the reference's names, argument order and error convention.
 *      Replacing raytrace.c by this library needs no change to any caller.
 *
 *  (2) RESIDENT layer (rtHip*) -- the same path split into upload / render / read-back so a host can keep a scene
 *      in HBM across frames, render a subset of 128x128 tiles (multi-GPU partition) and hand in device pointers.
 *      The drop-in RaytraceAll() is implemented on top of it.
 *
 * Vector layouts are the reference's padded OpenCL host types
 * (source/3rdparty/opencl-1.2/include/CL/cl_platform.h:501,725,1025): float3/int3 = 16 bytes (lane 3 is padding
 * and is never read), float2/uint2 = 8 bytes, uchar3 = 4 bytes.  When <CL/cl.h> has been included first the
 * cl_* names are used as-is, so this header can stand in for raytrace.h inside the plugin.
 */
#ifndef RAYTRACE_HIP_H
#define RAYTRACE_HIP_H

#include <stddef.h>
#include <stdint.h>
#include <time.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __OPENCL_CL_H
typedef int32_t  cl_int;
typedef uint32_t cl_uint;
typedef uint16_t cl_ushort;
typedef uint8_t  cl_uchar;
typedef int8_t   cl_char;
typedef float    cl_float;
typedef cl_uint  cl_bool;
typedef union { cl_float s[2]; } __attribute__((aligned(8)))  cl_float2;
typedef union { cl_uint  s[2]; } __attribute__((aligned(8)))  cl_uint2;
typedef union { cl_int   s[2]; } __attribute__((aligned(8)))  cl_int2;
typedef union { cl_float s[4]; } __attribute__((aligned(16))) cl_float4;
typedef union { cl_int   s[4]; } __attribute__((aligned(16))) cl_int4;
typedef union { cl_uchar s[4]; } __attribute__((aligned(4)))  cl_uchar4;
typedef cl_float4 cl_float3;
typedef cl_int4   cl_int3;
typedef cl_uchar4 cl_uchar3;
#define CL_FALSE 0
#define CL_TRUE  1
#endif

/* ------------------------------------------------------------------------------------------------------------
 * (1) DROP-IN layer
 * ---------------------------------------------------------------------------------------------------------- */

/* Replaces RaytraceAll (reference raytrace.h:58-106, raytrace.c:230-657).
 * computationType: 0 = the reference's in-thread CPU loop -- NOT provided by this library (it is the reference's
 * own code, raytrace.c:604-655): the call fails loudly and returns CL_FALSE.
 * k in 1..N = MI355X device k-1; N+1 = all N devices, image split into 128x128 tiles (only offered when N>1).
 * Blocking.  Caller owns every array; nothing is retained.  Output planes are zeroed first, like the reference's
 * OpenCL branch (raytrace.c:476,481,486), then accumulated.  Returns non-zero on success (raytrace.c:656). */
cl_bool RaytraceAll(cl_uint computationType,
                    cl_uint2 cameraImageDimension,
                    cl_float3 cameraEye,
                    cl_float3 cameraEyeToTopLeftVector,
                    cl_float3 cameraLeftToRightPixelSizeVector,
                    cl_float3 cameraTopToBottomPixelSizeVector,
                    cl_float cameraPixelSizeInv,
                    cl_uint *cameraPixelTriangleListStart,
                    cl_uint *cameraPixelTriangleListEnd,
                    cl_uint *cameraPixelTriangleList,
                    ptrdiff_t cameraPixelTriangleListSize,
                    cl_uint sampleCount,
                    cl_uint vertexCount,
                    cl_float3 *vertex,
                    cl_uint triangleCount,
                    cl_int3 *triangleVertexIndex,
                    cl_int *triangleMaterialId,
                    cl_float2 *triangleUv,
                    cl_float3 *triangleNormal,
                    cl_int axesDivCount,
                    cl_float3 *sceneBoxMin,
                    cl_uint *scenePixelTriangleListStart,
                    cl_uint *scenePixelTriangleList,
                    cl_uint materialCount,
                    cl_uint2 *materialImageSize,
                    cl_int *materialImageStart,
                    cl_uint texturesSize,
                    cl_uchar3 *textures,
                    cl_uint lightCount,
                    cl_int *lightType,
                    cl_float3 *lightPosition,
                    cl_float3 *lightDirection,
                    cl_float3 *lightColour,
                    cl_float *lightRadius,
                    cl_float *lightHalfAttenuationDistance,
                    cl_ushort *outputRed,
                    cl_ushort *outputGreen,
                    cl_ushort *outputBlue);

/* Device enumeration (reference raytrace.h:46-50, raytrace.c:74-153).  Name 0 is the literal
 * "Local CPU single thread" (raytrace.c:138); names 1..N are "AMD HIP <device name>"; name N+1 (N>1 only) is
 * "AMD HIP all N GPUs (tiled)".  InitOpenCL publishes the table last, like raytrace.c:117-120. */
void    InitOpenCL(void);
void    ResetComputationType(void);
cl_bool GetIsComputationTypeUpdated(void);
size_t  GetComputationTypeCount(void);
cl_bool GetComputationTypeName(size_t id, size_t strLen, cl_char *str);

/* Progress / timing polled by the GUI thread (reference raytrace.h:52-56, raytrace.c:156-173).  Progress stays
 * below 1 until the caller sets it (raytrace.c:580,607,614); start time becomes non-zero when the kernel phase
 * begins; relaxed atomics inside. */
cl_float GetProgress(void);
void     SetProgress(cl_float p);
clock_t  GetStartTime(void);
clock_t  GetEndTime(void);
void     ResetTime(void);

/* Math helpers other plugin translation units link against (reference raytrace.h:37-44; definitions
 * raytrace.c:18-45 and raytrace_opencl.c:83-101,124-172,174-193).  fp32, no contraction, same operation order. */
cl_float  dot(cl_float3 a, cl_float3 b);
cl_float3 cross(cl_float3 a, cl_float3 b);
cl_float3 normalize(cl_float3 v);
cl_float3 vector(cl_float3 a, cl_float3 b);
cl_float  bindf(cl_float value, cl_float a, cl_float b);
cl_float  GetPointToLineSqLen(cl_float3 origin, cl_float3 destination, cl_float3 point);
cl_bool   RayIntersectsTriangle(cl_float3 origin, cl_float3 ray, cl_float minDistance, cl_float maxDistance,
                                cl_float3 a, cl_float3 b, cl_float3 c,
                                cl_float *outRayMult, cl_float *outABL, cl_float *outACL);
cl_int3   GetBoxAddress(cl_int axesDivCount, cl_float3 *boxMin, cl_float3 position);

/* ------------------------------------------------------------------------------------------------------------
 * (2) RESIDENT layer
 * ---------------------------------------------------------------------------------------------------------- */

#define RT_HIP_TILE 128 /* tile edge in pixels: the reference's NDRange granule (raytrace.c:507) */

/* Everything RaytraceAll receives except the device choice and the output planes (same meaning, same layouts). */
typedef struct rtHipSceneDesc {
    cl_uint   width, height;
    cl_float  eye[4], eyeToTopLeft[4], leftToRight[4], topToBottom[4];
    cl_float  pixelSizeInv;
    const cl_uint *camStart, *camEnd, *camList;
    uint64_t  camListSize;
    cl_uint   sampleCount;
    cl_uint   vertexCount;
    const cl_float3 *vertex;
    cl_uint   triangleCount;
    const cl_int3 *triIndex;
    const cl_int  *triMaterial;
    const cl_float2 *triUv;
    const cl_float3 *triNormal;
    cl_int    axesDiv;
    const cl_float3 *boxMin;
    const cl_uint *gridStart, *gridList;
    cl_uint   materialCount;
    const cl_uint2 *matSize;
    const cl_int   *matStart;
    cl_uint   texturesSize;
    const cl_uchar3 *textures;
    cl_uint   lightCount;
    const cl_int *lightType;
    const cl_float3 *lightPos, *lightDir, *lightCol;
    const cl_float *lightRadius, *lightHalfAtt;
    cl_int    arraysOnDevice;   /* 0: every array is host memory (what RaytraceAll receives).  1: every array pointer is DEVICE memory of the
                                 * GPU the scene is created on -- e.g. the tensors an RCCL broadcast left there -- and is copied device to
                                 * device; only the small tables the host has to look at (split planes, material tables, texels, lights,
                                 * one grid word) come back to it */
} rtHipSceneDesc;

typedef struct rtHipScene rtHipScene; /* opaque: a scene resident in one GPU's HBM */

/* Work counters of one render, for the algorithmic-byte model. */
typedef struct rtHipStats {
    uint64_t primarySamples, primaryCandidates, gridRays, gridCells, gridCandidates, shadedHits, texelFetches;
} rtHipStats;

/* RaytraceAll keeps the scenes of its last call resident and rebuilds only what changed (content hashes of the input arrays:
 * geometry, grid, materials | lights | camera lists | sample count).  rtHipCacheClear frees them; RT_HIP_CACHE=0 makes every
 * call build and free, like the reference (raytrace.c:330-489,594-602). */
void rtHipCacheClear(void);

/* Number of HIP devices (0 when none / no driver).  Never fails. */
int rtHipDeviceCount(void);

/* Last error text of the calling thread ("" when none). */
const char *rtHipLastError(void);

/* Uploads a scene to `device` and builds the device-side layout (pre-resolved triangle records etc.).
 * tileCount/tileIds select the 128x128 tiles this scene instance will render (row-major tile ids); NULL/0 = all.
 * Only those tiles' slices of the camera lists are uploaded.  Returns NULL on failure.
 * Every id the kernels will index with is checked on the device before anything gathers through it, and a scene that fails is refused
 * with "scene rejected (0x<bits>): ..." in rtHipLastError(): a vertex id outside [0, vertexCount) in lanes x, y, z of a triangle (lane w
 * is never read), a material id >= materialCount (any negative id is legal and means "no material"), a camera or grid list entry >=
 * triangleCount, a pixel range that ends past cameraPixelTriangleListSize (End < Start is legal and reads as empty), and grid starts
 * that descend (equal starts are an empty cell).  The pixel ranges are read -- and therefore checked -- only for the pixels of THIS
 * instance's tiles: a bad range in a tile the instance does not own is not refused here, on purpose (the instance that owns the tile
 * refuses it); the camera LIST is uploaded whole and every entry of it is checked, also one that no pixel's range covers. */
rtHipScene *rtHipSceneCreate(int device, const rtHipSceneDesc *desc, const cl_uint *tileIds, cl_uint tileCount);
/* The same for a further instance of a scene that is already resident somewhere (`like`, built from the same description, on this or
 * another device): geometry, grid, materials and lights are copied from it device to device (hipMemcpyPeerAsync: xGMI between
 * GPUs) instead of uploaded and reshaped once more; only the instance's own tiles, camera ranges and path state are made anew. */
rtHipScene *rtHipSceneCreateLike(int device, const rtHipSceneDesc *desc, const cl_uint *tileIds, cl_uint tileCount, const rtHipScene *like);
void        rtHipSceneDestroy(rtHipScene *scene);

/* Bytes of HBM held by the scene. */
uint64_t rtHipSceneBytes(const rtHipScene *scene);

/* The camera of a resident scene, moved on the device.  rtHipSceneGetCamera gives the five fields in effect (after creation: the
 * description's; lane 3 of the vectors reads 0).  rtHipSceneSetCamera replaces them and rebuilds the per-pixel candidate lists of the
 * instance's tiles for the new view from the triangles the scene already holds (rt_camera_move.hip), so that a second view of a scene
 * costs a list build instead of a new scene.
 *   Equivalence.  After it returns 0 the scene is, for everything the public API shows, the scene rtHipSceneCreate would have made from
 *   the same description with the five camera fields replaced and camStart / camEnd / camList = what rtHipBuildCameraList returns for
 *   that camera (same image size, tile set and sample count): every later frame (both pipelines), rtHipReadbackPasses,
 *   rtHipReadbackSurfacePasses, rtHipSceneDenoise and rtHipSceneAmbientOcclusion result is bit-identical to that scene's.  Ray queries
 *   and the ambient occlusion bake do not read the camera and are unchanged.  "The same lists" are the same CONTENTS: every pixel of
 *   the instance's tiles reads the triangles the host builder gives it, in ascending order (one shared header decides membership for
 *   both).  The range numbers differ: the moved scene's ranges do not share storage between neighbouring pixels, its list is the
 *   concatenation of the pixels' lists in tile-major order, and pixels of a tile that lie outside the image read nothing.
 *   Only this instance's tiles.  An instance over a tile subset builds ranges for its own tiles; pixels of other tiles are dropped
 *   before their membership test.  Peers made with rtHipSceneCreateLike are moved one by one by the caller, and instances over a
 *   disjoint deal of the tiles still compose the full image.
 *   Everything stays on the device.  No vertex, index, range or list array crosses the bus in either direction; the host sends the
 *   camera and receives 16 bytes (the 64-bit entry total and the number of large triangles).  Geometry, grid, materials, lights, path
 *   state and the pass / surface / denoise / AO / bake scratch keep their allocations and addresses.
 *   Ordering.  The call is synchronous on the scene's own stream: it waits for the work already issued there (a frame in flight reads
 *   the old lists; planned frames are verified as by rtHipFrameFinish first) and on return the new camera is in effect for everything
 *   issued afterwards.  A caller that rendered on a stream of its own synchronises that stream first, as for rtHipReadback.  The launch
 *   plan of the old view is dropped: the next frame is a watched one.
 *   Transactional.  The new view is built into storage the frames do not read and takes the old one's place at the very end; on any
 *   failure the scene keeps its old camera and lists and renders what it rendered before.  Returns -1 for a NULL argument, -3 when the
 *   view's lists hold more than 2^32 - 1 entries or more than rtHipTune("build_list_limit", n) (decided from the 64-bit total before the
 *   list is sized, like rtHipBuildCameraListDevice), -4 when device memory could not be had, -2 for any other HIP failure; each with a
 *   text in rtHipLastError().
 *   Every bit pattern of the camera has a defined answer -- NaN, infinities, pixelSizeInv 0, an eye inside a triangle: the lists are
 *   those rtHipBuildCameraList gives for the same values.  Nothing is refused for its value and nothing indexes out of range.
 *   Memory.  The first move makes the build storage: 24 bytes per triangle of projected vertices, 4 per triangle for the list of large
 *   triangles, 4 per tile pixel of counts, the tile slot tables and the scan's temporaries in one block, and TWO sets of ranges (8 bytes
 *   per tile pixel each).  A move builds into the set that is not in use; the lists the scene was created with are freed after the first
 *   move.  A list buffer that is too small for a view is replaced by one of entries + entries / 8 (at least 1024) entries and never
 *   shrinks, and after a move the other set's list is made as large, so that a later move to a view of no more entries allocates
 *   nothing.  All of it is counted in rtHipSceneBytes and freed with the scene.
 *   Tuning.  The call reads "build_list_limit" once at entry, so a rtHipTune call made after the scene was created is seen by the next
 *   move; the scene's other tuning values stay those it was built with. */
typedef struct rtHipCamera {
    cl_float eye[4], eyeToTopLeft[4], leftToRight[4], topToBottom[4]; /* lane 3 is never read */
    cl_float pixelSizeInv;
} rtHipCamera;
int rtHipSceneGetCamera(const rtHipScene *scene, rtHipCamera *out);
int rtHipSceneSetCamera(rtHipScene *scene, const rtHipCamera *camera);

/* The SHAPE of a resident scene, changed on the device.  rtHipSceneSetGeometry replaces the vertex array (and, where given, the index array
 * and the corner normals) of a resident scene and rebuilds everything that depends on them where the data lives: triangle records, the
 * 256^3 grid, its dense view and pair records, and the per-pixel candidate lists of the camera in effect.  The triangle count never changes.
 *   Equivalence.  After it returns 0 the scene is, for everything the public API shows, the scene rtHipSceneCreate would have made from
 *   the same description with vertexCount, vertex (and triIndex, triNormal where given) replaced, boxMin / gridStart / gridList = what
 *   rtHipBuildSceneGrid returns for the new arrays, the camera in effect (after any rtHipSceneSetCamera) and camStart / camEnd / camList =
 *   what rtHipBuildCameraList returns for it: every later frame on both pipelines, pass, surface pass, denoise, AO image, AO bake and ray
 *   query is bit-identical to that scene's.  The per-pixel lists have the same CONTENTS as the host builder's, as after a camera move
 *   (range numbers may differ, see there).  UVs, material ids, materials, lights, tile set, sample count, pipeline and pass mask are
 *   untouched.
 *   Stages, all on the scene's stream: host arrays are staged to the device (device pointers are checked like rtHipSceneIntersectDevice's);
 *   every index is checked on the device before anything gathers through it (a retained index array too: V may have shrunk); new triangle
 *   records (rt_prepare_triangles' operations; UV, material and -- without triNormal -- normal words are carried over from the rows the
 *   scene holds); the grid from the device-resident arrays by the kernels of rtHipBuildSceneGridDevice; the dense view and the pair
 *   records; the camera lists through the resident camera build of rtHipSceneSetCamera; the swap.
 *   Everything stays on the device.  No array whose size grows with V, T, the pair count or the list entries crosses the bus from device
 *   to host, and host to device only the caller's own host arrays (and 4 KB of planes and cell table).  What the host reads: the error
 *   word, the fill's counters (24 bytes, up to four times), the 257 x 16 bytes of split planes, the camera build's 16 bytes.  Materials,
 *   lights, path state and the pass / surface / denoise / AO / bake scratch keep their allocations and addresses.
 *   Transactional.  The new records, grid and lists are built into storage the frames do not read and take the old ones' place at the
 *   very end; on any failure the scene keeps its old shape, camera lists, retained index array and launch plan and renders what it
 *   rendered before.  Returns -1 for a NULL argument, a NULL vertex with vertexCount > 0, triIndex == NULL when nothing is retained (a
 *   scene drops the index array it was created with: the first update brings one), or a bad device pointer; -5 with the text
 *   "scene rejected (0x..): ..." for an index outside [0, vertexCount); -3 when the grid holds 2^28 pairs or more (the trace kernel's record
 *   limit) or more than rtHipTune("build_list_limit"), or the camera lists exceed that limit; -7 as rtHipBuildSceneGridDevice; -4 when device
 *   memory could not be had; -2 for any other HIP failure; each with a text in rtHipLastError().
 *   Ordering.  Synchronous on the scene's own stream like rtHipSceneSetCamera: it waits for what was issued there, planned frames are
 *   verified first, and on return the new shape is in effect for everything issued afterwards; the launch plan is dropped, the next frame
 *   is a watched one.  With arraysOnDevice == 1 the CALLER has synchronised the stream that produced the arrays before the call (there is
 *   no stream argument), and the arrays are not needed after it returns.
 *   Vertices that are not finite: no promise beyond "the grid rtHipBuildSceneGridDevice gives for the same arrays".  Degenerate triangles
 *   (zero area, repeated corners) are handled like everywhere else.
 *   Peers.  Instances made with rtHipSceneCreateLike and instances over tile subsets are updated one by one by the caller; each builds
 *   its own grid.  A scene that was updated can be the `like` of a new instance.
 *   Memory.  The first update makes a SECOND set of everything the kernels read of the shape (64 + 128 bytes per triangle, 64 MB of grid
 *   starts, 50 MB of block table, 2 MB of occupancy words, 4 + 64 bytes per pair) -- updates build into the set that is not in use, and
 *   the parts the scene was created with are freed after the first one -- and the build scratch, which stays: the grid build's storage
 *   (two key buffers of max(32 T, 2^22) x 8 bytes, 24 bytes per vertex, 64 MB of cell counts, sort temporaries; when a triangle is too
 *   large for one thread also 8 fill queues of 64 MB and 16 maps of 2 MB), staging for host vertices and normals (made by the first update
 *   from host arrays, the normals' whether it brings normals or not), two index arrays of 16 bytes per triangle (the retained one and
 *   the one being checked), 4 bytes per triangle of stand-in material ids, 8 bytes per pair
 *   of pair order, and the camera move's storage.  A buffer too small for an update is replaced by one of needed + needed / 8 and never
 *   shrinks, and after an update the other set is made as large, so that a later update needing no more pairs and list entries
 *   allocates nothing.  All of it is counted in rtHipSceneBytes and freed with the scene.  A scene that is never updated holds none of it.
 *   Tuning.  The call reads "build_list_limit" and "build_key_cap" once at entry. */
typedef struct rtHipGeometryUpdate {
    cl_uint          vertexCount;     /* V of the new vertex array */
    const cl_float3 *vertex;          /* V x 16 bytes, required */
    const cl_int3   *triIndex;        /* T x 16 bytes (T = the scene's triangle count, which never changes); NULL = the index array the
                                         scene retained from its previous successful update */
    const cl_float3 *triNormal;       /* 3T x 16 bytes of corner normals; NULL = keep the normals the scene holds */
    cl_int           arraysOnDevice;  /* as in rtHipSceneDesc: 0 host arrays, 1 device arrays of the scene's device (16-byte aligned) */
} rtHipGeometryUpdate;
int rtHipSceneSetGeometry(rtHipScene *scene, const rtHipGeometryUpdate *update);

/* SCENE EDITS: LIGHTS AND MATERIALS.  The lights, the material tables and atlas, and the triangles' material ids of a resident scene,
 * replaced in place: rtHipSceneSetLights takes six new light arrays; rtHipSceneSetMaterials takes new tables and atlas
 * (replaceMaterials = 1), new material ids (triMaterial != NULL), or both.  A light is a few hundred bytes; none of these needs a new scene.
 *   Equivalence.  After a call returns 0 the scene is, for everything the public API shows, the scene rtHipSceneCreate would have made
 *   from the same description with the light arrays, the material tables / atlas and / or triMaterial replaced, the camera and the shape
 *   in effect (after any rtHipSceneSetCamera / rtHipSceneSetGeometry) staying as they are: every later frame on both pipelines, pass,
 *   surface pass (albedo and bump-mapped normals change with the materials), denoise, AO image, AO bake (its `material` filter reads the
 *   id word), ray query and motion output is bit-identical to that scene's, and rtHipTestPathClass equals rtHipScenePathClass of that
 *   description: a second light, or a reflective, transparent or luminous channel, moves the scene from the opaque-diffuse class to the
 *   general one, and taking them away moves it back.
 *   What a call leaves alone.  Geometry, grid, camera lists, tile set, pipeline, pass mask and stage-timing switch; the sample window,
 *   both what rtHipSceneGetSampleWindow reports as `next` and as `last`; the contents of the tile, pass and surface buffers (an
 *   accumulating window is not wiped); the motion reference and the temporal / moments history.  Whether a re-lit frame may blend with
 *   older ones is the CALLER's decision: call rtHipSceneTemporalReset where it may not.
 *   Light count.  Path state that only scenes of several lights use (16 + 8 bytes per path) is made by the first edit that brings a
 *   second light and kept from then on; no other path state is touched, whichever way the count crosses the one / several boundary.
 *   Ordering.  Synchronous on the scene's own stream like rtHipSceneSetCamera: the call waits for what was issued there, planned frames
 *   are verified first, and on return the edit is in effect for everything issued afterwards; the launch plan is dropped, the next frame
 *   is a watched one.  With triMaterialOnDevice == 1 the CALLER has synchronised the stream that produced the ids before the call.
 *   Transactional.  New tables, atlas and light arrays are built into storage the frames do not read and take the old ones' place at
 *   the very end; the old ones are freed after that.  Material ids are checked completely, on the device, before the first one is
 *   stored.  On any failure the scene renders what it rendered before and holds its tables and light arrays at their old addresses.
 *   Returns -1 for a NULL argument, lightCount >= 65536, a NULL light array with lightCount > 0, a NULL table with materialCount > 0, a
 *   channel of w > 0 texels a row whose matStart is negative or whose start + w * h exceeds texturesSize (w and h are full 32-bit values:
 *   the sum is formed without wrapping), a triMaterial that is not device memory of the scene's device, 4-byte aligned and T ids long
 *   when triMaterialOnDevice == 1 (checked like rtHipSceneIntersectDevice's pointers), or an update that brings neither tables nor ids;
 *   -5 with the text "scene rejected (0x..): ..." for an id >= materialCount among the ids that will be in effect -- the new triMaterial,
 *   or, with triMaterial == NULL and a smaller materialCount, the RESIDENT ids; every negative id is legal ("no material") --; -4 when
 *   device memory could not be had; -2 for any other HIP failure; each with a text in rtHipLastError().  rtHipLightsCheck and
 *   rtHipMaterialsCheck decide everything that needs neither a scene nor a GPU (0, or -1 with the text); the Set calls run them first.
 *   Values.  No light or texel value is refused: NaN, infinities, negative colours render as they would in a scene created with them.
 *   Ids.  The material id lives in one word of a triangle's 128-byte shading row; new ids are written into the rows in use, and a later
 *   rtHipSceneSetGeometry carries them over.  Host ids are staged to the device; device ids are read in place.
 *   Peers.  Instances made with rtHipSceneCreateLike and instances over tile subsets are edited one by one by the caller.  An edited
 *   scene can be the `like` of a new instance whose description describes the edited state.
 *   Memory.  New tables and arrays replace the old ones; host ids are staged in 4 bytes per triangle made by the first call that brings
 *   some.  Everything is counted in rtHipSceneBytes and freed with the scene; repeating an edit of the same sizes leaves rtHipSceneBytes
 *   unchanged from the second repetition on.
 *   rtHipSceneEditTimes gives the device time of the last successful edit's stages, from events on the scene's stream, in ms: [0] the
 *   light arrays, [1] the material tables and atlas, [2] the id check and the id store (0 for a stage the edit did not have). */
typedef struct rtHipLights {            /* host arrays, as in rtHipSceneDesc */
    cl_uint lightCount;
    const cl_int *lightType;
    const cl_float3 *lightPos, *lightDir, *lightCol;
    const cl_float *lightRadius, *lightHalfAtt;
} rtHipLights;
typedef struct rtHipMaterialUpdate {
    cl_int  replaceMaterials;           /* 0: keep the resident tables and atlas; the five fields below are ignored */
    cl_uint materialCount;
    const cl_uint2 *matSize;            /* 5 per material */
    const cl_int   *matStart;           /* 5 per material */
    cl_uint texturesSize;
    const cl_uchar3 *textures;
    const cl_int *triMaterial;          /* T ids (T = the scene's triangle count), or NULL = keep the resident ids */
    cl_int  triMaterialOnDevice;        /* 1: triMaterial is device memory of the scene's device, 4-byte aligned */
} rtHipMaterialUpdate;
int rtHipLightsCheck(const rtHipLights *lights);
int rtHipMaterialsCheck(const rtHipMaterialUpdate *update);
int rtHipSceneSetLights(rtHipScene *scene, const rtHipLights *lights);
int rtHipSceneSetMaterials(rtHipScene *scene, const rtHipMaterialUpdate *update);
int rtHipSceneEditTimes(const rtHipScene *scene, double ms[3]);

/* Renders all samples of the scene's tiles into its device-resident tile buffer
 * ([tile][plane R,G,B][128*128] u16, tiles in the order given at creation).  Asynchronous on `stream`
 * (a hipStream_t passed as void*; NULL = the scene's own stream).  Returns 0 on success. */
int rtHipRenderTiles(rtHipScene *scene, void *stream);

/* Frames after a scene's first are issued WITHOUT any host synchronisation (the first frame leaves a launch plan behind: how
 * many rounds the frame needs and how big each is; frames of one scene are deterministic).  Whether such a frame really was
 * complete is checked afterwards: rtHipSync and rtHipReadback do it themselves; a caller that consumes the tile buffer on the
 * stream (an RCCL gather enqueued behind the frame) calls rtHipFrameFinish once its own synchronisation is over.  If the plan
 * was too short the last frame is rendered again, watched, and *redone (optional) is set to 1: work that was enqueued behind
 * the incomplete frame has to be repeated.  RT_WF_BLOCKING=1 makes every frame a watched one.  Returns 0 on success. */
int rtHipFrameFinish(rtHipScene *scene, int *redone);

/* SAMPLE WINDOWS: successive frames of a resident scene draw different samples.  By default every frame renders samples 1..S of a
 * sequence of S (S = the sampleCount the scene was created with): sample s of pixel p is seeded p*S + s (raytrace_opencl.c:481), its
 * addend is trunc(out * (65535.0f / (float)S)), added with saturation in sample order (:726-741) -- so every frame of a still scene is
 * the same frame.  A window makes the frame a slice of a longer sequence instead:
 *   total      N: samples per pixel of the whole sequence = the seed stride; sample id i of pixel p is seeded (uint64)p*N + i
 *   first      f: the frame renders sample ids f+1 .. f+S, in that order (S is unchanged: it is what the path-state buffers are sized for)
 *   divisor    D: a sample's addend is trunc(out * (65535.0f / (float)D)), saturating, in sample order
 *   accumulate 1: the frame's first addend follows on what the tile buffer holds, unless f == 0 (the start of a sequence starts from
 *              zero); 0: every frame starts from zero
 *   advance    1: every frame issued moves f to (f + S) % N for the next one
 * The default window is {S, 0, S, 0, 0}; under it every kernel computes exactly what it computed before windows existed.
 * An N-sample frame of the reference is the ordered saturating sum of its samples' addends, which gives the two uses:
 *   PROGRESSIVE {N, 0, N, 1, 1}: after N / S frames the tile buffer is bit for bit the N-sample frame, saturation included.  The tile
 *              buffer may be read after any frame; the caller scales what it reads by N / done for a preview (no device-side preview).
 *   SEQUENCE   {N, 0, S, 0, 1}: each frame is a full-brightness image of S fresh samples per pixel; the frames repeat after N / S.  This
 *              is the input the temporal accumulation and the variance-guided filter (their blocks below) need under a still or
 *              slowly moving camera.
 * rtHipSampleWindowCheck (host only, no device) and rtHipSceneSetSampleWindow return -1 with the last-error text set for N == 0, D == 0,
 * f + S > N (compared in 64 bits), accumulate or advance other than 0 or 1, and advance with N % S != 0 or f % S != 0; a refused set
 * leaves the scene's window and its next frame unchanged.  A set is host-side state the next frame issued picks up: it synchronises
 * nothing, allocates nothing and keeps the launch plan (other sample ids of the same pixels need statistically the same rounds; a plan
 * that is too short is caught by rtHipFrameFinish as ever).  NULL sets the default window.
 * rtHipSceneGetSampleWindow: *next = the window the next frame will use, *last = the one the last issued frame used (all zero before
 * the first frame); either may be NULL.
 * Frames and their verification.  `advance` is applied when a frame is issued; an rtHipRenderTiles that returns -1 moves nothing
 * and leaves *last alone.  A frame rendered again by rtHipFrameFinish, rtHipSync or
 * rtHipReadback renders the window that frame had (*last) and does not advance again.  A frame that continues from the tile buffer
 * (accumulate == 1, f > 0) has already added into the planes when it is found incomplete and could not be redone: such frames are issued
 * with every batch watched, as under RT_WF_BLOCKING=1, after the frames before them are verified.
 * Both pipelines honour the window and keep producing identical planes.  Render passes (ALPHA, DEPTH, TRIANGLE, NORMAL, ALBEDO)
 * describe the window's own S samples: "sample 1" is sample id f + 1, means and alpha divide by S; passes never accumulate across
 * windows.  rtHipSceneDenoise, rtHipSceneTemporal and rtHipSceneTemporalVariance read the tile buffer, whatever window filled it.
 * rtHipRenderTilesCounted returns -1 while a window other than the default is in effect.  A scene made by RaytraceAll's cache or by
 * rtHipSceneCreateLike starts with the default window: instances (peers, tile subsets) are set one by one, and disjoint tile deals
 * under the same window still compose one image.
 * What leaves the window alone.  The window (*next, with the f it has advanced to) and *last belong to the scene, not to its camera,
 * geometry or pipeline: rtHipSceneSetCamera, rtHipSceneSetGeometry, rtHipSetPipeline, rtHipScenePasses, rtHipSceneMotionMark, the
 * filters, rtHipSceneTemporalReset and every refused call leave both as they are, and none of them touches the tile buffer.  So a frame
 * that continues after a move or an update adds its window's samples of the NEW state to what the frames of the old state left: a
 * plain mixture, defined and seldom wanted -- a caller that moves something mid-run sets the window again to start from f = 0. */
typedef struct rtHipSampleWindow {
    cl_uint total;      /* N */
    cl_uint first;      /* f */
    cl_uint divisor;    /* D */
    cl_uint accumulate; /* 0 or 1 */
    cl_uint advance;    /* 0 or 1 */
} rtHipSampleWindow;
int rtHipSampleWindowCheck(cl_uint sampleCount, const rtHipSampleWindow *window);
int rtHipSceneSetSampleWindow(rtHipScene *scene, const rtHipSampleWindow *window);
int rtHipSceneGetSampleWindow(const rtHipScene *scene, rtHipSampleWindow *next, rtHipSampleWindow *last);

/* Two implementations of the same frame (identical planes):
 *   WAVEFRONT (default) staged pipeline: primary -> rounds of (per-path logic, length sort of the new ray requests, grid
 *                       trace) -> ordered accumulate.  The first frame of a scene watches its ray queue from the host; later frames
 *                       are issued without synchronisation (rtHipFrameFinish).
 *                       Tuning aids read at scene creation: RT_WF_LOOKAHEAD=0|1, RT_WF_SEG="a,b,c,d" and
 *                       RT_WF_SEG_RAYS="a,b,c" (ray segmentation by round size), RT_WF_APPEND_RAYS=n (rounds below n rays skip the length sort), RT_WF_GROUPS=n, RT_WF_STATE_MB.
 *   MEGAKERNEL          one launch, one thread per pixel (kept for A/B runs and for the work counters). */
#define RT_HIP_PIPELINE_MEGAKERNEL 0
#define RT_HIP_PIPELINE_WAVEFRONT  1
int rtHipSetPipeline(rtHipScene *scene, int pipeline);

/* Per-stage device time: enable, render frames, then read the SUM over those frames in milliseconds for
 * [0] primary, [1] logic, [2] grid trace, [3] accumulate, [4] length sort of the trace input (HIP events on the launch
 * stream; adds two event records per launch, so leave it off in timed whole-frame runs).  *rounds = logic/trace rounds
 * of the last frame. */
int rtHipStageTiming(rtHipScene *scene, int enable);
int rtHipStageTimes(rtHipScene *scene, double ms[5], uint64_t *rounds);

/* Diagnostic: copies the scene's 8 device-side debug counters (and optionally clears them).  Synchronous. */
int rtHipDebugCounters(rtHipScene *scene, unsigned long long out[8], int clear);

/* Same, with work counters (slower; never used inside a timed region).  Synchronous. */
int rtHipRenderTilesCounted(rtHipScene *scene, rtHipStats *stats);

/* Device pointer / size in bytes of the tile buffer (for RCCL gathers and peer copies). */
void    *rtHipTileBuffer(rtHipScene *scene);
uint64_t rtHipTileBufferBytes(const rtHipScene *scene);

/* De-tiles `tileCount` tiles held in a device buffer laid out like rtHipTileBuffer into three row-major
 * width x height u16 DEVICE planes (saturating add into what is there).  Used by the gather root, once per
 * source rank.  tileIdsDevice is a DEVICE array of row-major tile ids (ids >= the image's tile count are
 * skipped).  Asynchronous on `stream` (a hipStream_t as void*, NULL = the default stream); no allocation. */
int rtHipDetile(int device, const void *tileBuffer, const cl_uint *tileIdsDevice, cl_uint tileCount,
                cl_uint width, cl_uint height, void *planeR, void *planeG, void *planeB, void *stream);

/* The same without the accumulate: the planes' pixels are overwritten by the tiles' (a gather root that would zero its planes first
 * anyway -- every pixel belongs to exactly one tile of a deal).  Pixels no tile covers keep their value. */
int rtHipDetileStore(int device, const void *tileBuffer, const cl_uint *tileIdsDevice, cl_uint tileCount,
                     cl_uint width, cl_uint height, void *planeR, void *planeG, void *planeB, void *stream);

/* Plain device memory for hosts that do not include HIP headers (a gather root's planes): allocate, free, and a blocking copy
 * (toDevice != 0: host -> device, else device -> host; the device is synchronised first). */
void *rtHipDeviceAlloc(int device, uint64_t bytes);
void  rtHipDeviceFree(int device, void *p);
int   rtHipDeviceCopy(int device, void *dst, const void *src, uint64_t bytes, int toDevice);

/* Blocks until the scene's work is done, then adds its tiles into three HOST planes (width*height u16 each). */
int rtHipReadback(rtHipScene *scene, cl_ushort *outR, cl_ushort *outG, cl_ushort *outB);

/* Waits for `stream` (NULL = scene stream). */
int rtHipSync(rtHipScene *scene, void *stream);

/* Render passes next to the beauty image (opt-in per scene, wavefront pipeline only).  For pixel p and its samples s = 1..S, from the
 * primary rays the frame traces anyway:
 *   ALPHA     u16  hits * 65535 / S (64-bit integer arithmetic, truncated); hits = samples whose primary ray hit a triangle
 *   DEPTH     f32  sample 1's eye-to-hit distance t * sqrt((dx*dx + dy*dy) + dz*dz) (its direction is not normalised); +inf on a miss
 *   TRIANGLE  u32  the triangle sample 1's primary ray hit; 0xffffffff on a miss
 * rtHipScenePasses allocates the pass buffer on first use (or frees it: mask 0) and takes effect from the next frame; it fails on a
 * scene on the megakernel pipeline, and rtHipSetPipeline(MEGAKERNEL) fails while passes are on.  The buffer is laid out like the tile
 * buffer: [slot][hits u32 | depth f32 | triangle u32][128*128].  rtHipReadbackPasses synchronises and finishes the frame like
 * rtHipReadback, then STORES the pixels of the scene's own tiles into row-major width x height host arrays (every other pixel keeps
 * its value, so instances with disjoint tile sets compose one image); NULL = not wanted, asking for a pass that is off is an error. */
#define RT_HIP_PASS_ALPHA    1u
#define RT_HIP_PASS_DEPTH    2u
#define RT_HIP_PASS_TRIANGLE 4u
int      rtHipScenePasses(rtHipScene *scene, cl_uint mask);
void    *rtHipPassBuffer(rtHipScene *scene);
uint64_t rtHipPassBufferBytes(const rtHipScene *scene);
int      rtHipReadbackPasses(rtHipScene *scene, cl_ushort *alpha, cl_float *depth, cl_uint *triangle);

/* Surface passes, the auxiliary images a denoiser takes next to the beauty: MEANS over all S samples of a pixel (anti-aliased like the
 * beauty), 3 x f32 per pixel, row-major and interleaved (xyz / rgb).  Sample s = 1..S of pixel p = y*W + x is the primary ray the renderer
 * traces: seed p*S + s, LR jitter first, then TB, the pixel's camera list scanned in order with a running closest hit (ties keep the
 * earlier candidate).  On a hit (tri, t, abL, acL), with where = eye + t*dir per component in fp32:
 *   NORMAL  n_s = GetTriangleNormal(where, eye, dir, tri, abL, acL) (raytrace_opencl.c:195-263, called at :548), the vector the
 *           renderer shades with: Phong-interpolated, NOT normalised unless a bump map applies, not flipped toward the viewer
 *   ALBEDO  a_s = the material's colour-channel texel at (abL, acL) (Get2dTableValue3, :554); (0,0,0) for material -1 or no colour channel
 * A miss gives n_s = a_s = (0,0,0).  Per component, in fp32:  acc = +0.0f; for s = 1..S in order: acc = acc + v_s;  pass = acc / (float)S.
 * The ALPHA pass tells where a mean mixes hits and misses.
 * The surface buffer is separate from the pass buffer: [slot][nx ny nz ar ag ab][128*128] f32 holding the SUMS (not the means).  The
 * pass buffer is used exactly while ALPHA, DEPTH or TRIANGLE is on, the surface buffer exactly while NORMAL or ALBEDO is on; each is
 * made on first need, freed when its bits go off, and counted in rtHipSceneBytes.  rtHipReadbackSurfacePasses has the contract of
 * rtHipReadbackPasses (W x H x 3 host arrays, only the scene's own tiles are stored) and divides by S on the host. */
#define RT_HIP_PASS_NORMAL   8u
#define RT_HIP_PASS_ALBEDO   16u
void    *rtHipSurfaceBuffer(rtHipScene *scene);
uint64_t rtHipSurfaceBufferBytes(const rtHipScene *scene);
int      rtHipReadbackSurfacePasses(rtHipScene *scene, cl_float *normal, cl_float *albedo);

/* RAY QUERIES: what does a ray of the caller's hit in a resident scene?  The answer is the reference's grid walk,
 * RayIntersectsTriangles (raytrace_opencl.c:324-401), the routine every secondary and shadow ray of a render goes through, on the
 * scene's own grid -- bit for bit what rt_oracle_grid_trace (oracle/rt_oracle.h) returns.
 *
 * Inputs per ray: origin o and direction d (not normalised: t is measured in units of d), tmin and tmax, and an excluded triangle id
 * (0xffffffff = none; excluded == NULL: none for every ray).  Answer per ray:
 *   triangle  the triangle hit, 0xffffffff on a miss;
 *   t         on a hit the hit's t; on a miss tmax (the walk resets its running maximum to tmax in every cell);
 *   abL, acL  on a hit the hit's barycentric coordinates along ab and ac; on a miss both 0 (the reference leaves them unwritten).
 * This is the reference's walk, NOT a geometric nearest hit.  The walk visits cells from the one holding o + tmin*d (clamped into the
 * grid's box) in DDA order and ends at the first cell that holds a candidate passing the test (tmin < t < running maximum, inside the
 * triangle, not the excluded one); in that cell it keeps the smallest t, on equal t the earliest candidate in the cell's list.  A
 * triangle that spans several cells can therefore win with a hit that lies beyond that cell, over a nearer triangle of a later cell:
 * the price of agreeing with the image the renderer produces.  The walk also ends at the cell of o + tmax*d (finite tmax) and where it
 * would leave the grid.
 * Every bit pattern of the inputs has a defined answer -- NaN, +-inf, +-0, subnormals, tmin > tmax, o + tmin*d overflowing, d = 0,
 * excluded ids >= the triangle count -- and no input makes the kernel read outside the grid arrays: a point's cell is a binary search
 * over the split planes (always in [0, 255]), and each step moves one axis one cell in a direction fixed per ray, so a walk ends within
 * 3 x 256 steps.
 * Queries read only the geometry and the grid: they may be interleaved with frames on the scene's stream and change nothing those frames
 * produce.  They work on every instance (rtHipSceneCreateLike peers, partial tile sets, passes on, either pipeline). */
typedef struct rtHipRay { cl_float o[3]; cl_float tmin; cl_float d[3]; cl_float tmax; } rtHipRay; /* 32 bytes */
typedef struct rtHipHit { cl_float t; cl_uint triangle; cl_float abL; cl_float acL; } rtHipHit;     /* 16 bytes */
/* HOST arrays, synchronous.  The rays go through a staging chunk the scene owns (allocated on first use -- device and pinned host memory,
 * 52 bytes per ray of a chunk, counted by rtHipSceneBytes -- freed with the scene), one kernel launch per chunk on the scene's stream.
 * count == 0 returns 0; a NULL scene, or NULL rays / hits with count > 0, returns -1. */
int rtHipSceneIntersect(rtHipScene *scene, const rtHipRay *rays, const cl_uint *excluded, cl_uint count, rtHipHit *hits);
/* DEVICE arrays of the scene's device (rays and hits 16-byte aligned), asynchronous on `stream` (a hipStream_t as void*; NULL = the
 * scene's stream): one kernel launch, no allocation, no synchronisation.  Every pointer is checked first (hipPointerGetAttributes: device
 * memory of the scene's device, the whole range inside one allocation); anything else returns -1 with the last-error text set and
 * launches nothing.  count == 0 returns 0 and launches nothing. */
int rtHipSceneIntersectDevice(rtHipScene *scene, const void *rays, const void *excluded, cl_uint count, void *hits, void *stream);

/* DENOISER: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by the normal and albedo passes.  K iterations of a
 * 5x5 B3-spline stencil dilated by h = 2^i; a tap's weight falls off across normal, albedo and colour edges.  The arithmetic is IEEE fp32
 * + - * /, sqrt and compares only (no transcendental, no FMA, divisions and square roots correctly rounded): tests/denoise_oracle.py
 * restates it in numpy and the device output equals it bit for bit.
 *
 * Inputs: W x H pixels, row-major, 3 x f32 interleaved per pixel: colour c, normal n, albedo a.
 * Parameters: iterations K in 0..12, colourInvSigma2 ic and albedoInvSigma2 ia finite and >= 0, normalPowerLog2 E in 0..10; also
 * ic * 4^(K-1) (computed as below) must be finite.  Anything else returns -1 before anything is launched.
 * Guides, once per call, per pixel: m = (nx*nx + ny*ny) + nz*nz; if m > 0: r = sqrt(m), n^ = (nx/r, ny/r, nz/r), z = false; otherwise
 * (zero, underflow, NaN) n^ = (0,0,0), z = true.
 * Iteration i = 0..K-1 reads C^i (C^0 = c) and writes C^(i+1); h = 2^i; ic_i = ic multiplied by 4.0f i times in fp32;
 * B = {1/16, 1/4, 3/8, 1/4, 1/16}.  For pixel p = (x, y), taps j = 0..4 (rows, outer) and k = 0..4 (columns, inner) at
 * q = (x + (k-2)h, y + (j-2)h); taps outside the image are skipped.  Per tap, in this order:
 *   dc = (dr*dr + dg*dg) + db*db with d = C^i_p - C^i_q;  da = the same on the albedo;
 *   wn = 1 if z_p and z_q, else d = (n^p.x*n^q.x + n^p.y*n^q.y) + n^p.z*n^q.z, d = (d > 0 ? d : 0), d = d*d repeated E times, wn = d;
 *   w = ((B[j]*B[k]) * wn) / ((1 + dc*ic_i) * (1 + da*ia));
 *   sw += w;  s_c += w * C^i_q per component (the sums start at +0.0f and add in tap order).
 * C^(i+1)_p = s_c / sw if sw > 0, else C^i_p.  The output is C^K (K = 0 copies the colour bit for bit).
 * Non-finite inputs give unspecified values but never an access out of range. */
typedef struct rtHipDenoiseParams {
    cl_uint  iterations;      /* K */
    cl_float colourInvSigma2; /* ic */
    cl_float albedoInvSigma2; /* ia */
    cl_uint  normalPowerLog2; /* E: the normal weight is max(dot, 0)^(2^E) */
} rtHipDenoiseParams;
/* K = 4, ic = 4, ia = 100, E = 7 ("Denoiser", says why). */
void     rtHipDenoiseDefaults(rtHipDenoiseParams *params);
/* Device scratch rtHipDenoiseDevice needs for a W x H image (16-byte aligned): two float4 colour buffers and the packed guides, 64 B per
 * pixel.  0 for a size rtHipDenoiseDevice refuses. */
uint64_t rtHipDenoiseScratchBytes(cl_uint width, cl_uint height);
/* DEVICE arrays of `device`, asynchronous on `stream` (a hipStream_t of `device` as void*; NULL = the null stream): no allocation, no
 * synchronisation.  colour, normal, albedo and out hold W x H x 3 f32 (4-byte aligned), scratch at least rtHipDenoiseScratchBytes
 * (16-byte aligned).  Every pointer is checked first like rtHipSceneIntersectDevice's (device memory of `device`, the whole range inside
 * one allocation); a non-NULL stream must belong to `device` (hipStreamGetDevice); out and scratch must not overlap each other nor any
 * input; W, H >= 1 and W*H <= 2^27.  Anything else returns -1 with
 * the last-error text set and launches nothing. */
int rtHipDenoiseDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *normal, const void *albedo, void *out,
                       void *scratch, uint64_t scratchBytes, const rtHipDenoiseParams *params, void *stream);
/* HOST arrays, synchronous; device memory is allocated and freed per call.  Same checks and results as rtHipDenoiseDevice. */
int rtHipDenoise(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *normal, const cl_float *albedo,
                 cl_float *out, const rtHipDenoiseParams *params);
/* The scene's last frame, denoised on its device without a host round trip: colour = (float)u16 / 65535.0f of the beauty planes, normal
 * and albedo = sum / (float)S, exactly what rtHipReadback and rtHipReadbackSurfacePasses give.  Needs RT_HIP_PASS_NORMAL |
 * RT_HIP_PASS_ALBEDO on and a tile set that holds every tile of the image once; otherwise -1.  Synchronises and finishes the frame like
 * rtHipReadback.  Outputs (each may be NULL, host arrays): outRgb W x H x 3 f32 = C^K, and u16 planes R, G, B with v = C * 65535.0f,
 * u = !(v > 0) ? 0 : (v >= 65534.5f ? 65535 : (u16)(v + 0.5f)).  The scratch belongs to the scene: made on first use, counted in
 * rtHipSceneBytes, freed with the scene or when the surface passes go off.  The tile and surface buffers are not changed. */
int rtHipSceneDenoise(rtHipScene *scene, const rtHipDenoiseParams *params, cl_float *outRgb, cl_ushort *outR, cl_ushort *outG,
                      cl_ushort *outB);
/* Device time in milliseconds of the scene's last rtHipSceneDenoise call, from HIP events on the scene's stream: ms[0] the gather, ms[1] the
 * guide prologue, ms[2] the K iterations and the output kernel.  All 0 before the first call.  Returns 0, or -1 for a NULL argument. */
int rtHipSceneDenoiseTimes(const rtHipScene *scene, cl_float *ms);

/* AMBIENT OCCLUSION: per pixel, the fraction of cosine-weighted hemisphere rays from the primary hit that reach `radius` unoccluded,
 * traced against a resident scene with the renderer's own grid walk (the answer rtHipSceneIntersect gives for each ray).  It needs the
 * camera, geometry and grid only: no frame has to be rendered, and a call changes nothing a later frame, read-back, pass or denoise
 * produces.  The arithmetic is IEEE fp32 + - * /, sqrt and compares (no FMA, division and square root correctly rounded) plus a 64-bit
 * integer hash: tests/ao_oracle.py restates it in numpy and, with rt_oracle_grid_trace for the walks, the device output equals it bit
 * for bit.  dot(a, b) = (a0*b0 + a1*b1) + a2*b2; cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).
 *
 * Parameters: raysPerHit R in 1..256, pixelSamples Sp in 1..64, radius > 0 (+inf allowed, NaN not), seed any u32.
 * Random numbers, mod 2^64: mix(z) = splitmix64's finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 * z *= 0x94D049BB133111EB; z ^= z >> 31); S0 = mix(seed); h(c) = mix(S0 + (c + 1) * 0x9E3779B97F4A7C15); U(c) = (float)(h(c) >> 40) *
 * 2^-24.  (Seed 0: h(0), h(1), h(2) = 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, splitmix64's outputs from state 0.)
 * Counter c = (((p*Sp + j)*(R + 1) + slot)*32 + draw): pixel p = y*W + x, pixel sample j, slot 0 the jitter and slot 1 + r AO ray r.
 * Pixel sample (x, y, j): u = v = 0.5 if Sp = 1, else u = U(slot 0, draw 0), v = U(slot 0, draw 1); the ray o = eye,
 * d = (topLeft + lr*((float)x + u)) + tb*((float)y + v) per component, tmin = 0, tmax = +inf, nothing excluded.  A miss counts R
 * unoccluded rays.  A hit (triangle tri, t): P = o + t*d per component; n = cross(ac, ab) (ab = b - a, ac = c - a from the vertices);
 * n = -n if dot(n, d) > 0; m = dot(n, n); if !(m > 0) the sample counts R unoccluded rays, else n^ = n / sqrt(m) (three divisions).
 * Frame (Duff et al. 2017): s = (n^z >= 0) ? 1 : -1, a = -1 / (s + n^z), b = (n^x*n^y)*a, t1 = (1 + ((s*n^x)*n^x)*a, s*b, -(s*n^x)),
 * t2 = (b, s + (n^y*n^y)*a, -n^y).  AO ray r (Malley): for k = 0..15, xd = 2*U(slot 1+r, draw 2k) - 1, yd = 2*U(slot 1+r, draw 2k+1) - 1,
 * r2 = xd*xd + yd*yd; the first k with r2 < 1 is taken, none gives xd = yd = r2 = 0.  z = sqrt(1 - r2), dir_c = (xd*t1_c + yd*t2_c) +
 * z*n^_c; the ray o = P, d = dir, tmin = 0, tmax = radius, excluding tri, is occluded iff the walk returns a triangle.
 * Output: U = unoccluded rays over the pixel's Sp samples, value = (float)U / (float)(Sp*R), in [0, 1].  Only the pixels of the scene's
 * own tiles are written; every other pixel keeps its value, so instances over a tile deal compose one image.  Every input bit pattern
 * has a defined answer (NaN directions, degenerate triangles, the eye outside the grid's box): the walk has one.
 * The scratch (the pixel counters and one chunk of primary hits, 32 bytes per pixel sample; "ao_samples" of rtHipTune) belongs to the
 * scene: made on first use, counted in rtHipSceneBytes, freed with the scene.  Calls on different streams are ordered by an event.
 * Both calls refuse, with -1, the last-error text set and nothing launched: a NULL argument, a parameter out of range, an image of
 * 2^32 pixels or more. */
typedef struct rtHipAoParams {
    cl_uint  raysPerHit;   /* R */
    cl_uint  pixelSamples; /* Sp */
    cl_float radius;       /* tmax of the AO rays */
    cl_uint  seed;
} rtHipAoParams;
/* R = 16, Sp = 1, radius = +inf, seed = 0. */
void rtHipAoDefaults(rtHipAoParams *params);
/* HOST W x H f32, row-major; synchronous, on the scene's stream. */
int  rtHipSceneAmbientOcclusion(rtHipScene *scene, const rtHipAoParams *params, cl_float *out);
/* DEVICE W x H f32 of the scene's device (4-byte aligned), asynchronous on `stream` (a hipStream_t as void*; NULL = the scene's stream):
 * no synchronisation.  out is checked like rtHipSceneIntersectDevice's pointers (device memory of the scene's device, the whole range
 * inside one allocation); a host pointer returns -1. */
int  rtHipSceneAmbientOcclusionDevice(rtHipScene *scene, const rtHipAoParams *params, void *out, void *stream);

/* MOTION VECTORS: per pixel, where on the PREVIOUS frame's screen the surface point now seen through the pixel's centre was, and what a
 * consumer needs to reject stale history.  "Previous" is the reference state recorded by rtHipSceneMotionMark; the pass is the flow
 * input of a temporal filter (history buffers, resampling and blending: TEMPORAL ACCUMULATION below, or the consumer's own).  It reads the camera, the triangle
 * records, the grid and the reference: no frame has to be rendered, it works on either pipeline, and a call changes nothing a later
 * frame, read-back, pass, denoise, AO, bake or query produces.  The arithmetic is IEEE fp32 + - * / and compares only (no FMA, division
 * correctly rounded); dot and cross as the AMBIENT OCCLUSION block defines them.  tests/motion_oracle.py restates it in numpy and,
 * with rt_oracle_grid_trace for the walks, the device output equals it bit for bit (up to the payload of a NaN).
 *
 * Reference state: rtHipSceneMotionMark records the camera in effect (five fields) and, per triangle, a, ab = b - a, ac = c - a (per
 * component) -- exactly the fp32 values the scene's triangle records hold at that moment.  A later rtHipSceneSetCamera or
 * rtHipSceneSetGeometry does not touch the reference; a new mark replaces it.  The triangle count of a scene never changes, so triangle
 * i now is triangle i then, also after an update that re-indexes the vertices.  The reference lives in storage of its own (it does not
 * point into the geometry update's two sets): made by the first mark, 48 bytes per triangle, counted in rtHipSceneBytes from then on and
 * freed with the scene; a scene that never marks holds none of it.  The mark is one copy kernel on the scene's stream: nothing crosses
 * the bus.  Instances made by rtHipSceneCreateLike mark for themselves.
 *
 * Pixel (x, y) of the scene's own tiles: the primary ray of the AO block at Sp = 1, o = eye, d = (topLeft + lr*((float)x + 0.5f)) +
 * tb*((float)y + 0.5f) per component, tmin = 0, tmax = +inf, nothing excluded, traced with the renderer's grid walk (the answer
 * rtHipSceneIntersect gives: tri, t, abL, acL).  Primes denote the reference: E', TL', lr', tb' and a', ab', ac' of triangle tri.
 *   hit:   P' = (a' + abL*ab') + acL*ac' per component;  w = P' - E' per component.
 *   miss:  w = d (the background is a point at infinity: a rotation of the camera moves it, a translation does not).
 *   n = cross(lr', tb');  den = dot(w, n);  px = dot(TL', cross(w, tb')) / den;  py = dot(TL', cross(lr', w)) / den
 *   (Cramer's rule for TL' + lr'*px + tb'*py parallel to w).
 * Outputs: motion = (px - ((float)x + 0.5f), py - ((float)y + 0.5f)), from the pixel to the previous position, in pixels;
 *   t = the hit's t, +inf on a miss;
 *   prevT = den / dot(TL', n) on a hit, +inf on a miss: the parameter at which the reference camera's ray through (px, py) reaches P'
 *   (<= 0: the point was behind that camera);
 *   triangle = tri, 0xffffffff on a miss.
 * No special cases: den = 0, NaN cameras, degenerate triangles and points behind the eye give what the operations give (infinities,
 * NaN); every bit pattern has a defined answer up to the payload of a NaN, and nothing indexes out of range.
 * Validating history: a consumer keeps last frame's t and triangle maps, looks them up at (x + 0.5 + motion.x, y + 0.5 + motion.y) and
 * compares them with prevT and triangle ("Motion vectors (reprojection)").
 * Only the pixels of the scene's own tiles are written; every other pixel keeps its value, so instances over a tile deal compose one
 * image.  Both rtHipSceneMotion calls refuse, with -1, the last-error text set and nothing launched: a NULL scene, every output NULL,
 * no mark yet ("no motion reference"), an image of 2^32 pixels or more, a bad device pointer. */
/* Records the scene's camera and triangles as the reference.  Asynchronous, on the scene's stream.  Returns 0, -1 on failure. */
int  rtHipSceneMotionMark(rtHipScene *scene);
/* The camera the last mark recorded; -1 before the first mark. */
int  rtHipSceneMotionReferenceCamera(const rtHipScene *scene, rtHipCamera *out);
/* HOST row-major W x H arrays: motion 2 x f32 interleaved, t f32, prevT f32, triangle u32; each may be NULL, not all.  Synchronous, on
 * the scene's stream.  Its staging (20 bytes per pixel of the scene's tiles) is made on first use and counted in rtHipSceneBytes. */
int  rtHipSceneMotion(rtHipScene *scene, cl_float *motion, cl_float *t, cl_float *prevT, cl_uint *triangle);
/* DEVICE arrays of the scene's device (4-byte aligned), asynchronous on `stream` (a hipStream_t as void*; NULL = the scene's stream): no
 * allocation, no synchronisation.  The pointers are checked like rtHipSceneIntersectDevice's; the call is ordered after the mark, and a
 * later mark after it, by events. */
int  rtHipSceneMotionDevice(rtHipScene *scene, void *motion, void *t, void *prevT, void *triangle, void *stream);

/* MATTES: anti-aliased id coverage over a pixel's samples -- the object buffer of a compositor.  Per pixel, the fraction of its samples
 * whose primary hit carries a given id (SELECTED MATTES, up to 16 ids the caller names), and the K ids that cover the pixel most with
 * their fractions (RANKED LAYERS, K <= 8: any matte can be pulled afterwards without knowing the ids in advance -- the idea of
 * Cryptomatte, with raw ids instead of hashed names).  Both come from one pass over the samples and both are exact: integer counts,
 * one fp32 division each.  The samples are the beauty's, so a matte's edge is anti-aliased exactly like the frame it cuts.  The pass
 * reads the camera, the camera lists, the triangle records, the shading rows' material word and the group table: no frame has to be
 * rendered, it works on either pipeline and with passes on or off, and a call changes nothing a later frame, read-back, pass, denoise,
 * AO, bake, query or motion call produces; it leaves the sample window and the tile buffer alone.  (The TRIANGLE pass of rtHipScenePasses
 * stays what it is: sample 1's id, one per pixel.)  tests/matte_oracle.py restates the definition in numpy and the device output equals
 * it bit for bit.
 *
 * Samples: pixel p = y*W + x of the scene's own tiles; sample j = 0..C-1 has sample id i = f + 1 + j; its generator is seeded
 * (uint64)p*N + i; its direction is (topLeft + lr*((float)x + r1)) + tb*((float)y + r2) per component, r1 and r2 the next two rand01
 * draws (LR first); the pixel's camera list is scanned in order from the eye with tmin = 0, tmax = +inf and a running closest hit, ties
 * keep the earlier candidate.  This is a frame's primary ray under the sample window {N, f, ...} (SAMPLE WINDOWS above), bit for bit:
 * with N = C = S, f = 0 the samples are the default frame's, with {N, 0, N} those of a whole progressive sequence.  C need not equal
 * the scene's S: no path state is involved.
 * The sample's id g_j: 0xffffffff (NONE) on a miss; on a hit of triangle tri,
 *   RT_HIP_MATTE_TRIANGLE (0)  tri;
 *   RT_HIP_MATTE_MATERIAL (1)  the resident material id (what rtHipSceneSetMaterials edits); every negative id reads as NONE;
 *   RT_HIP_MATTE_GROUP    (2)  groups[tri] of the scene's group table (rtHipSceneSetMatteGroups): any u32, 0xffffffff = "in no group".
 * Selected mattes: count_m = the number of j with g_j == select[m], m < M <= 16.  A repeated id gives equal planes; NONE is refused.
 * Layers: a table of K <= 8 slots, empty at j = 0.  The samples are taken in order j = 0..C-1; one with g_j == NONE is skipped; if g_j
 * is in the table its slot's count goes up by one; otherwise, if a slot is free, the first free slot takes (g_j, 1); otherwise `rest`
 * goes up by one.  After the last sample the used slots are ordered by count descending, equal counts by id ascending; unused slots
 * follow with id NONE and count 0.  So with K >= the number of distinct ids in the pixel the layers are exact and rest = 0; with a
 * smaller K the FIRST K distinct ids in sample order are the ones kept (not the K largest), and rest counts every sample of the others.
 * Always: the layer counts + rest + the NONE samples = C.
 * Outputs, each row-major W x H and plane-major where there are several planes:
 *   select        f32 [M][H][W] = (float)count_m / (float)C
 *   layerId       u32 [K][H][W]
 *   layerCoverage f32 [K][H][W] = (float)count / (float)C
 *   rest          f32 [H][W]    = (float)rest / (float)C
 * Each may be NULL; not all of them, not select with M = 0, not a layer output with K = 0.  Only the pixels of the scene's own tiles are
 * written; every other pixel keeps its value, so instances over a tile deal compose one image.  Every bit pattern of camera, vertices
 * and table has a defined answer, and nothing indexes out of range.
 * Parameters: rtHipMatteCheck (host only, no device) returns -1 with the last-error text set for a kind outside 0..2, N == 0, C == 0 or
 * C > 65536, f + C > N (compared in 64 bits), M > 16, K > 8, M == 0 && K == 0, a selected id of NONE; 0 otherwise.
 * The scratch (M + 2K + 1 words per pixel of the scene's tiles: the state between the launches of a call, each of which walks at most
 * "matte_chunk" samples, rtHipTune) belongs to the scene: made on first use, grown when M + 2K + 1 grows, counted in rtHipSceneBytes,
 * freed with the scene; a scene that never asks holds none of it.  Calls on different streams are ordered by an event.
 * Both rtHipSceneMattes calls refuse, with -1, the last-error text set and nothing launched: a NULL scene or params, a failed check,
 * the output rules above, kind GROUP without a table, an image of 2^32 pixels or more, a bad device pointer. */
#define RT_HIP_MATTE_TRIANGLE 0
#define RT_HIP_MATTE_MATERIAL 1
#define RT_HIP_MATTE_GROUP 2
#define RT_HIP_MATTE_NONE 0xffffffffu
#define RT_HIP_MATTE_MAX_SELECT 16
#define RT_HIP_MATTE_MAX_LAYERS 8
typedef struct rtHipMatteParams {
    cl_uint kind;        /* RT_HIP_MATTE_* */
    cl_uint total;       /* N */
    cl_uint first;       /* f */
    cl_uint samples;     /* C */
    cl_uint selectCount; /* M */
    cl_uint select[RT_HIP_MATTE_MAX_SELECT];
    cl_uint layers;      /* K */
} rtHipMatteParams;
int  rtHipMatteCheck(const rtHipMatteParams *params);
/* kind TRIANGLE, M = 0, K = 4 and {N, f, C} = {total, first, S} of the window the scene's last issued frame used (*last of
 * rtHipSceneGetSampleWindow), {S, 0, S} before the first frame.  Returns 0, or -1 for a NULL argument. */
int  rtHipMatteDefaults(const rtHipScene *scene, rtHipMatteParams *params);
/* The group table of kind GROUP: T ids (T = the scene's triangle count, which never changes), from host memory or -- onDevice -- from
 * memory of the scene's device, checked like rtHipSceneIntersectDevice's pointers.  The ids are copied into storage the scene owns
 * (counted in rtHipSceneBytes, freed with the scene), so the table survives rtHipSceneSetCamera, rtHipSceneSetGeometry,
 * rtHipSceneSetLights and rtHipSceneSetMaterials.  NULL frees the table.  Synchronous, on the scene's stream.  Returns 0, -1 on failure. */
int  rtHipSceneSetMatteGroups(rtHipScene *scene, const cl_uint *groups, cl_int onDevice);
/* HOST arrays; synchronous, on the scene's stream. */
int  rtHipSceneMattes(rtHipScene *scene, const rtHipMatteParams *params, cl_float *select, cl_uint *layerId, cl_float *layerCoverage,
                      cl_float *rest);
/* DEVICE arrays of the scene's device (4-byte aligned), asynchronous on `stream` (a hipStream_t as void*; NULL = the scene's stream): no
 * synchronisation, and no allocation when the scratch already fits.  The pointers are checked like rtHipSceneAmbientOcclusionDevice's. */
int  rtHipSceneMattesDevice(rtHipScene *scene, const rtHipMatteParams *params, void *select, void *layerId, void *layerCoverage, void *rest,
                            void *stream);
/* Device time in milliseconds of the scene's last matte call, from HIP events on its stream: ms[0] the count launches, ms[1] the finish
 * kernel.  Waits for that call to end.  Both 0 before the first call.  Returns 0, or -1 for a NULL argument. */
int  rtHipSceneMatteTimes(rtHipScene *scene, double ms[2]);

/* TEMPORAL ACCUMULATION: the consumer of the motion vectors.  The previous call's output (the history) is fetched bilinearly where the
 * flow says each pixel's surface point was, every tap validated against the triangle id and prevT, and blended with the new frame as a
 * running mean of at most maxHistory frames; a pixel without valid history starts again from the frame itself.  The arithmetic is IEEE
 * fp32 + - * /, floorf, fabsf and compares in a fixed order (no FMA, divisions correctly rounded): tests/temporal_oracle.py restates it
 * in numpy and the device output equals it bit for bit (up to the payload of a NaN).
 *
 * All arrays are W x H, row-major; W, H >= 1, W, H <= 16384 (so (float)W and the pixel coordinates are exact) and W*H <= 2^27.
 * Current frame: colour 3 x f32, motion 2 x f32, prevT f32, triangle u32 -- the last three exactly what rtHipSceneMotion writes.
 * History (the previous call's outputs and guides): histColour 3 x f32, histCount f32 (the history length; 0 = none), histT f32 (the
 * previous frame's t map), histTriangle u32.  Outputs: outColour 3 x f32, outCount f32.
 * Parameters: maxHistory finite in [1, 65536], depthTolerance finite and >= 0; anything else returns -1 before anything is launched.
 * Per pixel p = (x, y):
 *   gx = (((float)x + 0.5f) + motion.x) - 0.5f;  gy likewise with y
 *   ok = prevT > 0 && gx >= -1.0f && gx < (float)W && gy >= -1.0f && gy < (float)H            (a NaN compares false)
 *   if ok: x0f = floorf(gx), y0f = floorf(gy), ax = gx - x0f, ay = gy - y0f, x0 = (int)x0f, y0 = (int)y0f (converted only after the
 *     range test: x0 in [-1, W-1]); sw = sr = sg = sb = sn = +0.0f; for j = 0..1 (rows, outer), k = 0..1 (columns, inner):
 *       q = (x0 + k, y0 + j); a tap outside the image is skipped;
 *       b = (k ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
 *       accepted iff histCount_q >= 1.0f && histTriangle_q == triangle_p
 *                    && (histT_q == prevT || fabsf(histT_q - prevT) <= depthTolerance * prevT);
 *       accepted: sw += b;  sr += b * histColour_q.r (g, b alike);  sn += b * histCount_q
 *   if ok && sw > 0: hc = (sr/sw, sg/sw, sb/sw), hn = sn/sw;  n = hn + 1.0f;  if (n > maxHistory) n = maxHistory;  a = 1.0f / n;
 *     outColour = hc + (colour - hc) * a per component (a subtract, a multiply, an add), but colour itself if n == 1.0f;  outCount = n
 *     (n == 1 happens only with maxHistory = 1, which so returns the frame bit for bit: hc + (colour - hc) rounds twice and need not)
 *   else: outColour = colour;  outCount = 1.0f
 * The == arm lets a missed pixel (prevT = +inf, triangle 0xffffffff) accept a missed history pixel (t = +inf): the background accumulates
 * under a pure rotation and starts again wherever the flow points at geometry.  Every bit pattern of the inputs has a defined answer up to
 * the payload of a NaN, and no index is formed before its range test.  The outputs must not overlap any input nor each other: a history
 * tap belongs to a neighbour, so the filter cannot run in place. */
typedef struct rtHipTemporalParams {
    cl_float maxHistory;     /* the running mean's longest length, in frames */
    cl_float depthTolerance; /* relative: |histT - prevT| <= depthTolerance * prevT */
} rtHipTemporalParams;
/* maxHistory = 32, depthTolerance = 0.05 ("a few per cent: the stored value belongs to the nearest pixel centre"); defaults of a
 * parameter, not measurements. */
void rtHipTemporalDefaults(rtHipTemporalParams *params);
/* DEVICE arrays of `device`, asynchronous on `stream` (a hipStream_t of `device` as void*; NULL = the null stream): one launch, no
 * allocation, no synchronisation.  outCount may be NULL.  Every pointer is checked first like rtHipDenoiseDevice's (device memory of
 * `device`, the whole range inside one allocation, 4-byte aligned); a non-NULL stream must belong to `device`; outColour and outCount must
 * overlap nothing.  Anything else returns -1 with the last-error text set and launches nothing. */
int  rtHipTemporalDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *prevT,
                         const void *triangle, const void *histColour, const void *histCount, const void *histT, const void *histTriangle,
                         void *outColour, void *outCount, const rtHipTemporalParams *params, void *stream);
/* HOST arrays, synchronous; device memory is allocated and freed per call.  outCount may be NULL.  Same results as rtHipTemporalDevice. */
int  rtHipTemporal(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *prevT,
                   const cl_uint *triangle, const cl_float *histColour, const cl_float *histCount, const cl_float *histT,
                   const cl_uint *histTriangle, cl_float *outColour, cl_float *outCount, const rtHipTemporalParams *params);
/* The scene's last frame, accumulated on its device against the history the scene keeps.  The caller's loop is: rtHipSceneSetCamera and
 * / or rtHipSceneSetGeometry, render, rtHipSceneTemporal.  The call needs a tile set that holds every tile of the image once (as
 * rtHipSceneDenoise does), synchronises and finishes the frame like rtHipReadback, and then, on the scene's stream: marks the scene if
 * it has no motion reference yet; runs the motion pass into storage of its own; gathers the colour ((float)u16 / 65535.0f of the beauty
 * planes, what rtHipReadback gives); accumulates against the history; makes outColour, outCount and this frame's t and triangle maps the
 * new history; and marks the scene again, so that the reference becomes the state this frame was rendered from.  THE CALL OWNS THE
 * MARK: a later rtHipSceneMotion of the caller measures against this frame, and a mark of the caller between two calls changes what
 * the next call reprojects against.
 * denoise non-NULL (temporal, then spatial): needs RT_HIP_PASS_NORMAL | RT_HIP_PASS_ALBEDO on; the accumulated colour goes through the
 * DENOISER with the gathered normal and albedo (exactly rtHipSceneDenoise's) before it is output, in the scratch rtHipSceneDenoise uses.
 * The history keeps the unfiltered accumulation.
 * Outputs (each may be NULL, host arrays): outRgb W x H x 3 f32, the u16 planes R, G, B quantised as rtHipSceneDenoise's, outCount W x H
 * f32 (the history length each pixel now has).
 * Storage, made on first use in one block, counted in rtHipSceneBytes from then on and freed with the scene (a scene that never calls
 * holds none of it), with n = W*H and every part rounded up to 256 bytes: two history sets of colour 12n, count 4n, t 4n and triangle 4n
 * (24 B per pixel each); motion 8n and prevT 4n (this frame's t and triangle are written straight into the new history set, so the pass
 * keeps 12 B per pixel of its own); the gathered colour 12n; and the u16 output planes 3 x 2n.  A call with denoise non-NULL also
 * needs the scene's denoiser scratch (rtHipSceneDenoise's: 4 images of 12n, 3 planes of 2n, each rounded up to 256 bytes, plus
 * rtHipDenoiseScratchBytes): if no rtHipSceneDenoise has made it yet, that call makes it, and rtHipSceneBytes grows by it as well.
 * If a step fails after the accumulation was issued, the history is dropped: the next call starts again, as after a reset.
 * Refused with -1, the last-error text set and nothing launched: a NULL scene or params, parameters out of range, an image wider or
 * higher than 16384 or of more than 2^27 pixels, a tile subset, denoise without both surface passes. */
int  rtHipSceneTemporal(rtHipScene *scene, const rtHipTemporalParams *params, const rtHipDenoiseParams *denoise, cl_float *outRgb,
                        cl_ushort *outR, cl_ushort *outG, cl_ushort *outB, cl_float *outCount);
/* Sets the scene's history to "none": the next rtHipSceneTemporal outputs the frame itself with count 1.  Returns 0, -1 for NULL. */
int  rtHipSceneTemporalReset(rtHipScene *scene);
/* Device time in milliseconds of the scene's last rtHipSceneTemporal call, from HIP events on the scene's stream: ms[0] the motion pass,
 * ms[1] the colour gather (with denoise: the gather of colour, normal and albedo), ms[2] the accumulation, ms[3] the filter (if any) and
 * the output kernel.  All 0 before the first call.  Returns 0, or -1 for a NULL argument. */
int  rtHipSceneTemporalTimes(const rtHipScene *scene, cl_float ms[4]);

/* VARIANCE-GUIDED FILTER: the denoising chain's knowledge of how noisy each pixel still is (Schied et al. 2017, "SVGF").  (a) The first
 * two moments of the luminance are accumulated along TEMPORAL ACCUMULATION's reprojection; (b) a per-pixel variance is estimated from
 * them, spatially where the history is too short to tell; (c) an a-trous filter like the DENOISER runs with a luminance edge-stop scaled
 * by the local variance, and carries the variance through its iterations.  The arithmetic is IEEE fp32 + - * /, floorf, fabsf, sqrt
 * (guides only) and compares in a fixed order (no FMA, divisions correctly rounded): tests/variance_oracle.py restates it in numpy and the
 * device output equals it bit for bit (up to the payload of a NaN).
 *
 * lum(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b.  The guides n^ and z, the normal weight wn (with E) and the albedo distance da are
 * exactly the DENOISER block's; B = {1/16, 1/4, 3/8, 1/4, 1/16}.
 *
 * (a) Moments accumulation.  Inputs and per-pixel work as TEMPORAL ACCUMULATION, unchanged: outColour and outCount are bit-identical to
 * rtHipTemporal's for the same inputs.  In addition histMoments and outMoments, 2 x f32 per pixel (the means of lum and of lum*lum), and
 * outVariance f32:
 *   l = lum(colour_p), l2 = l*l;  s1 = s2 = +0.0f;  in the tap loop, for an accepted tap: s1 += b * histMoments_q[0];  s2 += b * histMoments_q[1]
 *   if ok && sw > 0: h1 = s1/sw, h2 = s2/sw;  if n != 1.0f: m1 = h1 + (l - h1)*a, m2 = h2 + (l2 - h2)*a;  if n == 1.0f: m1 = l, m2 = l2
 *   else: m1 = l, m2 = l2
 *   outMoments = (m1, m2);  v = m2 - m1*m1;  outVariance = (v > 0 ? v : 0)                       (a NaN gives 0)
 *
 * (b) Variance estimate V^0, from moments 2 x f32 and count f32 (the history length).  With both NULL: moments = (lum(c), lum(c)*lum(c))
 * and count = 1 in every pixel, the single-frame use.
 *   if count_p >= spatialBelow: V^0 = (v > 0 ? v : 0) with v = m2 - m1*m1
 *   otherwise (a NaN count too): a 7x7 window at spacing 1, dy = -3..3 (rows, outer), dx = -3..3 (columns, inner), q = (x + dx, y + dy);
 *     taps outside the image are skipped; sw = s1 = s2 = +0.0f;  per tap: w = wn / (1 + da*ia);  sw += w;  s1 += w*m1_q;  s2 += w*m2_q
 *     if sw > 0: M1 = s1/sw, M2 = s2/sw, v = M2 - M1*M1, v = (v > 0 ? v : 0), V^0 = v * (count_p >= 1.0f ? 4.0f/count_p : 4.0f)
 *     else: V^0 = 0
 *
 * (c) Iteration i = 0..K-1 reads the state (C^i, V^i) (C^0 = c) and writes (C^(i+1), V^(i+1)); h = 2^i.  Per pixel p = (x, y):
 *   G = {1/4, 1/2, 1/4};  gs = gw = +0.0f;  for j = 0..2 (rows, outer), k = 0..2 (columns, inner), q = (x + k-1, y + j-1), taps outside
 *     the image skipped: gs += (G[j]*G[k]) * V^i_q;  gw += G[j]*G[k]
 *   g = gs/gw;  il = 1.0f / (ls*g + floor)
 *   the 25 taps of the DENOISER block at spacing h, same order, same skipping; sw = s_c = sv = +0.0f; per tap:
 *     dl = lum(C^i_p) - lum(C^i_q)
 *     w = ((B[j]*B[k]) * wn) / ((1 + (dl*dl)*il) * (1 + da*ia))
 *     sw += w;  s_c += w * C^i_q per component;  sv += (w*w) * V^i_q
 *   if sw > 0: C^(i+1)_p = s_c/sw, V^(i+1)_p = sv / (sw*sw);  otherwise both are kept.
 * There is no sigma schedule: the variance shrinks by itself, and the edge-stop with it.  Outputs: C^K and, optionally, V^K.
 *
 * Parameters: iterations K in 0..12; luminanceSigma2 ls finite and >= 0; varianceFloor finite and >= 2^-100; albedoInvSigma2 ia and
 * normalPowerLog2 E as the DENOISER block's; spatialBelow finite and in [0, 65537].  Anything else returns -1 before anything is
 * launched.  Every bit pattern of the inputs has a defined answer up to the payload of a NaN (an infinite variance next to a zero weight
 * is a NaN by 0 * inf, and spreads), and nothing indexes out of range.
 *
 * Fresh samples per frame: under the default sample window every frame of a still scene is the same frame and the temporal variance is
 * 0.  Give the scene a sequence window (SAMPLE WINDOWS above: {N, 0, S, 0, 1}) and successive frames draw different samples. */
typedef struct rtHipVarianceParams {
    cl_uint  iterations;      /* K */
    cl_float luminanceSigma2; /* ls: the luminance edge-stop is (dl*dl) / (ls * variance + floor) */
    cl_float varianceFloor;   /* floor */
    cl_float albedoInvSigma2; /* ia */
    cl_uint  normalPowerLog2; /* E */
    cl_float spatialBelow;    /* pixels whose history is shorter than this take the 7x7 spatial estimate */
} rtHipVarianceParams;
/* K = 4, ls = 4, floor = 1e-8f, ia = 100, E = 7, spatialBelow = 4 ("Variance-guided filter", says why). */
void     rtHipVarianceDefaults(rtHipVarianceParams *params);
/* (a) on DEVICE arrays: rtHipTemporalDevice plus histMoments (input), outMoments and outVariance (outputs; outCount and outVariance may
 * be NULL).  Same checks: every pointer, overlap (no output may overlap anything else), stream and size as rtHipTemporalDevice; a
 * refusal launches nothing.  One launch. */
int  rtHipTemporalMomentsDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *prevT,
                                const void *triangle, const void *histColour, const void *histCount, const void *histT,
                                const void *histTriangle, const void *histMoments, void *outColour, void *outCount, void *outMoments,
                                void *outVariance, const rtHipTemporalParams *params, void *stream);
/* HOST arrays, synchronous; outCount and outVariance may be NULL.  Same results as rtHipTemporalMomentsDevice. */
int  rtHipTemporalMoments(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *prevT,
                          const cl_uint *triangle, const cl_float *histColour, const cl_float *histCount, const cl_float *histT,
                          const cl_uint *histTriangle, const cl_float *histMoments, cl_float *outColour, cl_float *outCount,
                          cl_float *outMoments, cl_float *outVariance, const rtHipTemporalParams *params);
/* Device scratch rtHipDenoiseVarianceDevice needs for a W x H image (16-byte aligned): two float4 states, the packed guides and il,
 * 68 B per pixel.  0 for a size it refuses. */
uint64_t rtHipVarianceScratchBytes(cl_uint width, cl_uint height);
/* (b) and (c) on DEVICE arrays of `device`, asynchronous on `stream`: no allocation, no synchronisation.  colour, normal, albedo and out
 * W x H x 3 f32, moments W x H x 2 f32 and count W x H f32 (both NULL or both given), outVariance W x H f32 (V^K; may be NULL), scratch at
 * least rtHipVarianceScratchBytes.  Checked exactly as rtHipDenoiseDevice checks: pointers, alignment (4 bytes, scratch 16), stream, W*H
 * <= 2^27; out, outVariance and scratch must overlap nothing.  Anything else returns -1 with the last-error text set and launches
 * nothing. */
int  rtHipDenoiseVarianceDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *normal, const void *albedo,
                                const void *moments, const void *count, void *out, void *outVariance, void *scratch, uint64_t scratchBytes,
                                const rtHipVarianceParams *params, void *stream);
/* HOST arrays, synchronous; device memory is allocated and freed per call.  Same checks and results as rtHipDenoiseVarianceDevice. */
int  rtHipDenoiseVariance(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *normal, const cl_float *albedo,
                          const cl_float *moments, const cl_float *count, cl_float *out, cl_float *outVariance,
                          const rtHipVarianceParams *params);
/* rtHipSceneTemporal with the moments carried along: the same sequence, the same ownership of the mark, the same outputs and the same
 * four timing slots of rtHipSceneTemporalTimes (the estimate and the filter go into ms[3]), with (a) in place of the accumulation.
 * variance NULL: no filter; outRgb and the planes are the accumulation and outVariance is (a)'s variance.  variance non-NULL: needs
 * RT_HIP_PASS_NORMAL | RT_HIP_PASS_ALBEDO on; the accumulated colour, the new moments and the new counts go through (b) and (c) with the
 * gathered normal and albedo, in the scratch rtHipSceneDenoise uses (made by this call if need be, and counted then); outRgb and the
 * planes are C^K and outVariance is V^K.  The history keeps the unfiltered accumulation and its moments.  outVariance W x H f32, host,
 * may be NULL like every other output.
 * Storage: the moments history shares colour, count, t and triangle with rtHipSceneTemporal's; it adds, in one block made on the first
 * call, counted in rtHipSceneBytes from then on and freed with the scene, with n = W*H and every part rounded up to 256 bytes: two sets
 * of moments 8n, the variance plane 4n and the filter's il plane 4n.
 * Mixing: rtHipSceneTemporal does not write moments, so a call to it leaves them stale.  An rtHipSceneTemporalVariance that finds a live
 * history with stale moments starts the history again, as after rtHipSceneTemporalReset; rtHipSceneTemporal after this call goes on
 * with the history this call left.  Refusals as rtHipSceneTemporal's, with the variance parameters and "a filter without both surface
 * passes" in place of the denoiser's. */
int  rtHipSceneTemporalVariance(rtHipScene *scene, const rtHipTemporalParams *params, const rtHipVarianceParams *variance, cl_float *outRgb,
                                cl_ushort *outR, cl_ushort *outG, cl_ushort *outB, cl_float *outCount, cl_float *outVariance);

/* TEMPORAL CLAMP: neighbourhood clamping of the reprojected history.  TEMPORAL ACCUMULATION accepts a history tap on geometry alone
 * (triangle id and prevT), so history that no longer agrees with the frame -- after rtHipSceneSetLights or rtHipSceneSetMaterials every
 * pixel's geometry is unchanged and every tap is accepted -- drags through up to maxHistory frames.  Here the history colour is pulled
 * into the colour box of the current frame's 3x3 neighbourhood before the blend: the box is the neighbourhood's min / max, or
 * mean +- gamma * sigma (Salvi's variance clipping), or the intersection of the two.  History that lies inside the box is untouched.  The
 * arithmetic is IEEE fp32 + - * /, sqrtf and compares in a fixed order (no FMA, division and square root correctly rounded):
 * tests/temporal_clamp_oracle.py restates it in numpy and the device output equals it bit for bit (up to the payload of a NaN).
 *
 * Parameters: mode in {1, 2, 3}, gamma finite and >= 0; anything else returns -1 before anything is launched.
 * Per pixel p = (x, y) and channel c of the current frame's colour: the taps dy = -1..1 (rows, outer), dx = -1..1 (columns, inner),
 * q = (x + dx, y + dy); taps outside the image are skipped.
 *   cnt = the number of taps inside the image as a float (1, 2, 3, 4, 6 or 9; it follows from x, y, W and H alone)
 *   s1 = s2 = +0.0f, mn = +inf, mx = -inf;  per tap, v = colour_q[c]:  s1 = s1 + v;  s2 = s2 + v*v;  if (v < mn) mn = v;  if (v > mx) mx = v
 *   mu = s1/cnt, ex2 = s2/cnt, var = ex2 - mu*mu, var = (var > 0 ? var : 0), e = gamma * sqrtf(var)
 *   mode 1: lo = mn, hi = mx;   mode 2: lo = mu - e, hi = mu + e;
 *   mode 3: lo = (mu - e > mn ? mu - e : mn), hi = (mu + e < mx ? mu + e : mx)
 * The rest of the pixel is TEMPORAL ACCUMULATION's, word for word -- gx, gy, ok, the four taps, sw, hc = s/sw, hn, n, a -- with one
 * insertion: when ok && sw > 0 && n != 1.0f, per channel, before the blend:
 *   h = hc[c];  if (h < lo) h = lo;  if (h > hi) h = hi
 * and the blend uses h in place of hc[c]: outColour[c] = h + (colour[c] - h) * a.  outCount is not changed by the clamp.  A constant
 * neighbourhood makes the box a point, so the output is then the frame itself.  Every bit pattern of the inputs has a defined answer up
 * to the payload of a NaN -- the compares above define it, in this order: a NaN history colour passes both and stays a NaN; a NaN in
 * the neighbourhood is skipped by mn and mx and makes mu a NaN (and var 0), so that mode 2's edges are NaN and compare false (no clamp)
 * and mode 3's are mn and mx.
 * With moments (the *MomentsClamp* calls and rtHipSceneTemporalVariance under a clamp): the two luminance moments accumulate exactly as
 * in VARIANCE-GUIDED FILTER (a), from the unclamped taps.  They are NOT clamped: a pixel whose colour was pulled shows a large temporal
 * variance for a few frames, which is what the variance-guided filter should see there (it widens the luminance edge-stop and the pixel
 * is filtered spatially while its history is wrong).
 * Out of scope: clamping the moments, shortening the count on a clamp, larger neighbourhoods, YCoCg. */
#define RT_HIP_CLAMP_MINMAX   1u
#define RT_HIP_CLAMP_VARIANCE 2u /* both bits: the intersection */
typedef struct rtHipTemporalClampParams {
    cl_uint  mode;  /* RT_HIP_CLAMP_MINMAX, RT_HIP_CLAMP_VARIANCE or both */
    cl_float gamma; /* the half-width of the variance box, in standard deviations */
} rtHipTemporalClampParams;
/* mode = 3, gamma = 1.0f: a parameter's default, not a measurement. */
void rtHipTemporalClampDefaults(rtHipTemporalClampParams *params);
/* 0 for legal parameters, -1 (the last-error text set) for NULL, a mode outside {1, 2, 3}, a gamma that is NaN, infinite or negative.
 * Needs no device. */
int  rtHipTemporalClampCheck(const rtHipTemporalClampParams *params);
/* rtHipTemporalDevice / rtHipTemporal with the clamp: the same arrays, the same pointer, overlap, stream and size checks, one launch;
 * a refusal launches nothing.  clamp NULL is a refusal: the unclamped call exists for that. */
int  rtHipTemporalClampDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *prevT,
                              const void *triangle, const void *histColour, const void *histCount, const void *histT,
                              const void *histTriangle, void *outColour, void *outCount, const rtHipTemporalParams *params,
                              const rtHipTemporalClampParams *clamp, void *stream);
int  rtHipTemporalClamp(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *prevT,
                        const cl_uint *triangle, const cl_float *histColour, const cl_float *histCount, const cl_float *histT,
                        const cl_uint *histTriangle, cl_float *outColour, cl_float *outCount, const rtHipTemporalParams *params,
                        const rtHipTemporalClampParams *clamp);
/* rtHipTemporalMomentsDevice / rtHipTemporalMoments with the clamp, likewise. */
int  rtHipTemporalMomentsClampDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *prevT,
                                     const void *triangle, const void *histColour, const void *histCount, const void *histT,
                                     const void *histTriangle, const void *histMoments, void *outColour, void *outCount, void *outMoments,
                                     void *outVariance, const rtHipTemporalParams *params, const rtHipTemporalClampParams *clamp,
                                     void *stream);
int  rtHipTemporalMomentsClamp(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion,
                               const cl_float *prevT, const cl_uint *triangle, const cl_float *histColour, const cl_float *histCount,
                               const cl_float *histT, const cl_uint *histTriangle, const cl_float *histMoments, cl_float *outColour,
                               cl_float *outCount, cl_float *outMoments, cl_float *outVariance, const rtHipTemporalParams *params,
                               const rtHipTemporalClampParams *clamp);
/* The scene's clamp: clamp non-NULL turns it on with these parameters, NULL turns it off (the default).  While it is on, the
 * accumulation step of rtHipSceneTemporal and of rtHipSceneTemporalVariance runs the clamped kernel on the gathered colour (ms[2] of
 * rtHipSceneTemporalTimes stays "the accumulation"); while it is off both calls issue exactly the launches they issue without this
 * block.  The setting is per scene and touches neither the history, the mark nor any buffer, and needs no storage.  Returns 0, or -1
 * for a NULL scene or parameters rtHipTemporalClampCheck refuses (the setting then stays what it was). */
int  rtHipSceneSetTemporalClamp(rtHipScene *scene, const rtHipTemporalClampParams *clamp);
/* 1 and *out = the parameters if the scene's clamp is on, 0 and *out zeroed if it is off, -1 for a NULL argument. */
int  rtHipSceneGetTemporalClamp(const rtHipScene *scene, rtHipTemporalClampParams *out);

/* MOTION BLUR: the other consumer of the motion vectors, the "vector motion blur" post effect.  A frame is blurred along its flow after
 * it was rendered: every pixel gathers `taps` samples along the dominant velocity of its neighbourhood, weighted by whether the sampled
 * pixel's own streak, or this pixel's, reaches the other and by which of the two is in front (McGuire, Hennessy, Bukowski and Osman
 * 2012, "A Reconstruction Filter for Plausible Motion Blur": the per-tile dominant velocity, its neighbourhood maximum, a depth-aware
 * gather).  The frame kernels are not involved: the camera's candidate lists belong to one instant.  The arithmetic is IEEE fp32
 * + - * /, sqrtf, fabsf and compares in the order written (no FMA, division and square root correctly rounded):
 * tests/motion_blur_oracle.py restates it in numpy and the device output equals it bit for bit (up to the payload of a NaN).  Every bit
 * pattern of the inputs has a defined answer up to the payload of a NaN, and no index is formed before its range test.
 *
 * All arrays are W x H, row-major; W, H and W*H limited as in TEMPORAL ACCUMULATION.  Inputs: colour 3 x f32; motion 2 x f32, exactly
 * what rtHipSceneMotion writes (from the pixel to its previous position, in pixels); depth f32, the motion pass's t (+inf on a miss).
 * Output: out 3 x f32; it must overlap no input (the taps belong to neighbours).
 * Parameters: shutter finite in [0, 4] (the share of the frame interval the exposure covers, centred on the frame); maxBlur finite in
 * [1, 32] pixels (the cap of a streak's half-extent); taps in [1, 64]; depthSoftness finite and >= 0 (relative).  Anything else returns
 * -1 before anything is launched.
 *   clamp01(r) = !(r > 0) ? 0 : (r > 1 ? 1 : r)                                                              (a NaN gives 0)
 * (a) Velocity of pixel q:
 *   s = shutter * 0.5f;  vx = motion.x * s;  vy = motion.y * s;  l2 = vx*vx + vy*vy
 *   if (!(l2 < +inf)) { vx = vy = 0; l = 0; } else l = sqrtf(l2)
 *   if (l > maxBlur) { k = maxBlur / l;  vx = vx * k;  vy = vy * k;  l = maxBlur; }
 * (b) Tile maximum.  Tiles are 32 x 32 pixels, tile(x, y) = (x >> 5, y >> 5).  tileMax[T] starts as (0, 0, 0) and is replaced by a pixel's
 *   (vx, vy, l) only when that pixel's l is strictly greater, the tile's pixels visited in row-major order: the greatest l, and among
 *   equals the smallest index (which is how a parallel reduction states it, so that the answer does not depend on its order).
 * (c) Neighbourhood maximum.  nbMax[T] likewise over the tiles (Tx + dx, Ty + dy) that exist, dy = -1..1 outer, dx = -1..1 inner, from
 *   (0, 0, 0), a candidate replacing only when strictly greater.
 * (d) Gather at p = (x, y), with (nx, ny, nl) = nbMax[tile(p)]:
 *   if (!(nl >= 0.5f)): out = colour_p, a copy, bit for bit.  Otherwise:
 *   lp = l_p < 0.5f ? 0.5f : l_p;  zp = depth_p;  wsum = 1.0f / lp;  sum = colour_p * wsum (per channel)
 *   j = ((x & 1) * 2 + (y & 1) * 3) & 3;  jit = ((float)j - 1.5f) * 0.25f                (a fixed 2 x 2 dither: no random state)
 *   for i = 0 .. taps-1:
 *     u = (((float)i + 0.5f) + jit) / (float)taps;  sg = u * 2.0f - 1.0f
 *     X = ((float)x + 0.5f) + nx * sg;  Y likewise with y and ny
 *     the tap is skipped unless X >= 0 && X < (float)W && Y >= 0 && Y < (float)H; then q = ((int)X, (int)Y)
 *     d = fabsf(sg) * nl;  lq = l_q < 0.5f ? 0.5f : l_q;  zq = depth_q;  e = depthSoftness * (zp < zq ? zp : zq)
 *     sdc(a, b) = (a == b) ? 1.0f : clamp01(1.0f - (a - b) / e);   f = sdc(zq, zp)  (q lies in front of p);   bk = sdc(zp, zq)
 *     cone(l) = clamp01(1.0f - d / l)
 *     cyl(l) = 1.0f - sm(clamp01((d - 0.95f*l) / (1.05f*l - 0.95f*l))),  sm(r) = (r*r) * (3.0f - 2.0f*r)
 *     w = (f * cone(lq) + bk * cone(lp)) + (cyl(lq) * cyl(lp)) * 2.0f
 *     wsum += w;  sum += colour_q * w (per channel: a multiply, an add)
 *   out = sum / wsum per channel
 * The == arm lets two missed pixels (both at +inf) count as one layer, as TEMPORAL ACCUMULATION's == arm does.  A tap that lands on p
 * itself is not special.  wsum starts positive and no weight is negative or a NaN, so out is a NaN only where a colour it sums is.
 * Not done: samples distributed over the shutter inside the frame kernels, sub-pixel reprojection, tile-dealt instances (their taps
 * cross tile borders: the array entry points take a composed image). */
typedef struct rtHipMotionBlurParams {
    cl_float shutter;       /* the exposure's share of the frame interval, centred on the frame */
    cl_float maxBlur;       /* pixels: the longest half-extent of a streak */
    cl_uint  taps;          /* samples along the streak */
    cl_float depthSoftness; /* relative: the depth extent over which "in front" falls from 1 to 0 */
} rtHipMotionBlurParams;
/* shutter = 0.5, maxBlur = 16, taps = 15, depthSoftness = 0.05: defaults of a parameter, not measurements. */
void rtHipMotionBlurDefaults(rtHipMotionBlurParams *params);
/* 0 for legal parameters, -1 (the last-error text set) for NULL or a value outside the ranges above.  Needs no device. */
int  rtHipMotionBlurCheck(const rtHipMotionBlurParams *params);
/* Bytes of scratch rtHipMotionBlurDevice needs for a width x height image: (l, depth) per pixel, 8 bytes, rounded up to 16, then tileMax
 * and nbMax at 16 bytes per 32 x 32 tile each.  0 for a size the filter refuses. */
uint64_t rtHipMotionBlurScratchBytes(cl_uint width, cl_uint height);
/* DEVICE arrays of `device`, asynchronous on `stream` (a hipStream_t of `device` as void*; NULL = the null stream): four launches, no
 * allocation, no synchronisation.  scratch: at least rtHipMotionBlurScratchBytes(width, height) bytes, 16-byte aligned, contents
 * irrelevant.  Pointer, overlap and stream checks are rtHipTemporalDevice's: out and scratch must overlap nothing.  Anything else returns
 * -1 with the last-error text set and launches nothing. */
int  rtHipMotionBlurDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *motion, const void *depth, void *out,
                           void *scratch, uint64_t scratchBytes, const rtHipMotionBlurParams *params, void *stream);
/* HOST arrays, synchronous; device memory is allocated and freed per call.  Same results as rtHipMotionBlurDevice. */
int  rtHipMotionBlur(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *motion, const cl_float *depth,
                     cl_float *out, const rtHipMotionBlurParams *params);
/* The scene's last frame, blurred on its device along the flow to the scene's motion reference.  The caller's loop is:
 * rtHipSceneMotionMark, rtHipSceneSetCamera and / or rtHipSceneSetGeometry, render, rtHipSceneMotionBlur.  The call needs a tile set
 * that holds every tile of the image once and a motion reference (without one: -1, "no motion reference"); it synchronises and finishes
 * the frame like rtHipReadback, and then, on the scene's stream: runs the motion pass (motion and t) into storage of its own; gathers
 * the colour ((float)u16 / 65535.0f of the beauty planes, what rtHipReadback gives); blurs; and quantises the planes as
 * rtHipSceneDenoise's.  THE CALL DOES NOT MARK: the reference stays the caller's.  rtHipSceneTemporal marks again, so a caller who wants
 * both on one frame blurs first and accumulates second (the accumulation then sees the unblurred frame and the same flow); or takes
 * rtHipSceneMotion before the temporal call and feeds its outColour to rtHipMotionBlur / rtHipMotionBlurDevice.
 * Outputs (each may be NULL, host arrays): outRgb W x H x 3 f32 and the u16 planes R, G, B.
 * Storage, made on first use in one block, counted in rtHipSceneBytes from then on and freed with the scene (a scene that never calls
 * holds none of it), with n = W*H and every part rounded up to 256 bytes: motion 8n, t 4n, the gathered colour 12n, the blurred image
 * 12n, the planes 3 x 2n and rtHipMotionBlurScratchBytes.
 * Refused with -1, the last-error text set and nothing launched: a NULL scene or params, parameters out of range, an image wider or
 * higher than 16384 or of more than 2^27 pixels, a tile subset, no motion reference, a reference made for another triangle count. */
int  rtHipSceneMotionBlur(rtHipScene *scene, const rtHipMotionBlurParams *params, cl_float *outRgb, cl_ushort *outR, cl_ushort *outG,
                          cl_ushort *outB);
/* Device time in milliseconds of the scene's last rtHipSceneMotionBlur call, from HIP events on the scene's stream: ms[0] the motion pass,
 * ms[1] the colour gather, ms[2] the blur and the output kernel.  All 0 before the first call.  Returns 0, or -1 for a NULL argument. */
int  rtHipSceneMotionBlurTimes(const rtHipScene *scene, cl_float ms[3]);

/* DEPTH OF FIELD: the lens as a post effect.  A frame is blurred by the circle of confusion its DEPTH pass gives every pixel: "scatter as
 * gather" -- a pixel q counts at p if q's own disc reaches p, spread over that disc's area --, with the gather's extent taken from a
 * per-tile maximum of the radius and its 3 x 3 neighbourhood maximum (the tile machinery of MOTION BLUR, after McGuire et al. 2012).
 * The frame kernels are not involved, and cannot be: every pixel's primary rays are tested against a candidate list built for ONE eye
 * point (rtHipBuildCameraList, rtHipSceneSetCamera), and a lens that moves the ray origin over an aperture would need other lists per
 * sample.  The arithmetic is IEEE fp32 + - * /, sqrtf, fabsf and compares in the order written (no FMA, no reciprocal-multiply, no
 * trigonometry; division and square root correctly rounded): tests/dof_oracle.py restates it in numpy and the device output equals it
 * bit for bit.  Every bit pattern of the inputs has a defined answer up to the payload of a NaN, and no index is formed before its
 * range test.
 *
 * All arrays are W x H, row-major; W, H and W*H limited as in TEMPORAL ACCUMULATION.  Inputs: colour 3 x f32; depth f32, exactly what
 * rtHipReadbackPasses writes for DEPTH: sample 1's distance from the eye to its hit ALONG THE RAY, +inf on a miss.  Output: out 3 x f32;
 * it must overlap no input (the taps belong to neighbours).
 * Parameters: focus finite and > 0, the distance in focus in the DEPTH pass's measure -- along the ray, so the surface in focus is a
 * sphere around the eye, not a plane --; cocScale finite in [0, 4096], pixels: the radius of the circle of confusion of a point
 * infinitely far away; maxCoc finite in [1, 32] pixels, the cap of a radius; rings in [1, 6]; depthSoftness finite and >= 0 (relative).
 * Anything else returns -1 before anything is launched.
 *   clamp01(r) = !(r > 0) ? 0 : (r > 1 ? 1 : r)                                                              (a NaN gives 0)
 *   sdc(a, b, e) = (a == b) ? 1.0f : clamp01(1.0f - (a - b) / e)            (is a in front of b, softly; as in MOTION BLUR)
 * (a) Radius of pixel q, z = depth_q:
 *   if (z == +inf) a = 1.0f;  else if (!(z > 0)) a = 0.0f  (a NaN, zero, negative, -inf);  else a = fabsf(z - focus) / z
 *   r = a * cocScale;  if (!(r < maxCoc)) r = cocScale > 0 ? maxCoc : 0.0f                       (also catches inf * 0, a NaN)
 *   So r is never negative and never a NaN, and cocScale == 0 gives r = 0 everywhere.
 * (b) Tile maximum.  Tiles are 32 x 32 pixels, tile(x, y) = (x >> 5, y >> 5).  tileMax[T] is the greatest r of the tile's pixels (a
 *   maximum of numbers that are not NaN: it does not depend on the order).
 * (c) Neighbourhood maximum.  nbMax[T] is the greatest tileMax over the tiles (Tx + dx, Ty + dy), dx, dy = -1..1, that exist.  Because
 *   maxCoc <= 32 = the tile's side, a pixel q whose disc reaches p (|q - p| <= r_q <= 32) lies in p's tile or in one of its eight
 *   neighbours, so r_q <= nbMax[tile(p)]: a gather of radius nbMax[tile(p)] around p visits the whole neighbourhood from which anything
 *   can reach p.  That makes the gather complete, and a neighbourhood whose maximum is below half a pixel a copy.
 * (d) Gather at p = (x, y), with R = nbMax[tile(p)]:
 *   if (!(R >= 0.5f)): out = colour_p, a copy, bit for bit.  Otherwise:
 *   rp = r_p < 0.5f ? 0.5f : r_p;  zp = depth_p
 *   j = ((x & 1) * 2 + (y & 1) * 3) & 3;  jit = ((float)j - 1.5f) * 0.25f                (a fixed 2 x 2 dither: no random state)
 *   wsum = 1.0f / (rp * rp);  sum = colour_p * wsum (per channel)                                              (the centre tap)
 *   The other taps lie on `rings` octagonal rings (no sine, no cosine).  V[0..8] = (1,0), (c,c), (0,1), (-c,c), (-1,0), (-c,-c), (0,-1),
 *   (c,-c), (1,0) with the one literal c = 0.70710678f.  Ring k = 1..rings has 8k taps s = 0..8k-1 (1 + 4*rings*(rings+1) taps in all,
 *   the centre included); for k ascending, and s ascending within k:
 *     v = s / k;  m = s % k  (integers);  f = (float)m / (float)k
 *     ux = V[v].x + (V[v+1].x - V[v].x) * f;  uy = V[v].y + (V[v+1].y - V[v].y) * f
 *     rad = (((float)k + jit) / (float)rings) * R;  ox = ux * rad;  oy = uy * rad
 *     X = ((float)x + 0.5f) + ox;  Y = ((float)y + 0.5f) + oy
 *     the tap is skipped unless X >= 0 && X < (float)W && Y >= 0 && Y < (float)H; then q = ((int)X, (int)Y)
 *     d = sqrtf(ox*ox + oy*oy);  rq = r_q < 0.5f ? 0.5f : r_q;  zq = depth_q;  e = depthSoftness * (zp < zq ? zp : zq)
 *     fr = sdc(zq, zp, e)        (1 when q lies in front of p or at p's depth, both at +inf included; 0 when it lies well behind)
 *     m2 = rq < rp ? rq : rp;  reff = rq * fr + m2 * (1.0f - fr)
 *     w = clamp01((reff - d) + 0.5f) / (reff * reff)
 *     wsum += w;  sum += colour_q * w (per channel: a multiply, an add)
 *   out = sum / wsum per channel
 * The (1 - fr) term keeps a sharp pixel sharp in front of a blurred background: a pixel behind p spreads no further over p than p's
 * own disc.  reff lies in [0.5, maxCoc], wsum starts positive and no weight is negative or a NaN, so out is a NaN only where a colour
 * it sums is.  The outermost ring of a pixel whose dither is positive lies up to R * 0.375 / rings outside R: such taps weigh little
 * or nothing and are read like any other.
 * Not done: lens sampling inside the frame kernels (the candidate lists belong to one eye point, above); axial depth (focus and depth
 * are distances along the ray: the surface in focus is a sphere); an anti-aliased depth (DEPTH is sample 1's: silhouettes are
 * classified per pixel); separate near and far layers with in-painting behind a blurred foreground (a blurred near object shows the
 * sharp background's own pixels through it, not what it hides); bokeh highlights (the weights are energy-preserving discs, nothing is
 * boosted); tile-dealt instances (their taps cross tile borders: the array entry points take a composed image). */
typedef struct rtHipDepthOfFieldParams {
    cl_float focus;         /* the distance in focus, along the ray (the DEPTH pass's measure) */
    cl_float cocScale;      /* pixels: the circle-of-confusion radius of a point infinitely far away */
    cl_float maxCoc;        /* pixels: the cap of a radius */
    cl_uint  rings;         /* octagonal rings of taps: 1 + 4*rings*(rings+1) taps */
    cl_float depthSoftness; /* relative: the depth extent over which "in front" falls from 1 to 0 */
} rtHipDepthOfFieldParams;
/* focus = 1, cocScale = 8, maxCoc = 16, rings = 3, depthSoftness = 0.05: defaults of a parameter, not measurements. */
void rtHipDepthOfFieldDefaults(rtHipDepthOfFieldParams *params);
/* 0 for legal parameters, -1 (the last-error text set) for NULL or a value outside the ranges above.  Needs no device. */
int  rtHipDepthOfFieldCheck(const rtHipDepthOfFieldParams *params);
/* Bytes of scratch rtHipDepthOfFieldDevice needs for a width x height image of n pixels and T = ceil(width/32) * ceil(height/32) tiles:
 * (r, depth) per pixel, 8n bytes rounded up to 16, then tileMax and nbMax, 4T bytes each rounded up to 16.  0 for a size the filter
 * refuses. */
uint64_t rtHipDepthOfFieldScratchBytes(cl_uint width, cl_uint height);
/* DEVICE arrays of `device`, asynchronous on `stream` (a hipStream_t of `device` as void*; NULL = the null stream): four launches, no
 * allocation, no synchronisation.  scratch: at least rtHipDepthOfFieldScratchBytes(width, height) bytes, 16-byte aligned, contents
 * irrelevant.  Pointer, overlap and stream checks are rtHipTemporalDevice's: out and scratch must overlap nothing.  Anything else returns
 * -1 with the last-error text set and launches nothing. */
int  rtHipDepthOfFieldDevice(int device, cl_uint width, cl_uint height, const void *colour, const void *depth, void *out, void *scratch,
                             uint64_t scratchBytes, const rtHipDepthOfFieldParams *params, void *stream);
/* HOST arrays, synchronous; device memory is allocated and freed per call.  Same results as rtHipDepthOfFieldDevice. */
int  rtHipDepthOfField(int device, cl_uint width, cl_uint height, const cl_float *colour, const cl_float *depth, cl_float *out,
                       const rtHipDepthOfFieldParams *params);
/* The scene's last frame, blurred on its device by its own DEPTH pass.  The call needs RT_HIP_PASS_DEPTH on (rtHipScenePasses, before
 * the frame) and a tile set that holds every tile of the image once; it synchronises and finishes the frame like rtHipReadback, and
 * then, on the scene's stream: gathers the colour ((float)u16 / 65535.0f of the beauty planes, what rtHipReadback gives) and the depth
 * (the pass buffer's words, what rtHipReadbackPasses gives) into row-major storage of its own; blurs; and quantises the planes as
 * rtHipSceneDenoise's.  It changes neither the tile buffer, the pass buffer, the temporal history nor the motion reference.
 * Outputs (each may be NULL, host arrays): outRgb W x H x 3 f32 and the u16 planes R, G, B.
 * Storage, made on first use in one block, counted in rtHipSceneBytes from then on and freed with the scene (a scene that never calls
 * holds none of it), with n = W*H and every part rounded up to 256 bytes: the gathered colour 12n, the depth 4n, the blurred image 12n,
 * the planes 3 x 2n and rtHipDepthOfFieldScratchBytes.
 * Refused with -1, the last-error text set and nothing launched: a NULL scene or params, parameters out of range, an image wider or
 * higher than 16384 or of more than 2^27 pixels, the depth pass off, a tile subset. */
int  rtHipSceneDepthOfField(rtHipScene *scene, const rtHipDepthOfFieldParams *params, cl_float *outRgb, cl_ushort *outR, cl_ushort *outG,
                            cl_ushort *outB);
/* Device time in milliseconds of the scene's last rtHipSceneDepthOfField call, from HIP events on the scene's stream: ms[0] the gather of
 * colour and depth, ms[1] the blur, ms[2] the output kernel.  All 0 before the first call.  Returns 0, or -1 for a NULL argument. */
int  rtHipSceneDepthOfFieldTimes(const rtHipScene *scene, cl_float ms[3]);
/* A thin lens into the parameters: fills inout->focus = focus and inout->cocScale = apertureRadius * focalPixels / focus, the radius in
 * pixels of the circle of confusion of a point infinitely far away for a lens of radius apertureRadius (scene units) focused at `focus`
 * (scene units, along the ray).  focalPixels is the distance from the eye to the image plane over the pixel pitch, from the camera's
 * vectors, in double with + - * / and sqrt only (lane 3 not read):
 *   n = leftToRight x topToBottom  (n.x = lr.y*tb.z - lr.z*tb.y, n.y = lr.z*tb.x - lr.x*tb.z, n.z = lr.x*tb.y - lr.y*tb.x)
 *   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z;  h = dot(eyeToTopLeft, n);  if (h < 0) h = -h
 *   plane = h / sqrt(dot(n, n));  pitch = sqrt(dot(leftToRight, leftToRight));  focalPixels = plane / pitch
 *   cocScale = (float)(((double)apertureRadius * focalPixels) / (double)focus)                                 (rounded once)
 * The other fields of *inout are kept.  Returns 0; -1 (the last-error text set, *inout unchanged) for a NULL argument, a camera whose
 * pitch or plane distance is zero or not finite, or a focus or cocScale outside the ranges rtHipDepthOfFieldCheck allows (the other fields are not looked
 * at).  Needs no device. */
int  rtHipDepthOfFieldLens(const rtHipCamera *camera, cl_float apertureRadius, cl_float focus, rtHipDepthOfFieldParams *inout);

/* AMBIENT OCCLUSION BAKE: a W x H texture of ambient occlusion over the scene's UV layout.  Each texel centre is mapped to the surface
 * point of the triangle whose UV triangle covers it, and the AO rays of the block above are traced from there with the same walk.  It
 * needs geometry, UVs, corner normals and the grid only: it works on every instance (whatever its tiles, passes or pipeline), ignores
 * the tile set, and changes nothing a later frame, read-back, pass, denoise or AO call produces.  The arithmetic is IEEE fp32 + - * /,
 * sqrt and compares (no FMA, division and square root correctly rounded) plus the AO block's hash; dot and cross as defined there.
 * tests/bake_oracle.py restates it in numpy and the device output equals it bit for bit.
 *
 * Parameters: W, H >= 1 with W*H <= 2^26; raysPerTexel R in 1..256; radius > 0 (+inf allowed, NaN not); seed any u32; dilate G in 0..64;
 * the triangles firstTriangle .. firstTriangle + triangleCount - 1 are selected (first + count <= T; triangleCount = 0xffffffff selects
 * first .. T - 1, first <= T), and of those, when matchMaterial is non-zero, only the ones whose material id equals `material` (-1 is an id).
 * Texel (x, y), index t = y*W + x, row 0 at v near 0 (the top row, as the renderer's textures are read): cu = ((float)x + 0.5f) / (float)W,
 * cv = ((float)y + 0.5f) / (float)H.  A selected triangle with corner UVs uvA, uvB, uvC (its triangleUv[3i .. 3i+2]) covers it iff
 * l1 >= 0 && l2 >= 0 && l1 + l2 <= 1, with e1 = uvB - uvA, e2 = uvC - uvA, q = (cu, cv) - uvA per component,
 * den = e1.x*e2.y - e1.y*e2.x, l1 = (q.x*e2.y - q.y*e2.x) / den, l2 = (e1.x*q.y - e1.y*q.x) / den.  NaN compares false: a triangle
 * with den = 0 or a NaN UV covers nothing.  UVs are not wrapped (the renderer's look-up wraps them; the bake clips to [0,1]^2).  Of
 * several covering triangles the smallest id wins.  Every bit pattern of the UVs has a defined answer.
 * A covered texel, winner tri: P = (a + l1*ab) + l2*ac per component (a, ab, ac = b - a, c - a from the vertices; l1 weighs b, l2 c);
 * n = cross(ac, ab); s = (nA + nB) + nC from the corner normals; n = -n if dot(n, s) < 0; m = dot(n, n); if !(m > 0) the texel counts
 * R open rays, else n^ = n / sqrt(m) (three divisions) and AO ray r (0 <= r < R) is the AO block's ray around n^ with counter
 * c = ((t*(R + 1) + 1 + r)*32 + draw) (the AO counter at p = t, Sp = 1, j = 0): o = P, tmin = 0, tmax = radius, excluding tri, occluded
 * iff the walk returns a triangle.  Value: (float)U / (float)R for a covered texel with U open rays, 0 for an uncovered one.  Triangle
 * map: the winner, 0xffffffff where nothing covers the texel.
 * Dilation (a gutter fill): G Jacobi passes.  A texel is valid at the start iff it is covered.  In a pass, an invalid texel sums the
 * values of its valid neighbours inside the map, rows dy = -1..1 outer, dx = -1..1 inner, itself skipped, in that order from +0.0f; if
 * k > 0 of them are valid it takes sum / (float)k and is valid from the next pass on.  The triangle map is not dilated.
 * Out of scope: one sample per texel (no super-sampling), no conservative coverage of UV slivers, and the renderer's texture look-up
 * (floor(u*(w-1))) sees a baked map shifted by up to one texel.
 * The scratch (winners, counters and values, 12 bytes per texel; one chunk of texels, 32 bytes each, "bake_texels" of rtHipTune; a list
 * of 4 bytes per triangle) belongs to the scene: made on first use, grown for a larger map, counted in rtHipSceneBytes, freed with the
 * scene.  Calls on different streams are ordered by an event.  Both calls refuse, with -1, the last-error text set and nothing launched:
 * a NULL scene, params or ao, a parameter out of range, a triangle range past T. */
typedef struct rtHipBakeParams {
    cl_uint  width, height;   /* W, H */
    cl_uint  raysPerTexel;    /* R */
    cl_float radius;          /* tmax of the AO rays */
    cl_uint  seed;
    cl_uint  dilate;          /* G */
    cl_uint  firstTriangle, triangleCount;
    cl_int   material;        /* the material filter, used when matchMaterial != 0 */
    cl_uint  matchMaterial;
} rtHipBakeParams;
/* R = 16, radius = +inf, seed = 0, G = 2, every triangle (first 0, count 0xffffffff), no material filter; width and height are set to 0,
 * which the calls refuse: the caller sets them. */
void rtHipBakeDefaults(rtHipBakeParams *params);
/* HOST W x H arrays, row-major: ao f32, triangle u32 (may be NULL); synchronous, on the scene's stream. */
int  rtHipSceneBakeAmbientOcclusion(rtHipScene *scene, const rtHipBakeParams *params, cl_float *ao, cl_uint *triangle);
/* DEVICE W x H arrays of the scene's device (4-byte aligned; triangle may be NULL), asynchronous on `stream` (a hipStream_t as void*;
 * NULL = the scene's stream).  Checked like rtHipSceneIntersectDevice's pointers; a host pointer returns -1. */
int  rtHipSceneBakeAmbientOcclusionDevice(rtHipScene *scene, const rtHipBakeParams *params, void *ao, void *triangle, void *stream);

/* Average device time in milliseconds of one rtHipRenderTiles frame (all its kernels) over the frames recorded since
 * the last call (HIP events on the launch stream), and the number of frames.  Returns 0 on success. */
int rtHipKernelTime(rtHipScene *scene, double *avgMs, uint64_t *launches);

/* ------------------------------------------------------------------------------------------------------------
 * Host-side acceleration-structure builders: the producers of the hot path's list inputs
 * (counterparts of CameraTriangleList::New, source/util/trianglelist.cpp:520-626, and SceneTriangleList::New,
 * :655-737).  Same membership tests in the same fp32 arithmetic; memory comes from malloc and is released with
 * rtHipFree.  threads<=0 = all hardware threads.
 * ---------------------------------------------------------------------------------------------------------- */
int rtHipBuildCameraList(cl_uint width, cl_uint height, const cl_float eye[4], const cl_float eyeToTopLeft[4],
                         const cl_float leftToRight[4], const cl_float topToBottom[4], cl_float pixelSizeInv,
                         cl_uint triangleCount, const cl_float3 *vertex, const cl_int3 *triIndex, int threads,
                         cl_uint **outStart, cl_uint **outEnd, cl_uint **outList, uint64_t *outListSize);

/* The same camera lists built on a HIP device (rt_build_device.hip): identical membership (the arithmetic is one shared
 * header compiled for both), every pixel's entries ascending, and the reference's neighbour de-duplication (:580-613: equal
 * neighbouring lists share storage) applied, so Start, End and the list equal rtHipBuildCameraList's.  Fails (no CPU
 * fallback) when the device is missing.  Returns -3, before the list is allocated, when it would hold more than 2^32 - 1 entries
 * (the host builder's limit; "build_list_limit" of rtHipTune lowers it).
 * *deviceMs (optional) = device time of the build without the transfers. */
int rtHipBuildCameraListDevice(int device, cl_uint width, cl_uint height, const cl_float eye[4], const cl_float eyeToTopLeft[4],
                               const cl_float leftToRight[4], const cl_float topToBottom[4], cl_float pixelSizeInv,
                               cl_uint vertexCount, cl_uint triangleCount, const cl_float3 *vertex, const cl_int3 *triIndex,
                               cl_uint **outStart, cl_uint **outEnd, cl_uint **outList, uint64_t *outListSize, double *deviceMs);

int rtHipBuildSceneGrid(cl_uint vertexCount, cl_uint triangleCount, const cl_float3 *vertex, const cl_int3 *triIndex,
                        int threads, cl_float3 outBoxMin[257], cl_uint **outStart, cl_uint **outList,
                        uint64_t *outListSize);

/* The same grid built on a HIP device (rt_build_device.hip): split planes from radix-sorted coordinates, the flood fill of
 * every triangle with the shared membership test (small triangles one thread each, big ones one workgroup each), pairs
 * radix-sorted on cell << 32 | triangle.  Same planes, starts and lists as rtHipBuildSceneGrid.  No CPU fallback.  Returns -3
 * for more than 2^32 - 1 pairs (lowered by "build_list_limit"), -7 when a single fill outgrows its workgroup queue. */
int rtHipBuildSceneGridDevice(int device, cl_uint vertexCount, cl_uint triangleCount, const cl_float3 *vertex, const cl_int3 *triIndex,
                              cl_float3 outBoxMin[257], cl_uint **outStart, cl_uint **outList, uint64_t *outListSize, double *deviceMs);

void rtHipFree(void *p);

/* ------------------------------------------------------------------------------------------------------------
 * (3) HEADLESS FRONT-END and OUTPUT SINKS (rt_frontend.cpp; host code, no GPU involved).
 * The SDK-free arithmetic of the reference's scene extraction (source/render.cpp) and of its output path, so that a
 * host without Cinema 4D can feed RaytraceAll from plain meshes and get an image file back.
 * ---------------------------------------------------------------------------------------------------------- */

/* SetCamera (render.cpp:461-491): camera vectors from eye position, look-at point, up vector, horizontal field of view
 * (radians) and image size.  Same operations in the same order: the eye-to-top-left vector keeps the LENGTH of
 * (object - position), pixel vectors are unit vectors divided by pixelSizeInv = width / (2 |object - position| tan(fov/2)). */
void rtHipSetCamera(cl_float3 *outEyeToTopLeft, cl_float3 *outLeftToRight, cl_float3 *outTopToBottom, cl_float *outPixelSizeInv,
                    const cl_float position[3], const cl_float object[3], const cl_float up[3], cl_float fov, cl_uint width, cl_uint height);

/* One polygon object as AddPolygonsRecursive sees it (render.cpp:707-963), points already in world space. */
typedef struct rtHipMesh {
    cl_uint pointCount;
    const cl_float3 *points;
    cl_uint polygonCount;
    const cl_int *polygons;           /* 4 indices a,b,c,d per polygon; c == d marks a triangle (render.cpp:736) */
    const cl_float3 *cornerNormals;   /* optional, 4 per polygon (a,b,c,d), any length; NULL -- or a zero vector at a corner of the triangle -- =
                                       * face normal turned to the camera (:754-771) */
    const cl_float2 *cornerUv;        /* optional, 4 per polygon; NULL = (0,0),(0,1),(1,1) for every triangle (:956-963) */
    const cl_int *polygonMaterial;    /* optional, one id per polygon; NULL = -1, "no material" (:1098) */
} rtHipMesh;

/* Sizes of the arrays rtHipMeshFill writes: vertices = all points, triangles = 1 per triangle + 2 per quad.
 * Returns 0, -1 null argument, -2 a polygon index outside its object's points, -3 too many elements. */
int rtHipMeshCount(const rtHipMesh *meshes, cl_uint meshCount, cl_uint *vertexCount, cl_uint *triangleCount);

/* Fills RaytraceAll's geometry arrays (vertex[V], triangleVertexIndex[T], triangleMaterialId[T], triangleUv[3T],
 * triangleNormal[3T]) from the meshes: a quad becomes (a,b,c) and (a,c,d) with its corner normals and UVs following. */
int rtHipMeshFill(const rtHipMesh *meshes, cl_uint meshCount, const cl_float cameraEye[3], cl_float3 *vertex, cl_int3 *triIndex,
                  cl_int *triMaterial, cl_float2 *triUv, cl_float3 *triNormal);

/* One light as render.cpp:965-993 stores it: direction normalised, colour x brightness, radius 0.52 (degrees; the sun's
 * angular size, used for every light), half-attenuation distance infinite.  `type` as in raytrace_opencl.h:1-12. */
void rtHipLightFill(cl_uint index, cl_int type, const cl_float position[3], const cl_float direction[3], const cl_float colour[3],
                    cl_float brightness, cl_int *lightType, cl_float3 *lightPosition, cl_float3 *lightDirection, cl_float3 *lightColour,
                    cl_float *lightRadius, cl_float *lightHalfAttenuationDistance);

/* Material channels in the reference's order: colour, reflection, transparency, bump, luminance (render.cpp:1136). */
typedef struct rtHipChannelSpec {
    cl_int enabled;            /* the channel exists and is switched on (render.cpp:1143-1145) */
    cl_uint width, height;     /* bitmap size; 0 = the channel has no bitmap */
    const cl_uchar3 *pixels;   /* width*height texels, row-major, 4 bytes each */
} rtHipChannelSpec;
typedef struct rtHipMaterialSpec {
    rtHipChannelSpec channel[5];
    cl_float color[3];         /* MATERIAL_COLOR_COLOR, used when the colour channel has no bitmap (render.cpp:1254-1275) */
    cl_float brightness;       /* MATERIAL_COLOR_BRIGHTNESS */
} rtHipMaterialSpec;

/* The channel table rules of render.cpp:1136-1309 for bitmaps and absent channels (C4D shaders need the SDK): a channel
 * that is off is 0x0; reflection / transparency switched on without an image are 1x1 of 0.2 / 1.0; every non-colour
 * channel still 0x0 becomes 1x1 black; a colour channel without an image becomes 1x1 of color x brightness;
 * materialImageStart[5*count] receives the texel total.  Call with textures == NULL to size the atlas (*texturesSize),
 * then again with a buffer.  Returns 0, -1 null argument, -2 capacity too small, -3 atlas larger than 2^31 texels. */
int rtHipBakeMaterials(const rtHipMaterialSpec *materials, cl_uint materialCount, cl_uint2 *materialImageSize, cl_int *materialImageStart,
                       cl_uchar3 *textures, cl_uint texturesCapacity, cl_uint *texturesSize);

/* FILE INPUT (rt_fileio.cpp).  The reference walks Cinema 4D's object tree (render.cpp:707-1003) and bakes C4D bitmaps
 * (render.cpp:1136-1309); a host without Cinema 4D has files.
 *
 * rtHipObjRead: a Wavefront OBJ (v / vt / vn / f with triangles, quads and larger faces -- fanned --, negative indices, usemtl,
 * mtllib) as ONE polygon object in rtHipMesh's shape: 4-float points, polygons a,b,c,d with c == d marking a triangle, and -- when
 * any face carries them -- 4 corner normals / 4 corner UVs per polygon (zero where a face has none), one material id per polygon
 * (-1 before the first usemtl).  The materials its MTL libraries define (paths relative to the OBJ) come back as rtHipObjMaterial:
 * Kd = material colour, d / Tr = opacity, Ke = emission, refl = reflectance, and the channel image paths map_Kd (colour), map_refl
 * (reflection), map_d (transparency), map_bump / map_Bump / bump (bump), map_Ke (luminance).  Arrays are malloc'ed: rtHipObjFree.
 * Returns 0, -1 null argument, -2 malformed file, -3 out of memory, -4 cannot open; on any failure *out is zeroed.
 *
 * The rules the readers keep (tests/fileio_oracle.py is an independent reader written from them; tests/test_fileio.py holds both to them):
 *
 * OBJ / MTL
 *  - A line ends at LF; carriage returns are dropped, so CR LF files read alike; the last line needs no newline.  Blanks and tabs
 *    separate tokens.  Every read stays inside the line.
 *  - The keyword is the line's first token.  v, vt, vn, f, usemtl and mtllib are recognised only as whole tokens: "vtx ..",
 *    "vnormal ..", "vp .." and every other keyword (o, g, s, l, ...) are ignored, as are lines whose first token starts with '#'.
 *  - v and vn need three numbers, vt one or two (a missing second is 0); fewer gives -2, and so does a recognised keyword with
 *    nothing behind it.  Tokens behind the numbers are ignored ("v x y z w").
 *  - A number is a whole token that strtof reads in decimal form: [+-] digits [. digits] [e [+-] digits] with at least one digit
 *    before the exponent, or [+-] inf / infinity / nan in any letter case.  Anything else where a number is due ("1.5abc", "0x1p3",
 *    "nan(1)", a second vt token that is no number) gives -2.
 *  - A face needs at least 3 corners; 3 or 4 make one polygon, more are fanned into triangles (0, k, k + 1).
 *  - A corner token is v, v/vt, v//vn or v/vt/vn; an index is an optional '-' and decimal digits.  An empty vt or vn field ("1/",
 *    "1//", "1/2/") means "absent".  The whole token must be consumed: "1x" and "1/2/3/4" give -2.  An index of 0 gives -2; so does
 *    an index outside what has been defined so far, counted from the start (positive) or from the end (negative), and an index that
 *    does not fit 32 bits ("4294967297", "-4294967297", 20 digits).
 *  - The name after usemtl / newmtl and the file name after mtllib / map_* run to the end of the line with leading and trailing blanks
 *    and tabs removed; they may contain blanks.  A path that starts with '/' is taken as given, any other is relative to the OBJ's
 *    directory.  Names are cut to 63 bytes in the record, paths to 255.
 *  - Materials are numbered in the order of first use (usemtl) and then of first definition (newmtl), the libraries read in the order
 *    of their mtllib lines after the whole OBJ.  A missing library leaves its materials at their defaults.
 *  - In a library the keywords newmtl, Kd, Ke, d, Tr, refl and the seven map_* spellings are whole tokens too; what stands before
 *    the first newmtl and every other statement (Ns, illum, ...) is ignored.  Kd and Ke need three numbers, d, Tr and refl one
 *    (dissolve = 1 - Tr in float); a statement of a material with fewer, or a newmtl or map_* without a name, gives -2.  The last
 *    statement of a kind wins. */
typedef struct rtHipObjMaterial {
    char name[64];
    cl_float kd[3];            /* Kd (default 1 1 1) */
    cl_float ke[3]; cl_int hasKe;
    cl_float dissolve;         /* d, or 1 - Tr (default 1 = opaque) */
    cl_float reflect; cl_int hasReflect;
    char map[5][256];          /* image path per channel in the reference's order (colour, reflection, transparency, bump, luminance); "" = none */
} rtHipObjMaterial;
typedef struct rtHipObjData {
    cl_uint pointCount; cl_float3 *points;
    cl_uint polygonCount; cl_int *polygons; cl_float3 *cornerNormals; cl_float2 *cornerUv; cl_int *polygonMaterial;
    cl_uint materialCount; rtHipObjMaterial *materials;
} rtHipObjData;
int  rtHipObjRead(const char *path, rtHipObjData *out);
void rtHipObjFree(rtHipObjData *data);

/* An image file as rtHipChannelSpec::pixels: binary or plain PPM (P6 / P3, maxval <= 255, scaled to 255) or an uncompressed 24 / 32-bit
 * BMP -> width*height texels of 4 bytes (r, g, b, 0), top row first, malloc'ed (rtHipFree).  Returns 0, -1 null argument, -2 not
 * such a file, -3 out of memory, -4 cannot open; on any failure *pixels is NULL and *width = *height = 0.
 *
 * PPM
 *  - "P6" or "P3", one white-space byte (C's isspace), then width, height and maxval as decimal digits, each after any run of white
 *    space and comments ('#' to the end of its line).  Width and height must be at least 1 (and at most 10^9), maxval 1..255.
 *  - In P6 exactly one white-space byte follows maxval, then 3wh sample bytes; anything else there gives -2.  Bytes behind the
 *    samples are ignored.  In P3 the samples are decimal numbers separated like the header's (comments allowed); what follows the
 *    last one is ignored.
 *  - A sample above maxval gives -2, in P6 as in P3.  A sample s becomes s * 255 / maxval, rounded down.
 *  - A file may end anywhere: if it ends before the last sample the result is -2, and no byte outside the file is read.
 *  - The header's size is checked against the bytes that are there before anything proportional to it is allocated: P6 needs 3wh
 *    bytes behind maxval's white-space byte, P3 at least 6wh - 1 bytes behind maxval (a digit per sample, a separator between two).
 * BMP
 *  - "BM", a 14-byte file header and an info header of at least 40 bytes (a V4 / V5 header is fine; what lies past the first 40 bytes
 *    of it is not read).  Refused with -2: a file shorter than 54 bytes; an info header smaller than 40 bytes; a pixel offset below
 *    14 + that header's size; a pixel offset or a row range past the end of the file; width < 1; height 0 or INT32_MIN; depths other
 *    than 24 / 32; compression other than 0 (or 3 at 32 bits, read as BGRA like 0).
 *  - Rows are padded to 4 bytes.  A positive height means bottom row first, a negative one top row first; both are read.  The fourth
 *    byte of a 32-bit texel is dropped.
 *  - The size is checked before anything is allocated. */
int rtHipImageRead(const char *path, cl_uint *width, cl_uint *height, cl_uchar3 **pixels);

/* ShdProjectPoint (render.cpp:495-673): the UV a point gets from a texture tag's projection when its polygon has no UVW tag
 * (render.cpp:917-945).  Same operations in the same order in double (the SDK's Float), results cast to float as at :940-941;
 * RT_PROJ_FRONTAL / RT_PROJ_UVW are not handled by the reference either (uv is left as it is).  The numbering is the Cinema 4D
 * SDK's (c4d_shader.h: P_SPHERICAL ...; not in this checkout).  Returns 1 when the texture tiles or uv lies in [0,1]^2, else 0. */
enum { RT_PROJ_SPHERICAL = 0, RT_PROJ_CYLINDRICAL = 1, RT_PROJ_FLAT = 2, RT_PROJ_CUBIC = 3, RT_PROJ_FRONTAL = 4, RT_PROJ_SPATIAL = 5,
       RT_PROJ_UVW = 6, RT_PROJ_SHRINKWRAP = 7, RT_PROJ_VOLUMESHADER = 10 };
int rtHipProjectUv(int projection, const cl_float point[3], const cl_float normal[3], cl_float offsetX, cl_float offsetY, cl_float lengthX,
                   cl_float lengthY, int tile, cl_float uv[2]);

/* u16 planes -> interleaved 8-bit RGB, top row first: value / 256 (render.cpp:1379-1382).  lowByteCompat != 0 keeps the LOW
 * byte instead, which is what the reference's debug BMP does (writebmp.cpp:136-141, a truncation bug). */
void rtHipPlanesToRgb8(cl_uint width, cl_uint height, const cl_ushort *red, const cl_ushort *green, const cl_ushort *blue,
                       cl_uchar *rgb, int lowByteCompat);

/* writebmp3s (writebmp.cpp:124-177) to a path of the caller's choice: 54-byte header with file size 54 + 3wh, 24-bit BGR,
 * bottom row first, rows padded to 4 bytes.  Returns 0, -1 bad argument, -3 image too large for the header, -4 I/O error. */
int rtHipWriteBmp(const char *path, cl_uint width, cl_uint height, const cl_ushort *red, const cl_ushort *green, const cl_ushort *blue,
                  int lowByteCompat);

/* Binary PPM (P6, maxval 255) of the same 8-bit image, top row first. */
int rtHipWritePpm(const char *path, cl_uint width, cl_uint height, const cl_ushort *red, const cl_ushort *green, const cl_ushort *blue);

/* Sinks of the render passes (rtHipReadbackPasses): an 8-bit binary PGM (P5, maxval 255, top row first) of a u16 plane, value >> 8
 * like the colour sinks; a PFM greyscale image (Pf, scale -1.0 = little-endian floats, bottom row first) of an f32 plane.
 * Returns 0, -1 bad argument, -4 I/O error. */
int rtHipWritePgm(const char *path, cl_uint width, cl_uint height, const cl_ushort *plane);
int rtHipWritePfm(const char *path, cl_uint width, cl_uint height, const cl_float *plane);
/* Sink of the surface passes (rtHipReadbackSurfacePasses): a colour PFM (PF, scale -1.0 = little-endian floats, bottom row first) of a
 * row-major width x height x 3 f32 image.  Returns 0, -1 bad argument, -4 I/O error. */
int rtHipWritePfmRgb(const char *path, cl_uint width, cl_uint height, const cl_float *rgb);

/* ------------------------------------------------------------------------------------------------------------
 * TEST-ONLY: device-side known-answer runner (rt_kat.hip).  Runs the kernels' own building blocks -- the restatements
 * of randF (raytrace_opencl.c:12-23), GetSpherePoint (:30-45), positive_modf (:25-28), RayIntersectsTriangle
 * (:124-172, on the pre-resolved record), GetPointToLineSqLen (:83-101), GetBoxAddress (:174-193), BindInCube
 * (:265-322) and the (float)pow(0.5f, x) of :631 -- over `count` items on a HIP device, one per thread; layouts per op
 * are documented at the top of rt_kat.hip.  `table` is only read by RT_KAT_BOX (split planes, 3 x 257 floats, one
 * array per axis).  Returns 0, -1 bad arguments, -2 no such device (there is no CPU stand-in), -3 HIP failure.
 * ---------------------------------------------------------------------------------------------------------- */
enum { RT_KAT_RANDF = 0, RT_KAT_SPHERE, RT_KAT_PMODF, RT_KAT_TRI, RT_KAT_PLINE, RT_KAT_BOX, RT_KAT_BIND, RT_KAT_POW, RT_KAT_QUOTIENT,
       RT_KAT_SPHERE_SPLIT, RT_KAT_ACCUM, RT_KAT_OPS };
int rtHipDeviceKat(int device, int op, cl_uint count, const void *in, cl_uint inStride, void *out, cl_uint outStride, const float *table);

/* TEST-ONLY: the shading building blocks -- the texel look-up (Get2dTableValue3, raytrace_opencl.c:103-122) on every route
 * texel_rec / texel take, and the shading normal (GetTriangleNormal, :195-263) in all three instantiations the kernels use -- run on
 * a RESIDENT scene's own device records (triangle records, shading rows, material descriptors, atlas, bump tables), `count` items
 * of 40 (RT_SHADE_KAT_TEXEL) or 48 (RT_SHADE_KAT_NORMAL) bytes in, 64 or 96 bytes out; layouts at the top of rt_kat.hip.
 * Returns 0, -1 bad arguments (an unknown op, a material, channel or triangle the scene does not have, an empty atlas),
 * -3 HIP failure. */
enum { RT_SHADE_KAT_TEXEL = 0, RT_SHADE_KAT_NORMAL = 1 };
int rtHipTestShadeKat(const rtHipScene *scene, int op, cl_uint count, const void *in, void *out);

/* TEST / TUNING ONLY.  The library reads no environment variables (a plugin host's environment must not be able to slow frames
 * down, make them redo themselves or fail); every tuning value and every fault injector of the tests is set here, process-wide,
 * and applies to scenes built afterwards.  Keys (rt_host.h, struct Tuning): "reset" (all defaults), "stage_mb", "extra_factor",
 * "state_mb", "groups", "lookahead", "seg0".."seg4", "seg_rays0".."seg_rays3", "fast_quotient", "spin_limit", "append_rays", "ordered_first", "extra_factor",
 * "slice_rays", "small_slices", "group_rays", "blocking", "batch_plan", "pipeline", "timing", "cache", "logic_class" (0: every scene's
 * paths run on the general logic kernel; 1, the default: on the kernel of the scene's path class), "dead_shadow" (0: trace every
 * shadow ray; 1, the default: none for a light whose answer would only feed the face that is never read), "logic_split" (1, the
 * default: the later logic rounds of an opaque-diffuse scene with look-ahead on stream the answers and shade the bounce hits densely; 0:
 * one logic kernel per round), "ray_clip" (1, the default: a grid ray without a far end stops where it leaves the convex bound of the
 * grid's occupied cells; 0: at the grid's wall), "place_direct" (1, the default: a planned frame's uncut ordered rounds of an
 * opaque-diffuse scene are written in sorted place from the placement table the round's last scatter launch recorded, and run no scatter
 * launch; 0: every ordered round is scattered), and the test hooks "place_skew" (once per scene, the first table a round is about to be
 * placed by is skewed by one entry between two cells: that frame is flagged and rendered again),
 * "plan_rounds", "plan_grid_tiny", "plan_shade_skip" (planned frames launch no shade pass), "visit_log" (every frame waits after each round's
 * trace launch and reads the round back for rtHipTestRoundVisits), "virtual_devices", and of the device list builders "build_key_cap" (first key capacity of
 * rtHipBuildSceneGridDevice, 0 = max(32 T, 2^22)) and "build_list_limit" (most entries either device builder may return, default
 * and most 2^32 - 1; above it they return -3), "query_rays" (rays per staging chunk of rtHipSceneIntersect, default 2^20), and
 * "ao_samples" (pixel samples per chunk of the ambient occlusion calls, default 2^20, at most 2^24), and "bake_texels" (texels per chunk
 * of the ambient occlusion bake, default 2^20, at most 2^24; a call uses at most 2^31 / R).  "matte_chunk" (samples per launch of the
 * matte count kernel, default 64) is read at the entry of every matte call, not at scene creation, and is refused outside 1..65536.
 * Returns 0, -1 for an unknown key. */
int rtHipTune(const char *key, double value);

/* TEST-ONLY: device addresses held by the first scene of RaytraceAll's cache -- triangle records, shading rows, the grid's pair
 * records, material descriptors, texture atlas, camera list -- so that a test can see which parts a call left in place.
 * Returns 0, -2 when nothing is cached. */
int rtHipTestCachePointers(const void *out[6]);

/* TEST-ONLY: the content hash RaytraceAll's scene cache compares per input array (rt_api.cpp, hash_chunk), on the host.  Two byte
 * strings that differ must hash differently for the cache to notice an edit; tests/test_abi.py probes the tail handling. */
uint64_t rtHipTestHashBytes(const void *bytes, uint64_t count);

/* The path class a scene description falls in, on the host (no device needed): 1 = opaque-diffuse (every material's reflection,
 * transparency and luminance absent or one black texel, every height map absent or one texel, at most one light), 0 = general.  The
 * arrays must be host memory.  Returns -1 on an invalid description. */
int rtHipScenePathClass(const rtHipSceneDesc *desc);

/* TEST-ONLY: the path class a resident scene's logic kernels run (0 when "logic_class" was 0 at its build).  -1 for NULL. */
int rtHipTestPathClass(const rtHipScene *scene);

/* TEST-ONLY: the rays of each round of the scene's last wavefront frame, summed over its tile groups (round 0: the paths the primary
 * rays made; round r > 0: the rays logic round r - 1 sent to the grid), for rounds [0, n); rounds the frame did not issue read 0.  Call
 * after the frame was synchronised; with several sample batches the figures are the last batch's.  Returns the frame's round count,
 * -1 for invalid arguments. */
int rtHipTestRoundLog(const rtHipScene *scene, cl_uint *rays, cl_uint n);

/* TEST-ONLY, for scenes built with the test hook "visit_log" on: what the trace rounds of the scene's last wavefront frame held, summed over
 * its tile groups and sample batches.  With the hook on, every frame stops after each round's trace launch, and the host reads the round's
 * queues back before the next logic launch consumes them: the entries as the planning kernels wrote them, the rays' answers, and which main
 * entry went out with a look-ahead entry.  out[RT_ROUND_VISIT_FIELDS * r + f] for r < rounds (round 0 traces nothing and reads 0):
 *   RT_ROUND_VISIT_ORDERED   1 when the round was an ordered one: its entries were planned by the kernel that spawned the rays, and the visit
 *                            fields count them; a round that is not ordered is planned inside the trace kernel and its visit fields read 0
 *   RT_ROUND_VISIT_ENTRIES   trace entries (a cut ray makes several), RT_ROUND_VISIT_ENDED those of them that carry an end cell
 *   then, for the three kinds of ray -- a main entry sent out with a look-ahead entry (a hit's shadow ray), a main entry on its own, a
 *   look-ahead entry (a bounce ray) -- RT_ROUND_VISIT_RAYS + 3 * kind: rays, rays that hit something, planned cell visits.
 * An entry's planned visits are the cells its walk makes if it hits nothing: the Manhattan distance from its start cell to its end cell + 1;
 * for an entry without an end cell the host takes the cell where the ray leaves the grid's box (the planner's own arithmetic, exact cell
 * search).  Returns the frame's round count, -1 for invalid arguments or a scene built without the hook. */
enum { RT_ROUND_VISIT_ORDERED = 0, RT_ROUND_VISIT_ENTRIES, RT_ROUND_VISIT_ENDED, RT_ROUND_VISIT_RAYS, RT_ROUND_VISIT_FIELDS = 12 };
int rtHipTestRoundVisits(const rtHipScene *scene, uint64_t *out, cl_uint rounds);

/* TEST-ONLY: the split logic rounds ("logic_split") of the scene's last wavefront frame.  listed[r] for r < n: the paths round r listed
 * for its shade pass, summed over the tile groups, as the last shade pass of that round logged it (a planned frame that skips the launch
 * because its plan says 0 logs nothing; rounds the frame did not issue read 0).  Call after the frame was synchronised.  Returns the
 * number of logic rounds the frame issued as answer + shade launches, over its sample batches and tile groups (0: none was split), -1
 * for invalid arguments. */
int rtHipTestShadeLog(const rtHipScene *scene, cl_uint *listed, cl_uint n);

/* TEST-ONLY: direct placement ("place_direct") in the scene's last wavefront frame, over its sample batches and tile groups: out[0] = the
 * ordered rounds whose entries the logic kernel wrote at their sorted positions from the round's placement table, out[1] = the scatter
 * launches the frame issued (a frame rendered again reports the watched frame that replaced it).  Returns 0, -1 for NULL.
 * rtHipTestPlaceView: of the scene's first tile group after a synchronisation -- table (may be NULL): the RT_PLACE_TABLE_WORDS words of
 * round `round`'s placement table as the last scatter launch of that round recorded it, 64 classes x 32 copies cells {first sorted position,
 * entries}, class-major, then the total, the slices and the segment length of the round's layout and a spare word; entries (may be NULL):
 * the first `positions` 64-byte trace entries of the entry array of the round's parity, 16 words each, word 0 = the entry's queue slot.
 * round is in 1 .. RT_PLACE_TABLE_ROUNDS.  Returns 0, -1 for invalid arguments. */
enum { RT_PLACE_TABLE_ROUNDS = 8, RT_PLACE_TABLE_WORDS = 2 * 64 * 32 + 4 };
int rtHipTestPlaceLog(const rtHipScene *scene, cl_uint out[2]);
int rtHipTestPlaceView(const rtHipScene *scene, cl_uint round, cl_uint *table, cl_uint *entries, cl_uint positions);

/* TEST-ONLY: what the calling thread's last device list builds did (rtHipBuildCameraListDevice, rtHipBuildSceneGridDevice; each
 * clears and fills its own fields), so that tests can prove which paths ran.  out[i] for i < n in the order of RT_BUILD_LOG_*:
 * camera triangles rasterised by one thread / by a workgroup (clipped rectangle above 1024 pixels), camera list entries before the
 * de-duplication; grid triangles filled by one thread / handed to workgroups, workgroup batches, first and final key capacity,
 * 1 when the key buffer grew for the big triangles, fill attempts (2 after the first fill overflowed), (cell, triangle) pairs.  The
 * grid's per-attempt fields are the last attempt's.  Fields past RT_BUILD_LOG_FIELDS read 0.  Returns RT_BUILD_LOG_FIELDS, -1 for
 * invalid arguments. */
enum { RT_BUILD_LOG_CAM_THREAD = 0, RT_BUILD_LOG_CAM_GROUP, RT_BUILD_LOG_CAM_ENTRIES, RT_BUILD_LOG_GRID_THREAD, RT_BUILD_LOG_GRID_GROUP,
       RT_BUILD_LOG_GRID_BATCHES, RT_BUILD_LOG_KEY_CAP_FIRST, RT_BUILD_LOG_KEY_CAP_FINAL, RT_BUILD_LOG_GREW, RT_BUILD_LOG_ATTEMPTS,
       RT_BUILD_LOG_PAIRS, RT_BUILD_LOG_FIELDS };
int rtHipTestBuildLog(uint64_t *out, cl_uint n);

/* TEST-ONLY: copies elements [firstElement, firstElement + count) of one of a resident scene's device arrays -- what the scene upload
 * (rt_scene_prep.hip, rt_prepare_triangles, rt_gather_pair_records) left for the kernels -- to host memory, after synchronising the
 * scene's stream.  `what` and the element of each array:
 *   RT_SCENE_VIEW_HEADER     cl_uint: planesTame, tileCount, tilesX, triangleCount, pair count (5 elements)
 *   RT_SCENE_VIEW_CAM_START  cl_uint: tile-major range starts, index slot*128*128 + ly*128 + lx (tileCount*128*128 elements)
 *   RT_SCENE_VIEW_CAM_END    cl_uint: the range ends, same index
 *   RT_SCENE_VIEW_TRI_REC    16 floats (64 bytes): a triangle's intersection record (triangleCount elements)
 *   RT_SCENE_VIEW_TRI_SHADE  24 floats (96 bytes): the packed words of a triangle's shading row -- b c | nA nB nC | uvA uvB uvC | material
 *                            id | two zero words -- gathered from the device's 128-byte rows
 *   RT_SCENE_VIEW_TRI_SHADE_ROW 32 floats (128 bytes): the shading row as the device stores it, one line per triangle: the 24 words above,
 *                            then the first four floats of the triangle's RT_SCENE_VIEW_TRI_REC record (vertex a, ab.x), then four zero words
 *   RT_SCENE_VIEW_GRID_BITS  uint64_t: the occupancy word of a 4x4x4 block, block (cx>>2) + 64*(cy>>2) + 4096*(cz>>2) (64^3 elements)
 *   RT_SCENE_VIEW_BLOCK_SPARSE cl_uint: the block table {word lo, word hi, rank}, entry 3*((cx>>2) | (cy>>2)<<8 | (cz>>2)<<16)
 *                            (3 * ((63<<16 | 63<<8 | 63) + 1) elements)
 *   RT_SCENE_VIEW_PAIR_REC   16 32-bit words (64 bytes): a (cell, triangle) pair record (pair count elements)
 *   RT_SCENE_VIEW_CELL_LUT   one byte: the cell estimate table [3][256]
 *   RT_SCENE_VIEW_CLIP_PLANES 4 floats: a plane {n.xyz, off} of the grid's clip bound -- every corner of every occupied cell has n.x <= off (at
 *                            most 8 elements, none for a scene whose occupied cells fill the grid's box; kept whatever "ray_clip" says),
 *                            read from behind the split planes on the device, where the planning kernels read them
 *   RT_SCENE_VIEW_CLIP_APPLIED cl_uint: how many of those planes the planning kernels apply, the word in front of them on the device (1
 *                            element: the number kept, or 0 for a scene built with "ray_clip" 0)
 * With out == NULL it returns the array's element count (firstElement and count are ignored); otherwise 0, or -1 with a
 * rtHipLastError() text for a NULL scene, an unknown `what`, a range that reaches past the array's end or a HIP failure. */
enum { RT_SCENE_VIEW_HEADER = 0, RT_SCENE_VIEW_CAM_START, RT_SCENE_VIEW_CAM_END, RT_SCENE_VIEW_TRI_REC, RT_SCENE_VIEW_TRI_SHADE,
       RT_SCENE_VIEW_GRID_BITS, RT_SCENE_VIEW_BLOCK_SPARSE, RT_SCENE_VIEW_PAIR_REC, RT_SCENE_VIEW_CELL_LUT, RT_SCENE_VIEWS,
       RT_SCENE_VIEW_CLIP_PLANES = 16, RT_SCENE_VIEW_CLIP_APPLIED /* (parts of the planes' buffer, numbered apart from the arrays 0 .. RT_SCENE_VIEWS - 1) */,
       RT_SCENE_VIEW_TRI_SHADE_ROW /* (18: another view of array RT_SCENE_VIEW_TRI_SHADE) */ };
int rtHipTestSceneView(const rtHipScene *scene, int what, uint64_t firstElement, uint64_t count, void *out);

/* TEST-ONLY, for rtHipSceneSetCamera.  rtHipTestSceneCameraList copies entries [first, first + count) of the scene's device camera list
 * (the one its ranges, RT_SCENE_VIEW_CAM_START / _END, index) after synchronising the scene's stream; with out == NULL it returns the
 * entry count.  rtHipTestScenePointers gives the device addresses of triRec, triShade, gridBlockSparse, pairRec, matRec and lightPos, so
 * that a test can show a move leaves them where they were.  rtHipTestSceneCameraLog gives, for the scene's last successful move:
 * triangles rasterised by one thread, triangles handed to workgroups (clipped rectangle above 1024 pixels), list entries (zeros before
 * the first move; a move does not write rtHipTestBuildLog's fields).  rtHipTestSceneCameraTimes gives that move's device time in
 * milliseconds: [0] projection, count pass and total, [1] scan, fill pass and per-pixel order (HIP events on the scene's stream; the
 * host's look at the total lies between the two).  Each returns 0, or -1 with a rtHipLastError() text. */
int rtHipTestSceneCameraList(const rtHipScene *scene, uint64_t first, uint64_t count, cl_uint *out);
int rtHipTestScenePointers(const rtHipScene *scene, const void *out[6]);
int rtHipTestSceneCameraLog(const rtHipScene *scene, uint64_t out[3]);
int rtHipTestSceneCameraTimes(const rtHipScene *scene, double out[2]);

/* TEST-ONLY, for rtHipSceneSetGeometry.  rtHipTestSceneGeometryLog gives, for the scene's last successful update, out[i] for i < n:
 * triangles whose cells one thread filled, triangles handed to workgroups, fill attempts (2 after the first fill overflowed its key
 * buffer), (cell, triangle) pairs, camera list entries, and 1 when any device buffer was allocated or replaced by that update (zeros
 * before the first update; fields past the sixth read 0); it returns 6.  rtHipTestSceneGeometryTimes gives that update's time on the
 * scene's stream in milliseconds, from HIP events: [0] index check and records, [1] grid, [2] dense view and pair gather, [3] camera
 * lists; the host's looks at counters lie inside the stages.  -1 with a rtHipLastError() text for a NULL argument. */
int rtHipTestSceneGeometryLog(const rtHipScene *scene, uint64_t *out, cl_uint n);
int rtHipTestSceneGeometryTimes(const rtHipScene *scene, double ms[4]);

#ifdef __cplusplus
}
#endif
#endif /* RAYTRACE_HIP_H */
