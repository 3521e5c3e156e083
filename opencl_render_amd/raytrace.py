"""ctypes binding of libraytrace_hip.so (the C ABI in include/raytrace_hip.h).

This is the stub a Python host would write against the library; it mirrors the reference's own interface for the
hot path (``RaytraceAll`` and friends, reference ``source/opencl/raytrace.h:37-106``) name for name, and adds the
resident layer (``rtHip*``).  There is no fallback: if the shared library is missing the import of this module's
``lib()`` raises, and on a machine without a HIP device every computing call returns failure.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from .scene import GRID_DIV, Scene

_HERE = os.path.dirname(os.path.abspath(__file__))
# RT_HIP_LIB selects another build of the same library (kernel A/B experiments); default is the in-tree build.
LIB_PATH = os.environ.get("RT_HIP_LIB") or os.path.join(_HERE, "libraytrace_hip.so")
TILE = 128
PIPELINE_MEGAKERNEL, PIPELINE_WAVEFRONT = 0, 1
PASS_ALPHA, PASS_DEPTH, PASS_TRIANGLE, PASS_NORMAL, PASS_ALBEDO = 1, 2, 4, 8, 16  # RT_HIP_PASS_*


class Float3(C.Structure):  # cl_float3 == cl_float4: 16 bytes, passed as two SSE eightbytes on SysV
    _fields_ = [("s", C.c_float * 4)]


class UInt2(C.Structure):
    _fields_ = [("s", C.c_uint32 * 2)]


class SceneDesc(C.Structure):  # rtHipSceneDesc
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("eye", C.c_float * 4), ("eyeToTopLeft", C.c_float * 4), ("leftToRight", C.c_float * 4), ("topToBottom", C.c_float * 4),
        ("pixelSizeInv", C.c_float),
        ("camStart", C.c_void_p), ("camEnd", C.c_void_p), ("camList", C.c_void_p),
        ("camListSize", C.c_uint64),
        ("sampleCount", C.c_uint32),
        ("vertexCount", C.c_uint32), ("vertex", C.c_void_p),
        ("triangleCount", C.c_uint32), ("triIndex", C.c_void_p), ("triMaterial", C.c_void_p), ("triUv", C.c_void_p), ("triNormal", C.c_void_p),
        ("axesDiv", C.c_int32), ("boxMin", C.c_void_p), ("gridStart", C.c_void_p), ("gridList", C.c_void_p),
        ("materialCount", C.c_uint32), ("matSize", C.c_void_p), ("matStart", C.c_void_p),
        ("texturesSize", C.c_uint32), ("textures", C.c_void_p),
        ("lightCount", C.c_uint32), ("lightType", C.c_void_p), ("lightPos", C.c_void_p), ("lightDir", C.c_void_p), ("lightCol", C.c_void_p),
        ("lightRadius", C.c_void_p), ("lightHalfAtt", C.c_void_p),
        ("arraysOnDevice", C.c_int32),
    ]


class Ray(C.Structure):  # rtHipRay: 32 bytes
    _fields_ = [("o", C.c_float * 3), ("tmin", C.c_float), ("d", C.c_float * 3), ("tmax", C.c_float)]


class Hit(C.Structure):  # rtHipHit: 16 bytes
    _fields_ = [("t", C.c_float), ("triangle", C.c_uint32), ("abL", C.c_float), ("acL", C.c_float)]


class DenoiseParams(C.Structure):  # rtHipDenoiseParams
    _fields_ = [("iterations", C.c_uint32), ("colourInvSigma2", C.c_float), ("albedoInvSigma2", C.c_float), ("normalPowerLog2", C.c_uint32)]


# rtHipDenoiseDefaults (include/raytrace_hip.h, "DENOISER"; DESIGN.md says why these values)
DENOISE_DEFAULTS = dict(iterations=4, colour_inv_sigma2=4.0, albedo_inv_sigma2=100.0, normal_power_log2=7)


class TemporalParams(C.Structure):  # rtHipTemporalParams
    _fields_ = [("maxHistory", C.c_float), ("depthTolerance", C.c_float)]


# rtHipTemporalDefaults (include/raytrace_hip.h, "TEMPORAL ACCUMULATION")
TEMPORAL_DEFAULTS = dict(max_history=32.0, depth_tolerance=0.05)


class VarianceParams(C.Structure):  # rtHipVarianceParams
    _fields_ = [("iterations", C.c_uint32), ("luminanceSigma2", C.c_float), ("varianceFloor", C.c_float), ("albedoInvSigma2", C.c_float),
                ("normalPowerLog2", C.c_uint32), ("spatialBelow", C.c_float)]


# rtHipVarianceDefaults (include/raytrace_hip.h, "VARIANCE-GUIDED FILTER"; DESIGN.md says why these values)
VARIANCE_DEFAULTS = dict(iterations=4, luminance_sigma2=4.0, variance_floor=1e-8, albedo_inv_sigma2=100.0, normal_power_log2=7,
                         spatial_below=4.0)


class TemporalClampParams(C.Structure):  # rtHipTemporalClampParams
    _fields_ = [("mode", C.c_uint32), ("gamma", C.c_float)]


# rtHipTemporalClampDefaults (include/raytrace_hip.h, "TEMPORAL CLAMP"); the modes by name, as the command line takes them
TEMPORAL_CLAMP_DEFAULTS = dict(mode=3, gamma=1.0)
TEMPORAL_CLAMP_MODES = dict(minmax=1, variance=2, both=3)


class MotionBlurParams(C.Structure):  # rtHipMotionBlurParams
    _fields_ = [("shutter", C.c_float), ("maxBlur", C.c_float), ("taps", C.c_uint32), ("depthSoftness", C.c_float)]


# rtHipMotionBlurDefaults (include/raytrace_hip.h, "MOTION BLUR")
MOTION_BLUR_DEFAULTS = dict(shutter=0.5, max_blur=16.0, taps=15, depth_softness=0.05)


class DofParams(C.Structure):  # rtHipDepthOfFieldParams
    _fields_ = [("focus", C.c_float), ("cocScale", C.c_float), ("maxCoc", C.c_float), ("rings", C.c_uint32), ("depthSoftness", C.c_float)]


# rtHipDepthOfFieldDefaults (include/raytrace_hip.h, "DEPTH OF FIELD")
DEPTH_OF_FIELD_DEFAULTS = dict(focus=1.0, coc_scale=8.0, max_coc=16.0, rings=3, depth_softness=0.05)


class AoParams(C.Structure):  # rtHipAoParams
    _fields_ = [("raysPerHit", C.c_uint32), ("pixelSamples", C.c_uint32), ("radius", C.c_float), ("seed", C.c_uint32)]


# rtHipAoDefaults (include/raytrace_hip.h, "AMBIENT OCCLUSION")
AO_DEFAULTS = dict(rays=16, radius=float("inf"), pixel_samples=1, seed=0)


class MatteParams(C.Structure):  # rtHipMatteParams
    _fields_ = [("kind", C.c_uint32), ("total", C.c_uint32), ("first", C.c_uint32), ("samples", C.c_uint32), ("selectCount", C.c_uint32),
                ("select", C.c_uint32 * 16), ("layers", C.c_uint32)]


# RT_HIP_MATTE_* (include/raytrace_hip.h, "MATTES"); "mesh" is kind GROUP with scene.tri_mesh as the table
MATTE_KINDS = dict(triangle=0, material=1, group=2)
MATTE_NONE = 0xFFFFFFFF
MATTE_MAX_SELECT, MATTE_MAX_LAYERS = 16, 8


class BakeParams(C.Structure):  # rtHipBakeParams
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("raysPerTexel", C.c_uint32), ("radius", C.c_float), ("seed", C.c_uint32),
                ("dilate", C.c_uint32), ("firstTriangle", C.c_uint32), ("triangleCount", C.c_uint32), ("material", C.c_int32),
                ("matchMaterial", C.c_uint32)]


# rtHipBakeDefaults (include/raytrace_hip.h, "AMBIENT OCCLUSION BAKE"); triangleCount ALL_TRIANGLES = first .. T - 1
BAKE_DEFAULTS = dict(rays=16, radius=float("inf"), seed=0, dilate=2)
ALL_TRIANGLES = 0xFFFFFFFF


class Camera(C.Structure):  # rtHipCamera
    _fields_ = [("eye", C.c_float * 4), ("eyeToTopLeft", C.c_float * 4), ("leftToRight", C.c_float * 4), ("topToBottom", C.c_float * 4),
                ("pixelSizeInv", C.c_float)]


class SampleWindow(C.Structure):  # rtHipSampleWindow
    _fields_ = [(n, C.c_uint32) for n in ("total", "first", "divisor", "accumulate", "advance")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class GeometryUpdate(C.Structure):  # rtHipGeometryUpdate
    _fields_ = [("vertexCount", C.c_uint32), ("vertex", C.c_void_p), ("triIndex", C.c_void_p), ("triNormal", C.c_void_p), ("arraysOnDevice", C.c_int32)]


class Lights(C.Structure):  # rtHipLights
    _fields_ = [("lightCount", C.c_uint32), ("lightType", C.c_void_p), ("lightPos", C.c_void_p), ("lightDir", C.c_void_p), ("lightCol", C.c_void_p),
                ("lightRadius", C.c_void_p), ("lightHalfAtt", C.c_void_p)]


class MaterialUpdate(C.Structure):  # rtHipMaterialUpdate
    _fields_ = [("replaceMaterials", C.c_int32), ("materialCount", C.c_uint32), ("matSize", C.c_void_p), ("matStart", C.c_void_p),
                ("texturesSize", C.c_uint32), ("textures", C.c_void_p), ("triMaterial", C.c_void_p), ("triMaterialOnDevice", C.c_int32)]


class Stats(C.Structure):  # rtHipStats
    _fields_ = [(n, C.c_uint64) for n in ("primarySamples", "primaryCandidates", "gridRays", "gridCells", "gridCandidates", "shadedHits", "texelFetches")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# Every symbol include/raytrace_hip.h declares, in declaration order (tests check the library exports them all).
DROPIN_SYMBOLS = [
    "RaytraceAll", "InitOpenCL", "ResetComputationType", "GetIsComputationTypeUpdated", "GetComputationTypeCount",
    "GetComputationTypeName", "GetProgress", "SetProgress", "GetStartTime", "GetEndTime", "ResetTime",
    "dot", "cross", "normalize", "vector", "bindf", "GetPointToLineSqLen", "RayIntersectsTriangle", "GetBoxAddress",
]
RESIDENT_SYMBOLS = [
    "rtHipCacheClear", "rtHipDeviceCount", "rtHipLastError", "rtHipSceneCreate", "rtHipSceneCreateLike", "rtHipSceneDestroy", "rtHipSceneBytes", "rtHipSceneGetCamera", "rtHipSceneSetCamera", "rtHipSceneSetGeometry",
    "rtHipLightsCheck", "rtHipMaterialsCheck", "rtHipSceneSetLights", "rtHipSceneSetMaterials", "rtHipSceneEditTimes", "rtHipRenderTiles", "rtHipFrameFinish",
    "rtHipSampleWindowCheck", "rtHipSceneSetSampleWindow", "rtHipSceneGetSampleWindow",
    "rtHipSetPipeline", "rtHipStageTiming", "rtHipStageTimes", "rtHipDebugCounters",
    "rtHipRenderTilesCounted", "rtHipTileBuffer", "rtHipTileBufferBytes", "rtHipDetile", "rtHipDetileStore", "rtHipDeviceAlloc", "rtHipDeviceFree", "rtHipDeviceCopy", "rtHipReadback", "rtHipSync",
    "rtHipScenePasses", "rtHipPassBuffer", "rtHipPassBufferBytes", "rtHipReadbackPasses",
    "rtHipSurfaceBuffer", "rtHipSurfaceBufferBytes", "rtHipReadbackSurfacePasses",
    "rtHipSceneIntersect", "rtHipSceneIntersectDevice",
    "rtHipDenoiseDefaults", "rtHipDenoiseScratchBytes", "rtHipDenoiseDevice", "rtHipDenoise", "rtHipSceneDenoise", "rtHipSceneDenoiseTimes",
    "rtHipAoDefaults", "rtHipSceneAmbientOcclusion", "rtHipSceneAmbientOcclusionDevice",
    "rtHipSceneMotionMark", "rtHipSceneMotionReferenceCamera", "rtHipSceneMotion", "rtHipSceneMotionDevice",
    "rtHipMatteCheck", "rtHipMatteDefaults", "rtHipSceneSetMatteGroups", "rtHipSceneMattes", "rtHipSceneMattesDevice", "rtHipSceneMatteTimes",
    "rtHipTemporalDefaults", "rtHipTemporalDevice", "rtHipTemporal", "rtHipSceneTemporal", "rtHipSceneTemporalReset", "rtHipSceneTemporalTimes",
    "rtHipVarianceDefaults", "rtHipTemporalMomentsDevice", "rtHipTemporalMoments", "rtHipVarianceScratchBytes", "rtHipDenoiseVarianceDevice",
    "rtHipDenoiseVariance", "rtHipSceneTemporalVariance",
    "rtHipTemporalClampDefaults", "rtHipTemporalClampCheck", "rtHipTemporalClampDevice", "rtHipTemporalClamp", "rtHipTemporalMomentsClampDevice",
    "rtHipTemporalMomentsClamp", "rtHipSceneSetTemporalClamp", "rtHipSceneGetTemporalClamp",
    "rtHipMotionBlurDefaults", "rtHipMotionBlurCheck", "rtHipMotionBlurScratchBytes", "rtHipMotionBlurDevice", "rtHipMotionBlur",
    "rtHipSceneMotionBlur", "rtHipSceneMotionBlurTimes",
    "rtHipDepthOfFieldDefaults", "rtHipDepthOfFieldCheck", "rtHipDepthOfFieldScratchBytes", "rtHipDepthOfFieldDevice", "rtHipDepthOfField",
    "rtHipSceneDepthOfField", "rtHipSceneDepthOfFieldTimes", "rtHipDepthOfFieldLens",
    "rtHipBakeDefaults", "rtHipSceneBakeAmbientOcclusion", "rtHipSceneBakeAmbientOcclusionDevice",
    "rtHipKernelTime", "rtHipBuildCameraList", "rtHipBuildCameraListDevice", "rtHipBuildSceneGrid", "rtHipBuildSceneGridDevice", "rtHipFree",
    "rtHipDeviceKat", "rtHipTune", "rtHipTestCachePointers", "rtHipTestHashBytes", "rtHipScenePathClass", "rtHipTestPathClass", "rtHipTestRoundLog", "rtHipTestRoundVisits", "rtHipTestShadeLog", "rtHipTestPlaceLog", "rtHipTestPlaceView", "rtHipTestBuildLog",
    "rtHipTestShadeKat", "rtHipTestSceneView", "rtHipTestSceneCameraList", "rtHipTestScenePointers", "rtHipTestSceneCameraLog", "rtHipTestSceneCameraTimes",
    "rtHipTestSceneGeometryLog", "rtHipTestSceneGeometryTimes",
    "rtHipSetCamera", "rtHipMeshCount", "rtHipMeshFill", "rtHipLightFill", "rtHipBakeMaterials", "rtHipPlanesToRgb8", "rtHipWriteBmp", "rtHipWritePpm", "rtHipWritePgm", "rtHipWritePfm", "rtHipWritePfmRgb",
    "rtHipObjRead", "rtHipObjFree", "rtHipImageRead", "rtHipProjectUv",
]

_lib = None


def lib() -> C.CDLL:
    """Loads libraytrace_hip.so (built by ``__graft_entry__.build()`` / ``make -C opencl_render_amd/csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the HIP path)")
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_float
    L.RaytraceAll.restype = u32
    L.RaytraceAll.argtypes = [u32, UInt2, Float3, Float3, Float3, Float3, f32, vp, vp, vp, C.c_ssize_t, u32, u32, vp, u32, vp, vp, vp, vp,
                              i32, vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.InitOpenCL.restype = None
    L.ResetComputationType.restype = None
    L.GetIsComputationTypeUpdated.restype = u32
    L.GetComputationTypeCount.restype = C.c_size_t
    L.GetComputationTypeName.restype = u32
    L.GetComputationTypeName.argtypes = [C.c_size_t, C.c_size_t, C.c_char_p]
    L.GetProgress.restype = f32
    L.SetProgress.argtypes = [f32]
    L.GetStartTime.restype = C.c_long
    L.GetEndTime.restype = C.c_long
    L.dot.restype = f32
    L.dot.argtypes = [Float3, Float3]
    L.cross.restype = Float3
    L.cross.argtypes = [Float3, Float3]
    L.normalize.restype = Float3
    L.normalize.argtypes = [Float3]
    L.vector.restype = Float3
    L.vector.argtypes = [Float3, Float3]
    L.bindf.restype = f32
    L.bindf.argtypes = [f32, f32, f32]
    L.GetPointToLineSqLen.restype = f32
    L.GetPointToLineSqLen.argtypes = [Float3, Float3, Float3]
    L.RayIntersectsTriangle.restype = u32
    L.RayIntersectsTriangle.argtypes = [Float3, Float3, f32, f32, Float3, Float3, Float3, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32)]
    L.GetBoxAddress.restype = type("Int3", (C.Structure,), {"_fields_": [("s", C.c_int32 * 4)]})
    L.GetBoxAddress.argtypes = [i32, vp, Float3]

    L.rtHipCacheClear.restype = None
    L.rtHipDeviceCount.restype = C.c_int
    L.rtHipLastError.restype = C.c_char_p
    L.rtHipSceneCreate.restype = vp
    L.rtHipSceneCreate.argtypes = [C.c_int, C.POINTER(SceneDesc), vp, u32]
    L.rtHipSceneCreateLike.restype = vp
    L.rtHipSceneCreateLike.argtypes = [C.c_int, C.POINTER(SceneDesc), vp, u32, vp]
    L.rtHipSceneDestroy.argtypes = [vp]
    L.rtHipSceneDestroy.restype = None
    L.rtHipSceneBytes.restype = u64
    L.rtHipSceneBytes.argtypes = [vp]
    L.rtHipSceneGetCamera.argtypes = [vp, C.POINTER(Camera)]
    L.rtHipSceneSetCamera.argtypes = [vp, C.POINTER(Camera)]
    L.rtHipTestSceneCameraList.argtypes = [vp, u64, u64, vp]
    L.rtHipTestScenePointers.argtypes = [vp, C.POINTER(vp * 6)]
    L.rtHipTestSceneCameraLog.argtypes = [vp, C.POINTER(u64 * 3)]
    L.rtHipTestSceneCameraTimes.argtypes = [vp, C.POINTER(C.c_double * 2)]
    L.rtHipSceneSetGeometry.argtypes = [vp, C.POINTER(GeometryUpdate)]
    L.rtHipTestSceneGeometryLog.argtypes = [vp, C.POINTER(u64 * 6), u32]
    L.rtHipTestSceneGeometryTimes.argtypes = [vp, C.POINTER(C.c_double * 4)]
    L.rtHipLightsCheck.argtypes = [C.POINTER(Lights)]
    L.rtHipMaterialsCheck.argtypes = [C.POINTER(MaterialUpdate)]
    L.rtHipSceneSetLights.argtypes = [vp, C.POINTER(Lights)]
    L.rtHipSceneSetMaterials.argtypes = [vp, C.POINTER(MaterialUpdate)]
    L.rtHipSceneEditTimes.argtypes = [vp, C.POINTER(C.c_double * 3)]
    L.rtHipRenderTiles.argtypes = [vp, vp]
    L.rtHipFrameFinish.argtypes = [vp, C.POINTER(C.c_int)]
    L.rtHipSampleWindowCheck.argtypes = [u32, C.POINTER(SampleWindow)]
    L.rtHipSceneSetSampleWindow.argtypes = [vp, C.POINTER(SampleWindow)]
    L.rtHipSceneGetSampleWindow.argtypes = [vp, C.POINTER(SampleWindow), C.POINTER(SampleWindow)]
    L.rtHipRenderTilesCounted.argtypes = [vp, C.POINTER(Stats)]
    L.rtHipDebugCounters.argtypes = [vp, C.POINTER(C.c_uint64 * 8), C.c_int]
    L.rtHipSetPipeline.argtypes = [vp, C.c_int]
    L.rtHipStageTiming.argtypes = [vp, C.c_int]
    L.rtHipStageTimes.argtypes = [vp, C.POINTER(C.c_double * 5), C.POINTER(u64)]
    L.rtHipTileBuffer.restype = vp
    L.rtHipTileBuffer.argtypes = [vp]
    L.rtHipTileBufferBytes.restype = u64
    L.rtHipTileBufferBytes.argtypes = [vp]
    L.rtHipDetile.argtypes = [C.c_int, vp, vp, u32, u32, u32, vp, vp, vp, vp]
    L.rtHipDetileStore.argtypes = [C.c_int, vp, vp, u32, u32, u32, vp, vp, vp, vp]
    L.rtHipReadback.argtypes = [vp, vp, vp, vp]
    L.rtHipDeviceAlloc.restype = vp
    L.rtHipDeviceAlloc.argtypes = [C.c_int, u64]
    L.rtHipDeviceFree.restype = None
    L.rtHipDeviceFree.argtypes = [C.c_int, vp]
    L.rtHipDeviceCopy.argtypes = [C.c_int, vp, vp, u64, C.c_int]
    L.rtHipSync.argtypes = [vp, vp]
    L.rtHipScenePasses.argtypes = [vp, u32]
    L.rtHipPassBuffer.restype = vp
    L.rtHipPassBuffer.argtypes = [vp]
    L.rtHipPassBufferBytes.restype = u64
    L.rtHipPassBufferBytes.argtypes = [vp]
    L.rtHipReadbackPasses.argtypes = [vp, vp, vp, vp]
    L.rtHipSurfaceBuffer.restype = vp
    L.rtHipSurfaceBuffer.argtypes = [vp]
    L.rtHipSurfaceBufferBytes.restype = u64
    L.rtHipSurfaceBufferBytes.argtypes = [vp]
    L.rtHipReadbackSurfacePasses.argtypes = [vp, vp, vp]
    L.rtHipSceneIntersect.argtypes = [vp, vp, vp, u32, vp]
    L.rtHipSceneIntersectDevice.argtypes = [vp, vp, vp, u32, vp, vp]
    L.rtHipDenoiseDefaults.restype = None
    L.rtHipDenoiseDefaults.argtypes = [C.POINTER(DenoiseParams)]
    L.rtHipDenoiseScratchBytes.restype = u64
    L.rtHipDenoiseScratchBytes.argtypes = [u32, u32]
    L.rtHipDenoiseDevice.argtypes = [C.c_int, u32, u32, vp, vp, vp, vp, vp, u64, C.POINTER(DenoiseParams), vp]
    L.rtHipDenoise.argtypes = [C.c_int, u32, u32, vp, vp, vp, vp, C.POINTER(DenoiseParams)]
    L.rtHipSceneDenoise.argtypes = [vp, C.POINTER(DenoiseParams), vp, vp, vp, vp]
    L.rtHipSceneDenoiseTimes.argtypes = [vp, C.POINTER(C.c_float)]
    L.rtHipAoDefaults.restype = None
    L.rtHipAoDefaults.argtypes = [C.POINTER(AoParams)]
    L.rtHipSceneAmbientOcclusion.argtypes = [vp, C.POINTER(AoParams), vp]
    L.rtHipSceneAmbientOcclusionDevice.argtypes = [vp, C.POINTER(AoParams), vp, vp]
    L.rtHipSceneMotionMark.argtypes = [vp]
    L.rtHipSceneMotionReferenceCamera.argtypes = [vp, C.POINTER(Camera)]
    L.rtHipSceneMotion.argtypes = [vp, vp, vp, vp, vp]
    L.rtHipSceneMotionDevice.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rtHipMatteCheck.argtypes = [C.POINTER(MatteParams)]
    L.rtHipMatteDefaults.argtypes = [vp, C.POINTER(MatteParams)]
    L.rtHipSceneSetMatteGroups.argtypes = [vp, vp, i32]
    L.rtHipSceneMattes.argtypes = [vp, C.POINTER(MatteParams), vp, vp, vp, vp]
    L.rtHipSceneMattesDevice.argtypes = [vp, C.POINTER(MatteParams), vp, vp, vp, vp, vp]
    L.rtHipSceneMatteTimes.argtypes = [vp, C.POINTER(C.c_double * 2)]
    L.rtHipTemporalDefaults.restype = None
    L.rtHipTemporalDefaults.argtypes = [C.POINTER(TemporalParams)]
    L.rtHipTemporalDevice.argtypes = [C.c_int, u32, u32] + [vp] * 10 + [C.POINTER(TemporalParams), vp]
    L.rtHipTemporal.argtypes = [C.c_int, u32, u32] + [vp] * 10 + [C.POINTER(TemporalParams)]
    L.rtHipSceneTemporal.argtypes = [vp, C.POINTER(TemporalParams), C.POINTER(DenoiseParams), vp, vp, vp, vp, vp]
    L.rtHipSceneTemporalReset.argtypes = [vp]
    L.rtHipSceneTemporalTimes.argtypes = [vp, C.POINTER(C.c_float)]
    L.rtHipVarianceDefaults.restype = None
    L.rtHipVarianceDefaults.argtypes = [C.POINTER(VarianceParams)]
    L.rtHipTemporalMomentsDevice.argtypes = [C.c_int, u32, u32] + [vp] * 13 + [C.POINTER(TemporalParams), vp]
    L.rtHipTemporalMoments.argtypes = [C.c_int, u32, u32] + [vp] * 13 + [C.POINTER(TemporalParams)]
    L.rtHipVarianceScratchBytes.restype = C.c_uint64
    L.rtHipVarianceScratchBytes.argtypes = [u32, u32]
    L.rtHipDenoiseVarianceDevice.argtypes = [C.c_int, u32, u32] + [vp] * 8 + [C.c_uint64, C.POINTER(VarianceParams), vp]
    L.rtHipDenoiseVariance.argtypes = [C.c_int, u32, u32] + [vp] * 7 + [C.POINTER(VarianceParams)]
    L.rtHipSceneTemporalVariance.argtypes = [vp, C.POINTER(TemporalParams), C.POINTER(VarianceParams), vp, vp, vp, vp, vp, vp]
    clamp = C.POINTER(TemporalClampParams)
    L.rtHipTemporalClampDefaults.restype = None
    L.rtHipTemporalClampDefaults.argtypes = [clamp]
    L.rtHipTemporalClampCheck.argtypes = [clamp]
    L.rtHipTemporalClampDevice.argtypes = [C.c_int, u32, u32] + [vp] * 10 + [C.POINTER(TemporalParams), clamp, vp]
    L.rtHipTemporalClamp.argtypes = [C.c_int, u32, u32] + [vp] * 10 + [C.POINTER(TemporalParams), clamp]
    L.rtHipTemporalMomentsClampDevice.argtypes = [C.c_int, u32, u32] + [vp] * 13 + [C.POINTER(TemporalParams), clamp, vp]
    L.rtHipTemporalMomentsClamp.argtypes = [C.c_int, u32, u32] + [vp] * 13 + [C.POINTER(TemporalParams), clamp]
    L.rtHipSceneSetTemporalClamp.argtypes = [vp, clamp]
    L.rtHipSceneGetTemporalClamp.argtypes = [vp, clamp]
    blur = C.POINTER(MotionBlurParams)
    L.rtHipMotionBlurDefaults.restype = None
    L.rtHipMotionBlurDefaults.argtypes = [blur]
    L.rtHipMotionBlurCheck.argtypes = [blur]
    L.rtHipMotionBlurScratchBytes.restype = C.c_uint64
    L.rtHipMotionBlurScratchBytes.argtypes = [u32, u32]
    L.rtHipMotionBlurDevice.argtypes = [C.c_int, u32, u32, vp, vp, vp, vp, vp, u64, blur, vp]
    L.rtHipMotionBlur.argtypes = [C.c_int, u32, u32, vp, vp, vp, vp, blur]
    L.rtHipSceneMotionBlur.argtypes = [vp, blur, vp, vp, vp, vp]
    L.rtHipSceneMotionBlurTimes.argtypes = [vp, C.POINTER(C.c_float)]
    dof = C.POINTER(DofParams)
    L.rtHipDepthOfFieldDefaults.restype = None
    L.rtHipDepthOfFieldDefaults.argtypes = [dof]
    L.rtHipDepthOfFieldCheck.argtypes = [dof]
    L.rtHipDepthOfFieldScratchBytes.restype = C.c_uint64
    L.rtHipDepthOfFieldScratchBytes.argtypes = [u32, u32]
    L.rtHipDepthOfFieldDevice.argtypes = [C.c_int, u32, u32, vp, vp, vp, vp, u64, dof, vp]
    L.rtHipDepthOfField.argtypes = [C.c_int, u32, u32, vp, vp, vp, dof]
    L.rtHipSceneDepthOfField.argtypes = [vp, dof, vp, vp, vp, vp]
    L.rtHipSceneDepthOfFieldTimes.argtypes = [vp, C.POINTER(C.c_float)]
    L.rtHipDepthOfFieldLens.argtypes = [C.POINTER(Camera), C.c_float, C.c_float, dof]
    L.rtHipBakeDefaults.restype = None
    L.rtHipBakeDefaults.argtypes = [C.POINTER(BakeParams)]
    L.rtHipSceneBakeAmbientOcclusion.argtypes = [vp, C.POINTER(BakeParams), vp, vp]
    L.rtHipSceneBakeAmbientOcclusionDevice.argtypes = [vp, C.POINTER(BakeParams), vp, vp, vp]
    L.rtHipKernelTime.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64)]
    L.rtHipBuildCameraList.argtypes = [u32, u32, vp, vp, vp, vp, f32, u32, vp, vp, C.c_int,
                                       C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.rtHipBuildSceneGrid.argtypes = [u32, u32, vp, vp, C.c_int, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.rtHipBuildSceneGridDevice.argtypes = [C.c_int, u32, u32, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_double)]
    L.rtHipBuildCameraListDevice.argtypes = [C.c_int, u32, u32, vp, vp, vp, vp, f32, u32, u32, vp, vp,
                                             C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_double)]
    L.rtHipDeviceKat.argtypes = [C.c_int, C.c_int, u32, vp, u32, vp, u32, vp]
    L.rtHipTune.argtypes = [C.c_char_p, C.c_double]
    L.rtHipTestHashBytes.restype = u64
    L.rtHipTestHashBytes.argtypes = [vp, u64]
    L.rtHipScenePathClass.argtypes = [C.POINTER(SceneDesc)]
    L.rtHipTestPathClass.argtypes = [vp]
    L.rtHipTestRoundLog.argtypes = [vp, C.POINTER(u32), u32]
    L.rtHipTestRoundVisits.argtypes = [vp, C.POINTER(C.c_uint64), u32]
    L.rtHipTestShadeLog.argtypes = [vp, C.POINTER(u32), u32]
    L.rtHipTestPlaceLog.argtypes = [vp, C.POINTER(u32)]
    L.rtHipTestPlaceView.argtypes = [vp, u32, vp, vp, u32]
    L.rtHipTestBuildLog.argtypes = [C.POINTER(u64), u32]
    L.rtHipTestShadeKat.argtypes = [vp, C.c_int, u32, vp, vp]
    L.rtHipTestSceneView.argtypes = [vp, C.c_int, u64, u64, vp]
    L.rtHipFree.argtypes = [vp]
    L.rtHipFree.restype = None
    _lib = L
    return L


# The library itself reads no environment variables.  Sweep scripts and tests steer it through the RT_* variables of THIS
# process: they are translated into rtHipTune() calls whenever a scene is about to be built.
_ENV_KEYS = {
    "RT_HIP_STAGE_MB": "stage_mb", "RT_WF_EXTRA_FACTOR": "extra_factor", "RT_WF_STATE_MB": "state_mb", "RT_WF_GROUPS": "groups",
    "RT_WF_LOOKAHEAD": "lookahead", "RT_WF_FAST_QUOTIENT": "fast_quotient", "RT_WF_SPIN_LIMIT": "spin_limit",
    "RT_WF_APPEND_RAYS": "append_rays", "RT_WF_ORDERED_FIRST": "ordered_first", "RT_WF_SLICE_RAYS": "slice_rays", "RT_WF_SMALL_SLICES": "small_slices", "RT_WF_GROUP_RAYS": "group_rays",
    "RT_WF_BLOCKING": "blocking", "RT_WF_BATCH_PLAN": "batch_plan", "RT_WF_PLAN_ROUNDS": "plan_rounds", "RT_HIP_PIPELINE": "pipeline",
    "RT_HIP_TIMING": "timing", "RT_HIP_VIRTUAL_DEVICES": "virtual_devices", "RT_HIP_CACHE": "cache",
    "RT_WF_LOGIC_CLASS": "logic_class", "RT_WF_DEAD_SHADOW": "dead_shadow", "RT_WF_RAY_CLIP": "ray_clip", "RT_WF_LOGIC_SPLIT": "logic_split", "RT_WF_PLACE_DIRECT": "place_direct", "RT_WF_PLACE_SKEW": "place_skew", "RT_WF_PLAN_SHADE_SKIP": "plan_shade_skip", "RT_WF_VISIT_LOG": "visit_log",
    "RT_BUILD_KEY_CAP": "build_key_cap", "RT_BUILD_LIST_LIMIT": "build_list_limit", "RT_HIP_QUERY_RAYS": "query_rays",
    "RT_MATTE_CHUNK": "matte_chunk",
}
# comma-separated lists: RT_WF_SEG=a,b,.. sets seg0, seg1, .. (at most 5 values), RT_WF_SEG_RAYS sets seg_rays0.. (at most 4)
_ENV_LISTS = (("RT_WF_SEG", "seg", 5), ("RT_WF_SEG_RAYS", "seg_rays", 4))


def tune(key: str, value: float) -> None:
    if lib().rtHipTune(key.encode(), float(value)) != 0:
        raise ValueError(last_error())


def apply_env_tuning() -> None:
    """rtHipTune("reset") followed by one call per RT_* variable that is set in os.environ."""
    tune("reset", 0)
    for var, key in _ENV_KEYS.items():
        if var in os.environ:
            tune(key, float(os.environ[var]))
    for var, key, n in _ENV_LISTS:
        for i, v in enumerate([x for x in os.environ.get(var, "").split(",") if x][:n]):
            tune(f"{key}{i}", float(v))
    if os.environ.get("RT_WF_PLAN_GRID") == "tiny":
        tune("plan_grid_tiny", 1)


def last_error() -> str:
    return lib().rtHipLastError().decode("utf-8", "replace")


def _ptr(a):
    """Address of a numpy array -- or of a torch tensor (a scene whose arrays are already on the GPU, see scene_desc)."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def _f3(v) -> Float3:
    out = Float3()
    for i in range(3):
        out.s[i] = float(v[i])
    out.s[3] = 0.0
    return out


def _take(ptr: C.c_void_p, count: int, dtype) -> np.ndarray:
    """Copies `count` items out of a malloc'ed block returned by a builder, then frees it."""
    n = max(int(count), 0)
    out = np.empty(n, dtype)
    if n:
        C.memmove(out.ctypes.data, ptr.value, n * out.itemsize)
    lib().rtHipFree(ptr)
    return out


# ---------------------------------------------------------------------------------------------------------------
# builders (counterparts of CameraTriangleList::New / SceneTriangleList::New, trianglelist.cpp:520-626,655-737)
# ---------------------------------------------------------------------------------------------------------------

def build_camera_list(sc: Scene, threads: int = 0) -> None:
    L = lib()
    ps, pe, pl, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    rc = L.rtHipBuildCameraList(sc.width, sc.height, _ptr(sc.eye), _ptr(sc.eye_to_top_left), _ptr(sc.left_to_right),
                                _ptr(sc.top_to_bottom), sc.pixel_size_inv, sc.triangle_count, _ptr(sc.vertex), _ptr(sc.tri_index),
                                threads, C.byref(ps), C.byref(pe), C.byref(pl), C.byref(n))
    if rc != 0:
        raise RuntimeError(f"rtHipBuildCameraList failed ({rc})")
    sc.cam_start = _take(ps, sc.pixels, np.uint32)
    sc.cam_end = _take(pe, sc.pixels, np.uint32)
    sc.cam_list = _take(pl, n.value, np.uint32)


def build_camera_list_device(sc: Scene, device: int = 0) -> float:
    """Camera lists built on the GPU (rt_build_device.hip); returns the device time of the build in ms."""
    L = lib()
    ps, pe, pl, n, ms = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_double()
    rc = L.rtHipBuildCameraListDevice(device, sc.width, sc.height, _ptr(sc.eye), _ptr(sc.eye_to_top_left), _ptr(sc.left_to_right),
                                      _ptr(sc.top_to_bottom), sc.pixel_size_inv, sc.vertex_count, sc.triangle_count, _ptr(sc.vertex),
                                      _ptr(sc.tri_index), C.byref(ps), C.byref(pe), C.byref(pl), C.byref(n), C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"rtHipBuildCameraListDevice failed ({rc})")
    sc.cam_start = _take(ps, sc.pixels, np.uint32)
    sc.cam_end = _take(pe, sc.pixels, np.uint32)
    sc.cam_list = _take(pl, n.value, np.uint32)
    return ms.value


def build_scene_grid(sc: Scene, threads: int = 0) -> None:
    L = lib()
    box = np.zeros((GRID_DIV + 1, 4), np.float32)
    ps, pl, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    rc = L.rtHipBuildSceneGrid(sc.vertex_count, sc.triangle_count, _ptr(sc.vertex), _ptr(sc.tri_index), threads, _ptr(box),
                               C.byref(ps), C.byref(pl), C.byref(n))
    if rc != 0:
        raise RuntimeError(f"rtHipBuildSceneGrid failed ({rc})")
    sc.box_min = box
    sc.grid_start = _take(ps, GRID_DIV ** 3 + 1, np.uint32)
    sc.grid_list = _take(pl, n.value, np.uint32)


def build_scene_grid_device(sc: Scene, device: int = 0) -> float:
    """The scene grid built on the GPU (rt_build_device.hip); returns the device time of the build in ms."""
    L = lib()
    box = np.zeros((GRID_DIV + 1, 4), np.float32)
    ps, pl, n, ms = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_double()
    rc = L.rtHipBuildSceneGridDevice(device, sc.vertex_count, sc.triangle_count, _ptr(sc.vertex), _ptr(sc.tri_index), _ptr(box),
                                     C.byref(ps), C.byref(pl), C.byref(n), C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"rtHipBuildSceneGridDevice failed ({rc})")
    sc.box_min = box
    sc.grid_start = _take(ps, GRID_DIV ** 3 + 1, np.uint32)
    sc.grid_list = _take(pl, n.value, np.uint32)
    return ms.value


# rtHipTestBuildLog's fields, in the order of RT_BUILD_LOG_* (include/raytrace_hip.h)
BUILD_LOG_FIELDS = ("cam_thread", "cam_group", "cam_entries", "grid_thread", "grid_group", "grid_batches", "key_cap_first", "key_cap_final",
                    "grew", "attempts", "pairs")


def build_log() -> dict:
    """What this thread's last device builds did (rtHipTestBuildLog): camera triangles rasterised by one thread / a workgroup and
    the entries before de-duplication; grid triangles filled by one thread / workgroups, workgroup batches, first and final key
    capacity, whether the key buffer grew, fill attempts and pairs."""
    out = (C.c_uint64 * len(BUILD_LOG_FIELDS))()
    if lib().rtHipTestBuildLog(out, len(BUILD_LOG_FIELDS)) != len(BUILD_LOG_FIELDS):
        raise RuntimeError("rtHipTestBuildLog: the library logs a different set of fields")
    return dict(zip(BUILD_LOG_FIELDS, (int(v) for v in out)))


def build_lists(sc: Scene, threads: int = 0) -> Scene:
    build_camera_list(sc, threads)
    build_scene_grid(sc, threads)
    return sc


# ---------------------------------------------------------------------------------------------------------------
# drop-in layer
# ---------------------------------------------------------------------------------------------------------------

def raytrace_all(computation_type: int, sc: Scene):
    """RaytraceAll through the drop-in ABI.  Returns (ok, R, G, B) with [H,W] uint16 planes."""
    L = lib()
    apply_env_tuning()
    r = np.zeros(sc.pixels, np.uint16)
    g = np.zeros(sc.pixels, np.uint16)
    b = np.zeros(sc.pixels, np.uint16)
    dim = UInt2()
    dim.s[0], dim.s[1] = sc.width, sc.height
    ok = L.RaytraceAll(
        computation_type, dim, _f3(sc.eye), _f3(sc.eye_to_top_left), _f3(sc.left_to_right), _f3(sc.top_to_bottom),
        sc.pixel_size_inv, _ptr(sc.cam_start), _ptr(sc.cam_end), _ptr(sc.cam_list), len(sc.cam_list), sc.sample_count,
        sc.vertex_count, _ptr(sc.vertex), sc.triangle_count, _ptr(sc.tri_index), _ptr(sc.tri_material), _ptr(sc.tri_uv),
        _ptr(sc.tri_normal), GRID_DIV, _ptr(sc.box_min), _ptr(sc.grid_start), _ptr(sc.grid_list), sc.material_count,
        _ptr(sc.mat_size), _ptr(sc.mat_start), len(sc.textures), _ptr(sc.textures), sc.light_count, _ptr(sc.light_type),
        _ptr(sc.light_pos), _ptr(sc.light_dir), _ptr(sc.light_col), _ptr(sc.light_radius), _ptr(sc.light_half_att),
        _ptr(r), _ptr(g), _ptr(b))
    shape = (sc.height, sc.width)
    return bool(ok), r.reshape(shape), g.reshape(shape), b.reshape(shape)


def denoise_params(iterations=DENOISE_DEFAULTS["iterations"], colour_inv_sigma2=DENOISE_DEFAULTS["colour_inv_sigma2"],
                   albedo_inv_sigma2=DENOISE_DEFAULTS["albedo_inv_sigma2"], normal_power_log2=DENOISE_DEFAULTS["normal_power_log2"]) -> DenoiseParams:
    """rtHipDenoiseParams from the Python keywords (the library checks the values)."""
    if not all(0 <= int(v) <= 0xFFFFFFFF for v in (iterations, normal_power_log2)):  # (ctypes would wrap them into the uint32 fields)
        raise ValueError(f"denoise: iterations and normal_power_log2 must be in 0..2^32-1 (got {iterations}, {normal_power_log2})")
    return DenoiseParams(int(iterations), float(colour_inv_sigma2), float(albedo_inv_sigma2), int(normal_power_log2))


def ao_params(rays=AO_DEFAULTS["rays"], radius=AO_DEFAULTS["radius"], pixel_samples=AO_DEFAULTS["pixel_samples"],
              seed=AO_DEFAULTS["seed"]) -> AoParams:
    """rtHipAoParams from the Python keywords (the library checks the ranges)."""
    if not all(0 <= int(v) <= 0xFFFFFFFF for v in (rays, pixel_samples, seed)):  # (ctypes would wrap them into the uint32 fields)
        raise ValueError(f"ambient_occlusion: rays, pixel_samples and seed must be in 0..2^32-1 (got {rays}, {pixel_samples}, {seed})")
    return AoParams(int(rays), int(pixel_samples), float(radius), int(seed))


def bake_params(width, height, rays=BAKE_DEFAULTS["rays"], radius=BAKE_DEFAULTS["radius"], seed=BAKE_DEFAULTS["seed"],
                dilate=BAKE_DEFAULTS["dilate"], triangles=None, material=None) -> BakeParams:
    """rtHipBakeParams from the Python keywords (the library checks the ranges).  triangles: None (all), a range with step 1 or
    (first, count); material: None (no filter) or a material id."""
    if triangles is None:
        first, count = 0, ALL_TRIANGLES
    elif isinstance(triangles, range):
        if triangles.step != 1:
            raise ValueError("bake_ambient_occlusion: triangles must be a range with step 1")
        first, count = triangles.start, max(len(triangles), 0)
    else:
        first, count = (int(v) for v in triangles)
    vals = (width, height, rays, seed, dilate, first, count)
    if not all(0 <= int(v) <= 0xFFFFFFFF for v in vals):  # (ctypes would wrap them into the uint32 fields)
        raise ValueError(f"bake_ambient_occlusion: width, height, rays, seed, dilate and the triangle range must be in 0..2^32-1 (got {vals})")
    if material is not None and not -(1 << 31) <= int(material) < (1 << 31):
        raise ValueError(f"bake_ambient_occlusion: material {material} is not an int32")
    return BakeParams(int(width), int(height), int(rays), float(radius), int(seed), int(dilate), int(first), int(count),
                      0 if material is None else int(material), 0 if material is None else 1)


def quantise(colour: np.ndarray) -> list:
    """[H, W, 3] f32 -> u16 planes R, G, B as rtHipSceneDenoise writes them: v = c * 65535, 0 unless v > 0, 65535 from v >= 65534.5,
    else (u16)(v + 0.5)."""
    v = np.asarray(colour, np.float32) * np.float32(65535.0)
    with np.errstate(invalid="ignore"):
        u = np.where(~(v > 0), np.float32(0), np.where(v >= np.float32(65534.5), np.float32(65535), np.floor(v + np.float32(0.5))))
    u = u.astype(np.uint16)
    return [np.ascontiguousarray(u[..., c]) for c in range(3)]


def denoise(colour, normal, albedo, iterations=DENOISE_DEFAULTS["iterations"], colour_inv_sigma2=DENOISE_DEFAULTS["colour_inv_sigma2"],
            albedo_inv_sigma2=DENOISE_DEFAULTS["albedo_inv_sigma2"], normal_power_log2=DENOISE_DEFAULTS["normal_power_log2"], device: int = 0,
            stream: int = 0):
    """The denoiser of include/raytrace_hip.h ("DENOISER") on [H, W, 3] float32 colour, normal and albedo images; returns C^K as
    [H, W, 3] float32.  numpy arrays go through rtHipDenoise (host arrays, synchronous).  torch tensors on cuda:`device` go through
    rtHipDenoiseDevice on torch's current stream (or `stream`) with a torch scratch tensor; the result is a tensor on that device."""
    p = denoise_params(iterations, colour_inv_sigma2, albedo_inv_sigma2, normal_power_log2)
    A = _Arrays("denoise", any(hasattr(v, "data_ptr") for v in (colour, normal, albedo)), device, stream)
    if A.on_gpu:
        c, n, a = (v.contiguous() if isinstance(v, A.torch.Tensor) else v for v in (colour, normal, albedo))
    else:
        c, n, a = (np.ascontiguousarray(v, np.float32) for v in (colour, normal, albedo))
    shape, *others = (tuple(getattr(v, "shape", ())) for v in (c, n, a))
    if len(shape) != 3 or shape[2] != 3 or any(sh != shape for sh in others):
        raise ValueError(f"denoise: colour, normal and albedo must all be [H, W, 3] (got {shape}, {others[0]}, {others[1]})")
    for name, v in (("colour", c), ("normal", n), ("albedo", a)):
        A.check(name, v, shape)
    (H, W), out = shape[:2], A.new(shape)
    if not A.on_gpu:
        if lib().rtHipDenoise(device, W, H, _ptr(c), _ptr(n), _ptr(a), _ptr(out), C.byref(p)) != 0:
            raise RuntimeError("rtHipDenoise failed: " + last_error())
        return out
    nbytes = lib().rtHipDenoiseScratchBytes(W, H)
    if nbytes == 0:
        raise ValueError(f"denoise: a {W} x {H} image is not 1..2^27 pixels")
    scratch = A.new(nbytes, np.uint8)
    if lib().rtHipDenoiseDevice(device, W, H, *[A.address(v) for v in (c, n, a, out, scratch)], nbytes, C.byref(p), A.stream_arg()) != 0:
        raise RuntimeError("rtHipDenoiseDevice failed: " + last_error())
    A.done([c, n, a, out, scratch])
    return out


def temporal_params(max_history=TEMPORAL_DEFAULTS["max_history"], depth_tolerance=TEMPORAL_DEFAULTS["depth_tolerance"]) -> TemporalParams:
    """rtHipTemporalParams from the Python keywords (the library checks the values)."""
    return TemporalParams(float(max_history), float(depth_tolerance))


def temporal_clamp_params(mode=TEMPORAL_CLAMP_DEFAULTS["mode"], gamma=TEMPORAL_CLAMP_DEFAULTS["gamma"]) -> TemporalClampParams:
    """rtHipTemporalClampParams from the Python keywords; mode 1, 2, 3 or a name of TEMPORAL_CLAMP_MODES (the library checks the values)."""
    mode = TEMPORAL_CLAMP_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if isinstance(mode, str) or not 0 <= int(mode) <= 0xFFFFFFFF:  # (ctypes would wrap it into the uint32 field)
        raise ValueError(f"temporal clamp: mode must be 1, 2, 3 or one of {sorted(TEMPORAL_CLAMP_MODES)} (got {mode!r})")
    return TemporalClampParams(int(mode), float(gamma))


_TEMPORAL_INPUTS = (("colour", 3, False), ("motion", 2, False), ("prev_t", 1, False), ("triangle", 1, True))
_TEMPORAL_HISTORY = (("colour", 3, False), ("count", 1, False), ("t", 1, False), ("triangle", 1, True))


def temporal(colour, motion, prev_t, triangle, history, max_history=TEMPORAL_DEFAULTS["max_history"],
             depth_tolerance=TEMPORAL_DEFAULTS["depth_tolerance"], out: Optional[dict] = None, device: int = 0, stream: int = 0,
             clamp: Optional[dict] = None) -> dict:
    """The temporal accumulation of include/raytrace_hip.h ("TEMPORAL ACCUMULATION"): the frame `colour` [H, W, 3] f32 with its flow --
    `motion` [H, W, 2] f32, `prev_t` [H, W] f32, `triangle` [H, W] u32, what ResidentScene.motion() gives -- against `history`, a dict
    with "colour" [H, W, 3] f32, "count" [H, W] f32 (0: none), "t" [H, W] f32 and "triangle" [H, W] u32: the previous call's outputs and
    the previous frame's t and triangle maps.  Returns {"colour": [H, W, 3] f32, "count": [H, W] f32}.  numpy arrays go through
    rtHipTemporal (host arrays, synchronous); torch tensors on cuda:`device` (triangle ids uint32 or int32, their bits) stay there and go
    through rtHipTemporalDevice on torch's current stream (or `stream`).  `out`: a dict with "colour" and, optionally, "count" to fill
    instead of new arrays (they must not overlap an input); without "count" the counts are not written.  `clamp`: a dict with "mode"
    and "gamma" ({} for the defaults) pulls the history colour into the frame's 3x3 colour box before the blend (include/raytrace_hip.h,
    "TEMPORAL CLAMP"; rtHipTemporalClamp / rtHipTemporalClampDevice); None: no clamp."""
    p = temporal_params(max_history, depth_tolerance)
    cp = temporal_clamp_params(**clamp) if clamp is not None else None
    tail = (C.byref(p),) if cp is None else (C.byref(p), C.byref(cp))
    host, dev = ("rtHipTemporal", "rtHipTemporalDevice") if cp is None else ("rtHipTemporalClamp", "rtHipTemporalClampDevice")
    missing = [k for k, _, _ in _TEMPORAL_HISTORY if k not in history]
    if missing:
        raise ValueError(f"temporal: history lacks {missing}")
    given = [(name, v, ch, ids) for (name, ch, ids), v in zip(_TEMPORAL_INPUTS, (colour, motion, prev_t, triangle))]
    given += [("history " + name, history[name], ch, ids) for name, ch, ids in _TEMPORAL_HISTORY]
    if out is not None and ("colour" not in out or any(k not in ("colour", "count") for k in out)):
        raise ValueError(f"temporal: out takes 'colour' and optionally 'count' (got {sorted(out)})")
    if len(colour.shape) != 3 or colour.shape[2] != 3:
        raise ValueError(f"temporal: colour must be [H, W, 3] (got {tuple(colour.shape)})")
    shape = (int(colour.shape[0]), int(colour.shape[1]))
    A = _Arrays("temporal", any(hasattr(v, "data_ptr") for _, v, _, _ in given), device, stream)
    for name, v, ch, ids in given:
        A.check(name, v, shape + (ch,) if ch > 1 else shape, ids)
    res = dict(out) if out is not None else {"colour": A.new(shape + (3,)), "count": A.new(shape)}
    for name, v in res.items():
        A.check(f"out[{name!r}]", v, shape + (3,) if name == "colour" else shape)
    ptrs = [A.address(v) for _, v, _, _ in given] + [A.address(res["colour"]), A.address(res.get("count"))]
    if not A.on_gpu:
        if getattr(lib(), host)(device, shape[1], shape[0], *ptrs, *tail) != 0:
            raise RuntimeError(host + " failed: " + last_error())
        return res
    if getattr(lib(), dev)(device, shape[1], shape[0], *ptrs, *tail, A.stream_arg()) != 0:
        raise RuntimeError(dev + " failed: " + last_error())
    A.done([v for _, v, _, _ in given] + list(res.values()))
    return res


def variance_params(iterations=VARIANCE_DEFAULTS["iterations"], luminance_sigma2=VARIANCE_DEFAULTS["luminance_sigma2"],
                    variance_floor=VARIANCE_DEFAULTS["variance_floor"], albedo_inv_sigma2=VARIANCE_DEFAULTS["albedo_inv_sigma2"],
                    normal_power_log2=VARIANCE_DEFAULTS["normal_power_log2"], spatial_below=VARIANCE_DEFAULTS["spatial_below"]) -> VarianceParams:
    """rtHipVarianceParams from the Python keywords (the library checks the ranges)."""
    if not (0 <= int(iterations) <= 0xFFFFFFFF and 0 <= int(normal_power_log2) <= 0xFFFFFFFF):  # (ctypes would wrap them into the uint32 fields)
        raise ValueError(f"variance: iterations and normal_power_log2 must be in 0..2^32-1 (got {iterations}, {normal_power_log2})")
    return VarianceParams(int(iterations), float(luminance_sigma2), float(variance_floor), float(albedo_inv_sigma2), int(normal_power_log2),
                          float(spatial_below))


class _Arrays:
    """What denoise, temporal, temporal_moments, denoise_variance, motion_blur and depth_of_field need of their arrays, for numpy (host entry point) or torch on
    cuda:`device` (device entry point on torch's current stream or `stream`)."""

    def __init__(self, who, on_gpu, device, stream):
        self.who, self.on_gpu, self.device = who, on_gpu, device
        if on_gpu:
            import torch

            self.torch, self.dev = torch, torch.device("cuda", device)
            self.cur = torch.cuda.current_stream(self.dev)
            self.run = torch.cuda.ExternalStream(stream, device=self.dev) if stream and stream != self.cur.cuda_stream else self.cur

    def check(self, name, v, shape, ids=False):
        if self.on_gpu:
            kinds = (self.torch.uint32, self.torch.int32) if ids else (self.torch.float32,)
            ok = isinstance(v, self.torch.Tensor) and v.device == self.dev and v.dtype in kinds and tuple(v.shape) == shape and v.is_contiguous()
        else:
            ok = isinstance(v, np.ndarray) and v.dtype == (np.uint32 if ids else np.float32) and v.shape == shape and v.flags.c_contiguous
        if not ok:
            raise ValueError(f"{self.who}: {name} must be a contiguous {'uint32' if ids else 'float32'} {shape} "
                             f"{'tensor on ' + str(self.dev) if self.on_gpu else 'array'}")
        return v

    def new(self, shape, dtype=np.float32):
        if self.on_gpu:
            return self.torch.empty(shape, dtype=self.torch.uint8 if dtype == np.uint8 else self.torch.float32, device=self.dev)
        return np.empty(shape, dtype)

    def address(self, v):
        if v is None:
            return None
        return C.c_void_p(v.data_ptr()) if self.on_gpu else _ptr(v)

    def stream_arg(self):
        if self.run is not self.cur:
            self.run.wait_stream(self.cur)
        return C.c_void_p(self.run.cuda_stream) if self.run.cuda_stream else None

    def done(self, buffers):
        if self.run is not self.cur:
            self.cur.wait_stream(self.run)
            for buf in buffers:
                if buf is not None:
                    buf.record_stream(self.run)


def motion_blur_params(shutter=MOTION_BLUR_DEFAULTS["shutter"], max_blur=MOTION_BLUR_DEFAULTS["max_blur"], taps=MOTION_BLUR_DEFAULTS["taps"],
                       depth_softness=MOTION_BLUR_DEFAULTS["depth_softness"]) -> MotionBlurParams:
    """rtHipMotionBlurParams from the Python keywords (the library checks the ranges)."""
    if not 0 <= int(taps) <= 0xFFFFFFFF:  # (ctypes would wrap it into the uint32 field)
        raise ValueError(f"motion blur: taps must be in 0..2^32-1 (got {taps})")
    return MotionBlurParams(float(shutter), float(max_blur), int(taps), float(depth_softness))


def motion_blur(colour, motion, depth, shutter=MOTION_BLUR_DEFAULTS["shutter"], max_blur=MOTION_BLUR_DEFAULTS["max_blur"],
                taps=MOTION_BLUR_DEFAULTS["taps"], depth_softness=MOTION_BLUR_DEFAULTS["depth_softness"], device: int = 0, stream: int = 0,
                out=None):
    """The vector motion blur of include/raytrace_hip.h ("MOTION BLUR"): the frame `colour` [H, W, 3] f32 blurred along `motion`
    [H, W, 2] f32 with `depth` [H, W] f32 deciding what lies in front -- "motion" and "t" of ResidentScene.motion().  Returns the
    blurred image [H, W, 3] f32: `out` if given (it must not overlap an input), else a new array.  numpy arrays go through rtHipMotionBlur
    (host arrays, synchronous); torch tensors on cuda:`device` stay there and go through rtHipMotionBlurDevice on torch's current stream
    (or `stream`) with a torch scratch tensor."""
    p = motion_blur_params(shutter, max_blur, taps, depth_softness)
    if len(colour.shape) != 3 or colour.shape[2] != 3:
        raise ValueError(f"motion_blur: colour must be [H, W, 3] (got {tuple(colour.shape)})")
    shape = (int(colour.shape[0]), int(colour.shape[1]))
    given = [("colour", colour, shape + (3,)), ("motion", motion, shape + (2,)), ("depth", depth, shape)]
    A = _Arrays("motion_blur", any(hasattr(v, "data_ptr") for _, v, _ in given), device, stream)
    for name, v, sh in given:
        A.check(name, v, sh)
    res = A.check("out", out, shape + (3,)) if out is not None else A.new(shape + (3,))
    ptrs = [A.address(v) for v in (colour, motion, depth, res)]
    H, W = shape
    if not A.on_gpu:
        if lib().rtHipMotionBlur(device, W, H, *ptrs, C.byref(p)) != 0:
            raise RuntimeError("rtHipMotionBlur failed: " + last_error())
        return res
    nbytes = lib().rtHipMotionBlurScratchBytes(W, H)
    if nbytes == 0:
        raise ValueError(f"motion_blur: a {W} x {H} image is not 1..16384 pixels wide and high and 1..2^27 pixels")
    scratch = A.new(nbytes, np.uint8)
    if lib().rtHipMotionBlurDevice(device, W, H, *ptrs, A.address(scratch), nbytes, C.byref(p), A.stream_arg()) != 0:
        raise RuntimeError("rtHipMotionBlurDevice failed: " + last_error())
    A.done([colour, motion, depth, res, scratch])
    return res


def dof_params(focus=DEPTH_OF_FIELD_DEFAULTS["focus"], coc_scale=DEPTH_OF_FIELD_DEFAULTS["coc_scale"], max_coc=DEPTH_OF_FIELD_DEFAULTS["max_coc"],
               rings=DEPTH_OF_FIELD_DEFAULTS["rings"], depth_softness=DEPTH_OF_FIELD_DEFAULTS["depth_softness"]) -> DofParams:
    """rtHipDepthOfFieldParams from the Python keywords (the library checks the ranges)."""
    if not 0 <= int(rings) <= 0xFFFFFFFF:  # (ctypes would wrap it into the uint32 field)
        raise ValueError(f"depth of field: rings must be in 0..2^32-1 (got {rings})")
    return DofParams(float(focus), float(coc_scale), float(max_coc), int(rings), float(depth_softness))


def dof_lens(camera: dict, aperture: float, focus: float, **params) -> DofParams:
    """rtHipDepthOfFieldLens: the parameters of a thin lens of radius `aperture` (scene units) focused at `focus` (scene units, along the
    ray) for `camera` (the dict ResidentScene.camera() gives); the other parameters from the keywords of dof_params."""
    cam = Camera()
    for dst, key in ((cam.eye, "eye"), (cam.eyeToTopLeft, "eye_to_top_left"), (cam.leftToRight, "left_to_right"), (cam.topToBottom, "top_to_bottom")):
        v = np.asarray(camera[key], np.float32).reshape(-1)
        for i in range(3):
            dst[i] = v[i]
    cam.pixelSizeInv = np.float32(camera["pixel_size_inv"])
    p = dof_params(**params)
    if lib().rtHipDepthOfFieldLens(C.byref(cam), float(aperture), float(focus), C.byref(p)) != 0:
        raise ValueError("rtHipDepthOfFieldLens failed: " + last_error())
    return p


def depth_of_field(colour, depth, focus=DEPTH_OF_FIELD_DEFAULTS["focus"], coc_scale=DEPTH_OF_FIELD_DEFAULTS["coc_scale"],
                   max_coc=DEPTH_OF_FIELD_DEFAULTS["max_coc"], rings=DEPTH_OF_FIELD_DEFAULTS["rings"],
                   depth_softness=DEPTH_OF_FIELD_DEFAULTS["depth_softness"], device: int = 0, stream: int = 0, out=None):
    """The depth of field of include/raytrace_hip.h ("DEPTH OF FIELD"): the frame `colour` [H, W, 3] f32 blurred by the circle of
    confusion `depth` [H, W] f32 gives every pixel -- "depth" of ResidentScene.readback_passes(), the distance along the ray, +inf on a
    miss.  Returns the blurred image [H, W, 3] f32: `out` if given (it must not overlap an input), else a new array.  numpy arrays go
    through rtHipDepthOfField (host arrays, synchronous); torch tensors on cuda:`device` stay there and go through
    rtHipDepthOfFieldDevice on torch's current stream (or `stream`) with a torch scratch tensor."""
    p = dof_params(focus, coc_scale, max_coc, rings, depth_softness)
    if len(colour.shape) != 3 or colour.shape[2] != 3:
        raise ValueError(f"depth_of_field: colour must be [H, W, 3] (got {tuple(colour.shape)})")
    shape = (int(colour.shape[0]), int(colour.shape[1]))
    given = [("colour", colour, shape + (3,)), ("depth", depth, shape)]
    A = _Arrays("depth_of_field", any(hasattr(v, "data_ptr") for _, v, _ in given), device, stream)
    for name, v, sh in given:
        A.check(name, v, sh)
    res = A.check("out", out, shape + (3,)) if out is not None else A.new(shape + (3,))
    ptrs = [A.address(v) for v in (colour, depth, res)]
    H, W = shape
    if not A.on_gpu:
        if lib().rtHipDepthOfField(device, W, H, *ptrs, C.byref(p)) != 0:
            raise RuntimeError("rtHipDepthOfField failed: " + last_error())
        return res
    nbytes = lib().rtHipDepthOfFieldScratchBytes(W, H)
    if nbytes == 0:
        raise ValueError(f"depth_of_field: a {W} x {H} image is not 1..16384 pixels wide and high and 1..2^27 pixels")
    scratch = A.new(nbytes, np.uint8)
    if lib().rtHipDepthOfFieldDevice(device, W, H, *ptrs, A.address(scratch), nbytes, C.byref(p), A.stream_arg()) != 0:
        raise RuntimeError("rtHipDepthOfFieldDevice failed: " + last_error())
    A.done([colour, depth, res, scratch])
    return res


_MOMENTS_HISTORY = _TEMPORAL_HISTORY + (("moments", 2, False),)


def temporal_moments(colour, motion, prev_t, triangle, history, max_history=TEMPORAL_DEFAULTS["max_history"],
                     depth_tolerance=TEMPORAL_DEFAULTS["depth_tolerance"], device: int = 0, stream: int = 0,
                     clamp: Optional[dict] = None) -> dict:
    """raytrace.temporal with the luminance moments carried along (include/raytrace_hip.h, "VARIANCE-GUIDED FILTER", (a)): `history` also
    holds "moments" [H, W, 2] f32.  Returns {"colour", "count", "moments" [H, W, 2] f32, "variance" [H, W] f32}; colour and count equal
    raytrace.temporal's.  numpy arrays go through rtHipTemporalMoments; torch tensors on cuda:`device` stay there and go through
    rtHipTemporalMomentsDevice on torch's current stream (or `stream`).  `clamp`: as raytrace.temporal's (rtHipTemporalMomentsClamp /
    rtHipTemporalMomentsClampDevice); the moments are not clamped."""
    p = temporal_params(max_history, depth_tolerance)
    cp = temporal_clamp_params(**clamp) if clamp is not None else None
    tail = (C.byref(p),) if cp is None else (C.byref(p), C.byref(cp))
    host, dev = (("rtHipTemporalMoments", "rtHipTemporalMomentsDevice") if cp is None else
                 ("rtHipTemporalMomentsClamp", "rtHipTemporalMomentsClampDevice"))
    missing = [k for k, _, _ in _MOMENTS_HISTORY if k not in history]
    if missing:
        raise ValueError(f"temporal_moments: history lacks {missing}")
    given = [(name, v, ch, ids) for (name, ch, ids), v in zip(_TEMPORAL_INPUTS, (colour, motion, prev_t, triangle))]
    given += [("history " + name, history[name], ch, ids) for name, ch, ids in _MOMENTS_HISTORY]
    if len(colour.shape) != 3 or colour.shape[2] != 3:
        raise ValueError(f"temporal_moments: colour must be [H, W, 3] (got {tuple(colour.shape)})")
    shape = (int(colour.shape[0]), int(colour.shape[1]))
    A = _Arrays("temporal_moments", any(hasattr(v, "data_ptr") for _, v, _, _ in given), device, stream)
    for name, v, ch, ids in given:
        A.check(name, v, shape + (ch,) if ch > 1 else shape, ids)
    res = {"colour": A.new(shape + (3,)), "count": A.new(shape), "moments": A.new(shape + (2,)), "variance": A.new(shape)}
    ptrs = [A.address(v) for _, v, _, _ in given] + [A.address(res[k]) for k in ("colour", "count", "moments", "variance")]
    if not A.on_gpu:
        if getattr(lib(), host)(device, shape[1], shape[0], *ptrs, *tail) != 0:
            raise RuntimeError(host + " failed: " + last_error())
        return res
    if getattr(lib(), dev)(device, shape[1], shape[0], *ptrs, *tail, A.stream_arg()) != 0:
        raise RuntimeError(dev + " failed: " + last_error())
    A.done([v for _, v, _, _ in given] + list(res.values()))
    return res


def denoise_variance(colour, normal, albedo, moments=None, count=None, device: int = 0, stream: int = 0, **params) -> dict:
    """The variance-guided filter of include/raytrace_hip.h ("VARIANCE-GUIDED FILTER", (b) and (c)) on [H, W, 3] float32 colour, normal
    and albedo images, with the `moments` [H, W, 2] f32 and `count` [H, W] f32 that temporal_moments returns (both None: the single-frame
    use).  Keywords as VARIANCE_DEFAULTS.  Returns {"colour": C^K [H, W, 3] f32, "variance": V^K [H, W] f32}.  numpy arrays go through
    rtHipDenoiseVariance; torch tensors on cuda:`device` go through rtHipDenoiseVarianceDevice on torch's current stream (or `stream`)
    with a torch scratch tensor."""
    p = variance_params(**params)
    if (moments is None) != (count is None):
        raise ValueError("denoise_variance: moments and count are both None or both given")
    if len(colour.shape) != 3 or colour.shape[2] != 3:
        raise ValueError(f"denoise_variance: colour must be [H, W, 3] (got {tuple(colour.shape)})")
    shape = (int(colour.shape[0]), int(colour.shape[1]))
    given = [("colour", colour, 3), ("normal", normal, 3), ("albedo", albedo, 3)]
    if moments is not None:
        given += [("moments", moments, 2), ("count", count, 1)]
    A = _Arrays("denoise_variance", any(hasattr(v, "data_ptr") for _, v, _ in given), device, stream)
    for name, v, ch in given:
        A.check(name, v, shape + (ch,) if ch > 1 else shape)
    res = {"colour": A.new(shape + (3,)), "variance": A.new(shape)}
    ptrs = [A.address(v) for v in (colour, normal, albedo, moments, count, res["colour"], res["variance"])]
    H, W = shape
    if not A.on_gpu:
        if lib().rtHipDenoiseVariance(device, W, H, *ptrs, C.byref(p)) != 0:
            raise RuntimeError("rtHipDenoiseVariance failed: " + last_error())
        return res
    nbytes = lib().rtHipVarianceScratchBytes(W, H)
    if nbytes == 0:
        raise ValueError(f"denoise_variance: a {W} x {H} image is not 1..2^27 pixels")
    scratch = A.new(nbytes, np.uint8)
    if lib().rtHipDenoiseVarianceDevice(device, W, H, *ptrs, A.address(scratch), nbytes, C.byref(p), A.stream_arg()) != 0:
        raise RuntimeError("rtHipDenoiseVarianceDevice failed: " + last_error())
    A.done([v for _, v, _ in given] + list(res.values()) + [scratch])
    return res


def computation_type_names() -> list:
    L = lib()
    L.InitOpenCL()
    names = []
    buf = C.create_string_buffer(256)
    for i in range(L.GetComputationTypeCount()):
        if L.GetComputationTypeName(i, 255, buf):
            names.append(buf.value.decode())
    return names


# ---------------------------------------------------------------------------------------------------------------
# resident layer
# ---------------------------------------------------------------------------------------------------------------

def scene_desc(sc: Scene) -> SceneDesc:
    d = SceneDesc()
    d.width, d.height = sc.width, sc.height
    for i in range(4):
        d.eye[i] = float(sc.eye[i]); d.eyeToTopLeft[i] = float(sc.eye_to_top_left[i])
        d.leftToRight[i] = float(sc.left_to_right[i]); d.topToBottom[i] = float(sc.top_to_bottom[i])
    d.pixelSizeInv = sc.pixel_size_inv
    d.camStart, d.camEnd, d.camList = _ptr(sc.cam_start), _ptr(sc.cam_end), _ptr(sc.cam_list)
    d.camListSize = len(sc.cam_list)
    d.sampleCount = sc.sample_count
    d.vertexCount, d.vertex = sc.vertex_count, _ptr(sc.vertex)
    d.triangleCount = sc.triangle_count
    d.triIndex, d.triMaterial, d.triUv, d.triNormal = _ptr(sc.tri_index), _ptr(sc.tri_material), _ptr(sc.tri_uv), _ptr(sc.tri_normal)
    d.axesDiv = GRID_DIV
    d.boxMin, d.gridStart, d.gridList = _ptr(sc.box_min), _ptr(sc.grid_start), _ptr(sc.grid_list)
    d.materialCount, d.matSize, d.matStart = sc.material_count, _ptr(sc.mat_size), _ptr(sc.mat_start)
    d.texturesSize, d.textures = len(sc.textures), _ptr(sc.textures)
    d.lightCount, d.lightType = sc.light_count, _ptr(sc.light_type)
    d.lightPos, d.lightDir, d.lightCol = _ptr(sc.light_pos), _ptr(sc.light_dir), _ptr(sc.light_col)
    d.lightRadius, d.lightHalfAtt = _ptr(sc.light_radius), _ptr(sc.light_half_att)
    # arrays that are torch CUDA tensors (tiles.broadcast_scene(keep_on_device=True)): the library copies them HBM to HBM
    on_device = [bool(getattr(getattr(sc, k), "is_cuda", False)) for k in ("vertex", "tri_index", "cam_start", "grid_start", "textures", "light_type")]
    if any(on_device) and not all(on_device):
        raise ValueError("a scene's arrays must be all host arrays or all device tensors")
    d.arraysOnDevice = 1 if all(on_device) else 0
    return d


PATH_CLASS_GENERAL, PATH_CLASS_OPAQUE_DIFFUSE = 0, 1

# rtHipTestSceneView: name -> (RT_SCENE_VIEW_*, dtype of a word, words per element)
SCENE_VIEWS = {
    "header": (0, np.uint32, 1), "cam_start": (1, np.uint32, 1), "cam_end": (2, np.uint32, 1), "tri_rec": (3, np.float32, 16),
    "tri_shade": (4, np.float32, 24), "grid_bits": (5, np.uint64, 1), "block_sparse": (6, np.uint32, 1), "pair_rec": (7, np.uint32, 16),
    "cell_lut": (8, np.uint8, 1),
}
# further views of those arrays, numbered apart from 0 .. RT_SCENE_VIEWS - 1 (scene_view takes either table's names):
# tri_shade_row = RT_SCENE_VIEW_TRI_SHADE_ROW, the shading rows as stored (128 bytes each; tri_shade is their first 24 words, packed)
SCENE_VIEWS_EXTRA = {"tri_shade_row": (18, np.float32, 32)}
SCENE_VIEW_CLIP_PLANES = 16  # (RT_SCENE_VIEW_CLIP_PLANES; read by ResidentScene.clip_planes)
SCENE_VIEW_CLIP_APPLIED = 17  # (RT_SCENE_VIEW_CLIP_APPLIED; read by ResidentScene.clip_applied)
ROUND_VISIT_FIELDS = 12  # (RT_ROUND_VISIT_FIELDS)
PLACE_TABLE_WORDS = 2 * 64 * 32 + 4  # (RT_PLACE_TABLE_WORDS)
SCENE_VIEW_HEADER = ("planes_tame", "tile_count", "tiles_x", "triangle_count", "pair_count")


def path_class(sc: Scene) -> int:
    """The logic kernel a scene's paths run on (rtHipScenePathClass), decided on the host: PATH_CLASS_OPAQUE_DIFFUSE when no material
    reflects, lets light through or glows, no height map is an image and there is at most one light; PATH_CLASS_GENERAL otherwise."""
    d = SceneDesc()  # (only the materials and the lights are looked at: the lists need not be built)
    d.materialCount, d.matSize, d.matStart = sc.material_count, _ptr(sc.mat_size), _ptr(sc.mat_start)
    d.texturesSize, d.textures = len(sc.textures), _ptr(sc.textures)
    d.lightCount, d.lightType = sc.light_count, _ptr(sc.light_type)
    c = lib().rtHipScenePathClass(C.byref(d))
    if c < 0:
        raise ValueError(last_error())
    return c


def tile_count(width: int, height: int) -> int:
    return ((width + TILE - 1) // TILE) * ((height + TILE - 1) // TILE)


def tiles_of_rank(width: int, height: int, rank: int, world: int) -> np.ndarray:
    """Round-robin deal of the 128x128 tiles."""
    return np.arange(rank, tile_count(width, height), world, dtype=np.uint32)


def look_at_vectors(position, look_at, up, fov: float, width: int, height: int):
    """(eye_to_top_left, left_to_right, top_to_bottom, pixel_size_inv) of a camera at `position` looking at `look_at`: frontend.set_camera."""
    from . import frontend
    return frontend.set_camera(position, look_at, up, fov, width, height)


def orbit_positions(position, look_at, count: int) -> list:
    """`count` eye positions on the circle through `position` about the vertical (y) axis through `look_at`: pose i is `position` turned by
    i * 360 / count degrees, so every pose keeps the first one's height and its distance to the axis (float64 arithmetic)."""
    p, c = np.asarray(position, np.float64)[:3], np.asarray(look_at, np.float64)[:3]
    dx, dz = p[0] - c[0], p[2] - c[2]
    out = []
    for i in range(count):
        a = 2.0 * np.pi * i / count
        out.append(np.array([c[0] + dx * np.cos(a) + dz * np.sin(a), p[1], c[2] - dx * np.sin(a) + dz * np.cos(a)], np.float64))
    return out


def orbit_path(path: str, index: int) -> str:
    """img.bmp -> img_007.bmp: the file an orbit's view `index` is written to."""
    import os
    root, ext = os.path.splitext(path)
    return f"{root}_{index:03d}{ext}"


def spin_vertices(points, centre, index: int, count: int) -> np.ndarray:
    """`points` ([n, 3] or [n, 4] float32 positions) turned by index * 360 / count degrees about the vertical axis through `centre`, the
    turn orbit_positions gives the eye: x and z in fp64 and rounded to fp32, heights (and lane 3) copied.  Pose 0 is the input, bit for bit."""
    src = np.asarray(points, np.float32)
    out = src.copy()
    if index % count == 0:
        return out
    c = np.asarray(centre, np.float64)
    a = 2.0 * np.pi * index / count
    dx, dz = src[:, 0].astype(np.float64) - c[0], src[:, 2].astype(np.float64) - c[2]
    out[:, 0] = c[0] + dx * np.cos(a) + dz * np.sin(a)
    out[:, 2] = c[2] - dx * np.sin(a) + dz * np.cos(a)
    return out


def spin_directions(normals, index: int, count: int) -> np.ndarray:
    """Direction vectors (corner normals) under the same turn: spin_vertices about the origin."""
    return spin_vertices(normals, (0.0, 0.0, 0.0), index, count)


LIGHT_FIELDS = ("light_type", "light_pos", "light_dir", "light_col", "light_radius", "light_half_att")


def scene_lights(sc) -> dict:
    """The six light arrays of a Scene under Scene's field names (what set_lights and relight take)."""
    return {k: getattr(sc, k) for k in LIGHT_FIELDS}


def _light_arrays(lights) -> dict:
    """`lights` -- a sequence of dicts as scene.pack_lights takes, or a dict of the six arrays under Scene's field names -- as contiguous
    arrays in the library's layouts: light_type [L] int32, light_pos / light_dir / light_col [L, 4] float32 (lane 3 zero where it is
    added), light_radius / light_half_att [L] float32."""
    from .scene import pack_lights
    if not isinstance(lights, dict):
        lights = dict(zip(LIGHT_FIELDS, pack_lights(list(lights))))
    missing = [k for k in LIGHT_FIELDS if k not in lights]
    if missing:
        raise ValueError(f"lights: missing {missing}")
    out = {"light_type": np.ascontiguousarray(lights["light_type"], np.int32).reshape(-1)}
    n = out["light_type"].shape[0]
    for k in ("light_pos", "light_dir", "light_col"):
        out[k] = _padded_rows(k, np.asarray(lights[k], np.float32).reshape(n, -1), np.float32, n)[0] if n else np.zeros((0, 4), np.float32)
    for k in ("light_radius", "light_half_att"):
        out[k] = np.ascontiguousarray(lights[k], np.float32).reshape(-1)
        if out[k].shape[0] != n:
            raise ValueError(f"{k}: {out[k].shape[0]} values for {n} lights")
    return out


def relight(lights, index: int, count: int) -> dict:
    """The light arrays (a dict under Scene's field names, scene_lights) with light 0's position and direction turned by index * 360 /
    count degrees about the vertical axis through the origin, in float32 arithmetic; heights, lane 3, the other four arrays and lights
    1.. are copied.  Pose 0 is the input, bit for bit."""
    out = {k: np.array(lights[k], copy=True) for k in LIGHT_FIELDS}
    if index % count == 0 or out["light_type"].shape[0] == 0:
        return out
    a = np.float32(2.0 * np.pi * index / count)
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    for k in ("light_pos", "light_dir"):
        x, z = np.float32(lights[k][0, 0]), np.float32(lights[k][0, 2])
        out[k][0, 0] = np.float32(x * c) + np.float32(z * s)
        out[k][0, 2] = np.float32(z * c) - np.float32(x * s)
    return out


def _padded_rows(name: str, a, dtype, rows: Optional[int] = None):
    """A [n, 3] or [n, 4] array (numpy, or a torch tensor on a GPU) as contiguous [n, 4] rows of `dtype`, lane 3 zero where it is added:
    the library's 16-byte cl_float3 / cl_int3.  Returns (array, on_device)."""
    if hasattr(a, "data_ptr"):
        import torch

        want = torch.float32 if dtype == np.float32 else torch.int32
        if a.dtype != want:
            raise TypeError(f"{name}: dtype {a.dtype}, expected {want}")
        if a.dim() != 2 or a.shape[1] not in (3, 4) or (rows is not None and a.shape[0] != rows):
            raise ValueError(f"{name}: shape {tuple(a.shape)}, expected [{rows if rows is not None else 'n'}, 3 or 4]")
        if not a.is_cuda:
            raise ValueError(f"{name}: a torch tensor must live on the scene's GPU (pass numpy arrays for host memory)")
        if a.shape[1] == 3:
            a = torch.nn.functional.pad(a, (0, 1))
        return a.contiguous(), True
    a = np.asarray(a)
    if a.dtype != dtype:
        raise TypeError(f"{name}: dtype {a.dtype}, expected {np.dtype(dtype)}")
    if a.ndim != 2 or a.shape[1] not in (3, 4) or (rows is not None and a.shape[0] != rows):
        raise ValueError(f"{name}: shape {a.shape}, expected [{rows if rows is not None else 'n'}, 3 or 4]")
    if a.shape[1] == 3:
        out = np.zeros((a.shape[0], 4), dtype)
        out[:, :3] = a
        return out, False
    return np.ascontiguousarray(a), False


class _ResidentView:
    """Mixed into the Scene class of ResidentScene.scene after a geometry update (see ResidentScene._describe_geometry)."""


def _resident_view_class(base):
    def array(name):
        def get(self):
            v = self.__dict__.get(name)
            if hasattr(v, "data_ptr"):  # handed over as a tensor: downloaded on first read
                v = self.__dict__[name] = v.cpu().numpy()
            return v

        def put(self, value):
            self.__dict__[name] = value
        return property(get, put)

    def built(name, kind):
        def get(self):
            stale = self.__dict__.get("_stale", set())
            if kind in stale:
                stale.discard(kind)  # (first: the builders read and write these attributes themselves)
                (build_scene_grid if kind == "grid" else build_camera_list)(self)
            return self.__dict__.get(name)

        def put(self, value):
            self.__dict__[name] = value
        return property(get, put)
    members = {n: array(n) for n in ("vertex", "tri_index", "tri_normal", "tri_material")}
    members.update({n: built(n, "grid") for n in ("box_min", "grid_start", "grid_list")})
    members.update({n: built(n, "camera") for n in ("cam_start", "cam_end", "cam_list")})
    members["triangle_count"] = property(lambda self: int(self.__dict__["tri_index"].shape[0]))  # (the counts do not download anything)
    members["vertex_count"] = property(lambda self: int(self.__dict__["vertex"].shape[0]))
    return type("Resident" + base.__name__, (base, _ResidentView), members)


class ResidentScene:
    """A scene resident in one GPU's HBM (rtHipScene)."""

    def __init__(self, sc: Scene, device: int = 0, tiles: Optional[Sequence[int]] = None, like: "Optional[ResidentScene]" = None):
        """`like`: a resident instance of the same scene whose geometry, grid, materials and lights are copied device to device."""
        L = lib()
        apply_env_tuning()
        self.scene = sc
        self.device = device
        self.tiles = None if tiles is None else np.ascontiguousarray(tiles, np.uint32)
        d = scene_desc(sc)
        self.handle = L.rtHipSceneCreateLike(device, C.byref(d), _ptr(self.tiles), 0 if self.tiles is None else len(self.tiles),
                                             None if like is None else like.handle)
        if not self.handle:
            raise RuntimeError("rtHipSceneCreate failed: " + last_error())
        if self.tiles is None:
            self.tiles = np.arange(tile_count(sc.width, sc.height), dtype=np.uint32)

    def close(self):
        if getattr(self, "handle", None):
            lib().rtHipSceneDestroy(self.handle)
            self.handle = None

    __del__ = close

    def try_set_camera(self, eye, eye_to_top_left, left_to_right, top_to_bottom, pixel_size_inv) -> int:
        """rtHipSceneSetCamera's return code (0, or a negative code with last_error() set): the scene's camera becomes the five fields and
        the candidate lists of its tiles are rebuilt on the device.  On failure the scene keeps its old view."""
        cam = Camera()
        for dst, src in ((cam.eye, eye), (cam.eyeToTopLeft, eye_to_top_left), (cam.leftToRight, left_to_right), (cam.topToBottom, top_to_bottom)):
            v = np.asarray(src, np.float32).reshape(-1)
            for i in range(3):
                dst[i] = v[i]
        cam.pixelSizeInv = np.float32(pixel_size_inv)
        return int(lib().rtHipSceneSetCamera(self.handle, C.byref(cam)))

    def set_camera(self, eye, eye_to_top_left, left_to_right, top_to_bottom, pixel_size_inv) -> None:
        """Moves the resident scene's camera (rtHipSceneSetCamera); raises RuntimeError when the move is refused."""
        rc = self.try_set_camera(eye, eye_to_top_left, left_to_right, top_to_bottom, pixel_size_inv)
        if rc != 0:
            raise RuntimeError(f"rtHipSceneSetCamera failed ({rc}): {last_error()}")

    def look_at(self, position, look_at, up, fov: float) -> None:
        """Moves the camera to `position`, looking at `look_at`: the vectors frontend.set_camera gives for the scene's image size."""
        self.set_camera(position, *look_at_vectors(position, look_at, up, fov, self.scene.width, self.scene.height))

    def camera(self) -> dict:
        """The camera in effect (rtHipSceneGetCamera): eye, eye_to_top_left, left_to_right, top_to_bottom ([4] float32), pixel_size_inv."""
        cam = Camera()
        self._check(lib().rtHipSceneGetCamera(self.handle, C.byref(cam)), "rtHipSceneGetCamera")
        return dict(eye=np.array(cam.eye, np.float32), eye_to_top_left=np.array(cam.eyeToTopLeft, np.float32),
                    left_to_right=np.array(cam.leftToRight, np.float32), top_to_bottom=np.array(cam.topToBottom, np.float32),
                    pixel_size_inv=float(cam.pixelSizeInv))

    def try_set_vertices(self, vertex, tri_index=None, tri_normal=None) -> int:
        """rtHipSceneSetGeometry's return code (0, or a negative code with last_error() set).  vertex [V, 3] or [V, 4] float32, tri_index
        [T, 3] or [T, 4] int32 (None: the index array the scene retained from its last update), tri_normal [3T, 3] or [3T, 4] float32
        (None: the normals stay): numpy arrays, or torch tensors on the scene's GPU (all of one kind), which are handed over as device
        pointers once torch's current stream has been synchronised; nothing of them comes to the host.  On success self.scene is replaced by a
        copy that describes what is resident (_describe_geometry says how, lazily); on failure nothing changes."""
        T = self.scene.triangle_count
        v, dev = _padded_rows("vertex", vertex, np.float32)
        arrays = [v]
        idx = nrm = None
        if tri_index is not None:
            idx, d = _padded_rows("tri_index", tri_index, np.int32, T)
            arrays.append(idx)
            if d != dev:
                raise ValueError("tri_index: numpy arrays and torch tensors cannot be mixed in one update")
        if tri_normal is not None:
            nrm, d = _padded_rows("tri_normal", tri_normal, np.float32, 3 * T)
            arrays.append(nrm)
            if d != dev:
                raise ValueError("tri_normal: numpy arrays and torch tensors cannot be mixed in one update")
        if dev:
            import torch

            for a in arrays:
                if a.device.index != self.device:
                    raise ValueError(f"a tensor lives on {a.device}, the scene on GPU {self.device}")
            torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()  # the call has no stream argument
        rc = self._set_geometry(v, idx, nrm, dev)
        if rc == 0:
            self._describe_geometry(v, idx, nrm, dev)
        return rc

    def _set_geometry(self, vertex, tri_index, tri_normal, on_device: bool) -> int:
        up = GeometryUpdate(int(vertex.shape[0]), _ptr(vertex), _ptr(tri_index), _ptr(tri_normal), 1 if on_device else 0)
        return int(lib().rtHipSceneSetGeometry(self.handle, C.byref(up)))

    def _describe_geometry(self, vertex, tri_index, tri_normal, on_device: bool) -> None:
        """self.scene becomes a copy that describes what is resident, without moving anything: arrays that were handed over as tensors stay
        on the GPU and come to the host when (and if) the copy's vertex / tri_index / tri_normal is first read; its camera is the one in
        effect; box_min / grid_* / cam_* are rebuilt by the host builders -- whose results the resident arrays equal -- when first read."""
        import copy

        sc = copy.copy(self.scene)
        if not isinstance(sc, _ResidentView):
            sc.__class__ = _resident_view_class(type(sc))
        for name, a in (("vertex", vertex), ("tri_index", tri_index), ("tri_normal", tri_normal)):
            if a is not None:
                setattr(sc, name, a)  # (a tensor is kept as it is: _ResidentView downloads it on first read)
        if self.handle:
            cam = self.camera()
            sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom = (cam[k] for k in ("eye", "eye_to_top_left", "left_to_right", "top_to_bottom"))
            sc.pixel_size_inv = cam["pixel_size_inv"]
        sc.__dict__["_stale"] = {"grid", "camera"}
        self.scene = sc

    def set_vertices(self, vertex, tri_index=None, tri_normal=None) -> None:
        """Changes the resident scene's shape (rtHipSceneSetGeometry); raises RuntimeError when the update is refused."""
        rc = self.try_set_vertices(vertex, tri_index, tri_normal)
        if rc != 0:
            raise RuntimeError(f"rtHipSceneSetGeometry failed ({rc}): {last_error()}")

    def try_set_lights(self, lights) -> int:
        """rtHipSceneSetLights' return code (0, or a negative code with last_error() set): the scene's lights become `lights`, a sequence of
        dicts as scene.pack_lights takes or a dict of the six arrays under Scene's field names.  Sample window, tile buffer and temporal
        history are kept (reset_temporal is the caller's decision).  On success self.scene is replaced by a copy that describes what is
        resident; on failure nothing changes."""
        a = _light_arrays(lights)
        arg = Lights(int(a["light_type"].shape[0]), *[_ptr(a[k]) for k in LIGHT_FIELDS])
        rc = int(lib().rtHipSceneSetLights(self.handle, C.byref(arg)))
        if rc == 0:
            self._describe_edit(**a)
        return rc

    def set_lights(self, lights) -> None:
        """Replaces the resident scene's lights (rtHipSceneSetLights); raises RuntimeError when the edit is refused."""
        rc = self.try_set_lights(lights)
        if rc != 0:
            raise RuntimeError(f"rtHipSceneSetLights failed ({rc}): {last_error()}")

    def try_set_materials(self, materials=None, tri_material=None) -> int:
        """rtHipSceneSetMaterials' return code (0, or a negative code with last_error() set).  materials: a sequence of dicts as
        scene.pack_materials takes, or a dict with mat_size, mat_start and textures; None keeps the resident tables and atlas.
        tri_material: [T] int32 ids, a numpy array or a torch tensor on the scene's GPU (handed over as a device pointer once torch's
        current stream has been synchronised); None keeps the resident ids.  On success self.scene is replaced by a copy that describes
        what is resident (a tensor is kept and comes to the host when the copy's tri_material is first read); on failure nothing changes."""
        from .scene import pack_materials
        up, fields, keep = MaterialUpdate(), {}, []
        if materials is not None:
            if not isinstance(materials, dict):
                materials = dict(zip(("mat_size", "mat_start", "textures"), pack_materials(list(materials))))
            size = np.ascontiguousarray(materials["mat_size"], np.uint32).reshape(-1, 2)
            start = np.ascontiguousarray(materials["mat_start"], np.int32).reshape(-1)
            tex = np.ascontiguousarray(materials["textures"], np.uint8).reshape(-1, 4)
            if size.shape[0] % 5 or start.shape[0] < size.shape[0]:
                raise ValueError(f"materials: {size.shape[0]} sizes and {start.shape[0]} starts (five channels per material)")
            up.replaceMaterials, up.materialCount, up.matSize, up.matStart = 1, size.shape[0] // 5, _ptr(size), _ptr(start)
            up.texturesSize, up.textures = tex.shape[0], _ptr(tex)
            fields.update(mat_size=size, mat_start=start, textures=tex)
            keep += [size, start, tex]
        if tri_material is not None:
            T = self.scene.triangle_count
            if hasattr(tri_material, "data_ptr"):
                import torch

                if tri_material.dtype != torch.int32 or tuple(tri_material.shape) != (T,):
                    raise ValueError(f"tri_material: {tri_material.dtype} {tuple(tri_material.shape)}, expected int32 [{T}]")
                if not tri_material.is_cuda or tri_material.device.index != self.device:
                    raise ValueError(f"tri_material: a torch tensor must live on the scene's GPU {self.device} (pass a numpy array for host memory)")
                ids = tri_material.contiguous()
                torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()  # the call has no stream argument
                up.triMaterialOnDevice = 1
            else:
                ids = np.asarray(tri_material)
                if ids.dtype != np.int32 or ids.shape != (T,):
                    raise ValueError(f"tri_material: {ids.dtype} {ids.shape}, expected int32 [{T}]")
                ids = np.ascontiguousarray(ids)
            up.triMaterial = _ptr(ids)
            fields["tri_material"] = ids
            keep.append(ids)
        rc = int(lib().rtHipSceneSetMaterials(self.handle, C.byref(up)))
        if rc == 0:
            self._describe_edit(**fields)
        return rc

    def set_materials(self, materials=None, tri_material=None) -> None:
        """Replaces the resident scene's materials and / or material ids (rtHipSceneSetMaterials); raises RuntimeError when the edit is
        refused."""
        rc = self.try_set_materials(materials, tri_material)
        if rc != 0:
            raise RuntimeError(f"rtHipSceneSetMaterials failed ({rc}): {last_error()}")

    def _describe_edit(self, **fields) -> None:
        """self.scene becomes a copy with `fields` replaced: what scene_desc for a later like=, a fresh twin and -- from the next frame
        on -- readback_passes' material ids read."""
        import copy

        sc = copy.copy(self.scene)
        if any(hasattr(v, "data_ptr") for v in fields.values()) and not isinstance(sc, _ResidentView):
            sc.__class__ = _resident_view_class(type(sc))
        for name, v in fields.items():
            setattr(sc, name, v)
        self.scene = sc

    def edit_times_ms(self) -> dict:
        """Device time of the last successful edit's stages (rtHipSceneEditTimes): the light arrays, the material tables and atlas, the id
        check and store."""
        out = (C.c_double * 3)()
        self._check(lib().rtHipSceneEditTimes(self.handle, C.byref(out)), "rtHipSceneEditTimes")
        return dict(lights=out[0], materials=out[1], ids=out[2])

    def geometry_log(self) -> dict:
        """The last update: triangles filled by one thread, by workgroups, fill attempts, pairs, camera list entries, and whether it
        allocated anything (rtHipTestSceneGeometryLog)."""
        out = (C.c_uint64 * 6)()
        if lib().rtHipTestSceneGeometryLog(self.handle, C.byref(out), 6) != 6:
            raise RuntimeError("rtHipTestSceneGeometryLog failed: " + last_error())
        return dict(thread=int(out[0]), group=int(out[1]), attempts=int(out[2]), pairs=int(out[3]), entries=int(out[4]), allocated=int(out[5]))

    def geometry_times_ms(self) -> dict:
        """Stream time of the last update's stages (rtHipTestSceneGeometryTimes)."""
        out = (C.c_double * 4)()
        self._check(lib().rtHipTestSceneGeometryTimes(self.handle, C.byref(out)), "rtHipTestSceneGeometryTimes")
        return dict(records=out[0], grid=out[1], dense=out[2], camera=out[3])

    def camera_list(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Entries of the device camera list the scene's ranges index (rtHipTestSceneCameraList)."""
        total = lib().rtHipTestSceneCameraList(self.handle, 0, 0, None)
        if total < 0:
            raise RuntimeError("rtHipTestSceneCameraList failed: " + last_error())
        if count is None:
            count = max(total - first, 0)
        out = np.zeros(count, np.uint32)
        self._check(lib().rtHipTestSceneCameraList(self.handle, first, count, _ptr(out)), "rtHipTestSceneCameraList")
        return out

    def pointers(self) -> tuple:
        """Device addresses of triRec, triShade, gridBlockSparse, pairRec, matRec, lightPos (rtHipTestScenePointers)."""
        out = (C.c_void_p * 6)()
        self._check(lib().rtHipTestScenePointers(self.handle, C.byref(out)), "rtHipTestScenePointers")
        return tuple(int(v or 0) for v in out)

    def camera_log(self) -> dict:
        """The last move: triangles rasterised by one thread, by a workgroup, list entries (rtHipTestSceneCameraLog)."""
        out = (C.c_uint64 * 3)()
        self._check(lib().rtHipTestSceneCameraLog(self.handle, C.byref(out)), "rtHipTestSceneCameraLog")
        return dict(thread=int(out[0]), group=int(out[1]), entries=int(out[2]))

    def camera_times_ms(self) -> dict:
        """Device time of the last move's two stages (rtHipTestSceneCameraTimes)."""
        out = (C.c_double * 2)()
        self._check(lib().rtHipTestSceneCameraTimes(self.handle, C.byref(out)), "rtHipTestSceneCameraTimes")
        return dict(count=out[0], fill=out[1])

    def path_class(self) -> int:
        """The path class this scene's logic kernels run (rtHipTestPathClass: 0 when it was built with logic_class = 0)."""
        return lib().rtHipTestPathClass(self.handle)

    def round_rays(self, n: int = 8) -> list:
        """Rays per round of the last frame (rtHipTestRoundLog; call after a synchronisation): round 0 = the paths, round r > 0 = the
        rays logic round r - 1 sent to the grid.  Rounds the frame did not issue read 0."""
        rays = (C.c_uint32 * n)()
        if lib().rtHipTestRoundLog(self.handle, rays, n) < 0:
            raise RuntimeError("rtHipTestRoundLog failed")
        return [int(v) for v in rays]

    def round_visits(self, n: int = 8) -> list:
        """What each trace round of the last frame held (rtHipTestRoundVisits; the scene was built with RT_WF_VISIT_LOG=1): per round a
        dict {ordered, entries, ended, and per kind of ray -- shadow (a main entry sent out with a look-ahead entry), main (a main entry
        on its own), bounce (a look-ahead entry) -- {rays, hits, visits}}; visits are planned cell visits, counted in ordered rounds."""
        out = (C.c_uint64 * (ROUND_VISIT_FIELDS * n))()
        if lib().rtHipTestRoundVisits(self.handle, out, n) < 0:
            raise RuntimeError("rtHipTestRoundVisits failed: " + last_error())
        rounds = []
        for r in range(n):
            f = [int(v) for v in out[ROUND_VISIT_FIELDS * r:ROUND_VISIT_FIELDS * (r + 1)]]
            row = dict(ordered=f[0], entries=f[1], ended=f[2])
            for k, kind in enumerate(("shadow", "main", "bounce")):
                row[kind] = dict(rays=f[3 + 3 * k], hits=f[4 + 3 * k], visits=f[5 + 3 * k])
            row["visits"] = sum(row[kind]["visits"] for kind in ("shadow", "main", "bounce"))
            rounds.append(row)
        return rounds

    def shade_log(self, n: int = 8):
        """(split logic rounds the last frame issued, paths each round listed for its shade pass) -- rtHipTestShadeLog; call after a
        synchronisation.  0 rounds: the frame ran one logic kernel per round."""
        listed = (C.c_uint32 * n)()
        rounds = lib().rtHipTestShadeLog(self.handle, listed, n)
        if rounds < 0:
            raise RuntimeError("rtHipTestShadeLog failed")
        return rounds, [int(v) for v in listed]

    def place_log(self):
        """(ordered rounds the last frame placed directly, scatter launches it issued) -- rtHipTestPlaceLog."""
        out = (C.c_uint32 * 2)()
        if lib().rtHipTestPlaceLog(self.handle, out) != 0:
            raise RuntimeError("rtHipTestPlaceLog failed")
        return int(out[0]), int(out[1])

    def place_view(self, round_: int, positions: Optional[int] = None):
        """rtHipTestPlaceView of the first tile group: (cells [64 classes, 32 copies, 2] u32 {first sorted position, entries}, total,
        (slices, segment length) of the recorded layout, entries [positions, 16] u32 -- by default the table's total of them)."""
        table = np.zeros(PLACE_TABLE_WORDS, np.uint32)
        self._check(lib().rtHipTestPlaceView(self.handle, round_, _ptr(table), None, 0), "rtHipTestPlaceView")
        total = int(table[PLACE_TABLE_WORDS - 4])
        n = total if positions is None else positions
        entries = np.zeros((n, 16), np.uint32)
        if n:
            self._check(lib().rtHipTestPlaceView(self.handle, round_, None, _ptr(entries), n), "rtHipTestPlaceView")
        return table[:PLACE_TABLE_WORDS - 4].reshape(64, 32, 2), total, (int(table[PLACE_TABLE_WORDS - 3]), int(table[PLACE_TABLE_WORDS - 2])), entries

    def shade_kat(self, op: int, inp: np.ndarray) -> np.ndarray:
        """rtHipTestShadeKat on this scene: `inp` holds one 40-byte (RT_SHADE_KAT_TEXEL) or 48-byte (RT_SHADE_KAT_NORMAL) row per item;
        returns the 64- or 96-byte rows as uint8."""
        inp = np.ascontiguousarray(inp)
        n = inp.shape[0]
        out = np.zeros((n, 64 if op == 0 else 96), np.uint8)
        self._check(lib().rtHipTestShadeKat(self.handle, op, n, _ptr(inp), _ptr(out)), "rtHipTestShadeKat")
        return out

    def scene_view(self, name: str, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Elements [first, first + count) (default: to the end) of one of the scene's device arrays (rtHipTestSceneView; names in
        SCENE_VIEWS): cam_start / cam_end tile-major u32, tri_rec [n, 16] f32, tri_shade [n, 24] f32, grid_bits u64, block_sparse u32
        words, pair_rec [n, 16] u32 words (floats as their bits), cell_lut u8, header u32 (SCENE_VIEW_HEADER); SCENE_VIEWS_EXTRA:
        tri_shade_row [n, 32] f32, the shading rows as the device stores them."""
        what, dtype, words = SCENE_VIEWS[name] if name in SCENE_VIEWS else SCENE_VIEWS_EXTRA[name]
        total = lib().rtHipTestSceneView(self.handle, what, 0, 0, None)
        if total < 0:
            raise RuntimeError("rtHipTestSceneView failed: " + last_error())
        if count is None:
            count = max(total - first, 0)
        out = np.zeros((count, words) if words > 1 else count, dtype)
        self._check(lib().rtHipTestSceneView(self.handle, what, first, count, _ptr(out)), "rtHipTestSceneView")
        return out

    def clip_planes(self) -> np.ndarray:
        """The planes [n, 4] f32 {n.xyz, off} of the grid's clip bound (RT_SCENE_VIEW_CLIP_PLANES, read from the device; n <= 8, 0 when none is kept)."""
        total = lib().rtHipTestSceneView(self.handle, SCENE_VIEW_CLIP_PLANES, 0, 0, None)
        if total < 0:
            raise RuntimeError("rtHipTestSceneView failed: " + last_error())
        out = np.zeros((total, 4), np.float32)
        if total:
            self._check(lib().rtHipTestSceneView(self.handle, SCENE_VIEW_CLIP_PLANES, 0, total, _ptr(out)), "rtHipTestSceneView")
        return out

    def clip_applied(self) -> int:
        """How many clip planes the planning kernels apply (RT_SCENE_VIEW_CLIP_APPLIED): len(clip_planes()), or 0 with ray_clip = 0."""
        out = np.zeros(1, np.uint32)
        self._check(lib().rtHipTestSceneView(self.handle, SCENE_VIEW_CLIP_APPLIED, 0, 1, _ptr(out)), "rtHipTestSceneView")
        return int(out[0])

    def scene_header(self) -> dict:
        return dict(zip(SCENE_VIEW_HEADER, (int(v) for v in self.scene_view("header"))))

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {last_error()}")

    def render(self, stream: int = 0):
        self._check(lib().rtHipRenderTiles(self.handle, stream or None), "rtHipRenderTiles")
        self._frame_scene = self.scene  # (the description the frame was issued under: readback_passes' material ids are that frame's)

    def finish(self) -> bool:
        """After the caller's own synchronisation: checks that the frames issued since the last check were complete
        (rtHipFrameFinish).  Returns True when the last frame had to be rendered again (its launch plan was too short)."""
        redone = C.c_int(0)
        self._check(lib().rtHipFrameFinish(self.handle, C.byref(redone)), "rtHipFrameFinish")
        if redone.value:
            self._frame_scene = self.scene  # (rendered again, under the description in effect now)
        return bool(redone.value)

    def set_sample_window(self, total: Optional[int] = None, first: int = 0, divisor: Optional[int] = None, accumulate: bool = False,
                          advance: bool = False) -> None:
        """The sample window of the frames to come (rtHipSceneSetSampleWindow; include/raytrace_hip.h, "SAMPLE WINDOWS"): a frame renders
        sample ids first+1 .. first+S of a sequence of `total` samples per pixel, each scaled by 65535 / divisor.  None means S, so
        set_sample_window() is the default window."""
        S = int(self.scene.sample_count)
        w = SampleWindow(S if total is None else total, first, S if divisor is None else divisor, int(accumulate), int(advance))
        self._check(lib().rtHipSceneSetSampleWindow(self.handle, C.byref(w)), "rtHipSceneSetSampleWindow")

    def sample_window(self) -> dict:
        """{"next": the window the next frame will use, "last": the one the last issued frame used (all zero before the first frame)}."""
        nxt, last = SampleWindow(), SampleWindow()
        self._check(lib().rtHipSceneGetSampleWindow(self.handle, C.byref(nxt), C.byref(last)), "rtHipSceneGetSampleWindow")
        return {"next": nxt.as_dict(), "last": last.as_dict()}

    def progressive(self, total: int, stream: int = 0):
        """Renders a frame of `total` samples per pixel in total / S frames of S: sets the progressive window {total, 0, total, 1, 1} and
        yields (samples_done, planes) after each frame, planes as readback() returns them.  The last planes are bit for bit the frame of a
        scene created with `total` samples; an earlier one, scaled by total / samples_done on the host, is a preview."""
        S = int(self.scene.sample_count)
        self.set_sample_window(total, 0, total, accumulate=True, advance=True)
        for done in range(S, int(total) + 1, S):
            self.render(stream)
            yield done, self.readback()

    def set_pipeline(self, pipeline: int):
        self._check(lib().rtHipSetPipeline(self.handle, pipeline), "rtHipSetPipeline")

    def stage_timing(self, enable: bool):
        self._check(lib().rtHipStageTiming(self.handle, 1 if enable else 0), "rtHipStageTiming")

    def stage_times_ms(self):
        """Sum over the frames since stage_timing(True): dict of stage -> ms, and rounds of the last frame."""
        ms, rounds = (C.c_double * 5)(), C.c_uint64()
        self._check(lib().rtHipStageTimes(self.handle, C.byref(ms), C.byref(rounds)), "rtHipStageTimes")
        return dict(primary=ms[0], logic=ms[1], trace=ms[2], accum=ms[3], sort=ms[4]), rounds.value

    def debug_counters(self, clear: bool = True):
        out = (C.c_uint64 * 8)()
        self._check(lib().rtHipDebugCounters(self.handle, C.byref(out), 1 if clear else 0), "rtHipDebugCounters")
        return [int(v) for v in out]

    def render_counted(self) -> dict:
        st = Stats()
        self._check(lib().rtHipRenderTilesCounted(self.handle, C.byref(st)), "rtHipRenderTilesCounted")
        return st.as_dict()

    def sync(self, stream: int = 0):
        self._check(lib().rtHipSync(self.handle, stream or None), "rtHipSync")

    def kernel_time_ms(self):
        ms, n = C.c_double(), C.c_uint64()
        self._check(lib().rtHipKernelTime(self.handle, C.byref(ms), C.byref(n)), "rtHipKernelTime")
        return ms.value, n.value

    def tile_buffer(self):
        return lib().rtHipTileBuffer(self.handle), lib().rtHipTileBufferBytes(self.handle)

    def bytes(self) -> int:
        return lib().rtHipSceneBytes(self.handle)

    def readback(self, planes=None):
        sc = self.scene
        if planes is None:
            planes = [np.zeros(sc.pixels, np.uint16) for _ in range(3)]
        self._check(lib().rtHipReadback(self.handle, _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2])), "rtHipReadback")
        return planes

    def set_passes(self, alpha: bool = False, depth: bool = False, triangle: bool = False, normal: bool = False, albedo: bool = False):
        """Render passes from the next frame on (rtHipScenePasses); a buffer whose passes are all off is freed."""
        mask = (PASS_ALPHA if alpha else 0) | (PASS_DEPTH if depth else 0) | (PASS_TRIANGLE if triangle else 0)
        mask |= (PASS_NORMAL if normal else 0) | (PASS_ALBEDO if albedo else 0)
        self._check(lib().rtHipScenePasses(self.handle, mask), "rtHipScenePasses")
        self.passes = mask

    def pass_buffer(self):
        return lib().rtHipPassBuffer(self.handle), lib().rtHipPassBufferBytes(self.handle)

    def surface_buffer(self):
        """The NORMAL / ALBEDO sums on the device ([slot][nx ny nz ar ag ab][128*128] f32), and their size; (None, 0) while both are off."""
        return lib().rtHipSurfaceBuffer(self.handle), lib().rtHipSurfaceBufferBytes(self.handle)

    def readback_passes(self, out: Optional[dict] = None) -> dict:
        """The passes that are on, as [H, W] arrays: alpha u16, depth f32, triangle u32, and with triangle also material i32
        (-1 on a miss) and -- for a scene made by frontend.scene_from_meshes -- mesh i32 (-1 on a miss); normal and albedo as [H, W, 3]
        f32, the means over the pixel's samples.  The material ids are those of the frame that filled the pass buffers, like every
        other pass: the last frame of render() (or that frame rendered again by finish()).  A later set_materials shows in them once
        render() has issued a frame under it; render_counted() runs the megakernel, which writes no pass, so it leaves them alone.  `out`: arrays of an earlier
        call (another instance's tiles) to store this instance's tiles into; pixels of other tiles keep their values."""
        sc = self.scene
        mask = getattr(self, "passes", 0)
        shape = (sc.height, sc.width)
        if out is None:
            out = {}
        if mask & PASS_ALPHA:
            out.setdefault("alpha", np.zeros(shape, np.uint16))
        if mask & PASS_DEPTH:
            out.setdefault("depth", np.full(shape, np.inf, np.float32))
        if mask & PASS_TRIANGLE:
            out.setdefault("triangle", np.full(shape, 0xFFFFFFFF, np.uint32))
        if mask & PASS_NORMAL:
            out.setdefault("normal", np.zeros(shape + (3,), np.float32))
        if mask & PASS_ALBEDO:
            out.setdefault("albedo", np.zeros(shape + (3,), np.float32))
        for k, dt, shp in (("alpha", np.uint16, shape), ("depth", np.float32, shape), ("triangle", np.uint32, shape),
                           ("normal", np.float32, shape + (3,)), ("albedo", np.float32, shape + (3,))):
            if k in out and (out[k].dtype != dt or out[k].shape != shp or not out[k].flags.c_contiguous):
                raise ValueError(f"readback_passes: out[{k!r}] must be a C-contiguous {shp} {np.dtype(dt).name} array")
        self._check(lib().rtHipReadbackPasses(self.handle, _ptr(out.get("alpha")), _ptr(out.get("depth")), _ptr(out.get("triangle"))),
                    "rtHipReadbackPasses")
        if mask & (PASS_NORMAL | PASS_ALBEDO):
            self._check(lib().rtHipReadbackSurfacePasses(self.handle, _ptr(out.get("normal")), _ptr(out.get("albedo"))),
                        "rtHipReadbackSurfacePasses")
        if "triangle" in out:
            tri = out["triangle"]
            hit = tri != 0xFFFFFFFF
            idx = np.where(hit, tri, 0).astype(np.int64)
            mat = np.asarray(getattr(self, "_frame_scene", sc).tri_material, np.int32)
            out["material"] = np.where(hit, mat[idx] if len(mat) else -1, -1).astype(np.int32)
            tri_mesh = getattr(sc, "tri_mesh", None)
            if tri_mesh is not None:
                tm = np.asarray(tri_mesh, np.int32)
                out["mesh"] = np.where(hit, tm[idx] if len(tm) else -1, -1).astype(np.int32)
        return out

    def denoise(self, **params) -> dict:
        """The last frame denoised on the device (rtHipSceneDenoise; keywords as for raytrace.denoise): {"colour": [H, W, 3] f32 C^K,
        "planes": [r, g, b] [H, W] u16}.  Needs set_passes(normal=True, albedo=True) and every tile of the image in this instance."""
        p = denoise_params(**params)
        sc = self.scene
        colour = np.empty((sc.height, sc.width, 3), np.float32)
        planes = [np.empty((sc.height, sc.width), np.uint16) for _ in range(3)]
        self._check(lib().rtHipSceneDenoise(self.handle, C.byref(p), _ptr(colour), _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2])),
                    "rtHipSceneDenoise")
        return {"colour": colour, "planes": planes}

    def denoise_times_ms(self) -> dict:
        """Device time of the last denoise() (rtHipSceneDenoiseTimes): gather, prologue (guides), filter (iterations and output)."""
        ms = (C.c_float * 3)()
        self._check(lib().rtHipSceneDenoiseTimes(self.handle, ms), "rtHipSceneDenoiseTimes")
        return dict(gather=ms[0], prologue=ms[1], filter=ms[2])

    def temporal(self, denoise: Optional[dict] = None, **params) -> dict:
        """The last frame accumulated over the frames before it on the device (rtHipSceneTemporal; keywords max_history and
        depth_tolerance as for raytrace.temporal): {"colour": [H, W, 3] f32, "planes": [r, g, b] [H, W] u16, "count": [H, W] f32, the
        history length of each pixel}.  The loop is set_camera / set_vertices, render(), temporal(); the call marks the scene (mark_motion)
        after itself, so a later motion() measures against this frame.  `denoise`: a dict of raytrace.denoise's keywords ({} for the
        defaults) runs the denoiser on the accumulation before it is returned (needs set_passes(normal=True, albedo=True)); the history
        keeps the unfiltered colour.  Needs every tile of the image in this instance."""
        p = temporal_params(**params)
        d = denoise_params(**denoise) if denoise is not None else None
        sc = self.scene
        colour = np.empty((sc.height, sc.width, 3), np.float32)
        planes = [np.empty((sc.height, sc.width), np.uint16) for _ in range(3)]
        count = np.empty((sc.height, sc.width), np.float32)
        self._check(lib().rtHipSceneTemporal(self.handle, C.byref(p), C.byref(d) if d is not None else None, _ptr(colour), _ptr(planes[0]),
                                             _ptr(planes[1]), _ptr(planes[2]), _ptr(count)), "rtHipSceneTemporal")
        return {"colour": colour, "planes": planes, "count": count}

    def temporal_variance(self, filter: Optional[dict] = None, **params) -> dict:
        """temporal() with the luminance moments carried along (rtHipSceneTemporalVariance): also returns "variance" [H, W] f32.
        `filter`: a dict of raytrace.denoise_variance's keywords ({} for the defaults) runs the variance-guided filter on the accumulation
        (needs set_passes(normal=True, albedo=True)); "colour" and "planes" are then C^K and "variance" is V^K, otherwise the accumulation
        and its temporal variance.  The history keeps the unfiltered colour; a temporal() between two calls makes the next one start again."""
        p = temporal_params(**params)
        v = variance_params(**filter) if filter is not None else None
        sc = self.scene
        colour = np.empty((sc.height, sc.width, 3), np.float32)
        planes = [np.empty((sc.height, sc.width), np.uint16) for _ in range(3)]
        count = np.empty((sc.height, sc.width), np.float32)
        variance = np.empty((sc.height, sc.width), np.float32)
        self._check(lib().rtHipSceneTemporalVariance(self.handle, C.byref(p), C.byref(v) if v is not None else None, _ptr(colour),
                                                     _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2]), _ptr(count), _ptr(variance)),
                    "rtHipSceneTemporalVariance")
        return {"colour": colour, "planes": planes, "count": count, "variance": variance}

    def set_temporal_clamp(self, mode=TEMPORAL_CLAMP_DEFAULTS["mode"], gamma=TEMPORAL_CLAMP_DEFAULTS["gamma"]) -> None:
        """Turns the scene's temporal clamp on (rtHipSceneSetTemporalClamp; include/raytrace_hip.h, "TEMPORAL CLAMP"): from now on
        temporal() and temporal_variance() pull the reprojected history into the frame's 3x3 colour box before the blend, so that a
        set_lights or set_materials shows in one frame instead of fading in over max_history frames.  mode 1 / "minmax", 2 / "variance" or
        3 / "both"; set_temporal_clamp(None) turns it off (the default).  History, mark and buffers are not touched."""
        cp = temporal_clamp_params(mode, gamma) if mode is not None else None
        self._check(lib().rtHipSceneSetTemporalClamp(self.handle, C.byref(cp) if cp is not None else None), "rtHipSceneSetTemporalClamp")

    def temporal_clamp(self) -> Optional[dict]:
        """The scene's temporal clamp (rtHipSceneGetTemporalClamp): {"mode", "gamma"}, or None while it is off."""
        cp = TemporalClampParams()
        on = lib().rtHipSceneGetTemporalClamp(self.handle, C.byref(cp))
        if on < 0:
            self._check(on, "rtHipSceneGetTemporalClamp")
        return dict(mode=int(cp.mode), gamma=float(cp.gamma)) if on else None

    def reset_temporal(self) -> None:
        """Forgets the history of temporal() (rtHipSceneTemporalReset): the next call returns the frame itself with count 1."""
        self._check(lib().rtHipSceneTemporalReset(self.handle), "rtHipSceneTemporalReset")

    def temporal_times_ms(self) -> dict:
        """Device time of the last temporal() (rtHipSceneTemporalTimes): motion pass, gather, accumulate, filter (denoiser, if any, and
        output)."""
        ms = (C.c_float * 4)()
        self._check(lib().rtHipSceneTemporalTimes(self.handle, ms), "rtHipSceneTemporalTimes")
        return dict(motion=ms[0], gather=ms[1], accumulate=ms[2], filter=ms[3])

    def motion_blur(self, **params) -> dict:
        """The last frame blurred along its motion vectors on the device (rtHipSceneMotionBlur; keywords shutter, max_blur, taps and
        depth_softness as for raytrace.motion_blur): {"rgb": [H, W, 3] f32, "planes": [r, g, b] [H, W] u16}.  The loop is mark_motion(),
        set_camera / set_vertices, render(), motion_blur(): the call needs a reference and does NOT mark, the reference stays the
        caller's.  temporal() marks again, so with both on one frame blur first.  Needs every tile of the image in this instance."""
        p = motion_blur_params(**params)
        sc = self.scene
        rgb = np.empty((sc.height, sc.width, 3), np.float32)
        planes = [np.empty((sc.height, sc.width), np.uint16) for _ in range(3)]
        self._check(lib().rtHipSceneMotionBlur(self.handle, C.byref(p), _ptr(rgb), _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2])),
                    "rtHipSceneMotionBlur")
        return {"rgb": rgb, "planes": planes}

    def motion_blur_times_ms(self) -> dict:
        """Device time of the last motion_blur() (rtHipSceneMotionBlurTimes): motion pass, gather, blur (the filter and the output)."""
        ms = (C.c_float * 3)()
        self._check(lib().rtHipSceneMotionBlurTimes(self.handle, ms), "rtHipSceneMotionBlurTimes")
        return dict(motion=ms[0], gather=ms[1], blur=ms[2])

    def depth_of_field(self, aperture=None, focus=None, focus_pixel=None, **params) -> dict:
        """The last frame blurred by its depth pass's circle of confusion on the device (rtHipSceneDepthOfField; keywords coc_scale,
        max_coc, rings and depth_softness as for raytrace.depth_of_field): {"rgb": [H, W, 3] f32, "planes": [r, g, b] [H, W] u16,
        "params": the keywords in effect}.  `focus`: the distance in focus along the ray; `focus_pixel` = (x, y): that pixel's depth
        instead (a ValueError where its ray missed).  `aperture`: a thin lens of that radius in scene units through
        rtHipDepthOfFieldLens and the scene's camera, which sets coc_scale.  Needs set_passes(depth=True) before the frame and every
        tile of the image in this instance."""
        sc = self.scene
        if focus_pixel is not None:
            if focus is not None:
                raise ValueError("depth_of_field: focus and focus_pixel exclude each other")
            if not getattr(self, "passes", 0) & PASS_DEPTH:
                raise RuntimeError("depth_of_field: focus_pixel needs the depth pass (set_passes(depth=True))")
            x, y = (int(v) for v in focus_pixel)
            if not (0 <= x < sc.width and 0 <= y < sc.height):
                raise ValueError(f"depth_of_field: focus_pixel {(x, y)} is not inside the {sc.width} x {sc.height} image")
            depth = np.full((sc.height, sc.width), np.inf, np.float32)
            self._check(lib().rtHipReadbackPasses(self.handle, None, _ptr(depth), None), "rtHipReadbackPasses")
            focus = float(depth[y, x])
            if not (np.isfinite(focus) and focus > 0):
                raise ValueError(f"depth_of_field: the ray of focus_pixel {(x, y)} hit nothing (depth {focus})")
        if focus is not None:
            params["focus"] = focus
        if aperture is not None:
            if "coc_scale" in params:
                raise ValueError("depth_of_field: aperture and coc_scale exclude each other")
            p = dof_lens(self.camera(), aperture, params.pop("focus", DEPTH_OF_FIELD_DEFAULTS["focus"]), **params)
        else:
            p = dof_params(**params)
        rgb = np.empty((sc.height, sc.width, 3), np.float32)
        planes = [np.empty((sc.height, sc.width), np.uint16) for _ in range(3)]
        self._check(lib().rtHipSceneDepthOfField(self.handle, C.byref(p), _ptr(rgb), _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2])),
                    "rtHipSceneDepthOfField")
        used = dict(focus=p.focus, coc_scale=p.cocScale, max_coc=p.maxCoc, rings=p.rings, depth_softness=p.depthSoftness)
        return {"rgb": rgb, "planes": planes, "params": used}

    def depth_of_field_times_ms(self) -> dict:
        """Device time of the last depth_of_field() (rtHipSceneDepthOfFieldTimes): gather of colour and depth, blur, output kernel."""
        ms = (C.c_float * 3)()
        self._check(lib().rtHipSceneDepthOfFieldTimes(self.handle, ms), "rtHipSceneDepthOfFieldTimes")
        return dict(gather=ms[0], blur=ms[1], output=ms[2])

    def ambient_occlusion(self, rays=AO_DEFAULTS["rays"], radius=AO_DEFAULTS["radius"], pixel_samples=AO_DEFAULTS["pixel_samples"],
                          seed=AO_DEFAULTS["seed"], out=None, stream: int = 0):
        """Ambient occlusion from the scene's camera (include/raytrace_hip.h, "AMBIENT OCCLUSION"): per pixel the fraction of `rays`
        cosine-weighted hemisphere rays per pixel sample that travel `radius` unoccluded, over `pixel_samples` jittered samples.  Returns
        [H, W] float32: a numpy array (rtHipSceneAmbientOcclusion) -- `out` if given, else a new one of zeros -- or, when `out` is a
        float32 [H, W] tensor on this scene's device, that tensor, filled by rtHipSceneAmbientOcclusionDevice on torch's current stream
        (or `stream`).  Only the pixels of this instance's tiles are written."""
        p = ao_params(rays, radius, pixel_samples, seed)
        sc = self.scene
        shape = (sc.height, sc.width)
        if hasattr(out, "data_ptr"):
            import torch

            dev = torch.device("cuda", self.device)
            if not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != shape \
                    or not out.is_contiguous():
                raise ValueError(f"ambient_occlusion: out must be a contiguous float32 {shape} tensor on {dev}")
            self._on_torch_stream(stream, [out], lambda run: self._check(lib().rtHipSceneAmbientOcclusionDevice(
                self.handle, C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(run)), "rtHipSceneAmbientOcclusionDevice"))
            return out
        if out is None:
            out = np.zeros(shape, np.float32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == shape and out.flags.c_contiguous):
            raise ValueError(f"ambient_occlusion: out must be a C-contiguous float32 {shape} array")
        self._check(lib().rtHipSceneAmbientOcclusion(self.handle, C.byref(p), _ptr(out)), "rtHipSceneAmbientOcclusion")
        return out

    def mark_motion(self) -> None:
        """Records the camera and the triangles now resident as the reference of motion() (rtHipSceneMotionMark): "the previous frame"."""
        self._check(lib().rtHipSceneMotionMark(self.handle), "rtHipSceneMotionMark")

    def motion_reference_camera(self) -> dict:
        """The camera the last mark_motion() recorded (rtHipSceneMotionReferenceCamera), in camera()'s form; raises before the first mark."""
        cam = Camera()
        self._check(lib().rtHipSceneMotionReferenceCamera(self.handle, C.byref(cam)), "rtHipSceneMotionReferenceCamera")
        return dict(eye=np.array(cam.eye, np.float32), eye_to_top_left=np.array(cam.eyeToTopLeft, np.float32),
                    left_to_right=np.array(cam.leftToRight, np.float32), top_to_bottom=np.array(cam.topToBottom, np.float32),
                    pixel_size_inv=float(cam.pixelSizeInv))

    def motion(self, out: Optional[dict] = None, stream: int = 0) -> dict:
        """Motion vectors against the marked reference (include/raytrace_hip.h, "MOTION VECTORS"): {"motion": [H, W, 2] f32 (from the
        pixel to where its surface point was, in pixels), "t": [H, W] f32, "prev_t": [H, W] f32, "triangle": [H, W] u32 (0xffffffff: a
        miss)} as numpy arrays (rtHipSceneMotion; zeros where this instance's tiles do not reach).  `out`: a dict with any subset of the
        keys; numpy arrays of those shapes are filled and returned with the missing keys left out, and torch tensors on this scene's
        device (float32; triangle uint32 or int32, the ids' bits) are filled by rtHipSceneMotionDevice on torch's current stream (or
        `stream`) and returned as they are."""
        sc = self.scene
        shapes = dict(motion=(sc.height, sc.width, 2), t=(sc.height, sc.width), prev_t=(sc.height, sc.width), triangle=(sc.height, sc.width))
        keys = ("motion", "t", "prev_t", "triangle")
        if out is None:
            out = {k: np.zeros(shapes[k], np.uint32 if k == "triangle" else np.float32) for k in keys}
        unknown = [k for k in out if k not in keys]
        if unknown or not out:
            raise ValueError(f"motion: out takes a non-empty subset of {keys} (got {sorted(out)})")
        if any(hasattr(v, "data_ptr") for v in out.values()):
            import torch

            dev = torch.device("cuda", self.device)
            for k, v in out.items():
                kinds = (torch.uint32, torch.int32) if k == "triangle" else (torch.float32,)
                if not isinstance(v, torch.Tensor) or v.device != dev or v.dtype not in kinds or tuple(v.shape) != shapes[k] or not v.is_contiguous():
                    raise ValueError(f"motion: out[{k!r}] must be a contiguous {kinds[0]} {shapes[k]} tensor on {dev}")
            ptrs = [C.c_void_p(out[k].data_ptr()) if k in out else None for k in keys]
            self._on_torch_stream(stream, list(out.values()), lambda run: self._check(lib().rtHipSceneMotionDevice(
                self.handle, *ptrs, C.c_void_p(run)), "rtHipSceneMotionDevice"))
            return out
        for k, v in out.items():
            kind = np.uint32 if k == "triangle" else np.float32
            if not (isinstance(v, np.ndarray) and v.dtype == kind and v.shape == shapes[k] and v.flags.c_contiguous):
                raise ValueError(f"motion: out[{k!r}] must be a C-contiguous {np.dtype(kind).name} {shapes[k]} array")
        self._check(lib().rtHipSceneMotion(self.handle, *[_ptr(out.get(k)) for k in keys]), "rtHipSceneMotion")
        return out

    def set_matte_groups(self, groups) -> None:
        """The group table of mattes(kind="group") (rtHipSceneSetMatteGroups): one u32 id per triangle, 0xffffffff = in no group; a numpy
        array (any integer type whose values fit u32), or a torch tensor (uint32 or int32, the ids' bits) on the scene's GPU, handed over
        as a device pointer once torch's current stream has been synchronised.  The scene keeps a copy of its own.  None frees the table."""
        self._mesh_groups = False
        if groups is None:
            self._check(lib().rtHipSceneSetMatteGroups(self.handle, None, 0), "rtHipSceneSetMatteGroups")
            return
        T = self.scene.triangle_count
        if hasattr(groups, "data_ptr"):
            import torch

            if groups.dtype not in (torch.uint32, torch.int32) or tuple(groups.shape) != (T,):
                raise ValueError(f"set_matte_groups: {groups.dtype} {tuple(groups.shape)}, expected uint32 or int32 [{T}]")
            if not groups.is_cuda or groups.device.index != self.device:
                raise ValueError(f"set_matte_groups: a torch tensor must live on the scene's GPU {self.device} (pass a numpy array for host memory)")
            ids = groups.contiguous()
            torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()  # the call has no stream argument
            on_device = 1
        else:
            g = np.asarray(groups)
            if g.shape != (T,) or g.dtype.kind not in "iu":
                raise ValueError(f"set_matte_groups: {g.dtype} {g.shape}, expected integers [{T}]")
            if g.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)):
                if g.size and (int(g.min()) < 0 or int(g.max()) > MATTE_NONE):
                    raise ValueError("set_matte_groups: an id does not fit 32 bits")
                g = g.astype(np.uint32)
            ids = np.ascontiguousarray(g).view(np.uint32)
            on_device = 0
        self._check(lib().rtHipSceneSetMatteGroups(self.handle, _ptr(ids), on_device), "rtHipSceneSetMatteGroups")

    def matte_defaults(self) -> dict:
        """rtHipMatteDefaults: kind triangle, no selected id, 4 layers, and {total, first, samples} of the last issued frame's window."""
        p = MatteParams()
        self._check(lib().rtHipMatteDefaults(self.handle, C.byref(p)), "rtHipMatteDefaults")
        kind = [k for k, v in MATTE_KINDS.items() if v == p.kind][0]
        return dict(kind=kind, select=tuple(p.select[:p.selectCount]), layers=int(p.layers), total=int(p.total), first=int(p.first),
                    samples=int(p.samples))

    def mattes(self, kind: str = "triangle", select=(), layers: int = 4, total: Optional[int] = None, first: Optional[int] = None,
               samples: Optional[int] = None, out: Optional[dict] = None, stream: int = 0) -> dict:
        """Anti-aliased id coverage over each pixel's samples (include/raytrace_hip.h, "MATTES").  kind: "triangle", "material", "group"
        (the table of set_matte_groups) or "mesh" (scene.tri_mesh, installed as the group table once).  select: up to 16 ids, one coverage
        plane each; layers: K <= 8 ranked (id, coverage) layers per pixel.  total, first, samples: the sample window {N, f} and the number
        of samples C; None takes rtHipMatteDefaults' value (the last issued frame's window and the scene's sample count).
        Returns {"select": [M, H, W] f32, "layer_id": [K, H, W] u32 (0xffffffff: an unused slot), "layer_coverage": [K, H, W] f32,
        "rest": [H, W] f32} as numpy arrays (rtHipSceneMattes; zeros where this instance's tiles do not reach; "select" is left out for
        M = 0, the layer arrays for K = 0).  `out`: a dict with any subset of the keys; numpy arrays of those shapes are filled and
        returned with the missing keys left out, and torch tensors on this scene's device (float32; layer_id uint32 or int32, the ids'
        bits) are filled by rtHipSceneMattesDevice on torch's current stream (or `stream`) and returned as they are."""
        if kind == "mesh":
            if getattr(self.scene, "tri_mesh", None) is None:
                raise ValueError("mattes: kind 'mesh' needs a scene with tri_mesh (frontend.scene_from_meshes)")
            if not getattr(self, "_mesh_groups", False):
                self.set_matte_groups(np.asarray(self.scene.tri_mesh, np.int32))
                self._mesh_groups = True
        elif kind not in MATTE_KINDS:
            raise ValueError(f"mattes: kind {kind!r} is not one of {sorted(MATTE_KINDS) + ['mesh']}")
        select = [int(v) for v in select]
        if len(select) > MATTE_MAX_SELECT or any(not 0 <= v <= MATTE_NONE for v in select):
            raise ValueError(f"mattes: select takes at most {MATTE_MAX_SELECT} u32 ids")
        p = MatteParams()
        self._check(lib().rtHipMatteDefaults(self.handle, C.byref(p)), "rtHipMatteDefaults")
        p.kind = MATTE_KINDS["group" if kind == "mesh" else kind]
        for name, v in (("total", total), ("first", first), ("samples", samples), ("layers", layers)):
            if v is not None:
                if not 0 <= int(v) <= MATTE_NONE:
                    raise ValueError(f"mattes: {name} = {v} does not fit 32 bits")
                setattr(p, name, int(v))
        p.selectCount = len(select)
        for m, v in enumerate(select):
            p.select[m] = v
        if lib().rtHipMatteCheck(C.byref(p)) != 0:
            raise ValueError(last_error())
        sc = self.scene
        M, K, H, W = len(select), int(p.layers), sc.height, sc.width
        keys = ("select", "layer_id", "layer_coverage", "rest")
        shapes = dict(select=(M, H, W), layer_id=(K, H, W), layer_coverage=(K, H, W), rest=(H, W))
        if out is None:
            out = {k: np.zeros(shapes[k], np.uint32 if k == "layer_id" else np.float32) for k in keys if shapes[k][0]}
        unknown = [k for k in out if k not in keys]
        if unknown or not out:
            raise ValueError(f"mattes: out takes a non-empty subset of {keys} (got {sorted(out)})")
        if any(hasattr(v, "data_ptr") for v in out.values()):
            import torch

            dev = torch.device("cuda", self.device)
            for k, v in out.items():
                kinds = (torch.uint32, torch.int32) if k == "layer_id" else (torch.float32,)
                if not isinstance(v, torch.Tensor) or v.device != dev or v.dtype not in kinds or tuple(v.shape) != shapes[k] or not v.is_contiguous():
                    raise ValueError(f"mattes: out[{k!r}] must be a contiguous {kinds[0]} {shapes[k]} tensor on {dev}")
            ptrs = [C.c_void_p(out[k].data_ptr()) if k in out else None for k in keys]
            self._on_torch_stream(stream, list(out.values()), lambda run: self._check(lib().rtHipSceneMattesDevice(
                self.handle, C.byref(p), *ptrs, C.c_void_p(run)), "rtHipSceneMattesDevice"))
            return out
        for k, v in out.items():
            want = np.uint32 if k == "layer_id" else np.float32
            if not (isinstance(v, np.ndarray) and v.dtype == want and v.shape == shapes[k] and v.flags.c_contiguous):
                raise ValueError(f"mattes: out[{k!r}] must be a C-contiguous {np.dtype(want).name} {shapes[k]} array")
        self._check(lib().rtHipSceneMattes(self.handle, C.byref(p), *[_ptr(out.get(k)) for k in keys]), "rtHipSceneMattes")
        return out

    def matte_times_ms(self) -> dict:
        """Device time of the last mattes() (rtHipSceneMatteTimes): the count launches and the finish kernel; waits for that call."""
        ms = (C.c_double * 2)()
        self._check(lib().rtHipSceneMatteTimes(self.handle, C.byref(ms)), "rtHipSceneMatteTimes")
        return dict(count=ms[0], finish=ms[1])

    def _on_torch_stream(self, stream, tensors, call):
        """call(hipStream_t as int) on torch's current stream of this scene's device, or on `stream`, ordered after the current stream's
        work and before its later work; `tensors` are recorded on a stream other than the current one."""
        import torch

        dev = torch.device("cuda", self.device)
        cur = torch.cuda.current_stream(dev)
        if stream and stream != cur.cuda_stream:
            run = torch.cuda.ExternalStream(stream, device=dev)
        elif cur.cuda_stream:
            run = cur
        else:  # the null stream would mean "the scene's own stream" to the library (see _intersect_torch)
            if getattr(self, "_side_stream", None) is None:
                self._side_stream = torch.cuda.Stream(dev)
            run = self._side_stream
        if run is not cur:
            run.wait_stream(cur)
        call(run.cuda_stream)
        if run is not cur:
            cur.wait_stream(run)
            for t in tensors:
                t.record_stream(run)

    def bake_ambient_occlusion(self, width, height, rays=BAKE_DEFAULTS["rays"], radius=BAKE_DEFAULTS["radius"], seed=BAKE_DEFAULTS["seed"],
                               dilate=BAKE_DEFAULTS["dilate"], triangles=None, material=None, out=None, triangle_out=None, stream: int = 0) -> dict:
        """Ambient occlusion baked into a width x height texture over the scene's UVs (include/raytrace_hip.h, "AMBIENT OCCLUSION
        BAKE"): per texel the fraction of `rays` cosine-weighted hemisphere rays from the covering triangle's surface point that travel
        `radius` unoccluded, then `dilate` gutter-fill passes.  triangles: None (all), a range or (first, count); material: None or the
        only material id baked.  Returns {"ao": [H, W] f32, "triangle": [H, W] winner ids (0xffffffff: uncovered)}: numpy arrays
        (rtHipSceneBakeAmbientOcclusion; `out` / `triangle_out` if given, u32) or, when `out` is a float32 [H, W] tensor on this scene's
        device, tensors filled by rtHipSceneBakeAmbientOcclusionDevice on torch's current stream (or `stream`): `triangle_out` an int32
        [H, W] tensor there (the ids' bits), or a new one."""
        p = bake_params(width, height, rays, radius, seed, dilate, triangles, material)
        shape = (int(height), int(width))
        if hasattr(out, "data_ptr"):
            import torch

            dev = torch.device("cuda", self.device)
            for t, dt, name in ((out, torch.float32, "out"), (triangle_out, torch.int32, "triangle_out")):
                if t is not None and (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or tuple(t.shape) != shape
                                      or not t.is_contiguous()):
                    raise ValueError(f"bake_ambient_occlusion: {name} must be a contiguous {dt} {shape} tensor on {dev}")
            if triangle_out is None:
                triangle_out = torch.empty(shape, dtype=torch.int32, device=dev)
            self._on_torch_stream(stream, [out, triangle_out], lambda run: self._check(lib().rtHipSceneBakeAmbientOcclusionDevice(
                self.handle, C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(triangle_out.data_ptr()), C.c_void_p(run)),
                "rtHipSceneBakeAmbientOcclusionDevice"))
            return dict(ao=out, triangle=triangle_out)
        if out is None:
            out = np.zeros(shape, np.float32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == shape and out.flags.c_contiguous):
            raise ValueError(f"bake_ambient_occlusion: out must be a C-contiguous float32 {shape} array")
        if triangle_out is None:
            triangle_out = np.zeros(shape, np.uint32)
        elif not (isinstance(triangle_out, np.ndarray) and triangle_out.dtype == np.uint32 and triangle_out.shape == shape
                  and triangle_out.flags.c_contiguous):
            raise ValueError(f"bake_ambient_occlusion: triangle_out must be a C-contiguous uint32 {shape} array")
        self._check(lib().rtHipSceneBakeAmbientOcclusion(self.handle, C.byref(p), _ptr(out), _ptr(triangle_out)), "rtHipSceneBakeAmbientOcclusion")
        return dict(ao=out, triangle=triangle_out)

    def intersect(self, origins, directions, tmin=0.0, tmax=np.inf, exclude=None, stream: int = 0) -> dict:
        """What rays hit in this scene: the reference's grid walk, RayIntersectsTriangles (raytrace_opencl.c:324-401), bit for bit
        (contract in include/raytrace_hip.h, rtHipSceneIntersect).  origins, directions: [N, 3] float32; tmin, tmax, exclude
        (triangle ids, 0xffffffff = none): scalars or [N].  Returns t, triangle (u32, 0xffffffff on a miss), ab, ac (0 on a miss), hit,
        position (o + t*d in float32) and material (i32, -1 on a miss) -- and mesh for a scene made by frontend.scene_from_meshes.
        numpy inputs go through the host entry point.  torch tensors on this scene's device never leave it: the rays are packed on the
        device, the query runs on torch's current stream (or `stream`), and the results are tensors on that device."""
        if hasattr(origins, "data_ptr") or hasattr(directions, "data_ptr"):
            return self._intersect_torch(origins, directions, tmin, tmax, exclude, stream)
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(directions, np.float32)
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError(f"intersect: origins and directions must both be [N, 3] (got {o.shape} and {d.shape})")
        n = o.shape[0]
        if n >= 1 << 32:
            raise ValueError("intersect: at most 2^32 - 1 rays per call")
        rays = np.empty((n, 8), np.float32)
        rays[:, 0:3] = o
        rays[:, 4:7] = d
        try:
            rays[:, 3] = np.broadcast_to(np.asarray(tmin, np.float32), (n,))
            rays[:, 7] = np.broadcast_to(np.asarray(tmax, np.float32), (n,))
            excl = None if exclude is None else np.ascontiguousarray(np.broadcast_to(np.asarray(exclude).astype(np.uint32), (n,)))
        except ValueError as e:
            raise ValueError(f"intersect: tmin, tmax and exclude must be scalars or [{n}] arrays ({e})") from None
        hits = np.zeros((n, 4), np.float32)
        self._check(lib().rtHipSceneIntersect(self.handle, _ptr(rays), _ptr(excl), n, _ptr(hits)), "rtHipSceneIntersect")
        t = hits[:, 0].copy()
        tri = hits[:, 1].copy().view(np.uint32)
        hit = tri != 0xFFFFFFFF
        idx = np.where(hit, tri, 0).astype(np.int64)
        out = dict(t=t, triangle=tri, ab=hits[:, 2].copy(), ac=hits[:, 3].copy(), hit=hit, position=o + t[:, None] * d)
        for key, table in (("material", self.scene.tri_material), ("mesh", getattr(self.scene, "tri_mesh", None))):
            if key == "mesh" and table is None:
                continue
            table = np.asarray(table, np.int32)
            out[key] = np.where(hit, table[idx] if len(table) else -1, -1).astype(np.int32)
        return out

    def _intersect_torch(self, origins, directions, tmin, tmax, exclude, stream):
        import torch

        dev = torch.device("cuda", self.device)

        def on_device(name, v):
            if not isinstance(v, torch.Tensor) or v.device != dev:
                where = v.device if isinstance(v, torch.Tensor) else type(v).__name__
                raise ValueError(f"intersect: {name} must be a tensor on {dev} (the scene's device), not {where}")
            return v

        o = on_device("origins", origins).to(torch.float32)
        d = on_device("directions", directions).to(torch.float32)
        if o.dim() != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError(f"intersect: origins and directions must both be [N, 3] (got {tuple(o.shape)} and {tuple(d.shape)})")
        n = o.shape[0]
        if n >= 1 << 32:
            raise ValueError("intersect: at most 2^32 - 1 rays per call")

        def per_ray(name, v, dtype):
            """A [n] tensor on the device, or a Python scalar (filled in on the device: no host-to-device copy)."""
            if not isinstance(v, torch.Tensor) and np.ndim(v) == 0:
                return np.asarray(v, np.float32 if dtype == torch.float32 else np.int64).item()
            v = on_device(name, v) if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v), device=dev)
            if v.dim() > 1 or (v.dim() == 1 and v.shape[0] != n):
                raise ValueError(f"intersect: {name} must be a scalar or a [{n}] tensor (got {tuple(v.shape)})")
            return v.to(dtype).expand(n)

        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        rays[:, 0:3] = o
        rays[:, 4:7] = d
        rays[:, 3] = per_ray("tmin", tmin, torch.float32)
        rays[:, 7] = per_ray("tmax", tmax, torch.float32)
        excl = None
        if exclude is not None:
            e = per_ray("exclude", exclude, torch.int64)
            if isinstance(e, int):
                e &= 0xFFFFFFFF
                excl = torch.full((n,), e - (1 << 32) if e >= 1 << 31 else e, dtype=torch.int32, device=dev)
            else:
                e = e & 0xFFFFFFFF
                excl = torch.where(e >= 1 << 31, e - (1 << 32), e).to(torch.int32).contiguous()  # the u32 bits in an int32 tensor
        hits = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        # The query runs on `run`: torch's current stream, or the caller's `stream`, or -- when the current stream is the null stream, which
        # the library would take for "the scene's own stream" -- a side stream of this scene.  A stream other than the current one is ordered
        # after the packing above and before everything enqueued on the current stream afterwards (events, no host synchronisation), and
        # the buffers are recorded on it so that the caching allocator does not hand them out while the query may still use them.
        cur = torch.cuda.current_stream(dev)
        if stream and stream != cur.cuda_stream:
            run = torch.cuda.ExternalStream(stream, device=dev)
        elif cur.cuda_stream:
            run = cur
        else:
            if getattr(self, "_side_stream", None) is None:
                self._side_stream = torch.cuda.Stream(dev)
            run = self._side_stream
        if run is not cur:
            run.wait_stream(cur)
        self._check(lib().rtHipSceneIntersectDevice(self.handle, C.c_void_p(rays.data_ptr()), None if excl is None else C.c_void_p(excl.data_ptr()),
                                                    n, C.c_void_p(hits.data_ptr()), C.c_void_p(run.cuda_stream)), "rtHipSceneIntersectDevice")
        if run is not cur:
            cur.wait_stream(run)
            for buf in (rays, excl, hits):
                if buf is not None:
                    buf.record_stream(run)
        bits = hits.view(torch.int32)
        t = hits[:, 0].contiguous()
        tri32 = bits[:, 1].contiguous()
        hit = tri32 != -1
        idx = torch.where(hit, tri32.to(torch.int64) & 0xFFFFFFFF, 0)
        out = dict(t=t, triangle=tri32.view(torch.uint32), ab=hits[:, 2].contiguous(), ac=hits[:, 3].contiguous(), hit=hit,
                   position=o + t[:, None] * d)
        for key, table in self._device_id_tables(dev).items():
            none = torch.full_like(tri32, -1)
            out[key] = torch.where(hit, table[idx], none) if table.numel() else none
        return out

    def _device_id_tables(self, dev) -> dict:
        """The scene's per-triangle material (and mesh) ids as int32 tensors on `dev`, uploaded once per scene."""
        tables = getattr(self, "_id_tables", None)
        if tables is None:
            import torch
            tables = {"material": torch.as_tensor(np.asarray(self.scene.tri_material, np.int32), device=dev)}
            if getattr(self.scene, "tri_mesh", None) is not None:
                tables["mesh"] = torch.as_tensor(np.asarray(self.scene.tri_mesh, np.int32), device=dev)
            self._id_tables = tables
        return tables

def render_resident(sc: Scene, device: int = 0):
    """Upload, render every tile once, read back: returns [H,W] uint16 R,G,B."""
    rs = ResidentScene(sc, device)
    try:
        rs.render()
        planes = rs.readback()
    finally:
        rs.close()
    return [p.reshape(sc.height, sc.width) for p in planes]
