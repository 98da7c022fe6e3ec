"""Host-side mirror of the reference's renderer API, bound to the MI355X-native shared libraries.

The reference's host interface for the render hot path is three ``extern "C"`` functions
(/root/reference/kernels.h:6-8) called from ``main()`` (/root/reference/main.cpp:94-101,138):

    initRenderer(ksc, cam, &fb, nx, ny, maxDepth); runRenderer(ns, tx, ty); cleanupRenderer();

This module binds exactly those symbols (plus the additive ones of include/rt_api.h) from
``librt_mi355x.so`` with ctypes, and the host-side scene / BVH / PPM / .ref helpers of
include/rt_host.h from ``librt_host.so``.  Same names, same argument meaning, same error
behaviour (a HIP failure prints and ``exit(99)``s the process, /root/reference/kernels.cu:27-38).

There is NO CPU fallback: if ``librt_mi355x.so`` is missing the import of the renderer fails
loudly (``load_renderer``), and without a GPU ``initRenderer*`` terminates the process the way
the reference does.  The CPU oracle lives in ``oracle/`` and is never imported from here.

Directory name contains '-' (it mirrors the reference repo's name), so import it through the
``cuda_raytracing_optimized_amd`` alias module at the repo root.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
RENDERER_LIB = os.path.join(_HERE, "librt_mi355x.so")
HOST_LIB = os.path.join(_HERE, "librt_host.so")

RT_DIFFUSE, RT_METAL, RT_GLASS = 0, 1, 2
# additive: the reference's dormant look presets (scene_materials.h:22-93), see include/rt_types.h
(RT_FLOOR_COAT, RT_FLOOR_DIFFUSE, RT_FLOOR_CHECKER, RT_MODEL_COAT, RT_MODEL_DIFFUSE, RT_MODEL_GLOSSY, RT_MODEL_GLASS,
 RT_MODEL_TINTEDGLASS, RT_MODEL_SSS) = range(3, 12)
RT_SKY_CONST_GREY, RT_SKY_GRADIENT = 0, 1
RT_RNG_REFERENCE_STREAM, RT_RNG_COUNTER = 0, 1
RT_FP_PARITY, RT_FP_FAST = 0, 1
RT_MAX_DEVICES = 8

# ---------------------------------------------------------------------------------------------
# ctypes mirrors of include/rt_types.h (layouts identical to /root/reference/helper_structs.h)
# ---------------------------------------------------------------------------------------------


class vec3(C.Structure):
    _fields_ = [("e", C.c_float * 3)]


class camera(C.Structure):
    _fields_ = [("origin", vec3), ("lower_left_corner", vec3), ("horizontal", vec3), ("vertical", vec3),
                ("u", vec3), ("v", vec3), ("w", vec3), ("lens_radius", C.c_float)]


class sphere(C.Structure):
    _fields_ = [("center", vec3), ("radius", C.c_float)]


class plane(C.Structure):
    _fields_ = [("norm", vec3), ("point", vec3)]


class bbox(C.Structure):
    _fields_ = [("min", vec3), ("max", vec3)]


class triangle(C.Structure):
    _fields_ = [("v", vec3 * 3), ("texCoords", C.c_float * 6), ("meshID", C.c_ubyte), ("_pad", C.c_ubyte * 3)]


class bvh_node(C.Structure):
    _fields_ = [("a", vec3), ("b", vec3)]


class material(C.Structure):
    _fields_ = [("type", C.c_int32), ("color", vec3), ("param", C.c_float), ("texId", C.c_int32)]


class stexture(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_float)), ("width", C.c_int32), ("height", C.c_int32)]


class mesh(C.Structure):
    _fields_ = [("tris", C.POINTER(triangle)), ("numTris", C.c_uint32), ("bvh", C.POINTER(bvh_node)),
                ("numBvhNodes", C.c_int32), ("bounds", bbox)]


class kernel_scene(C.Structure):
    _fields_ = [("m", C.POINTER(mesh)), ("floor", plane), ("materials", C.POINTER(material)),
                ("numMaterials", C.c_int32), ("textures", C.POINTER(stexture)), ("numTextures", C.c_int32),
                ("numPrimitivesPerLeaf", C.c_int32)]


class render_options(C.Structure):
    _fields_ = [("sky", C.c_int32), ("nee", C.c_int32), ("rr", C.c_int32), ("t_min", C.c_float),
                ("rng", C.c_int32), ("fp", C.c_int32), ("light", sphere), ("lightColor", vec3),
                ("stripe_rows", C.c_int32), ("num_devices", C.c_int32), ("devices", C.c_int32 * RT_MAX_DEVICES),
                ("part_rank", C.c_int32), ("part_world", C.c_int32), ("variant", C.c_int32), ("counters", C.c_int32),
                ("samples_per_item", C.c_int32), ("floor", C.c_int32)]


class render_stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("samples", C.c_int64),
                ("num_launches", C.c_int32), ("vgprs", C.c_int32), ("rays", C.c_uint64),
                ("prim_tests", C.c_uint64), ("node_visits", C.c_uint64), ("exec_tests", C.c_uint64),
                ("shadow_rays", C.c_uint64), ("box_tests", C.c_uint64), ("ref_stats", C.c_uint64 * 18)]


# indices into render_stats.ref_stats: the reference's STATS counters, /root/reference/kernels.cu:47-67
(RT_STAT_PRIMARY, RT_STAT_PRIMARY_HIT_MESH, RT_STAT_PRIMARY_NOHITS, RT_STAT_PRIMARY_BBOX_NOHITS, RT_STAT_SECONDARY,
 RT_STAT_SECONDARY_MESH, RT_STAT_SECONDARY_NOHIT, RT_STAT_SECONDARY_MESH_NOHIT, RT_STAT_SECONDARY_BBOX_NOHIT, RT_STAT_SHADOWS,
 RT_STAT_SHADOWS_BBOX_NOHITS, RT_STAT_SHADOWS_NOHITS, RT_STAT_LOW_POWER, RT_STAT_EXCEED_MAX_BOUNCE, RT_STAT_RUSSIAN_KILL,
 RT_STAT_NAN, RT_STAT_NODES_BOTH, RT_STAT_NODES_SINGLE) = range(18)
RT_STAT_NAMES = ["primary", "primary hit mesh", "primary nohit", "primary bb nohit", "secondary", "secondary mesh", "secondary no hit",
                 "secondary mesh nohit", "secondary bb nohit", "shadows", "shadows bb nohit", "shadows nohit", "power < 0.01",
                 "exceeded max bounce", "russian roulette", "NaNs", "both nodes hit", "single node hit"]


_SIZES = {vec3: 12, camera: 88, sphere: 16, plane: 24, bbox: 24, triangle: 64, bvh_node: 24, material: 24,
          stexture: 16, mesh: 56, kernel_scene: 64}
for _t, _s in _SIZES.items():
    assert C.sizeof(_t) == _s, (_t, C.sizeof(_t), _s)

# numpy views of the array-of-struct types
sphere_dtype = np.dtype([("center", np.float32, 3), ("radius", np.float32)])
material_dtype = np.dtype([("type", np.int32), ("color", np.float32, 3), ("param", np.float32), ("texId", np.int32)])
triangle_dtype = np.dtype([("v", np.float32, (3, 3)), ("texCoords", np.float32, 6), ("meshID", np.uint8), ("_pad", np.uint8, 3)])
bvh_node_dtype = np.dtype([("a", np.float32, 3), ("b", np.float32, 3)])
assert sphere_dtype.itemsize == 16 and material_dtype.itemsize == 24
assert triangle_dtype.itemsize == 64 and bvh_node_dtype.itemsize == 24

# symbols every library must export (tests check the .so against the headers with these)
RENDERER_SYMBOLS = ["initRenderer", "runRenderer", "cleanupRenderer", "initRendererSpheres",
                    "getDefaultRenderOptions", "setRenderOptions", "setExternalFramebuffer", "getRenderStats",
                    "rtDeviceCount", "rtApiVersion", "rtStructSizes", "rtLastLaunches",
                    "runRendererProgressive", "rtProgressiveSamples", "rtResetProgressive", "setCamera",
                    "renderGuides", "rtLastGuidesMs",
                    "rtDefaultDenoiseFlags", "denoiseFrame", "rtLastDenoiseMs",
                    "accumulateFrame", "rtResetHistory", "rtHistoryFrames", "rtLastAccumulateMs",
                    "previewFrame", "rtResetPreview", "rtPreviewFrames", "rtLastPreviewMs",
                    "displayFrame", "rtLastExposure", "rtDisplayHistogram", "rtResetDisplay", "rtLastDisplayMs",
                    "traceRays", "occludedRays", "rtLastRaysMs",
                    "renderPixels", "rtLastPixelsMs",
                    "radianceRays", "rtLastRadianceMs",
                    "rtGatherWidth", "gatherRadiance", "rtGatherDirections", "rtLastGatherMs",
                    "rasterTexels", "bakeTexels", "rtLastTexelsMs", "rtLastBakeMs",
                    "filterTexels", "rtLastFilterMs",
                    "sampleTexels", "renderLightmap", "rtLastSampleMs", "rtLastLightmapMs",
                    "refineFrame", "rtResetRefine", "rtRefineSamples", "rtRefineLastList", "rtLastRefineMs",
                    "updateTriangles", "updateMaterials", "updateSpheres", "getMeshBvh", "rtLastUpdateMs",
                    "rebuildBvh", "rtLastRebuildMs",
                    "rtMarkPose", "rtClearPose", "rtPoseMarked", "renderMotion", "rtLastMotionMs",
                    "rtLastSphereForm"]
RT_API_VERSION = 1002       # include/rt_api.h: the version this mirror was written against
# the structs that cross the C-ABI, in the order of the RT_SIZEOF_* indices of include/rt_api.h
ABI_STRUCTS = [render_options, render_stats, camera, sphere, material, triangle, bvh_node, mesh, kernel_scene, stexture, plane, bbox, vec3]
HOST_SYMBOLS = ["rtMakeCamera", "rtRandomFloat", "rtSceneThreeSpheres", "rtSceneRandomSpheres", "rtStaircaseCamera",
                "rtBuildBvh", "rtBuildBvhLevels", "rtLoadBvhFile", "rtSaveBvhFile", "rtFreeMesh", "rtMeshView",
                "rtSceneStaircaseProcedural", "rtLinearToSRGB", "rtWritePPM", "rtSaveReference", "rtLoadReference", "rtRmse",
                "rtDisplayFrameHost", "rtCentreRays", "rtPinholeCamera", "rtRefitBvhArrays", "rtRefitBvh", "rtRebuildBvhArrays", "rtRebuildBvh",
                "rtGatherDirectionsHost", "rtRasterTexelsHost", "rtAtlasGrid", "rtFilterTexelsHost", "rtSampleTexelsHost"]

_renderer = None
_host = None


def load_host():
    """librt_host.so (plain C++; works without a GPU)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise ImportError(f"{HOST_LIB} is not built: run `make` (or __graft_entry__.build())")
        h = C.CDLL(HOST_LIB)
        fp = C.POINTER(C.c_float)
        h.rtMakeCamera.argtypes = [fp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(camera)]
        h.rtMakeCamera.restype = None
        h.rtRandomFloat.argtypes = [C.POINTER(C.c_uint32)]
        h.rtRandomFloat.restype = C.c_float
        h.rtSceneThreeSpheres.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(camera)]
        h.rtSceneThreeSpheres.restype = C.c_int
        h.rtSceneRandomSpheres.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(camera)]
        h.rtSceneRandomSpheres.restype = C.c_int
        h.rtStaircaseCamera.argtypes = [C.c_int, C.c_int, C.POINTER(camera)]
        h.rtStaircaseCamera.restype = None
        h.rtBuildBvh.argtypes = [C.c_void_p, C.c_int, C.c_int]
        h.rtBuildBvh.restype = C.c_void_p
        h.rtBuildBvhLevels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        h.rtBuildBvhLevels.restype = C.c_void_p
        h.rtLoadBvhFile.argtypes = [C.c_char_p]
        h.rtLoadBvhFile.restype = C.c_void_p
        h.rtSaveBvhFile.argtypes = [C.c_void_p, C.c_char_p]
        h.rtSaveBvhFile.restype = C.c_int
        h.rtFreeMesh.argtypes = [C.c_void_p]
        h.rtFreeMesh.restype = None
        h.rtMeshView.argtypes = [C.c_void_p, C.POINTER(mesh)]
        h.rtMeshView.restype = C.c_int
        h.rtSceneStaircaseProcedural.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        h.rtSceneStaircaseProcedural.restype = C.c_int
        h.rtLinearToSRGB.argtypes = [C.c_float]
        h.rtLinearToSRGB.restype = C.c_uint32
        h.rtWritePPM.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        h.rtWritePPM.restype = C.c_int
        h.rtSaveReference.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        h.rtSaveReference.restype = C.c_int
        h.rtLoadReference.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
        h.rtLoadReference.restype = C.c_int
        h.rtRmse.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        h.rtRmse.restype = C.c_double
        h.rtDisplayFrameHost.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float),
                                         C.POINTER(C.c_uint32)]
        h.rtDisplayFrameHost.restype = C.c_int
        h.rtCentreRays.argtypes = [C.POINTER(camera), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, fp, fp]
        h.rtCentreRays.restype = None
        h.rtPinholeCamera.argtypes = [fp, fp, C.POINTER(camera)]
        h.rtPinholeCamera.restype = None
        h.rtRefitBvhArrays.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.POINTER(bbox)]
        h.rtRefitBvhArrays.restype = C.c_int
        h.rtRefitBvh.argtypes = [C.c_void_p]
        h.rtRefitBvh.restype = C.c_int
        h.rtRebuildBvhArrays.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.POINTER(bbox), C.c_void_p]
        h.rtRebuildBvhArrays.restype = C.c_int
        h.rtRebuildBvh.argtypes = [C.c_void_p, C.c_void_p]
        h.rtRebuildBvh.restype = C.c_int
        h.rtGatherDirectionsHost.argtypes = [C.c_int, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_float, fp, fp, C.POINTER(C.c_uint32)]
        h.rtGatherDirectionsHost.restype = None
        i32p = C.POINTER(C.c_int32)
        h.rtRasterTexelsHost.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, i32p, i32p, fp, fp, fp]
        h.rtRasterTexelsHost.restype = C.c_int
        h.rtAtlasGrid.argtypes = [C.c_void_p, C.c_int, C.c_float]
        h.rtAtlasGrid.restype = C.c_int
        h.rtFilterTexelsHost.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
        h.rtFilterTexelsHost.restype = C.c_int
        h.rtSampleTexelsHost.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_int32), fp, fp, C.c_int, C.c_int, C.c_int, fp, C.c_int, fp,
                                         C.POINTER(C.c_uint8)]
        h.rtSampleTexelsHost.restype = C.c_int
        _host = h
    return _host


def check_abi(lib, path=RENDERER_LIB, structs=None):
    """Version + struct-size handshake with a loaded librt_mi355x.so.  getDefaultRenderOptions / getRenderStats write sizeof(struct) bytes
    through the caller's pointer: a mirror of another generation than the library must be an ImportError here, not a heap overrun there
    (what the round-2 crash was: a rebuilt library beside a stale mirror)."""
    structs = ABI_STRUCTS if structs is None else structs
    if not hasattr(lib, "rtStructSizes"):
        raise ImportError(f"{path} predates the ABI handshake (no rtStructSizes): rebuild it with `make`")
    lib.rtApiVersion.argtypes = []
    lib.rtApiVersion.restype = C.c_int
    lib.rtStructSizes.argtypes = [C.POINTER(C.c_int32), C.c_int]
    lib.rtStructSizes.restype = C.c_int
    ver = lib.rtApiVersion()
    if ver != RT_API_VERSION:
        raise ImportError(f"{path} has API version {ver}, this binding was written against {RT_API_VERSION}: rebuild the library or update the mirror")
    out = (C.c_int32 * len(structs))()
    n = lib.rtStructSizes(out, len(structs))
    if n != len(structs):
        raise ImportError(f"{path} reports {n} ABI structs, the mirror has {len(structs)}")
    for t, sz in zip(structs, out):
        if C.sizeof(t) != sz:
            raise ImportError(f"{path}: sizeof({t.__name__}) is {sz} in the library and {C.sizeof(t)} in the Python mirror - "
                              "library and mirror are of different generations; refusing to call into it")


def load_renderer():
    """librt_mi355x.so — the HIP renderer.  Raises ImportError if it is not built: there is no fallback."""
    global _renderer
    if _renderer is None:
        if not os.path.exists(RENDERER_LIB):
            raise ImportError(f"{RENDERER_LIB} is not built: run `make` (or __graft_entry__.build()); "
                              "there is no CPU fallback for the render path")
        r = C.CDLL(RENDERER_LIB)
        check_abi(r)
        r.initRenderer.argtypes = [kernel_scene, camera, C.POINTER(C.POINTER(vec3)), C.c_int, C.c_int, C.c_int]
        r.initRenderer.restype = None
        r.runRenderer.argtypes = [C.c_int, C.c_int, C.c_int]
        r.runRenderer.restype = None
        r.cleanupRenderer.argtypes = []
        r.cleanupRenderer.restype = None
        r.initRendererSpheres.argtypes = [C.c_void_p, C.c_void_p, C.c_int, camera, C.POINTER(C.POINTER(vec3)),
                                          C.c_int, C.c_int, C.c_int]
        r.initRendererSpheres.restype = None
        r.getDefaultRenderOptions.argtypes = [C.POINTER(render_options), C.c_int]
        r.getDefaultRenderOptions.restype = None
        r.setRenderOptions.argtypes = [C.POINTER(render_options)]
        r.setRenderOptions.restype = None
        r.setExternalFramebuffer.argtypes = [C.c_void_p]
        r.setExternalFramebuffer.restype = None
        r.getRenderStats.argtypes = [C.POINTER(render_stats)]
        r.getRenderStats.restype = None
        r.rtDeviceCount.argtypes = []
        r.rtDeviceCount.restype = C.c_int
        r.rtApiVersion.argtypes = []
        r.rtApiVersion.restype = C.c_int
        r.rtLastLaunches.argtypes = [C.POINTER(C.c_int32), C.c_int]
        r.rtLastLaunches.restype = C.c_int
        r.runRendererProgressive.argtypes = [C.c_int, C.c_int, C.c_int]
        r.runRendererProgressive.restype = None
        r.rtProgressiveSamples.argtypes = []
        r.rtProgressiveSamples.restype = C.c_int
        r.rtResetProgressive.argtypes = []
        r.rtResetProgressive.restype = None
        r.setCamera.argtypes = [C.POINTER(camera)]
        r.setCamera.restype = None
        r.renderGuides.argtypes = [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        r.renderGuides.restype = None
        r.rtLastGuidesMs.argtypes = []
        r.rtLastGuidesMs.restype = C.c_double
        r.rtDefaultDenoiseFlags.argtypes = []
        r.rtDefaultDenoiseFlags.restype = C.c_int
        r.denoiseFrame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
        r.denoiseFrame.restype = None
        r.rtLastDenoiseMs.argtypes = []
        r.rtLastDenoiseMs.restype = C.c_double
        r.accumulateFrame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]
        r.accumulateFrame.restype = None
        r.rtResetHistory.argtypes = []
        r.rtResetHistory.restype = None
        r.rtHistoryFrames.argtypes = []
        r.rtHistoryFrames.restype = C.c_int
        r.rtLastAccumulateMs.argtypes = []
        r.rtLastAccumulateMs.restype = C.c_double
        r.previewFrame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
        r.previewFrame.restype = None
        r.rtResetPreview.argtypes = []
        r.rtResetPreview.restype = None
        r.rtPreviewFrames.argtypes = []
        r.rtPreviewFrames.restype = C.c_int
        r.rtLastPreviewMs.argtypes = []
        r.rtLastPreviewMs.restype = C.c_double
        r.displayFrame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]
        r.displayFrame.restype = None
        r.rtLastExposure.argtypes = []
        r.rtLastExposure.restype = C.c_float
        r.rtDisplayHistogram.argtypes = [C.POINTER(C.c_uint32), C.c_int]
        r.rtDisplayHistogram.restype = C.c_int
        r.rtResetDisplay.argtypes = []
        r.rtResetDisplay.restype = None
        r.rtLastDisplayMs.argtypes = []
        r.rtLastDisplayMs.restype = C.c_double
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        r.traceRays.argtypes = [C.c_int, fp, fp, fp, fp, C.c_int, fp, ip, fp, fp, ip]
        r.traceRays.restype = None
        r.occludedRays.argtypes = [C.c_int, fp, fp, fp, fp, C.POINTER(C.c_uint8)]
        r.occludedRays.restype = None
        r.rtLastRaysMs.argtypes = []
        r.rtLastRaysMs.restype = C.c_double
        up = C.POINTER(C.c_uint32)
        r.renderPixels.argtypes = [C.c_int, ip, C.c_int, ip, ip, up, C.POINTER(vec3), up]
        r.renderPixels.restype = None
        r.rtLastPixelsMs.argtypes = []
        r.rtLastPixelsMs.restype = C.c_double
        r.radianceRays.argtypes = [C.c_int, fp, fp, up, C.c_int, ip, ip, up, C.POINTER(vec3), up]
        r.radianceRays.restype = None
        r.rtLastRadianceMs.argtypes = []
        r.rtLastRadianceMs.restype = C.c_double
        r.rtGatherWidth.argtypes = [C.c_int]
        r.rtGatherWidth.restype = C.c_int
        r.gatherRadiance.argtypes = [C.c_int, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_float, C.c_float, fp, fp, up]
        r.gatherRadiance.restype = None
        r.rtGatherDirections.argtypes = [C.c_int, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_float, fp, fp, up]
        r.rtGatherDirections.restype = None
        r.rtLastGatherMs.argtypes = []
        r.rtLastGatherMs.restype = C.c_double
        r.rasterTexels.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, fp, fp, fp]
        r.rasterTexels.restype = C.c_int
        r.bakeTexels.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_float, C.c_float, fp, fp, up, ip, ip]
        r.bakeTexels.restype = C.c_int
        r.filterTexels.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
        r.filterTexels.restype = C.c_int
        r.rtLastFilterMs.argtypes = []
        r.rtLastFilterMs.restype = C.c_double
        r.sampleTexels.argtypes = [C.c_int, ip, fp, fp, C.c_int, C.c_int, C.c_int, fp, C.c_int, fp, C.POINTER(C.c_uint8)]
        r.sampleTexels.restype = C.c_int
        r.renderLightmap.argtypes = [C.c_int, C.c_int, C.c_int, fp, C.c_int, fp, C.POINTER(vec3)]
        r.renderLightmap.restype = None
        r.rtLastSampleMs.argtypes = []
        r.rtLastSampleMs.restype = C.c_double
        r.rtLastLightmapMs.argtypes = []
        r.rtLastLightmapMs.restype = C.c_double
        r.rtLastTexelsMs.argtypes = []
        r.rtLastTexelsMs.restype = C.c_double
        r.rtLastBakeMs.argtypes = []
        r.rtLastBakeMs.restype = C.c_double
        r.refineFrame.argtypes = [C.POINTER(vec3), ip, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]
        r.refineFrame.restype = C.c_int
        r.rtResetRefine.argtypes = []
        r.rtResetRefine.restype = None
        r.rtRefineSamples.argtypes = []
        r.rtRefineSamples.restype = C.c_longlong
        r.rtRefineLastList.argtypes = [ip, C.c_int]
        r.rtRefineLastList.restype = C.c_int
        r.rtLastRefineMs.argtypes = []
        r.rtLastRefineMs.restype = C.c_double
        r.updateTriangles.argtypes = [C.c_int, C.c_int, C.c_void_p]
        r.updateTriangles.restype = None
        r.updateMaterials.argtypes = [C.c_void_p, C.c_int]
        r.updateMaterials.restype = None
        r.updateSpheres.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        r.updateSpheres.restype = None
        r.getMeshBvh.argtypes = [C.c_void_p, C.c_int, C.POINTER(bbox)]
        r.getMeshBvh.restype = C.c_int
        r.rtLastUpdateMs.argtypes = []
        r.rtLastUpdateMs.restype = C.c_double
        r.rebuildBvh.argtypes = [C.c_void_p]
        r.rebuildBvh.restype = None
        r.rtLastRebuildMs.argtypes = []
        r.rtLastRebuildMs.restype = C.c_double
        r.rtMarkPose.argtypes = []
        r.rtMarkPose.restype = None
        r.rtClearPose.argtypes = []
        r.rtClearPose.restype = None
        r.rtPoseMarked.argtypes = []
        r.rtPoseMarked.restype = C.c_int
        r.renderMotion.argtypes = [C.c_int, C.POINTER(camera), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        r.renderMotion.restype = None
        r.rtLastMotionMs.argtypes = []
        r.rtLastMotionMs.restype = C.c_double
        _renderer = r
    return _renderer


# ---------------------------------------------------------------------------------------------
# host-side helpers (scene set-up; what main.cpp / staircase_scene.h do before initRenderer)
# ---------------------------------------------------------------------------------------------

def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def make_camera(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist):
    """camera::camera, /root/reference/helper_structs.h:194-207."""
    cam = camera()
    load_host().rtMakeCamera(_f3(lookfrom), _f3(lookat), _f3(vup), vfov, aspect, aperture, focus_dist, C.byref(cam))
    return cam


def scene_three_spheres(nx, ny):
    """C1 of SURVEY.md §8d. Returns (spheres, materials, camera)."""
    sp = np.zeros(3, sphere_dtype)
    mt = np.zeros(3, material_dtype)
    cam = camera()
    n = load_host().rtSceneThreeSpheres(sp.ctypes.data, mt.ctypes.data, 3, nx, ny, C.byref(cam))
    assert n == 3
    return sp, mt, cam


def scene_random_spheres(nx, ny, seed=0):
    """C2/C3/C5 of SURVEY.md §8d: 488 spheres. Returns (spheres, materials, camera)."""
    cap = 488
    sp = np.zeros(cap, sphere_dtype)
    mt = np.zeros(cap, material_dtype)
    cam = camera()
    n = load_host().rtSceneRandomSpheres(seed, sp.ctypes.data, mt.ctypes.data, cap, nx, ny, C.byref(cam))
    assert n == cap, n
    return sp, mt, cam


def staircase_camera(nx, ny):
    cam = camera()
    load_host().rtStaircaseCamera(nx, ny, C.byref(cam))
    return cam


class HostMesh:
    """Owns a BVH'd mesh built/loaded by librt_host.so; `.view` is an rt_mesh for kernel_scene.m."""

    def __init__(self, handle):
        if not handle:
            raise ValueError("mesh build/load failed")
        self._h = C.c_void_p(handle)
        self.view = mesh()
        self.nppl = load_host().rtMeshView(self._h, C.byref(self.view))

    @classmethod
    def build(cls, tris, nppl=5, extra_levels=None):
        """rtBuildBvh; extra_levels: rtBuildBvhLevels (None = the builder's default)."""
        tris = np.ascontiguousarray(tris, dtype=triangle_dtype)
        if extra_levels is None:
            return cls(load_host().rtBuildBvh(tris.ctypes.data, len(tris), nppl))
        return cls(load_host().rtBuildBvhLevels(tris.ctypes.data, len(tris), nppl, extra_levels))

    @classmethod
    def load(cls, path):
        return cls(load_host().rtLoadBvhFile(os.fsencode(path)))

    def save(self, path):
        return load_host().rtSaveBvhFile(self._h, os.fsencode(path))

    @property
    def tris(self):
        return np.ctypeslib.as_array(C.cast(self.view.tris, C.POINTER(C.c_ubyte)), (self.view.numTris * 64,)).view(triangle_dtype)

    @property
    def bvh(self):
        return np.ctypeslib.as_array(C.cast(self.view.bvh, C.POINTER(C.c_ubyte)), (self.view.numBvhNodes * 24,)).view(bvh_node_dtype)

    def refit(self):
        """rtRefitBvh: every node and the bounds from `.tris` as they are now (a writable view: edit it in place, then refit), in the order include/rt_api.h
        defines - what updateTriangles computes on the device, and the scene the CPU oracle renders.  `.bvh` and `.view` follow."""
        if load_host().rtRefitBvh(self._h) != 0:
            raise ValueError("rtRefitBvh refused the mesh")
        self.nppl = load_host().rtMeshView(self._h, C.byref(self.view))

    def rebuild(self):
        """rtRebuildBvh: the visible triangles assigned to the leaf slots anew by the builder, the tree's shape kept, then the refit - the rebuild include/rt_api.h
        defines and rebuildBvh computes on the device.  Returns old_slot (int32, one entry per slot: the slot its triangle came from, -1 for a sentinel).
        `.tris`, `.bvh` and `.view` follow."""
        old_slot = np.zeros(self.view.numTris, np.int32)
        if load_host().rtRebuildBvh(self._h, old_slot.ctypes.data) != 0:
            raise ValueError("rtRebuildBvh refused the mesh")
        self.nppl = load_host().rtMeshView(self._h, C.byref(self.view))
        return old_slot

    def close(self):
        if self._h:
            load_host().rtFreeMesh(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def scene_staircase_procedural(detail=1):
    """Procedural stand-in for the absent staircase asset. Returns (triangles, materials[20])."""
    h = load_host()
    mats = np.zeros(20, material_dtype)
    need = h.rtSceneStaircaseProcedural(detail, None, 0, mats.ctypes.data)
    n = -need if need < 0 else need
    tris = np.zeros(n, triangle_dtype)
    got = h.rtSceneStaircaseProcedural(detail, tris.ctypes.data, n, mats.ctypes.data)
    assert got == n, (got, n)
    return tris, mats


def make_kernel_scene(host_mesh, materials, textures=(), floor=None):
    """setup_kernel_scene, /root/reference/staircase_scene.h:166-184. Returns (kernel_scene, keepalive).
    floor = (norm xyz, point xyz) of kernel_scene.floor (read by the renderer only with rt_render_options.floor = 1)."""
    materials = np.ascontiguousarray(materials, dtype=material_dtype)
    ks = kernel_scene()
    ks.m = C.pointer(host_mesh.view)
    ks.materials = C.cast(materials.ctypes.data, C.POINTER(material))
    ks.numMaterials = len(materials)
    tex_arr = (stexture * max(1, len(textures)))()
    keep = [materials, tex_arr, host_mesh]
    for k, t in enumerate(textures):
        t = np.ascontiguousarray(t, dtype=np.float32)       # (height, width, 3)
        keep.append(t)
        tex_arr[k].data = t.ctypes.data_as(C.POINTER(C.c_float))
        tex_arr[k].height, tex_arr[k].width = t.shape[0], t.shape[1]
    ks.textures = tex_arr if textures else None
    ks.numTextures = len(textures)
    ks.numPrimitivesPerLeaf = host_mesh.nppl
    if floor is not None:
        for a in range(3):
            ks.floor.norm.e[a] = float(floor[a])
            ks.floor.point.e[a] = float(floor[3 + a])
    return ks, keep


# ---------------------------------------------------------------------------------------------
# renderer API (same names as the C symbols)
# ---------------------------------------------------------------------------------------------

_state = {"fb": None, "nx": 0, "ny": 0, "keep": None, "spheres": False}


def _fb_view(fbp, nx, ny):
    arr = np.ctypeslib.as_array(C.cast(fbp, C.POINTER(C.c_float)), (ny, nx, 3))
    return arr


def initRenderer(ksc, cam, nx, ny, maxDepth, keepalive=None):
    """extern "C" initRenderer (/root/reference/kernels.h:6). Returns the framebuffer as a (ny, nx, 3) float32 view."""
    r = load_renderer()
    fbp = C.POINTER(vec3)()
    r.initRenderer(ksc, cam, C.byref(fbp), nx, ny, maxDepth)
    _state.update(fb=_fb_view(fbp, nx, ny), nx=nx, ny=ny, keep=keepalive, spheres=False, num_tris=int(ksc.m.contents.numTris))
    return _state["fb"]


def initRendererSpheres(spheres, materials, cam, nx, ny, maxDepth):
    """Additive: sphere-scene initialiser (include/rt_api.h). Returns the framebuffer view."""
    r = load_renderer()
    spheres = np.ascontiguousarray(spheres, dtype=sphere_dtype)
    materials = np.ascontiguousarray(materials, dtype=material_dtype)
    if len(spheres) != len(materials):
        raise ValueError("one material per sphere")
    fbp = C.POINTER(vec3)()
    r.initRendererSpheres(spheres.ctypes.data, materials.ctypes.data, len(spheres), cam, C.byref(fbp), nx, ny, maxDepth)
    _state.update(fb=_fb_view(fbp, nx, ny), nx=nx, ny=ny, keep=None, spheres=True)
    return _state["fb"]


def runRenderer(ns, tx=8, ty=8):
    """extern "C" runRenderer (/root/reference/kernels.h:7); blocking."""
    load_renderer().runRenderer(ns, tx, ty)


def runRendererProgressive(ns, tx=8, ty=8):
    """Adds ns samples per pixel to the progressive frame; the framebuffer holds the mean of all samples since the last reset (include/rt_api.h)."""
    load_renderer().runRendererProgressive(ns, tx, ty)


def progressive_samples():
    """Samples per pixel accumulated by runRendererProgressive since init / the last reset."""
    return load_renderer().rtProgressiveSamples()


def resetProgressive():
    """The next runRendererProgressive starts again at sample 0."""
    load_renderer().rtResetProgressive()


def setCamera(cam):
    """Replaces the camera for the following frames (no re-upload of the scene); resets the progressive frame."""
    load_renderer().setCamera(C.byref(cam))


# renderGuides (include/rt_api.h): the planes of the mask, the primitive ids of a floor hit and of a miss
RT_GUIDE_ALBEDO, RT_GUIDE_NORMAL, RT_GUIDE_DEPTH, RT_GUIDE_PRIM, RT_GUIDE_NODES = 1, 2, 4, 8, 16
RT_GUIDE_PRIM_NONE, RT_GUIDE_PRIM_FLOOR = -1, -2
GUIDE_PLANES = (("albedo", RT_GUIDE_ALBEDO, np.float32, 3), ("normal", RT_GUIDE_NORMAL, np.float32, 3), ("depth", RT_GUIDE_DEPTH, np.float32, 1),
                ("prim", RT_GUIDE_PRIM, np.int32, 1), ("nodes", RT_GUIDE_NODES, np.int32, 1))


def renderGuides(mask=RT_GUIDE_ALBEDO | RT_GUIDE_NORMAL | RT_GUIDE_DEPTH | RT_GUIDE_PRIM, out=None):
    """First-hit guide planes of the centre rays (include/rt_api.h).  Returns a dict with the planes of `mask`: albedo, normal (ny, nx, 3) float32;
    depth (ny, nx) float32; prim, nodes (ny, nx) int32.  `out`: a dict of caller-owned C-contiguous arrays of those shapes and types (e.g. views of shared
    memory) to fill instead of new ones; only the rows this process owns are written.  Blocking; RT_GUIDE_NODES is defined for mesh scenes only."""
    nx, ny = _state["nx"], _state["ny"]
    res, ptrs = {}, []
    for name, bit, dtype, comps in GUIDE_PLANES:
        if not (mask & bit):
            ptrs.append(None)
            continue
        shape = (ny, nx, 3) if comps == 3 else (ny, nx)
        if out is not None and name in out:
            a = out[name]
            if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"] and a.shape == shape):
                raise ValueError(f"renderGuides: out[{name!r}] must be a writable C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        else:
            a = np.zeros(shape, dtype)
        res[name] = a
        ptrs.append(a.ctypes.data_as(C.POINTER(C.c_float if dtype == np.float32 else C.c_int32)))
    load_renderer().renderGuides(mask, *ptrs)
    return res


def last_guides_ms():
    """HIP-event time of the guide kernel(s) of the last renderGuides (the largest over the in-process devices), in milliseconds."""
    return load_renderer().rtLastGuidesMs()


# traceRays / occludedRays (include/rt_api.h): batched queries with the caller's own rays
RT_RAY_T, RT_RAY_PRIM, RT_RAY_NORMAL, RT_RAY_UV, RT_RAY_NODES = 1, 2, 4, 8, 16
RT_RAY_CHUNK = 1 << 22
RAY_PLANES = (("t", RT_RAY_T, np.float32, 1), ("prim", RT_RAY_PRIM, np.int32, 1), ("normal", RT_RAY_NORMAL, np.float32, 3), ("uv", RT_RAY_UV, np.float32, 2),
              ("nodes", RT_RAY_NODES, np.int32, 1))


def _ray_inputs(fn, org, dir, t_min, t_max):
    """Contiguous float32 copies (or the arrays themselves) of the rays and their ctypes pointers; a wrong shape is a ValueError."""
    org = np.ascontiguousarray(org, dtype=np.float32)
    dir = np.ascontiguousarray(dir, dtype=np.float32)
    if org.ndim != 2 or org.shape[1] != 3 or dir.shape != org.shape:
        raise ValueError(f"{fn}: org and dir must both have shape (n, 3), got {org.shape} and {dir.shape}")
    n = org.shape[0]
    keep, ptrs = [org, dir], []
    for name, a in (("t_min", t_min), ("t_max", t_max)):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != (n,):
                raise ValueError(f"{fn}: {name} must have shape ({n},), got {a.shape}")
        keep.append(a)
    fp = C.POINTER(C.c_float)
    ptrs = [None if a is None else a.ctypes.data_as(fp) for a in keep]
    return n, keep, ptrs


def _ray_out(fn, out, name, shape, dtype):
    if out is not None and not isinstance(out, dict):
        out = {name: out}
    if out is not None and name in out:
        a = out[name]
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"] and a.shape == shape):
            raise ValueError(f"{fn}: out[{name!r}] must be a writable C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        return a
    return np.zeros(shape, dtype)


def trace_rays(org, dir, t_min=None, t_max=None, mask=None, out=None):
    """First hits of the caller's rays (traceRays, include/rt_api.h).  org, dir: (n, 3), converted to contiguous float32; t_min, t_max: (n,) or None (the
    options' t_min, FLT_MAX).  Returns a dict with the planes of `mask` (default: every plane the scene kind has): t (n,) float32, prim (n,) int32,
    normal (n, 3), uv (n, 2) float32, nodes (n,) int32 (mesh scenes).  `out`: a dict of caller-owned C-contiguous arrays of those shapes and types to fill
    instead of new ones; arrays of planes that are not in the mask are left alone.  Blocking."""
    n, keep, ptrs = _ray_inputs("trace_rays", org, dir, t_min, t_max)
    if mask is None:
        mask = RT_RAY_T | RT_RAY_PRIM | RT_RAY_NORMAL | RT_RAY_UV | (0 if _state.get("spheres") else RT_RAY_NODES)
    res, outs = {}, []
    for name, bit, dtype, comps in RAY_PLANES:
        if not (mask & bit):
            outs.append(None)
            continue
        a = _ray_out("trace_rays", out, name, (n,) if comps == 1 else (n, comps), dtype)
        res[name] = a
        outs.append(a.ctypes.data_as(C.POINTER(C.c_float if dtype == np.float32 else C.c_int32)))
    load_renderer().traceRays(n, *ptrs, mask, *outs)
    return res


def occluded_rays(org, dir, t_min=None, t_max=None, out=None):
    """Any-hit query of the caller's rays (occludedRays, include/rt_api.h): (n,) uint8, 1 = something lies between the ray's bounds.  `out`: a caller-owned
    C-contiguous uint8 array of shape (n,) to fill instead of a new one.  Blocking."""
    n, keep, ptrs = _ray_inputs("occluded_rays", org, dir, t_min, t_max)
    a = _ray_out("occluded_rays", out, "occluded", (n,), np.uint8)
    load_renderer().occludedRays(n, *ptrs, a.ctypes.data_as(C.POINTER(C.c_uint8)))
    return a


def last_rays_ms():
    """HIP-event time of the ray kernels of the last trace_rays / occluded_rays (not the copies), summed over its chunks, in milliseconds."""
    return load_renderer().rtLastRaysMs()


# renderPixels (include/rt_api.h): path-trace a list of pixels, resumable
RT_PIXEL_CHUNK = 1 << 22
RT_PROGRESSIVE_MAX_SAMPLES = 65536


def render_pixels(ij, ns, first=None, state=None, rays=False):
    """Path-traces the pixels ij = (n, 2) int (column i, row j; row 0 = bottom) (renderPixels, include/rt_api.h).  ns: an int - samples for every pixel - or
    an (n,) int array; first: None (every pixel starts its stream) or an (n,) int array of the first sample of each pixel, which needs `state` = the (n, 4)
    uint32 array an earlier call returned for the same pixels after that many samples.  Returns (out, state, rays): out (n, 3) float32 = sum / (first + ns);
    state (n, 4) uint32 after the last sample (a new array: the caller's is not written); rays (n,) uint32 closest-hit queries of these samples, or None
    unless rays=True.  Blocking."""
    ij = np.ascontiguousarray(ij, dtype=np.int32)
    if ij.ndim != 2 or ij.shape[1] != 2:
        raise ValueError(f"render_pixels: ij must have shape (n, 2), got {ij.shape}")
    n = ij.shape[0]
    ip, up = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)

    def per_pixel(name, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        if a.shape != (n,):
            raise ValueError(f"render_pixels: {name} must be an int or have shape ({n},), got {a.shape}")
        return a

    ns_all, ns_arr = 0, None
    if isinstance(ns, (int, np.integer)) and not isinstance(ns, bool):
        ns_all = int(ns)
    else:
        ns_arr = per_pixel("ns", ns)
    first_arr = None if first is None else per_pixel("first", first)
    if state is None:
        if first_arr is not None:
            raise ValueError("render_pixels: first needs the state the pixels resume from")
        st = np.zeros((n, 4), np.uint32)
    else:
        st = np.array(state, dtype=np.uint32, order="C")            # (a copy: renderPixels updates the states in place)
        if st.shape != (n, 4):
            raise ValueError(f"render_pixels: state must have shape ({n}, 4), got {st.shape}")
    out = np.zeros((n, 3), np.float32)
    nrays = np.zeros(n, np.uint32) if rays else None
    load_renderer().renderPixels(n, ij.ctypes.data_as(ip), ns_all, None if ns_arr is None else ns_arr.ctypes.data_as(ip),
                                 None if first_arr is None else first_arr.ctypes.data_as(ip), st.ctypes.data_as(up),
                                 out.ctypes.data_as(C.POINTER(vec3)), None if nrays is None else nrays.ctypes.data_as(up))
    return out, st, nrays


def render_region(x0, y0, x1, y1, ns):
    """The pixel rectangle [x0, x1) x [y0, y1) (columns, rows from the bottom) at ns samples per pixel, path-traced by render_pixels: a (y1 - y0, x1 - x0, 3)
    float32 array, row 0 = row y0 - in PARITY mode the bits runRenderer(ns) stores there."""
    if not (x0 <= x1 and y0 <= y1):
        raise ValueError("render_region: needs x0 <= x1 and y0 <= y1")
    jj, ii = np.mgrid[y0:y1, x0:x1]
    out, _, _ = render_pixels(np.stack([ii.ravel(), jj.ravel()], axis=1), ns)
    return out.reshape(y1 - y0, x1 - x0, 3)


def last_pixels_ms():
    """HIP-event time of the pixel kernels of the last render_pixels / render_region (not the copies), summed over its chunks, in milliseconds."""
    return load_renderer().rtLastPixelsMs()


# radianceRays (include/rt_api.h): path-trace the caller's own rays, resumable
def radiance_rays(org, dir, ns, ids=None, first=None, state=None, rays=False):
    """Path-traces the rays (org, dir), both (n, 3) float (dir raw, non-zero: normalised once on the device) (radianceRays, include/rt_api.h).  ns: an int -
    samples for every ray - or an (n,) int array; ids: None (ray k is seeded by k) or an (n,) uint32 array of seed ids; first: None (every ray starts its
    stream) or an (n,) int array of the first sample of each ray, which needs `state` = the (n, 4) uint32 array an earlier call returned for the same rays
    after that many samples.  Returns (out, state, rays): out (n, 3) float32 = sum / (first + ns); state (n, 4) uint32 after the last sample (a new array:
    the caller's is not written); rays (n,) uint32 closest-hit queries of these samples, or None unless rays=True.  Blocking."""
    org = np.ascontiguousarray(org, dtype=np.float32)
    d = np.ascontiguousarray(dir, dtype=np.float32)
    if org.ndim != 2 or org.shape[1] != 3 or d.shape != org.shape:
        raise ValueError(f"radiance_rays: org and dir must both have shape (n, 3), got {org.shape} and {d.shape}")
    n = org.shape[0]
    fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)

    def per_ray(name, a, dtype=np.int32):
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape != (n,):
            raise ValueError(f"radiance_rays: {name} must have shape ({n},), got {a.shape}")
        return a

    ns_all, ns_arr = 0, None
    if isinstance(ns, (int, np.integer)) and not isinstance(ns, bool):
        ns_all = int(ns)
    else:
        ns_arr = per_ray("ns", ns)
    ids_arr = None if ids is None else per_ray("ids", ids, np.uint32)
    first_arr = None if first is None else per_ray("first", first)
    if state is None:
        if first_arr is not None:
            raise ValueError("radiance_rays: first needs the state the rays resume from")
        st = np.zeros((n, 4), np.uint32)
    else:
        st = np.array(state, dtype=np.uint32, order="C")            # (a copy: radianceRays updates the states in place)
        if st.shape != (n, 4):
            raise ValueError(f"radiance_rays: state must have shape ({n}, 4), got {st.shape}")
    out = np.zeros((n, 3), np.float32)
    nrays = np.zeros(n, np.uint32) if rays else None
    load_renderer().radianceRays(n, org.ctypes.data_as(fp), d.ctypes.data_as(fp), None if ids_arr is None else ids_arr.ctypes.data_as(up), ns_all,
                                 None if ns_arr is None else ns_arr.ctypes.data_as(ip), None if first_arr is None else first_arr.ctypes.data_as(ip),
                                 st.ctypes.data_as(up), out.ctypes.data_as(C.POINTER(vec3)), None if nrays is None else nrays.ctypes.data_as(up))
    return out, st, nrays


def last_radiance_ms():
    """HIP-event time of the radiance kernels of the last radiance_rays (not the copies), summed over its chunks, in milliseconds."""
    return load_renderer().rtLastRadianceMs()


# gatherRadiance (include/rt_api.h): irradiance, SH9 and visibility at points, on the device
RT_GATHER_IRRADIANCE, RT_GATHER_SH9, RT_GATHER_VISIBILITY = 0, 1, 2
RT_GATHER_MAX_DIRS = 65536
_GATHER_WIDTH = {RT_GATHER_IRRADIANCE: 3, RT_GATHER_SH9: 27, RT_GATHER_VISIBILITY: 1}


def gather_width(mode):
    """Floats per point in acc / out of gather_radiance (rtGatherWidth): 3, 27, 1."""
    return load_renderer().rtGatherWidth(mode)


def _gather_points(fn, pos, nrm, mode):
    """Contiguous float32 copies (or the arrays themselves) of the points and normals; a wrong shape or an unknown mode is a ValueError."""
    if mode not in _GATHER_WIDTH:
        raise ValueError(f"{fn}: unknown mode {mode!r}")
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"{fn}: pos must have shape (n, 3), got {pos.shape}")
    if nrm is None:
        if mode != RT_GATHER_SH9:
            raise ValueError(f"{fn}: nrm may be None only in RT_GATHER_SH9")
    else:
        nrm = np.ascontiguousarray(nrm, dtype=np.float32)
        if nrm.shape != pos.shape:
            raise ValueError(f"{fn}: nrm must have shape {pos.shape}, got {nrm.shape}")
    return pos, nrm


def gather_radiance(pos, nrm, mode, dirs, ns=1, first=0, dirs_total=None, acc=None, base_id=0, bias=0.0, max_dist=0.0, rays=False):
    """Gathers at the points pos (n, 3) with normals nrm (n, 3; None in RT_GATHER_SH9): directions first .. first+dirs-1 of dirs_total (default first + dirs)
    per point, drawn, traced at ns samples and reduced on the device (gatherRadiance, include/rt_api.h).  acc: None, or the (n, W) float32 sums an earlier
    call returned for the same points after `first` directions (needed for first > 0).  Returns (out (n, W) float32, acc (n, W) float32 - a new array: the
    caller's is not written -, rays (n,) uint32 or None unless rays=True), W = gather_width(mode).  Blocking."""
    pos, nrm = _gather_points("gather_radiance", pos, nrm, mode)
    n, W = pos.shape[0], _GATHER_WIDTH[mode]
    if dirs_total is None:
        dirs_total = first + dirs
    if acc is None:
        if first > 0:
            raise ValueError("gather_radiance: first > 0 needs the acc the points resume from")
        a = np.zeros((n, W), np.float32)
    else:
        a = np.array(acc, dtype=np.float32, order="C")              # (a copy: gatherRadiance updates the sums in place)
        if a.shape != (n, W):
            raise ValueError(f"gather_radiance: acc must have shape ({n}, {W}), got {a.shape}")
    out = np.zeros((n, W), np.float32)
    nrays = np.zeros(n, np.uint32) if rays else None
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    load_renderer().gatherRadiance(n, pos.ctypes.data_as(fp), None if nrm is None else nrm.ctypes.data_as(fp), mode, first, dirs, dirs_total, ns, base_id,
                                   bias, max_dist, a.ctypes.data_as(fp), out.ctypes.data_as(fp), None if nrays is None else nrays.ctypes.data_as(up))
    return out, a, nrays


def _gather_directions(fn, call, pos, nrm, mode, dirs, first, dirs_total, base_id, bias):
    pos, nrm = _gather_points(fn, pos, nrm, mode)
    n = pos.shape[0]
    if dirs_total is None:
        dirs_total = first + dirs
    if dirs < 1 or first < 0 or first + dirs > dirs_total or dirs_total > RT_GATHER_MAX_DIRS:
        raise ValueError(f"{fn}: needs 1 <= dirs, 0 <= first and first + dirs <= dirs_total <= RT_GATHER_MAX_DIRS")
    org, d, ids = np.zeros((n * dirs, 3), np.float32), np.zeros((n * dirs, 3), np.float32), np.zeros(n * dirs, np.uint32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    call(n, pos.ctypes.data_as(fp), None if nrm is None else nrm.ctypes.data_as(fp), mode, first, dirs, dirs_total, base_id, bias,
         org.ctypes.data_as(fp), d.ctypes.data_as(fp), ids.ctypes.data_as(up))
    return org, d, ids


def gather_directions(pos, nrm, mode, dirs, first=0, dirs_total=None, base_id=0, bias=0.0):
    """The rays gather_radiance traces, from the generator kernel alone (rtGatherDirections): (org (n * dirs, 3), dir (n * dirs, 3) raw, ids (n * dirs,) uint32),
    entry k * dirs + (m - first).  Blocking."""
    return _gather_directions("gather_directions", load_renderer().rtGatherDirections, pos, nrm, mode, dirs, first, dirs_total, base_id, bias)


def gather_directions_host(pos, nrm, mode, dirs, first=0, dirs_total=None, base_id=0, bias=0.0):
    """gather_directions on the CPU (librt_host.so, rtGatherDirectionsHost; no GPU, no renderer state): the same bits."""
    if not np.isfinite(bias):
        raise ValueError("gather_directions_host: bias must be finite")
    return _gather_directions("gather_directions_host", load_host().rtGatherDirectionsHost, pos, nrm, mode, dirs, first, dirs_total, base_id, bias)


def last_gather_ms():
    """HIP-event time of generator + trace + reduce of the last gather_radiance (not the copies), summed over its chunks, in milliseconds."""
    return load_renderer().rtLastGatherMs()


# rasterTexels / bakeTexels (include/rt_api.h): the mesh's UV atlas rasterised on the device, a gather per covered texel, texel planes back
RT_TEXEL_MAX_SIZE, RT_TEXEL_MAX_DILATE = 8192, 16
TEXEL_PLANES = ("prim", "src", "bary", "pos", "nrm")


def _texel_planes(fn, W, H, dilate, want):
    """The planes `want` names as zeroed arrays of an H x W atlas (None for the others); a size or a name out of range is a ValueError."""
    if not (1 <= W <= RT_TEXEL_MAX_SIZE and 1 <= H <= RT_TEXEL_MAX_SIZE and 0 <= dilate <= RT_TEXEL_MAX_DILATE):
        raise ValueError(f"{fn}: needs 1 <= W, H <= RT_TEXEL_MAX_SIZE and 0 <= dilate <= RT_TEXEL_MAX_DILATE")
    if not want or set(want) - set(TEXEL_PLANES):
        raise ValueError(f"{fn}: want must name at least one of {TEXEL_PLANES}")
    shape = {"prim": (H, W), "src": (H, W), "bary": (H, W, 2), "pos": (H, W, 3), "nrm": (H, W, 3)}
    return {k: (np.zeros(shape[k], np.int32 if k in ("prim", "src") else np.float32) if k in want else None) for k in TEXEL_PLANES}


def _plane_ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def raster_texels(W, H, dilate=0, want=TEXEL_PLANES):
    """Rasterises the live triangles' UV atlas at W x H on the device (rasterTexels): returns (owned, planes) - the number of owned texels and a dict of the
    planes `want` names: prim (H, W) int32, src (H, W) int32 after `dilate` iterations, bary (H, W, 2), pos (H, W, 3), nrm (H, W, 3) float32.  Blocking."""
    pl = _texel_planes("raster_texels", W, H, dilate, want)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    owned = load_renderer().rasterTexels(W, H, dilate, _plane_ptr(pl["prim"], ip), _plane_ptr(pl["src"], ip), _plane_ptr(pl["bary"], fp),
                                         _plane_ptr(pl["pos"], fp), _plane_ptr(pl["nrm"], fp))
    return owned, {k: v for k, v in pl.items() if v is not None}


def raster_texels_host(tris, W, H, dilate=0, want=TEXEL_PLANES):
    """raster_texels on the CPU (librt_host.so, rtRasterTexelsHost; no GPU, no renderer state) over `tris`, a 1-D array of triangle_dtype in slot order:
    the same bits."""
    tris = _records("raster_texels_host", "triangle", tris, triangle_dtype)
    pl = _texel_planes("raster_texels_host", W, H, dilate, want)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    owned = load_host().rtRasterTexelsHost(tris.ctypes.data if len(tris) else None, len(tris), W, H, dilate, _plane_ptr(pl["prim"], ip),
                                           _plane_ptr(pl["src"], ip), _plane_ptr(pl["bary"], fp), _plane_ptr(pl["pos"], fp), _plane_ptr(pl["nrm"], fp))
    return owned, {k: v for k, v in pl.items() if v is not None}


def atlas_grid(tris, margin=0.05):
    """Overwrites texCoords of `tris` (a writable 1-D array of triangle_dtype) with the trivial non-overlapping atlas of rtAtlasGrid (include/rt_host.h): two
    triangles per square cell.  Returns the cells per side."""
    tris = _records("atlas_grid", "triangle", tris, triangle_dtype)
    if not tris.flags["WRITEABLE"] or len(tris) < 1 or not (0.0 <= margin < 0.25):
        raise ValueError("atlas_grid: needs a writable, non-empty array and 0 <= margin < 0.25")
    return load_host().rtAtlasGrid(tris.ctypes.data, len(tris), margin)


def bake_texels(W, H, mode, dirs, ns=1, dilate=0, first=0, dirs_total=None, acc=None, base_id=0, bias=0.0, max_dist=0.0, rays=False, want=("prim", "src")):
    """Rasterises the atlas at W x H and gathers at every owned texel (bakeTexels, include/rt_api.h): directions first .. first+dirs-1 of dirs_total (default
    first + dirs), as gather_radiance over the points (pos(t), nrm(t)) with point index t.  acc: None, or the (H, W, Wd) float32 sums an earlier call returned
    (needed for first > 0).  Returns (owned, planes): planes["out"] (H, W, Wd) float32 - dilated through src -, planes["acc"] (a new array), planes["rays"]
    (H, W) uint32 with rays=True, and the prim / src planes `want` names; Wd = gather_width(mode).  Blocking."""
    if mode not in _GATHER_WIDTH:
        raise ValueError(f"bake_texels: unknown mode {mode!r}")
    if set(want) - {"prim", "src"}:
        raise ValueError("bake_texels: want names prim and src only")
    pl = _texel_planes("bake_texels", W, H, dilate, tuple(want) or ("prim",))
    Wd = _GATHER_WIDTH[mode]
    if dirs_total is None:
        dirs_total = first + dirs
    if acc is None:
        if first > 0:
            raise ValueError("bake_texels: first > 0 needs the acc the texels resume from")
        a = np.zeros((H, W, Wd), np.float32)
    else:
        a = np.array(acc, dtype=np.float32, order="C")              # (a copy: bakeTexels updates the sums in place)
        if a.shape != (H, W, Wd):
            raise ValueError(f"bake_texels: acc must have shape ({H}, {W}, {Wd}), got {a.shape}")
    out = np.zeros((H, W, Wd), np.float32)
    nrays = np.zeros((H, W), np.uint32) if rays else None
    ip, fp, up = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    owned = load_renderer().bakeTexels(W, H, dilate, mode, first, dirs, dirs_total, ns, base_id, bias, max_dist, a.ctypes.data_as(fp), out.ctypes.data_as(fp),
                                       _plane_ptr(nrays, up), _plane_ptr(pl["prim"] if "prim" in want else None, ip),
                                       _plane_ptr(pl["src"] if "src" in want else None, ip))
    planes = {"out": out, "acc": a}
    if rays:
        planes["rays"] = nrays
    planes.update({k: pl[k] for k in want})
    return owned, planes


def last_texels_ms():
    """HIP-event time of the raster, resolve, dilation and compaction kernels of the last raster_texels / bake_texels, in milliseconds."""
    return load_renderer().rtLastTexelsMs()


def last_bake_ms():
    """HIP-event time of generator + trace + reduce + scatter of the last bake_texels (not the copies), summed over its chunks, in milliseconds."""
    return load_renderer().rtLastBakeMs()


# filterTexels (include/rt_api.h, "filtering texels"): the edge-aware, chart-aware denoise of baked texel planes; the defaults are the header's RT_FILTER_*
RT_FILTER_ITERATIONS, RT_FILTER_SQUARINGS, RT_FILTER_SIGMA_D, RT_FILTER_SIGMA_Z, RT_FILTER_SIGMA_C = 3, 5, 2.0, 2.0, 0.5


def _filter_planes(fn, W, H, dilate, mode, plane, out, needs_plane):
    """(in, out) of a filter call: `plane` as a C-contiguous float32 (H, W, Wd) array (None stays None where the call allows it), `out` the caller's array
    or a new one; a size, mode or shape out of range is a ValueError."""
    if mode not in _GATHER_WIDTH:
        raise ValueError(f"{fn}: unknown mode {mode!r}")
    if not (1 <= W <= RT_TEXEL_MAX_SIZE and 1 <= H <= RT_TEXEL_MAX_SIZE and 0 <= dilate <= RT_TEXEL_MAX_DILATE):
        raise ValueError(f"{fn}: needs 1 <= W, H <= RT_TEXEL_MAX_SIZE and 0 <= dilate <= RT_TEXEL_MAX_DILATE")
    shape = (H, W, _GATHER_WIDTH[mode])
    if plane is None:
        if needs_plane:
            raise ValueError(f"{fn}: needs a plane")
    else:
        plane = np.ascontiguousarray(plane, dtype=np.float32)
        if plane.shape != shape:
            raise ValueError(f"{fn}: the plane must have shape {shape}, got {plane.shape}")
    if out is None:
        out = np.zeros(shape, np.float32)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == shape and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]):
        raise ValueError(f"{fn}: out must be a writable C-contiguous float32 array of shape {shape}")
    return plane, out


def filter_texels(W, H, mode, plane=None, dilate=0, iterations=RT_FILTER_ITERATIONS, normal_squarings=RT_FILTER_SQUARINGS, sigma_d=RT_FILTER_SIGMA_D,
                  sigma_z=RT_FILTER_SIGMA_Z, sigma_c=RT_FILTER_SIGMA_C, out=None):
    """Filters a texel plane of the live atlas at W x H on the device (filterTexels, include/rt_api.h): `plane` is an (H, W, Wd) float32 array, Wd =
    gather_width(mode) - bake_texels' planes["out"] -, or None: the out plane of the last bake_texels, where it lies on the device.  `out`: None (a new
    array) or the array to write, which may be `plane` itself.  Returns (owned, out).  Blocking."""
    plane, out = _filter_planes("filter_texels", W, H, dilate, mode, plane, out, False)
    fp = C.POINTER(C.c_float)
    owned = load_renderer().filterTexels(W, H, dilate, mode, _plane_ptr(plane, fp), out.ctypes.data_as(fp), iterations, normal_squarings, sigma_d, sigma_z,
                                         sigma_c)
    return owned, out


def filter_texels_host(tris, W, H, mode, plane, dilate=0, iterations=RT_FILTER_ITERATIONS, normal_squarings=RT_FILTER_SQUARINGS, sigma_d=RT_FILTER_SIGMA_D,
                       sigma_z=RT_FILTER_SIGMA_Z, sigma_c=RT_FILTER_SIGMA_C, out=None):
    """filter_texels on the CPU (librt_host.so, rtFilterTexelsHost; no GPU, no renderer state) over `tris`, a 1-D array of triangle_dtype in slot order: the
    same bits.  Returns (owned, out); what the device call would refuse is a ValueError."""
    tris = _records("filter_texels_host", "triangle", tris, triangle_dtype)
    plane, out = _filter_planes("filter_texels_host", W, H, dilate, mode, plane, out, True)
    fp = C.POINTER(C.c_float)
    owned = load_host().rtFilterTexelsHost(tris.ctypes.data if len(tris) else None, len(tris), W, H, dilate, mode, plane.ctypes.data_as(fp),
                                           out.ctypes.data_as(fp), iterations, normal_squarings, sigma_d, sigma_z, sigma_c)
    if owned < 0:
        raise ValueError("filter_texels_host: iterations, normal_squarings or a sigma is out of range")
    return owned, out


def last_filter_ms():
    """HIP-event time of the raster, prologue, iteration and scatter kernels of the last filter_texels (not the copies), in milliseconds."""
    return load_renderer().rtLastFilterMs()


# sampleTexels / renderLightmap (include/rt_api.h, "sampling texels"): texel planes looked up at hits, and the frame lit by them
RT_SAMPLE_BILINEAR, RT_LIGHTMAP_ALBEDO, RT_TEXELS_FROM_BAKE, RT_TEXELS_FROM_FILTER = 1, 2, 4, 8


def _sample_hits(fn, prim, uv, normal, mode):
    """The hits as C-contiguous arrays: prim (n,) int32, uv (n, 2) float32, normal (n, 3) float32 or None (RT_GATHER_SH9 needs it); a wrong shape is a
    ValueError."""
    if mode not in _GATHER_WIDTH:
        raise ValueError(f"{fn}: unknown mode {mode!r}")
    prim = np.ascontiguousarray(prim, dtype=np.int32)
    uv = np.ascontiguousarray(uv, dtype=np.float32)
    n = len(prim)
    if prim.ndim != 1 or uv.shape != (n, 2):
        raise ValueError(f"{fn}: prim must have shape (n,) and uv (n, 2), got {prim.shape} and {uv.shape}")
    if normal is not None:
        normal = np.ascontiguousarray(normal, dtype=np.float32)
        if normal.shape != (n, 3):
            raise ValueError(f"{fn}: normal must have shape ({n}, 3), got {normal.shape}")
    elif mode == RT_GATHER_SH9:
        raise ValueError(f"{fn}: RT_GATHER_SH9 needs the normals")
    return n, prim, uv, normal


def _sample_planes(fn, W, H, mode, planes):
    """`planes` as a C-contiguous float32 (H, W, Wd) array (None stays None); a size, mode or shape out of range is a ValueError."""
    if mode not in _GATHER_WIDTH:
        raise ValueError(f"{fn}: unknown mode {mode!r}")
    if not (1 <= W <= RT_TEXEL_MAX_SIZE and 1 <= H <= RT_TEXEL_MAX_SIZE):
        raise ValueError(f"{fn}: needs 1 <= W, H <= RT_TEXEL_MAX_SIZE")
    if planes is not None:
        planes = np.ascontiguousarray(planes, dtype=np.float32)
        if planes.shape != (H, W, _GATHER_WIDTH[mode]):
            raise ValueError(f"{fn}: the planes must have shape {(H, W, _GATHER_WIDTH[mode])}, got {planes.shape}")
    return planes


def sample_texels(prim, uv, normal, W, H, mode, planes=None, flags=0):
    """Looks texel planes up at hits on the device (sampleTexels, include/rt_api.h): prim (n,) and uv (n, 2) as trace_rays returns them, normal (n, 3) or
    None (RT_GATHER_SH9 needs it); `planes` an (H, W, Wd) float32 array, Wd = gather_width(mode), or None with RT_TEXELS_FROM_BAKE / RT_TEXELS_FROM_FILTER in
    `flags`: the out plane of the last bake_texels / filter_texels, where it lies on the device.  RT_SAMPLE_BILINEAR: four taps instead of the nearest texel.
    Returns (valid hits, out (n, 3) float32, valid (n,) uint8).  Blocking."""
    n, prim, uv, normal = _sample_hits("sample_texels", prim, uv, normal, mode)
    planes = _sample_planes("sample_texels", W, H, mode, planes)
    out, valid = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    count = load_renderer().sampleTexels(n, prim.ctypes.data_as(ip), uv.ctypes.data_as(fp), _plane_ptr(normal, fp), W, H, mode, _plane_ptr(planes, fp), flags,
                                         out.ctypes.data_as(fp), valid.ctypes.data_as(C.POINTER(C.c_uint8)))
    return count, out, valid


def sample_texels_host(tris, prim, uv, normal, W, H, mode, planes, flags=0):
    """sample_texels on the CPU (librt_host.so, rtSampleTexelsHost; no GPU, no renderer state) over `tris`, a 1-D array of triangle_dtype in slot order: the
    same bits.  Returns (valid hits, out, valid); what the device call would refuse, and planes None, is a ValueError."""
    tris = _records("sample_texels_host", "triangle", tris, triangle_dtype)
    n, prim, uv, normal = _sample_hits("sample_texels_host", prim, uv, normal, mode)
    planes = _sample_planes("sample_texels_host", W, H, mode, planes)
    out, valid = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    count = load_host().rtSampleTexelsHost(tris.ctypes.data if len(tris) else None, len(tris), n, prim.ctypes.data_as(ip), uv.ctypes.data_as(fp),
                                           _plane_ptr(normal, fp), W, H, mode, _plane_ptr(planes, fp), flags, out.ctypes.data_as(fp),
                                           valid.ctypes.data_as(C.POINTER(C.c_uint8)))
    if count < 0:
        raise ValueError("sample_texels_host: needs planes and no flag but RT_SAMPLE_BILINEAR")
    return count, out, valid


def render_lightmap(W, H, mode, planes=None, flags=0, floor_value=None, out=None):
    """The frame of the centre rays lit by texel planes (renderLightmap, include/rt_api.h): `planes` and the FROM flags as sample_texels takes them;
    RT_LIGHTMAP_ALBEDO multiplies a hit by the RT_GUIDE_ALBEDO value of its pixel; floor_value: what a floor hit is lit with, None = (1, 1, 1).  `out`: None
    (a new array) or a writable C-contiguous (ny, nx, 3) float32 array.  Returns the frame, row 0 at the bottom.  Blocking."""
    planes = _sample_planes("render_lightmap", W, H, mode, planes)
    shape = (_state["ny"], _state["nx"], 3)
    if out is None:
        out = np.zeros(shape, np.float32)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == shape and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]):
        raise ValueError(f"render_lightmap: out must be a writable C-contiguous float32 array of shape {shape}")
    fp = C.POINTER(C.c_float)
    fv = None if floor_value is None else (C.c_float * 3)(*[float(v) for v in floor_value])
    load_renderer().renderLightmap(W, H, mode, _plane_ptr(planes, fp), flags, None if fv is None else C.cast(fv, fp), out.ctypes.data_as(C.POINTER(vec3)))
    return out


def last_sample_ms():
    """HIP-event time of the lookup kernels of the last sample_texels (not the copies), summed over its chunks, in milliseconds."""
    return load_renderer().rtLastSampleMs()


def last_lightmap_ms():
    """HIP-event time of ray generator + trace + shade of the last render_lightmap (not the copies), summed over its chunks, in milliseconds."""
    return load_renderer().rtLastLightmapMs()


def pinhole_camera(o, target):
    """The camera under which every pixel of a frame is the ray from o towards target (rtPinholeCamera, librt_host.so; no GPU): origin = o,
    lower_left_corner = target, every other field 0.  The pixel with global id `id` of runRenderer(ns) under it is radiance_rays of (o, target - o, id)."""
    fp = C.POINTER(C.c_float)
    o = np.ascontiguousarray(o, dtype=np.float32)
    t = np.ascontiguousarray(target, dtype=np.float32)
    if o.shape != (3,) or t.shape != (3,):
        raise ValueError(f"pinhole_camera: o and target must have shape (3,), got {o.shape} and {t.shape}")
    cam = camera()
    load_host().rtPinholeCamera(o.ctypes.data_as(fp), t.ctypes.data_as(fp), C.byref(cam))
    return cam


# refineFrame (include/rt_api.h): adaptive sampling on the device over the pixel kernels
RT_REFINE_DILATE = 1
RT_REFINE_LUM_EPS = 1e-3
REFINE_PLANES = ("out", "samples", "error")


def refine_frame(batch, min_batches, max_samples, threshold, flags=0, want=REFINE_PLANES):
    """One pass of the adaptive frame (refineFrame, include/rt_api.h): selects the pixels that are not converged under these parameters, traces `batch` more
    samples for each and updates their statistics.  Returns (sampled, out, samples, error): the number of pixels sampled - 0 = the frame is finished under
    these parameters - and the planes named in `want`, None for the others: out (ny, nx, 3) float32 = the mean, samples (ny, nx) int32, error (ny, nx)
    float32; row 0 = bottom.  want=() downloads nothing.  Blocking."""
    for name, v in (("batch", batch), ("min_batches", min_batches), ("max_samples", max_samples), ("flags", flags)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise ValueError(f"refine_frame: {name} must be an int, got {v!r}")
    if not isinstance(threshold, (int, float, np.floating, np.integer)) or isinstance(threshold, bool):
        raise ValueError(f"refine_frame: threshold must be a number, got {threshold!r}")
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in REFINE_PLANES]
    if unknown:
        raise ValueError(f"refine_frame: want names unknown planes {unknown}; the planes are {REFINE_PLANES}")
    ny, nx = _state["ny"], _state["nx"]
    out = np.zeros((ny, nx, 3), np.float32) if "out" in want else None
    samples = np.zeros((ny, nx), np.int32) if "samples" in want else None
    error = np.zeros((ny, nx), np.float32) if "error" in want else None
    sampled = load_renderer().refineFrame(None if out is None else out.ctypes.data_as(C.POINTER(vec3)),
                                          None if samples is None else samples.ctypes.data_as(C.POINTER(C.c_int32)),
                                          None if error is None else error.ctypes.data_as(C.POINTER(C.c_float)),
                                          int(batch), int(min_batches), int(max_samples), float(threshold), int(flags))
    return sampled, out, samples, error


def reset_refine():
    """The next refine_frame starts at sample 0 (rtResetRefine)."""
    load_renderer().rtResetRefine()


def refine_samples():
    """Samples traced by refine_frame since the last reset, over all pixels (rtRefineSamples)."""
    return load_renderer().rtRefineSamples()


def refine_last_list():
    """The list of the last refine_frame's pass in the order it was handed to the pixel kernel (rtRefineLastList): (n, 2) int32, column i then row j."""
    r = load_renderer()
    n = r.rtRefineLastList(None, 0)
    ij = np.zeros((n, 2), np.int32)
    if n > 0:
        r.rtRefineLastList(ij.ctypes.data_as(C.POINTER(C.c_int32)), n)
    return ij


def last_refine_ms():
    """HIP-event time of select + pixel kernel + update of the last refine_frame (not the deliver kernel or the copies), in milliseconds."""
    return load_renderer().rtLastRefineMs()


# updateTriangles / updateMaterials / updateSpheres (include/rt_api.h): edit the scene in place.  The wrappers take arrays of the exact record type and
# convert nothing: a wrong dtype or shape is a ValueError before the library is called.
def _records(fn, name, a, dtype):
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.ndim == 1):
        raise ValueError(f"{fn}: {name} must be a one-dimensional numpy array of {name}_dtype records")
    return np.ascontiguousarray(a)


def update_triangles(first, tris):
    """Replaces slots [first, first + len(tris)) of the leaf-ordered triangle array given to initRenderer (HostMesh.tris) and refits the BVH on every device
    (updateTriangles).  tris: a 1-D array of triangle_dtype.  Blocking; an empty array changes nothing."""
    tris = _records("update_triangles", "triangle", tris, triangle_dtype)
    if isinstance(first, bool) or not isinstance(first, (int, np.integer)):
        raise ValueError("update_triangles: first must be an integer")
    load_renderer().updateTriangles(int(first), len(tris), tris.ctypes.data if len(tris) else None)


def update_materials(mats):
    """Replaces the material array of a mesh scene (updateMaterials): a 1-D array of material_dtype, as many as at init."""
    mats = _records("update_materials", "material", mats, material_dtype)
    load_renderer().updateMaterials(mats.ctypes.data, len(mats))


def update_spheres(spheres, mats):
    """Replaces spheres and materials of a sphere scene (updateSpheres): 1-D arrays of sphere_dtype and material_dtype, as many as at init."""
    spheres = _records("update_spheres", "sphere", spheres, sphere_dtype)
    mats = _records("update_spheres", "material", mats, material_dtype)
    if len(spheres) != len(mats):
        raise ValueError("update_spheres: one material per sphere")
    load_renderer().updateSpheres(spheres.ctypes.data, mats.ctypes.data, len(spheres))


def mesh_bvh():
    """The first device's current BVH of a mesh scene (getMeshBvh): (nodes, bounds) - numBvhNodes records of bvh_node_dtype, node 0 unused, and the scene
    bounds as a (2, 3) float32 array (min, max)."""
    r = load_renderer()
    n = r.getMeshBvh(None, 0, None)
    nodes = np.zeros(n, bvh_node_dtype)
    b = bbox()
    r.getMeshBvh(nodes.ctypes.data, n, C.byref(b))
    return nodes, np.array([list(b.min.e), list(b.max.e)], np.float32)


def last_update_ms():
    """HIP-event time of the refit kernels of the last update_triangles (the largest over the in-process devices), in milliseconds; 0 before the first."""
    return load_renderer().rtLastUpdateMs()


def _header_constant(name):
    """An integer #define of include/rt_api.h (a literal or 1 << k): constants the header exports are read from it, not written down twice."""
    import re
    text = open(os.path.join(os.path.dirname(_HERE), "include", "rt_api.h")).read()
    m = re.search(r"^#define\s+%s\s+\(?\s*(\d+)\s*(?:<<\s*(\d+))?\s*\)?\s*$" % name, text, re.M)
    if not m:
        raise ImportError(f"include/rt_api.h does not define {name}")
    return int(m.group(1)) << int(m.group(2) or 0)


RT_REBUILD_TILE = _header_constant("RT_REBUILD_TILE")            # elements one workgroup of the rebuild's scan kernels covers
RT_REBUILD_MAX_TRIS = _header_constant("RT_REBUILD_MAX_TRIS")


def rebuild_bvh():
    """Re-splits the BVH of a mesh scene on every device (rebuildBvh): the tree's shape stays, the triangles are assigned to leaf slots anew, the boxes are
    refitted.  Blocking.  Returns old_slot: int32, one entry per slot of the triangle array - the slot its triangle came from, -1 for a sentinel."""
    r = load_renderer()
    old_slot = np.zeros(int(_state.get("num_tris") or 0) if not _state.get("spheres") else 0, np.int32)
    r.rebuildBvh(old_slot.ctypes.data if len(old_slot) else None)
    return old_slot


def last_rebuild_ms():
    """HIP-event time of the build and refit kernels of the last rebuild_bvh (the largest over the in-process devices), in milliseconds; 0 before the first."""
    return load_renderer().rtLastRebuildMs()


def rebuild_bvh_arrays(tris, bvh, nppl):
    """rtRebuildBvhArrays on caller-owned arrays: rebuilds in place `tris` (1-D triangle_dtype, writable) and `bvh` (1-D bvh_node_dtype, writable).  Returns
    (bounds, old_slot) - the bounds as a (2, 3) float32 array, old_slot as int32 per slot - or None where the library refuses the arrays (-1)."""
    for name, a, dt in (("tris", tris, triangle_dtype), ("bvh", bvh, bvh_node_dtype)):
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.ndim == 1 and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"]):
            raise ValueError(f"rebuild_bvh_arrays: {name} must be a writable C-contiguous one-dimensional array of its record dtype")
    if isinstance(nppl, bool) or not isinstance(nppl, (int, np.integer)):
        raise ValueError("rebuild_bvh_arrays: nppl must be an integer")
    b = bbox()
    old_slot = np.zeros(len(tris), np.int32)
    if load_host().rtRebuildBvhArrays(tris.ctypes.data, len(tris), bvh.ctypes.data, len(bvh), int(nppl), C.byref(b), old_slot.ctypes.data) != 0:
        return None
    return np.array([list(b.min.e), list(b.max.e)], np.float32), old_slot


def refit_bvh_arrays(tris, bvh, nppl):
    """rtRefitBvhArrays on caller-owned arrays: refits `bvh` (1-D bvh_node_dtype, writable) in place from `tris` (1-D triangle_dtype).  Returns the bounds as a
    (2, 3) float32 array, or None where the library refuses the arrays (-1)."""
    tris = _records("refit_bvh_arrays", "triangle", tris, triangle_dtype)
    if not (isinstance(bvh, np.ndarray) and bvh.dtype == bvh_node_dtype and bvh.ndim == 1 and bvh.flags["C_CONTIGUOUS"] and bvh.flags["WRITEABLE"]):
        raise ValueError("refit_bvh_arrays: bvh must be a writable C-contiguous one-dimensional array of bvh_node_dtype records")
    b = bbox()
    if load_host().rtRefitBvhArrays(tris.ctypes.data, len(tris), bvh.ctypes.data, len(bvh), int(nppl), C.byref(b)) != 0:
        return None
    return np.array([list(b.min.e), list(b.max.e)], np.float32)


def centre_rays(cam, nx, ny, ij):
    """The centre rays of pixels ij = (n, 2) int (column i, row j; row 0 = bottom) of an nx x ny image as renderGuides defines them (rtCentreRays,
    librt_host.so; no GPU): (org, dir), both (n, 3) float32, dir of unit length."""
    ij = np.ascontiguousarray(ij, dtype=np.int32)
    if ij.ndim != 2 or ij.shape[1] != 2:
        raise ValueError(f"centre_rays: ij must have shape (n, 2), got {ij.shape}")
    n = ij.shape[0]
    org, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    fp = C.POINTER(C.c_float)
    load_host().rtCentreRays(C.byref(cam), nx, ny, ij.ctypes.data_as(C.POINTER(C.c_int32)), n, org.ctypes.data_as(fp), d.ctypes.data_as(fp))
    return org, d


# denoiseFrame (include/rt_api.h): the flags, the limits and the defaults
RT_DENOISE_DEMODULATE, RT_DENOISE_SAME_PRIM = 1, 2
RT_DENOISE_MAX_ITERATIONS, RT_DENOISE_MAX_SQUARINGS, RT_DENOISE_ALBEDO_FLOOR = 8, 7, 0.01


def default_denoise_flags():
    """DEMODULATE | SAME_PRIM for the sphere scene that is initialised, DEMODULATE for a mesh scene."""
    return load_renderer().rtDefaultDenoiseFlags()


def _frame_in_out(who, fb, out):
    """The arrays of a whole-image pass, checked against (ny, nx, 3) float32 C-contiguous: (address of the input frame or None, the output array: `out`,
    which must be writable, or a new one)."""
    shape = (_state["ny"], _state["nx"], 3)
    ok = lambda a: isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and a.shape == shape
    if fb is not None and not ok(fb):
        raise ValueError(f"{who}: fb must be a C-contiguous float32 array of shape {shape}")
    if out is None:
        out = np.empty(shape, np.float32)
    elif not (ok(out) and out.flags["WRITEABLE"]):
        raise ValueError(f"{who}: out must be a writable C-contiguous float32 array of shape {shape}")
    return None if fb is None else fb.ctypes.data, out


def denoiseFrame(fb=None, iterations=5, flags=None, normal_squarings=5, sigma_z=0.01, sigma_c=1.0, out=None):
    """The guide-driven edge-avoiding a-trous filter on a whole frame (include/rt_api.h).  fb: a (ny, nx, 3) float32 array, row 0 = bottom; None = the
    framebuffer the renderer currently delivers into.  flags None = the scene kind's default.  Returns the denoised (ny, nx, 3) float32 array: a new one, or
    `out` (a writable C-contiguous float32 array of that shape; it may be `fb` itself: in place).  Blocking; always the whole image on the first device."""
    r = load_renderer()
    if flags is None:
        flags = r.rtDefaultDenoiseFlags()
    src, out = _frame_in_out("denoiseFrame", fb, out)
    r.denoiseFrame(src, out.ctypes.data, iterations, flags, normal_squarings, sigma_z, sigma_c)
    return out


def last_denoise_ms():
    """HIP-event time of the kernels of the last denoiseFrame (prologue + iterations), in milliseconds; 0 before the first call."""
    return load_renderer().rtLastDenoiseMs()


# accumulateFrame (include/rt_api.h): the largest history length
RT_ACCUM_MAX_HISTORY = 1024


def accumulateFrame(fb=None, out=None, history=False, flags=None, max_history=32, sigma_z=0.01, normal_min=0.9):
    """Temporal accumulation for a moving camera (include/rt_api.h): blends the frame with the previous call's result, reprojected through the hit points
    and checked against the previous frame's geometry.  fb: a (ny, nx, 3) float32 array, row 0 = bottom; None = the framebuffer the renderer currently
    delivers into.  out: a writable C-contiguous float32 array of that shape (it may be `fb` itself: in place), None = a new one.  history: True = also
    return the per-pixel history length N as a (ny, nx) float32 array, or such an array to fill.  flags None = the scene kind's default.  Returns out, or
    (out, history).  Blocking; always the whole image on the first device.  The loop of a camera move: setCamera, runRenderer(1), accumulateFrame,
    denoiseFrame."""
    nx, ny = _state["nx"], _state["ny"]
    r = load_renderer()
    if flags is None:
        flags = r.rtDefaultDenoiseFlags()
    src, out = _frame_in_out("accumulateFrame", fb, out)
    hist = None
    if history is True:
        hist = np.empty((ny, nx), np.float32)
    elif history is not False and history is not None:
        hist = history
        if not (isinstance(hist, np.ndarray) and hist.dtype == np.float32 and hist.flags["C_CONTIGUOUS"] and hist.flags["WRITEABLE"] and hist.shape == (ny, nx)):
            raise ValueError(f"accumulateFrame: history must be True, False or a writable C-contiguous float32 array of shape {(ny, nx)}")
    r.accumulateFrame(src, out.ctypes.data, None if hist is None else hist.ctypes.data, flags, max_history, sigma_z, normal_min)
    return out if hist is None else (out, hist)


def reset_history():
    """The next accumulateFrame has no history."""
    load_renderer().rtResetHistory()


def history_frames():
    """accumulateFrame calls since init / the last reset of the history."""
    return load_renderer().rtHistoryFrames()


def last_accumulate_ms():
    """HIP-event time of the kernel of the last accumulateFrame, in milliseconds; 0 before the first call."""
    return load_renderer().rtLastAccumulateMs()


# previewFrame (include/rt_api.h): the history length below which the variance is the spatial estimate, and the floor of the luminance width
RT_PREVIEW_MIN_HISTORY, RT_PREVIEW_LUM_EPS = 4.0, 1e-4


def _pixel_plane(who, what, plane):
    """An optional (ny, nx) float32 plane of a whole-image pass: True = a new array, False / None = none, or a writable C-contiguous array to fill."""
    shape = (_state["ny"], _state["nx"])
    if plane is True:
        return np.empty(shape, np.float32)
    if plane is False or plane is None:
        return None
    if not (isinstance(plane, np.ndarray) and plane.dtype == np.float32 and plane.flags["C_CONTIGUOUS"] and plane.flags["WRITEABLE"] and plane.shape == shape):
        raise ValueError(f"{who}: {what} must be True, False or a writable C-contiguous float32 array of shape {shape}")
    return plane


def previewFrame(fb=None, out=None, history=False, variance=False, flags=None, max_history=32, iterations=5, normal_squarings=5, sigma_z=0.01, normal_min=0.9,
                 sigma_l=4.0):
    """accumulateFrame and denoiseFrame in one device pass, the filter's colour width set pixel by pixel by the variance of the accumulated luminance
    (include/rt_api.h).  fb, out, history as accumulateFrame's; variance: True = also return the per-pixel variance of stage V as a (ny, nx) float32 array, or
    such an array to fill.  flags None = the scene kind's default.  Returns out, or a tuple (out, history and / or variance, in that order).  Blocking; always
    the whole image on the first device; a history of its own.  The loop of a camera move: setCamera, runRenderer(1), previewFrame."""
    r = load_renderer()
    if flags is None:
        flags = r.rtDefaultDenoiseFlags()
    src, out = _frame_in_out("previewFrame", fb, out)
    hist = _pixel_plane("previewFrame", "history", history)
    var = _pixel_plane("previewFrame", "variance", variance)
    r.previewFrame(src, out.ctypes.data, None if hist is None else hist.ctypes.data, None if var is None else var.ctypes.data, flags, max_history, iterations,
                   normal_squarings, sigma_z, normal_min, sigma_l)
    planes = tuple(a for a in (hist, var) if a is not None)
    return (out,) + planes if planes else out


def reset_preview():
    """The next previewFrame has no history."""
    load_renderer().rtResetPreview()


def preview_frames():
    """previewFrame calls since init / the last reset of its history."""
    return load_renderer().rtPreviewFrames()


def last_preview_ms():
    """HIP-event time of the kernels of the last previewFrame (temporal, variance, iterations), in milliseconds; 0 before the first call."""
    return load_renderer().rtLastPreviewMs()


# rtMarkPose / renderMotion (include/rt_api.h): the planes of the mask
RT_MOTION_POS, RT_MOTION_NORMAL, RT_MOTION_SCREEN = 1, 2, 4
MOTION_PLANES = (("prev_pos", RT_MOTION_POS, 3), ("prev_normal", RT_MOTION_NORMAL, 3), ("screen", RT_MOTION_SCREEN, 2))


def mark_pose():
    """Remembers the scene's geometry as it is now - "the previous frame's pose" (rtMarkPose): from now on accumulateFrame and previewFrame reproject every
    pixel through the point its surface point had in that pose, so what an edit moves keeps its history.  The loop of an animated frame: mark_pose,
    update_triangles / update_spheres (and rebuild_bvh), setCamera, runRenderer(1), previewFrame, display_frame."""
    load_renderer().rtMarkPose()


def clear_pose():
    """Forgets the marked pose (rtClearPose): the passes reproject through the current hit points again."""
    load_renderer().rtClearPose()


def pose_marked():
    """True while a pose is marked."""
    return bool(load_renderer().rtPoseMarked())


def renderMotion(prev_cam=None, mask=RT_MOTION_POS | RT_MOTION_NORMAL | RT_MOTION_SCREEN):
    """The motion planes of the current camera against the marked pose (include/rt_api.h).  Returns a dict with the planes of `mask`: prev_pos, prev_normal
    (ny, nx, 3) float32 - where every pixel's surface point was in the marked pose and the normal it had there - and screen (ny, nx, 2) float32 - where
    prev_cam (None = the current camera) saw that point, relative to the pixel, in pixels.  Without a marked pose prev_pos and prev_normal are the current hit
    point and normal.  Blocking; always the whole image on the first device."""
    nx, ny = _state["nx"], _state["ny"]
    res, ptrs = {}, []
    for name, bit, comps in MOTION_PLANES:
        if not (mask & bit):
            ptrs.append(None)
            continue
        res[name] = np.zeros((ny, nx, comps), np.float32)
        ptrs.append(res[name].ctypes.data_as(C.POINTER(C.c_float)))
    load_renderer().renderMotion(mask, None if prev_cam is None else C.byref(prev_cam), *ptrs)
    return res


def last_motion_ms():
    """HIP-event time of the motion kernel of the last renderMotion, in milliseconds; 0 before the first call."""
    return load_renderer().rtLastMotionMs()


# displayFrame (include/rt_api.h): the flags, the tone maps, the histogram's size, the key the median luminance is exposed to, the dither matrix
RT_DISPLAY_TOP_DOWN, RT_DISPLAY_DITHER, RT_DISPLAY_AUTO_EXPOSURE, RT_DISPLAY_FROM_PREVIEW = 1, 2, 4, 8
RT_TONEMAP_NONE, RT_TONEMAP_REINHARD, RT_TONEMAP_ACES = 0, 1, 2
RT_DISPLAY_BINS, RT_DISPLAY_KEY = 256, 0.18
RT_DISPLAY_BAYER8 = ((0, 32, 8, 40, 2, 34, 10, 42), (48, 16, 56, 24, 50, 18, 58, 26), (12, 44, 4, 36, 14, 46, 6, 38), (60, 28, 52, 20, 62, 30, 54, 22),
                     (3, 35, 11, 43, 1, 33, 9, 41), (51, 19, 59, 27, 49, 17, 57, 25), (15, 47, 7, 39, 13, 45, 5, 37), (63, 31, 55, 23, 61, 29, 53, 21))


def _display_in_out(who, src, out, shape):
    """The arrays of a display call, checked: (address of the (ny, nx, 3) float32 input or None, the (ny, nx, 4) uint8 output: `out` or a new one)."""
    if src is not None and not (isinstance(src, np.ndarray) and src.dtype == np.float32 and src.flags["C_CONTIGUOUS"] and src.shape == shape + (3,)):
        raise ValueError(f"{who}: src must be a C-contiguous float32 array of shape {shape + (3,)}")
    if out is None:
        out = np.empty(shape + (4,), np.uint8)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.shape == shape + (4,)):
        raise ValueError(f"{who}: out must be a writable C-contiguous uint8 array of shape {shape + (4,)}")
    return None if src is None else src.ctypes.data, out


def display_frame(src=None, out=None, flags=0, tonemap=0, exposure=1.0, adapt=1.0):
    """Exposure, tone map, sRGB and optional ordered dither on the device (include/rt_api.h): returns the (ny, nx, 4) uint8 picture R, G, B, 255 - a new array, or
    `out`.  src: a (ny, nx, 3) float32 array, row 0 = bottom; None = the framebuffer the renderer currently delivers into, or with RT_DISPLAY_FROM_PREVIEW the
    output of the last previewFrame where it lies on the device.  RT_DISPLAY_TOP_DOWN flips the rows; RT_DISPLAY_AUTO_EXPOSURE exposes the median luminance to
    RT_DISPLAY_KEY, adapting by `adapt` per call.  Blocking; always the whole image on the first device."""
    src, out = _display_in_out("display_frame", src, out, (_state["ny"], _state["nx"]))
    load_renderer().displayFrame(src, out.ctypes.data, flags, tonemap, exposure, adapt)
    return out


def last_exposure():
    """E_used of the last display_frame; 1 before the first."""
    return load_renderer().rtLastExposure()


def display_histogram():
    """The RT_DISPLAY_BINS luminance bins of the last RT_DISPLAY_AUTO_EXPOSURE call (8 per octave over 2^-16 .. 2^16) as a uint32 array; zero after a reset."""
    out = np.zeros(RT_DISPLAY_BINS, np.uint32)
    n = load_renderer().rtDisplayHistogram(out.ctypes.data_as(C.POINTER(C.c_uint32)), RT_DISPLAY_BINS)
    assert n == RT_DISPLAY_BINS
    return out


def reset_display():
    """The next RT_DISPLAY_AUTO_EXPOSURE call adapts from nothing."""
    load_renderer().rtResetDisplay()


def last_display_ms():
    """HIP-event time of the kernels of the last display_frame, in milliseconds; 0 before the first call."""
    return load_renderer().rtLastDisplayMs()


def display_frame_host(src, out=None, flags=0, tonemap=0, exposure=1.0, adapt=1.0, state=None, histogram=False):
    """display_frame's definition on the CPU (librt_host.so, rtDisplayFrameHost; no GPU, no renderer state): the same bytes.  src: any (ny, nx, 3) float32
    array.  state: None, or a one-element float32 array holding E' (NaN = adapt from nothing) that receives E.  histogram=True: returns (out, bins)."""
    if not (isinstance(src, np.ndarray) and src.ndim == 3):
        raise ValueError("display_frame_host: src must be a (ny, nx, 3) float32 array")
    addr, out = _display_in_out("display_frame_host", src, out, src.shape[:2])
    if state is not None and not (isinstance(state, np.ndarray) and state.dtype == np.float32 and state.size == 1 and state.flags["WRITEABLE"]):
        raise ValueError("display_frame_host: state must be None or a writable float32 array of one element")
    hist = np.zeros(RT_DISPLAY_BINS, np.uint32) if histogram else None
    rc = load_host().rtDisplayFrameHost(addr, out.ctypes.data, src.shape[1], src.shape[0], flags, tonemap, exposure, adapt,
                                        None if state is None else state.ctypes.data_as(C.POINTER(C.c_float)),
                                        None if hist is None else hist.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != 0:
        raise ValueError("display_frame_host: arguments displayFrame would refuse (flags, tonemap, exposure or adapt)")
    return (out, hist) if histogram else out


def cleanupRenderer():
    """extern "C" cleanupRenderer (/root/reference/kernels.h:8). The framebuffer view is dead afterwards."""
    load_renderer().cleanupRenderer()
    _state.update(fb=None, keep=None)


def getDefaultRenderOptions(is_sphere_scene):
    o = render_options()
    load_renderer().getDefaultRenderOptions(C.byref(o), 1 if is_sphere_scene else 0)
    return o


def setRenderOptions(opt=None, **kw):
    """Set options for the following runRenderer calls; keyword arguments override fields of `opt`."""
    if opt is None:
        raise ValueError("pass the options struct from getDefaultRenderOptions()")
    for k, v in kw.items():
        if k == "devices":
            opt.num_devices = len(v)
            for idx, d in enumerate(v):
                opt.devices[idx] = d
        else:
            setattr(opt, k, v)
    load_renderer().setRenderOptions(C.byref(opt))
    return opt


def setExternalFramebuffer(array):
    """Deliver the following renders into `array` ((ny, nx, 3) float32, C-contiguous, e.g. a shared memmap); None reverts."""
    if array is None:
        load_renderer().setExternalFramebuffer(None)
        _state["ext"] = None
        return
    assert array.dtype == np.float32 and array.flags["C_CONTIGUOUS"] and array.shape == (_state["ny"], _state["nx"], 3)
    load_renderer().setExternalFramebuffer(array.ctypes.data)
    _state["ext"] = array


def getRenderStats():
    s = render_stats()
    load_renderer().getRenderStats(C.byref(s))
    return s


def device_count():
    return load_renderer().rtDeviceCount()


# rtLastLaunches (include/rt_api.h): kernel families and the words of a launch record
RT_KERNEL_SPHERE_QUEUE, RT_KERNEL_SPHERE_TILES, RT_KERNEL_MESH_QUEUE, RT_KERNEL_MESH_TILES = 1, 2, 3, 4
LAUNCH_FIELDS = ("family", "phase", "cls", "chunked", "dbg", "scene", "lean", "threads", "blocks", "device", "fp")


def last_launches():
    """The render-kernel launches of the last runRenderer, in launch order: one dict per launch with the LAUNCH_FIELDS of its record."""
    lib = load_renderer()
    n = lib.rtLastLaunches(None, 0)
    buf = (C.c_int32 * (n * len(LAUNCH_FIELDS)))()
    n = min(n, lib.rtLastLaunches(buf, n))
    return [dict(zip(LAUNCH_FIELDS, buf[k * len(LAUNCH_FIELDS):(k + 1) * len(LAUNCH_FIELDS)])) for k in range(n)]


RT_SPHERE_FORM_NONE, RT_SPHERE_FORM_GENERAL, RT_SPHERE_FORM_DEFAULT = -1, 0, 1


def last_sphere_form():
    """rtLastSphereForm (include/rt_api.h): the form of the cost-ordered sphere dispatch of the last frame or pass, RT_SPHERE_FORM_NONE if it had none."""
    lib = load_renderer()
    lib.rtLastSphereForm.argtypes = []
    lib.rtLastSphereForm.restype = C.c_int
    return lib.rtLastSphereForm()


# ---------------------------------------------------------------------------------------------
# output / verification harness (main.cpp:25-60,105-128; staircase_scene.h:22-43)
# ---------------------------------------------------------------------------------------------

def write_ppm(path, fb):
    fb = np.ascontiguousarray(fb, dtype=np.float32)
    return load_host().rtWritePPM(os.fsencode(path), fb.shape[1], fb.shape[0], fb.ctypes.data)


def save_reference(path, fb):
    fb = np.ascontiguousarray(fb, dtype=np.float32)
    return load_host().rtSaveReference(os.fsencode(path), fb.shape[1], fb.shape[0], fb.ctypes.data)


def load_reference(path, nx, ny):
    out = np.zeros((ny, nx, 3), np.float32)
    rc = load_host().rtLoadReference(os.fsencode(path), out.ctypes.data, nx, ny)
    return rc, out


def rmse(f, g):
    f = np.ascontiguousarray(f, dtype=np.float32)
    g = np.ascontiguousarray(g, dtype=np.float32)
    assert f.shape == g.shape
    return load_host().rtRmse(f.ctypes.data, g.ctypes.data, f.shape[1], f.shape[0])


# ---------------------------------------------------------------------------------------------
# per-function device probes (include/rt_probe.h)
# ---------------------------------------------------------------------------------------------

PROBE_SYMBOLS = [f"rtProbe{n}_{m}" for n in ("Rng", "DiskSphere", "GetRay", "SphereHit", "TriangleHit", "Bbox", "Scatter", "Math", "ShadowRay", "PlaneHit", "SinCos", "Schlick")
                 for m in ("parity", "fast")] + ["rtProbeRenorm_parity", "rtProbeExactDiv_parity", "rtProbeExactDivStored_parity"]


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Probe:
    """probe = Probe('parity'); probe.sphere_hit(...)  — every method returns numpy arrays."""

    def __init__(self, mode="parity"):
        assert mode in ("parity", "fast")
        self.lib = load_renderer()
        self.sfx = "_" + mode

    def _fn(self, name):
        f = getattr(self.lib, "rtProbe" + name + self.sfx)
        f.restype = None
        return f

    def rng(self, pixel_ids):
        ids = _u32(pixel_ids); n = len(ids)
        seed = np.zeros(n, np.uint32); draws = np.zeros((n, 4), np.float32); state = np.zeros(n, np.uint32)
        self._fn("Rng")(_p(ids), C.c_int(n), _p(seed), _p(draws), _p(state))
        return seed, draws, state

    def disk_sphere(self, states):
        st = _u32(states); n = len(st)
        disk = np.zeros((n, 3), np.float32); sd = np.zeros(n, np.uint32)
        sph = np.zeros((n, 3), np.float32); ss = np.zeros(n, np.uint32)
        self._fn("DiskSphere")(_p(st), C.c_int(n), _p(disk), _p(sd), _p(sph), _p(ss))
        return disk, sd, sph, ss

    def get_ray(self, cam, s, t, states):
        s = _f32(s); t = _f32(t); st = _u32(states); n = len(s)
        org = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32); sa = np.zeros(n, np.uint32)
        self._fn("GetRay")(C.byref(cam), _p(s), _p(t), _p(st), C.c_int(n), _p(org), _p(d), _p(sa))
        return org, d, sa

    def sphere_hit(self, spheres, org, dirs, tmin, tmax):
        sp = np.ascontiguousarray(spheres, dtype=sphere_dtype); n = len(sp)
        org = _f32(org); dirs = _f32(dirs); tmin = _f32(tmin); tmax = _f32(tmax)
        out = np.zeros(n, np.float32)
        self._fn("SphereHit")(_p(sp), _p(org), _p(dirs), _p(tmin), _p(tmax), C.c_int(n), _p(out))
        return out

    def triangle_hit(self, tris, org, dirs, tmin, tmax):
        tr = np.ascontiguousarray(tris, dtype=triangle_dtype); n = len(tr)
        org = _f32(org); dirs = _f32(dirs); tmin = _f32(tmin); tmax = _f32(tmax)
        t = np.zeros(n, np.float32); u = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
        self._fn("TriangleHit")(_p(tr), _p(org), _p(dirs), _p(tmin), _p(tmax), C.c_int(n), _p(t), _p(u), _p(v))
        return t, u, v

    def bbox(self, bmin, bmax, org, dirs, tmax):
        bmin = _f32(bmin); bmax = _f32(bmax); org = _f32(org); dirs = _f32(dirs); tmax = _f32(tmax); n = len(tmax)
        dist = np.zeros(n, np.float32); hit = np.zeros(n, np.int32)
        self._fn("Bbox")(_p(bmin), _p(bmax), _p(org), _p(dirs), _p(tmax), C.c_int(n), _p(dist), _p(hit))
        return dist, hit

    def scatter(self, t, normal, inside, wo, mats, color, states, hit_point=None):
        t = _f32(t); normal = _f32(normal); inside = np.ascontiguousarray(inside, dtype=np.int32); wo = _f32(wo)
        hp = _f32(hit_point if hit_point is not None else np.zeros((len(t), 3), np.float32))
        mats = np.ascontiguousarray(mats, dtype=material_dtype); color = _f32(color); st = _u32(states); n = len(t)
        wi = np.zeros((n, 3), np.float32); thr = np.zeros((n, 3), np.float32); flags = np.zeros(n, np.int32)
        tout = np.zeros(n, np.float32); sa = np.zeros(n, np.uint32)
        self._fn("Scatter")(_p(t), _p(hp), _p(normal), _p(inside), _p(wo), _p(mats), _p(color), _p(st), C.c_int(n),
                            _p(wi), _p(thr), _p(flags), _p(tout), _p(sa))
        return wi, thr, flags, tout, sa

    def shadow_ray(self, light, light_color, org, atten, normal, states):
        """generateShadowRay (kernels.cu:363-393). Returns (generated, shadowDir, lightContribution, lightDist, cosAMax, draws, state_after)."""
        org = _f32(org); atten = _f32(atten); normal = _f32(normal); st = _u32(states); n = len(st)
        out = np.zeros((n, 9), np.float32); ok = np.zeros(n, np.int32); sa = np.zeros(n, np.uint32)
        self._fn("ShadowRay")(C.byref(light), C.byref(light_color), _p(org), _p(atten), _p(normal), _p(st), C.c_int(n), _p(out), _p(ok), _p(sa))
        return ok, out[:, 0:3], out[:, 3:6], out[:, 6], out[:, 7], out[:, 8].astype(np.int32), sa

    def plane_hit(self, planes, org, dirs, tmin, tmax):
        pl = np.ascontiguousarray(planes, dtype=np.float32).reshape(-1, 6); n = len(pl)
        org = _f32(org); dirs = _f32(dirs); tmin = _f32(tmin); tmax = _f32(tmax)
        out = np.zeros(n, np.float32)
        self._fn("PlaneHit")(_p(pl), _p(org), _p(dirs), _p(tmin), _p(tmax), C.c_int(n), _p(out))
        return out

    def sincos(self, y):
        """sinf / cosf as generateShadowRay computes them on the device (csrc/rt_glibc_sincosf.h)."""
        y = _f32(y); n = len(y)
        s = np.zeros(n, np.float32); c = np.zeros(n, np.float32)
        self._fn("SinCos")(_p(y), C.c_int(n), _p(s), _p(c))
        return s, c

    def schlick(self, cosine, ref_idx, u):
        """schlick (material.h:9-13) with the device's powf(x, 5) (csrc/rt_glibc_powf.h), and `u < schlick` as the path decides it."""
        c = _f32(cosine); r = _f32(ref_idx); u = _f32(u); n = len(c)
        out = np.zeros(n, np.float32); above = np.zeros(n, np.int32)
        self._fn("Schlick")(_p(c), _p(r), _p(u), C.c_int(n), _p(out), _p(above))
        return out, above

    def renorm(self, v):
        """unit_vector of directions that are unit already, as hit() renormalises the path's direction (csrc/rt_renorm.h).  The parity build only."""
        assert self.sfx == "_parity", "the fast build keeps the plain operators: it has no rtProbeRenorm"
        v = _f32(v).reshape(-1, 3); n = len(v)
        out = np.zeros((n, 3), np.float32)
        self._fn("Renorm")(_p(v), C.c_int(n), _p(out))
        return out

    def exactdiv(self, xyzl):
        """The divisions of csrc/rt_exactdiv.h beside the plain operators, per operand set (x, y, z, l): 14 floats each (include/rt_probe.h).  The parity
        build only."""
        assert self.sfx == "_parity", "the fast build keeps the plain operators: it has no rtProbeExactDiv"
        v = _f32(xyzl).reshape(-1, 4); n = len(v)
        out = np.zeros((n, 14), np.float32)
        self._fn("ExactDiv")(_p(v), C.c_int(n), _p(out))
        return out

    def exactdiv_stored(self, xyzl):
        """(x, y, z) / l by the divisor's stored reciprocal (csrc/rt_exactdiv.h rt_exdiv3_y: the reciprocal from one kernel launch, the quotients from a
        second) beside the plain operator, per operand set (x, y, z, l): 7 floats each (include/rt_probe.h).  The parity build only."""
        assert self.sfx == "_parity", "the fast build keeps the plain operators: it has no rtProbeExactDivStored"
        v = _f32(xyzl).reshape(-1, 4); n = len(v)
        out = np.zeros((n, 7), np.float32)
        self._fn("ExactDivStored")(_p(v), C.c_int(n), _p(out))
        return out

    def math(self, a, b):
        a = _f32(a); b = _f32(b); n = len(a)
        q = np.zeros(n, np.float32); r = np.zeros(n, np.float32); p5 = np.zeros(n, np.float32); u3 = np.zeros((n, 3), np.float32)
        self._fn("Math")(_p(a), _p(b), C.c_int(n), _p(q), _p(r), _p(p5), _p(u3))
        return q, r, p5, u3
