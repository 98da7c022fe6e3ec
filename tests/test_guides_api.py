"""CPU checks of the first-hit guide interface (include/rt_api.h): renderGuides / rtLastGuidesMs are declared, exported and bound with their argument
types, the constants agree between header and Python, the ABI version and struct sizes are the parent's, a call before init is the library's misuse exit
(the check precedes any HIP call), and the test reference (tests/guides_reference.py) shows on every frame of the GPU tests what that frame is there to
cover - a frame that exercises nothing fails here, without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import guides_reference as R
from preview_support import exits_99

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
NEW = ("renderGuides", "rtLastGuidesMs")


def test_declared_exported_and_bound(rt):
    assert re.search(r"void\s+renderGuides\s*\(\s*int\s+mask\s*,\s*float\s*\*\s*albedo\s*,\s*float\s*\*\s*normal\s*,\s*float\s*\*\s*depth\s*,"
                     r"\s*int32_t\s*\*\s*prim\s*,\s*int32_t\s*\*\s*nodes\s*\)\s*;", API)
    assert re.search(r"double\s+rtLastGuidesMs\s*\(\s*void\s*\)\s*;", API)
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    r = rt.load_renderer()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert r.renderGuides.argtypes == [C.c_int, fp, fp, fp, ip, ip] and r.renderGuides.restype is None
    assert r.rtLastGuidesMs.argtypes == [] and r.rtLastGuidesMs.restype is C.c_double
    assert callable(rt.renderGuides) and callable(rt.last_guides_ms)
    assert r.rtLastGuidesMs() == 0.0                            # before the first call; no device is touched


def test_constants_agree_between_header_and_python(rt):
    enums = dict(re.findall(r"\b(RT_GUIDE_[A-Z_]+)\s*=\s*(-?\d+)", API))
    assert {k: int(v) for k, v in enums.items()} == {"RT_GUIDE_ALBEDO": 1, "RT_GUIDE_NORMAL": 2, "RT_GUIDE_DEPTH": 4, "RT_GUIDE_PRIM": 8, "RT_GUIDE_NODES": 16,
                                                    "RT_GUIDE_PRIM_NONE": -1, "RT_GUIDE_PRIM_FLOOR": -2}
    for name, value in enums.items():
        assert getattr(rt, name) == int(value), name
    assert (R.PRIM_NONE, R.PRIM_FLOOR) == (rt.RT_GUIDE_PRIM_NONE, rt.RT_GUIDE_PRIM_FLOOR)
    assert [(n, b) for n, b, _, _ in rt.GUIDE_PLANES] == [("albedo", 1), ("normal", 2), ("depth", 4), ("prim", 8), ("nodes", 16)]


def test_abi_unchanged(rt):
    assert rt.load_renderer().rtApiVersion() == 1002 == rt.RT_API_VERSION
    assert re.search(r"#define RT_API_VERSION 1002\b", API)
    sizes = (C.c_int32 * 32)()
    n = rt.load_renderer().rtStructSizes(sizes, 32)
    assert n == 13 and [sizes[k] for k in range(n)] == [C.sizeof(s) for s in rt.ABI_STRUCTS]


def test_before_init_exits_99():
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99("rt.renderGuides(rt.RT_GUIDE_DEPTH)\n")


def test_guide_kernels_are_built_once_and_keep_away_from_the_form_tables():
    """One arithmetic for both fp modes (PARITY objects only), and names the production-form tripwire does not scan for."""
    for name, kern in (("rt_kernels_spheres.hip", "k_guides_spheres"), ("rt_kernels_mesh.hip", "k_guides_mesh")):
        src = open(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc", name)).read()
        i = src.index("void __launch_bounds__(kThreads) " + kern)
        assert src.rfind("#if defined(RT_MODE_PARITY)", 0, i) > src.rfind("#endif", 0, i), kern
        for scanned in ("launch_mesh_queue<", "k_render_mesh<", "k_render_spheres_tiles<", "launch_queue_form", "launch_kind_of"):
            body = src[i:src.index("#endif", i)]
            assert scanned not in body, (kern, scanned)


# ---- the test reference on the frames of the GPU tests: coverage conditions ------------------------------------------

@pytest.mark.parametrize("name", ["random_96x64", "random_50x37"])
def test_reference_covers_random_spheres(rt, O, name):
    """Hits and misses on at least 10 % of the pixels each, all three material types."""
    c = R.coverage(rt, O, name)
    print(name, c)
    assert c["hit"] >= 0.10 and c["miss"] >= 0.10
    assert c["types"] == [rt.RT_DIFFUSE, rt.RT_METAL, rt.RT_GLASS]


@pytest.mark.parametrize("name", ["three_spheres", "cloud_hybrid", "cloud_global", "tie", "tie_mirror"])
def test_reference_covers_other_sphere_frames(rt, O, name):
    c = R.coverage(rt, O, name)
    print(name, c)
    assert c["hit"] > 0 and c["miss"] > 0
    if name == "tie":                                           # spheres 1 and 3 coincide: the lower caller index takes every pixel of the pair
        prim = R.reference(rt, O, name)["prim"]
        assert (prim == 1).sum() > 0 and (prim == 3).sum() == 0
    if name == "tie_mirror":
        # the pair the renderer scans in the opposite order (see _tie_mirror_scene): equal t on the centre column, the lower caller index has the pixel,
        # and both spheres own pixels elsewhere; x is the axis the slots are sorted on (largest extent, more than 16 small spheres)
        sp = R.sphere_frame(rt, name)[0]
        ext = sp["center"][1:].max(axis=0) - sp["center"][1:].min(axis=0)
        assert len(sp) - 1 > 16 and ext[0] > ext[1] and ext[0] > ext[2] and sp["center"][2][0] < sp["center"][1][0]
        prim = R.reference(rt, O, name)["prim"]
        tied = R.tie_mirror_pixels(rt, O)
        print("tie_mirror: pixels with equal t", tied)
        assert len(tied) >= 2 and all(i == 20 for i, _ in tied)
        assert all(prim[j, i] == 1 for i, j in tied)
        assert (prim == 1).sum() > len(tied) and (prim == 2).sum() > 0


@pytest.mark.parametrize("name", ["staircase_a", "staircase_b"])
def test_reference_covers_staircase(rt, O, name):
    """Every kind the frame puts on a mesh id (textured, plain, presets, the checker among them) on at least one pixel; between the two frames one of each
    preset type, two textures of unequal width and height."""
    c = R.coverage(rt, O, name)
    print(name, c)
    assert c["kinds_seen"] == sorted(R.STAIR_KINDS[name])
    assert "RT_FLOOR_CHECKER" in c["kinds_seen"] and "tex0" in c["kinds_seen"] and "tex1" in c["kinds_seen"]
    presets = {k for kinds in R.STAIR_KINDS.values() for k in kinds if k.startswith("RT_FLOOR") or k.startswith("RT_MODEL")}
    assert presets == {"RT_FLOOR_COAT", "RT_FLOOR_DIFFUSE", "RT_FLOOR_CHECKER", "RT_MODEL_COAT", "RT_MODEL_DIFFUSE", "RT_MODEL_GLOSSY", "RT_MODEL_GLASS",
                       "RT_MODEL_TINTEDGLASS", "RT_MODEL_SSS"}
    assert all(t.shape[0] != t.shape[1] for t in R.stair_textures())
    g = R.reference(rt, O, name)
    f = R.mesh_frame(rt, O, name)
    ids = f["hm"].tris["meshID"][g["prim"]]
    for mid, kind in f["kinds"].items():                        # the checker shows both of its colours, a texture more than one texel
        if kind == "RT_FLOOR_CHECKER" or kind.startswith("tex"):
            assert len(np.unique(g["albedo"][ids == mid], axis=0)) >= 2, kind
    assert c["nodes"][0] >= 1


def test_reference_covers_open_mesh(rt, O):
    """Rays that miss the bounds, rays that miss inside the bounds and hits on at least 5 % of the pixels each; with the floor, floor pixels."""
    c = R.coverage(rt, O, "tris300")
    print(c)
    assert c["bounds_miss"] >= 0.05 and c["inside_miss"] >= 0.05 and c["tri"] >= 0.05
    cf = R.coverage(rt, O, "tris300_floor")
    print(cf)
    assert cf["floor"] >= 0.05 and cf["tri"] == c["tri"]
    g = R.reference(rt, O, "tris300_floor")
    floor = g["prim"] == R.PRIM_FLOOR
    assert np.array_equal(np.unique(g["normal"][floor], axis=0), np.array([[0, 1, 0]], np.float32))
    assert len(np.unique(g["albedo"][floor], axis=0)) == 1
