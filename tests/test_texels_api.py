"""CPU checks of rasterTexels / bakeTexels (include/rt_api.h, "baking texels"): the calls are declared, exported and bound, the device calls before init are
the library's misuse exit, and the CPU twin of the raster (rtRasterTexelsHost, librt_host.so) equals the numpy restatement (tests/texels_reference.py) bit
for bit, every plane, on atlases whose reference planes are first shown to hold the cases they are there for; rtAtlasGrid against numpy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import texels_reference as TR
from preview_support import exits_99, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
HOST = open(os.path.join(ROOT, "include", "rt_host.h")).read()
PLANES = ("prim", "src", "bary", "pos", "nrm")


def _sig(name, ret, args):
    return ret + r"\s+" + name + r"\s*\(\s*" + r"\s*,\s*".join(a.replace(" ", r"\s+").replace("*", r"\s*\*\s*") for a in args) + r"\s*\)\s*;"


def check_planes(got, ref, what):
    owned, planes = got
    assert owned == ref["owned"], (what, owned, ref["owned"])
    for k in planes:
        assert planes[k].shape == ref[k].shape and planes[k].dtype == ref[k].dtype, (what, k)
        same(planes[k], ref[k], f"{what}: {k}")


def test_declared_exported_and_bound(rt):
    raster_args = ["int W", "int H", "int dilate", "int32_t* prim", "int32_t* src", "float* bary", "float* pos", "float* nrm"]
    assert re.search(_sig("rasterTexels", "int", raster_args), API)
    assert re.search(_sig("bakeTexels", "int", ["int W", "int H", "int dilate", "int mode", "int first", "int dirs", "int dirs_total", "int ns", "uint32_t base_id",
                                                "float bias", "float max_dist", "float* acc", "float* out", "uint32_t* rays", "int32_t* prim", "int32_t* src"]), API)
    assert re.search(_sig("rtRasterTexelsHost", "int", ["const rt_triangle* tris", "uint32_t numTris"] + raster_args), HOST)
    assert re.search(_sig("rtAtlasGrid", "int", ["rt_triangle* tris", "int n", "float margin"]), HOST)
    assert re.search(r"double\s+rtLastTexelsMs\s*\(\s*void\s*\)\s*;", API) and re.search(r"double\s+rtLastBakeMs\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"#define RT_TEXEL_MAX_SIZE 8192\b", API) and re.search(r"#define RT_TEXEL_MAX_DILATE 16\b", API)
    assert re.search(r"#define RT_API_VERSION 1002\b", API) and rt.RT_API_VERSION == 1002      # additive: the version stays
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in ("rasterTexels", "bakeTexels", "rtLastTexelsMs", "rtLastBakeMs"):
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    host = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_host.so"))
    for name in ("rtRasterTexelsHost", "rtAtlasGrid"):
        assert hasattr(host, name) and name in rt.HOST_SYMBOLS, name
    r = rt.load_renderer()
    ip, fp, up = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    i, u, f = C.c_int, C.c_uint32, C.c_float
    assert r.rasterTexels.argtypes == [i, i, i, ip, ip, fp, fp, fp] and r.rasterTexels.restype is i
    assert r.bakeTexels.argtypes == [i, i, i, i, i, i, i, i, u, f, f, fp, fp, up, ip, ip] and r.bakeTexels.restype is i
    assert r.rtLastTexelsMs.restype is C.c_double and r.rtLastBakeMs.restype is C.c_double
    for name in ("raster_texels", "bake_texels", "raster_texels_host", "atlas_grid", "last_texels_ms", "last_bake_ms"):
        assert callable(getattr(rt, name)), name
    assert (rt.RT_TEXEL_MAX_SIZE, rt.RT_TEXEL_MAX_DILATE) == (TR.MAX_SIZE, TR.MAX_DILATE) == (8192, 16)
    assert rt.triangle_dtype == TR.TRIANGLE


@pytest.mark.parametrize("call", ["rt.raster_texels(16, 16)", "rt.bake_texels(16, 16, rt.RT_GATHER_VISIBILITY, 4)",
                                  "rt.bake_texels(16, 16, rt.RT_GATHER_IRRADIANCE, 4, dilate=2)", "rt.last_texels_ms()", "rt.last_bake_ms()"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99(call + "\n")


# ---- the raster: the CPU twin against numpy --------------------------------------------------------------------------------------------

def test_exact_edge_hits(rt):
    """(a): the inclusive rule and the lowest-slot ties, on centres that edges and vertices hit exactly."""
    tris, W, H = TR.atlas_exact(TR.random_triangles(12))
    ref = TR.raster(tris, W, H)
    sx, sy = TR.samples(W, H)
    assert (sx.astype(np.float64) * 32 == 2 * np.arange(W) + 1).all() and (sy.astype(np.float64)[:, 0] * 32 == 2 * np.arange(H) + 1).all()     # exact centres
    assert (ref["covers"] >= 2).any(), "no texel has two covering slots"
    assert ref["on_edge"].any(), "no texel lies exactly on an edge"
    assert (ref["prim"] == TR.PRIM_NONE).any(), "no texel is unowned"
    on_diagonal = (np.add.outer(np.arange(H), np.arange(W)) == 8)
    assert (ref["covers"][on_diagonal] >= 2).all() and (ref["prim"][on_diagonal] == 0).all()       # the shared diagonal: both cover it, slot 0 owns it
    assert ref["prim"][2, 10] == 3 and (ref["bary"][2, 10] == 0).all()                            # a vertex exactly on a centre
    assert (ref["prim"][1:4, 1:4] == 0).all() and (ref["covers"][1, 1] == 2)                      # slot 2 lies wholly on slot 0: the lower slot wins
    check_planes(rt.raster_texels_host(tris, W, H), ref, "exact")


def test_odd_sizes_and_bad_triangles(rt):
    """(b): 37 x 23, clipped and outside triangles, d == 0, a NaN UV, a sub-texel triangle between centres, a sentinel slot."""
    tris, W, H = TR.atlas_odd(TR.random_triangles(64))
    ref = TR.raster(tris, W, H)
    tc = tris["texCoords"].reshape(-1, 3, 2)
    sx, sy = TR.samples(W, H)
    per = [int(TR.cover(t["texCoords"], sx, sy)[0].sum()) if not np.isinf(t["v"][0, 0]) else -1 for t in tris]
    live = np.flatnonzero(~np.isinf(tris["v"][:, 0, 0]))
    outside = [(tc[k, :, 0].max() < 0 or tc[k, :, 0].min() > 1 or tc[k, :, 1].max() < 0 or tc[k, :, 1].min() > 1) for k in live[:60]]
    clipped = [per[k] > 0 and (tc[k].min() < 0 or tc[k].max() > 1) for k in live[:60]]
    print("owned", ref["owned"], "of", W * H, "outside", sum(outside), "clipped", sum(clipped), "most covers", int(ref["covers"].max()))
    assert sum(outside) >= 1 and sum(clipped) >= 3
    assert np.isinf(tris["v"][7, 0, 0]) and per[live[11]] == 0 and per[live[23]] == 0 and per[live[37]] == 0
    assert np.isnan(tris["texCoords"][live[23]]).any()
    assert 0 < ref["owned"] < W * H and (ref["covers"] >= 3).any()
    assert not (ref["prim"] == 7).any()
    check_planes(rt.raster_texels_host(tris, W, H), ref, "odd")


@pytest.mark.parametrize("size", [(1, 1), (1, 5)])
def test_smallest_atlases(rt, size):
    tris, W, H = TR.atlas_small(TR.random_triangles(4), *size)
    ref = TR.raster(tris, W, H, dilate=1)
    assert ref["owned"] == W * H and (H == 1 or len(np.unique(ref["prim"])) == 2)
    check_planes(rt.raster_texels_host(tris, W, H, dilate=1), ref, f"{W} x {H}")


@pytest.mark.parametrize("dilate", [0, 1, 3, 16])
def test_dilation(rt, dilate):
    tris, W, H = TR.atlas_odd(TR.random_triangles(64))
    ref = TR.raster(tris, W, H, dilate=dilate)
    owned = ref["prim"] != TR.PRIM_NONE
    assert (ref["src"][owned] == np.flatnonzero(owned.ravel())).all()                               # owned texels keep themselves
    filled = ref["src"] != -1
    assert owned.ravel()[ref["src"][filled]].all()                                                  # every source is an owned texel
    if dilate == 0:
        assert (filled == owned).all() and not owned.all()
    if dilate == 16:
        settle, settled = TR.fill_iterations(tris, W, H)
        print("dilation settles after", settle, "iterations")
        assert 3 < settle <= 16 and filled.all()
        same(ref["src"], settled, "16 iterations against the first count that fills the image")
    check_planes(rt.raster_texels_host(tris, W, H, dilate=dilate), ref, f"dilate {dilate}")


def test_host_twin_writes_only_what_is_asked_and_refuses_quietly(rt):
    tris, W, H = TR.atlas_odd(TR.random_triangles(64))
    ref = TR.raster(tris, W, H, dilate=2)
    for k in PLANES:
        check_planes(rt.raster_texels_host(tris, W, H, dilate=2, want=(k,)), ref, f"{k} alone")
    h = rt.load_host()
    prim = np.full((H, W), 7, np.int32)
    ip = C.POINTER(C.c_int32)
    for args in ((0, H, 0), (W, 0, 0), (8193, H, 0), (W, H, -1), (W, H, 17)):
        assert h.rtRasterTexelsHost(tris.ctypes.data, len(tris), *args, prim.ctypes.data_as(ip), None, None, None, None) == -1
    assert h.rtRasterTexelsHost(tris.ctypes.data, len(tris), W, H, 0, None, None, None, None, None) == -1
    assert (prim == 7).all()
    for bad in (dict(W=0), dict(dilate=17), dict(want=()), dict(want=("depth",))):
        with pytest.raises(ValueError):
            rt.raster_texels_host(tris, **dict(dict(W=W, H=H), **bad))


# ---- rtAtlasGrid -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 7, 300])
def test_atlas_grid_equals_numpy(rt, n):
    tris = TR.random_triangles(n, seed=n)
    ref, cells = TR.atlas_grid(tris, 0.05)
    got = tris.copy()
    assert rt.atlas_grid(got, 0.05) == cells == int(np.ceil(np.sqrt(np.ceil(n / 2))))
    same(got["texCoords"], ref["texCoords"], f"n = {n}")
    assert got["v"].tobytes() == tris["v"].tobytes()                                               # nothing else is touched
    r = TR.raster(ref, 64, 64)
    print("n", n, "cells", cells, "owned", r["owned"], "most covers", int(r["covers"].max()))
    assert r["covers"].max() == 1 and len(np.unique(r["prim"][r["prim"] >= 0])) == n               # no texel is covered twice, every triangle owns some
    check_planes(rt.raster_texels_host(got, 64, 64), r, f"the grid of {n} at 64 x 64")


def test_atlas_grid_refuses(rt):
    tris = TR.random_triangles(4)
    before = tris.copy()
    h = rt.load_host()
    for n, margin in ((0, 0.05), (4, -0.01), (4, 0.25), (4, float("nan"))):
        assert h.rtAtlasGrid(tris.ctypes.data, n, margin) == 0
    assert h.rtAtlasGrid(None, 4, 0.05) == 0
    assert tris.tobytes() == before.tobytes()
    with pytest.raises(ValueError):
        rt.atlas_grid(tris, 0.3)
