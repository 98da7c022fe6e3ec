"""CPU checks of sampleTexels / renderLightmap (include/rt_api.h, "sampling texels"): the calls are declared, exported and bound, the device calls before
init are the library's misuse exit, and the CPU twin (rtSampleTexelsHost, librt_host.so) equals the numpy restatement of tests/lightmap_reference.py bit for
bit on hit lists that the reference alone first shows to hold every edge the definition names; a nearest lookup at the raster's own (prim, bary) of every
owned texel returns that texel; and the SH9 constants reproduce two analytic values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lightmap_reference as LR
import texels_reference as TR
from preview_support import exits_99, same
from texels_support import private_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
HOST = open(os.path.join(ROOT, "include", "rt_host.h")).read()
SHAPES = ("1 x 1", "1 x 5", "exact", "grid")
F = np.float32


def _sig(name, ret, args):
    return ret + r"\s+" + name + r"\s*\(\s*" + r"\s*,\s*".join(a.replace(" ", r"\s+").replace("*", r"\s*\*\s*").replace("[", r"\[").replace("]", r"\]")
                                                               for a in args) + r"\s*\)\s*;"


@pytest.fixture(scope="module")
def atlases(rt, tmp_path_factory):
    """name -> (tris with a sentinel slot, W, H): 1 x 1, 1 x 5, the 16 x 16 exact atlas, and 37 x 23 on the rtAtlasGrid atlas of M1."""
    out = {}
    for shape in SHAPES:
        if shape == "exact":
            tris, W, H = TR.atlas_exact(TR.random_triangles(12))
        elif shape == "grid":
            tris, W, H = private_mesh(rt, "M1", tmp_path_factory.mktemp("lightmap")).tris.copy(), 37, 23
        else:
            tris, W, H = TR.atlas_small(TR.random_triangles(4), *((1, 1) if shape == "1 x 1" else (1, 5)))
        out[shape] = (LR.with_dead_slot(tris)[0], W, H)
    return out


@pytest.fixture(scope="module")
def inputs(atlases):
    """Asserts, on the reference alone, that the hit lists hold what they are there for; returns name -> (prim, uv, normal)."""
    hits, seen = {}, dict(left=0, right=0, bottom=0, top=0, ax0=0, outside=0, nan_uv=0, none=0, floor=0, past=0, dead=0, sh_clamped=0, valid=0)
    for i, shape in enumerate(SHAPES):
        tris, W, H = atlases[shape]
        prim, uv, nrm = hits[shape] = LR.edge_hits(tris, 40 + i)
        d = {}
        out, ok = LR.lookup(tris, prim, uv, nrm, W, H, LR.SH9, LR.random_planes(W, H, 27, 7), True, details=d)
        v = ok == 1
        frac = v & (d["ax"] > 0) & (d["ay"] > 0)                       # (a clamped tap with a weight that counts)
        seen["left"] += int((frac & (d["kx"] < 0)).sum()); seen["right"] += int((frac & (d["kx"] + 1 > W - 1)).sum())
        seen["bottom"] += int((frac & (d["ky"] < 0)).sum()); seen["top"] += int((frac & (d["ky"] + 1 > H - 1)).sum())
        seen["ax0"] += int((v & (d["ax"] == 0) & (d["kx"] >= 0) & (d["kx"] < W) & np.isfinite(d["tcu"])).sum())
        seen["outside"] += int((v & ((uv < 0) | (uv > 1)).any(axis=1)).sum())
        seen["nan_uv"] += int((v & np.isnan(uv).any(axis=1)).sum())
        seen["none"] += int((prim == LR.PRIM_NONE).sum()); seen["floor"] += int((prim == LR.PRIM_FLOOR).sum())
        seen["past"] += int((prim >= len(tris)).sum())
        seen["dead"] += int(((prim >= 0) & (prim < len(tris)) & ~v).sum())
        seen["sh_clamped"] += int((v & (d["raw"] < 0).any(axis=1) & (out == 0).any(axis=1)).sum())
        seen["valid"] += int(v.sum())
        assert (out[~v] == 0).all() and np.isfinite(out).all(), shape
    print(seen)
    for k, n in seen.items():
        assert n > 0, k
    return hits


def test_declared_exported_and_bound(rt):
    assert re.search(_sig("sampleTexels", "int", ["int n", "const int32_t* prim", "const float* uv", "const float* normal", "int W", "int H", "int mode",
                                                  "const float* planes", "int flags", "float* out", "uint8_t* valid"]), API)
    assert re.search(_sig("renderLightmap", "void", ["int W", "int H", "int mode", "const float* planes", "int flags", "const float floor_value[3]",
                                                     "rt_vec3* out"]), API)
    assert re.search(r"double\s+rtLastSampleMs\s*\(\s*void\s*\)\s*;", API) and re.search(r"double\s+rtLastLightmapMs\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"enum\s*\{\s*RT_SAMPLE_BILINEAR\s*=\s*1\s*,\s*RT_LIGHTMAP_ALBEDO\s*=\s*2\s*,\s*RT_TEXELS_FROM_BAKE\s*=\s*4\s*,\s*RT_TEXELS_FROM_FILTER\s*=\s*8\s*\}", API)
    assert re.search(_sig("rtSampleTexelsHost", "int", ["const rt_triangle* tris", "uint32_t numTris", "int n", "const int32_t* prim", "const float* uv",
                                                        "const float* normal", "int W", "int H", "int mode", "const float* planes", "int flags", "float* out",
                                                        "uint8_t* valid"]), HOST)
    assert re.search(r"#define RT_API_VERSION 1002\b", API) and rt.RT_API_VERSION == 1002          # additive: the version stays
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in ("sampleTexels", "renderLightmap", "rtLastSampleMs", "rtLastLightmapMs"):
        assert hasattr(lib, name) and name in rt.RENDERER_SYMBOLS, name
    host = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_host.so"))
    assert hasattr(host, "rtSampleTexelsHost") and "rtSampleTexelsHost" in rt.HOST_SYMBOLS
    r = rt.load_renderer()
    fp, ip, bp, i = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_int
    assert r.sampleTexels.argtypes == [i, ip, fp, fp, i, i, i, fp, i, fp, bp] and r.sampleTexels.restype is i
    assert r.renderLightmap.argtypes == [i, i, i, fp, i, fp, C.POINTER(rt.vec3)] and r.renderLightmap.restype is None
    assert r.rtLastSampleMs.restype is C.c_double and r.rtLastLightmapMs.restype is C.c_double
    for name in ("sample_texels", "sample_texels_host", "render_lightmap", "last_sample_ms", "last_lightmap_ms"):
        assert callable(getattr(rt, name)), name
    assert (rt.RT_SAMPLE_BILINEAR, rt.RT_LIGHTMAP_ALBEDO, rt.RT_TEXELS_FROM_BAKE, rt.RT_TEXELS_FROM_FILTER) == (LR.BILINEAR, LR.ALBEDO, LR.FROM_BAKE,
                                                                                                                 LR.FROM_FILTER) == (1, 2, 4, 8)
    assert LR.WIDTH == {rt.RT_GATHER_IRRADIANCE: 3, rt.RT_GATHER_SH9: 27, rt.RT_GATHER_VISIBILITY: 1}


@pytest.mark.parametrize("call", ["rt.sample_texels([0], [[0.2, 0.2]], None, 8, 8, rt.RT_GATHER_IRRADIANCE, np.zeros((8, 8, 3), np.float32))",
                                  "rt.sample_texels([0], [[0.2, 0.2]], None, 8, 8, rt.RT_GATHER_VISIBILITY, None, rt.RT_TEXELS_FROM_BAKE)",
                                  "rt.render_lightmap(8, 8, rt.RT_GATHER_IRRADIANCE, np.zeros((8, 8, 3), np.float32))",
                                  "rt.render_lightmap(8, 8, rt.RT_GATHER_SH9, None, rt.RT_TEXELS_FROM_FILTER | rt.RT_LIGHTMAP_ALBEDO)",
                                  "rt.last_sample_ms()", "rt.last_lightmap_ms()"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99(call + "\n")


# ---- the twin against the restatement ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("C_", [1, 3, 27])
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_equals_numpy(rt, atlases, inputs, shape, C_, bilinear):
    tris, W, H = atlases[shape]
    prim, uv, nrm = inputs[shape]
    planes = LR.random_planes(W, H, C_, 11 + C_)
    ref, ok = LR.lookup(tris, prim, uv, nrm, W, H, LR.MODE_OF[C_], planes, bilinear)
    count, out, valid = rt.sample_texels_host(tris, prim, uv, nrm if C_ == 27 else None, W, H, LR.MODE_OF[C_], planes, LR.BILINEAR if bilinear else 0)
    what = f"{shape} C {C_} {'bilinear' if bilinear else 'nearest'}"
    assert count == int(ok.sum()) and np.array_equal(valid, ok), what
    same(out, ref, what + ": the twin against numpy")
    assert 0 < count < len(prim) and (out[ok == 1] != 0).any()


@pytest.mark.parametrize("shape", ["exact", "grid"])
def test_nearest_at_the_rasters_own_points_returns_the_texel(rt, atlases, shape):
    """Planes that hold the texel index: the lookup inverts the raster at every owned texel - the reference first, then the twin."""
    tris, W, H = atlases[shape]
    ras = TR.raster(tris, W, H)
    owned = ras["prim"] != TR.PRIM_NONE
    t = np.flatnonzero(owned.ravel())
    prim, bary = ras["prim"].ravel()[t], ras["bary"].reshape(-1, 2)[t]
    assert len(t) == ras["owned"] > 0
    for C_ in (1, 3):
        planes = LR.index_planes(W, H, C_)
        want = np.repeat(t.astype(F)[:, None], 3, axis=1)
        ref, ok = LR.lookup(tris, prim, bary, None, W, H, LR.MODE_OF[C_], planes, False)
        assert (ok == 1).all() and np.array_equal(ref, want), (shape, C_, int((ref != want).any(axis=1).sum()))
        count, out, valid = rt.sample_texels_host(tris, prim, bary, None, W, H, LR.MODE_OF[C_], planes)
        assert count == len(t) and (valid == 1).all()
        same(out, want, f"{shape} C {C_}: the twin returns the texel")


def test_sh9_constants_reproduce_two_analytic_values(rt):
    """From the constants of the definition: a constant radiance of 1 / (0.282095 * ...) gives 1; L(w) = max(w.z, 0) gives 0.661458 at n = (0, 0, 1)."""
    tris = TR.atlas_small(TR.random_triangles(4), 1, 1)[0]
    one = np.zeros((1, 1, 27), F)
    one[0, 0, 0:3] = 3.544908
    lobe = np.zeros((1, 1, 27), F)
    lobe[0, 0, 0:3], lobe[0, 0, 6:9], lobe[0, 0, 18:21] = 0.886227, 1.023327, 0.495416
    slot = int(TR.live_slots(tris)[0])
    prim, uv = np.array([slot, slot], np.int32), np.array([[0.2, 0.2], [0.3, 0.1]], F)
    nrm = np.array([[0.6, 0.0, 0.8], [0.0, 0.0, 1.0]], F)
    for bilinear in (False, True):
        a = LR.lookup(tris, prim, uv, nrm, 1, 1, LR.SH9, one, bilinear)[0]
        b = LR.lookup(tris, prim, uv, nrm, 1, 1, LR.SH9, lobe, bilinear)[0]
        print(a, b)
        assert np.abs(a - 1.0).max() <= 1e-5 and np.abs(b[1] - 0.661458).max() <= 1e-4
        same(rt.sample_texels_host(tris, prim, uv, nrm, 1, 1, LR.SH9, one, int(bilinear))[1], a, "constant radiance: the twin")
        same(rt.sample_texels_host(tris, prim, uv, nrm, 1, 1, LR.SH9, lobe, int(bilinear))[1], b, "clamped cosine: the twin")


def test_the_twin_refuses_quietly(rt, atlases, inputs):
    tris, W, H = atlases["exact"]
    prim, uv, nrm = inputs["exact"]
    h = rt.load_host()
    fp, ip, bp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    planes = LR.random_planes(W, H, 27, 3)
    keep, kv = np.full((len(prim), 3), 7, F), np.full(len(prim), 7, np.uint8)
    good = dict(n=len(prim), prim=prim, uv=uv, nrm=nrm, W=W, H=H, mode=1, planes=planes, flags=1, out=keep)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    call = lambda a: h.rtSampleTexelsHost(tris.ctypes.data, len(tris), a["n"], ptr(a["prim"], ip), ptr(a["uv"], fp), ptr(a["nrm"], fp), a["W"], a["H"],
                                          a["mode"], ptr(a["planes"], fp), a["flags"], ptr(a["out"], fp), ptr(kv, bp))
    for bad in (dict(n=-1), dict(prim=None), dict(uv=None), dict(out=None), dict(nrm=None), dict(W=0), dict(H=8193), dict(mode=3), dict(mode=-1),
                dict(flags=2), dict(flags=4), dict(flags=16), dict(planes=None), dict(planes=None, flags=4)):
        assert call(dict(good, **bad)) == -1, bad
    assert (keep == 7).all() and (kv == 7).all()
    assert call(dict(good, n=0)) == 0 and (keep == 7).all()
    assert call(dict(good, mode=0, nrm=None)) > 0                                                  # only SH9 reads the normals
    for bad in (dict(mode=5), dict(W=0), dict(planes=planes[:, :, :3]), dict(planes=None), dict(flags=2), dict(uv=uv[:, :1])):
        with pytest.raises(ValueError):
            a = dict(dict(prim=prim, uv=uv, normal=nrm, W=W, H=H, mode=1, planes=planes, flags=0), **bad)
            rt.sample_texels_host(tris, a["prim"], a["uv"], a["normal"], a["W"], a["H"], a["mode"], a["planes"], a["flags"])
