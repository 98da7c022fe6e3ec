"""CPU checks of filterTexels (include/rt_api.h, "filtering texels"): the calls are declared, exported and bound, the device calls before init are the library's
misuse exit, and the CPU twin (rtFilterTexelsHost, librt_host.so) equals both restatements of tests/texel_filter_reference.py bit for bit, on every texel, on
inputs that the reference alone first shows to hold every reason a tap is dropped or zeroed; what `in` holds at unowned texels has no influence; dilation
changes unowned texels only; and the filter with the header's defaults lowers the error of a noisy synthetic."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import texel_filter_reference as FR
import texels_reference as TR
from preview_support import bits, exits_99, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
HOST = open(os.path.join(ROOT, "include", "rt_host.h")).read()
SHAPES = ("exact", "odd", "1 x 1", "1 x 5", "grid")
FILTER_ARGS = ["int iterations", "int normal_squarings", "float sigma_d", "float sigma_z", "float sigma_c"]


def _sig(name, ret, args):
    return ret + r"\s+" + name + r"\s*\(\s*" + r"\s*,\s*".join(a.replace(" ", r"\s+").replace("*", r"\s*\*\s*") for a in args) + r"\s*\)\s*;"


@functools.lru_cache(maxsize=None)
def atlas(shape):
    """(tris, W, H) of a named shape."""
    if shape == "exact":
        return TR.atlas_exact(TR.random_triangles(12))
    if shape == "odd":
        return TR.atlas_odd(TR.random_triangles(64))
    if shape == "grid":
        return FR.small_mesh(), 24, 16
    W, H = (1, 1) if shape == "1 x 1" else (1, 5)
    return TR.atlas_small(TR.random_triangles(4), W, H)


@functools.lru_cache(maxsize=None)
def raster(shape, dilate):
    tris, W, H = atlas(shape)
    return TR.raster(tris, W, H, dilate)


@functools.lru_cache(maxsize=None)
def plane(shape, C):
    return FR.noisy_plane(raster(shape, 0), C, seed=17 + C)


@pytest.fixture(scope="module")
def inputs():
    """Asserts, on the reference alone, that the shapes hold what they are there for; returns the shapes."""
    total = FR.new_stats()
    for shape in SHAPES:
        tris, W, H = atlas(shape)
        st = FR.new_stats()
        FR.iterate(tris, raster(shape, 0), plane(shape, 3), 8, 5, 2.0, 2.0, 0.5, stats=st)
        print(shape, st)
        for k in st:
            total[k] += st[k]
        if shape == "grid":
            f2 = FR.footprint(tris, raster(shape, 0), 2.0, 2.0)[0][raster(shape, 0)["prim"] != TR.PRIM_NONE]
            print("grid: f2 == 0 at", int((f2 == 0).sum()), "inf at", int(np.isinf(f2).sum()), "of", f2.size, "owned texels")
            assert (f2 == 0).any() and np.isinf(f2).any(), "no degenerate footprint"
            assert st["reach_other_cell"] > 0, "the reach test never separates two grid cells"
            assert st["wn0"] > 0 and st["wz0"] > 0
    for k in ("outside", "unowned", "reach", "wn0", "wz0", "wc0", "accepted"):
        assert total[k] > 0, k
    return SHAPES


def test_declared_exported_and_bound(rt):
    assert re.search(_sig("filterTexels", "int", ["int W", "int H", "int dilate", "int mode", "const float* in", "float* out"] + FILTER_ARGS), API)
    assert re.search(r"double\s+rtLastFilterMs\s*\(\s*void\s*\)\s*;", API)
    assert re.search(_sig("rtFilterTexelsHost", "int", ["const rt_triangle* tris", "uint32_t numTris", "int W", "int H", "int dilate", "int mode",
                                                        "const float* in", "float* out"] + FILTER_ARGS), HOST)
    assert re.search(r"#define RT_API_VERSION 1002\b", API) and rt.RT_API_VERSION == 1002          # additive: the version stays
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in ("filterTexels", "rtLastFilterMs"):
        assert hasattr(lib, name) and name in rt.RENDERER_SYMBOLS, name
    host = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_host.so"))
    assert hasattr(host, "rtFilterTexelsHost") and "rtFilterTexelsHost" in rt.HOST_SYMBOLS
    r = rt.load_renderer()
    fp, i, f = C.POINTER(C.c_float), C.c_int, C.c_float
    assert r.filterTexels.argtypes == [i, i, i, i, fp, fp, i, i, f, f, f] and r.filterTexels.restype is i
    assert r.rtLastFilterMs.restype is C.c_double
    for name in ("filter_texels", "filter_texels_host", "last_filter_ms"):
        assert callable(getattr(rt, name)), name
    # the defaults: the header's, the mirror's and the reference's are one set
    d = FR.DEFAULTS
    for macro, key, mirror in (("ITERATIONS", "iterations", rt.RT_FILTER_ITERATIONS), ("SQUARINGS", "normal_squarings", rt.RT_FILTER_SQUARINGS),
                               ("SIGMA_D", "sigma_d", rt.RT_FILTER_SIGMA_D), ("SIGMA_Z", "sigma_z", rt.RT_FILTER_SIGMA_Z),
                               ("SIGMA_C", "sigma_c", rt.RT_FILTER_SIGMA_C)):
        m = re.search(r"#define RT_FILTER_%s\s+([0-9.]+)f?\b" % macro, API)
        assert m and float(m.group(1)) == d[key] == mirror, macro
    assert (FR.MAX_ITERATIONS, FR.MAX_SQUARINGS) == (rt.RT_DENOISE_MAX_ITERATIONS, rt.RT_DENOISE_MAX_SQUARINGS)
    assert FR.WIDTH == {rt.RT_GATHER_IRRADIANCE: 3, rt.RT_GATHER_SH9: 27, rt.RT_GATHER_VISIBILITY: 1}


@pytest.mark.parametrize("call", ["rt.filter_texels(16, 16, rt.RT_GATHER_IRRADIANCE, np.zeros((16, 16, 3), np.float32))",
                                  "rt.filter_texels(16, 16, rt.RT_GATHER_VISIBILITY, None, dilate=2)", "rt.last_filter_ms()"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99(call + "\n")


# ---- the twin against the two restatements -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C_", [1, 3, 27])
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_equals_both_restatements(rt, inputs, shape, C_):
    """Iterations 1, 4 and 8 (stride 128 is far beyond every atlas), squarings 0 and 5, sigma_c 0 and 0.5, dilate 0 and 3: every texel, bit for bit."""
    tris, W, H = atlas(shape)
    src, mode = plane(shape, C_), FR.MODE_OF[C_]
    for squarings in (0, 5):
        for sigma_c in (0.0, 0.5):
            kw = dict(normal_squarings=squarings, sigma_d=2.0, sigma_z=2.0, sigma_c=sigma_c)
            steps = FR.iterate(tris, raster(shape, 0), src, 8, **kw)
            scalar = FR.iterate_scalar(tris, raster(shape, 0), src, 8, **kw)
            for iterations in (1, 4, 8):
                what = f"{shape} C {C_} squarings {squarings} sigma_c {sigma_c} iterations {iterations}"
                same(scalar[iterations - 1], steps[iterations - 1], what + ": the scalar restatement against numpy")
                for dilate in (0, 3):
                    ras = raster(shape, dilate)
                    owned, out = rt.filter_texels_host(tris, W, H, mode, src, dilate=dilate, iterations=iterations, **kw)
                    assert owned == ras["owned"]
                    same(out, FR.scatter(steps[iterations - 1], ras["src"]), what + f" dilate {dilate}: the twin against numpy")
            assert shape != "grid" or (bits(steps[0]) != bits(steps[7])).any()                     # (the later iterations do something)


@pytest.mark.parametrize("shape", ["odd", "grid"])
def test_unowned_input_has_no_influence(rt, inputs, shape):
    tris, W, H = atlas(shape)
    ras = raster(shape, 3)
    clean = plane(shape, 3)
    dirty = clean.copy()
    dirty[ras["prim"] == TR.PRIM_NONE] = np.nan
    assert np.isnan(dirty).any() and np.isfinite(clean).all()
    a = rt.filter_texels_host(tris, W, H, FR.MODE_OF[3], clean, dilate=3)[1]
    b = rt.filter_texels_host(tris, W, H, FR.MODE_OF[3], dirty, dilate=3)[1]
    same(b, a, f"{shape}: NaN at every unowned texel of in")
    assert not np.isnan(b).any()
    same(FR.filter_numpy(tris, W, H, 3, dirty, **FR.DEFAULTS)[1], a, f"{shape}: numpy, the same")


@pytest.mark.parametrize("shape", ["odd", "grid"])
def test_dilate_changes_unowned_texels_only(rt, inputs, shape):
    tris, W, H = atlas(shape)
    owned = raster(shape, 0)["prim"] != TR.PRIM_NONE
    a = rt.filter_texels_host(tris, W, H, FR.MODE_OF[3], plane(shape, 3), dilate=0)[1]
    b = rt.filter_texels_host(tris, W, H, FR.MODE_OF[3], plane(shape, 3), dilate=3)[1]
    same(b[owned], a[owned], f"{shape}: owned texels under dilate 0 and 3")
    assert (a[~owned] == 0).all() and (b[~owned] != 0).any()
    filled = raster(shape, 3)["src"] != -1
    assert (b[~filled] == 0).all() and (filled & ~owned).any()


def test_out_may_be_in_and_the_twin_refuses_quietly(rt, inputs):
    tris, W, H = atlas("odd")
    src = plane("odd", 3)
    ref = rt.filter_texels_host(tris, W, H, FR.MODE_OF[3], src)[1]
    buf = src.copy()
    owned, out = rt.filter_texels_host(tris, W, H, FR.MODE_OF[3], buf, out=buf)
    assert out is buf
    same(buf, ref, "out is in")
    h = rt.load_host()
    fp = C.POINTER(C.c_float)
    keep = np.full((H, W, 3), 7, np.float32)
    good = dict(W=W, H=H, dilate=0, mode=0, iterations=4, squarings=5, sd=2.0, sz=2.0, sc=1.0)
    call = lambda a, inp=src: h.rtFilterTexelsHost(tris.ctypes.data, len(tris), a["W"], a["H"], a["dilate"], a["mode"], None if inp is None else
                                                   inp.ctypes.data_as(fp), keep.ctypes.data_as(fp), a["iterations"], a["squarings"], a["sd"], a["sz"], a["sc"])
    for bad in (dict(W=0), dict(H=8193), dict(dilate=17), dict(mode=3), dict(iterations=0), dict(iterations=9), dict(squarings=-1), dict(squarings=8),
                dict(sd=0.0), dict(sd=float("nan")), dict(sz=-1.0), dict(sz=float("inf")), dict(sc=float("nan")), dict(sc=float("inf"))):
        assert call(dict(good, **bad)) == -1, bad
    assert call(good, None) == -1
    assert (keep == 7).all()
    assert call(dict(good, sc=-1.0)) == raster("odd", 0)["owned"]                                  # a negative sigma_c is the colour weight switched off
    same(keep, rt.filter_texels_host(tris, W, H, 0, src, iterations=4, sigma_c=0.0)[1], "sigma_c < 0 against sigma_c == 0")
    for bad in (dict(mode=5), dict(W=0), dict(plane=src[:, :, :1]), dict(iterations=9)):
        with pytest.raises(ValueError):
            rt.filter_texels_host(tris, **dict(dict(W=W, H=H, mode=0, plane=src), **bad))


def test_defaults_lower_the_error_of_a_noisy_synthetic(inputs):
    """From the reference alone: Lambert shading of pos / nrm under a point light plus seeded noise on the grid atlas of the small mesh at 64 x 64."""
    tris = FR.small_mesh(degenerate=False)
    ras = TR.raster(tris, 64, 64)
    owned = ras["prim"] != TR.PRIM_NONE
    clean = FR.lambert(ras)
    noisy = (clean + np.random.default_rng(5).normal(0.0, 0.15, clean.shape).astype(np.float32)).astype(np.float32)
    got = FR.filter_numpy(tris, 64, 64, 0, noisy, ras=ras, **FR.DEFAULTS)[1]
    rmse = lambda a: float(np.sqrt(np.mean((a[owned].astype(np.float64) - clean[owned]) ** 2)))
    ratio = rmse(got) / rmse(noisy)
    print(f"owned {int(owned.sum())} of 4096, RMSE noisy {rmse(noisy):.5f}, filtered {rmse(got):.5f}, ratio {ratio:.4f}")
    assert np.isfinite(clean).all() and ratio < 1.0
