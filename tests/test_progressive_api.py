"""CPU checks of the progressive-rendering interface (include/rt_api.h): the four entry points are declared, exported and bound, the ABI version and
struct sizes are those of the parent interface, and the largest accepted total keeps the cost ordering's 32-bit arithmetic exact."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
NEW = ("runRendererProgressive", "rtProgressiveSamples", "rtResetProgressive", "setCamera")


def test_declared_exported_and_bound(rt):
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, API), name
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in NEW:
        assert hasattr(lib, name), name
    r = rt.load_renderer()
    assert all(n in rt.RENDERER_SYMBOLS for n in NEW)
    assert r.runRendererProgressive.argtypes == [C.c_int, C.c_int, C.c_int] and r.runRendererProgressive.restype is None
    assert r.rtProgressiveSamples.restype is C.c_int and r.rtResetProgressive.restype is None
    assert r.setCamera.argtypes == [C.POINTER(rt.camera)]
    for f in (rt.runRendererProgressive, rt.progressive_samples, rt.resetProgressive, rt.setCamera):
        assert callable(f)


def test_abi_unchanged(rt):
    assert rt.load_renderer().rtApiVersion() == 1002 == rt.RT_API_VERSION
    assert re.search(r"#define RT_API_VERSION 1002\b", API)
    sizes = (C.c_int32 * 32)()
    n = rt.load_renderer().rtStructSizes(sizes, 32)
    assert [sizes[k] for k in range(n)] == [C.sizeof(s) for s in rt.ABI_STRUCTS]


def _cost_class_words(rays_per_sample, total):
    """The 32-bit products of k_order_by_cost's cost_class for a 3x3 window of pixels that each spent `rays_per_sample` rays on `total` samples."""
    px = rays_per_sample * total
    return {"px_rays": px, "own": px * 12, "window": 9 * px * 16, "divisor": 9 * total}


@pytest.mark.parametrize("depth", [50, 255])
def test_largest_total_fits_the_ordering_arithmetic(depth):
    """A path takes at most max_depth (<= 255) rays per sample: at RT_PROGRESSIVE_MAX_SAMPLES every product of the ordering pass fits 32 bits; at 2^17
    samples of 255-ray paths the window sum would not (the guard is needed, and the static_assert next to cost_class holds it at build time)."""
    limit = int(re.search(r"#define RT_PROGRESSIVE_MAX_SAMPLES (\d+)", API).group(1))
    assert all(v < 2 ** 32 for v in _cost_class_words(depth, limit).values())
    assert _cost_class_words(255, 2 * limit)["window"] >= 2 ** 32
    src = open(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc", "rt_kernels_spheres.hip")).read()
    assert "static_assert(9ull * 16ull * 255ull * RT_PROGRESSIVE_MAX_SAMPLES <= 0xFFFFFFFFull" in src
    ren = open(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc", "rt_renderer.hip")).read()
    assert "ns > RT_PROGRESSIVE_MAX_SAMPLES - c.prog_samples" in ren
