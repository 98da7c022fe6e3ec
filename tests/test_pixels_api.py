"""CPU checks of renderPixels (include/rt_api.h): renderPixels / rtLastPixelsMs are declared, exported and bound with their argument types, the constants
agree between header and Python, the ABI version and struct sizes are the parent's, both calls before init are the library's misuse exit, and the test
reference (tests/pixels_reference.py) shows on the standard lists of the GPU tests what they are there to cover - conditions on the inputs, no tolerance: a
seed that misses one is changed, never the threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pixels_reference as PR
from preview_support import bits, exits_99

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
NEW = ("renderPixels", "rtLastPixelsMs")


def test_declared_exported_and_bound(rt):
    assert re.search(r"void\s+renderPixels\s*\(\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*ij\s*,\s*int\s+ns_all\s*,\s*const\s+int32_t\s*\*\s*ns\s*,"
                     r"\s*const\s+int32_t\s*\*\s*first\s*,\s*uint32_t\s*\*\s*state\s*,\s*rt_vec3\s*\*\s*out\s*,\s*uint32_t\s*\*\s*rays\s*\)\s*;", API)
    assert re.search(r"double\s+rtLastPixelsMs\s*\(\s*void\s*\)\s*;", API)
    assert API.index("double rtLastRaysMs") < API.index("renderPixels(int n") < API.index("--- editing the scene")       # the section's place
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    r = rt.load_renderer()
    ip, up = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    assert r.renderPixels.argtypes == [C.c_int, ip, C.c_int, ip, ip, up, C.POINTER(rt.vec3), up] and r.renderPixels.restype is None
    assert r.rtLastPixelsMs.argtypes == [] and r.rtLastPixelsMs.restype is C.c_double
    for name in ("render_pixels", "render_region", "last_pixels_ms"):
        assert callable(getattr(rt, name)), name


def test_constants_agree_between_header_and_python(rt):
    assert re.search(r"^#define RT_PIXEL_CHUNK \(1 << 22\)$", API, re.M) and rt.RT_PIXEL_CHUNK == 1 << 22
    assert int(re.search(r"^#define RT_PROGRESSIVE_MAX_SAMPLES (\d+)$", API, re.M).group(1)) == rt.RT_PROGRESSIVE_MAX_SAMPLES == 65536


def test_abi_unchanged(rt):
    assert rt.load_renderer().rtApiVersion() == 1002 == rt.RT_API_VERSION
    assert re.search(r"#define RT_API_VERSION 1002\b", API)
    sizes = (C.c_int32 * 32)()
    n = rt.load_renderer().rtStructSizes(sizes, 32)
    assert n == 13 and [sizes[k] for k in range(n)] == [C.sizeof(s) for s in rt.ABI_STRUCTS]


@pytest.mark.parametrize("call", ["rt.render_pixels(np.zeros((4, 2), np.int32), 2)", "rt.render_region(0, 0, 2, 2, 1)", "rt.last_pixels_ms()",
                                  "rt.render_pixels(np.zeros((0, 2), np.int32), 2)"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99(call + "\n")


def test_wrong_shapes_are_value_errors(rt):
    ij = np.zeros((4, 2), np.int32)
    for bad in (np.zeros((4, 3), np.int32), np.zeros(8, np.int32)):
        with pytest.raises(ValueError):
            rt.render_pixels(bad, 2)
    with pytest.raises(ValueError):
        rt.render_pixels(ij, np.ones(3, np.int32))
    with pytest.raises(ValueError):
        rt.render_pixels(ij, 2, first=np.ones(4, np.int32))                                 # first without state
    with pytest.raises(ValueError):
        rt.render_pixels(ij, 2, first=np.ones(4, np.int32), state=np.zeros((3, 4), np.uint32))
    with pytest.raises(ValueError):
        rt.render_region(3, 0, 2, 2, 1)


# ---- the standard lists: conditions, from the reference alone ----------------------------------------------------------------------

@pytest.mark.parametrize("tag", sorted(PR.SCENES))
def test_standard_list_is_every_pixel_once_plus_duplicates(tag):
    nx, ny, _ = PR.SCENES[tag]
    ij, first = PR.standard_list(tag)
    assert ij.dtype == np.int32 and ij.shape == (nx * ny + 37, 2) and len(ij) % 64 != 0
    ids = ij[:, 1].astype(np.int64) * nx + ij[:, 0]
    assert set(ids.tolist()) == set(range(nx * ny)) and int(first.sum()) == nx * ny
    assert np.array_equal(np.sort(ids[first]), np.arange(nx * ny))
    assert 0 in ids and nx * ny - 1 in ids                                                  # both corners
    assert not np.array_equal(ids[first], np.arange(nx * ny))                               # shuffled
    assert (~first[: len(ij) // 2]).any() and (~first[len(ij) // 2:]).any()                # duplicates in both halves of the list
    if tag == "S2":
        assert len(ij) == 3109


def test_costs_in_one_list_span_a_factor_of_8(rt, O):
    """Per-pixel oracle rays at 4 spp on S2: 4 (one ray per sample) to 98, median 8 - the ragged cost the queue is there to absorb."""
    _, rays = PR.oracle_planes(rt, O, "S2", 4)
    print("S2 rays per pixel at 4 spp: min", int(rays.min()), "max", int(rays.max()), "median", float(np.median(rays)))
    assert int(rays.max()) >= 8 * int(rays.min()) and int(rays.min()) >= 4


@pytest.mark.parametrize("tag,ns,total", [("S2", 4, 28561), ("M1", 3, 19219), ("M2_floor", 3, 12274)])
def test_per_pixel_rays_add_up_to_the_frames(rt, O, tag, ns, total):
    """The per-pixel `rays` of the region renders add up to the whole frame's orc_counters.rays, and the per-pixel colours are the frame's."""
    col, rays = PR.oracle_planes(rt, O, tag, ns)
    fb, cnt = PR.oracle_frame(rt, O, tag, ns)
    assert int(rays.sum(dtype=np.uint64)) == int(cnt.rays) == total
    assert np.array_equal(bits(col), bits(fb))


@pytest.mark.parametrize("tag", ["S2", "M1"])
def test_three_and_seven_samples_differ(rt, O, tag):
    """Without this a continuation test proves nothing: the colours of 3 and of 7 samples differ at more than half of the pixels."""
    a, _ = PR.oracle_planes(rt, O, tag, 3)
    b, _ = PR.oracle_planes(rt, O, tag, 7)
    share = float((bits(a) != bits(b)).any(axis=2).mean())
    print(tag, "share of pixels whose 3- and 7-sample colours differ", share)
    assert share > 0.5


def test_variants_change_the_frame_they_vary(rt, O):
    """The textured material changes M1, and the floor plane changes the frame of M2_floor: measured 1254 of 1536 pixels, and the share printed.  (The staircase
    is a closed room: no ray of M1_floor reaches a plane below it, so that variant runs the floor's test on every ray that leaves the mesh and never its
    scatter; M2_floor is there for the scatter.)"""
    base, _ = PR.oracle_planes(rt, O, "M1", 3)
    tex, _ = PR.oracle_planes(rt, O, "M1_tex", 3)
    assert int((bits(tex) != bits(base)).any(axis=2).sum()) > 500
    s = PR.scene(rt, "M2_floor")
    opt = O.default_options(False)
    off, _ = O.render(O.mesh_scene(s["hm"], s["mats"], s["tex"], s["floor"]), s["cam"], opt, s["nx"], s["ny"], 3, s["depth"])
    on, _ = PR.oracle_frame(rt, O, "M2_floor", 3)
    share = float((bits(on) != bits(off)).any(axis=2).mean())
    print("M2_floor: share of pixels the floor plane changes", share)
    assert share > 0.25
