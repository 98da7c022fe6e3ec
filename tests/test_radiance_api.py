"""CPU checks of radianceRays (include/rt_api.h): the calls are declared, exported and bound, rtPinholeCamera (include/rt_host.h) is the camera the
definition speaks of - under it the oracle's get_ray returns the caller's ray bit for bit -, the calls before init are the library's misuse exit, and the test
reference (tests/radiance_reference.py) shows on the standard lists of the GPU tests what they are there to cover.  Those are conditions on the inputs - caps,
not measurements: a construction that misses one is changed, never the cap."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pixels_reference as PR
import radiance_reference as RR
from preview_support import bits, exits_99, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
HOST = open(os.path.join(ROOT, "include", "rt_host.h")).read()
TAGS = sorted(RR.LIST_SEED)


def _cam_words(cam):
    return bytes(cam)


def test_declared_exported_and_bound(rt):
    assert re.search(r"void\s+radianceRays\s*\(\s*int\s+n\s*,\s*const\s+float\s*\*\s*org\s*,\s*const\s+float\s*\*\s*dir\s*,\s*const\s+uint32_t\s*\*\s*ids\s*,"
                     r"\s*int\s+ns_all\s*,\s*const\s+int32_t\s*\*\s*ns\s*,\s*const\s+int32_t\s*\*\s*first\s*,\s*uint32_t\s*\*\s*state\s*,"
                     r"\s*rt_vec3\s*\*\s*out\s*,\s*uint32_t\s*\*\s*rays\s*\)\s*;", API)
    assert re.search(r"double\s+rtLastRadianceMs\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"void\s+rtPinholeCamera\s*\(\s*const\s+float\s+o\s*\[3\]\s*,\s*const\s+float\s+target\s*\[3\]\s*,\s*rt_camera\s*\*\s*out\s*\)\s*;", HOST)
    assert HOST.index("void rtCentreRays") < HOST.index("void rtPinholeCamera")                 # beside rtCentreRays
    assert re.search(r"#define RT_API_VERSION 1002\b", API) and rt.RT_API_VERSION == 1002      # additive: the version stays
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in ("radianceRays", "rtLastRadianceMs"):
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    assert hasattr(C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_host.so")), "rtPinholeCamera")
    assert "rtPinholeCamera" in rt.HOST_SYMBOLS
    r = rt.load_renderer()
    fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    assert r.radianceRays.argtypes == [C.c_int, fp, fp, up, C.c_int, ip, ip, up, C.POINTER(rt.vec3), up] and r.radianceRays.restype is None
    assert r.rtLastRadianceMs.argtypes == [] and r.rtLastRadianceMs.restype is C.c_double
    for name in ("radiance_rays", "last_radiance_ms", "pinhole_camera"):
        assert callable(getattr(rt, name)), name


def test_pinhole_camera_is_the_python_construction(rt):
    rng = np.random.default_rng(1)
    for _ in range(50):
        o, T = rng.uniform(-50, 50, 3).astype(np.float32), rng.uniform(-50, 50, 3).astype(np.float32)
        cam = rt.pinhole_camera(o, T)
        assert _cam_words(cam) == _cam_words(RR.pinhole(o, T))
        assert list(cam.origin.e) == o.tolist() and list(cam.lower_left_corner.e) == T.tolist()
        for f in ("horizontal", "vertical", "u", "v", "w"):
            assert list(getattr(cam, f).e) == [0.0, 0.0, 0.0]
        assert cam.lens_radius == 0.0
    with pytest.raises(ValueError):
        rt.pinhole_camera(np.zeros(2), np.zeros(3))


def test_the_pinhole_returns_the_callers_ray(rt, O):
    """get_ray of the oracle (camera.h:8-12) under the pinhole at o towards T, at a random jitter and stream word: origin o and direction unit(fl(T - o)), bit
    for bit, on 20 000 random pairs - a quarter with one coordinate of T equal to o's (an axis-parallel component), a tenth with a zero origin."""
    lib = O.load_oracle()
    rng = np.random.default_rng(7)
    n = 20000
    o = rng.uniform(-100, 100, (n, 3)).astype(np.float32)
    T = (o + rng.uniform(-30, 30, (n, 3))).astype(np.float32)
    o[rng.random(n) < 0.1] = 0.0
    equal = rng.random(n) < 0.25
    axis = rng.integers(0, 3, n)
    T[equal, axis[equal]] = o[equal, axis[equal]]
    two = rng.random(n) < 0.05                              # two equal coordinates: the ray runs along an axis
    T[two, (axis[two] + 1) % 3] = o[two, (axis[two] + 1) % 3]
    T[two, (axis[two] + 2) % 3] = o[two, (axis[two] + 2) % 3]
    keep = (T != o).any(axis=1)
    o, T = o[keep] + np.float32(0), T[keep] + np.float32(0)
    d = T - o
    assert not np.signbit(d[d == 0]).any() and ((d == 0).sum(axis=1) == 1).sum() > 3000 and ((d == 0).sum(axis=1) == 2).sum() > 500
    length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    assert length.dtype == np.float32
    dn = d / length[:, None]
    s, t = rng.uniform(0, 1, len(o)).astype(np.float32), rng.uniform(0, 1, len(o)).astype(np.float32)
    words = rng.integers(1, 2 ** 32, len(o), dtype=np.uint64).astype(np.uint32)
    got_o, got_d = np.zeros_like(o), np.zeros_like(o)
    for k in range(len(o)):
        cam = RR.pinhole(o[k], T[k])
        st = C.c_uint32(int(words[k]))
        oo, dd = (C.c_float * 3)(), (C.c_float * 3)()
        lib.orc_get_ray(C.byref(cam), float(s[k]), float(t[k]), C.byref(st), oo, dd)
        got_o[k], got_d[k] = oo[:], dd[:]
    same(got_o, o, "the pinhole's origin")
    same(got_d, dn, "the pinhole's direction against unit(fl(T - o))")


@pytest.mark.parametrize("call", ["rt.radiance_rays(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32), 2)", "rt.last_radiance_ms()",
                                  "rt.radiance_rays(np.zeros((0, 3), np.float32), np.ones((0, 3), np.float32), 2)"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99(call + "\n")


def test_wrong_shapes_are_value_errors(rt):
    org, d = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    for bad in (np.zeros((4, 2), np.float32), np.zeros(12, np.float32), np.zeros((3, 3), np.float32)):
        with pytest.raises(ValueError):
            rt.radiance_rays(bad, d, 2)
        with pytest.raises(ValueError):
            rt.radiance_rays(org, bad, 2)
    with pytest.raises(ValueError):
        rt.radiance_rays(org, d, np.ones(3, np.int32))
    with pytest.raises(ValueError):
        rt.radiance_rays(org, d, 2, ids=np.zeros(5, np.uint32))
    with pytest.raises(ValueError):
        rt.radiance_rays(org, d, 2, first=np.ones(4, np.int32))                                 # first without state
    with pytest.raises(ValueError):
        rt.radiance_rays(org, d, 2, first=np.ones(4, np.int32), state=np.zeros((3, 4), np.uint32))


# ---- the standard lists: conditions, from the reference alone ----------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_standard_list_is_built_as_stated(rt, tag):
    org, T, d = RR.standard_list(tag)
    mesh = PR.is_mesh(tag)
    n = RR.N + (0 if mesh else RR.AXIS_PARALLEL)
    assert org.shape == T.shape == d.shape == (n, 3) and org.dtype == T.dtype == d.dtype == np.float32 and n % 64 != 0
    same(d, T - org, f"{tag}: d = fl32(T - o)")
    for a in (org, T, d):
        assert np.isfinite(a).all() and not np.signbit(a[a == 0]).any()
    share = np.abs(d.astype(np.float64)).min(axis=1) / np.linalg.norm(d.astype(np.float64), axis=1)
    if mesh:
        assert share.min() >= RR.MIN_AXIS_SHARE
    else:
        zeros = (d == 0).sum(axis=1)
        assert (zeros > 0).sum() == RR.AXIS_PARALLEL and (zeros == 2).sum() == 12 and (zeros == 1).sum() == 4
    cam_o = np.array(list(PR.scene(rt, tag)["cam"].origin.e), np.float32)
    at_camera = (org == cam_o).all(axis=1)
    assert RR.N // 2 <= at_camera.sum() and (~at_camera).sum() >= RR.N // 2
    lo, hi = RR.scene_box(tag)
    probes = org[~at_camera].astype(np.float64)
    assert (probes >= lo - 1e-3).all() and (probes <= hi + 1e-3).all()


@pytest.mark.parametrize("tag", TAGS)
def test_standard_list_covers_what_the_gpu_tests_need(tag):
    mesh = PR.is_mesh(tag)
    ns = 3 if mesh else 4
    org, T, _ = RR.standard_list(tag)
    out, rays, shadows = RR.oracle_standard(tag, ns)
    n = len(out)
    black = float((out == 0).all(axis=1).mean())
    differ = float((bits(out)[1:] != bits(out)[:-1]).any(axis=1).mean())
    print(tag, "entries", n, "black", black, "adjacent entries that differ", differ, "rays == ns", float((rays == ns).mean()), "max rays", int(rays.max()),
          "shadow rays", int(shadows.sum()))
    assert np.isfinite(out).all()
    assert black <= 0.25
    assert differ >= 0.99
    if mesh:
        assert int(shadows.sum()) > 0
    else:
        assert (rays == ns).mean() >= 0.20 and int(rays.max()) >= 10 * ns
    # the seed id is the stream: one ray under two ids differs, under one id twice it is equal (the dearest entries that are not black: paths that draw)
    lit = np.flatnonzero((out != 0).any(axis=1))
    pick = lit[np.argsort(rays[lit])[-8:]]
    again, _ = RR.oracle_rays(tag, org[pick], T[pick], pick, ns)
    other, _ = RR.oracle_rays(tag, org[pick], T[pick], pick + 7919, ns)
    same(again, out[pick], f"{tag}: one id twice")
    assert (bits(other) != bits(out[pick])).any(axis=1).all()
