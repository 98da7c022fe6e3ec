"""CPU checks of gatherRadiance (include/rt_api.h): the calls are declared, exported and bound, the calls before init are the library's misuse exit, the CPU
twin of the generator (rtGatherDirectionsHost, librt_host.so) equals the numpy restatement (tests/gather_reference.py) bit for bit, the reference shows on
the standard list what the GPU tests are there to cover - conditions on the inputs, caps, not measurements -, the directions have the distribution the
definition claims within derived widths, and the reduction of a constant is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gather_reference as GR
from preview_support import bits, exits_99, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
HOST = open(os.path.join(ROOT, "include", "rt_host.h")).read()
MODES = (GR.IRRADIANCE, GR.SH9, GR.VISIBILITY)
BASE_IDS = (0, 17, 0xFFFFFFF0)
FIRST, DIRS, TOTAL = 3, 9, 16


def _sig(name, ret, args):
    return ret + r"\s+" + name + r"\s*\(\s*" + r"\s*,\s*".join(a.replace(" ", r"\s+").replace("*", r"\s*\*\s*") for a in args) + r"\s*\)\s*;"


def test_declared_exported_and_bound(rt):
    dirs_args = ["int n", "const float* pos", "const float* nrm", "int mode", "int first", "int dirs", "int dirs_total", "uint32_t base_id", "float bias",
                 "float* org", "float* dir", "uint32_t* ids"]
    assert re.search(_sig("gatherRadiance", "void", ["int n", "const float* pos", "const float* nrm", "int mode", "int first", "int dirs", "int dirs_total", "int ns",
                                                     "uint32_t base_id", "float bias", "float max_dist", "float* acc", "float* out", "uint32_t* rays"]), API)
    assert re.search(_sig("rtGatherDirections", "void", dirs_args), API)
    assert re.search(_sig("rtGatherDirectionsHost", "void", dirs_args), HOST)
    assert re.search(r"int\s+rtGatherWidth\s*\(\s*int\s+mode\s*\)\s*;", API) and re.search(r"double\s+rtLastGatherMs\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"enum\s*\{\s*RT_GATHER_IRRADIANCE\s*=\s*0\s*,\s*RT_GATHER_SH9\s*=\s*1\s*,\s*RT_GATHER_VISIBILITY\s*=\s*2\s*\}\s*;", API)
    assert re.search(r"#define RT_GATHER_MAX_DIRS 65536\b", API)
    assert API.index("void   radianceRays") < API.index("void   gatherRadiance") < API.index("int    refineFrame")       # beside radianceRays
    assert re.search(r"#define RT_API_VERSION 1002\b", API) and rt.RT_API_VERSION == 1002      # additive: the version stays
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in ("gatherRadiance", "rtGatherDirections", "rtGatherWidth", "rtLastGatherMs"):
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    assert hasattr(C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_host.so")), "rtGatherDirectionsHost")
    assert "rtGatherDirectionsHost" in rt.HOST_SYMBOLS
    r, h = rt.load_renderer(), rt.load_host()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    i, u, f = C.c_int, C.c_uint32, C.c_float
    assert r.gatherRadiance.argtypes == [i, fp, fp, i, i, i, i, i, u, f, f, fp, fp, up] and r.gatherRadiance.restype is None
    assert r.rtGatherDirections.argtypes == [i, fp, fp, i, i, i, i, u, f, fp, fp, up] and r.rtGatherDirections.restype is None
    assert h.rtGatherDirectionsHost.argtypes == r.rtGatherDirections.argtypes and h.rtGatherDirectionsHost.restype is None
    assert r.rtGatherWidth.argtypes == [i] and r.rtGatherWidth.restype is i
    assert r.rtLastGatherMs.argtypes == [] and r.rtLastGatherMs.restype is C.c_double
    for name in ("gather_radiance", "gather_directions", "gather_directions_host", "gather_width", "last_gather_ms"):
        assert callable(getattr(rt, name)), name
    assert (rt.RT_GATHER_IRRADIANCE, rt.RT_GATHER_SH9, rt.RT_GATHER_VISIBILITY, rt.RT_GATHER_MAX_DIRS) == (0, 1, 2, 65536)
    # rtGatherWidth needs no init and never exits for a known mode
    assert [rt.gather_width(m) for m in MODES] == [3, 27, 1] == [GR.WIDTH[m] for m in MODES]


@pytest.mark.parametrize("call", ["rt.gather_radiance(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32), rt.RT_GATHER_IRRADIANCE, 4)",
                                  "rt.gather_radiance(np.zeros((0, 3), np.float32), np.ones((0, 3), np.float32), rt.RT_GATHER_VISIBILITY, 4)",
                                  "rt.gather_directions(np.zeros((4, 3), np.float32), None, rt.RT_GATHER_SH9, 4)",
                                  "rt.last_gather_ms()", "rt.gather_width(3)"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99(call + "\n")


def test_wrong_shapes_are_value_errors(rt):
    pos, nrm = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    for fn in (lambda p, n, m: rt.gather_radiance(p, n, m, 4), lambda p, n, m: rt.gather_directions(p, n, m, 4),
               lambda p, n, m: rt.gather_directions_host(p, n, m, 4)):
        for bad in (np.zeros((4, 2), np.float32), np.zeros(12, np.float32)):
            with pytest.raises(ValueError):
                fn(bad, nrm, rt.RT_GATHER_IRRADIANCE)
        with pytest.raises(ValueError):
            fn(pos, np.ones((3, 3), np.float32), rt.RT_GATHER_VISIBILITY)
        with pytest.raises(ValueError):
            fn(pos, None, rt.RT_GATHER_IRRADIANCE)                                              # only SH9 goes without normals
        with pytest.raises(ValueError):
            fn(pos, nrm, 3)
    with pytest.raises(ValueError):
        rt.gather_radiance(pos, nrm, rt.RT_GATHER_IRRADIANCE, 4, first=2)                       # first without acc
    with pytest.raises(ValueError):
        rt.gather_radiance(pos, nrm, rt.RT_GATHER_SH9, 4, first=2, acc=np.zeros((4, 3), np.float32))
    for kw in (dict(dirs=0), dict(dirs=4, first=-1), dict(dirs=4, first=2, dirs_total=5), dict(dirs=65537)):
        with pytest.raises(ValueError):
            rt.gather_directions_host(pos, nrm, rt.RT_GATHER_IRRADIANCE, **kw)


# ---- the generator: the CPU twin against numpy ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("base_id", BASE_IDS)
@pytest.mark.parametrize("bias", [0.0, 1e-3])
def test_host_twin_equals_the_numpy_generator(rt, mode, base_id, bias):
    pos, nrm = GR.standard_points()
    ref_o, ref_d, ref_ids = GR.directions(pos, nrm, mode, FIRST, DIRS, TOTAL, base_id, bias)
    org, d, ids = rt.gather_directions_host(pos, None if mode == GR.SH9 else nrm, mode, DIRS, first=FIRST, dirs_total=TOTAL, base_id=base_id, bias=bias)
    assert org.shape == d.shape == (GR.N_POINTS * DIRS, 3) and ids.shape == (GR.N_POINTS * DIRS,)
    assert np.array_equal(ids, ref_ids)
    same(org, ref_o, f"mode {mode} base {base_id} bias {bias}: origins")
    same(d, ref_d, f"mode {mode} base {base_id} bias {bias}: directions")
    if base_id == 0xFFFFFFF0:
        assert (ids < 0x1000).any() and (ids >= 0xFFFFFFF0).any()                              # the ids wrap past 2^32
    if mode == GR.SH9:
        same(org, np.repeat(pos, DIRS, axis=0), "SH9: o = P")
    elif bias == 0.0:
        same(org, np.repeat(pos + np.float32(0.0) * GR.unit_normals(nrm), DIRS, axis=0), "bias 0: o = P + 0 * Nn")


def test_host_twin_writes_only_what_is_asked_and_refuses_quietly(rt):
    pos, nrm = GR.standard_points()
    h = rt.load_host()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    p = lambda a, t: a.ctypes.data_as(t)
    n = GR.N_POINTS
    _, ref_d, ref_ids = GR.directions(pos, nrm, GR.IRRADIANCE, 0, 2, 2)
    d, ids = np.zeros((n * 2, 3), np.float32), np.zeros(n * 2, np.uint32)
    h.rtGatherDirectionsHost(n, p(pos, fp), p(nrm, fp), 0, 0, 2, 2, 0, 0.0, None, p(d, fp), None)
    same(d, ref_d, "dir alone")
    h.rtGatherDirectionsHost(n, p(pos, fp), p(nrm, fp), 0, 0, 2, 2, 0, 0.0, None, None, p(ids, up))
    assert np.array_equal(ids, ref_ids)
    d[:] = 7.0
    for args in ((n, p(pos, fp), None, 0, 0, 2, 2), (n, None, p(nrm, fp), 0, 0, 2, 2), (n, p(pos, fp), p(nrm, fp), 3, 0, 2, 2), (n, p(pos, fp), p(nrm, fp), 0, 1, 2, 2),
                 (n, p(pos, fp), p(nrm, fp), 0, 0, 0, 2), (n, p(pos, fp), p(nrm, fp), 0, -1, 2, 2), (-1, p(pos, fp), p(nrm, fp), 0, 0, 2, 2)):
        h.rtGatherDirectionsHost(*args, 0, 0.0, None, p(d, fp), None)
    h.rtGatherDirectionsHost(n, p(pos, fp), p(nrm, fp), 0, 0, 2, 2, 0, float("nan"), None, p(d, fp), None)
    assert (d == 7.0).all()


# ---- conditions on the reference's inputs: caps ----------------------------------------------------------------------------------------

BIG = 4096


@pytest.fixture(scope="module")
def big():
    pos, nrm = GR.standard_points()
    cos_lists = GR.directions(pos, nrm, GR.IRRADIANCE, 0, BIG, BIG, details=True)
    sph_lists = GR.directions(pos, None, GR.SH9, 0, BIG, BIG, details=True)
    return cos_lists, sph_lists


def test_the_standard_lists_cover_what_the_tests_need(big):
    pos, nrm = GR.standard_points()
    l = np.linalg.norm(nrm.astype(np.float64), axis=1)
    axis = ((nrm != 0).sum(axis=1) == 1)
    assert axis.sum() == 12 and (np.abs(l - 1e-3) < 1e-5).sum() == 4 and (np.abs(l - 1e3) < 1).sum() == 4 and (np.abs(l - 1) > 0.05).sum() > 50
    assert not np.signbit(nrm[nrm == 0]).any()
    for mode in MODES:
        for base_id in BASE_IDS:
            _, D, _, rounds, _ = GR.directions(pos, nrm, mode, FIRST, DIRS, TOTAL, base_id, details=True)
            print("mode", mode, "base", base_id, "max rounds", int(rounds.max()), "smallest |D|", float(np.linalg.norm(D.astype(np.float64), axis=1).min()))
            assert rounds.max() > (8 if base_id == 17 else 1)                                   # the rejection loop diverges: one list has a loop of more than 8 rounds
            assert not (D == 0).all(axis=1).any() and not np.signbit(D[D == 0]).any()
    (_, D, _, rounds, _), (_, Ds, _, rounds_s, _) = big
    print("70 x 4096: max rounds", int(rounds.max()), int(rounds_s.max()), "smallest |D|", float(np.linalg.norm(D.astype(np.float64), axis=1).min()))
    assert rounds.max() > 8 and rounds_s.max() > 8                                              # at least one loop runs more than 8 rounds
    assert not (D == 0).all(axis=1).any()                                                       # no D is all-zero
    assert not np.signbit(D[D == 0]).any() and not np.signbit(Ds[Ds == 0]).any()                # no D has a negative zero
    # the two streams of a ray do not share a seed
    g = GR.ray_ids(GR.N_POINTS, 0, 64, 64, 0)
    assert not np.intersect1d(GR.pixel_seed(g), GR.pixel_seed((~g) & GR.M32)).size


def test_the_directions_have_the_claimed_distribution(big):
    """Over T = 70 x 4096 directions: D = Nn + u is cosine-distributed about Nn, so E cos = 2/3 with Var cos = 1/2 - 4/9 = 1/18; u is uniform on the sphere, so
    each component has mean 0 and variance 1/3.  Five standard errors of the mean each: widths from the distributions, not from what the generator gives."""
    pos, nrm = GR.standard_points()
    (_, D, _, _, _), (_, _, _, _, u) = big
    T = GR.N_POINTS * BIG
    nn = np.repeat(GR.unit_normals(nrm).astype(np.float64), BIG, axis=0)
    D = D.astype(np.float64)
    cos = (D * nn).sum(axis=1) / np.linalg.norm(D, axis=1) / np.linalg.norm(nn, axis=1)
    sigma = np.sqrt((1 / 18) / T)
    print("mean cos", cos.mean(), "in sigma", (cos.mean() - 2 / 3) / sigma)
    assert cos.min() >= -1e-6 and abs(cos.mean() - 2 / 3) <= 5 * sigma
    sigma = np.sqrt((1 / 3) / T)
    mean = u.astype(np.float64).mean(axis=0)
    print("mean u in sigma", mean / sigma)
    assert (np.abs(mean) <= 5 * sigma).all()
    assert np.abs(np.linalg.norm(u.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_the_reduction_of_a_constant_is_exact():
    pos, nrm = GR.standard_points()
    ones = lambda org, D, ids: (np.ones((len(D), 3), np.float32), np.full(len(D), 2))
    out, acc, rays = GR.gather(pos, nrm, GR.IRRADIANCE, 0, 11, 11, ones)
    assert (out == 1.0).all() and (acc == 11.0).all() and (rays == 22).all() and out.shape == (GR.N_POINTS, 3)
    out2, acc2, _ = GR.gather(pos, nrm, GR.IRRADIANCE, 11, 5, 16, ones, acc=acc)
    assert (out2 == 1.0).all() and (acc2 == 16.0).all()
    vis = lambda org, D, ids: (np.ones(len(D), np.float32), np.zeros(len(D)))
    out, acc, rays = GR.gather(pos, nrm, GR.VISIBILITY, 0, 11, 11, vis)
    assert (out == 1.0).all() and (acc == 11.0).all() and (rays == 0).all() and out.shape == (GR.N_POINTS, 1)
    # SH9 of a constant: the band-0 coefficient is 4 pi * 0.282095 whatever the directions, and a split equals the whole
    out, acc, _ = GR.gather(pos, None, GR.SH9, 0, 16, 16, ones)
    assert out.shape == (GR.N_POINTS, 27) and np.allclose(out[:, :3], 12.566371 * 0.282095, rtol=1e-6)
    _, part, _ = GR.gather(pos, None, GR.SH9, 0, 5, 16, ones)
    out2, acc2, _ = GR.gather(pos, None, GR.SH9, 5, 11, 16, ones, acc=part)
    same(out2, out, "SH9 in two parts against one")
    same(acc2, acc, "SH9 sums in two parts against one")
    assert (bits(out[:, 3:]) != 0).any()
