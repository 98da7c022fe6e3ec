"""GPU checks of filterTexels (include/rt_api.h, "filtering texels"), bit for bit: the device call against the CPU twin and the numpy restatement
(tests/texel_filter_reference.py) on the scenes' own rtAtlasGrid atlases in both fp modes and on the atlases of tests/test_texels_api.py, through
updateTriangles and rebuildBvh; a bake filtered where it lies (in = NULL) against the same bake filtered from the downloaded plane; out may be in; nothing
another call observes changes; misuse is the library's exit 99 (the calls before init: tests/test_texel_filter_api.py)."""
import os

import numpy as np
import pytest

import gather_reference as GR
import texel_filter_reference as FR
import texels_reference as TR
from preview_support import bits, exits_99, same
from texels_support import init, max_dist_of, private_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW, BH, DIRS, NS, DILATE = 24, 16, 5, 2, 2


@pytest.fixture(scope="module")
def meshes(rt, tmp_path_factory):
    """M1 and M2_floor with rtAtlasGrid UVs, read-only: a test that edits a mesh takes a private_mesh of its own."""
    return {tag: private_mesh(rt, tag, tmp_path_factory.mktemp("texel_filter")) for tag in ("M1", "M2_floor")}


_RASTERS = {}


def raster_of(key, tris, W, H, dilate):
    """texels_reference.raster of `tris`, computed once per `key` and size (the tests leave it unchanged); the dilation is applied to a copy."""
    if (key, W, H) not in _RASTERS:
        _RASTERS[key, W, H] = TR.raster(tris, W, H)
    ras = dict(_RASTERS[key, W, H])
    for _ in range(dilate):
        ras["src"] = TR.dilate_once(ras["src"])
    return ras


def check_filter(rt, key, tris, W, H, C, dilate, what, seed=3, **kw):
    """filterTexels now against the twin and numpy over `tris`, the triangles the device holds.  Returns (the raster, the input plane, the device's out)."""
    ras = raster_of(key, tris, W, H, dilate)
    plane = FR.noisy_plane(ras, C, seed)
    args = dict(FR.DEFAULTS, **kw)
    owned, got = rt.filter_texels(W, H, FR.MODE_OF[C], plane, dilate=dilate, **args)
    ms = rt.last_filter_ms()
    t_owned, twin = rt.filter_texels_host(tris, W, H, FR.MODE_OF[C], plane, dilate=dilate, **args)
    n_owned, ref = FR.filter_numpy(tris, W, H, dilate, plane, ras=ras, **args)
    print(what, f"{W} x {H} x {C} dilate {dilate} {kw}: owned", owned, "kernel ms", ms)
    assert owned == t_owned == n_owned == ras["owned"], (what, owned, t_owned, n_owned)
    same(got, twin, f"{what}: against the host twin")
    same(got, ref, f"{what}: against numpy")
    assert ms > 0.0 and np.isfinite(got).all()
    return ras, plane, got


# ---- 1. the device against the twin and numpy -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp", ["parity", "fast"])
@pytest.mark.parametrize("tag", ["M1", "M2_floor"])
def test_filter_of_the_grid_atlas(rt, meshes, tag, fp):
    """Widths 1, 3 and 27, iterations 1, 4 and 8, both sigma_c regimes (for 27 channels too: the leading group steers the other eight), dilate 0 and 3."""
    tris = meshes[tag].tris.copy()
    init(rt, meshes, tag, **({"fp": rt.RT_FP_FAST} if fp == "fast" else {}))
    try:
        ras, plane, got = check_filter(rt, tag, tris, 37, 23, 3, 3, tag)                                            # the defaults
        owned = ras["prim"] != TR.PRIM_NONE
        assert (bits(got[owned]) != bits(plane[owned])).any() and (got[ras["src"] == -1] == 0).all()
        check_filter(rt, tag, tris, 64, 64, 27, 0, tag, iterations=8, normal_squarings=0, sigma_c=0.5)
        check_filter(rt, tag, tris, 64, 64, 1, 3, tag, iterations=1, sigma_c=0.0)
        check_filter(rt, tag, tris, 37, 23, 27, 3, tag, sigma_c=0.0, sigma_d=3.0, sigma_z=1.0)
        check_filter(rt, tag, tris, 37, 23, 1, 0, tag, iterations=8, normal_squarings=7, sigma_c=0.25)
        check_filter(rt, tag, tris, 64, 64, 3, 0, tag, iterations=8, sigma_c=-1.0)
    finally:
        rt.cleanupRenderer()


def test_filter_of_the_test_atlases(rt, meshes):
    """(a) - (c) of tests/test_texels_api.py and random overlapping UVs on M1's slots, uploaded through updateTriangles after init."""
    base = meshes["M1"].tris.copy()
    init(rt, meshes, "M1")
    try:
        for name, (tris, W, H), C, dilate, kw in (("exact", TR.atlas_exact(base), 3, 0, dict(sigma_c=0.5)),
                                                  ("overlapping", (TR.atlas_overlapping(base), 37, 23), 27, 3, dict(iterations=8, sigma_c=0.5)),
                                                  ("1 x 1", TR.atlas_small(base, 1, 1), 1, 3, dict(iterations=8)),
                                                  ("1 x 5", TR.atlas_small(base, 1, 5), 27, 0, dict(iterations=4, sigma_c=0.5)),
                                                  ("1 x 5", TR.atlas_small(base, 1, 5), 3, 3, dict(iterations=1, sigma_c=0.0))):
            rt.update_triangles(0, tris)
            check_filter(rt, name, tris, W, H, C, dilate, name, **kw)
        rt.update_triangles(0, base)
    finally:
        rt.cleanupRenderer()


def test_filter_follows_update_triangles_and_rebuild(rt, tmp_path):
    """The real triangles permuted among the real slots and shifted, then rebuildBvh: the call follows the live raster both times."""
    hm = private_mesh(rt, "M1", tmp_path)
    base = hm.tris.copy()
    init(rt, {"M1": hm}, "M1")
    try:
        _, _, before = check_filter(rt, "before", base, 37, 23, 3, 1, "before")
        new = base.copy()
        real = np.flatnonzero(~np.isinf(new["v"][:, 0, 0]))
        rng = np.random.default_rng(71)
        new[real] = new[real][rng.permutation(len(real))]
        new["v"][real] += rng.uniform(-0.5, 0.5, (len(real), 1, 3)).astype(np.float32)
        rt.update_triangles(0, new)
        _, _, moved = check_filter(rt, "moved", new, 37, 23, 3, 1, "after updateTriangles")
        assert (bits(moved) != bits(before)).any()
        hm.tris[:] = new
        hm.refit()
        old = rt.rebuild_bvh()
        assert (old != np.arange(len(old))).any()
        check_filter(rt, "rebuilt", hm.tris.copy(), 37, 23, 3, 1, "after rebuildBvh")
    finally:
        rt.cleanupRenderer()


# ---- 2. a bake filtered where it lies ------------------------------------------------------------------------------------------------------

def test_null_in_is_the_last_bake_where_it_lies(rt, meshes):
    tris = meshes["M1"].tris.copy()
    init(rt, meshes, "M1")
    try:
        for mode in (GR.IRRADIANCE, GR.VISIBILITY):
            _, baked = rt.bake_texels(BW, BH, mode, DIRS, ns=NS, dilate=DILATE, bias=1e-3, max_dist=max_dist_of("M1"))
            owned, here = rt.filter_texels(BW, BH, mode, None, dilate=DILATE, sigma_c=0.5)
            again = rt.filter_texels(BW, BH, mode, None, dilate=DILATE, sigma_c=0.5)[1]               # (the bake's plane is read, not written)
            o2, down = rt.filter_texels(BW, BH, mode, baked["out"], dilate=DILATE, sigma_c=0.5)
            twin = rt.filter_texels_host(tris, BW, BH, mode, baked["out"], dilate=DILATE, sigma_c=0.5)[1]
            assert owned == o2 and (baked["out"] != 0).any()
            same(here, down, f"mode {mode}: in = NULL against the downloaded out")
            same(again, here, f"mode {mode}: in = NULL, a second time")
            same(here, twin, f"mode {mode}: against the host twin")
            buf = baked["out"].copy()
            assert rt.filter_texels(BW, BH, mode, buf, dilate=DILATE, sigma_c=0.5, out=buf)[1] is buf
            same(buf, down, f"mode {mode}: out is in")
    finally:
        rt.cleanupRenderer()


# ---- 3. leaves everything else alone -----------------------------------------------------------------------------------------------------------

def test_changes_nothing_another_call_observes(rt, meshes):
    pos, nrm = (np.ascontiguousarray(a[:40]) for a in GR.standard_points())
    init(rt, meshes, "M1")
    try:
        kw = dict(ns=NS, dilate=DILATE, bias=1e-3, max_dist=max_dist_of("M1"), rays=True)
        g_before = rt.gather_radiance(pos, nrm, GR.IRRADIANCE, DIRS, ns=NS, bias=1e-3, rays=True)
        b_before = rt.bake_texels(BW, BH, GR.IRRADIANCE, DIRS, **kw)
        r_before = rt.raster_texels(37, 23, 3)
        seen = lambda: (rt.last_texels_ms(), rt.last_bake_ms(), rt.last_gather_ms())
        was = seen()
        assert min(was) > 0
        plane = FR.noisy_plane(dict(pos=r_before[1]["pos"], nrm=r_before[1]["nrm"], prim=r_before[1]["prim"]), 27, 1)
        rt.filter_texels(37, 23, GR.SH9, plane, dilate=1, sigma_c=0.5)
        rt.filter_texels(64, 64, GR.VISIBILITY, np.ones((64, 64, 1), np.float32))
        rt.filter_texels(BW, BH, GR.IRRADIANCE, None, dilate=DILATE)
        assert rt.last_filter_ms() > 0 and seen() == was
        r_after = rt.raster_texels(37, 23, 3)
        b_after = rt.bake_texels(BW, BH, GR.IRRADIANCE, DIRS, **kw)
        g_after = rt.gather_radiance(pos, nrm, GR.IRRADIANCE, DIRS, ns=NS, bias=1e-3, rays=True)
        assert r_after[0] == r_before[0] and b_after[0] == b_before[0]
        for k in r_before[1]:
            same(r_after[1][k], r_before[1][k], f"rasterTexels around the filter: {k}")
        for k in b_before[1]:
            same(b_after[1][k], b_before[1][k], f"bakeTexels around the filter: {k}")
        for k in range(2):
            same(g_after[k], g_before[k], "gatherRadiance around the filter")
        assert np.array_equal(g_after[2], g_before[2])
    finally:
        rt.cleanupRenderer()


# ---- 4. misuse -------------------------------------------------------------------------------------------------------------------------------

_INIT = ("import sys; sys.path.insert(0, %r); import pixels_reference as PR\n" % os.path.join(ROOT, "tests") +
         "PR.init(rt, 'M1'); r = rt.load_renderer(); fp = C.POINTER(C.c_float)\n"
         "a = np.zeros((8, 8, 27), np.float32); p = a.ctypes.data_as(fp)\n"
         "F = lambda **kw: rt.filter_texels(kw.pop('W', 8), kw.pop('H', 8), kw.pop('mode', 0), kw.pop('plane', a[:, :, :3]), **kw)\n"
         "B = lambda W=8, H=8, mode=0: rt.bake_texels(W, H, mode, 4, max_dist=1.0)\n")
_SPHERES = ("import sys; sys.path.insert(0, %r); import pixels_reference as PR\n" % os.path.join(ROOT, "tests") + "PR.init(rt, 'S1')\n")


@pytest.mark.parametrize("body", [
    _SPHERES + "rt.filter_texels(8, 8, 0, np.zeros((8, 8, 3), np.float32))",                                            # a sphere scene
    _INIT + "r.filterTexels(0, 8, 0, 0, p, p, 4, 5, 2.0, 2.0, 1.0)",                                                    # what rasterTexels refuses
    _INIT + "r.filterTexels(8, 8193, 0, 0, p, p, 4, 5, 2.0, 2.0, 1.0)",
    _INIT + "r.filterTexels(8, 8, -1, 0, p, p, 4, 5, 2.0, 2.0, 1.0)",
    _INIT + "r.filterTexels(8, 8, 17, 0, p, p, 4, 5, 2.0, 2.0, 1.0)",
    _INIT + "r.filterTexels(8, 8, 0, 3, p, p, 4, 5, 2.0, 2.0, 1.0)",                                                    # an unknown mode
    _INIT + "r.filterTexels(8, 8, 0, -1, p, p, 4, 5, 2.0, 2.0, 1.0)",
    _INIT + "r.filterTexels(8, 8, 0, 0, p, None, 4, 5, 2.0, 2.0, 1.0)",                                                 # out NULL
    _INIT + "F(iterations=0)", _INIT + "F(iterations=9)", _INIT + "F(normal_squarings=-1)", _INIT + "F(normal_squarings=8)",
    _INIT + "F(sigma_d=0.0)", _INIT + "F(sigma_d=float('nan'))", _INIT + "F(sigma_d=float('inf'))",
    _INIT + "F(sigma_z=-1.0)", _INIT + "F(sigma_z=float('nan'))", _INIT + "F(sigma_z=float('inf'))",
    _INIT + "F(sigma_c=float('nan'))", _INIT + "F(sigma_c=float('inf'))",
    _INIT + "F(plane=None)",                                                                                            # in NULL: no bake yet,
    _INIT + "B(); F(plane=None, W=9)", _INIT + "B(); F(plane=None, H=7)",                                               # a bake of another size,
    _INIT + "B(mode=0); F(plane=None, mode=2)", _INIT + "B(mode=1); F(plane=None, mode=0)",                             # of another width,
    _INIT + "B(); r.bakeTexels(8, 8, 0, 0, 0, 4, 4, 1, 0, 0.0, 1.0, p, None, None, None, None); F(plane=None)",         # the last bake without out,
    _INIT + "B(); F(plane=None); rt.cleanupRenderer(); PR.init(rt, 'M1'); F(plane=None)",                               # cleanupRenderer + init
], ids=lambda body: ("spheres: " if body.startswith(_SPHERES) else "") + body.rsplit("\n", 1)[-1][:70])
def test_misuse_exits_99(body):
    exits_99(body + "\n")


def test_what_misuse_does_not_cover_is_accepted(rt, meshes):
    """The edges of the checks from the inside: the largest counts, a negative sigma_c, a bake of another mode of the same width, and an atlas no triangle
    covers - 0 owned texels, out all zero."""
    base = meshes["M1"].tris.copy()
    init(rt, meshes, "M1")
    try:
        rt.bake_texels(BW, BH, GR.IRRADIANCE, DIRS, max_dist=1.0)
        a = rt.filter_texels(BW, BH, GR.IRRADIANCE, None, dilate=16, iterations=8, normal_squarings=7, sigma_c=-3.0)
        parked = base.copy()
        parked["texCoords"] = TR.PARKED
        rt.update_triangles(0, parked)
        b = rt.filter_texels(9, 7, GR.SH9, np.ones((7, 9, 27), np.float32), dilate=3)
        rt.update_triangles(0, base)
    finally:
        rt.cleanupRenderer()
    assert a[0] > 0 and np.isfinite(a[1]).all()
    assert b[0] == 0 and (b[1] == 0).all()
