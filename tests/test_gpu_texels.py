"""GPU checks of rasterTexels / bakeTexels (include/rt_api.h, "baking texels"), bit for bit: the device raster against the CPU twin and the numpy
restatement (tests/texels_reference.py) on the atlases of tests/test_texels_api.py and on the scenes' own rtAtlasGrid atlases, through updateTriangles and
rebuildBvh; the bake against this library's gatherRadiance over the full W*H point list built from rasterTexels' planes, in both fp modes; resumption by
first / acc; a bake that crosses the chunk; the optional planes; nothing another call observes changes; misuse is the library's exit 99 (the calls before
init: tests/test_texels_api.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import gather_reference as GR
import pixels_reference as PR
import radiance_reference as RR
import texels_reference as TR
from preview_support import bits, exits_99, same, stats_tuple
from texels_support import MARGIN, check_bake, check_raster, full_list, init, max_dist_of, private_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (GR.IRRADIANCE, GR.SH9, GR.VISIBILITY)
BW, BH, DIRS, NS, DILATE = 24, 16, 5, 2, 2


@pytest.fixture(scope="module")
def meshes(rt, tmp_path_factory):
    """M1 and M2_floor with rtAtlasGrid UVs, read-only: a test that edits a mesh takes a private_mesh of its own."""
    return {tag: private_mesh(rt, tag, tmp_path_factory.mktemp("texels")) for tag in ("M1", "M2_floor")}


# ---- 1. the raster ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["M1", "M2_floor"])
def test_raster_of_the_grid_atlas(rt, meshes, tag):
    tris = meshes[tag].tris.copy()
    init(rt, meshes, tag)
    try:
        a = check_raster(rt, tris, 37, 23, 2, tag)
        b = check_raster(rt, tris, 64, 64, 0, tag)
    finally:
        rt.cleanupRenderer()
    assert a["owned"] > 0 and b["covers"].max() == 1 and (b["prim"] == TR.PRIM_NONE).any()


def test_raster_of_the_test_atlases(rt, meshes):
    """(a) - (c) of tests/test_texels_api.py and random overlapping UVs on M1's slots, uploaded through updateTriangles after init."""
    base = meshes["M1"].tris.copy()
    assert np.isinf(base["v"][:, 0, 0]).any()                                                     # the leaf padding: sentinel slots
    init(rt, meshes, "M1")
    try:
        for name, (tris, W, H), dilate in (("exact", TR.atlas_exact(base), 0), ("odd", TR.atlas_odd(base), 3), ("1 x 1", TR.atlas_small(base, 1, 1), 1),
                                           ("1 x 5", TR.atlas_small(base, 1, 5), 1), ("overlapping", (TR.atlas_overlapping(base), 37, 23), 16)):
            rt.update_triangles(0, tris)
            ref = check_raster(rt, tris, W, H, dilate, name)
            if name == "exact":
                assert (ref["covers"] >= 2).any() and ref["on_edge"].any() and (ref["prim"] == TR.PRIM_NONE).any()
            if name == "overlapping":
                assert (ref["covers"] >= 4).any() and (ref["src"] != -1).all()
        rt.update_triangles(0, base)
    finally:
        rt.cleanupRenderer()


def test_raster_follows_update_triangles_and_rebuild(rt, tmp_path):
    """The real triangles permuted among the real slots with their UVs and their vertices shifted (vertices and UVs move), then rebuildBvh: prim names the
    new slots, and the planes equal the twin run on rtRebuildBvh's triangles."""
    hm = private_mesh(rt, "M1", tmp_path)
    base = hm.tris.copy()
    init(rt, {"M1": hm}, "M1")
    try:
        before = check_raster(rt, base, 37, 23, 1, "before")
        new = base.copy()
        real = np.flatnonzero(~np.isinf(new["v"][:, 0, 0]))
        rng = np.random.default_rng(71)
        new[real] = new[real][rng.permutation(len(real))]
        new["v"][real] += rng.uniform(-0.5, 0.5, (len(real), 1, 3)).astype(np.float32)
        rt.update_triangles(0, new)
        moved = check_raster(rt, new, 37, 23, 1, "after updateTriangles")
        assert (moved["prim"] != before["prim"]).any() and (bits(moved["pos"]) != bits(before["pos"])).any()
        hm.tris[:] = new
        hm.refit()
        old = rt.rebuild_bvh()
        assert np.array_equal(old, hm.rebuild()) and (old != np.arange(len(old))).any()
        rebuilt = check_raster(rt, hm.tris.copy(), 37, 23, 1, "after rebuildBvh")
        owned = rebuilt["prim"] != TR.PRIM_NONE
        assert (owned == (moved["prim"] != TR.PRIM_NONE)).all()                                   # the same texels are covered (no two slots overlap) ...
        assert (old[rebuilt["prim"][owned]] == moved["prim"][owned]).all()                        # ... by the same triangles under their new names
        assert (rebuilt["prim"] != moved["prim"]).any()
        same(rebuilt["pos"], moved["pos"], "positions through the rebuild")
    finally:
        rt.cleanupRenderer()


# ---- 2. the bake against gatherRadiance over the full point list ------------------------------------------------------------------------

@pytest.mark.parametrize("fp", ["parity", "fast"])
@pytest.mark.parametrize("tag", ["M1", "M2_floor"])
def test_bake_equals_gather_over_the_full_list(rt, meshes, tag, fp):
    kw = dict(ns=NS, base_id=5, bias=1e-3, max_dist=max_dist_of(tag), rays=True)
    init(rt, meshes, tag, **({"fp": rt.RT_FP_FAST} if fp == "fast" else {}))
    try:
        owned, pl, pos, nrm = full_list(rt, BW, BH, DILATE)
        dilated = (pl["src"] != -1) & (pl["prim"] == TR.PRIM_NONE)
        assert 64 < owned < BW * BH and dilated.any()
        assert tag != "M1" or (pl["src"] == -1).any()                                              # owned, dilated and (M1) still empty texels occur
        for mode in MODES:
            got = rt.bake_texels(BW, BH, mode, DIRS, dilate=DILATE, **kw)
            print(tag, fp, "mode", mode, "owned", got[0], "texels ms", rt.last_texels_ms(), "bake ms", rt.last_bake_ms(), "mean out", float(got[1]["out"].mean()))
            if fp == "parity" or mode == GR.VISIBILITY:
                ref = rt.gather_radiance(pos, None if mode == GR.SH9 else nrm, mode, DIRS, **kw)
                check_bake(got, pl, ref, f"{tag} {fp} mode {mode}")
            else:
                assert np.array_equal(got[1]["prim"], pl["prim"]) and np.array_equal(got[1]["src"], pl["src"])
                assert np.isfinite(got[1]["out"]).all() and np.isfinite(got[1]["acc"]).all()
            mask = pl["prim"] != TR.PRIM_NONE
            assert (got[1]["out"][mask] != 0).any() and (got[1]["acc"][~mask] == 0).all() and (got[1]["rays"][~mask] == 0).all()
            assert (got[1]["out"][pl["src"] == -1] == 0).all()
            if mode != GR.VISIBILITY:
                assert (got[1]["rays"][mask] >= DIRS * NS).all()
    finally:
        rt.cleanupRenderer()


# ---- 3. a split equals the whole ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_split_equals_one_call(rt, meshes, mode):
    kw = dict(ns=NS, dilate=DILATE, base_id=11, bias=1e-3, max_dist=max_dist_of("M1"), rays=True, dirs_total=8)
    init(rt, meshes, "M1")
    try:
        _, one = rt.bake_texels(BW, BH, mode, 8, **kw)
        _, a = rt.bake_texels(BW, BH, mode, 3, **kw)
        _, b = rt.bake_texels(BW, BH, mode, 2, first=3, acc=a["acc"], **kw)
        _, c = rt.bake_texels(BW, BH, mode, 3, first=5, acc=b["acc"], **kw)
    finally:
        rt.cleanupRenderer()
    same(c["out"], one["out"], f"mode {mode}: (0, 3), (3, 2), (5, 3) against (0, 8), out")
    same(c["acc"], one["acc"], f"mode {mode}: acc")
    assert np.array_equal(a["rays"].astype(np.uint64) + b["rays"] + c["rays"], one["rays"])
    assert (bits(a["acc"]) != bits(one["acc"])).any() and (one["out"] != 0).any()


# ---- 4. across the chunk --------------------------------------------------------------------------------------------------------------

def test_chunk_crossing(rt, meshes):
    """VISIBILITY at dirs = RT_GATHER_MAX_DIRS: 64 list entries per chunk, on an atlas with more than 64 owned texels.  Point k is the texel index, whatever the
    compaction or chunking."""
    dirs = rt.RT_GATHER_MAX_DIRS
    assert rt.RT_RAY_CHUNK // dirs == 64
    W, H = BW, BH
    kw = dict(base_id=3, bias=1e-3, max_dist=max_dist_of("M1"), rays=True)
    init(rt, meshes, "M1")
    try:
        owned, pl, pos, nrm = full_list(rt, W, H, 1)
        assert 64 < owned < 128 < W * H                                                            # two chunks
        got = rt.bake_texels(W, H, GR.VISIBILITY, dirs, dilate=1, **kw)
        print("owned", owned, "rays", owned * dirs, "bake ms", rt.last_bake_ms())
        ref = rt.gather_radiance(pos, nrm, GR.VISIBILITY, dirs, **kw)
    finally:
        rt.cleanupRenderer()
    check_bake(got, pl, ref, "two chunks")
    mask = pl["prim"] != TR.PRIM_NONE
    assert len(np.unique(got[1]["out"][mask])) > 8


# ---- 5. the optional planes ---------------------------------------------------------------------------------------------------------------

def test_only_the_requested_planes_are_written(rt, meshes):
    ip, fp, up = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    n = BW * BH
    init(rt, meshes, "M1")
    try:
        r = rt.load_renderer()
        owned, full = rt.bake_texels(BW, BH, GR.IRRADIANCE, DIRS, ns=NS, dilate=DILATE, bias=1e-3, rays=True)
        _, ras = rt.raster_texels(BW, BH, DILATE)
        assert rt.last_texels_ms() > 0.0 and rt.last_bake_ms() > 0.0

        def bake(**want):
            arr = dict(acc=np.full((n, 3), 7, np.float32), out=np.full((n, 3), 7, np.float32), rays=np.full(n, 7, np.uint32), prim=np.full(n, 7, np.int32),
                       src=np.full(n, 7, np.int32))
            t = dict(acc=fp, out=fp, rays=up, prim=ip, src=ip)
            ptr = {k: (arr[k].ctypes.data_as(t[k]) if want.get(k) else None) for k in arr}
            ret = r.bakeTexels(BW, BH, DILATE, GR.IRRADIANCE, 0, DIRS, DIRS, NS, 0, 1e-3, 0.0, ptr["acc"], ptr["out"], ptr["rays"], ptr["prim"], ptr["src"])
            assert ret == owned
            for k in arr:
                if want.get(k):
                    same(arr[k].ravel(), full[k].ravel(), f"{sorted(want)}: {k}")
                else:
                    assert (arr[k] == 7).all(), (sorted(want), k)

        bake(out=True)
        bake(acc=True, src=True)
        bake(rays=True, prim=True)
        for k, t in (("prim", ip), ("src", ip), ("bary", fp), ("pos", fp), ("nrm", fp)):
            a = np.full(ras[k].shape, 7, ras[k].dtype)
            ptr = {j: (a.ctypes.data_as(t) if j == k else None) for j in ("prim", "src", "bary", "pos", "nrm")}
            assert r.rasterTexels(BW, BH, DILATE, ptr["prim"], ptr["src"], ptr["bary"], ptr["pos"], ptr["nrm"]) == owned
            same(a, ras[k], k + " alone")
    finally:
        rt.cleanupRenderer()


# ---- 6. leaves everything else alone ------------------------------------------------------------------------------------------------------

def test_changes_nothing_another_call_observes(rt, meshes):
    pos, nrm = (np.ascontiguousarray(a[:40]) for a in GR.standard_points())
    org, _, d = RR.standard_list("M1")
    fb = init(rt, meshes, "M1")
    try:
        rt.runRenderer(4, 8, 8)
        rt.runRendererProgressive(2, 8, 8)
        rt.radiance_rays(org[:100], d[:100], 2)
        g_before = rt.gather_radiance(pos, nrm, GR.IRRADIANCE, DIRS, ns=NS, bias=1e-3, rays=True)
        seen = lambda: (bits(np.array(fb, copy=True)).tobytes(), stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.progressive_samples(),
                        rt.last_gather_ms(), rt.last_radiance_ms(), rt.last_rays_ms(), rt.last_pixels_ms(), rt.last_update_ms(), rt.last_rebuild_ms())
        was = seen()
        assert was[3] == 2 and was[4] > 0 and was[5] > 0
        for mode in MODES:
            rt.bake_texels(BW, BH, mode, DIRS, ns=NS, dilate=DILATE, bias=1e-3, max_dist=max_dist_of("M1"))
            assert rt.last_bake_ms() > 0 and rt.last_texels_ms() > 0
        rt.raster_texels(37, 23, 3)
        assert seen() == was
        g_after = rt.gather_radiance(pos, nrm, GR.IRRADIANCE, DIRS, ns=NS, bias=1e-3, rays=True)
        for k in range(2):
            same(g_after[k], g_before[k], "gatherRadiance around the bakes")
        assert np.array_equal(g_after[2], g_before[2])
        rt.runRendererProgressive(2, 8, 8)
        assert rt.progressive_samples() == 4
    finally:
        rt.cleanupRenderer()


# ---- 7. misuse ------------------------------------------------------------------------------------------------------------------------------

_INIT = ("import sys; sys.path.insert(0, %r); import pixels_reference as PR\n" % os.path.join(ROOT, "tests") +
         "PR.init(rt, 'M1'); r = rt.load_renderer(); fp = C.POINTER(C.c_float); ip = C.POINTER(C.c_int32)\n"
         "out = np.zeros((8, 8, 27), np.float32); prim = np.zeros((8, 8), np.int32)\n"
         "B = lambda **kw: rt.bake_texels(kw.pop('W', 8), kw.pop('H', 8), kw.pop('mode', 0), kw.pop('dirs', 4), **kw)\n")
_SPHERES = ("import sys; sys.path.insert(0, %r); import pixels_reference as PR\n" % os.path.join(ROOT, "tests") + "PR.init(rt, 'S1')\n")


@pytest.mark.parametrize("body", [
    _SPHERES + "rt.raster_texels(8, 8)", _SPHERES + "rt.bake_texels(8, 8, 2, 4)",                                       # a sphere scene
    _INIT + "r.rasterTexels(0, 8, 0, prim.ctypes.data_as(ip), None, None, None, None)",                                 # W, H, dilate out of range
    _INIT + "r.rasterTexels(8, 8193, 0, prim.ctypes.data_as(ip), None, None, None, None)",
    _INIT + "r.rasterTexels(8, 8, -1, prim.ctypes.data_as(ip), None, None, None, None)",
    _INIT + "r.rasterTexels(8, 8, 17, prim.ctypes.data_as(ip), None, None, None, None)",
    _INIT + "r.rasterTexels(8, 8, 0, None, None, None, None, None)",                                                    # all planes NULL
    _INIT + "r.bakeTexels(8, 8, 0, 2, 0, 4, 4, 1, 0, 0.0, 0.0, None, None, None, prim.ctypes.data_as(ip), None)",
    _INIT + "r.bakeTexels(8193, 8, 0, 2, 0, 4, 4, 1, 0, 0.0, 0.0, None, out.ctypes.data_as(fp), None, None, None)",
    _INIT + "r.bakeTexels(8, 0, 0, 2, 0, 4, 4, 1, 0, 0.0, 0.0, None, out.ctypes.data_as(fp), None, None, None)",
    _INIT + "r.bakeTexels(8, 8, 17, 2, 0, 4, 4, 1, 0, 0.0, 0.0, None, out.ctypes.data_as(fp), None, None, None)",
    _INIT + "r.bakeTexels(8, 8, 0, 3, 0, 4, 4, 1, 0, 0.0, 0.0, None, out.ctypes.data_as(fp), None, None, None)",        # what gatherRadiance refuses: unknown mode
    _INIT + "B(dirs=0)", _INIT + "B(first=-1, acc=out[:, :, :3])", _INIT + "B(first=2, dirs_total=5, acc=out[:, :, :3])", _INIT + "B(dirs=65537)",
    _INIT + "r.bakeTexels(8, 8, 0, 0, 1, 4, 5, 1, 0, 0.0, 0.0, None, out.ctypes.data_as(fp), None, None, None)",        # first > 0 without acc
    _INIT + "B(bias=float('inf'))", _INIT + "B(max_dist=float('nan'))", _INIT + "B(max_dist=-1.0, mode=2)",
    _INIT + "B(ns=0)", _INIT + "B(ns=65537, mode=1)",
    _INIT + "rt.setRenderOptions(rt.getDefaultRenderOptions(False), rng=rt.RT_RNG_COUNTER); B()",
    _INIT + "rt.setRenderOptions(rt.getDefaultRenderOptions(False), variant=1); B()",
], ids=lambda body: ("spheres: " if body.startswith(_SPHERES) else "") + body.rsplit("\n", 1)[-1][:70])
def test_misuse_exits_99(body):
    exits_99(body + "\n")


def test_what_misuse_does_not_cover_is_accepted(rt, meshes):
    """The edges of the checks from the inside: the largest dilation, ns ignored by VISIBILITY, a 1 x 1 atlas, and an atlas no triangle covers - 0 owned
    texels, every plane zero, src all -1."""
    base = meshes["M1"].tris.copy()
    init(rt, meshes, "M1")
    try:
        a = rt.bake_texels(1, 1, GR.VISIBILITY, 4, ns=-5, dilate=16, rays=True)
        parked = base.copy()
        parked["texCoords"] = TR.PARKED
        rt.update_triangles(0, parked)
        b = rt.bake_texels(9, 7, GR.IRRADIANCE, 4, dilate=3, rays=True)
        rt.update_triangles(0, base)
    finally:
        rt.cleanupRenderer()
    assert a[0] in (0, 1) and a[1]["out"].shape == (1, 1, 1)
    assert b[0] == 0 and (b[1]["prim"] == TR.PRIM_NONE).all() and (b[1]["src"] == -1).all()
    assert (b[1]["out"] == 0).all() and (b[1]["acc"] == 0).all() and (b[1]["rays"] == 0).all()
