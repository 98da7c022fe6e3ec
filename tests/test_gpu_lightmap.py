"""GPU checks of sampleTexels / renderLightmap (include/rt_api.h, "sampling texels"), bit for bit: the lookup against the CPU twin and the numpy restatement
(tests/lightmap_reference.py) over the first hits of every pixel's centre ray and the synthetic edge list, in both fp modes; the frame against the numpy
composition of renderGuides' albedo plane, traceRays' planes and the lookup; a bake and a filtered bake read where they lie against the downloaded planes;
both calls through updateTriangles and rebuildBvh; nothing another call observes changes; misuse is the library's exit 99 (the calls before init:
tests/test_lightmap_api.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import gather_reference as GR
import lightmap_reference as LR
import pixels_reference as PR
import texels_reference as TR
from preview_support import bits, exits_99, same
from texels_support import init, max_dist_of, private_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW, BH, DIRS, NS, DILATE = 24, 16, 5, 2, 2
ATLASES = ((37, 23), (64, 64), (1, 1), (1, 5))


@pytest.fixture(scope="module")
def meshes(rt, tmp_path_factory):
    """M1 and M2_floor with rtAtlasGrid UVs, read-only: a test that edits a mesh takes a private_mesh of its own."""
    return {tag: private_mesh(rt, tag, tmp_path_factory.mktemp("lightmap")) for tag in ("M1", "M2_floor")}


def first_hits(rt, tag):
    """traceRays over rtCentreRays of every pixel of the tag's image, pixel id = row * nx + column: the dict of planes."""
    s = PR.scene(rt, tag)
    nx, ny = s["nx"], s["ny"]
    ij = np.stack(np.meshgrid(np.arange(nx), np.arange(ny)), axis=-1).reshape(-1, 2).astype(np.int32)
    org, d = rt.centre_rays(s["cam"], nx, ny, ij)
    return rt.trace_rays(org, d, mask=rt.RT_RAY_T | rt.RT_RAY_PRIM | rt.RT_RAY_NORMAL | rt.RT_RAY_UV)


def check_frame(rt, tag, tris, W, H, mode, planes, flags, floor_value, what, hits=None, source=None):
    """renderLightmap now against the composition over `tris`, the triangles the device holds.  `source`: the flags to call with in place of the planes."""
    s = PR.scene(rt, tag)
    hits = first_hits(rt, tag) if hits is None else hits
    albedo = rt.renderGuides(rt.RT_GUIDE_ALBEDO)["albedo"]
    shape = (s["ny"], s["nx"])
    ref = LR.compose(albedo, hits["prim"].reshape(shape), hits["uv"].reshape(shape + (2,)), hits["normal"].reshape(shape + (3,)), tris, W, H, mode, planes,
                     flags, floor_value)
    got = rt.render_lightmap(W, H, mode, planes if source is None else None, flags | (source or 0), floor_value)
    ms = rt.last_lightmap_ms()
    print(what, f"{W} x {H} mode {mode} flags {flags} floor {floor_value}: kernel ms", ms)
    same(got, ref, what)
    assert ms > 0.0
    return got, hits


# ---- 1. the lookup against the twin and numpy ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp", ["parity", "fast"])
@pytest.mark.parametrize("tag", ["M1", "M2_floor"])
def test_sample_texels_equals_the_twin_and_numpy(rt, meshes, tag, fp):
    tris = meshes[tag].tris.copy()
    assert np.isinf(tris["v"][:, 0, 0]).any()                                                      # (the leaf padding: a sentinel slot to name)
    init(rt, meshes, tag, **({"fp": rt.RT_FP_FAST} if fp == "fast" else {}))
    try:
        h = first_hits(rt, tag)
        e_prim, e_uv, e_nrm = LR.edge_hits(tris, 77)
        prim, uv, nrm = np.concatenate([h["prim"], e_prim]), np.concatenate([h["uv"], e_uv]), np.concatenate([h["normal"], e_nrm])
        assert (h["prim"] >= 0).any() and (tag != "M2_floor" or ((h["prim"] == LR.PRIM_NONE).any() and (h["prim"] == LR.PRIM_FLOOR).any()))
        for W, H in ATLASES:
            for C_ in (1, 3, 27):
                planes = LR.random_planes(W, H, C_, 5 + C_)
                for flags in (0, LR.BILINEAR):
                    what = f"{tag} {fp} {W} x {H} C {C_} flags {flags}"
                    count, out, valid = rt.sample_texels(prim, uv, nrm if C_ == 27 else None, W, H, LR.MODE_OF[C_], planes, flags)
                    ms = rt.last_sample_ms()
                    t_count, twin, t_valid = rt.sample_texels_host(tris, prim, uv, nrm if C_ == 27 else None, W, H, LR.MODE_OF[C_], planes, flags)
                    ref, ok = LR.lookup(tris, prim, uv, nrm, W, H, LR.MODE_OF[C_], planes, bool(flags))
                    assert count == t_count == int(ok.sum()) and np.array_equal(valid, ok) and np.array_equal(t_valid, ok), what
                    same(out, twin, what + ": against the host twin")
                    same(out, ref, what + ": against numpy")
                    assert ms > 0.0 and 0 < count < len(prim)
        assert rt.sample_texels(prim[:0], uv[:0], None, 8, 8, 0, np.zeros((8, 8, 3), np.float32))[0] == 0     # n == 0
    finally:
        rt.cleanupRenderer()


# ---- 2. the frame against the composition ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp", ["parity", "fast"])
def test_render_lightmap_of_a_textured_scene(rt, fp):
    """M1_tex under its own UVs, which leave [0, 1]^2: a textured albedo and a wrapped texture are met, and the lookup clamps where the texture wraps."""
    s = PR.scene(rt, "M1_tex")
    tris = s["hm"].tris.copy()
    PR.init(rt, "M1_tex", **({"fp": rt.RT_FP_FAST} if fp == "fast" else {}))
    try:
        hits = first_hits(rt, "M1_tex")
        p = hits["prim"]
        hit = p >= 0
        textured = hit & (s["mats"]["texId"][tris["meshID"][np.where(hit, p, 0)]] != -1)
        tcu, tcv = LR.atlas_point(tris["texCoords"][np.where(hit, p, 0)], hits["uv"][:, 0], hits["uv"][:, 1])
        wrapped = textured & ((tcu < 0) | (tcu >= 1) | (tcv < 0) | (tcv >= 1))
        print("textured pixels", int(textured.sum()), "of them wrapped", int(wrapped.sum()), "of", len(p))
        assert textured.any() and wrapped.any() and (hit & ~textured).any()
        for W, H, C_, flags in ((37, 23, 3, LR.ALBEDO), (37, 23, 3, 0), (37, 23, 27, LR.ALBEDO | LR.BILINEAR), (64, 64, 1, LR.ALBEDO | LR.BILINEAR),
                                (1, 5, 27, LR.BILINEAR), (1, 1, 1, LR.ALBEDO)):
            planes = LR.random_planes(W, H, C_, 9 + C_) + np.float32(0.5 if C_ != 27 else 0.0)
            got, _ = check_frame(rt, "M1_tex", tris, W, H, LR.MODE_OF[C_], planes, flags, None, f"M1_tex {fp}", hits=hits)
            assert np.isfinite(got).all() and (got != 0).any()
        plain = rt.render_lightmap(37, 23, 0, np.ones((23, 37, 3), np.float32))
        lit = rt.render_lightmap(37, 23, 0, np.ones((23, 37, 3), np.float32), LR.ALBEDO)
        same(lit, rt.renderGuides(rt.RT_GUIDE_ALBEDO)["albedo"], "planes of ones with the albedo: the albedo plane")
        assert (bits(plain) != bits(lit)).any()
    finally:
        rt.cleanupRenderer()


@pytest.mark.parametrize("fp", ["parity", "fast"])
def test_render_lightmap_with_the_floor_and_the_sky(rt, meshes, fp):
    tris = meshes["M2_floor"].tris.copy()
    init(rt, meshes, "M2_floor", **({"fp": rt.RT_FP_FAST} if fp == "fast" else {}))
    try:
        hits = first_hits(rt, "M2_floor")
        p = hits["prim"]
        assert (p >= 0).any() and (p == LR.PRIM_FLOOR).any() and (p == LR.PRIM_NONE).any()
        frames = []
        for W, H, C_, flags, fv in ((37, 23, 3, LR.ALBEDO, None), (37, 23, 3, LR.ALBEDO, (0.25, 0.5, 2.0)), (37, 23, 27, LR.BILINEAR, (0.25, 0.5, 2.0)),
                                    (64, 64, 1, LR.BILINEAR, None), (1, 5, 3, LR.ALBEDO | LR.BILINEAR, (3.0, 0.0, -1.0)), (1, 1, 27, 0, None)):
            planes = LR.random_planes(W, H, C_, 19 + C_)
            frames.append(check_frame(rt, "M2_floor", tris, W, H, LR.MODE_OF[C_], planes, flags, fv, f"M2_floor {fp}", hits=hits)[0])
        floor = (p == LR.PRIM_FLOOR).reshape(frames[0].shape[:2])
        assert (bits(frames[0][floor]) != bits(frames[1][floor])).any()                            # floor_value NULL against a given one
        assert (frames[3][floor] == 1).all() and (frames[2][floor] == np.float32((0.25, 0.5, 2.0))).all()
        sky = (p == LR.PRIM_NONE).reshape(floor.shape)
        same(frames[0][sky], frames[5][sky], "the sky does not depend on the planes or the flags")
    finally:
        rt.cleanupRenderer()


# ---- 3. a bake read where it lies -----------------------------------------------------------------------------------------------------------------

def test_the_device_resident_loop(rt, meshes):
    """bakeTexels, then renderLightmap(FROM_BAKE) and sampleTexels(FROM_BAKE) against the same calls on the downloaded out; after filterTexels the same with
    FROM_FILTER, whose plane a second bake of another size does not disturb."""
    tris = meshes["M1"].tris.copy()
    init(rt, meshes, "M1")
    try:
        hits = first_hits(rt, "M1")
        for mode in (GR.IRRADIANCE, GR.SH9, GR.VISIBILITY):
            _, baked = rt.bake_texels(BW, BH, mode, DIRS, ns=NS, dilate=DILATE, bias=1e-3, max_dist=max_dist_of("M1"))
            assert (baked["out"] != 0).any()
            for flags in (LR.ALBEDO, LR.BILINEAR):
                here, _ = check_frame(rt, "M1", tris, BW, BH, mode, baked["out"], flags, None, f"mode {mode}: FROM_BAKE", hits=hits, source=LR.FROM_BAKE)
                same(here, rt.render_lightmap(BW, BH, mode, baked["out"], flags), f"mode {mode}: FROM_BAKE against the downloaded out")
            a = rt.sample_texels(hits["prim"], hits["uv"], hits["normal"], BW, BH, mode, None, LR.FROM_BAKE | LR.BILINEAR)
            b = rt.sample_texels(hits["prim"], hits["uv"], hits["normal"], BW, BH, mode, baked["out"], LR.BILINEAR)
            assert a[0] == b[0] > 0 and np.array_equal(a[2], b[2])
            same(a[1], b[1], f"mode {mode}: sampleTexels FROM_BAKE against the downloaded out")
            _, filtered = rt.filter_texels(BW, BH, mode, None, dilate=DILATE, sigma_c=0.5)
            assert (bits(filtered) != bits(baked["out"])).any()
            rt.bake_texels(9, 7, GR.VISIBILITY, 2, max_dist=1.0)                                   # (the filter's plane is its own)
            for flags in (LR.ALBEDO | LR.BILINEAR, 0):
                here, _ = check_frame(rt, "M1", tris, BW, BH, mode, filtered, flags, None, f"mode {mode}: FROM_FILTER", hits=hits, source=LR.FROM_FILTER)
            a = rt.sample_texels(hits["prim"], hits["uv"], hits["normal"], BW, BH, mode, None, LR.FROM_FILTER)
            same(a[1], rt.sample_texels(hits["prim"], hits["uv"], hits["normal"], BW, BH, mode, filtered)[1], f"mode {mode}: sampleTexels FROM_FILTER")
    finally:
        rt.cleanupRenderer()


# ---- 4. the live triangles ----------------------------------------------------------------------------------------------------------------------------

def test_both_calls_follow_update_triangles_and_rebuild(rt, tmp_path):
    """The UVs moved by updateTriangles, then the real triangles permuted and shifted and rebuildBvh: both calls follow the live array both times."""
    hm = private_mesh(rt, "M1", tmp_path)
    base = hm.tris.copy()
    init(rt, {"M1": hm}, "M1")
    try:
        planes = LR.random_planes(37, 23, 3, 4) + np.float32(1.5)

        def both(tris, what):
            frame, hits = check_frame(rt, "M1", tris, 37, 23, 0, planes, LR.ALBEDO | LR.BILINEAR, None, what)
            count, out, valid = rt.sample_texels(hits["prim"], hits["uv"], None, 37, 23, 0, planes)
            ref, ok = LR.lookup(tris, hits["prim"], hits["uv"], None, 37, 23, 0, planes, False)
            assert count == int(ok.sum()) > 0 and np.array_equal(valid, ok)
            same(out, ref, what + ": sampleTexels")
            return frame
        before = both(base, "before")
        new = base.copy()
        real = np.flatnonzero(~np.isinf(new["v"][:, 0, 0]))
        new["texCoords"][real] = (np.float32(0.5) * new["texCoords"][real] + np.float32(0.25)).astype(np.float32)
        rt.update_triangles(0, new)
        moved = both(new, "after updateTriangles moved the UVs")
        assert (bits(moved) != bits(before)).any()
        rng = np.random.default_rng(71)
        new[real] = new[real][rng.permutation(len(real))]
        new["v"][real] += rng.uniform(-0.5, 0.5, (len(real), 1, 3)).astype(np.float32)
        rt.update_triangles(0, new)
        shifted = both(new, "after updateTriangles moved the triangles")
        old = rt.rebuild_bvh()
        assert (old != np.arange(len(old))).any()
        dead = int(np.flatnonzero(np.isinf(new["v"][:, 0, 0]))[0])
        rebuilt = new[np.where(old >= 0, old, dead)]               # (the device's slots: the old ones read through old_slot, a sentinel where it is -1)
        after = both(rebuilt, "after rebuildBvh")
        assert (bits(shifted) != bits(moved)).any() and np.isfinite(after).all()
    finally:
        rt.cleanupRenderer()


# ---- 5. leaves everything else alone -----------------------------------------------------------------------------------------------------------------

def test_changes_nothing_another_call_observes(rt, meshes):
    fb = init(rt, meshes, "M1")
    try:
        rt.runRenderer(1)
        frame = np.array(fb, copy=True)
        kw = dict(ns=NS, dilate=DILATE, bias=1e-3, max_dist=max_dist_of("M1"), rays=True)
        h_before = first_hits(rt, "M1")
        rt.renderGuides(rt.RT_GUIDE_ALBEDO)
        r_before = rt.raster_texels(37, 23, 3)
        b_before = rt.bake_texels(BW, BH, GR.IRRADIANCE, DIRS, **kw)
        f_before = rt.filter_texels(BW, BH, GR.IRRADIANCE, None, dilate=DILATE)
        seen = lambda: (rt.last_rays_ms(), rt.last_guides_ms(), rt.last_texels_ms(), rt.last_bake_ms(), rt.last_filter_ms())
        was = seen()
        assert min(was) > 0
        rt.render_lightmap(37, 23, GR.SH9, LR.random_planes(37, 23, 27, 1), LR.ALBEDO | LR.BILINEAR)
        rt.render_lightmap(BW, BH, GR.IRRADIANCE, None, LR.FROM_BAKE)
        rt.sample_texels(h_before["prim"], h_before["uv"], h_before["normal"], 64, 64, GR.SH9, LR.random_planes(64, 64, 27, 2), LR.BILINEAR)
        rt.sample_texels(h_before["prim"], h_before["uv"], None, BW, BH, GR.IRRADIANCE, None, LR.FROM_FILTER)
        assert rt.last_sample_ms() > 0 and rt.last_lightmap_ms() > 0 and seen() == was
        same(fb, frame, "the framebuffer around the new calls")
        f_after = rt.filter_texels(BW, BH, GR.IRRADIANCE, None, dilate=DILATE)                     # (the bake's plane is read, not written)
        r_after = rt.raster_texels(37, 23, 3)
        b_after = rt.bake_texels(BW, BH, GR.IRRADIANCE, DIRS, **kw)
        h_after = first_hits(rt, "M1")
        assert r_after[0] == r_before[0] and b_after[0] == b_before[0] and f_after[0] == f_before[0]
        same(f_after[1], f_before[1], "filterTexels of the bake around the new calls")
        for k in r_before[1]:
            same(r_after[1][k], r_before[1][k], f"rasterTexels around the new calls: {k}")
        for k in b_before[1]:
            same(b_after[1][k], b_before[1][k], f"bakeTexels around the new calls: {k}")
        for k in h_before:
            same(h_after[k], h_before[k], f"traceRays around the new calls: {k}")
    finally:
        rt.cleanupRenderer()


# ---- 6. misuse -------------------------------------------------------------------------------------------------------------------------------

_INIT = ("import sys; sys.path.insert(0, %r); import pixels_reference as PR\n" % os.path.join(ROOT, "tests") +
         "PR.init(rt, 'M1'); r = rt.load_renderer(); fp = C.POINTER(C.c_float); ip = C.POINTER(C.c_int32)\n"
         "a = np.zeros((8, 8, 27), np.float32); p = a.ctypes.data_as(fp); o = np.zeros((64, 3), np.float32); op = o.ctypes.data_as(fp)\n"
         "pr = np.zeros(4, np.int32); pp = pr.ctypes.data_as(ip); uv = np.zeros((4, 2), np.float32); up = uv.ctypes.data_as(fp)\n"
         "fr = np.zeros((32, 48, 3), np.float32); frp = fr.ctypes.data_as(C.POINTER(rt.vec3))\n"
         "S = lambda n=4, prim=pp, uv=up, nrm=op, W=8, H=8, mode=0, planes=p, flags=0, out=op: r.sampleTexels(n, prim, uv, nrm, W, H, mode, planes, flags, out, None)\n"
         "L = lambda W=8, H=8, mode=0, planes=p, flags=0, out=frp: r.renderLightmap(W, H, mode, planes, flags, None, out)\n"
         "B = lambda W=8, H=8, mode=0: rt.bake_texels(W, H, mode, 4, max_dist=1.0)\n"
         "FT = lambda W=8, H=8, mode=0: rt.filter_texels(W, H, mode, a[:, :, :3] if mode == 0 else a)\n")
_SPHERES = ("import sys; sys.path.insert(0, %r); import pixels_reference as PR\n" % os.path.join(ROOT, "tests") + "PR.init(rt, 'S1')\n")


@pytest.mark.parametrize("body", [
    _SPHERES + "rt.sample_texels([0], [[0.2, 0.2]], None, 8, 8, 0, np.zeros((8, 8, 3), np.float32))",                   # a sphere scene
    _SPHERES + "rt.render_lightmap(8, 8, 0, np.zeros((8, 8, 3), np.float32))",
    _INIT + "S(n=-1)", _INIT + "S(prim=None)", _INIT + "S(uv=None)", _INIT + "S(out=None)", _INIT + "L(out=None)",      # n < 0, NULL arrays
    _INIT + "S(mode=1, nrm=None)",                                                                                      # normal NULL in SH9
    _INIT + "S(W=0)", _INIT + "S(H=8193)", _INIT + "L(W=8193)", _INIT + "L(H=0)",                                       # the atlas size
    _INIT + "S(mode=3)", _INIT + "S(mode=-1)", _INIT + "L(mode=3)",                                                     # an unknown mode
    _INIT + "S(flags=16)", _INIT + "L(flags=16)", _INIT + "L(flags=-1)",                                                # unknown flag bits
    _INIT + "S(flags=2)",                                                                                               # RT_LIGHTMAP_ALBEDO to sampleTexels
    _INIT + "S(planes=None)", _INIT + "L(planes=None)",                                                                 # NULL without a FROM flag,
    _INIT + "B(); FT(); S(planes=None, flags=12)", _INIT + "B(); FT(); L(planes=None, flags=12)",                       # with both,
    _INIT + "B(); S(flags=4)", _INIT + "FT(); L(flags=8)",                                                              # a FROM flag with planes given,
    _INIT + "S(planes=None, flags=4)", _INIT + "L(planes=None, flags=8)",                                               # no bake / no filter yet,
    _INIT + "B(); L(planes=None, flags=8)", _INIT + "FT(); S(planes=None, flags=4)",                                    # the other call's plane,
    _INIT + "B(); S(planes=None, flags=4, W=9)", _INIT + "B(); L(planes=None, flags=4, H=7)",                           # a bake of another size,
    _INIT + "FT(); L(planes=None, flags=8, W=9)",
    _INIT + "B(mode=0); S(planes=None, flags=4, mode=2)", _INIT + "B(mode=1); L(planes=None, flags=4, mode=0)",         # of another width,
    _INIT + "FT(mode=1); S(planes=None, flags=8, mode=0)",
    _INIT + "B(); r.bakeTexels(8, 8, 0, 0, 0, 4, 4, 1, 0, 0.0, 1.0, p, None, None, None, None); L(planes=None, flags=4)",   # the last bake without out,
    _INIT + "B(); L(planes=None, flags=4); rt.cleanupRenderer(); PR.init(rt, 'M1'); L(planes=None, flags=4)",           # cleanupRenderer + init
    _INIT + "FT(); S(planes=None, flags=8); rt.cleanupRenderer(); PR.init(rt, 'M1'); S(planes=None, flags=8)",
], ids=lambda body: ("spheres: " if body.startswith(_SPHERES) else "") + body.rsplit("\n", 1)[-1][:70])
def test_misuse_exits_99(body):
    exits_99(body + "\n")


def test_what_misuse_does_not_cover_is_accepted(rt, meshes):
    """The edges of the checks from the inside: n == 0 with NULL arrays, valid NULL, normal NULL outside SH9, a bake of another mode of the same width, an
    atlas no triangle covers."""
    base = meshes["M1"].tris.copy()
    init(rt, meshes, "M1")
    try:
        r = rt.load_renderer()
        assert r.sampleTexels(0, None, None, None, 8, 8, 0, None, 0, None, None) == 0
        hits = first_hits(rt, "M1")
        planes = LR.random_planes(8, 8, 3, 1)
        out = np.zeros((len(hits["prim"]), 3), np.float32)
        fp = C.POINTER(C.c_float)
        n = r.sampleTexels(len(out), hits["prim"].ctypes.data_as(C.POINTER(C.c_int32)), hits["uv"].ctypes.data_as(fp), None, 8, 8, 0, planes.ctypes.data_as(fp),
                           1, out.ctypes.data_as(fp), None)
        assert n == int((hits["prim"] >= 0).sum()) > 0
        same(out, LR.lookup(base, hits["prim"], hits["uv"], None, 8, 8, 0, planes, True)[0], "valid NULL, normal NULL")
        rt.bake_texels(BW, BH, GR.IRRADIANCE, DIRS, ns=NS, bias=1e-3, max_dist=max_dist_of("M1"))
        a = rt.render_lightmap(BW, BH, GR.IRRADIANCE, None, LR.FROM_BAKE | LR.ALBEDO | LR.BILINEAR, (0.0, 0.0, 0.0))
        parked = base.copy()
        parked["texCoords"] = TR.PARKED
        rt.update_triangles(0, parked)
        b = rt.sample_texels(hits["prim"], hits["uv"], hits["normal"], 9, 7, GR.SH9, np.ones((7, 9, 27), np.float32), LR.BILINEAR)
        rt.update_triangles(0, base)
    finally:
        rt.cleanupRenderer()
    assert np.isfinite(a).all() and (a != 0).any()
    assert b[0] == n and np.isfinite(b[1]).all()
