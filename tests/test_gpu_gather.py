"""GPU checks of gatherRadiance / rtGatherDirections (include/rt_api.h), bit for bit: the generator kernel against the numpy restatement
(tests/gather_reference.py) and the CPU twin; the irradiance and SH9 gathers against the numpy reduction of this library's radianceRays on the reference's
explicit rays (org, D, ids = g), in both fp modes and through the refill path; an anchor against the CPU oracle's one-pixel renders at the one origin where
the pinhole identity fl(T - o) = D holds for every D; the visibility gather against occludedRays; resumption by first / acc; a call that crosses the chunk;
nothing another call observes changes, scene edits are followed, and misuse is the library's exit 99 (the calls before init: tests/test_gather_api.py)."""
import functools
import os

import numpy as np
import pytest

import gather_reference as GR
import pixels_reference as PR
import radiance_reference as RR
from preview_support import bits, exits_99, same, stats_tuple

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (GR.IRRADIANCE, GR.SH9, GR.VISIBILITY)
N, DIRS, NS = 70, 11, 3


@functools.lru_cache(maxsize=None)
def points(tag):
    """70 points (no multiple of 64) in the middle 90 % of the scene's box with unnormalised random normals, read-only."""
    lo, hi = RR.scene_box(tag)
    rng = np.random.default_rng(400 + sorted(PR.SCENES).index(tag))
    pos = rng.uniform(lo, hi, (N, 3)).astype(np.float32)
    nrm = (rng.normal(size=(N, 3)) * rng.uniform(0.3, 3.0, (N, 1))).astype(np.float32)
    pos.setflags(write=False)
    nrm.setflags(write=False)
    return pos, nrm


def by_radiance_rays(rt, ns):
    """The per-ray source of the reference: this library's radianceRays on the reference's explicit rays."""
    def trace(org, D, ids):
        out, _, rays = rt.radiance_rays(org, D, ns, ids=ids, rays=True)
        return out, rays
    return trace


def by_occluded_rays(rt, max_dist):
    def trace(org, D, ids):
        occ = rt.occluded_rays(org, D, t_max=None if max_dist == 0 else np.full(len(org), max_dist, np.float32))
        return np.where(occ != 0, np.float32(0), np.float32(1)), np.zeros(len(org), np.uint32)
    return trace


def check(got, ref, what):
    (out, acc, rays), (ref_out, ref_acc, ref_rays) = got, ref
    assert out.shape == ref_out.shape and acc.shape == ref_acc.shape
    same(out, ref_out, what + ": out")
    same(acc, ref_acc, what + ": acc")
    assert np.array_equal(rays, ref_rays), (what, int((rays != ref_rays).sum()))


# ---- 1. the generator kernel ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_generator_equals_numpy_and_the_host_twin(rt, mode):
    pos, nrm = GR.standard_points()
    nrm_arg = None if mode == GR.SH9 else nrm
    PR.init(rt, "S1")
    try:
        got = {(b, bias): rt.gather_directions(pos, nrm_arg, mode, 9, first=3, dirs_total=16, base_id=b, bias=bias)
               for b in (0, 17, 0xFFFFFFF0) for bias in (0.0, 1e-3)}
    finally:
        rt.cleanupRenderer()
    for (b, bias), (org, d, ids) in got.items():
        ref_o, ref_d, ref_ids = GR.directions(pos, nrm, mode, 3, 9, 16, b, bias)
        h_o, h_d, h_ids = rt.gather_directions_host(pos, nrm_arg, mode, 9, first=3, dirs_total=16, base_id=b, bias=bias)
        what = f"mode {mode} base {b} bias {bias}"
        assert np.array_equal(ids, ref_ids) and np.array_equal(ids, h_ids), what
        same(org, ref_o, what + ": origins against numpy")
        same(d, ref_d, what + ": directions against numpy")
        same(org, h_o, what + ": origins against the host twin")
        same(d, h_d, what + ": directions against the host twin")


def test_generator_writes_only_what_is_asked(rt):
    import ctypes as C
    pos, nrm = GR.standard_points()
    _, ref_d, ref_ids = GR.directions(pos, nrm, GR.VISIBILITY, 0, 5, 5, 9, 0.5)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    p = lambda a, t: a.ctypes.data_as(t)
    d, ids = np.zeros((N * 5, 3), np.float32), np.zeros(N * 5, np.uint32)
    PR.init(rt, "S1")
    try:
        r = rt.load_renderer()
        r.rtGatherDirections(N, p(pos, fp), p(nrm, fp), GR.VISIBILITY, 0, 5, 5, 9, 0.5, None, p(d, fp), None)
        r.rtGatherDirections(N, p(pos, fp), p(nrm, fp), GR.VISIBILITY, 0, 5, 5, 9, 0.5, None, None, p(ids, up))
    finally:
        rt.cleanupRenderer()
    same(d, ref_d, "dir alone")
    assert np.array_equal(ids, ref_ids)


# ---- 2. irradiance and SH9 against the numpy reduction of radianceRays ----------------------------------------------------------------

@pytest.mark.parametrize("fp", ["parity", "fast"])
@pytest.mark.parametrize("tag", ["S1", "S2", "M1", "M2_floor"])
def test_radiance_modes_equal_the_reduction_of_radiance_rays(rt, monkeypatch, tag, fp):
    """Same kernel, same inputs - the chunk's batch is entry for entry the reference's list -: bit for bit in PARITY and in FAST; then again through the refill
    path.  PARITY: RT_PIXELS_WAVES = 2, 770 rays through two waves, against the uncapped reference - a ray's bits do not depend on who traces it.  FAST makes no
    such promise (its bits depend on which rays share a wave, and two waves race for the queue): there the cap is one wave - a fixed schedule - for the
    reference's radianceRays and for the gather alike."""
    pos, nrm = points(tag)
    PR.init(rt, tag, **({"fp": rt.RT_FP_FAST} if fp == "fast" else {}))
    try:
        for mode, base_id, bias in ((GR.IRRADIANCE, 5, 1e-3), (GR.SH9, 1000, 0.0)):
            nrm_arg = None if mode == GR.SH9 else nrm
            ref = GR.gather(pos, nrm, mode, 0, DIRS, DIRS, by_radiance_rays(rt, NS), base_id, bias)
            got = rt.gather_radiance(pos, nrm_arg, mode, DIRS, ns=NS, base_id=base_id, bias=bias, rays=True)
            ms = rt.last_gather_ms()
            print(tag, fp, "mode", mode, "kernel ms", ms, "mean out", float(got[0].mean()), "rays", int(got[2].sum()))
            check(got, ref, f"{tag} {fp} mode {mode}")
            assert ms > 0.0 and np.isfinite(got[0]).all() and (got[2] >= DIRS * NS).all() and (got[0] != 0).any()
            monkeypatch.setenv("RT_PIXELS_WAVES", "1" if fp == "fast" else "2")
            if fp == "fast":
                ref = GR.gather(pos, nrm, mode, 0, DIRS, DIRS, by_radiance_rays(rt, NS), base_id, bias)
            capped = rt.gather_radiance(pos, nrm_arg, mode, DIRS, ns=NS, base_id=base_id, bias=bias, rays=True)
            monkeypatch.delenv("RT_PIXELS_WAVES")
            check(capped, ref, f"{tag} {fp} mode {mode}, through the refill path")
    finally:
        rt.cleanupRenderer()


# ---- 3. the oracle anchor ------------------------------------------------------------------------------------------------------------

def _free_origin_scene(rt):
    """A ground sphere below y = -0.5 and six spheres of the three materials around the origin, which lies in free space."""
    centres = [(0, -100.5, 0), (1.5, 0, 0), (-1.5, 0, 0), (0, 0, 1.5), (0, 0, -1.5), (0, 1.6, 0), (1.1, 0.9, -1.1)]
    radii = [100, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    kinds = [(rt.RT_DIFFUSE, (0.5, 0.5, 0.5), 0.0), (rt.RT_DIFFUSE, (0.8, 0.3, 0.2), 0.0), (rt.RT_METAL, (0.8, 0.8, 0.9), 0.2), (rt.RT_GLASS, (1, 1, 1), 1.5),
             (rt.RT_DIFFUSE, (0.2, 0.4, 0.8), 0.0), (rt.RT_METAL, (0.9, 0.6, 0.2), 0.0), (rt.RT_GLASS, (1, 1, 1), 1.3)]
    sp, mt = np.zeros(7, rt.sphere_dtype), np.zeros(7, rt.material_dtype)
    sp["center"], sp["radius"] = centres, radii
    for k, (t, col, param) in enumerate(kinds):
        mt[k] = (t, col, param, -1)
    assert (np.linalg.norm(sp["center"].astype(np.float64), axis=1) > sp["radius"] + 0.4).all()     # no sphere contains the origin, or comes near it
    return sp, mt


@pytest.mark.parametrize("mode", [GR.IRRADIANCE, GR.SH9])
def test_oracle_anchor_at_the_origin(rt, O, mode):
    """The pinhole identity fl(T - o) = D holds for every D only at o = 0: 24 points there with different normals, bias 0, so that ray (0, D, g) is the pixel g
    of the oracle's frame through the pinhole at 0 towards D.  Per-ray L and rays from the oracle, reduced in numpy, against gatherRadiance in PARITY."""
    sp, mt = _free_origin_scene(rt)
    rng = np.random.default_rng(31)
    pos = np.zeros((24, 3), np.float32)
    nrm = (rng.normal(size=(24, 3)) * rng.uniform(0.5, 2.0, (24, 1))).astype(np.float32)
    depth, dirs, ns, base_id = 50, 5, 2, 3
    org_ref, D_ref, g = GR.directions(pos, nrm, mode, 0, dirs, dirs, base_id, 0.0)
    assert not np.signbit(D_ref[D_ref == 0]).any() and (org_ref == 0).all() and not np.signbit(org_ref).any()     # conditions on the inputs
    sc, opt = O.sphere_scene(sp, mt), O.default_options(True)

    def by_oracle(org, D, ids):
        return RR.oracle_rays_in(sc, opt, depth, org, D, ids, ns)

    ref = GR.reduce(mode, 0, dirs, D_ref, *by_oracle(org_ref, D_ref, g))
    rt.initRendererSpheres(sp, mt, rt.make_camera((3, 2, 3), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 4.0), 8, 8, depth)
    try:
        got = rt.gather_radiance(pos, None if mode == GR.SH9 else nrm, mode, dirs, ns=ns, base_id=base_id, rays=True)
    finally:
        rt.cleanupRenderer()
    check(got, ref, f"mode {mode} against the oracle")
    assert (got[2] > dirs * ns).any() and len(np.unique(bits(got[0]), axis=0)) > 12             # paths bounce, the points differ


# ---- 4. visibility -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["S1", "M1"])
def test_visibility_equals_the_reduction_of_occluded_rays(rt, tag):
    pos, nrm = points(tag)
    lo, hi = RR.scene_box(tag)
    finite = float(np.float32(0.15 * np.linalg.norm(hi - lo)))
    PR.init(rt, tag)
    try:
        res = {}
        for max_dist in (0.0, finite):
            ref = GR.gather(pos, nrm, GR.VISIBILITY, 0, DIRS, DIRS, by_occluded_rays(rt, max_dist), 7, 1e-3)
            got = rt.gather_radiance(pos, nrm, GR.VISIBILITY, DIRS, ns=0, base_id=7, bias=1e-3, max_dist=max_dist, rays=True)      # (ns is ignored)
            check(got, ref, f"{tag} max_dist {max_dist}")
            assert got[0].shape == (N, 1) and (got[2] == 0).all() and (got[0] >= 0).all() and (got[0] <= 1).all()
            same(got[0], got[1] / np.float32(DIRS), "out = acc / M")
            res[max_dist] = got[0]
        print(tag, "openness", float(res[0.0].mean()), "within", finite, float(res[finite].mean()))
    finally:
        rt.cleanupRenderer()
    assert (res[finite] >= res[0.0]).all() and (res[finite] > res[0.0]).any()                   # the bound matters: nearer occluders only
    assert len(np.unique(res[finite])) > 2                                                      # (M1 is a closed room: without a bound nothing is open)


# ---- 5. a split equals the whole -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["S2", "M1"])
@pytest.mark.parametrize("mode", MODES)
def test_split_equals_one_call(rt, tag, mode):
    pos, nrm = points(tag)
    nrm_arg = None if mode == GR.SH9 else nrm
    lo, hi = RR.scene_box(tag)
    base = dict(ns=2, base_id=11, bias=1e-3, max_dist=float(np.float32(0.15 * np.linalg.norm(hi - lo))), rays=True)      # (a bound: M1 is a closed room)
    kw = dict(base, dirs_total=16)
    PR.init(rt, tag)
    try:
        one = rt.gather_radiance(pos, nrm_arg, mode, 16, **kw)
        part = rt.gather_radiance(pos, nrm_arg, mode, 5, **kw)
        rest = rt.gather_radiance(pos, nrm_arg, mode, 11, first=5, acc=part[1], **kw)
        alone = rt.gather_radiance(pos, nrm_arg, mode, 5, **base)                               # dirs_total = 5: other ids from the second point on
    finally:
        rt.cleanupRenderer()
    same(rest[0], one[0], f"{tag} mode {mode}: (0, 5) then (5, 11) against (0, 16), out")
    same(rest[1], one[1], f"{tag} mode {mode}: acc")
    assert np.array_equal(part[2].astype(np.uint64) + rest[2], one[2])
    same(part[0], part[1] / np.float32(5) if mode != GR.SH9 else (part[1] * np.float32(12.566371)) / np.float32(5), "the part's out is over its own M")
    assert (bits(part[1]) != bits(one[1])).any()
    same(alone[1][:1], part[1][:1], "point 0 does not depend on dirs_total")
    assert (bits(alone[1][1:]) != bits(part[1][1:])).any()


# ---- 6. across the chunk -------------------------------------------------------------------------------------------------------------

def test_chunk_crossing(rt):
    """n = 70 at dirs = dirs_total = RT_GATHER_MAX_DIRS: 64 points per chunk, two chunks, 4.6 M rays at one sample on S2.  Point k is the index in the caller's
    list: the second chunk's ids go on from 64 * 65536."""
    dirs = rt.RT_GATHER_MAX_DIRS
    assert rt.RT_RAY_CHUNK // dirs == 64 < N
    pos, nrm = points("S2")
    PR.init(rt, "S2")
    try:
        got = rt.gather_radiance(pos, nrm, GR.IRRADIANCE, dirs, ns=1, bias=1e-3, rays=True)
        ms = rt.last_gather_ms()
        ref = GR.gather(pos, nrm, GR.IRRADIANCE, 0, dirs, dirs, by_radiance_rays(rt, 1), 0, 1e-3)
    finally:
        rt.cleanupRenderer()
    print("rays", N * dirs, "kernel ms", ms)
    check(got, ref, "two chunks")
    assert ms > 0.0 and len(np.unique(bits(got[0][64:]), axis=0)) == N - 64


# ---- 7. leaves everything else alone, follows the scene ------------------------------------------------------------------------------

def test_changes_nothing_another_call_observes(rt, O):
    pos, nrm = points("S2")
    org, _, d = RR.standard_list("S2")
    ij, _ = PR.standard_list("S2")
    fb = PR.init(rt, "S2")
    try:
        rt.runRenderer(8, 8, 8)
        rt.renderGuides()
        rt.trace_rays(*rt.centre_rays(PR.scene(rt, "S2")["cam"], 64, 48, ij[:100]))
        rt.render_pixels(ij[:200], 2)
        rad_out, rad_state, _ = rt.radiance_rays(org[:300], d[:300], 2)
        rt.denoiseFrame()                                   # every pass and query that has a timer of its own has run once: the timers are not 0 ...
        rt.accumulateFrame()
        rt.previewFrame()
        rt.display_frame()
        rt.renderMotion()
        assert rt.refine_frame(2, 2, 8, 0.05, want=())[0] > 0
        rt.runRendererProgressive(2, 8, 8)
        seen = lambda: (bits(np.array(fb, copy=True)).tobytes(), stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.last_sphere_form(),
                        rt.progressive_samples(), rt.last_rays_ms(), rt.last_guides_ms(), rt.last_pixels_ms(), rt.last_radiance_ms(),
                        rt.last_denoise_ms(), rt.last_accumulate_ms(), rt.last_preview_ms(), rt.last_display_ms(), rt.last_motion_ms(),
                        rt.last_refine_ms(), rt.last_update_ms(), rt.last_rebuild_ms(), rt.history_frames(), rt.preview_frames())
        was = seen()
        assert was[4] == 2 and all(x > 0 for x in was[5:15]) and was[15:] == (0.0, 0.0, 1, 1)    # (... but those of the scene edits, which this test does not make)
        for mode in MODES:
            rt.gather_radiance(pos, nrm, mode, DIRS, ns=2)
            assert rt.last_gather_ms() > 0
        rt.gather_directions(pos, nrm, GR.IRRADIANCE, DIRS)
        assert seen() == was
        # radianceRays resumes from its own state as if nothing had happened, and so does the progressive frame
        more, _, _ = rt.radiance_rays(org[:300], d[:300], 2, first=np.full(300, 2, np.int32), state=rad_state)
        same(more, rt.radiance_rays(org[:300], d[:300], 4)[0], "radianceRays continued around the gathers")
        rt.runRendererProgressive(2, 8, 8)
        assert rt.progressive_samples() == 4
        same(np.array(fb, copy=True), PR.oracle_frame(rt, O, "S2", 4)[0], "the progressive frame after 2 + 2 samples around the gathers")
    finally:
        rt.cleanupRenderer()


def test_follows_update_spheres(rt):
    pos, nrm = points("S2")
    s = PR.scene(rt, "S2")
    sp2, mt2 = s["sp"].copy(), s["mt"].copy()
    sp2["center"][1:40, 1] += 0.35                          # lift a few dozen spheres, recolour them (tests/test_gpu_radiance.py)
    mt2["color"][1:40] = mt2["color"][1:40][:, ::-1]
    PR.init(rt, "S2")
    try:
        before = rt.gather_radiance(pos, nrm, GR.IRRADIANCE, DIRS, ns=NS, bias=1e-3, rays=True)
        rt.update_spheres(sp2, mt2)
        ref = GR.gather(pos, nrm, GR.IRRADIANCE, 0, DIRS, DIRS, by_radiance_rays(rt, NS), 0, 1e-3)
        got = rt.gather_radiance(pos, nrm, GR.IRRADIANCE, DIRS, ns=NS, bias=1e-3, rays=True)
    finally:
        rt.cleanupRenderer()
    check(got, ref, "after updateSpheres")
    assert (bits(got[0]) != bits(before[0])).any(axis=1).mean() > 0.02


# ---- 8. misuse -----------------------------------------------------------------------------------------------------------------------

_INIT = ("import sys; sys.path.insert(0, %r); import pixels_reference as PR\n" % os.path.join(ROOT, "tests") +
         "PR.init(rt, 'S1'); r = rt.load_renderer(); pos = np.zeros((4, 3), np.float32); nrm = np.ones((4, 3), np.float32)\n"
         "fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32); p = lambda a: a.ctypes.data_as(fp); out = np.zeros((4, 27), np.float32)\n"
         "G = lambda **kw: rt.gather_radiance(pos, nrm, kw.pop('mode', 0), kw.pop('dirs', 4), **kw)\n")


@pytest.mark.parametrize("body", [
    "r.gatherRadiance(-1, p(pos), p(nrm), 0, 0, 4, 4, 1, 0, 0.0, 0.0, None, p(out), None)",                              # n < 0
    "r.gatherRadiance(4, None, p(nrm), 0, 0, 4, 4, 1, 0, 0.0, 0.0, None, p(out), None)",                                # pos NULL
    "r.gatherRadiance(4, p(pos), None, 0, 0, 4, 4, 1, 0, 0.0, 0.0, None, p(out), None)",                                # nrm NULL outside SH9
    "r.gatherRadiance(4, p(pos), None, 2, 0, 4, 4, 1, 0, 0.0, 0.0, None, p(out), None)",
    "r.gatherRadiance(4, p(pos), p(nrm), 3, 0, 4, 4, 1, 0, 0.0, 0.0, None, p(out), None)",                              # unknown mode
    "G(dirs=0)", "G(first=-1, acc=out[:, :3])", "G(first=2, dirs_total=5, acc=out[:, :3])", "G(dirs=65537)",
    "r.gatherRadiance(4, p(pos), p(nrm), 0, 1, 4, 5, 1, 0, 0.0, 0.0, None, p(out), None)",                              # first > 0 without acc
    "r.gatherRadiance(4, p(pos), p(nrm), 0, 0, 4, 4, 1, 0, 0.0, 0.0, None, None, None)",                                # all outputs NULL
    "G(bias=float('inf'))", "G(max_dist=float('nan'))", "G(max_dist=-1.0, mode=2)",
    "G(ns=0)", "G(ns=65537, mode=1)",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), rng=rt.RT_RNG_COUNTER); G()",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), variant=1); G()",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), nee=1); G(mode=1)",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); G(mode=2)",                                        # every mode: the floor on a sphere scene
    "r.rtGatherDirections(4, p(pos), p(nrm), 0, 0, 4, 4, 0, 0.0, None, None, None)",
    "rt.gather_directions(pos, nrm, 0, 4, bias=float('nan'))",
])
def test_misuse_exits_99(body):
    exits_99(_INIT + body + "\n")


def test_what_misuse_does_not_cover_is_accepted(rt):
    """The edges of the checks from the inside: dirs_total = RT_GATHER_MAX_DIRS with two directions of it, ns ignored by VISIBILITY, max_dist = +inf as no bound,
    an empty list that writes nothing and leaves rtLastGatherMs as it was."""
    import ctypes as C
    pos, nrm = (np.ascontiguousarray(a[:3]) for a in points("S1"))
    PR.init(rt, "S1")
    try:
        a = rt.gather_radiance(pos, nrm, GR.IRRADIANCE, 2, first=65534, dirs_total=65536, acc=np.zeros((3, 3), np.float32), rays=True)
        b = rt.gather_radiance(pos, nrm, GR.VISIBILITY, 4, ns=-5, max_dist=float("inf"))
        c = rt.gather_radiance(pos, nrm, GR.VISIBILITY, 4)
        before = rt.last_gather_ms()
        out = np.full((3, 3), 7.0, np.float32)
        fp = C.POINTER(C.c_float)
        rt.load_renderer().gatherRadiance(0, pos.ctypes.data_as(fp), nrm.ctypes.data_as(fp), 0, 0, 4, 4, 1, 0, 0.0, 0.0, None, out.ctypes.data_as(fp), None)
        assert (out == 7.0).all() and rt.last_gather_ms() == before and before > 0
    finally:
        rt.cleanupRenderer()
    same(a[0], a[1] / np.float32(65536), "out over M = first + dirs")
    same(b[0], c[0], "max_dist = +inf is no bound")
