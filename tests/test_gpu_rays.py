"""traceRays / occludedRays (include/rt_api.h) on the GPU against the test reference (tests/rays_reference.py): every plane of every ray set bit for bit
(np.array_equal on the raw 32-bit words: no tolerance, nothing left out) and occluded byte for byte, with the sets' own bounds and with NULL bounds; the
centre rays against renderGuides on the GPU; batch sizes around the wave and the workgroup, subset masks, a batch that crosses the chunk size, options,
partitions, the three sphere scene copies, no side effects, the empty batch, two broken rays among 128 good ones, and the misuse exits."""
import numpy as np
import pytest

import guides_reference as G
import rays_reference as R
from preview_support import bits as _bits, exits_99, init_frame, same, stats_tuple as _stats_tuple

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC0FFEE                                           # a word no plane produces: a NaN payload as float, a huge id as int
SENTINEL_BYTE = 0xA5


def _planes(mesh):
    return [p for p in R.PLANES if mesh or p != "nodes"]


def _rays(rt, O, name, own):
    org, d, t_min, t_max = R.ray_set(rt, O, name)
    return (org, d, t_min, t_max) if own else (org, d, None, None)


def _check(rt, O, name, ref, own, what):
    """Both calls on the set, every plane and occluded against `ref`."""
    mesh = R.is_mesh(R.frame_of(name))
    got = rt.trace_rays(*_rays(rt, O, name, own))
    assert rt.last_rays_ms() > 0.0
    assert sorted(got) == sorted(_planes(mesh)), (what, sorted(got))
    for k in got:
        same(got[k], ref[k], f"{what}: plane {k}")
    occ = rt.occluded_rays(*_rays(rt, O, name, own))
    assert rt.last_rays_ms() > 0.0
    diff = int((occ != ref["occluded"]).sum())
    print(f"{what}: occluded, {diff} of {occ.size} bytes differ")
    assert occ.dtype == np.uint8 and np.array_equal(occ, ref["occluded"]), (what, diff)


# ---- 1. every set, both calls, own bounds and NULL bounds ------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.SETS)
def test_sets_match_the_reference(rt, O, name):
    """centre: six guide frames - the full LDS copy (random_50x37, tie_mirror), the hybrid and the global scene copy, the staircase with its textures, the
    loose triangles with the floor -, also against renderGuides of the same initialised frame on the GPU; sph_random, sph_axis, mesh_random and the edge sets
    - mesh_axis and sph_axis on the clouds (exactly-zero direction components of both signs, origins on box planes), mesh_surface and sph_surface (origins
    on a surface, t_min = 0 and a denormal), mesh_inf and sph_inf (t_max = +inf) -: see tests/test_rays_api.py for what each set holds.  Once with the set's
    t_min / t_max arrays, once with NULL for both."""
    frame = R.frame_of(name)
    init_frame(rt, O, frame)
    has_own = R.ray_set(rt, O, name)[2] is not None
    try:
        if has_own:
            _check(rt, O, name, R.reference(rt, O, name), True, name + " own bounds")
        _check(rt, O, name, R.reference(rt, O, name, own=False), False, name + " NULL bounds")
        if name.startswith("centre:"):
            mesh = R.is_mesh(frame)
            g = rt.renderGuides(rt.RT_GUIDE_NORMAL | rt.RT_GUIDE_DEPTH | rt.RT_GUIDE_PRIM | (rt.RT_GUIDE_NODES if mesh else 0))
            got = rt.trace_rays(*_rays(rt, O, name, False))
            same(got["t"], g["depth"].reshape(-1), name + " t against renderGuides")
            same(got["prim"], g["prim"].reshape(-1), name + " prim against renderGuides")
            same(got["normal"], g["normal"].reshape(-1, 3), name + " normal against renderGuides")
            if mesh:
                same(got["nodes"], g["nodes"].reshape(-1), name + " nodes against renderGuides")
    finally:
        rt.cleanupRenderer()


# ---- 2. sizes ------------------------------------------------------------------------------------------------------------------

def _sentinel_out(rt, n, mesh, extra=64):
    """Arrays of n + extra entries full of the sentinel, and their first n entries as the views a call fills."""
    big, view = {}, {}
    for name, bit, dtype, comps in rt.RAY_PLANES:
        if name == "nodes" and not mesh:
            continue
        a = np.empty((n + extra,) if comps == 1 else (n + extra, comps), dtype)
        a.view(np.uint32)[...] = SENTINEL
        big[name], view[name] = a, a[:n]
    return big, view


@pytest.mark.parametrize("name", ["sph_random:random_50x37", "mesh_random:tris300"])
def test_sizes(rt, O, name):
    """n in {1, 63, 64, 65, 1023, 1025}: below, at and above a wave, below and above the sphere kernel's 1024-ray tile (and four 256-ray workgroups of the
    mesh kernel).  The set holds 1000 rays, so the prefixes are taken of the set twice in a row (2000 rays), whose reference is the set's twice in a row.
    Every output array has 64 entries more than n, pre-filled with a sentinel: they stay untouched."""
    mesh = R.is_mesh(R.frame_of(name))
    rays = [np.concatenate([a, a]) for a in R.ray_set(rt, O, name)]
    ref = {k: np.concatenate([v, v]) for k, v in R.reference(rt, O, name).items()}
    init_frame(rt, O, R.frame_of(name))
    try:
        for n in (1, 63, 64, 65, 1023, 1025):
            big, view = _sentinel_out(rt, n, mesh)
            got = rt.trace_rays(*[a[:n] for a in rays], out=view)
            for k in _planes(mesh):
                assert got[k] is view[k]
                same(big[k][:n], ref[k][:n], f"{name} n={n}: plane {k}")
                assert np.all(_bits(big[k][n:]) == SENTINEL), (n, k)
            occ = np.full(n + 64, SENTINEL_BYTE, np.uint8)
            rt.occluded_rays(*[a[:n] for a in rays], out=occ[:n])
            assert np.array_equal(occ[:n], ref["occluded"][:n]), n
            assert np.all(occ[n:] == SENTINEL_BYTE), n
    finally:
        rt.cleanupRenderer()


# ---- 3. masks ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["sph_random:three_spheres", "mesh_random:staircase_a"])
def test_subset_masks(rt, O, name):
    """{T}, {PRIM | UV}, {NORMAL}: the other pointers are NULL; requested planes equal the reference, and arrays passed through `out` for planes that were
    not requested keep their sentinel."""
    mesh = R.is_mesh(R.frame_of(name))
    ref = R.reference(rt, O, name)
    rays = R.ray_set(rt, O, name)
    n = len(rays[0])
    init_frame(rt, O, R.frame_of(name))
    try:
        for mask, wanted in ((rt.RT_RAY_T, ["t"]), (rt.RT_RAY_PRIM | rt.RT_RAY_UV, ["prim", "uv"]), (rt.RT_RAY_NORMAL, ["normal"])):
            got = rt.trace_rays(*rays, mask=mask)
            assert sorted(got) == sorted(wanted)
            for k in wanted:
                same(got[k], ref[k], f"{name} mask {mask}: plane {k}")
            big, view = _sentinel_out(rt, n, mesh, extra=0)
            got = rt.trace_rays(*rays, mask=mask, out=view)
            assert sorted(got) == sorted(wanted)
            for k in view:
                if k in wanted:
                    same(view[k], ref[k], f"{name} mask {mask} into out: plane {k}")
                else:
                    assert np.all(_bits(view[k]) == SENTINEL), (mask, k)
    finally:
        rt.cleanupRenderer()


# ---- 4. a batch larger than a chunk ------------------------------------------------------------------------------------------------

def test_chunk_crossing(rt, O):
    """(1 << 22) + 65 rays on three_spheres - 257 distinct rays of sph_random with their own bounds, repeated: the second chunk holds 65 rays and starts in the
    middle of a repetition.  t, prim and occluded equal the repeated reference, in the caller's order."""
    name = "sph_random:three_spheres"
    n, m = rt.RT_RAY_CHUNK + 65, 257
    assert n == (1 << 22) + 65
    idx = np.arange(n) % m
    rays = [np.ascontiguousarray(a[:m][idx]) for a in R.ray_set(rt, O, name)]
    ref = R.reference(rt, O, name)
    init_frame(rt, O, "three_spheres")
    try:
        got = rt.trace_rays(*rays, mask=rt.RT_RAY_T | rt.RT_RAY_PRIM)
        ms = rt.last_rays_ms()
        occ = rt.occluded_rays(*rays)
    finally:
        rt.cleanupRenderer()
    assert ms > 0.0
    assert np.array_equal(_bits(got["t"]), _bits(ref["t"][:m])[idx])
    assert np.array_equal(got["prim"], ref["prim"][:m][idx])
    assert np.array_equal(occ, ref["occluded"][:m][idx])
    assert len(np.unique(ref["prim"][:m])) >= 3 and 0 < ref["occluded"][:m].sum() < m


# ---- 5. options and independence -----------------------------------------------------------------------------------------------------

def test_sphere_options(rt, O):
    """t_min of the options is the NULL-t_min default; FAST gives PARITY's bits; setCamera changes nothing; with stripe_rows = 8, part_rank = 1,
    part_world = 2 every ray is still answered in full."""
    name = "sph_random:random_50x37"
    fb, o, _ = init_frame(rt, O, "random_50x37")
    try:
        ref = R.reference(rt, O, name)
        rt.setRenderOptions(o, fp=rt.RT_FP_FAST)
        _check(rt, O, name, ref, True, name + " FAST")
        rt.setRenderOptions(o, fp=rt.RT_FP_PARITY, stripe_rows=8, part_rank=1, part_world=2)
        _check(rt, O, name, ref, True, name + " rank 1 of 2")
        rt.setRenderOptions(o, part_rank=0, part_world=1)
        rt.setCamera(rt.make_camera((-6, 3, 9), (0, 0.5, 0), (0, 1, 0), 30.0, 50 / 37, 0.1, 10.0))
        _check(rt, O, name, ref, True, name + " after setCamera")
        dflt = R.reference(rt, O, name, own=False)
        rt.setRenderOptions(o, t_min=0.5)
        ref_t = R.reference(rt, O, name, own=False, t_min=0.5)
        assert (_bits(ref_t["t"]) != _bits(dflt["t"])).sum() >= 20
        _check(rt, O, name, ref_t, False, name + " options t_min = 0.5")
        _check(rt, O, name, ref, True, name + " own bounds under options t_min = 0.5")       # the arrays, not the default
    finally:
        rt.cleanupRenderer()


def test_mesh_options(rt, O):
    """Toggling rt_render_options.floor on the tris300 frame moves the result between the two references and leaves occluded alone; t_min of the options;
    FAST; a partition."""
    name, name_f = "mesh_random:tris300", "mesh_random:tris300_floor"
    ref, ref_f = R.reference(rt, O, name), R.reference(rt, O, name_f)
    assert (ref_f["prim"] == R.PRIM_FLOOR).sum() >= 30 and np.array_equal(ref["occluded"], ref_f["occluded"])
    fb, o, _ = init_frame(rt, O, "tris300_floor")                   # the scene with kernel_scene.floor set; init_frame switches the option on
    try:
        _check(rt, O, name_f, ref_f, True, "floor on")
        rt.setRenderOptions(o, floor=0)
        _check(rt, O, name, ref, True, "floor off")
        rt.setRenderOptions(o, floor=1, fp=rt.RT_FP_FAST, stripe_rows=8, part_rank=1, part_world=2)
        _check(rt, O, name_f, ref_f, True, "floor on again, FAST, rank 1 of 2")
        rt.setRenderOptions(o, floor=0, fp=rt.RT_FP_PARITY, part_rank=0, part_world=1, t_min=1.5)
        ref_t = R.reference(rt, O, name, own=False, t_min=1.5)
        assert (_bits(ref_t["t"]) != _bits(R.reference(rt, O, name, own=False)["t"])).sum() >= 5
        _check(rt, O, name, ref_t, False, "options t_min = 1.5")
    finally:
        rt.cleanupRenderer()


# ---- 6. no side effects ------------------------------------------------------------------------------------------------------------

def _observed(rt, fb):
    return (_bits(fb).copy(), _stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.progressive_samples(), rt.history_frames(), rt.preview_frames(),
            rt.last_guides_ms(), rt.last_denoise_ms(), rt.last_accumulate_ms(), rt.last_preview_ms(), rt.last_display_ms())


@pytest.mark.parametrize("kind", ["spheres", "mesh"])
def test_no_side_effects(rt, O, kind):
    """After a frame, the guides and every preview pass: framebuffer bits, stats, launch report, progressive samples, the histories' frame counts and every
    other rtLast*Ms are the same before and after a traceRays + occludedRays pair.  Progressive 8 + the pair + 8 equals runRenderer(16)."""
    frame, name = ("random_50x37", "sph_random:random_50x37") if kind == "spheres" else ("staircase_a", "mesh_random:staircase_a")
    fb, o, mesh = init_frame(rt, O, frame)
    try:
        rays = R.ray_set(rt, O, name)
        rt.runRenderer(16)
        whole = np.array(fb, copy=True)
        rt.renderGuides()
        rt.denoiseFrame()
        rt.accumulateFrame()
        rt.previewFrame()
        rt.display_frame()
        before = _observed(rt, fb)
        assert before[2] and before[4] == 1 and before[5] == 1 and all(ms > 0.0 for ms in before[6:])
        rt.trace_rays(*rays)
        rt.occluded_rays(*rays)
        after = _observed(rt, fb)
        assert np.array_equal(before[0], after[0])
        assert before[1:] == after[1:]
        rt.runRendererProgressive(8)
        rt.trace_rays(*rays)
        rt.occluded_rays(*rays)
        assert rt.progressive_samples() == 8
        rt.runRendererProgressive(8)
        assert rt.progressive_samples() == 16
        assert np.array_equal(_bits(fb), _bits(whole))
    finally:
        rt.cleanupRenderer()


# ---- 7. the empty batch, the timing --------------------------------------------------------------------------------------------------

def test_empty_batch_and_timing(rt, O):
    name = "sph_random:three_spheres"
    rays = R.ray_set(rt, O, name)
    init_frame(rt, O, "three_spheres")
    try:
        assert rt.last_rays_ms() == 0.0                         # before the first call
        none = [a[:0] for a in rays]
        big, view = _sentinel_out(rt, 0, False)
        got = rt.trace_rays(*none, out=view)
        assert all(v.shape[0] == 0 for v in got.values()) and all(np.all(_bits(b) == SENTINEL) for b in big.values())
        occ = np.full(64, SENTINEL_BYTE, np.uint8)
        assert rt.occluded_rays(*none, out=occ[:0]).shape == (0,) and np.all(occ == SENTINEL_BYTE)
        assert rt.last_rays_ms() == 0.0
        rt.trace_rays(*rays)
        ms = rt.last_rays_ms()
        assert ms > 0.0
        rt.trace_rays(*none)
        rt.occluded_rays(*none)
        assert rt.last_rays_ms() == ms                          # as it was
        rt.occluded_rays(*rays)
        assert rt.last_rays_ms() > 0.0
    finally:
        rt.cleanupRenderer()


# ---- 8. isolation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", ["random_50x37", "cloud_global", "tris300"])
def test_broken_rays_do_not_disturb_the_others(rt, O, frame):
    """130 rays, ray 7 with d = (0, 0, 0) and ray 70 with a NaN origin: the call returns and the other 128 results equal the reference.  Nothing is asserted
    about the two rays themselves.  Sphere scenes: the LDS copy and the global one.  A mesh: tris300, a tree of 256 nodes and nothing larger - every box test
    of a NaN ray passes, so it visits every node."""
    name = {"random_50x37": "sph_random:random_50x37", "cloud_global": "centre:cloud_global", "tris300": "mesh_random:tris300"}[frame]
    if frame == "tris300":
        assert G.mesh_frame(rt, O, frame)["hm"].view.numBvhNodes == 256
    org, d, t_min, t_max = [None if a is None else np.array(a[:130]) for a in R.ray_set(rt, O, name)]
    ref = R.reference(rt, O, name)
    d[7] = 0.0
    org[70, 1] = np.nan
    good = np.ones(130, bool)
    good[[7, 70]] = False
    init_frame(rt, O, frame)
    try:
        got = rt.trace_rays(org, d, t_min, t_max)
        occ = rt.occluded_rays(org, d, t_min, t_max)
    finally:
        rt.cleanupRenderer()
    for k in got:
        same(got[k][good], ref[k][:130][good], f"{name} with two broken rays: plane {k}")
    assert np.array_equal(occ[good], ref["occluded"][:130][good])


# ---- 9. misuse ---------------------------------------------------------------------------------------------------------------------

_SPHERES = ("sp, mt, cam = rt.scene_random_spheres(64, 48); rt.initRendererSpheres(sp, mt, cam, 64, 48, 10)\n"
            "o = np.zeros((4, 3), np.float32); d = np.ones((4, 3), np.float32); fp = C.POINTER(C.c_float); ip = C.POINTER(C.c_int32)\n"
            "po, pd = o.ctypes.data_as(fp), d.ctypes.data_as(fp); t = np.zeros(4, np.float32); pt = t.ctypes.data_as(fp); r = rt.load_renderer()\n")
_MISUSE = {
    "negative_n": _SPHERES + "r.traceRays(-1, po, pd, None, None, rt.RT_RAY_T, pt, None, None, None, None)\n",
    "negative_n_occluded": _SPHERES + "r.occludedRays(-1, po, pd, None, None, np.zeros(4, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)))\n",
    "null_org": _SPHERES + "r.traceRays(4, None, pd, None, None, rt.RT_RAY_T, pt, None, None, None, None)\n",
    "null_dir": _SPHERES + "r.occludedRays(4, po, None, None, None, np.zeros(4, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)))\n",
    "mask_zero": _SPHERES + "rt.trace_rays(o, d, mask=0)\n",
    "unknown_bit": _SPHERES + "rt.trace_rays(o, d, mask=rt.RT_RAY_T | 32)\n",
    "null_plane": _SPHERES + "r.traceRays(4, po, pd, None, None, rt.RT_RAY_T | rt.RT_RAY_PRIM, pt, None, None, None, None)\n",
    "nodes_on_spheres": _SPHERES + "rt.trace_rays(o, d, mask=rt.RT_RAY_NODES)\n",
    "null_occluded": _SPHERES + "r.occludedRays(4, po, pd, None, None, None)\n",
    "floor_on_spheres": _SPHERES + "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); rt.trace_rays(o, d, mask=rt.RT_RAY_T)\n",
    "floor_on_spheres_occluded": _SPHERES + "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); rt.occluded_rays(o, d)\n",
    "after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.trace_rays(o, d, mask=rt.RT_RAY_T)\n",
    "last_ms_after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.last_rays_ms()\n",
}


@pytest.mark.parametrize("case", sorted(_MISUSE))
def test_misuse_exits_99(case):
    """The library's misuse convention, each case in a child process of its own: 'rt error' on stderr and exit status 99 (a clean exit of a host-side check)."""
    exits_99(_MISUSE[case])
