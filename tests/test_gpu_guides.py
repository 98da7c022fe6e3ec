"""renderGuides (include/rt_api.h) on the GPU against the test reference (tests/guides_reference.py): every plane of every frame, all pixels, bit for bit
(np.array_equal on the raw 32-bit words: no tolerance, nothing left out); option independence, partitions, subset masks, setCamera, no side effects on
frames / stats / launch report / progressive accumulation, and the misuse exits."""
import numpy as np
import pytest

import guides_reference as R
from preview_support import bits as _bits, exits_99, init_frame, same, stats_tuple as _stats_tuple

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC0FFEE                                           # a word no plane produces: a NaN payload as float, a huge id as int


def _same(got, ref, what):
    assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        same(got[k], ref[k], f"{what}: plane {k}")


def _all_mask(rt, mesh):
    m = rt.RT_GUIDE_ALBEDO | rt.RT_GUIDE_NORMAL | rt.RT_GUIDE_DEPTH | rt.RT_GUIDE_PRIM
    return m | rt.RT_GUIDE_NODES if mesh else m


def _init_spheres(rt, name, **opts):
    return init_frame(rt, None, name, **opts)[:2] + (R.sphere_frame(rt, name),)


def _init_mesh(rt, O, name, **opts):
    return init_frame(rt, O, name, **opts)[:2] + (R.mesh_frame(rt, O, name),)


# ---- 1. sphere scenes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.SPHERE_FRAMES)
def test_sphere_frames_match_the_reference(rt, O, name):
    """Random spheres at a multiple of 8 and at 50x37, three spheres, the hybrid and the global scene copy, two coincident spheres, and a mirrored pair with equal t that the
    renderer scans in the opposite order of the caller's indices."""
    _init_spheres(rt, name)
    got = rt.renderGuides(_all_mask(rt, False))
    ms = rt.last_guides_ms()
    rt.cleanupRenderer()
    assert ms > 0.0
    _same(got, R.reference(rt, O, name), name)


# ---- 2. / 3. mesh scenes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.MESH_FRAMES)
def test_mesh_frames_match_the_reference(rt, O, name):
    """The staircase with textures, plain materials and every preset; 300 loose triangles seen from outside, without and with the floor plane."""
    _init_mesh(rt, O, name)
    got = rt.renderGuides(_all_mask(rt, True))
    rt.cleanupRenderer()
    ref = R.reference(rt, O, name)
    _same(got, ref, name)
    if name == "tris300_floor":
        assert (got["prim"] == rt.RT_GUIDE_PRIM_FLOOR).sum() == (ref["prim"] == R.PRIM_FLOOR).sum() > 0


# ---- 4. options ------------------------------------------------------------------------------------------------------

def test_sphere_options(rt, O):
    """FAST gives the bits of PARITY; rr / counters / variant change nothing; the sky changes the miss albedo only; t_min is honoured."""
    name = "random_50x37"
    ref = R.reference(rt, O, name)
    fb, o, (sp, mt, cam, nx, ny) = _init_spheres(rt, name)
    mask = _all_mask(rt, False)
    for opts in (dict(fp=rt.RT_FP_FAST), dict(fp=rt.RT_FP_PARITY, rr=1), dict(rr=0, counters=1), dict(counters=0, variant=1), dict(variant=0, rng=rt.RT_RNG_COUNTER)):
        rt.setRenderOptions(o, **opts)
        _same(rt.renderGuides(mask), ref, f"{name} {opts}")
    rt.setRenderOptions(o, rng=rt.RT_RNG_REFERENCE_STREAM, sky=rt.RT_SKY_CONST_GREY)
    grey = rt.renderGuides(mask)
    miss = ref["prim"] == R.PRIM_NONE
    assert np.array_equal(_bits(grey["albedo"][miss]), _bits(np.full((int(miss.sum()), 3), 0.5, np.float32)))
    assert np.array_equal(_bits(grey["albedo"][~miss]), _bits(ref["albedo"][~miss]))
    for k in ("normal", "depth", "prim"):
        assert np.array_equal(_bits(grey[k]), _bits(ref[k])), k
    # t_min above the nearest hits: those rays take the far root or the next sphere, as the reference with the same t_min does
    t_min = float(np.median(ref["depth"][~miss]))
    rt.setRenderOptions(o, sky=rt.RT_SKY_GRADIENT, t_min=t_min)
    got = rt.renderGuides(mask)
    rt.cleanupRenderer()
    ref_t = R.sphere_guides(rt, O, sp, mt, cam, nx, ny, t_min=t_min)
    assert (ref_t["prim"] != ref["prim"]).mean() > 0.05
    _same(got, ref_t, f"{name} t_min={t_min}")


def test_mesh_options(rt, O):
    """FAST = PARITY; nee / rr / counters / variant change nothing; the gradient sky changes the miss albedo only; t_min is honoured."""
    name = "tris300"
    ref = R.reference(rt, O, name)
    fb, o, f = _init_mesh(rt, O, name)
    mask = _all_mask(rt, True)
    for opts in (dict(fp=rt.RT_FP_FAST), dict(fp=rt.RT_FP_PARITY, nee=0, rr=0), dict(nee=1, counters=1), dict(counters=0, variant=1), dict(variant=0)):
        rt.setRenderOptions(o, **opts)
        _same(rt.renderGuides(mask), ref, f"{name} {opts}")
    rt.setRenderOptions(o, sky=rt.RT_SKY_GRADIENT)
    got = rt.renderGuides(mask)
    ref_s = R.mesh_guides(rt, O, f["hm"], f["mats"], f["tex"], f["cam"], f["nx"], f["ny"], sky=rt.RT_SKY_GRADIENT)
    _same(got, ref_s, f"{name} gradient sky")
    miss = ref["prim"] == R.PRIM_NONE
    assert np.array_equal(_bits(ref_s["albedo"][~miss]), _bits(ref["albedo"][~miss])) and not np.array_equal(ref_s["albedo"][miss], ref["albedo"][miss])
    t_min = float(np.median(ref["depth"][~miss]))
    rt.setRenderOptions(o, sky=rt.RT_SKY_CONST_GREY, t_min=t_min)
    got = rt.renderGuides(mask)
    rt.cleanupRenderer()
    ref_t = R.mesh_guides(rt, O, f["hm"], f["mats"], f["tex"], f["cam"], f["nx"], f["ny"], t_min=t_min)
    assert (ref_t["prim"] != ref["prim"]).mean() > 0.02
    _same(got, ref_t, f"{name} t_min={t_min}")


# ---- 5. partitions ---------------------------------------------------------------------------------------------------

def _sentinel_planes(rt, nx, ny, mesh):
    out = {}
    for name, bit, dtype, comps in rt.GUIDE_PLANES:
        if name == "nodes" and not mesh:
            continue
        a = np.empty((ny, nx, 3) if comps == 3 else (ny, nx), dtype)
        a.view(np.uint32)[...] = SENTINEL
        out[name] = a
    return out


def _rows_of(ny, sr, rank, world):
    return np.array([j for j in range(ny) if (j // sr) % world == rank], int)


@pytest.mark.parametrize("name,stripe_rows", [("random_50x37", 8), ("random_50x37", 16), ("staircase_a", 8), ("staircase_a", 16)])
def test_two_ranks_fill_one_set_of_arrays(rt, O, name, stripe_rows):
    """part_world = 2: both ranks in turn into the same arrays equal the single-partition reference; after rank 0 alone the rows of rank 1 still hold
    the sentinel.  ny (37, 50) is no multiple of stripe_rows (8, 16)."""
    mesh = name in R.MESH_FRAMES
    ref = R.reference(rt, O, name)
    if mesh:
        fb, o, f = _init_mesh(rt, O, name)
        nx, ny = f["nx"], f["ny"]
    else:
        fb, o, (_, _, _, nx, ny) = _init_spheres(rt, name)
    assert ny % stripe_rows != 0
    out = _sentinel_planes(rt, nx, ny, mesh)
    mask = _all_mask(rt, mesh)
    rt.setRenderOptions(o, stripe_rows=stripe_rows, part_rank=0, part_world=2)
    rt.renderGuides(mask, out=out)
    own, other = _rows_of(ny, stripe_rows, 0, 2), _rows_of(ny, stripe_rows, 1, 2)
    for k in ref:
        assert np.all(_bits(out[k])[other] == SENTINEL), k
        assert np.array_equal(_bits(out[k])[own], _bits(ref[k])[own]), k
    rt.setRenderOptions(o, part_rank=1)
    rt.renderGuides(mask, out=out)
    rt.cleanupRenderer()
    _same(out, ref, f"{name} two ranks, stripes of {stripe_rows}")


def test_two_in_process_devices(rt, O):
    if rt.device_count() < 2:
        pytest.skip("needs two HIP devices")
    name = "random_50x37"
    fb, o, _ = _init_spheres(rt, name, devices=[0, 1])
    got = rt.renderGuides(_all_mask(rt, False))
    rt.cleanupRenderer()
    _same(got, R.reference(rt, O, name), "two devices")


# ---- 6. subset masks, setCamera --------------------------------------------------------------------------------------

def test_subset_mask_and_set_camera(rt, O):
    name = "staircase_b"
    ref = R.reference(rt, O, name)
    fb, o, f = _init_mesh(rt, O, name)
    got = rt.renderGuides(rt.RT_GUIDE_DEPTH | rt.RT_GUIDE_NODES)          # the other three pointers are NULL
    assert sorted(got) == ["depth", "nodes"]
    _same(got, {k: ref[k] for k in got}, "depth + nodes")
    got = rt.renderGuides(rt.RT_GUIDE_ALBEDO)
    _same(got, {"albedo": ref["albedo"]}, "albedo alone")
    out = _sentinel_planes(rt, f["nx"], f["ny"], True)                  # arrays passed but not named in the mask stay untouched
    rt.renderGuides(rt.RT_GUIDE_PRIM, out=out)
    assert np.array_equal(_bits(out["prim"]), _bits(ref["prim"]))
    assert all(np.all(_bits(out[k]) == SENTINEL) for k in ("albedo", "normal", "depth", "nodes"))
    cam2 = rt.make_camera((467, 588, 1288), (5, 210, 200), (0, 1, 0), 35.0, f["nx"] / f["ny"], 0.2, 40.0)      # the staircase from outside: bounds misses too
    rt.setCamera(cam2)
    got = rt.renderGuides(_all_mask(rt, True))
    rt.cleanupRenderer()
    ref2 = R.mesh_guides(rt, O, f["hm"], f["mats"], f["tex"], cam2, f["nx"], f["ny"])
    assert 0 < (ref2["prim"] == R.PRIM_NONE).sum() < ref2["prim"].size
    _same(got, ref2, "after setCamera")


def test_set_camera_spheres(rt, O):
    fb, o, (sp, mt, cam, nx, ny) = _init_spheres(rt, "random_50x37")
    cam2 = rt.make_camera((-6, 3, 9), (0, 0.5, 0), (0, 1, 0), 30.0, nx / ny, 0.1, 10.0)
    rt.setCamera(cam2)
    got = rt.renderGuides(_all_mask(rt, False))
    rt.cleanupRenderer()
    ref2 = R.sphere_guides(rt, O, sp, mt, cam2, nx, ny)
    assert 0 < (ref2["prim"] == R.PRIM_NONE).sum() < ref2["prim"].size
    _same(got, ref2, "spheres after setCamera")


# ---- 7. no side effects ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["spheres", "mesh"])
def test_no_side_effects(rt, O, kind):
    """runRenderer(16); framebuffer, stats and launch report are the same after renderGuides.  Progressive 8 + renderGuides + 8 equals runRenderer(16)."""
    if kind == "spheres":
        fb, o, _ = _init_spheres(rt, "random_96x64")
    else:
        fb, o, _ = _init_mesh(rt, O, "staircase_a")
    mask = _all_mask(rt, kind == "mesh")
    rt.runRenderer(16)
    frame, stats, launches = np.array(fb, copy=True), _stats_tuple(rt.getRenderStats()), rt.last_launches()
    assert launches
    rt.renderGuides(mask)
    assert np.array_equal(_bits(fb), _bits(frame))
    assert _stats_tuple(rt.getRenderStats()) == stats
    assert rt.last_launches() == launches
    rt.runRendererProgressive(8)
    rt.renderGuides(mask)
    assert rt.progressive_samples() == 8
    rt.runRendererProgressive(8)
    assert rt.progressive_samples() == 16
    total = np.array(fb, copy=True)
    rt.cleanupRenderer()
    assert np.array_equal(_bits(total), _bits(frame))


# ---- 8. misuse -------------------------------------------------------------------------------------------------------

_SPHERES = "sp, mt, cam = rt.scene_random_spheres(64, 48); rt.initRendererSpheres(sp, mt, cam, 64, 48, 10)\n"
_MISUSE = {
    "mask_zero": _SPHERES + "rt.renderGuides(0)\n",
    "unknown_bit": _SPHERES + "rt.renderGuides(rt.RT_GUIDE_DEPTH | 32)\n",
    "null_plane": _SPHERES + "rt.load_renderer().renderGuides(rt.RT_GUIDE_DEPTH | rt.RT_GUIDE_PRIM, None, None, None, "
                             "np.zeros((48, 64), np.int32).ctypes.data_as(C.POINTER(C.c_int32)), None)\n",
    "nodes_on_spheres": _SPHERES + "rt.renderGuides(rt.RT_GUIDE_NODES)\n",
    "floor_on_spheres": _SPHERES + "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); rt.renderGuides(rt.RT_GUIDE_DEPTH)\n",
    "after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.renderGuides(rt.RT_GUIDE_DEPTH)\n",
}


@pytest.mark.parametrize("case", sorted(_MISUSE))
def test_misuse_exits_99(case):
    """The library's misuse convention, each case in a child process of its own: 'rt error' on stderr and exit status 99 (a clean exit of a host-side check)."""
    exits_99(_MISUSE[case])
