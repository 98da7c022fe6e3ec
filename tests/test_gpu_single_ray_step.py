"""The single-ray step of the folded sphere kinds (k_render_spheres_queue with FORM = 1): a wave with one live ray scans the scene with
scan_single - every lane pre-tests its own slot of every round of 64 - and shades the one hit; in the folded kinds the refill loop in front of it is
skipped while the wave holds the lanes it was capped at.  The cases are those of the section's five instruction cuts - the rounds of the pre-test loop,
the three materials under one live lane, the hit normal's division on both sides of the shared-reciprocal form's window - so that the two cuts that were
measured inside the noise and left out can come back against a test that is already there.  None of it may move a bit: every frame here is the CPU
oracle's, word for word, free of NaN (the framebuffer is NaN-poisoned before a frame), rendered twice in a row - measured, then ordered by the first
frame's cost map - and both frames must report the folded form.  The idioms are those of test_gpu_sphere_form.py: the random-spheres scene seen in a
close-up of a sphere's contact with the ground, where pixels of 24 rays per sample and more go one to a wave (chain list 0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VIEW = dict(lookfrom=(2.5, 0.4, 1.5), lookat=(0.5, 0.1, 0.5), vfov=20.0, focus=3.0)
LIST0 = 24                          # rays per sample from which a pixel goes to chain list 0 (RtSwitches::top_thr / 16)
GENERAL, DEFAULT = 0, 1
KINDS_FULL = (1, 3, 7, 11, 15, 19, 27, 35, 43)      # the kinds that are built folded
DEPTH = 50
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, ref, what=""):
    assert not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    assert np.array_equal(_bits(got), _bits(ref)), (what, int(np.count_nonzero(_bits(got) != _bits(ref))))


def _camera(rt, nx, ny):
    return rt.make_camera(VIEW["lookfrom"], VIEW["lookat"], (0, 1, 0), VIEW["vfov"], nx / ny, 0.0, VIEW["focus"])


def _scene(rt):
    """The random-spheres scene (its spheres and materials do not depend on the image size), shared read-only."""
    if "scene" not in _CACHE:
        sp, mt, _ = rt.scene_random_spheres(32, 24)
        sp.setflags(write=False)
        mt.setflags(write=False)
        _CACHE["scene"] = (sp, mt)
    return _CACHE["scene"]


def _oracle(O, sp, mt, cam, nx, ny, ns):
    return O.render(O.sphere_scene(sp, mt), cam, O.default_options(True), nx, ny, ns, DEPTH)[0]


def _rays(O, sp, mt, cam, nx, ny, ns):
    """The oracle's rays of every pixel over its first ns samples (one pixel per call)."""
    sc, opt = O.sphere_scene(sp, mt), O.default_options(True)
    return np.array([O.render(sc, cam, opt, nx, ny, ns, DEPTH, region=(x, y, x + 1, y + 1), counters=True)[1].rays for y in range(ny) for x in range(nx)], dtype=np.int64)


def _a_wave_ends_on_one_lane(O, sp, mt, cam, nx, ny, ns):
    """Said by the oracle alone, for a frame of at most 1024 pixels (one workgroup: every pixel is fetched in the first iteration of the cost-ordered
    dispatch, which resumes the pixels after the 2 samples of the first one, and a live lane traces one ray per iteration - extra rays only in steps that
    select at most four lanes).  Either a pixel is on chain list 0 in both estimates (it is dealt alone to a wave), or the rays that are left after the
    first dispatch have ONE largest value: the wave that holds that pixel traces its last rays with no other lane live."""
    r2, rn = _rays(O, sp, mt, cam, nx, ny, 2), _rays(O, sp, mt, cam, nx, ny, ns)
    left = rn - r2
    return (r2.max() >= LIST0 * 2 and rn.max() >= LIST0 * ns) or int((left == left.max()).sum()) == 1


def _two_frames(rt, sp, mt, cam, nx, ny, ns, lean=None):
    """Two frames in a row with default options: measured (TwoDispatch), then ordered by the first frame's cost map (OrderedSingle).  Both must have run the
    folded form of a kind that is built folded, without diagnostics; `lean`: the kind expected."""
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, DEPTH)
    frames = []
    for want in ([1, 2], [2]):
        rt.runRenderer(ns)
        got, recs, form = np.array(fb, copy=True), rt.last_launches(), rt.last_sphere_form()
        last = recs[-1]
        assert [r["phase"] for r in recs] == want and form == DEFAULT and (last["cls"], last["dbg"]) == (2, 0) and last["lean"] in KINDS_FULL, (want, form, last)
        if lean is not None:
            assert last["lean"] == lean, last
        frames.append(got)
    rt.cleanupRenderer()
    return frames


def _check(rt, O, sp, mt, nx, ny, ns, lean=None, what=""):
    cam = _camera(rt, nx, ny)
    ref = _oracle(O, sp, mt, cam, nx, ny, ns)
    assert not np.isnan(ref).any(), what
    measured, ordered = _two_frames(rt, sp, mt, cam, nx, ny, ns, lean)
    _same(measured, ref, what + " measured")
    _same(ordered, ref, what + " ordered by the map")
    return measured


@pytest.mark.parametrize("nx,ny,ns", [(96, 64, 16), (13, 7, 8), (8, 8, 8)])
def test_close_up(rt, O, nx, ny, ns):
    """The close-up of test_gpu_sphere_form.py (which holds, with the oracle, that 96x64 puts pixels on chain list 0: one-pixel waves trace whole pixels
    in the single-ray step), and one workgroup with partial tiles."""
    sp, mt = _scene(rt)
    got = _check(rt, O, sp, mt, nx, ny, ns, lean=3, what=f"{nx}x{ny}")
    if (nx, ny) == (96, 64):
        got.setflags(write=False)
        _CACHE["close-up"] = got


def _first_n(rt, n):
    """The first n spheres of the scene, the ground sphere (index 0) included; beyond the scene's 488, copies of its first small spheres set above them."""
    sp, mt = _scene(rt)
    if n <= len(sp):
        return sp[:n].copy(), mt[:n].copy()
    extra = n - len(sp)
    s2, m2 = np.concatenate([sp, sp[1:1 + extra]]), np.concatenate([mt, mt[1:1 + extra]])
    s2["center"][len(sp):, 1] += 0.45
    return s2, m2


@pytest.mark.parametrize("n", [1, 64, 65, 192, 256, 257, 488, 520])
def test_round_counts_of_the_pre_test_loop(rt, O, n):
    """n spheres are 1 to 9 rounds of 64 slots: the trip of four rounds alone, the remainder loop alone, and both.  32x24 at 8 samples, one workgroup.
    Where the oracle shows that a wave of that frame ends on one live lane, the frame itself drives the single-ray step.  Where it cannot - with the ground
    alone every pixel traces 2 rays a sample and the twelve full waves end together; small scenes can tie for the longest pixel - the same scene is rendered
    as a frame of ONE pixel as well: its wave has one live lane for every ray of the frame."""
    nx, ny, ns = 32, 24, 8
    sp, mt = _first_n(rt, n)
    assert len(sp) == n
    alone = _a_wave_ends_on_one_lane(O, sp, mt, _camera(rt, nx, ny), nx, ny, ns)
    _check(rt, O, sp, mt, nx, ny, ns, what=f"{n} spheres")
    if not alone:
        _check(rt, O, sp, mt, 1, 1, ns, what=f"{n} spheres, one pixel")


@pytest.mark.parametrize("name,param", [("diffuse", 0.0), ("metal", 0.1), ("metal", 0.0), ("glass", 1.5)], ids=["diffuse", "metal_fuzz", "metal_mirror", "glass"])
def test_each_material_under_the_single_live_lane(rt, O, name, param):
    """16x16 of the close-up with every sphere but the ground made diffuse / metal with and without fuzz / glass (the variants of tools/sweep_scenes.py): the
    contact-line pixels that a wave traces alone bounce off that material.  The oracle says that such a wave exists."""
    nx, ny, ns = 16, 16, 8
    sp, mt = _scene(rt)
    m2 = mt.copy()
    m2["type"][1:] = {"diffuse": rt.RT_DIFFUSE, "metal": rt.RT_METAL, "glass": rt.RT_GLASS}[name]
    m2["param"][1:] = param
    assert _a_wave_ends_on_one_lane(O, sp, m2, _camera(rt, nx, ny), nx, ny, ns)
    _check(rt, O, sp, m2, nx, ny, ns, what=name)


def test_hit_normal_on_both_sides_of_the_guard(rt, O):
    """The hit normal (hp - c) / radius: the shared-reciprocal form of rt_exactdiv.h (measured in DESIGN.md 3.26, not in the tree) would take the operands
    inside rt_exdiv3_window - radius and the offset's components in [2^-40, 2^40] - and leave the plain division to those outside; the tree divides
    plainly on both sides.  The condition is on the operands, so the oracle alone says which side is populated: a sphere of radius 2^45 (every hit on
    it has a divisor above the window: the plain side) beside the scene's ordinary spheres (radii 0.2 to 1000: the shared side), and one of radius 2^-45.
    The frame with the giant sphere differs from the frame without it and from the frame of the giant alone, so both kinds of hit are in it.  (Nothing
    hits the tiny sphere - a ray would have to pass within 3e-14 of its centre; the oracle agrees: the frame is the same without it.  Below the window
    the device is held by rtProbeExactDiv, test_gpu_exactdiv.py.)"""
    nx, ny, ns = 32, 24, 8
    sp, mt = _scene(rt)
    n = len(sp)
    s2, m2 = np.concatenate([sp, sp[:2]]), np.concatenate([mt, mt[:2]])
    s2["center"][n], s2["radius"][n] = (0.9, 0.45, 0.8), 2.0 ** -45
    s2["center"][n + 1], s2["radius"][n + 1] = (-2.0 ** 45, 0.0, 0.0), 2.0 ** 45
    m2["type"][n:] = rt.RT_DIFFUSE
    m2["color"][n:] = (0.9, 0.2, 0.2)
    m2["param"][n:] = 0.0
    cam = _camera(rt, nx, ny)
    full = _oracle(O, s2, m2, cam, nx, ny, ns)
    assert not np.array_equal(_bits(full), _bits(_oracle(O, s2[:n + 1], m2[:n + 1], cam, nx, ny, ns)))      # the giant sphere is hit
    assert not np.array_equal(_bits(full), _bits(_oracle(O, s2[n:], m2[n:], cam, nx, ny, ns)))              # ordinary spheres are hit
    assert np.array_equal(_bits(full), _bits(_oracle(O, np.delete(s2, n), np.delete(m2, n), cam, nx, ny, ns)))   # the tiny one is not
    _check(rt, O, s2, m2, nx, ny, ns, what="radii 2^-45 and 2^45")


@pytest.mark.parametrize("env", [{"RT_SINGLE_RAY": "0"}, {"RT_POOL": "8"}], ids=["single_ray_0", "pool_8"])
def test_the_general_form_renders_the_same_frame(rt, O, env, monkeypatch):
    """RT_SINGLE_RAY=0 (no single-ray step at all) and RT_POOL=8 (a scheduling constant the folded kernel is not compiled with) leave the folded form: the
    general kernel, which has no early-out in front of its refill loop, renders the default form's close-up frame."""
    if "close-up" not in _CACHE:
        sp, mt = _scene(rt)
        _CACHE["close-up"] = _two_frames(rt, sp, mt, _camera(rt, 96, 64), 96, 64, 16, lean=3)[0]
    want = _CACHE["close-up"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sp, mt = _scene(rt)
    fb = rt.initRendererSpheres(sp, mt, _camera(rt, 96, 64), 96, 64, DEPTH)
    for frame in ("measured", "ordered by the map"):
        rt.runRenderer(16)
        got, recs, form = np.array(fb, copy=True), rt.last_launches(), rt.last_sphere_form()
        assert recs[-1]["phase"] == 2 and recs[-1]["cls"] == 2 and form == GENERAL, (frame, form, recs[-1])
        _same(got, want, frame)
    rt.cleanupRenderer()
