"""Helpers of tests/test_gpu_ray_step_loads.py (no test in here): the close-up frames of tests/test_gpu_single_ray_step.py - the random-spheres scene
seen where a sphere rests on the ground, rendered twice in a row (measured, then ordered by the first frame's cost map), both frames in the folded form
and both the CPU oracle's, word for word - and the padding rule of csrc/rt_scene_layout.h restated, so that a test can say on the CPU how many rounds of
64 slots the single-ray scan makes over a scene."""
import numpy as np

VIEW = dict(lookfrom=(2.5, 0.4, 1.5), lookat=(0.5, 0.1, 0.5), vfov=20.0, focus=3.0)
LIST0 = 24                          # rays per sample from which a pixel goes to chain list 0 (RtSwitches::top_thr / 16)
GENERAL, DEFAULT = 0, 1
KINDS_FULL = (1, 3, 7, 11, 15, 19, 27, 35, 43)      # the kinds that are built folded
DEPTH = 50
GROUP = 16                          # kSphereGroup
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, ref, what=""):
    assert not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    assert np.array_equal(bits(got), bits(ref)), (what, int(np.count_nonzero(bits(got) != bits(ref))))


def camera(rt, nx, ny):
    return rt.make_camera(VIEW["lookfrom"], VIEW["lookat"], (0, 1, 0), VIEW["vfov"], nx / ny, 0.0, VIEW["focus"])


def scene(rt):
    """The random-spheres scene (its spheres and materials do not depend on the image size), shared read-only."""
    if "scene" not in _CACHE:
        sp, mt, _ = rt.scene_random_spheres(32, 24)
        sp.setflags(write=False)
        mt.setflags(write=False)
        _CACHE["scene"] = (sp, mt)
    return _CACHE["scene"]


def first_n(rt, n):
    """The first n spheres of the scene, the ground sphere (index 0) included; beyond the scene's 488, copies of its first small spheres set above them."""
    sp, mt = scene(rt)
    if n <= len(sp):
        return sp[:n].copy(), mt[:n].copy()
    extra = n - len(sp)
    s2, m2 = np.concatenate([sp, sp[1:1 + extra]]), np.concatenate([mt, mt[1:1 + extra]])
    s2["center"][len(sp):, 1] += 0.45
    return s2, m2


def n_padded(spheres):
    """The slots of a scene's device image (build_sphere_scene, csrc/rt_scene_layout.h): the big spheres - radius above four times the median radius
    (the element n / 2 of the sorted radii), or not finite - padded to whole groups of 16, then the small ones padded to whole groups, the total padded
    to a multiple of 64."""
    r = np.abs(np.asarray(spheres["radius"], np.float32))
    n = len(r)
    big_above = np.float32(4.0) * np.sort(r)[n // 2]
    n_big = int(((r > big_above) | ~np.isfinite(r)).sum())
    up = lambda k, m: -(-k // m) * m
    return up(up(n_big, GROUP) + up(n - n_big, GROUP), 64)


def rounds(spheres):
    """Rounds of 64 slots of the single-ray scan (scan_single: n_padded >> 6)."""
    return n_padded(spheres) >> 6


def oracle(O, sp, mt, cam, nx, ny, ns):
    return O.render(O.sphere_scene(sp, mt), cam, O.default_options(True), nx, ny, ns, DEPTH)[0]


def rays(O, sp, mt, cam, nx, ny, ns):
    """The oracle's rays of every pixel over its first ns samples (one pixel per call)."""
    sc, opt = O.sphere_scene(sp, mt), O.default_options(True)
    return np.array([O.render(sc, cam, opt, nx, ny, ns, DEPTH, region=(x, y, x + 1, y + 1), counters=True)[1].rays for y in range(ny) for x in range(nx)], dtype=np.int64)


def a_wave_ends_on_one_lane(O, sp, mt, cam, nx, ny, ns):
    """Said by the oracle alone, for a frame of at most 1024 pixels (one workgroup: every pixel is fetched in the first iteration of the cost-ordered
    dispatch, which resumes the pixels after the 2 samples of the first one, and a live lane traces one ray per iteration - extra rays only in steps that
    select at most four lanes).  Either a pixel is on chain list 0 in both estimates (it is dealt alone to a wave), or the rays that are left after the
    first dispatch have ONE largest value: the wave that holds that pixel traces its last rays with no other lane live."""
    r2, rn = rays(O, sp, mt, cam, nx, ny, 2), rays(O, sp, mt, cam, nx, ny, ns)
    left = rn - r2
    return (r2.max() >= LIST0 * 2 and rn.max() >= LIST0 * ns) or int((left == left.max()).sum()) == 1


def two_frames(rt, sp, mt, cam, nx, ny, ns, lean=None):
    """Two frames in a row with default options: measured (TwoDispatch), then ordered by the first frame's cost map (OrderedSingle).  Both must have run the
    folded form of a kind that is built folded, without diagnostics; `lean`: the kind expected."""
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, DEPTH)
    frames = []
    try:
        for want in ([1, 2], [2]):
            rt.runRenderer(ns)
            got, recs, form = np.array(fb, copy=True), rt.last_launches(), rt.last_sphere_form()
            last = recs[-1]
            assert [r["phase"] for r in recs] == want and form == DEFAULT and (last["cls"], last["dbg"]) == (2, 0) and last["lean"] in KINDS_FULL, (want, form, last)
            if lean is not None:
                assert last["lean"] == lean, last
            frames.append(got)
    finally:
        rt.cleanupRenderer()
    return frames


def check(rt, O, sp, mt, nx, ny, ns, lean=None, what=""):
    cam = camera(rt, nx, ny)
    ref = oracle(O, sp, mt, cam, nx, ny, ns)
    assert not np.isnan(ref).any(), what
    measured, ordered = two_frames(rt, sp, mt, cam, nx, ny, ns, lean)
    same(measured, ref, what + " measured")
    same(ordered, ref, what + " ordered by the map")
    return measured
