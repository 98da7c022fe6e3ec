"""denoiseFrame (include/rt_api.h) on the GPU against the test reference (tests/denoise_reference.py): every frame, all pixels, bit for bit (np.array_equal on
the raw 32-bit words: no tolerance, nothing left out).  The reference filters the very framebuffer the GPU rendered (copied before the call) with the guide
reference's planes, so nothing here leans on render parity.  Then synthetic input in place over the parameter space, one large frame, partitions, setCamera,
no side effects, progressive use and the misuse exits."""
import numpy as np
import pytest

import denoise_reference as D
import guides_reference as R
from preview_support import bits as _bits, exits_99, init_frame as _init, same as _same, stats_tuple as _stats_tuple

pytestmark = pytest.mark.gpu
FRAMES = ("random_96x64", "random_50x37", "three_spheres", "cloud_hybrid", "tie", "staircase_a", "staircase_b", "tris300", "tris300_floor")


def _reference(rt, O, name, frame, **kw):
    g, origin, dn, mesh = D.frame_inputs(rt, O, name)
    kw = dict(dict(D.DEFAULTS, flags=D.default_flags(mesh)), **kw)
    return D.denoise(frame, g, origin, dn, **kw)


# ---- 1. rendered frames ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FRAMES)
def test_rendered_frames_match_the_reference(rt, O, name):
    """runRenderer(4), a copy of the framebuffer, denoiseFrame(NULL, out, defaults): out equals the reference applied to that copy."""
    fb, o, mesh = _init(rt, O, name)
    assert rt.default_denoise_flags() == D.default_flags(mesh)
    rt.runRenderer(4)
    frame = np.array(fb, copy=True)
    got = rt.denoiseFrame()
    ms = rt.last_denoise_ms()
    assert np.array_equal(_bits(fb), _bits(frame))              # the framebuffer was the input, not the output
    rt.cleanupRenderer()
    assert ms > 0.0
    ref = _reference(rt, O, name, frame)
    valid = R.reference(rt, O, name)["prim"] != R.PRIM_NONE
    print(f"{name}: kernels {ms:.3f} ms, {float((D.ulp_distance(ref, frame).max(axis=-1) > 1)[valid].mean()):.3f} of the valid pixels change")
    _same(got, ref, name)


# ---- 2. synthetic input, in place, over the parameter space ----------------------------------------------------------

_CASES = [dict(iterations=1), dict(iterations=8), dict(flags=0), dict(flags=1), dict(flags=2), dict(flags=3), dict(normal_squarings=0), dict(normal_squarings=7),
          dict(sigma_c=0.0), dict(sigma_c=-1.0), dict(sigma_z=100.0), dict(sigma_z=1e-5), dict(iterations=8, flags=0, normal_squarings=0, sigma_c=0.0, sigma_z=100.0)]


@pytest.mark.parametrize("name", ["random_96x64", "staircase_a"])
def test_synthetic_input_in_place(rt, O, name):
    """A seeded random image, uniform in [0, 4), passed explicitly with out == in.  sigma_z = 100: wz is about 1 on most taps; 1e-5: most taps get 0."""
    fb, o, mesh = _init(rt, O, name)
    g, origin, dn, _ = D.frame_inputs(rt, O, name)
    ny, nx = g["prim"].shape
    valid = g["prim"] != R.PRIM_NONE
    try:
        for k, case in enumerate(_CASES):
            src = np.random.default_rng(100 + k).uniform(0, 4, (ny, nx, 3)).astype(np.float32)
            kw = dict(dict(D.DEFAULTS, flags=D.default_flags(mesh)), **case)
            cnt = {}
            ref = D.denoise(src, g, origin, dn, counts=cnt, **kw)
            buf = src.copy()
            got = rt.denoiseFrame(buf, out=buf, **kw)
            assert got is buf
            print(name, case, "accepted taps with wz < 1: %.3f, with wc < 1: %.3f; valid pixels that change: %.3f" % (
                cnt["wz_lt1"] / max(1, cnt["accepted"]), cnt["wc_lt1"] / max(1, cnt["accepted"]),
                float((D.ulp_distance(ref, src).max(axis=-1) > 1)[valid].mean())))
            _same(buf, ref, f"{name} {case}")
            assert np.array_equal(_bits(ref[~valid]), _bits(src[~valid]))
    finally:
        rt.cleanupRenderer()


# ---- 3. one large frame ----------------------------------------------------------------------------------------------

def test_large_frame(rt, O):
    """1200 x 800 random spheres, 4 spp, 5 iterations.  The per-pixel guide reference is too slow here: the guide planes are renderGuides' (pinned bit-exact by
    tests/test_gpu_guides.py) and P comes from the numpy restatement of the centre ray (pinned against orc_get_ray by tests/test_denoise_api.py)."""
    nx, ny = 1200, 800
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    rt.runRenderer(4)
    frame = np.array(fb, copy=True)
    g = rt.renderGuides()
    got = rt.denoiseFrame()
    ms = rt.last_denoise_ms()
    rt.cleanupRenderer()
    origin, dn = D.centre_dirs_numpy(cam, nx, ny)
    ref = D.denoise(frame, g, origin, dn, flags=D.default_flags(False), **D.DEFAULTS)
    print(f"1200x800: kernels {ms:.3f} ms")
    _same(got, ref, "1200x800")


# ---- 4. partitions ---------------------------------------------------------------------------------------------------

def test_partitioned_renderer_still_denoises_the_whole_image(rt, O):
    """part_world = 2, part_rank = 1 with stripes of 8 rows (the smallest the renderer accepts): the render fills half the rows; denoiseFrame with an explicit
    full input returns the whole-image result of the unpartitioned call.  Then a partition in which this process owns no row at all."""
    name = "random_96x64"
    fb, o, mesh = _init(rt, O, name)
    rt.runRenderer(4)
    frame = np.array(fb, copy=True)
    whole = rt.denoiseFrame(frame)
    rt.setRenderOptions(o, stripe_rows=8, part_rank=1, part_world=2)
    fb[...] = -1.0
    rt.runRenderer(4)
    own = np.array([(j // 8) % 2 == 1 for j in range(frame.shape[0])])
    assert own.sum() * 2 == own.size
    assert np.array_equal(_bits(fb[own]), _bits(frame[own])) and np.all(fb[~own] == -1.0)
    part = rt.denoiseFrame(frame)
    rt.setRenderOptions(o, stripe_rows=64, part_rank=1, part_world=2)          # 64 rows = one stripe: rank 1 owns nothing
    none = rt.denoiseFrame(frame)
    rt.cleanupRenderer()
    ref = _reference(rt, O, name, frame)
    _same(whole, ref, "unpartitioned")
    _same(part, ref, "rank 1 of 2")
    _same(none, ref, "a rank without rows")


def test_two_in_process_devices(rt, O):
    if rt.device_count() < 2:
        pytest.skip("needs two HIP devices")
    name = "random_50x37"
    fb, o, mesh = _init(rt, O, name, devices=[0, 1])
    rt.runRenderer(4)
    frame = np.array(fb, copy=True)
    got = rt.denoiseFrame()
    rt.cleanupRenderer()
    _same(got, _reference(rt, O, name, frame), "two devices")


# ---- 5. camera, options ----------------------------------------------------------------------------------------------

def test_follows_set_camera(rt, O):
    name = "random_50x37"
    sp, mt, cam, nx, ny = R.sphere_frame(rt, name)
    fb, o, mesh = _init(rt, O, name)
    rt.runRenderer(4)
    first = rt.denoiseFrame()
    cam2 = rt.make_camera((-6, 3, 9), (0, 0.5, 0), (0, 1, 0), 30.0, nx / ny, 0.1, 10.0)
    rt.setCamera(cam2)
    rt.runRenderer(4)
    frame = np.array(fb, copy=True)
    got = rt.denoiseFrame()
    rt.cleanupRenderer()
    g2 = R.sphere_guides(rt, O, sp, mt, cam2, nx, ny)
    origin, dn = D.centre_dirs(rt, O, cam2, nx, ny)
    ref = D.denoise(frame, g2, origin, dn, flags=D.default_flags(False), **D.DEFAULTS)
    assert not np.array_equal(_bits(first), _bits(got))
    _same(got, ref, "after setCamera")


def test_follows_t_min_and_reinit_with_another_size(rt, O):
    """t_min above the nearest hits changes the guides and so the result; a second init with another image size allocates the buffers again."""
    name = "random_50x37"
    sp, mt, cam, nx, ny = R.sphere_frame(rt, name)
    fb, o, mesh = _init(rt, O, name)
    g0 = R.reference(rt, O, name)
    t_min = float(np.median(g0["depth"][g0["prim"] != R.PRIM_NONE]))
    rt.setRenderOptions(o, t_min=t_min)
    src = np.random.default_rng(3).uniform(0, 4, (ny, nx, 3)).astype(np.float32)
    got = rt.denoiseFrame(src)
    gt = R.sphere_guides(rt, O, sp, mt, cam, nx, ny, t_min=t_min)
    origin, dn = D.centre_dirs(rt, O, cam, nx, ny)
    _same(got, D.denoise(src, gt, origin, dn, flags=D.default_flags(False), **D.DEFAULTS), f"t_min={t_min}")
    fb, o, mesh = _init(rt, O, "staircase_a")                   # 40 x 50 after 50 x 37, a mesh after spheres
    rt.runRenderer(4)
    frame = np.array(fb, copy=True)
    got = rt.denoiseFrame()
    rt.cleanupRenderer()
    _same(got, _reference(rt, O, "staircase_a", frame), "after a second init")


# ---- 6. no side effects, progressive use -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["random_96x64", "staircase_a"])
def test_no_side_effects(rt, O, name):
    """Framebuffer, stats, launch report, guide timing and the progressive frame are the same with and without a denoiseFrame in between."""
    fb, o, mesh = _init(rt, O, name)
    rt.runRenderer(4)
    four = np.array(fb, copy=True)
    rt.renderGuides()
    rt.runRenderer(8)
    frame, stats, launches, guides_ms = np.array(fb, copy=True), _stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.last_guides_ms()
    assert launches and guides_ms > 0.0
    rt.denoiseFrame()
    rt.denoiseFrame(four, iterations=2)
    assert np.array_equal(_bits(fb), _bits(frame))
    assert _stats_tuple(rt.getRenderStats()) == stats
    assert rt.last_launches() == launches
    assert rt.last_guides_ms() == guides_ms
    rt.runRendererProgressive(2)
    assert rt.progressive_samples() == 2
    rt.denoiseFrame()
    assert rt.progressive_samples() == 2
    rt.runRendererProgressive(2)
    assert rt.progressive_samples() == 4
    total = np.array(fb, copy=True)
    rt.cleanupRenderer()
    assert np.array_equal(_bits(total), _bits(four))


def test_progressive_use(rt, O):
    """Three passes of one sample, each followed by denoiseFrame: every denoised frame is the reference of that pass's framebuffer, and the progressive frame
    still ends as runRenderer(3)."""
    name = "random_96x64"
    fb, o, mesh = _init(rt, O, name)
    rt.runRenderer(3)
    three = np.array(fb, copy=True)
    pairs = []
    for _ in range(3):
        rt.runRendererProgressive(1)
        frame = np.array(fb, copy=True)
        pairs.append((frame, rt.denoiseFrame()))
    final = np.array(fb, copy=True)
    rt.cleanupRenderer()
    assert np.array_equal(_bits(final), _bits(three))
    for k, (frame, got) in enumerate(pairs):
        _same(got, _reference(rt, O, name, frame), f"pass {k + 1}")


# ---- 7. misuse -------------------------------------------------------------------------------------------------------

_SPHERES = ("sp, mt, cam = rt.scene_random_spheres(64, 48); rt.initRendererSpheres(sp, mt, cam, 64, 48, 10)\n"
            "a = np.zeros((48, 64, 3), np.float32); call = rt.load_renderer().denoiseFrame; p = a.ctypes.data\n")
_MISUSE = {
    "out_null": _SPHERES + "call(p, None, 5, 3, 5, 0.01, 1.0)\n",
    "iterations_0": _SPHERES + "call(p, p, 0, 3, 5, 0.01, 1.0)\n",
    "iterations_9": _SPHERES + "call(p, p, 9, 3, 5, 0.01, 1.0)\n",
    "squarings_minus_1": _SPHERES + "call(p, p, 5, 3, -1, 0.01, 1.0)\n",
    "squarings_8": _SPHERES + "call(p, p, 5, 3, 8, 0.01, 1.0)\n",
    "unknown_flag": _SPHERES + "call(p, p, 5, 4, 5, 0.01, 1.0)\n",
    "sigma_z_zero": _SPHERES + "call(p, p, 5, 3, 5, 0.0, 1.0)\n",
    "sigma_z_negative": _SPHERES + "call(p, p, 5, 3, 5, -0.01, 1.0)\n",
    "sigma_z_nan": _SPHERES + "call(p, p, 5, 3, 5, float('nan'), 1.0)\n",
    "sigma_z_inf": _SPHERES + "call(p, p, 5, 3, 5, float('inf'), 1.0)\n",
    "sigma_c_nan": _SPHERES + "call(p, p, 5, 3, 5, 0.01, float('nan'))\n",
    "sigma_c_inf": _SPHERES + "call(p, p, 5, 3, 5, 0.01, float('inf'))\n",
    "floor_on_spheres": _SPHERES + "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); call(p, p, 5, 3, 5, 0.01, 1.0)\n",
    "after_cleanup": _SPHERES + "rt.cleanupRenderer(); call(p, p, 5, 3, 5, 0.01, 1.0)\n",
}


@pytest.mark.parametrize("case", sorted(_MISUSE))
def test_misuse_exits_99(case):
    """The library's misuse convention, each case in a child process of its own: 'rt error' on stderr and exit status 99 (a clean exit of a host-side check)."""
    exits_99(_MISUSE[case])


def test_valid_edge_parameters_are_accepted(rt, O):
    """The other side of the misuse list: iterations 1 and 8, squarings 0 and 7, sigma_c <= 0 run."""
    fb, o, mesh = _init(rt, O, "tie")
    rt.runRenderer(1)
    for kw in (dict(iterations=1, normal_squarings=0, sigma_c=-3.0), dict(iterations=8, normal_squarings=7, sigma_c=0.0)):
        assert np.isfinite(rt.denoiseFrame(**kw)).all()
    assert rt.last_denoise_ms() > 0.0
    rt.cleanupRenderer()
