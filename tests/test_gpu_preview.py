"""previewFrame (include/rt_api.h) on the GPU against the test reference (tests/preview_reference.py): every call, all pixels, out, the history length and the
variance, bit for bit (np.array_equal on the raw 32-bit words: no tolerance, nothing left out).  The reference is fed the very framebuffers the GPU rendered
(copied before the call) and the guide reference's planes, and keeps its own history, so nothing here leans on render parity.  Then synthetic input in place
over the parameter space, the stride-16 taps, a frame that is no multiple of the tile, sizes around and below a tile, special pixel values, the reset rules,
no side effects, the interplay with accumulateFrame and denoiseFrame, partitions and the misuse exits.

A history reaches RT_PREVIEW_MIN_HISTORY = 4 with the fourth call, so the sequences that have to reach the temporal branch of the variance run four calls
(the reference's counts say which do)."""
import numpy as np
import pytest

import accumulate_reference as A
import denoise_reference as D
import guides_reference as R
import preview_reference as V
import preview_support as S
from preview_support import bits as _bits, exits_99, init_frame as _init, same as _same, stats_tuple as _stats_tuple

pytestmark = pytest.mark.gpu
PLANES = ("out", "history", "variance")


def _step(rt, pre, frames, k, src=None, fb=None, default_flags=3, counts=None, **kw):
    """One call on both sides under frames[k] = (camera, guide planes, origin, centre directions): src None: runRenderer(1) and a copy of the framebuffer as the
    input, passed as NULL; else src is passed explicitly with out == in.  The library is given `kw` as it is, the reference the scene kind's default flags
    where kw has none.  Returns (input, (got out, N, variance), (reference out, N, variance))."""
    cam, g, origin, dn = frames[k]
    rt.setCamera(cam)
    if src is None:
        rt.runRenderer(1)
        frame = np.array(fb, copy=True)
        got = rt.previewFrame(history=True, variance=True, **kw)
        assert np.array_equal(_bits(fb), _bits(frame))          # the framebuffer was the input, not the output
    else:
        frame = src.copy()
        buf = src.copy()
        got = rt.previewFrame(buf, out=buf, history=True, variance=True, **kw)
        assert got[0] is buf
    ref = pre.step(frame, g, cam, origin, dn, counts=counts, **dict(dict(flags=default_flags), **kw))
    return frame, got, ref


class _Sequence:
    """frames[k] of a named sequence of accumulate_reference, computed on demand."""

    def __init__(self, rt, O, name):
        self.args = (rt, O, name)

    def __getitem__(self, k):
        return A.sequence_inputs(*self.args, k)


def _call(rt, O, pre, name, k, **kw):
    return _step(rt, pre, _Sequence(rt, O, name), k, default_flags=D.default_flags(name in R.MESH_FRAMES), **kw)


def _check(what, res, nan=None):
    frame, got, ref = res
    for plane, g, r in zip(PLANES, got, ref):
        if nan is not None and plane != "history":
            S.same_but_nan(g, r, f"{what} {plane}", nan, S.NAN_CAP)
        else:
            _same(g, r, f"{what} {plane}")


# ---- 1. rendered sequences -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,calls", [("three_spheres", 4), ("random_50x37", 4), ("tris300_floor", 4), ("staircase_a", 2)])
def test_rendered_sequences_match_the_reference(rt, O, name, calls):
    """Per step setCamera, runRenderer(1), a copy of the framebuffer, previewFrame(NULL, out, history, variance): all three of every call equal the reference fed
    the same copies.  Three calls stay on the spatial variance; the fourth takes the temporal one where the history held."""
    fb, o, mesh = _init(rt, O, name)
    assert rt.preview_frames() == 0
    pre, res, cnt = V.Previewer(), [], {}
    try:
        for k in range(calls):
            res.append(_call(rt, O, pre, name, k, fb=fb, counts=cnt))
            assert rt.preview_frames() == k + 1 and rt.last_preview_ms() > 0.0
    finally:
        rt.cleanupRenderer()
    print(name, {k: cnt.get(k, 0) for k in V.COUNTS})
    for k, r in enumerate(res):
        _check(f"{name} call {k}", r)
    assert float(res[-1][2][1].max()) > 1.0                     # the last call did blend
    assert cnt["spatial_variance"] > 0 and (cnt.get("temporal_variance", 0) > 0) == (calls >= 4)


# ---- 2. synthetic input, in place, over the parameter space ----------------------------------------------------------

_CASES = [dict(flags=0), dict(flags=1), dict(flags=2), dict(flags=3), dict(iterations=1), dict(iterations=8), dict(normal_squarings=0), dict(normal_squarings=7),
          dict(max_history=1), dict(max_history=2), dict(max_history=3), dict(max_history=4), dict(max_history=1024), dict(sigma_z=100.0), dict(sigma_z=1e-5), dict(normal_min=-1.0), dict(normal_min=1.0),
          dict(sigma_l=0.25), dict(sigma_l=64.0)]


def test_synthetic_input_in_place(rt, O):
    """random_50x37, seeded random images, uniform in [0, 4), passed explicitly with out == in, four calls along the sequence per parameter set.  From the
    reference's counts: the fourth call reaches the temporal variance unless max_history < 4 caps the history below RT_PREVIEW_MIN_HISTORY."""
    name = "random_50x37"
    fb, o, mesh = _init(rt, O, name)
    ny, nx = fb.shape[:2]
    try:
        for n, case in enumerate(_CASES):
            rt.reset_preview()
            pre, cnt = V.Previewer(), {}
            for k in range(4):
                res = _call(rt, O, pre, name, k, src=S.synthetic(300 + 4 * n + k, ny, nx), counts=cnt, **case)
                _check(f"{case} call {k}", res)
                if k == 2:
                    assert cnt.get("temporal_variance", 0) == 0
            print(case, {key: cnt.get(key, 0) for key in V.COUNTS}, "N max %.3f" % float(res[2][1].max()))
            assert float(res[2][1].max()) <= float(case.get("max_history", 32))
            if "max_history" in case or case == dict(flags=3):
                assert (cnt.get("temporal_variance", 0) > 0) == (case.get("max_history", 32) >= 4), cnt
    finally:
        rt.cleanupRenderer()


# ---- 3. the widest stride, and a frame that is no multiple of the tile -----------------------------------------------

def test_stride_16_taps_reach_real_pixels(rt, O):
    """random_96x64, two calls, the default five iterations: the taps of the last one lie 16 and 32 pixels away, inside the image for most pixels."""
    nx, ny = 96, 64
    sp, mt, frames = S.tiny_spheres(rt, O, nx, ny)
    fb = rt.initRendererSpheres(sp, mt, frames[0][0], nx, ny, 20)
    try:
        pre = V.Previewer()
        res = [_step(rt, pre, frames, k, fb=fb) for k in range(2)]
    finally:
        rt.cleanupRenderer()
    for k, r in enumerate(res):
        _check(f"96x64 call {k}", r)


def test_frame_that_is_no_multiple_of_the_tile(rt, O):
    """333 x 130 random spheres (10.4 x 16.25 tiles), 1 spp, two cameras one degree apart.  The per-pixel guide reference is too slow here: the guide planes are
    renderGuides' (pinned bit-exact by tests/test_gpu_guides.py) and P comes from the numpy restatement of the centre ray (pinned against orc_get_ray by
    tests/test_denoise_api.py)."""
    nx, ny = 333, 130
    sp, mt, cam0 = rt.scene_random_spheres(nx, ny)
    cams = [cam0, rt.make_camera(A.orbit((13, 2, 3), (0, 0, 0), 1.0), (0, 0, 0), (0, 1, 0), 30.0, nx / ny, 0.1, 10.0)]
    fb = rt.initRendererSpheres(sp, mt, cam0, nx, ny, 50)
    steps = []
    try:
        for cam in cams:
            rt.setCamera(cam)
            rt.runRenderer(1)
            frame = np.array(fb, copy=True)
            g = rt.renderGuides()
            steps.append((cam, frame, g, rt.previewFrame(history=True, variance=True), rt.last_preview_ms()))
    finally:
        rt.cleanupRenderer()
    pre, cnt = V.Previewer(), {}
    for k, (cam, frame, g, got, ms) in enumerate(steps):
        origin, dn = D.centre_dirs_numpy(cam, nx, ny)
        ref = pre.step(frame, g, cam, origin, dn, flags=D.default_flags(False), counts=cnt)
        print(f"333x130 call {k}: kernels {ms:.3f} ms")
        _check(f"333x130 call {k}", (frame, got, ref))
    print(cnt)
    assert cnt["blended"] > 0.4 * cnt["valid"]                  # (half of `valid` is the first call's)


# ---- 4. sizes around and below a tile --------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", S.TINY_SIZES)
def test_tiny_sphere_frames(rt, O, nx, ny):
    """The random-spheres scene from 1 x 1 to two tiles plus one: the 7 x 7 and the a-trous taps are mostly outside the image and read the pixel's own records."""
    sp, mt, frames = S.tiny_spheres(rt, O, nx, ny)
    rt.initRendererSpheres(sp, mt, frames[0][0], nx, ny, 20)
    try:
        pre = V.Previewer()
        res = [_step(rt, pre, frames, k, src=S.synthetic(320 + k, ny, nx)) for k in range(2)]
    finally:
        rt.cleanupRenderer()
    for k, r in enumerate(res):
        _check(f"{nx}x{ny} call {k}", r)


@pytest.mark.parametrize("nx,ny", S.TINY_MESH_SIZES)
def test_tiny_mesh_frames(rt, O, nx, ny):
    f, frames = S.tiny_mesh(rt, O, nx, ny)
    ks, keep = rt.make_kernel_scene(f["hm"], f["mats"], f["tex"], floor=f["floor"])
    rt.initRenderer(ks, frames[0][0], nx, ny, 16, keepalive=keep)
    try:
        rt.setRenderOptions(rt.getDefaultRenderOptions(False), floor=1)
        pre = V.Previewer()
        res = [_step(rt, pre, frames, k, src=S.synthetic(330 + k, ny, nx), default_flags=1) for k in range(2)]
    finally:
        rt.cleanupRenderer()
    for k, r in enumerate(res):
        _check(f"{nx}x{ny} mesh call {k}", r)


# ---- 5. special pixel values -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["no_hit_poison", "finite_extremes", "denormal"])
def test_edge_images(rt, O, kind):
    """random_96x64, two calls, each with an edge image of its own: non-finite values in pixels without a first hit never reach a pixel with one (a rejected tap
    is selected away, not multiplied by zero); denormals, signed zeros and negative radiance go through every stage as the reference's.  Plain bit equality."""
    nx, ny = 96, 64
    sp, mt, frames = S.tiny_spheres(rt, O, nx, ny)
    rt.initRendererSpheres(sp, mt, frames[0][0], nx, ny, 20)
    try:
        pre = V.Previewer()
        res = [_step(rt, pre, frames, k, src=S.edge_image(kind, frames[k][1]["prim"] != R.PRIM_NONE, 340 + k)) for k in range(2)]
    finally:
        rt.cleanupRenderer()
    for k, r in enumerate(res):
        _check(f"{kind} call {k}", r)
        valid = frames[k][1]["prim"] != R.PRIM_NONE
        assert np.isfinite(r[1][0][valid]).all() and np.array_equal(_bits(r[1][0][~valid]), _bits(r[0][~valid]))


def test_poison_in_first_hit_pixels(rt, O):
    """random_96x64, iterations = 1: NaN, +-Inf, +-FLT_MAX and 1e30 in one first-hit pixel each.  The definition carries a non-finite value to every pixel
    whose tap set holds it, whatever the tap's weight (0 * NaN).  The reference's NaN share of the first-hit pixels is computed first and lies under
    NAN_CAP; the NaN words are the reference's, every other word is bit-equal."""
    nx, ny = 96, 64
    sp, mt, frames = S.tiny_spheres(rt, O, nx, ny)
    cam, g, origin, dn = frames[0]
    valid = g["prim"] != R.PRIM_NONE
    src = S.edge_image("poison", valid, 350)
    ref = V.Previewer().step(src, g, cam, origin, dn, flags=3, iterations=1)
    shares = [S.nan_share(ref[0], valid), S.nan_share(ref[2], valid)]
    print("NaN share of the first-hit pixels: out %.4f, variance %.4f" % tuple(shares))
    assert 0.0 < max(shares) <= S.NAN_CAP
    rt.initRendererSpheres(sp, mt, cam, nx, ny, 20)
    try:
        res = _step(rt, V.Previewer(), frames, 0, src=src, flags=3, iterations=1)
    finally:
        rt.cleanupRenderer()
    _check("poison", res, nan=valid)


# ---- 6. what resets the history and what does not ---------------------------------------------------------------------

def test_reset_rules(rt, O):
    """rtResetPreview, setRenderOptions and a second init with another size (without cleanupRenderer) make the next call a first call; setCamera and
    setExternalFramebuffer do not; rtPreviewFrames follows."""
    name = "random_50x37"
    fb, o, mesh = _init(rt, O, name)
    ny, nx = fb.shape[:2]
    src = [S.synthetic(360 + k, ny, nx) for k in range(6)]
    res = {}
    try:
        assert rt.preview_frames() == 0
        pre = V.Previewer()
        res["first"] = _call(rt, O, pre, name, 0, src=src[0])
        res["after setCamera"] = _call(rt, O, pre, name, 1, src=src[1])
        ext = np.zeros((ny, nx, 3), np.float32)
        rt.setExternalFramebuffer(ext)
        res["after setExternalFramebuffer"] = _call(rt, O, pre, name, 2, src=src[2])
        rt.setExternalFramebuffer(None)
        assert rt.preview_frames() == 3
        rt.reset_preview()
        assert rt.preview_frames() == 0
        pre = V.Previewer()
        res["after reset"] = _call(rt, O, pre, name, 1, src=src[3])
        res["after reset, second"] = _call(rt, O, pre, name, 2, src=src[4])
        assert rt.preview_frames() == 2
        rt.setRenderOptions(o)
        assert rt.preview_frames() == 0
        res["after setRenderOptions"] = _call(rt, O, V.Previewer(), name, 0, src=src[5])
        assert rt.preview_frames() == 1
        fb2, o2, mesh2 = _init(rt, O, "three_spheres")          # 64 x 40 after 50 x 37, the buffers live
        assert rt.preview_frames() == 0
        pre = V.Previewer()
        res["after second init"] = _call(rt, O, pre, "three_spheres", 1, fb=fb2)
        res["after second init, second"] = _call(rt, O, pre, "three_spheres", 2, fb=fb2)
        rt.setRenderOptions(o2, stripe_rows=8, part_rank=1, part_world=2)      # a new device layout: the buffers are freed
        assert rt.preview_frames() == 0
        pre = V.Previewer()
        res["after a new layout"] = _call(rt, O, pre, "three_spheres", 0, src=S.synthetic(366, 40, 64))
        res["after a new layout, second"] = _call(rt, O, pre, "three_spheres", 1, src=S.synthetic(367, 40, 64))
        rt.setRenderOptions(o2, stripe_rows=64, part_rank=1, part_world=2)     # this process owns no row at all
        pre = V.Previewer()
        res["a rank without rows"] = _call(rt, O, pre, "three_spheres", 0, src=S.synthetic(368, 40, 64))
        res["a rank without rows, second"] = _call(rt, O, pre, "three_spheres", 1, src=S.synthetic(369, 40, 64))
        assert rt.preview_frames() == 2
    finally:
        rt.cleanupRenderer()
    for what, r in res.items():
        _check(what, r)
        first = not (what.endswith(", second") or what in ("after setCamera", "after setExternalFramebuffer"))
        assert (float(r[1][1].max()) == 1.0) == first, what


# ---- 7. no side effects, and the three passes side by side -------------------------------------------------------------

@pytest.mark.parametrize("name", ["random_50x37", "staircase_a"])
def test_no_side_effects(rt, O, name):
    """Framebuffer, stats, launch report, the other timings, the results of later denoiseFrame and accumulateFrame calls and the progressive frame are the same
    with and without previewFrame calls in between."""
    fb, o, mesh = _init(rt, O, name)
    try:
        rt.runRenderer(4)
        four = np.array(fb, copy=True)
        rt.renderGuides()
        den = rt.denoiseFrame(four)
        rt.accumulateFrame(four)
        rt.runRenderer(2)
        frame, stats, launches = np.array(fb, copy=True), _stats_tuple(rt.getRenderStats()), rt.last_launches()
        timings = (rt.last_guides_ms(), rt.last_denoise_ms(), rt.last_accumulate_ms())
        assert launches and min(timings) > 0.0
        rt.previewFrame()
        rt.previewFrame(four, history=True, variance=True, max_history=2)
        assert rt.preview_frames() == 2 and rt.history_frames() == 1
        assert np.array_equal(_bits(fb), _bits(frame))
        assert _stats_tuple(rt.getRenderStats()) == stats
        assert rt.last_launches() == launches
        assert (rt.last_guides_ms(), rt.last_denoise_ms(), rt.last_accumulate_ms()) == timings
        assert np.array_equal(_bits(rt.denoiseFrame(four)), _bits(den))
        rt.runRendererProgressive(2)
        assert rt.progressive_samples() == 2
        rt.previewFrame()
        assert rt.progressive_samples() == 2 and rt.preview_frames() == 3
        rt.runRendererProgressive(2)
        assert rt.progressive_samples() == 4
        total = np.array(fb, copy=True)
    finally:
        rt.cleanupRenderer()
    assert np.array_equal(_bits(total), _bits(four))


def test_interleaved_with_accumulate_and_denoise(rt, O):
    """accumulateFrame, denoiseFrame, renderGuides and previewFrame interleaved over three cameras: each equals its own reference, which saw none of the others."""
    name = "random_50x37"
    fb, o, mesh = _init(rt, O, name)
    acc, pre = A.Accumulator(), V.Previewer()
    steps = []
    try:
        for k in range(3):
            cam, g, origin, dn = A.sequence_inputs(rt, O, name, k)
            p = _call(rt, O, pre, name, k, fb=fb)               # (setCamera, runRenderer(1))
            a, hist = rt.accumulateFrame(p[0], history=True)
            d = rt.denoiseFrame(a, sigma_c=0.5)
            planes = rt.renderGuides()
            steps.append((p, a, hist, d, planes))
            assert rt.preview_frames() == rt.history_frames() == k + 1
    finally:
        rt.cleanupRenderer()
    for k, (p, a, hist, d, planes) in enumerate(steps):
        cam, g, origin, dn = A.sequence_inputs(rt, O, name, k)
        _check(f"preview {k}", p)
        ref, N = acc.step(p[0], g, cam, origin, dn, flags=D.default_flags(False))
        _same(a, ref, f"accumulate {k} out"); _same(hist, N, f"accumulate {k} history")
        _same(d, D.denoise(a, g, origin, dn, **dict(D.DEFAULTS, flags=D.default_flags(False), sigma_c=0.5)), f"denoise {k}")
        for plane in ("albedo", "normal", "depth", "prim"):
            _same(planes[plane], g[plane], f"renderGuides {k} {plane}")


def test_two_in_process_devices(rt, O):
    if rt.device_count() < 2:
        pytest.skip("needs two HIP devices")
    name = "random_50x37"
    fb, o, mesh = _init(rt, O, name, devices=[0, 1])
    try:
        pre = V.Previewer()
        steps = [_call(rt, O, pre, name, k, fb=fb) for k in range(2)]
    finally:
        rt.cleanupRenderer()
    for k, r in enumerate(steps):
        _check(f"two devices call {k}", r)


# ---- 8. misuse -------------------------------------------------------------------------------------------------------

_SPHERES = ("sp, mt, cam = rt.scene_random_spheres(64, 48); rt.initRendererSpheres(sp, mt, cam, 64, 48, 10)\n"
            "a = np.zeros((48, 64, 3), np.float32); call = rt.load_renderer().previewFrame; p = a.ctypes.data\n")
_ARGS = dict(flags=3, max_history=32, iterations=5, normal_squarings=5, sigma_z=0.01, normal_min=0.9, sigma_l=4.0)


def _bad(**kw):
    return _SPHERES + "call(p, p, None, None, %s)\n" % ", ".join(str(v) for v in dict(_ARGS, **kw).values())


_MISUSE = {
    "out_null": _SPHERES + "call(p, None, None, None, 3, 32, 5, 5, 0.01, 0.9, 4.0)\n",
    "unknown_flag": _bad(flags=4),
    "max_history_0": _bad(max_history=0), "max_history_1025": _bad(max_history=1025), "max_history_negative": _bad(max_history=-1),
    "iterations_0": _bad(iterations=0), "iterations_9": _bad(iterations=9),
    "normal_squarings_negative": _bad(normal_squarings=-1), "normal_squarings_8": _bad(normal_squarings=8),
    "sigma_z_zero": _bad(sigma_z=0.0), "sigma_z_negative": _bad(sigma_z=-0.01), "sigma_z_nan": _bad(sigma_z="float('nan')"), "sigma_z_inf": _bad(sigma_z="float('inf')"),
    "normal_min_nan": _bad(normal_min="float('nan')"), "normal_min_inf": _bad(normal_min="float('inf')"), "normal_min_above_1": _bad(normal_min=1.5),
    "normal_min_below_minus_1": _bad(normal_min=-1.5),
    "sigma_l_zero": _bad(sigma_l=0.0), "sigma_l_negative": _bad(sigma_l=-4.0), "sigma_l_nan": _bad(sigma_l="float('nan')"), "sigma_l_inf": _bad(sigma_l="float('inf')"),
    "floor_on_spheres": _SPHERES + "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); call(p, p, None, None, 3, 32, 5, 5, 0.01, 0.9, 4.0)\n",
    "after_cleanup": _SPHERES + "rt.cleanupRenderer(); call(p, p, None, None, 3, 32, 5, 5, 0.01, 0.9, 4.0)\n",
    "reset_after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.reset_preview()\n",
    "frames_after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.preview_frames()\n",
}


@pytest.mark.parametrize("case", sorted(_MISUSE))
def test_misuse_exits_99(case):
    """The library's misuse convention, each case in a child process of its own: 'rt error' on stderr and exit status 99 (a clean exit of a host-side check)."""
    exits_99(_MISUSE[case])


def test_valid_edge_parameters_are_accepted(rt, O):
    """The other side of the misuse list: the ends of every range, no optional plane, every flag combination."""
    fb, o, mesh = _init(rt, O, "tie")
    try:
        rt.runRenderer(1)
        for kw in (dict(max_history=1, normal_min=-1.0, flags=0, iterations=1, normal_squarings=0), dict(flags=1), dict(flags=2),
                   dict(max_history=rt.RT_ACCUM_MAX_HISTORY, normal_min=1.0, flags=3, iterations=rt.RT_DENOISE_MAX_ITERATIONS,
                        normal_squarings=rt.RT_DENOISE_MAX_SQUARINGS, sigma_l=1e-6)):
            out = rt.previewFrame(**kw)
            assert isinstance(out, np.ndarray) and np.isfinite(out).all()
        out, var = rt.previewFrame(variance=True)
        assert np.isfinite(var).all() and float(var.min()) >= 0.0
        assert rt.last_preview_ms() > 0.0 and rt.preview_frames() == 5
    finally:
        rt.cleanupRenderer()
