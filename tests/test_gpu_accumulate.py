"""accumulateFrame (include/rt_api.h) on the GPU against the test reference (tests/accumulate_reference.py): every call, all pixels, out and the history length,
bit for bit (np.array_equal on the raw 32-bit words: no tolerance, nothing left out).  The reference is fed the very framebuffers the GPU rendered (copied
before the call) and the guide reference's planes, and keeps its own history, so nothing here leans on render parity.  Then synthetic input in place over the
parameter space, one large frame, the reset rules, the interplay with denoiseFrame and renderGuides, no side effects, partitions and the misuse exits."""
import numpy as np
import pytest

import accumulate_reference as A
import denoise_reference as D
import guides_reference as R
from preview_support import bits as _bits, exits_99, init_frame as _init, same as _same, stats_tuple as _stats_tuple

pytestmark = pytest.mark.gpu


def _synthetic(seed, shape):
    return np.random.default_rng(seed).uniform(0, 4, shape + (3,)).astype(np.float32)


def _call(rt, O, acc, name, k, src=None, fb=None, still=False, counts=None, **kw):
    """One step on both sides: setCamera(frame k's camera); src None: runRenderer(1) and a copy of the framebuffer as the input, passed as NULL; else src is
    passed explicitly with out == in.  Returns (input, got out, got N, reference out, reference N)."""
    cam, g, origin, dn = A.sequence_inputs(rt, O, name, k, still)
    rt.setCamera(cam)
    if src is None:
        rt.runRenderer(1)
        frame = np.array(fb, copy=True)
        got, hist = rt.accumulateFrame(history=True, **kw)
        assert np.array_equal(_bits(fb), _bits(frame))          # the framebuffer was the input, not the output
    else:
        frame = src.copy()
        buf = src.copy()
        got, hist = rt.accumulateFrame(buf, out=buf, history=True, **kw)
        assert got is buf
    ref, N = acc.step(frame, g, cam, origin, dn, counts=counts, **dict(dict(flags=D.default_flags(name in R.MESH_FRAMES)), **kw))
    return frame, got, hist, ref, N


# ---- 1. rendered sequences -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,calls", [("three_spheres", 3), ("random_50x37", 3), ("tris300_floor", 3), ("staircase_a", 2)])
def test_rendered_sequences_match_the_reference(rt, O, name, calls):
    """Per step setCamera, runRenderer(1), a copy of the framebuffer, accumulateFrame(NULL, out, history): out and history of every call equal the reference
    fed the same copies."""
    fb, o, mesh = _init(rt, O, name)
    assert rt.history_frames() == 0
    acc, res = A.Accumulator(), []
    try:
        for k in range(calls):
            res.append(_call(rt, O, acc, name, k, fb=fb))
            assert rt.history_frames() == k + 1 and rt.last_accumulate_ms() > 0.0
    finally:
        rt.cleanupRenderer()
    for k, (frame, got, hist, ref, N) in enumerate(res):
        valid = N > 0
        print(f"{name} call {k}: mean N {float(N[valid].mean()):.3f}, {float((D.ulp_distance(ref, frame).max(axis=-1) > 1)[valid].mean()):.3f} of the valid pixels change")
        _same(hist, N, f"{name} call {k} history")
        _same(got, ref, f"{name} call {k} out")
    assert float(res[-1][4].max()) > 1.0                        # the last call did blend


# ---- 2. synthetic input, in place, over the parameter space ----------------------------------------------------------

_CASES = [dict(flags=0), dict(flags=1), dict(flags=2), dict(flags=3), dict(max_history=1), dict(max_history=2), dict(normal_min=-1.0), dict(normal_min=1.0),
          dict(sigma_z=100.0), dict(sigma_z=1e-5), dict(flags=0, max_history=1024, sigma_z=100.0, normal_min=-1.0)]


def test_synthetic_input_in_place(rt, O):
    """random_50x37, seeded random images, uniform in [0, 4), passed explicitly with out == in, three calls along the sequence per parameter set (the third
    shows max_history = 2).  sigma_z = 100 accepts nearly every tap that passes the other tests, 1e-5 nearly none; normal_min = 1 leaves equal normals only."""
    name = "random_50x37"
    fb, o, mesh = _init(rt, O, name)
    ny, nx = fb.shape[:2]
    try:
        for n, case in enumerate(_CASES):
            rt.reset_history()
            acc, cnt = A.Accumulator(), {}
            for k in range(3):
                frame, got, hist, ref, N = _call(rt, O, acc, name, k, src=_synthetic(100 + 3 * n + k, (ny, nx)), counts=cnt, **case)
                _same(hist, N, f"{case} call {k} history")
                _same(got, ref, f"{case} call {k} out")
            print(case, {key: cnt[key] for key in A.COUNTS}, "N max %.3f" % float(N.max()))
            assert float(N.max()) <= float(case.get("max_history", 32))
    finally:
        rt.cleanupRenderer()


def test_camera_turned_away_and_camera_unchanged(rt, O):
    """A camera that turns its back on the previous one: the hit points lie behind the previous camera, no pixel is a candidate and the call returns what a
    first call returns.  Then the same camera three times: every valid pixel reprojects onto itself (x = i up to rounding)."""
    name = "random_50x37"
    sp, mt, cam0, nx, ny = R.sphere_frame(rt, name)
    away = rt.make_camera((13, 2, 3), (26, 0, 6), (0, 1, 0), 30.0, nx / ny, 0.1, 10.0)
    g_away = R.sphere_guides(rt, O, sp, mt, away, nx, ny)
    o_away, dn_away = D.centre_dirs(rt, O, away, nx, ny)
    fb, o, mesh = _init(rt, O, name)
    try:
        acc, cnt = A.Accumulator(), {}
        first = _call(rt, O, acc, name, 0, src=_synthetic(7, (ny, nx)))
        rt.setCamera(away)
        src = _synthetic(8, (ny, nx))
        got, hist = rt.accumulateFrame(src, history=True)
        ref, N = acc.step(src, g_away, away, o_away, dn_away, counts=cnt)
        fresh, _ = A.Accumulator().step(src, g_away, away, o_away, dn_away)
        # the unchanged camera: three calls at frame 0
        rt.reset_history()
        acc2, cnt2 = A.Accumulator(), {}
        same = [_call(rt, O, acc2, name, 0, src=_synthetic(9 + k, (ny, nx)), counts=cnt2) for k in range(3)]
    finally:
        rt.cleanupRenderer()
    print("turned away", cnt, "unchanged", cnt2)
    assert cnt["valid"] > 0 and cnt["candidate"] == 0
    _same(got, ref, "turned away out"); _same(hist, N, "turned away history"); _same(ref, fresh, "turned away = a first call")
    assert cnt2["no_candidate"] == 0 and cnt2["blended"] == cnt2["valid"] > 0
    for k, (frame, g, h, ref, N) in enumerate(same):
        _same(g, ref, f"unchanged camera call {k} out"); _same(h, N, f"unchanged camera call {k} history")


# ---- 3. one large frame ----------------------------------------------------------------------------------------------

def test_large_frame(rt, O):
    """1200 x 800 random spheres, 1 spp, two cameras one degree apart.  The per-pixel guide reference is too slow here: the guide planes are renderGuides'
    (pinned bit-exact by tests/test_gpu_guides.py) and P comes from the numpy restatement of the centre ray (pinned against orc_get_ray by
    tests/test_denoise_api.py)."""
    nx, ny = 1200, 800
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
            got, hist = rt.accumulateFrame(history=True)
            steps.append((cam, frame, g, got, hist, rt.last_accumulate_ms()))
    finally:
        rt.cleanupRenderer()
    acc, cnt = A.Accumulator(), {}
    for k, (cam, frame, g, got, hist, ms) in enumerate(steps):
        origin, dn = D.centre_dirs_numpy(cam, nx, ny)
        ref, N = acc.step(frame, g, cam, origin, dn, flags=D.default_flags(False), counts=cnt)
        print(f"1200x800 call {k}: kernel {ms:.3f} ms")
        _same(hist, N, f"1200x800 call {k} history")
        _same(got, ref, f"1200x800 call {k} out")
    print(cnt)
    assert cnt["blended"] > 0.9 * cnt["valid"]


# ---- 4. what resets the history and what does not ---------------------------------------------------------------------

def test_reset_rules(rt, O):
    """rtResetHistory, setRenderOptions and a second init with another size make the next call a first call; setCamera and setExternalFramebuffer do not;
    rtHistoryFrames follows."""
    name = "random_50x37"
    fb, o, mesh = _init(rt, O, name)
    ny, nx = fb.shape[:2]
    src = [_synthetic(40 + k, (ny, nx)) for k in range(8)]
    try:
        assert rt.history_frames() == 0
        acc = A.Accumulator()
        a = _call(rt, O, acc, name, 0, src=src[0])
        assert rt.history_frames() == 1
        b = _call(rt, O, acc, name, 1, src=src[1])              # (setCamera in between)
        assert rt.history_frames() == 2
        ext = np.zeros((ny, nx, 3), np.float32)
        rt.setExternalFramebuffer(ext)
        c = _call(rt, O, acc, name, 2, src=src[2])
        rt.setExternalFramebuffer(None)
        assert rt.history_frames() == 3
        rt.reset_history()
        assert rt.history_frames() == 0
        acc_d = A.Accumulator()
        d = _call(rt, O, acc_d, name, 1, src=src[3])
        e = _call(rt, O, acc_d, name, 2, src=src[4])
        assert rt.history_frames() == 2
        rt.setRenderOptions(o)
        assert rt.history_frames() == 0
        acc_f = A.Accumulator()
        f = _call(rt, O, acc_f, name, 0, src=src[5])
        assert rt.history_frames() == 1
        fb2, o2, mesh2 = _init(rt, O, "three_spheres")                 # 64 x 40 after 50 x 37
        assert rt.history_frames() == 0
        acc_g = A.Accumulator()
        g = _call(rt, O, acc_g, "three_spheres", 1, fb=fb2)
        h = _call(rt, O, acc_g, "three_spheres", 2, fb=fb2)
        assert rt.history_frames() == 2
    finally:
        rt.cleanupRenderer()
    for what, (frame, got, hist, ref, N) in dict(first=a, after_setCamera=b, after_setExternalFramebuffer=c, after_reset=d, after_reset_second=e,
                                                 after_setRenderOptions=f, after_second_init=g, after_second_init_second=h).items():
        _same(got, ref, what + " out"); _same(hist, N, what + " history")
    for first in (a, d, f, g):
        assert float(first[2].max()) == 1.0
    for later in (b, c, e, h):
        assert float(later[2].max()) > 1.0


# ---- 5. interplay with denoiseFrame and renderGuides -----------------------------------------------------------------

def test_interplay_with_denoise_and_guides(rt, O):
    """accumulate, denoiseFrame, renderGuides, setCamera, accumulate: the second result is the reference's (neither call disturbed the history), and the denoised
    frame is denoise_reference of its input."""
    name = "random_50x37"
    fb, o, mesh = _init(rt, O, name)
    try:
        acc = A.Accumulator()
        a = _call(rt, O, acc, name, 0, fb=fb)
        den = rt.denoiseFrame(a[1])
        planes = rt.renderGuides()
        b = _call(rt, O, acc, name, 1, fb=fb)
        den2 = rt.denoiseFrame(b[1], sigma_c=0.5)
    finally:
        rt.cleanupRenderer()
    for k, (frame, got, hist, ref, N) in enumerate((a, b)):
        _same(got, ref, f"call {k} out"); _same(hist, N, f"call {k} history")
    for k, got, kw in ((0, den, {}), (1, den2, dict(sigma_c=0.5))):
        cam, g, origin, dn = A.sequence_inputs(rt, O, name, k)
        _same(got, D.denoise((a, b)[k][1], g, origin, dn, **dict(dict(D.DEFAULTS, flags=D.default_flags(False)), **kw)), f"denoised {k}")
    g0 = A.sequence_inputs(rt, O, name, 0)[1]
    for plane in ("albedo", "normal", "depth", "prim"):
        _same(planes[plane], g0[plane], "renderGuides " + plane)


def test_both_passes_live_through_reinit_relayout_and_cleanup(rt, O):
    """Both passes allocated, then: a second init with another size without cleanupRenderer, a setRenderOptions that replaces the device layout, cleanupRenderer
    and a third init.  The history is empty after each; every out, history plane and denoised frame equals the references, which start afresh there."""
    small, large = "random_50x37", "random_96x64"
    res, den = {}, {}
    try:
        fb, o, mesh = _init(rt, O, small)
        acc = A.Accumulator()
        res["first 0"] = _call(rt, O, acc, small, 0, fb=fb)
        res["first 1"] = _call(rt, O, acc, small, 1, fb=fb)
        den["first"] = (rt.denoiseFrame(res["first 1"][1]), res["first 1"][1], A.sequence_inputs(rt, O, small, 1)[1:])
        fb, o, mesh = _init(rt, O, large)                       # 96 x 64 after 50 x 37, both passes' buffers live
        assert rt.history_frames() == 0
        cam = R.sphere_frame(rt, large)[2]
        g, origin, dn, _ = D.frame_inputs(rt, O, large)
        acc = A.Accumulator()
        rt.runRenderer(1)
        frame = np.array(fb, copy=True)
        got, hist = rt.accumulateFrame(history=True)
        res["second init"] = (frame, got, hist) + acc.step(frame, g, cam, origin, dn, flags=D.default_flags(False))
        den["second init"] = (rt.denoiseFrame(got), got, (g, origin, dn))
        rt.setRenderOptions(o, stripe_rows=8, part_rank=1, part_world=2)
        assert rt.history_frames() == 0
        acc = A.Accumulator()
        src = _synthetic(80, fb.shape[:2])
        got, hist = rt.accumulateFrame(src, history=True)
        res["new layout"] = (src, got, hist) + acc.step(src, g, cam, origin, dn, flags=D.default_flags(False))
        src = _synthetic(81, fb.shape[:2])
        den["new layout"] = (rt.denoiseFrame(src), src, (g, origin, dn))
        rt.cleanupRenderer()
        fb, o, mesh = _init(rt, O, small)
        assert rt.history_frames() == 0
        res["third init"] = _call(rt, O, A.Accumulator(), small, 0, fb=fb)
        den["third init"] = (rt.denoiseFrame(res["third init"][1]), res["third init"][1], A.sequence_inputs(rt, O, small, 0)[1:])
    finally:
        rt.cleanupRenderer()
    for what, (frame, got, hist, ref, N) in res.items():
        _same(got, ref, what + " out"); _same(hist, N, what + " history")
    for what in ("second init", "new layout", "third init"):
        assert float(res[what][4].max()) == 1.0                 # a first call
    assert float(res["first 1"][4].max()) > 1.0
    for what, (got, src, (g, origin, dn)) in den.items():
        _same(got, D.denoise(src, g, origin, dn, flags=D.default_flags(False), **D.DEFAULTS), what + " denoised")


# ---- 6. no side effects ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["random_50x37", "staircase_a"])
def test_no_side_effects(rt, O, name):
    """Framebuffer, stats, launch report, guide and denoise timing, a later denoiseFrame and the progressive frame are the same with and without accumulateFrame
    calls in between."""
    fb, o, mesh = _init(rt, O, name)
    try:
        rt.runRenderer(4)
        four = np.array(fb, copy=True)
        rt.renderGuides()
        den = rt.denoiseFrame(four)
        rt.runRenderer(2)
        frame, stats, launches = np.array(fb, copy=True), _stats_tuple(rt.getRenderStats()), rt.last_launches()
        guides_ms, denoise_ms = rt.last_guides_ms(), rt.last_denoise_ms()
        assert launches and guides_ms > 0.0 and denoise_ms > 0.0
        rt.accumulateFrame()
        rt.accumulateFrame(four, history=True, max_history=2)
        assert rt.history_frames() == 2
        assert np.array_equal(_bits(fb), _bits(frame))
        assert _stats_tuple(rt.getRenderStats()) == stats
        assert rt.last_launches() == launches
        assert rt.last_guides_ms() == guides_ms and rt.last_denoise_ms() == denoise_ms
        assert np.array_equal(_bits(rt.denoiseFrame(four)), _bits(den))
        rt.runRendererProgressive(2)
        assert rt.progressive_samples() == 2
        rt.accumulateFrame()
        assert rt.progressive_samples() == 2 and rt.history_frames() == 3
        rt.runRendererProgressive(2)
        assert rt.progressive_samples() == 4
        total = np.array(fb, copy=True)
    finally:
        rt.cleanupRenderer()
    assert np.array_equal(_bits(total), _bits(four))


# ---- 7. partitions ---------------------------------------------------------------------------------------------------

def test_partitioned_renderer_still_accumulates_the_whole_image(rt, O):
    """part_world = 2, part_rank = 1 with stripes of 8 rows, then a partition in which this process owns no row at all: two calls with explicit full inputs
    return the whole-image results of the reference."""
    name = "random_50x37"
    fb, o, mesh = _init(rt, O, name)
    ny, nx = fb.shape[:2]
    res = {}
    try:
        for what, opts in (("rank 1 of 2", dict(stripe_rows=8, part_rank=1, part_world=2)), ("a rank without rows", dict(stripe_rows=64, part_rank=1, part_world=2))):
            rt.setRenderOptions(o, **opts)
            assert rt.history_frames() == 0
            acc = A.Accumulator()
            res[what] = [_call(rt, O, acc, name, k, src=_synthetic(60 + k, (ny, nx))) for k in range(2)]
    finally:
        rt.cleanupRenderer()
    for what, steps in res.items():
        for k, (frame, got, hist, ref, N) in enumerate(steps):
            _same(got, ref, f"{what} call {k} out"); _same(hist, N, f"{what} call {k} history")


def test_two_in_process_devices(rt, O):
    if rt.device_count() < 2:
        pytest.skip("needs two HIP devices")
    name = "random_50x37"
    fb, o, mesh = _init(rt, O, name, devices=[0, 1])
    try:
        acc = A.Accumulator()
        steps = [_call(rt, O, acc, name, k, fb=fb) for k in range(2)]
    finally:
        rt.cleanupRenderer()
    for k, (frame, got, hist, ref, N) in enumerate(steps):
        _same(got, ref, f"two devices call {k} out"); _same(hist, N, f"two devices call {k} history")


# ---- 8. misuse -------------------------------------------------------------------------------------------------------

_SPHERES = ("sp, mt, cam = rt.scene_random_spheres(64, 48); rt.initRendererSpheres(sp, mt, cam, 64, 48, 10)\n"
            "a = np.zeros((48, 64, 3), np.float32); call = rt.load_renderer().accumulateFrame; p = a.ctypes.data\n")
_MISUSE = {
    "out_null": _SPHERES + "call(p, None, None, 3, 32, 0.01, 0.9)\n",
    "unknown_flag": _SPHERES + "call(p, p, None, 4, 32, 0.01, 0.9)\n",
    "max_history_0": _SPHERES + "call(p, p, None, 3, 0, 0.01, 0.9)\n",
    "max_history_1025": _SPHERES + "call(p, p, None, 3, 1025, 0.01, 0.9)\n",
    "sigma_z_zero": _SPHERES + "call(p, p, None, 3, 32, 0.0, 0.9)\n",
    "sigma_z_negative": _SPHERES + "call(p, p, None, 3, 32, -0.01, 0.9)\n",
    "sigma_z_nan": _SPHERES + "call(p, p, None, 3, 32, float('nan'), 0.9)\n",
    "sigma_z_inf": _SPHERES + "call(p, p, None, 3, 32, float('inf'), 0.9)\n",
    "normal_min_nan": _SPHERES + "call(p, p, None, 3, 32, 0.01, float('nan'))\n",
    "max_history_negative": _SPHERES + "call(p, p, None, 3, -1, 0.01, 0.9)\n",
    "normal_min_inf": _SPHERES + "call(p, p, None, 3, 32, 0.01, float('inf'))\n",
    "normal_min_minus_inf": _SPHERES + "call(p, p, None, 3, 32, 0.01, float('-inf'))\n",
    "normal_min_above_1": _SPHERES + "call(p, p, None, 3, 32, 0.01, 1.5)\n",
    "normal_min_below_minus_1": _SPHERES + "call(p, p, None, 3, 32, 0.01, -1.5)\n",
    "floor_on_spheres": _SPHERES + "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); call(p, p, None, 3, 32, 0.01, 0.9)\n",
    "after_cleanup": _SPHERES + "rt.cleanupRenderer(); call(p, p, None, 3, 32, 0.01, 0.9)\n",
    "reset_after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.reset_history()\n",
    "frames_after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.history_frames()\n",
}


@pytest.mark.parametrize("case", sorted(_MISUSE))
def test_misuse_exits_99(case):
    """The library's misuse convention, each case in a child process of its own: 'rt error' on stderr and exit status 99 (a clean exit of a host-side check)."""
    exits_99(_MISUSE[case])


def test_valid_edge_parameters_are_accepted(rt, O):
    """The other side of the misuse list: max_history 1 and RT_ACCUM_MAX_HISTORY, normal_min -1 and 1, no history plane, every flag combination."""
    fb, o, mesh = _init(rt, O, "tie")
    try:
        rt.runRenderer(1)
        for kw in (dict(max_history=1, normal_min=-1.0, flags=0), dict(max_history=rt.RT_ACCUM_MAX_HISTORY, normal_min=1.0, flags=3), dict(flags=1), dict(flags=2)):
            out = rt.accumulateFrame(**kw)
            assert isinstance(out, np.ndarray) and np.isfinite(out).all()
        assert rt.last_accumulate_ms() > 0.0 and rt.history_frames() == 4
    finally:
        rt.cleanupRenderer()
