"""displayFrame (include/rt_api.h) on the GPU against the test reference (tests/display_reference.py, libm's powf): the RGBA bytes of every call with
np.array_equal - all pixels, no tolerance - and with them rtLastExposure (its bits) and the histogram.  Rendered frames, synthetic frames at sizes on both sides
of a wave, a workgroup and the dither tile, special pixel values, the adaptation and what restarts it, RT_DISPLAY_FROM_PREVIEW, no side effects, partitions,
the misuse exits."""
import numpy as np
import pytest

import display_reference as D
from preview_support import bits as _bits, exits_99, init_frame as _init, stats_tuple as _stats_tuple

pytestmark = pytest.mark.gpu
A = D.AUTO_EXPOSURE
ALL = D.TOP_DOWN | D.DITHER | D.AUTO_EXPOSURE


def _f32_bits(x):
    return int(np.float32(x).view(np.uint32))


_check = D.check                # one call on both sides, bit for bit (shared with tests/test_gpu_capped_grids.py)


def _spheres(rt, nx, ny):
    sp, mt, cam = rt.scene_three_spheres(nx, ny)
    return rt.initRendererSpheres(sp, mt, cam, nx, ny, 20)


# ---- 1. rendered frames ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_spheres", "tris300_floor"])
def test_rendered_frames(rt, O, name):
    """After runRenderer(1): in = NULL and the same frame passed explicitly, all three tone maps, each flag alone and all together.  The exposure state runs
    through the whole sequence on both sides."""
    fb, o, mesh = _init(rt, O, name)
    try:
        assert rt.last_exposure() == 1.0 and not rt.display_histogram().any() and rt.last_display_ms() == 0.0
        rt.runRenderer(1)
        frame = np.array(fb, copy=True)
        assert np.isfinite(frame).all() and float(frame.max()) > 0.0
        ref = D.Display()
        for tonemap, flags in D.CASES:
            _check(rt, ref, frame, None, flags, tonemap, what=f"{name} NULL")
            _check(rt, ref, frame, frame, flags, tonemap, exposure=1.7, adapt=0.5, what=f"{name} explicit")
            assert np.array_equal(_bits(fb), _bits(frame))
    finally:
        rt.cleanupRenderer()


# ---- 2. synthetic frames -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", D.SIZES)
def test_synthetic_frames(rt, nx, ny):
    """Values over 2^-20 .. 2^20 with luminances exactly on bin edges, in the first and the last bin and beyond both, negative channels
    (tests/test_display_api.py::test_synthetic_frames_cover_the_edges says what the largest holds): every tone map and flag set, two calls each."""
    frame = D.synthetic(100 + nx, nx, ny)
    _spheres(rt, nx, ny)
    try:
        ref = D.Display()
        for tonemap, flags in D.CASES:
            _check(rt, ref, frame, np.ascontiguousarray(frame), flags, tonemap, what=f"{nx}x{ny}")
            _check(rt, ref, frame, np.ascontiguousarray(frame), flags, tonemap, exposure=0.37, adapt=0.5, what=f"{nx}x{ny}")
    finally:
        rt.cleanupRenderer()


# ---- 3. special pixel values -------------------------------------------------------------------------------------------

def test_special_pixels(rt):
    """NaN and -inf encode to 0, +inf, 1e30 and FLT_MAX to 255, denormals and both zeros to 0; non-finite and non-positive luminance is left out of the
    histogram; an all-black frame gives T = 0 and E = 1.  Every tone map and flag set equals the reference on the special frame; rtLinearToSRGB itself is
    compared on the finite inputs below 2^40 only, where the C conversion is defined."""
    frame = np.ascontiguousarray(D.special_frame())
    ny, nx = frame.shape[:2]
    fb = _spheres(rt, nx, ny)
    try:
        ref = D.Display()
        for tonemap, flags in D.CASES:
            _check(rt, ref, frame, frame, flags, tonemap, what="special")
        plain = rt.display_frame(frame)
        code = {v: [int(plain[k, col, k]) for k in range(3)] for col, v in enumerate(map(repr, D.SPECIAL_VALUES))}
        print(code)
        assert code["nan"] == [0] * 3 and code["-inf"] == [0] * 3 and code["-1e+30"] == [0] * 3 and code["1e-40"] == [0] * 3 and code["-0.0"] == [0] * 3
        assert code["inf"] == [255] * 3 and code["1e+30"] == [255] * 3 and code["3.4028234e+38"] == [255] * 3 and (plain[..., 3] == 255).all()
        h = rt.load_host()
        finite = np.isfinite(frame) & (np.abs(frame) < 2.0 ** 40)
        want = np.array([h.rtLinearToSRGB(float(x)) for x in frame[finite]], np.uint32)
        assert finite.sum() > 60 and np.array_equal(plain[..., :3][finite].astype(np.uint32), want)
        rt.reset_display()
        rt.display_frame(frame, flags=A)
        l = D.lum(frame)
        hist = rt.display_histogram()
        assert hist.sum() == int((np.isfinite(l) & (l > 0)).sum()) < l.size
        rt.reset_display()
        fb[...] = 0.0                                           # an all-black framebuffer, in = NULL
        out = rt.display_frame(flags=A, exposure=2.0)
        assert not rt.display_histogram().any() and rt.last_exposure() == 2.0 and not out[..., :3].any() and (out[..., 3] == 255).all()
        rt.display_frame(frame, flags=A, adapt=0.5)             # ... and E' = 1 is what the next call adapts from
        target = D.target_of(D.histogram(frame))
        assert _f32_bits(rt.last_exposure()) == _f32_bits(np.float32(1) + np.float32(0.5) * (target - np.float32(1)))
    finally:
        rt.cleanupRenderer()


# ---- 4. adaptation -----------------------------------------------------------------------------------------------------

def test_adaptation_and_what_restarts_it(rt):
    """Four AUTO_EXPOSURE calls with adapt = 0.25 on frames of different brightness follow the reference's E bit for bit, a call without the flag in between
    does not disturb them; rtResetDisplay, setRenderOptions and a second init restart the adaptation: the next E is the target itself."""
    nx, ny = 50, 37
    frames = [np.ascontiguousarray(D.synthetic(7, nx, ny, scale)) for scale in (1.0, 16.0, 0.01, 300.0)]
    targets = [D.target_of(D.histogram(f)) for f in frames]
    assert len({float(t) for t in targets}) == 4
    _spheres(rt, nx, ny)
    try:
        ref = D.Display()
        _check(rt, ref, frames[0], frames[0], A, D.NONE, adapt=0.25, what="adapt 0")
        assert _f32_bits(rt.last_exposure()) == _f32_bits(targets[0])
        _check(rt, ref, frames[1], frames[1], A, D.REINHARD, adapt=0.25, what="adapt 1")
        _check(rt, ref, frames[2], frames[2], D.DITHER, D.ACES, exposure=3.0, adapt=0.25, what="no auto exposure in between")
        assert rt.last_exposure() == 3.0
        hist = rt.display_histogram()
        assert np.array_equal(hist, D.histogram(frames[1]))     # still the last AUTO_EXPOSURE call's
        _check(rt, ref, frames[2], frames[2], A, D.ACES, exposure=0.5, adapt=0.25, what="adapt 2")
        _check(rt, ref, frames[3], frames[3], A | D.TOP_DOWN, D.NONE, adapt=0.25, what="adapt 3")
        assert _f32_bits(rt.last_exposure()) not in [_f32_bits(t) for t in targets]       # a blend, not a target
        rt.reset_display()
        assert not rt.display_histogram().any()
        ref.reset()
        _check(rt, ref, frames[1], frames[1], A, D.NONE, adapt=0.25, what="after rtResetDisplay")
        assert _f32_bits(rt.last_exposure()) == _f32_bits(targets[1])
        _check(rt, ref, frames[2], frames[2], A, D.NONE, adapt=0.25, what="after rtResetDisplay, second")
        rt.setRenderOptions(rt.getDefaultRenderOptions(True))
        ref.reset()
        _check(rt, ref, frames[3], frames[3], A, D.NONE, adapt=0.25, what="after setRenderOptions")
        assert _f32_bits(rt.last_exposure()) == _f32_bits(targets[3])
        _spheres(rt, nx, ny)                                    # a second init without cleanupRenderer
        assert rt.last_exposure() == 1.0 and rt.last_display_ms() == 0.0
        ref.reset()
        _check(rt, ref, frames[0], frames[0], A, D.NONE, adapt=0.25, what="after a second init")
        assert _f32_bits(rt.last_exposure()) == _f32_bits(targets[0])
    finally:
        rt.cleanupRenderer()


# ---- 5. the output of previewFrame, where it lies ------------------------------------------------------------------------

def test_from_preview(rt, O):
    """Two previewFrame calls, then displayFrame(NULL, RT_DISPLAY_FROM_PREVIEW): the bytes of displayFrame on the host copy the second previewFrame returned,
    and the reference's on it; previewFrame's own state is not touched."""
    fb, o, mesh = _init(rt, O, "three_spheres")
    try:
        rt.runRenderer(1)
        rt.previewFrame()
        rt.runRenderer(2)
        shown = rt.previewFrame()
        assert rt.preview_frames() == 2
        ref = D.Display()
        for tonemap, flags in ((D.NONE, 0), (D.ACES, ALL), (D.REINHARD, D.TOP_DOWN), (D.NONE, A)):
            rt.reset_display()
            ref.reset()
            got = rt.display_frame(flags=flags | D.FROM_PREVIEW, tonemap=tonemap, exposure=1.3)
            E = rt.last_exposure()
            rt.reset_display()
            again = _check(rt, ref, shown, shown, flags, tonemap, exposure=1.3, what="from preview")
            assert np.array_equal(got, again) and _f32_bits(E) == _f32_bits(rt.last_exposure())
        assert rt.preview_frames() == 2
    finally:
        rt.cleanupRenderer()


# ---- 6. no side effects ------------------------------------------------------------------------------------------------

def test_no_side_effects(rt, O):
    """Framebuffer bits, stats, launches, rtProgressiveSamples, rtHistoryFrames, rtPreviewFrames and the other rtLast*Ms are the same across displayFrame calls,
    and the next previewFrame returns what it returns in a run without them."""
    def run(display):
        fb, o, mesh = _init(rt, O, "three_spheres")
        try:
            rt.runRendererProgressive(2)
            rt.renderGuides()
            rt.runRenderer(1)
            noisy = np.array(fb, copy=True)
            rt.denoiseFrame()
            rt.accumulateFrame()
            first = rt.previewFrame()
            before = (np.array(fb, copy=True), _stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.progressive_samples(), rt.history_frames(),
                      rt.preview_frames(), rt.last_guides_ms(), rt.last_denoise_ms(), rt.last_accumulate_ms(), rt.last_preview_ms())
            if display:
                rt.display_frame()
                rt.display_frame(noisy, flags=ALL, tonemap=D.ACES, exposure=2.0, adapt=0.5)
                rt.display_frame(flags=D.FROM_PREVIEW | A, tonemap=D.REINHARD)
                rt.reset_display()
                after = (np.array(fb, copy=True), _stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.progressive_samples(), rt.history_frames(),
                         rt.preview_frames(), rt.last_guides_ms(), rt.last_denoise_ms(), rt.last_accumulate_ms(), rt.last_preview_ms())
                assert np.array_equal(_bits(before[0]), _bits(after[0])) and before[1:] == after[1:]
                assert before[2] and before[3] == 2 and before[4] == 1 and before[5] == 1 and min(before[6:]) > 0.0
            second, hist, var = rt.previewFrame(history=True, variance=True)
            rt.runRendererProgressive(2)
            return first, second, hist, var, np.array(fb, copy=True), rt.progressive_samples()
        finally:
            rt.cleanupRenderer()
    plain, shown = run(False), run(True)
    for a, b in zip(plain[:5], shown[:5]):
        assert np.array_equal(_bits(a), _bits(b))
    assert plain[5] == shown[5] == 4


# ---- 7. partitions -----------------------------------------------------------------------------------------------------

def test_partitions(rt, O):
    """Stripes of 8 rows (the smallest the library accepts: setRenderOptions refuses a stripe_rows that is no multiple of 8) over part_world 2 and 3: the call
    still works on the whole image - an explicit frame gives the whole-image bytes, and in = NULL shows the framebuffer as it is (this rank's stripes
    rendered, the rest as they were)."""
    fb, o, mesh = _init(rt, O, "three_spheres")
    try:
        rt.runRenderer(1)
        frame = np.array(fb, copy=True)
        whole = rt.display_frame(frame, flags=ALL, tonemap=D.ACES)
        hist, E = rt.display_histogram(), rt.last_exposure()
        for rank, world in ((0, 2), (1, 2), (2, 3)):
            rt.setRenderOptions(o, stripe_rows=8, part_rank=rank, part_world=world)      # (resets the adaptation, as every setRenderOptions)
            assert np.array_equal(rt.display_frame(frame, flags=ALL, tonemap=D.ACES), whole)
            assert np.array_equal(rt.display_histogram(), hist) and _f32_bits(rt.last_exposure()) == _f32_bits(E)
            fb[...] = 0.125
            rt.runRenderer(1)
            mine = np.array(fb, copy=True)
            rows = (np.arange(fb.shape[0]) // 8) % world == rank
            assert np.array_equal(_bits(mine[rows]), _bits(frame[rows])) and (mine[~rows] == 0.125).all()
            ref = D.Display()
            rt.reset_display()
            _check(rt, ref, mine, None, ALL, D.REINHARD, what=f"rank {rank} of {world}")
    finally:
        rt.cleanupRenderer()


# ---- 8. misuse ---------------------------------------------------------------------------------------------------------

_SPHERES = ("sp, mt, cam = rt.scene_three_spheres(16, 12); rt.initRendererSpheres(sp, mt, cam, 16, 12, 10)\n"
            "a = np.zeros((12, 16, 3), np.float32); o = np.zeros((12, 16, 4), np.uint8); call = rt.load_renderer().displayFrame; p = a.ctypes.data; q = o.ctypes.data\n")
_ARGS = dict(flags=0, tonemap=0, exposure=1.0, adapt=1.0)


def _bad(**kw):
    return _SPHERES + "call(p, q, %s)\n" % ", ".join(str(v) for v in dict(_ARGS, **kw).values())


_NAN, _INF = "float('nan')", "float('inf')"
_MISUSE = {
    "out_null": _SPHERES + "call(p, None, 0, 0, 1.0, 1.0)\n",
    "unknown_flag": _bad(flags=16), "unknown_flag_high": _bad(flags=1 << 20),
    "tonemap_3": _bad(tonemap=3), "tonemap_negative": _bad(tonemap=-1),
    "exposure_zero": _bad(exposure=0.0), "exposure_negative": _bad(exposure=-1.0), "exposure_nan": _bad(exposure=_NAN), "exposure_inf": _bad(exposure=_INF),
    "adapt_zero": _bad(adapt=0.0), "adapt_negative": _bad(adapt=-0.5), "adapt_above_1": _bad(adapt=1.5), "adapt_nan": _bad(adapt=_NAN), "adapt_inf": _bad(adapt=_INF),
    "from_preview_with_in": _SPHERES + "rt.runRenderer(1); rt.previewFrame(); call(p, q, 8, 0, 1.0, 1.0)\n",
    "from_preview_before_previewFrame": _SPHERES + "rt.runRenderer(1); call(None, q, 8, 0, 1.0, 1.0)\n",
    "from_preview_after_reset": _SPHERES + "rt.runRenderer(1); rt.previewFrame(); rt.reset_preview(); call(None, q, 8, 0, 1.0, 1.0)\n",
    "after_cleanup": _SPHERES + "rt.cleanupRenderer(); call(p, q, 0, 0, 1.0, 1.0)\n",
    "last_exposure_after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.last_exposure()\n",
    "histogram_after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.display_histogram()\n",
    "reset_after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.reset_display()\n",
    "ms_after_cleanup": _SPHERES + "rt.cleanupRenderer(); rt.last_display_ms()\n",
}


@pytest.mark.parametrize("case", sorted(_MISUSE))
def test_misuse_exits_99(case):
    """The library's misuse convention, each case in a child process of its own: 'rt error' on stderr and exit status 99 (a clean exit of a host-side check)."""
    exits_99(_MISUSE[case])


def test_valid_edge_parameters_are_accepted(rt):
    """The other side of the misuse list: adapt = 1 and a tiny one, tiny and huge exposures, every flag with FROM_PREVIEW after a previewFrame."""
    fb = _spheres(rt, 16, 12)
    try:
        rt.runRenderer(1)
        rt.previewFrame()
        for kw in (dict(adapt=1.0, flags=A), dict(adapt=1e-6, flags=A), dict(exposure=1e-30), dict(exposure=1e30), dict(flags=D.FROM_PREVIEW | ALL, tonemap=D.ACES)):
            out = rt.display_frame(**kw)
            assert out.shape == (12, 16, 4) and (out[..., 3] == 255).all()
        assert not rt.display_frame(exposure=1e-30)[..., :3].any()
        buf = np.zeros((12, 16, 4), np.uint8)
        assert rt.display_frame(out=buf) is buf and buf[..., :3].any()
        assert rt.last_display_ms() > 0.0
    finally:
        rt.cleanupRenderer()
