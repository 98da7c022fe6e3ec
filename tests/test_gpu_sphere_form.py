"""The folded form of the cost-ordered sphere dispatch (k_render_spheres_queue with FORM = 1, csrc/rt_sphere_form.h): the frame every
production call renders - a queue per XCD, packed parked records, no middle tier, the compact device framebuffer, no diagnostics - runs a kernel compiled
for exactly that, and every switch that leaves it takes the general kernel.  The fold only deletes code, so every frame here must be the CPU oracle's bit
for bit ("bits" = float32 words) and free of NaN (the framebuffer is NaN-poisoned before a frame: a lost pixel would show), and rtLastSphereForm must name
the form that ran.  Random-spheres scene; the view is a close-up of the glass sphere's contact with the ground, chosen with the oracle (checked below) so
that chain list 0 - pixels estimated at 24 rays per sample and more, one pixel to a wave - is not empty in either estimate."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, NY, NS = 96, 64, 16             # six workgroups: two XCDs' queues, chain lists included, are emptied by the other XCDs' waves alone (the leftovers rule)
VIEW = dict(lookfrom=(2.5, 0.4, 1.5), lookat=(0.5, 0.1, 0.5), vfov=20.0, focus=3.0)
LIST0 = 24                          # rays per sample from which a pixel goes to chain list 0 (RtSwitches::top_thr / 16)
GENERAL, DEFAULT = 0, 1
_REFS = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, ref, what=""):
    assert not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    assert np.array_equal(_bits(got), _bits(ref)), (what, int(np.count_nonzero(_bits(got) != _bits(ref))))


def _scene(rt, nx, ny):
    sp, mt, _ = rt.scene_random_spheres(nx, ny)
    cam = rt.make_camera(VIEW["lookfrom"], VIEW["lookat"], (0, 1, 0), VIEW["vfov"], nx / ny, 0.0, VIEW["focus"])
    return sp, mt, cam


def _ref(rt, O, nx, ny, ns):
    """The oracle's frame, computed once per (size, samples) and shared (read-only)."""
    key = (nx, ny, ns)
    if key not in _REFS:
        sp, mt, cam = _scene(rt, nx, ny)
        fb, _ = O.render(O.sphere_scene(sp, mt), cam, O.default_options(True), nx, ny, ns, 50)
        fb.setflags(write=False)
        _REFS[key] = fb
    return _REFS[key]


def _init(rt, nx=NX, ny=NY):
    sp, mt, cam = _scene(rt, nx, ny)
    return rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)


def _report(rt):
    """(phases of the frame's launches, form of its cost-ordered dispatch); that dispatch is the last launch: PHASE 2, CLS 2, the lean one-list kind, no diagnostics."""
    recs = rt.last_launches()
    return [r["phase"] for r in recs], rt.last_sphere_form(), recs[-1]


def _default_frame(rt, O):
    """The 96x64x16 frame in the default form (measured, not reused), rendered once and shared (read-only)."""
    if "default frame" not in _REFS:
        fb = _init(rt)
        rt.runRenderer(NS)
        got, (phases, form, last) = np.array(fb, copy=True), _report(rt)
        rt.cleanupRenderer()
        assert phases == [1, 2] and form == DEFAULT and (last["cls"], last["dbg"], last["lean"]) == (2, 0, 3), (phases, form, last)
        got.setflags(write=False)
        _REFS["default frame"] = got
    return _REFS["default frame"]


def test_the_view_has_pixels_of_chain_list_0(rt, O):
    """The oracle's rays of every pixel (one pixel per call) over the first dispatch's 2 samples and over the frame's 16: both estimates - the measuring
    dispatch's and the cost map's - put at least one pixel on chain list 0."""
    sp, mt, cam = _scene(rt, NX, NY)
    sc, opt = O.sphere_scene(sp, mt), O.default_options(True)
    for ns in (2, NS):
        rays = [O.render(sc, cam, opt, NX, NY, ns, 50, region=(x, y, x + 1, y + 1), counters=True)[1].rays for y in range(NY) for x in range(NX)]
        assert max(rays) >= LIST0 * ns, (ns, max(rays))


def test_two_frames_in_a_row_take_the_folded_form(rt, O):
    """TwoDispatch (the first frame measures), then OrderedSingle (ordered by the first frame's cost map): both in the folded form, both the oracle's frame."""
    ref = _ref(rt, O, NX, NY, NS)
    _same(_default_frame(rt, O), ref, "measured")
    fb = _init(rt)
    rt.runRenderer(NS)
    rt.runRenderer(NS)
    second, (phases, form, last) = np.array(fb, copy=True), _report(rt)
    rt.cleanupRenderer()
    assert phases == [2] and form == DEFAULT and (last["cls"], last["dbg"], last["lean"]) == (2, 0, 3), (phases, form, last)
    _same(second, ref, "ordered by the map")


@pytest.mark.parametrize("nx,ny", [(13, 7), (8, 8)])
def test_one_workgroup(rt, O, nx, ny):
    """One workgroup: seven of the eight XCD queues have no wave of their own, the one workgroup's waves empty them all (13x7: partial tiles)."""
    ns = 8
    ref = _ref(rt, O, nx, ny, ns)
    fb = _init(rt, nx, ny)
    for want in ([1, 2], [2]):
        rt.runRenderer(ns)
        got, (phases, form, last) = np.array(fb, copy=True), _report(rt)
        assert phases == want and form == DEFAULT and last["blocks"] == 1, (phases, form, last)
        _same(got, ref, str(want))
    rt.cleanupRenderer()


def test_progressive_continuation_pass(rt, O):
    """runRendererProgressive 8 + 8: the second pass is the ordering pass and the cost-ordered dispatch alone (TwoDispatchResume), in the folded form; the
    frame is the single call's."""
    fb = _init(rt)
    rt.runRendererProgressive(8)
    first = _report(rt)
    rt.runRendererProgressive(8)
    got, (phases, form, last) = np.array(fb, copy=True), _report(rt)
    rt.cleanupRenderer()
    assert first[1] == DEFAULT, first
    assert phases == [2] and form == DEFAULT and last["cls"] == 2, (phases, form, last)
    _same(got, _default_frame(rt, O), "8 + 8 against the single call")
    _same(got, _ref(rt, O, NX, NY, NS), "8 + 8 against the oracle")


@pytest.mark.parametrize("env,counters", [({"RT_XCD_QUEUES": "0"}, 0), ({"RT_ORD_PACKED": "0"}, 0), ({"RT_FB_DIRECT": "1"}, 0), ({"RT_MID": "2,16"}, 0),
                                          ({"RT_TUNE": "1,2"}, 0), ({"RT_POOL": "8"}, 0), ({}, 1)],
                         ids=["xcd_queues_0", "ord_packed_0", "fb_direct_1", "mid_2_16", "tune", "pool_8", "counters"])
def test_each_switch_that_leaves_the_default_form(rt, O, env, counters, monkeypatch):
    """One switch at a time: the general form runs (both frames: measured, then ordered by the map) and renders the default form's frame.  (RT_MID on this
    six-workgroup grid: the launcher leaves the middle tier out - its lists have no leftovers rule - and still takes the general form.  RT_POOL: a scheduling
    constant that is not the one the folded kernel is compiled with.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = _default_frame(rt, O)
    fb = _init(rt)
    rt.setRenderOptions(rt.getDefaultRenderOptions(True), counters=counters)
    for frame in ("measured", "ordered by the map"):
        rt.runRenderer(NS)
        got, (phases, form, last) = np.array(fb, copy=True), _report(rt)
        assert phases[-1] == 2 and last["cls"] == 2 and form == GENERAL, (frame, phases, form, last)
        _same(got, want, frame)
    rt.cleanupRenderer()               # (an init starts from the default options again)


def test_middle_tier_on_a_grid_that_reaches_every_xcd(rt, O, monkeypatch):
    """128x64: eight workgroups, one on every XCD, so RT_MID keeps its middle waves (general form): the oracle's frame, measured and ordered by the map."""
    monkeypatch.setenv("RT_MID", "2,16")
    nx, ny = 128, 64
    ref = _ref(rt, O, nx, ny, NS)
    fb = _init(rt, nx, ny)
    for frame in ("measured", "ordered by the map"):
        rt.runRenderer(NS)
        got, (phases, form, last) = np.array(fb, copy=True), _report(rt)
        assert last["blocks"] == 8 and form == GENERAL, (frame, phases, form, last)
        _same(got, ref, frame)
    rt.cleanupRenderer()


def test_a_frame_without_a_cost_ordered_dispatch_reports_none(rt):
    fb = _init(rt)
    rt.runRenderer(2)               # below 8 samples: one dispatch in the centre-ray order
    form, phases = rt.last_sphere_form(), [r["phase"] for r in rt.last_launches()]
    rt.cleanupRenderer()
    assert phases == [0] and form == rt.RT_SPHERE_FORM_NONE, (phases, form)
