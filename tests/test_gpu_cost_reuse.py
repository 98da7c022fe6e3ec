"""Sphere frames ordered by the last frame's cost map (RT_COST_REUSE): a runRenderer frame records the rays of every pixel, and the next
frame of the same device state, image, partition, depth, rr, RNG mode and camera runs as the ordering pass and ONE cost-ordered dispatch of whole pixels (launch
record [2], cls 2) instead of measuring first ([1, 2]).  The work order is a hint only: every frame here is compared bit for bit ("bits" = float32 words)
with the CPU oracle of its camera and sample count, and must be free of NaN - the framebuffer is NaN-poisoned before a frame, so a pixel the ordered
dispatch lost would show."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, NY, NS = 96, 64, 10             # six workgroups; a chain pixel on an XCD that has no wave (test_gpu_parity_spheres.py)
_REFS = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, ref, what=""):
    assert not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    assert np.array_equal(_bits(got), _bits(ref)), (what, int(np.count_nonzero(_bits(got) != _bits(ref))))


def _cameras(rt, nx, ny):
    """The scene's own camera, one moved a little, one that sees only sky (it looks straight up from above every sphere)."""
    return {"default": rt.scene_random_spheres(nx, ny)[2],
            "moved": rt.make_camera((12.6, 2.1, 3.5), (0, 0, 0), (0, 1, 0), 20.0, nx / ny, 0.1, 10.0),
            "sky": rt.make_camera((13, 2.5, 3), (13, 100, 3), (1, 0, 0), 20.0, nx / ny, 0.1, 10.0)}


def _ref(rt, O, nx, ny, ns, cam="default", rr=0):
    """The oracle's frame and counters, computed once per (size, samples, camera, rr) and shared (read-only)."""
    key = (nx, ny, ns, cam, rr)
    if key not in _REFS:
        sp, mt, _ = rt.scene_random_spheres(nx, ny)
        o = O.default_options(True)
        o.rr = rr
        fb, cnt = O.render(O.sphere_scene(sp, mt), _cameras(rt, nx, ny)[cam], o, nx, ny, ns, 50, counters=True)
        fb.setflags(write=False)
        _REFS[key] = (fb, cnt)
    return _REFS[key]


def _init(rt, nx=NX, ny=NY):
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    return rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)


def _phases(rt):
    return [r["phase"] for r in rt.last_launches()]


def _assert_reused(rt):
    recs = rt.last_launches()
    assert [r["phase"] for r in recs] == [2] and recs[0]["cls"] == 2, recs


@pytest.mark.parametrize("counters", [1, 0])
@pytest.mark.parametrize("nx,ny,ns", [(96, 64, 10), (61, 37, 9)])
def test_small_grids(rt, O, nx, ny, ns, counters):
    """96x64 (six workgroups) and 61x37 (three, partial tiles): the first frame measures, the second is ordered by the map; both are the oracle's frame.
    counters=1 (the diagnostic instantiation): the reused frame traces exactly the oracle's rays; counters=0: the lean production kind."""
    ref, cnt = _ref(rt, O, nx, ny, ns)
    fb = _init(rt, nx, ny)
    rt.setRenderOptions(rt.getDefaultRenderOptions(True), counters=counters)
    rt.runRenderer(ns)
    first, p1 = np.array(fb, copy=True), _phases(rt)
    rt.runRenderer(ns)
    second, recs, st = np.array(fb, copy=True), rt.last_launches(), rt.getRenderStats()
    rt.cleanupRenderer()
    assert p1 == [1, 2], p1
    assert [r["phase"] for r in recs] == [2] and recs[0]["cls"] == 2 and recs[0]["dbg"] == counters, recs
    _same(first, ref, "measured")
    _same(second, ref, "reused")
    if counters:
        assert st.rays == cnt.rays, (st.rays, cnt.rays)
    assert st.samples == nx * ny * ns


def test_moved_camera_keeping_the_map(rt, O, monkeypatch):
    """RT_COST_REUSE=2: setCamera keeps the map - a slightly moved camera, a camera that sees only sky, and back to the scene.  Coming back the map says one
    ray per sample everywhere: every pixel lands in the last cost list, the chain lists are empty and the chain waves turn to the general queue at once.
    A map that is wrong costs time, never a pixel: every reused frame is the oracle's frame for its camera."""
    monkeypatch.setenv("RT_COST_REUSE", "2")
    cams = _cameras(rt, NX, NY)
    fb = _init(rt)
    rt.runRenderer(NS)
    assert _phases(rt) == [1, 2]
    _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, NS)[0], "default, measured")
    for name in ("moved", "sky", "default"):
        rt.setCamera(cams[name])
        rt.runRenderer(NS)
        _assert_reused(rt)
        _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, NS, name)[0], name)
    rt.cleanupRenderer()


def test_moved_camera_measures_again(rt, O):
    """The default: a setCamera that changes the camera drops the map (a frame ordered by the old view's map is slower than a measured one: DESIGN.md 3.15) -
    the next frame measures, the one after it reuses; setCamera with the camera already set changes nothing."""
    cams = _cameras(rt, NX, NY)
    fb = _init(rt)
    rt.runRenderer(NS)
    assert _phases(rt) == [1, 2]
    for name in ("moved", "sky", "default"):
        rt.setCamera(cams[name])
        rt.runRenderer(NS)
        assert _phases(rt) == [1, 2], name
        _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, NS, name)[0], (name, "measured"))
        rt.setCamera(cams[name])
        rt.runRenderer(NS)
        _assert_reused(rt)
        _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, NS, name)[0], (name, "reused"))
    rt.cleanupRenderer()


def test_changing_ns(rt, O):
    """ns = 1, 10, 9, 30 in a row: the ordering pass divides the map by the samples of the frame that recorded it (10, then 9).  The 1-spp frame is a single
    dispatch ordered by the centre-ray pre-pass (below 8 spp nothing is measured or reused) and records, but a map of one sample says less than the first
    dispatch's two: the frame behind it measures.  Then 2, 10: a 2-spp map is reused."""
    fb = _init(rt)
    for ns, phases in ((1, [0]), (10, [1, 2]), (9, [2]), (30, [2]), (2, [0]), (10, [2])):
        rt.runRenderer(ns)
        assert _phases(rt) == phases, (ns, _phases(rt))
        _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, ns)[0], ns)
    rt.cleanupRenderer()


def test_partition(rt, O):
    """200x120 at 8 spp, 3-way row partition.  Alternating ranks never reuse (another partition member is another device state: its rows are other rows);
    the same rank twice - options set again with equal values in between - reuses.  Every member's rows are the oracle's."""
    nx, ny, ns, world = 200, 120, 8, 3
    ref = _ref(rt, O, nx, ny, ns)[0]
    rows_of = lambda r: np.concatenate([np.arange(k * 8, min((k + 1) * 8, ny)) for k in range((ny + 7) // 8) if k % world == r])
    fb = _init(rt, nx, ny)
    o = rt.getDefaultRenderOptions(True)
    for r in (0, 1, 0, 2, 1):
        rt.setRenderOptions(o, part_rank=r, part_world=world)
        rt.runRenderer(ns)
        assert _phases(rt) == [1, 2], r
        _same(np.array(fb, copy=True)[rows_of(r)], ref[rows_of(r)], ("alternating", r))
    for r in range(world):
        for frame in range(2):
            rt.setRenderOptions(o, part_rank=r, part_world=world)
            fb[:] = 0
            rt.runRenderer(ns)
            if frame == 0:
                assert _phases(rt) == [1, 2], r
            else:
                _assert_reused(rt)
            _same(np.array(fb, copy=True)[rows_of(r)], ref[rows_of(r)], ("twice", r, frame))
    rt.cleanupRenderer()


@pytest.mark.parametrize("combo", [{"RT_FB_DIRECT": "1"}, {"RT_XCD_QUEUES": "0"}, {"RT_ORD_PACKED": "0"},
                                   {"RT_FB_DIRECT": "1", "RT_XCD_QUEUES": "0", "RT_ORD_PACKED": "0"}, "external"])
def test_traffic_forms_on_the_reused_frame(rt, O, combo, monkeypatch):
    """The first frame measures under the default switches; the second is ordered by the map under another traffic form (the switches are read per
    frame): direct delivery (no first dispatch poisons the host framebuffer: k_poison_fb does), one queue for the machine, the parked state in three
    arrays (allocated by this frame, the records freed), all three, and an external framebuffer set between the frames.  A third frame goes back to the
    defaults."""
    ref = _ref(rt, O, NX, NY, NS)[0]
    fb = _init(rt)
    rt.runRenderer(NS)
    assert _phases(rt) == [1, 2]
    _same(np.array(fb, copy=True), ref, "default form")
    ext = None
    if combo == "external":
        ext = np.full((NY, NX, 3), np.nan, np.float32)
        rt.setExternalFramebuffer(ext)
    else:
        for k, v in combo.items():
            monkeypatch.setenv(k, v)
    rt.runRenderer(NS)
    _assert_reused(rt)
    _same(ext.copy() if ext is not None else np.array(fb, copy=True), ref, combo)
    if ext is not None:
        rt.setExternalFramebuffer(None)
    else:
        for k in combo:
            monkeypatch.delenv(k)
    rt.runRenderer(NS)
    _assert_reused(rt)
    _same(np.array(fb, copy=True), ref, ("back to the defaults", combo))
    rt.cleanupRenderer()


def test_off_switch(rt, O, monkeypatch):
    """RT_COST_REUSE=0: every frame measures."""
    monkeypatch.setenv("RT_COST_REUSE", "0")
    ref = _ref(rt, O, NX, NY, NS)[0]
    fb = _init(rt)
    for frame in range(2):
        rt.runRenderer(NS)
        assert _phases(rt) == [1, 2], frame
        _same(np.array(fb, copy=True), ref, frame)
    rt.cleanupRenderer()


def test_invalidation(rt, O):
    """A changed rr measures again (and the frame after it reuses); so does a new init."""
    fb = _init(rt)
    o = rt.getDefaultRenderOptions(True)
    rt.runRenderer(NS)
    assert _phases(rt) == [1, 2]
    rt.setRenderOptions(o, rr=1)
    rt.runRenderer(NS)
    assert _phases(rt) == [1, 2]
    _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, NS, rr=1)[0], "rr = 1, measured")
    rt.setRenderOptions(o, rr=1)
    rt.runRenderer(NS)
    _assert_reused(rt)
    _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, NS, rr=1)[0], "rr = 1, reused")
    rt.cleanupRenderer()
    fb = _init(rt)
    rt.runRenderer(NS)
    assert _phases(rt) == [1, 2]
    _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, NS)[0], "new init")
    rt.cleanupRenderer()


def test_interleaved_progressive_passes(rt, O):
    """Progressive passes neither use nor record the map: runRenderer(10) measures, the first pass of 12 is the two-dispatch frame, its continuation the
    ordering pass over the accumulated rays and PHASE 2, and the runRenderer(10) behind them is ordered by the first frame's map."""
    fb = _init(rt)
    rt.runRenderer(10)
    assert _phases(rt) == [1, 2]
    _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, 10)[0], "runRenderer 10")
    rt.runRendererProgressive(12)
    assert _phases(rt) == [1, 2]
    _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, 12)[0], "progressive 12")
    rt.runRendererProgressive(12)
    _assert_reused(rt)
    _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, 24)[0], "progressive 12 + 12")
    rt.runRenderer(10)
    _assert_reused(rt)
    _same(np.array(fb, copy=True), _ref(rt, O, NX, NY, 10)[0], "runRenderer 10 again")
    rt.cleanupRenderer()


def test_headline_frame(rt):
    """The benchmark's frame (1200x800, 100 spp) once: frame 1 measures, frame 2 is ordered by its map, and the two framebuffers are equal word for word."""
    nx, ny, ns = 1200, 800, 100
    fb = _init(rt, nx, ny)
    rt.runRenderer(ns)
    first, p1 = np.array(fb, copy=True), _phases(rt)
    rt.runRenderer(ns)
    second = np.array(fb, copy=True)
    _assert_reused(rt)
    rt.cleanupRenderer()
    assert p1 == [1, 2], p1
    _same(second, first, "reused against measured")
