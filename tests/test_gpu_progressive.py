"""Progressive rendering (runRendererProgressive, include/rt_api.h): a frame built up in passes continues every pixel's RNG stream and running sum, so
after passes of ns_1 .. ns_k samples the PARITY framebuffer holds the bits of runRenderer(ns_1 + .. + ns_k) - and of the CPU oracle at that total.
"Bits" = float32 words compared exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_forms as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, ref, what=""):
    assert not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    assert np.array_equal(_bits(got), _bits(ref)), (what, int(np.count_nonzero(_bits(got) != _bits(ref))))


def _oracle_spheres(O, sp, mt, cam, nx, ny, ns, depth=50, counters=False, region=None):
    return O.render(O.sphere_scene(sp, mt), cam, O.default_options(True), nx, ny, ns, depth, counters=counters, region=region)


def _stripes_of(rank, world, ny, rows=8):
    return np.concatenate([np.arange(k * rows, min((k + 1) * rows, ny)) for k in range((ny + rows - 1) // rows) if k % world == rank])


def test_passes_match_the_oracle_at_every_total(rt, O):
    """Passes of 1, 2, 5, 4 spp (totals 1, 3, 8, 12): after every pass the oracle's bits at the total, no NaN, the sample count; with counters on,
    each pass traces exactly the rays the oracle adds between the previous total and this one (no sample is traced twice)."""
    nx, ny = 200, 120
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    rt.setRenderOptions(rt.getDefaultRenderOptions(True), counters=1)
    assert rt.progressive_samples() == 0
    total, prev_rays = 0, 0
    for ns in (1, 2, 5, 4):
        rt.runRendererProgressive(ns)
        total += ns
        got = np.array(fb, copy=True)
        st = rt.getRenderStats()
        ref, cnt = _oracle_spheres(O, sp, mt, cam, nx, ny, total, counters=True)
        _same(got, ref, total)
        assert rt.progressive_samples() == total
        assert st.samples == nx * ny * ns
        assert st.rays == cnt.rays - prev_rays, (total, st.rays, cnt.rays, prev_rays)
        prev_rays = cnt.rays
    rt.cleanupRenderer()


def test_continuation_of_the_two_dispatch_frame(rt, O):
    """12 + 12 spp on 480x320: the first pass is the two-dispatch frame (PHASE 1, ordering, PHASE 2), the continuation only the ordering pass over
    the accumulated rays and PHASE 2 - no PHASE 1 record.  The bits of runRenderer(24) and of the oracle at 24."""
    nx, ny = 480, 320
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    rt.runRenderer(24)
    mono = np.array(fb, copy=True)
    rt.runRendererProgressive(12)
    assert [r["phase"] for r in rt.last_launches()] == [1, 2]
    rt.runRendererProgressive(12)
    recs = rt.last_launches()
    assert [r["phase"] for r in recs] == [2] and recs[0]["cls"] == 2, recs
    got = np.array(fb, copy=True)
    rt.cleanupRenderer()
    _same(got, mono, "runRenderer(24)")
    _same(got, _oracle_spheres(O, sp, mt, cam, nx, ny, 24)[0], "oracle 24")


def test_interleaving_and_resets(rt, O):
    """runRenderer between passes leaves the progressive frame alone; rtResetProgressive, setRenderOptions and setCamera start it again at sample 0;
    setCamera renders what a fresh init with that camera renders."""
    nx, ny = 160, 96
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    ref = lambda ns, c=cam: _oracle_spheres(O, sp, mt, c, nx, ny, ns)[0]
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    rt.runRendererProgressive(6)
    _same(np.array(fb, copy=True), ref(6), "progressive 6")
    rt.runRenderer(5)
    _same(np.array(fb, copy=True), ref(5), "runRenderer 5")
    assert rt.progressive_samples() == 6
    rt.runRendererProgressive(6)
    _same(np.array(fb, copy=True), ref(12), "progressive 6 + 6")
    rt.resetProgressive()
    assert rt.progressive_samples() == 0
    rt.runRendererProgressive(4)
    _same(np.array(fb, copy=True), ref(4), "after reset")
    rt.runRendererProgressive(4)
    rt.setRenderOptions(rt.getDefaultRenderOptions(True))
    assert rt.progressive_samples() == 0
    rt.runRendererProgressive(4)
    _same(np.array(fb, copy=True), ref(4), "after setRenderOptions")
    cam2 = rt.make_camera((11, 3, 4), (0, 0.5, 0), (0, 1, 0), 25.0, nx / ny, 0.1, 10.0)
    rt.setCamera(cam2)
    assert rt.progressive_samples() == 0
    rt.runRendererProgressive(4)
    moved = np.array(fb, copy=True)
    rt.cleanupRenderer()
    _same(moved, ref(4, cam2), "setCamera")
    fb = rt.initRendererSpheres(sp, mt, cam2, nx, ny, 50)
    rt.runRenderer(4)
    fresh = np.array(fb, copy=True)
    rt.cleanupRenderer()
    _same(moved, fresh, "fresh init with cam2")


@pytest.mark.parametrize("combo", [{}, {"RT_FB_DIRECT": "1"}, {"RT_XCD_QUEUES": "0"}, {"RT_ORD_PACKED": "0"}, {"RT_P1_TILE": "0"}, {"RT_P1_TILE": "1"},
                                   {"RT_FB_DIRECT": "1", "RT_XCD_QUEUES": "0", "RT_ORD_PACKED": "0", "RT_P1_TILE": "1"}])
def test_traffic_switches_across_a_continuation(rt, O, combo, monkeypatch):
    """The traffic forms of the two-dispatch frame (read per frame), alone and all together: 10 + 6 spp equal the oracle at 16.  With direct delivery the
    continuation has no first dispatch to poison the host framebuffer: k_poison_fb does it, and no pixel is left NaN."""
    for k, v in combo.items():
        monkeypatch.setenv(k, v)
    nx, ny = 333, 200
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    rt.runRendererProgressive(10)
    rt.runRendererProgressive(6)
    got = np.array(fb, copy=True)
    rt.cleanupRenderer()
    _same(got, _oracle_spheres(O, sp, mt, cam, nx, ny, 16)[0], combo)


def test_row_partition_and_external_delivery(rt, O):
    """part_world = 3: each rank's stripes after 3 + 9 spp equal the oracle's at 12.  Passes delivered into a setExternalFramebuffer target (set between
    the two passes: that does not reset the frame) give the same bits."""
    nx, ny, world = 200, 120, 3
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    ref = _oracle_spheres(O, sp, mt, cam, nx, ny, 12)[0]
    for r in range(world):
        fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
        rt.setRenderOptions(rt.getDefaultRenderOptions(True), part_rank=r, part_world=world)
        rt.runRendererProgressive(3)
        rt.runRendererProgressive(9)
        rows = _stripes_of(r, world, ny)
        got = np.array(fb, copy=True)[rows]
        rt.cleanupRenderer()
        _same(got, ref[rows], ("rank", r))
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    rt.runRendererProgressive(3)
    ext = np.full((ny, nx, 3), np.nan, np.float32)
    rt.setExternalFramebuffer(ext)
    assert rt.progressive_samples() == 3
    rt.runRendererProgressive(9)
    got = ext.copy()
    rt.setExternalFramebuffer(None)
    rt.cleanupRenderer()
    _same(got, ref, "external framebuffer")


@pytest.mark.parametrize("counters", [0, 1])
def test_mesh_staircase_passes(rt, O, counters):
    """The procedural staircase with NEE + RR, a floor and textures (the general mesh kernel; counters on: the STATS kernel, which has no second
    dispatch): passes of 2, 6, 8 equal the oracle at 16 after the last, and at 8 after the second."""
    nx, ny = 96, 64
    form = dict(name="progressive_mesh", scene=("staircase", True), ns=16)
    _, hm, mats, tex, cam = K.build_scene(rt, form["scene"], nx, ny)
    floor = (0.0, 1.0, 0.0, 0.0, -1.0, 0.0)                             # plane {norm, point} under the staircase
    ks, keep = rt.make_kernel_scene(hm, mats, tex, floor=floor)
    fb = rt.initRenderer(ks, cam, nx, ny, 24, keepalive=keep)
    rt.setRenderOptions(rt.getDefaultRenderOptions(False), floor=1, counters=counters)
    o = O.default_options(False)
    o.floor = 1
    scene = O.mesh_scene(hm, mats, tex, floor=floor)
    rt.runRendererProgressive(2)
    rt.runRendererProgressive(6)
    _same(np.array(fb, copy=True), O.render(scene, cam, o, nx, ny, 8, 24)[0], "mesh 8")
    rt.runRendererProgressive(8)
    got = np.array(fb, copy=True)
    rt.cleanupRenderer()
    _same(got, O.render(scene, cam, o, nx, ny, 16, 24)[0], "mesh 16")


@pytest.mark.parametrize("recipe,scene_word", [(("cloud", 2100, "volume", False), 2), (("cloud", 6000, "volume", False), 1)])
def test_hybrid_and_global_scene_forms(rt, O, recipe, scene_word):
    """The hybrid scene copy and the global scene render in one scattered dispatch (no PHASE 2 for them): the continuation resumes in PHASE 0.
    3 + 5 spp equal runRenderer(8); every pass reports the scene form."""
    nx, ny = K.NX, K.NY
    _, sp, mt, cam = K.build_scene(rt, recipe, nx, ny)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 20)
    rt.runRenderer(8)
    mono = np.array(fb, copy=True)
    for ns in (3, 5):
        rt.runRendererProgressive(ns)
        recs = rt.last_launches()
        assert [(r["phase"], r["scene"]) for r in recs] == [(0, scene_word)], recs
    got = np.array(fb, copy=True)
    rt.cleanupRenderer()
    _same(got, mono, recipe)


def _large_frame(rt, nx, ny):
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    rt.runRenderer(64)
    mono = np.array(fb, copy=True)
    rt.runRendererProgressive(4)
    rt.runRendererProgressive(60)
    lean = rt.last_launches()[0]["lean"]
    got = np.array(fb, copy=True)
    rt.cleanupRenderer()
    return mono, got, lean


def test_large_frame(rt, O):
    """1920x1080 spheres, 4 + 60 spp: the whole frame equals runRenderer(64), an oracle crop matches."""
    nx, ny = 1920, 1080
    mono, got, _ = _large_frame(rt, nx, ny)
    _same(got, mono, "runRenderer(64)")
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    x0, y0, x1, y1 = 900, 500, 964, 532
    ref = _oracle_spheres(O, sp, mt, cam, nx, ny, 64, region=(x0, y0, x1, y1))[0]
    _same(got[y0:y1, x0:x1], ref[y0:y1, x0:x1], "oracle crop")


def test_large_frame_six_wave_kind(rt, O, monkeypatch):
    """The same with the six-wave kind (RT_LEAN6_PIXELS=1)."""
    monkeypatch.setenv("RT_LEAN6_PIXELS", "1")
    mono, got, lean = _large_frame(rt, 1920, 1080)
    assert lean & 4
    _same(got, mono, "six-wave runRenderer(64)")
    sp, mt, cam = rt.scene_random_spheres(1920, 1080)
    x0, y0, x1, y1 = 300, 200, 364, 232
    ref = _oracle_spheres(O, sp, mt, cam, 1920, 1080, 64, region=(x0, y0, x1, y1))[0]
    _same(got[y0:y1, x0:x1], ref[y0:y1, x0:x1], "six-wave oracle crop")


def test_fast_mode_progressive_total(rt, O):
    """FAST fp mode: 1 + 3 spp at 300x200 are held to the tolerance of test_fast_mode_within_tolerance against the oracle at 4."""
    nx, ny = 300, 200
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    rt.setRenderOptions(rt.getDefaultRenderOptions(True), fp=rt.RT_FP_FAST)
    rt.runRendererProgressive(1)
    rt.runRendererProgressive(3)
    got = np.array(fb, copy=True)
    rt.cleanupRenderer()
    ref = _oracle_spheres(O, sp, mt, cam, nx, ny, 4)[0]
    close = np.abs(got - ref) <= 1e-4
    assert close.mean() >= 0.97, close.mean()
    assert np.abs(got - ref).mean() <= 2e-3
    assert rt.rmse(got, ref) <= 0.03


@pytest.mark.parametrize("case", ["counter_rng", "zero_samples", "variant"])
def test_misuse_exits_99(rt, case):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99."""
    opts = {"counter_rng": "rng=rt.RT_RNG_COUNTER", "zero_samples": "counters=0", "variant": "variant=1"}[case]
    ns = 0 if case == "zero_samples" else 2
    code = ("import sys; sys.path.insert(0, %r); import cuda_raytracing_optimized_amd as rt\n"
            "sp, mt, cam = rt.scene_random_spheres(64, 48); rt.initRendererSpheres(sp, mt, cam, 64, 48, 10)\n"
            "rt.setRenderOptions(rt.getDefaultRenderOptions(True), %s); rt.runRendererProgressive(%d)\n") % (ROOT, opts, ns)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 99, (r.returncode, r.stderr[-1000:])
    assert "rt error" in r.stderr
