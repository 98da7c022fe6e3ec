"""GPU: the mesh kernels under a moved, resized and coloured light (rt_render_options.light / .lightColor), against the CPU oracle's frame for that light.
Lights, frames and oracle renders: tests/mesh_lights_support.py; that each light does what it is named for: tests/test_mesh_lights_api.py.

Every other path-traced frame of the suite uses the default light, which lies outside every test scene and is grey.  Under it a shadow traversal that ran
to FLT_MAX instead of lightDist, a light colour read from one channel, and a wrong "the escaping specular path sees the light" branch all render the
default frame.  Here the light sits inside the scene (occluders behind it), reaches the geometry (cosAMax towards 0, origins inside: NaN and no draws),
lies between the soup's floor and its bounds (the scene-bounds test fails by t_max = lightDist), fills the sky (seen directly with nee = 0), is so small
that cosAMax is exactly 1 (shadow rays counted, contribution exactly 0) - and has the colour (30, 12, 3).

Every comparison is np.array_equal on the 32-bit words; NaN is asserted absent.  The 18 STATS counters live in the queue kernel alone; the tile kernel
(variant 1) carries rays, shadow rays, node visits and triangle tests, and refuses the floor: the soup runs there without it.

The FAST objects carry no bit promise: test_fast_reads_the_light asserts only that the FAST frame under `inside` is nearer (rt.rmse) to the oracle's
`inside` frame than the oracle's default-light frame is."""
import numpy as np
import pytest

import mesh_lights_support as L
import mesh_materials_support as M
import refine_reference as RR
from mesh_materials_support import bits

pytestmark = pytest.mark.gpu
SPP = 4
VARIANTS = (0, 1 << 24, 1)      # persistent queue kernel, its classic while-while traversal, tile per wave
FRAME_LIGHTS = [(f, n) for f in L.FRAMES for n in L.names(f)]


def _same(got, ref, what):
    assert not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    diff = (bits(got) != bits(ref)).any(axis=-1)
    assert not diff.any(), (what, f"{int(diff.sum())} of {diff.size} pixels differ", np.argwhere(diff)[:5].tolist())


def _floor(frame, variant):
    """The soup's floor: on in the queue kernel, off in the tile kernel (the host refuses it there)."""
    return (0 if variant == 1 else 1) if M.is_soup(frame) else 0


# ---- counting launches -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("frame,name", FRAME_LIGHTS)
def test_counting_launches_bit_exact(rt, O, frame, name, variant):
    """counters = 1, nee on and off: the frame's bits, rays, shadow rays, node visits, triangle tests - and, in the queue kernel, all 18 STATS counters."""
    floor = _floor(frame, variant)
    for nee in (1, 0):
        ref, cnt = L.oracle_frame(rt, O, frame, name, SPP, nee, floor)
        fb = L.init(rt, O, frame, name, nee=nee, floor=floor, counters=1, variant=variant)
        try:
            rt.runRenderer(SPP, 8, 8)
            got, st = np.array(fb, copy=True), rt.getRenderStats()
        finally:
            rt.cleanupRenderer()
        _same(got, ref, (frame, name, variant, nee))
        assert (st.rays, st.shadow_rays, st.node_visits, st.prim_tests) == (cnt.rays, cnt.shadow_rays, cnt.node_visits, cnt.prim_tests), (frame, name, variant, nee)
        assert nee or st.shadow_rays == 0               # (nee = 1: soup_exact without its floor has no origin outside `huge`, and no shadow ray)
        if variant != 1:
            assert list(st.ref_stats) == list(cnt.ref_stats), (nee, list(zip(rt.RT_STAT_NAMES, st.ref_stats, cnt.ref_stats)))


# ---- production launches -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["inside", "sky"])
@pytest.mark.parametrize("frame", L.FRAMES)
def test_production_launches_bit_exact(rt, O, frame, name):
    """16 spp with counters off: two dispatches, the general instantiation on the preset tables and the lean one on the plain staircase; the oracle's
    frame, and again in a second frame into the same buffers."""
    ref, _ = L.oracle_frame(rt, O, frame, name, 16)
    fb = L.init(rt, O, frame, name)
    try:
        rt.runRenderer(16, 8, 8)
        launches = rt.last_launches()
        first = np.array(fb, copy=True)
        rt.runRenderer(16, 8, 8)
        second = np.array(fb, copy=True)
    finally:
        rt.cleanupRenderer()
    lean = 1 if frame == "stair_plain" else 0
    assert [l["phase"] for l in launches] == [1, 2] and all(l["lean"] == lean for l in launches), launches
    _same(first, ref, (frame, name, "first frame"))
    _same(second, ref, (frame, name, "second frame"))


# ---- progressive passes and the pixel kernels under `inside` -----------------------------------------------------------------------

@pytest.mark.parametrize("frame", L.FRAMES)
def test_progressive_passes_bit_exact(rt, O, frame):
    """Passes of 2, 6 and 8 samples: the oracle at 8 and at 16."""
    fb = L.init(rt, O, frame, "inside")
    try:
        rt.runRendererProgressive(2)
        rt.runRendererProgressive(6)
        at8 = np.array(fb, copy=True)
        rt.runRendererProgressive(8)
        at16 = np.array(fb, copy=True)
        assert rt.progressive_samples() == 16
    finally:
        rt.cleanupRenderer()
    _same(at8, L.oracle_frame(rt, O, frame, "inside", 8)[0], (frame, 8))
    _same(at16, L.oracle_frame(rt, O, frame, "inside", 16)[0], (frame, 16))


@pytest.mark.parametrize("frame", L.FRAMES)
def test_render_pixels_bit_exact(rt, O, frame):
    """The whole image as a shuffled pixel list with duplicates: the oracle's frame and ray total; 2 samples continued by 2 through `state` equal 4 at once."""
    ij, first = M.pixel_list(rt, O, L.base(frame)[0])
    ref, cnt = L.oracle_frame(rt, O, frame, "inside", SPP)
    L.init(rt, O, frame, "inside")
    try:
        out, state4, rays = rt.render_pixels(ij, SPP, rays=True)
        _, state2, rays2 = rt.render_pixels(ij, 2, rays=True)
        cont, state22, rays22 = rt.render_pixels(ij, 2, first=np.full(len(ij), 2, np.int32), state=state2, rays=True)
    finally:
        rt.cleanupRenderer()
    _same(out, ref[ij[:, 1], ij[:, 0]], (frame, "the list against the oracle"))
    assert int(rays[first].sum(dtype=np.uint64)) == int(cnt.rays)
    _same(cont, out, (frame, "2 + 2 samples through state against 4 at once"))
    assert np.array_equal(state22, state4) and np.array_equal(rays2 + rays22, rays)


# ---- refineFrame -------------------------------------------------------------------------------------------------------------------

def test_refine_to_completion(rt, O):
    """stair_exact under `inside` to completion against tests/refine_reference.py over the oracle's frames, every call (as
    tests/test_gpu_refine.py::test_to_completion_every_call)."""
    from test_gpu_refine import _check_call
    frame, name = "stair_exact", "inside"
    batch, min_batches, max_samples, threshold = RR.CASES["M1"]
    f = M.frame(rt, O, frame)
    model = RR.Frame(rt, O, None, batch, frames=lambda n: L.oracle_frame(rt, O, frame, name, n)[0], shape=(f["ny"], f["nx"]))
    ref = []
    while not ref or ref[-1][0]:
        ref.append(model.call(min_batches, max_samples, threshold, RR.DILATE))
        assert len(ref) < 64
    L.init(rt, O, frame, name)
    try:
        assert rt.refine_samples() == 0
        got, totals = [], []
        for _ in ref:
            got.append(rt.refine_frame(batch, min_batches, max_samples, threshold, RR.DILATE))
            totals.append(rt.refine_samples())
    finally:
        rt.cleanupRenderer()
    print("sampled per call", [g[0] for g in got], "samples at the end", np.unique(got[-1][2], return_counts=True))
    traced = 0
    for k, (g, r) in enumerate(zip(got, ref)):
        _check_call(g, r, f"{frame} {name} call {k + 1}")
        traced += r[0] * batch
        assert totals[k] == traced
    assert got[-1][0] == 0 and len(ref) >= 3 and len(np.unique(got[-1][2])) >= 2         # the selection did select


# ---- the light changes without a new init ------------------------------------------------------------------------------------------

LIGHT_STEPS = [("default", {}), ("inside", {}), ("inside", dict(colour=(3.0, 12.0, 30.0))), ("sky", {}), ("sky", dict(radius=100.0)), ("default", {})]


@pytest.mark.parametrize("frame", ["stair_exact", "stair_plain"])
def test_the_light_changes_without_a_new_init(rt, O, frame):
    """One initRenderer; setRenderOptions with the default light -> inside -> the same light, only lightColor changed -> sky -> only the radius changed ->
    the default light.  After each: runRenderer in the queue kernel, runRenderer in the tile kernel, render_pixels on 200 pixels and one progressive pass
    equal the oracle's frame for the light in force, and the progressive count is 0 after every setRenderOptions."""
    ij = np.ascontiguousarray(M.pixel_list(rt, O, L.base(frame)[0])[0][:200])
    got = []
    fb = L.init(rt, O, frame)
    try:
        for name, kw in LIGHT_STEPS:
            L.set_light(rt, frame, name, **kw)
            after_set = [rt.progressive_samples()]
            rt.runRenderer(SPP, 8, 8)
            queue, lean = np.array(fb, copy=True), sorted({l["lean"] for l in rt.last_launches()})
            pixels = rt.render_pixels(ij, SPP)[0]
            rt.runRendererProgressive(SPP)
            progressive, count = np.array(fb, copy=True), rt.progressive_samples()
            L.set_light(rt, frame, name, variant=1, **kw)
            after_set.append(rt.progressive_samples())
            rt.runRenderer(SPP, 8, 8)
            got.append((queue, pixels, progressive, np.array(fb, copy=True), after_set, count, lean))
    finally:
        rt.cleanupRenderer()
    refs = [L.oracle_frame(rt, O, frame, name, SPP, **kw)[0] for name, kw in LIGHT_STEPS]
    for k, ((name, kw), ref, (queue, pixels, progressive, tile, after_set, count, lean)) in enumerate(zip(LIGHT_STEPS, refs, got)):
        what = (frame, k, name, kw)
        assert after_set == [0, 0] and count == SPP, what
        assert lean == [1 if frame == "stair_plain" else 0], what
        _same(queue, ref, what + ("queue kernel",))
        _same(tile, ref, what + ("tile kernel",))
        _same(pixels, ref[ij[:, 1], ij[:, 0]], what + ("render_pixels",))
        _same(progressive, ref, what + ("progressive pass",))
    for a, b in zip(refs, refs[1:]):
        assert not np.array_equal(bits(a), bits(b))                                      # every step is a different frame
    assert np.array_equal(bits(refs[0]), bits(refs[-1]))


# ---- partition ---------------------------------------------------------------------------------------------------------------------

def test_stripe_partition_is_invisible(rt, O):
    """part_world = 3 rendered in turn and merged equals the whole frame under `inside`."""
    frame = "stair_exact"
    ref, _ = L.oracle_frame(rt, O, frame, "inside", SPP)
    ny = ref.shape[0]
    merged = np.zeros_like(ref)
    fb = L.init(rt, O, frame, "inside")
    try:
        for r in range(3):
            L.set_light(rt, frame, "inside", part_rank=r, part_world=3, stripe_rows=8)
            rt.runRenderer(SPP, 8, 8)
            part = np.array(fb, copy=True)
            for k in range(r, (ny + 7) // 8, 3):
                merged[k * 8:(k + 1) * 8] = part[k * 8:(k + 1) * 8]
    finally:
        rt.cleanupRenderer()
    _same(merged, ref, "three stripe members merged")


def test_two_in_process_devices(rt, O):
    """The same frame over two devices of this process."""
    if rt.device_count() < 2:
        pytest.skip("needs two HIP devices")
    frame = "stair_exact"
    ref, _ = L.oracle_frame(rt, O, frame, "inside", SPP)
    fb = L.init(rt, O, frame, "inside", devices=[0, 1], stripe_rows=8)
    try:
        rt.runRenderer(SPP, 8, 8)
        got = np.array(fb, copy=True)
    finally:
        rt.cleanupRenderer()
    _same(got, ref, "two in-process devices")


# ---- FAST --------------------------------------------------------------------------------------------------------------------------

def test_fast_reads_the_light(rt, O):
    """The RT_FP_FAST frame of stair_exact under `inside` is nearer to the oracle's `inside` frame than the oracle's default-light frame is.  Only the
    ordering: FAST carries no bit promise and no bound is derivable here.  Measured on an MI355X: see DESIGN.md."""
    frame = "stair_exact"
    ref = L.oracle_frame(rt, O, frame, "inside", SPP)[0]
    other = L.oracle_frame(rt, O, frame, L.DEFAULT, SPP)[0]
    fb = L.init(rt, O, frame, "inside", fp=rt.RT_FP_FAST)
    try:
        rt.runRenderer(SPP, 8, 8)
        got = np.array(fb, copy=True)
    finally:
        rt.cleanupRenderer()
    assert not np.isnan(got).any()
    near, far = rt.rmse(got, ref), rt.rmse(other, ref)
    print(f"FAST under inside: rmse to the oracle's inside frame {near:.6g}, the oracle's default-light frame to it {far:.6g}")
    assert near < far
