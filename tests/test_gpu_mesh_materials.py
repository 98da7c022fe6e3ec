"""GPU: path-traced mesh frames with every material kind of include/rt_types.h against the CPU oracle (frames and oracle renders:
tests/mesh_materials_support.py; what they cover and why the bounds are the reference's own: tests/test_mesh_materials_api.py).  One preset material sends
a mesh frame to the general instantiations; these tests run material_scatter's presets ALONG A PATH in all four mesh kernels - k_render_mesh_queue
(thresholded and classic traversal, counting and production instantiations, one and two dispatches, a progressive continuation), k_render_mesh<1> and
k_pixels_mesh - with next-event estimation after a preset bounce, the light and the sky behind glossy and dielectric presets, the `inside` flag, the
path-length argument of the absorbing presets, the checker's hit point, a texture as a metal's tint, and mesh ids 128..255 beside non-zero padding.

The exact frames (kinds whose arithmetic is IEEE fp32 on both sides) are held to the oracle's bits and counters.  The loose frames add the checker,
tinted-glass and subsurface presets (sinf / logf / expf: the device's libm may differ from the host's by an ulp): the device must agree with itself bit
for bit across its kernels, give the oracle's bits on every pixel no such preset had a part in, and stay within 1e-5 * max(|ref|, 1e-3) on 99.5 % of
all channels.

The 18 STATS counters live in the queue kernel alone ("live in this kernel"): the tile kernel (variant 1) carries rays, shadow rays, node
visits and triangle tests, and is held to those four."""
import numpy as np
import pytest

import mesh_materials_support as M
from mesh_materials_support import bits

pytestmark = pytest.mark.gpu
SPP = 4
VARIANTS = (0, 1 << 24, 1)      # persistent queue kernel, its classic while-while traversal, tile per wave


def _same(got, ref, what):
    assert not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    diff = (bits(got) != bits(ref)).any(axis=-1)
    assert not diff.any(), (what, f"{int(diff.sum())} of {diff.size} pixels differ", np.argwhere(diff)[:5].tolist())


def _frame(rt, O, name, ns, mats=None, **opts):
    """One runRenderer of the frame: (framebuffer copy, stats, launches)."""
    fb = M.init(rt, O, name, mats, **opts)
    try:
        rt.runRenderer(ns, 8, 8)
        return np.array(fb, copy=True), rt.getRenderStats(), rt.last_launches()
    finally:
        rt.cleanupRenderer()


def _counting_cases():
    for variant in VARIANTS:
        for nee in (1, 0):
            yield "stair_exact", variant, nee, 0
        for floor in (1, 0):
            if not (floor and variant == 1):            # the host refuses the floor in the tile kernel
                yield "soup_exact", variant, 1, floor


# ---- exact frames ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant,nee,floor", list(_counting_cases()))
def test_counting_launches_bit_exact(rt, O, name, variant, nee, floor):
    """counters = 1: the frame's bits, rays, shadow rays, node visits, triangle tests - and, in the queue kernel, all 18 STATS counters."""
    ref, cnt = M.oracle_frame(rt, O, name, SPP, nee, floor)
    got, st, _ = _frame(rt, O, name, SPP, **M.device_options(name, nee, floor, counters=1, variant=variant))
    _same(got, ref, (name, variant, nee, floor))
    assert (st.rays, st.shadow_rays, st.node_visits, st.prim_tests) == (cnt.rays, cnt.shadow_rays, cnt.node_visits, cnt.prim_tests)
    assert (st.shadow_rays > 0) == bool(nee)
    if variant != 1:
        assert list(st.ref_stats) == list(cnt.ref_stats), list(zip(rt.RT_STAT_NAMES, st.ref_stats, cnt.ref_stats))


@pytest.mark.parametrize("name,floor", [("stair_exact", 0), ("soup_exact", 1), ("soup_exact", 0)])
def test_production_launches_bit_exact(rt, O, name, floor):
    """16 spp with counters off: two dispatches of the general (non-lean) instantiation; the oracle's frame, and again in a second frame into the same
    buffers."""
    ref, _ = M.oracle_frame(rt, O, name, 16, 1, floor)
    fb = M.init(rt, O, name, **M.device_options(name, 1, floor))
    try:
        rt.runRenderer(16, 8, 8)
        launches = rt.last_launches()
        first = np.array(fb, copy=True)
        rt.runRenderer(16, 8, 8)
        second = np.array(fb, copy=True)
    finally:
        rt.cleanupRenderer()
    assert [l["phase"] for l in launches] == [1, 2] and all(l["lean"] == 0 for l in launches), launches
    _same(first, ref, (name, floor, "first frame"))
    _same(second, ref, (name, floor, "second frame"))


@pytest.mark.parametrize("name", M.EXACT_FRAMES)
def test_progressive_passes_bit_exact(rt, O, name):
    """Passes of 2, 6 and 8 samples: the oracle at 8 and at 16."""
    fb = M.init(rt, O, name, **M.device_options(name))
    try:
        rt.runRendererProgressive(2)
        rt.runRendererProgressive(6)
        at8 = np.array(fb, copy=True)
        rt.runRendererProgressive(8)
        at16 = np.array(fb, copy=True)
        assert rt.progressive_samples() == 16
    finally:
        rt.cleanupRenderer()
    _same(at8, M.oracle_frame(rt, O, name, 8)[0], (name, 8))
    _same(at16, M.oracle_frame(rt, O, name, 16)[0], (name, 16))


@pytest.mark.parametrize("name", M.EXACT_FRAMES)
def test_render_pixels_bit_exact(rt, O, name):
    """The whole image as a shuffled pixel list with duplicates: the frame of the same process, the oracle's frame, the oracle's ray total."""
    ij, first = M.pixel_list(rt, O, name)
    ref, cnt = M.oracle_frame(rt, O, name, SPP)
    fb = M.init(rt, O, name, **M.device_options(name, counters=1))
    try:
        rt.runRenderer(SPP, 8, 8)
        frame = np.array(fb, copy=True)
        frame_rays = int(rt.getRenderStats().rays)
        out, _, rays = rt.render_pixels(ij, SPP, rays=True)
    finally:
        rt.cleanupRenderer()
    _same(out, frame[ij[:, 1], ij[:, 0]], (name, "the list against the frame of the same process"))
    _same(out, ref[ij[:, 1], ij[:, 0]], (name, "the list against the oracle"))
    assert int(rays[first].sum(dtype=np.uint64)) == frame_rays == int(cnt.rays)


def test_update_materials_against_the_oracle(rt, O):
    """Plain staircase table (lean kernel) -> the stair_exact table (general) -> back: each frame is the ORACLE's of that table, not only a fresh init's."""
    name = "stair_exact"
    plain, own = M.plain_stair_table(rt), M.frame(rt, O, name)["mats"]
    got, lean = [], []
    fb = M.init(rt, O, name, plain)
    try:
        for table in (None, own, plain):
            if table is not None:
                rt.update_materials(table)
            rt.runRenderer(SPP, 8, 8)
            got.append(np.array(fb, copy=True))
            lean.append(sorted({l["lean"] for l in rt.last_launches()}))
    finally:
        rt.cleanupRenderer()
    assert lean == [[1], [0], [1]], lean
    for frame, table, what in zip(got, ("plain", "own", "plain"), ("init with the plain table", "updated to the preset table", "updated back")):
        _same(frame, M.oracle_frame(rt, O, name, SPP, table=table)[0], what)
    assert not np.array_equal(bits(got[0]), bits(got[1]))


# ---- loose frames ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", M.LOOSE_FRAMES)
def test_loose_frames_device_agrees_with_itself(rt, O, name):
    """Four kernel texts, one device libm: the queue kernel (counting and production instantiations, classic traversal), the tile kernel, the pixel
    kernel and a progressive 1 + 3 split give the same bits - and the same ray and shadow-ray counts where they count."""
    opts = M.device_options(name)
    base, st0, _ = _frame(rt, O, name, SPP, **dict(opts, counters=1))
    assert not np.isnan(base).any()
    production, _, launches = _frame(rt, O, name, SPP, **opts)
    assert all(l["lean"] == 0 for l in launches), launches
    _same(production, base, (name, "production instantiation"))
    classic, st1, _ = _frame(rt, O, name, SPP, **dict(opts, counters=1, variant=1 << 24))
    _same(classic, base, (name, "classic traversal"))
    assert (st1.rays, st1.shadow_rays) == (st0.rays, st0.shadow_rays)
    # the tile kernel has no floor: the soup without it, queue kernel against tile kernel
    if M.is_soup(name):
        no_floor = M.device_options(name, floor=0)
        q, sq, _ = _frame(rt, O, name, SPP, **dict(no_floor, counters=1))
        t, stt, _ = _frame(rt, O, name, SPP, **dict(no_floor, counters=1, variant=1))
        assert (bits(q) != bits(base)).any()
        _same(t, q, (name, "tile kernel, no floor"))
        assert (stt.rays, stt.shadow_rays) == (sq.rays, sq.shadow_rays)
    else:
        t, stt, _ = _frame(rt, O, name, SPP, **dict(opts, counters=1, variant=1))
        _same(t, base, (name, "tile kernel"))
        assert (stt.rays, stt.shadow_rays) == (st0.rays, st0.shadow_rays)
    ij, first = M.pixel_list(rt, O, name)
    fb = M.init(rt, O, name, **opts)
    try:
        out, _, rays = rt.render_pixels(ij, SPP, rays=True)
        rt.runRendererProgressive(1)
        rt.runRendererProgressive(3)
        progressive = np.array(fb, copy=True)
    finally:
        rt.cleanupRenderer()
    _same(out, base[ij[:, 1], ij[:, 0]], (name, "pixel kernel"))
    assert int(rays[first].sum(dtype=np.uint64)) == int(st0.rays)
    _same(progressive, base, (name, "progressive 1 + 3"))


@pytest.mark.parametrize("name", M.LOOSE_FRAMES)
def test_loose_frames_against_the_oracle(rt, O, name):
    """Every untouched pixel has the oracle's bits; at least 99.5 % of all channels are within 1e-5 * max(|ref|, 1e-3) of the oracle.  The ray counts are
    printed beside the oracle's, not asserted: an ulp may flip a decision (a checker cell, a subsurface event)."""
    ref, cnt = M.oracle_frame(rt, O, name, SPP)
    got, st, _ = _frame(rt, O, name, SPP, **M.device_options(name, counters=1))
    assert not np.isnan(got).any()
    u = M.untouched(rt, O, name, SPP)
    ok = M.within_loose_bound(got, ref)
    differ = bits(got) != bits(ref)
    print(f"{name}: untouched pixels {int(u.sum())} of {u.size}, channels within the bound {ok.mean():.5f}, channels that differ in bits {differ.mean():.5f}, "
          f"largest difference {np.abs(got - ref).max():.3g}, rays {st.rays} / {cnt.rays}, shadow rays {st.shadow_rays} / {cnt.shadow_rays}")
    bad = differ.any(axis=2) & u
    assert not bad.any(), (name, "untouched pixels that differ", np.argwhere(bad)[:5].tolist())
    assert ok.mean() >= 0.995, (name, float(ok.mean()))
