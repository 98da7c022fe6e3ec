"""updateTriangles / updateMaterials / updateSpheres / getMeshBvh (include/rt_api.h, "editing the scene") on the GPU.  The contract: after any sequence of edits
everything the library computes is bit-identical to cleanupRenderer + init* with the edited scene - for a mesh the edited triangles with rtRefitBvh's nodes and
bounds (HostMesh.refit, the CPU twin) - and so, in PARITY mode, to the CPU oracle on that scene.  Every comparison is np.array_equal on the raw 32-bit words: no
tolerance, nothing left out.  Frames are 40x50 (staircase) and 48x40 (tris300) at 4 spp with 16 bounces.  Every test edits a mesh of its own: the cached
frames of guides_reference are copied (scene_update_support.fresh_copy), never edited."""
import numpy as np
import pytest

import guides_reference as G
import scene_update_support as S
from preview_support import bits, exits_99, same, stats_tuple

pytestmark = pytest.mark.gpu
SPP, DEPTH = 4, 16
ALL_GUIDES = 1 | 2 | 4 | 8 | 16


def _init_mesh(rt, hm, mats, tex, cam, nx, ny, floor=None, **opts):
    ks, keep = rt.make_kernel_scene(hm, mats, tex, floor=floor)
    fb = rt.initRenderer(ks, cam, nx, ny, DEPTH, keepalive=keep)
    o = rt.getDefaultRenderOptions(False)
    if floor is not None:
        opts = dict(opts, floor=1)
    if opts:
        rt.setRenderOptions(o, **opts)
    return fb, o


def _all_pixels(nx, ny):
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny)), -1).reshape(-1, 2).astype(np.int32)


def _counted(st):
    return stats_tuple(st)[2:]                                  # everything but the two timings


def _collect(rt, fb, cam, nx, ny, mesh, o=None):
    """What a scene yields: the frame, every guide plane, every plane of traceRays on the frame's centre rays and, with `o` (mesh scenes), the counters = 1
    statistics with that frame and the RT_FP_FAST frame."""
    out = {}
    rt.runRenderer(SPP)
    out["frame"] = np.array(fb, copy=True)
    for k, v in rt.renderGuides(ALL_GUIDES if mesh else ALL_GUIDES & ~16).items():
        out["guide " + k] = v
    org, d = rt.centre_rays(cam, nx, ny, _all_pixels(nx, ny))
    for k, v in rt.trace_rays(org, d).items():
        out["ray " + k] = v
    out["occluded"] = rt.occluded_rays(org, d).astype(np.uint32)
    if o is not None:
        rt.setRenderOptions(o, counters=1)
        rt.runRenderer(SPP)
        out["counted frame"] = np.array(fb, copy=True)
        out["stats"] = np.array([int(x) for x in _flat(_counted(rt.getRenderStats()))], np.uint64).view(np.uint32)
        rt.setRenderOptions(o, counters=0, fp=rt.RT_FP_FAST)
        rt.runRenderer(SPP)
        out["fast frame"] = np.array(fb, copy=True)
        rt.setRenderOptions(o, fp=rt.RT_FP_PARITY)
    return out


def _flat(t):
    for x in t:
        if isinstance(x, tuple):
            yield from _flat(x)
        else:
            yield x


def _same_all(got, ref, what):
    assert sorted(got) == sorted(ref)
    for k in got:
        same(got[k], ref[k], f"{what}: {k}")


def _nodes_match_twin(rt, hm, what):
    nodes, bounds = rt.mesh_bvh()
    assert len(nodes) == hm.view.numBvhNodes
    same(nodes, hm.bvh, what + ": nodes against the CPU twin")
    same(bounds, S.view_bounds(hm), what + ": bounds against the CPU twin")
    return nodes


def _apply(rt, hm, first, new):
    """The edit on the device and on the host mesh: slots [first, first + len(new)) become `new`, the device refits, the twin refits."""
    rt.update_triangles(first, new)
    hm.tris[first:first + len(new)] = new
    hm.refit()


def _oracle_mesh(rt, O, hm, mats, tex, cam, nx, ny, floor=None):
    opt = O.default_options(False)
    if floor is not None:
        opt.floor = 1
    return O.render(O.mesh_scene(hm, mats, tex, floor), cam, opt, nx, ny, SPP, DEPTH)[0]


# ---- 1. one object moves out of its boxes --------------------------------------------------------------------------------------------------

def test_moved_object(rt, O):
    """Every triangle of the steel ball (mesh id 12, visible from the staircase camera) translated by (25, 10, -30): an upload without a refit leaves the
    ball outside every box that is traversed for it."""
    ball = 12
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    nx, ny = G.STAIR_NX, G.STAIR_NY
    cam = rt.staircase_camera(nx, ny)
    fb, o = _init_mesh(rt, hm, mats, [], cam, nx, ny)
    try:
        prim = rt.renderGuides(rt.RT_GUIDE_PRIM)["prim"]
        assert (hm.tris["meshID"][prim[prim >= 0]] == ball).sum() >= 20, "the ball is not visible"
        before = rt.mesh_bvh()[0]
        same(before, hm.bvh, "before the edit: nodes against the builder's")
        sel = np.flatnonzero(S.is_real(hm.tris) & (hm.tris["meshID"] == ball))
        first, last = int(sel.min()), int(sel.max())
        new = hm.tris[first:last + 1].copy()
        new["v"][sel - first] = new["v"][sel - first] + np.array([25, 10, -30], np.float32)
        _apply(rt, hm, first, new)
        assert rt.last_update_ms() > 0.0
        nodes = _nodes_match_twin(rt, hm, "moved ball")
        assert (bits(nodes) != bits(before)).sum() > 100
        got = _collect(rt, fb, cam, nx, ny, True)
    finally:
        rt.cleanupRenderer()
    same(got["frame"], _oracle_mesh(rt, O, hm, mats, [], cam, nx, ny), "moved ball: frame against the oracle on the edited mesh")
    fb, o = _init_mesh(rt, hm, mats, [], cam, nx, ny)
    try:
        ref = _collect(rt, fb, cam, nx, ny, True)
    finally:
        rt.cleanupRenderer()
    _same_all(got, ref, "moved ball against a fresh init")
    moved = hm.tris["meshID"][ref["guide prim"][ref["guide prim"] >= 0]] == ball
    assert moved.sum() >= 20, "the moved ball is not visible"


# ---- 2. everything moves -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tris300", "tris300_floor"])
def test_everything_moves(rt, O, name, tmp_path):
    f = G.mesh_frame(rt, O, name)
    hm = S.fresh_copy(rt, f["hm"], tmp_path)
    args = (f["mats"], f["tex"], f["cam"], f["nx"], f["ny"], f["floor"])
    fb, o = _init_mesh(rt, hm, *args)
    try:
        _apply(rt, hm, 0, S.jitter(hm.tris, 31))
        _nodes_match_twin(rt, hm, name + " jittered")
        got = _collect(rt, fb, f["cam"], f["nx"], f["ny"], True, o)
    finally:
        rt.cleanupRenderer()
    same(got["frame"], _oracle_mesh(rt, O, hm, *args), name + " jittered: frame against the oracle on the edited mesh")
    fb, o = _init_mesh(rt, hm, *args)
    try:
        ref = _collect(rt, fb, f["cam"], f["nx"], f["ny"], True, o)
    finally:
        rt.cleanupRenderer()
    _same_all(got, ref, name + " jittered against a fresh init")
    assert ref["stats"].view(np.uint64)[4] > 0                  # node visits were counted


# ---- 3. there and back ---------------------------------------------------------------------------------------------------------------------

def test_round_trip(rt, O, tmp_path):
    f = G.mesh_frame(rt, O, "tris300")
    hm = S.fresh_copy(rt, f["hm"], tmp_path)
    original, built = hm.tris.copy(), hm.bvh.copy()
    fb, o = _init_mesh(rt, hm, f["mats"], f["tex"], f["cam"], f["nx"], f["ny"])
    try:
        rt.runRenderer(SPP)
        frame0 = np.array(fb, copy=True)
        _apply(rt, hm, 0, S.jitter(original, 32))
        moved = _nodes_match_twin(rt, hm, "there")
        assert (bits(moved[1:]) != bits(built[1:])).mean() > 0.5
        rt.runRenderer(SPP)
        assert not np.array_equal(bits(fb), bits(frame0))
        _apply(rt, hm, 0, original)
        nodes, bounds = rt.mesh_bvh()
        same(nodes, built, "back: nodes against the builder's original")
        same(bounds, S.view_bounds(f["hm"]), "back: bounds against the builder's original")
        rt.runRenderer(SPP)
        same(fb, frame0, "back: frame against the frame before any edit")
    finally:
        rt.cleanupRenderer()


# ---- 4. ranges -----------------------------------------------------------------------------------------------------------------------------

def test_ranges(rt):
    """512 leaves of 5 slots, two workgroups of the bottom kernel: one slot, the last real slot, a pair across the two subtrees, a run with sentinels in it."""
    nppl = 5
    hm = S.blob_mesh(rt, 512, nppl)
    real = S.is_real(hm.tris)
    last_real = int(np.flatnonzero(real).max())
    cross = 256 * nppl - 1
    run = (100 * nppl, 12 * nppl)
    assert real[0] and real[cross + 1] and real[run[0]:run[0] + run[1]].any() and not real[run[0]:run[0] + run[1]].all()
    cam = rt.make_camera((30, 18, 42), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.1, 50.0)
    mats = np.zeros(4, rt.material_dtype)
    mats["texId"] = -1
    _init_mesh(rt, hm, mats, [], cam, 16, 16)
    try:
        for seed, (first, count) in enumerate(((0, 1), (last_real, 1), (cross, 2), run)):
            new = S.jitter(hm.tris[first:first + count], 40 + seed)
            before = rt.mesh_bvh()[0]
            _apply(rt, hm, first, new)
            nodes = _nodes_match_twin(rt, hm, f"range ({first}, {count})")
            assert not np.array_equal(bits(nodes), bits(before)), (first, count)
    finally:
        rt.cleanupRenderer()


# ---- 5. tree shapes ------------------------------------------------------------------------------------------------------------------------

def _shape_mesh(rt, O, case):
    if case == "tris300 nppl 1, 2^17 leaves":
        f = G.mesh_frame(rt, O, "tris300")
        src = f["hm"].tris
        return rt.HostMesh.build(src[S.is_real(src)], 1, extra_levels=8)
    if case == "sentinel before real":
        return S.sentinel_first_mesh(rt)
    if case == "signed zeros":
        return rt.HostMesh.build(S.zero_tris(rt), 5)
    if case == "extremes":
        return S.blob_mesh(rt, 128, 5)
    first_leaf, nppl = case
    return S.blob_mesh(rt, first_leaf, nppl)


SHAPES = [(2, 1), (4, 1), (4, 7), (128, 5), (256, 1), (256, 7), (512, 5), "tris300 nppl 1, 2^17 leaves", "sentinel before real", "signed zeros", "extremes"]


@pytest.mark.parametrize("case", SHAPES, ids=[str(c) for c in SHAPES])
def test_tree_shapes(rt, O, case):
    """getMeshBvh against the twin, no render: trees lower than one workgroup's subtree, exactly one, two, and three reduction passes (2^17 mostly empty
    leaves); 1, 5 and 7 slots per leaf; a mesh without compact leaf records; boxes whose zeros' signs depend on the visiting order; an edit that brings NaN
    coordinates (ignored by the boxes), coordinates near FLT_MAX and denormal ones."""
    hm = _shape_mesh(rt, O, case)
    if isinstance(case, tuple):
        assert hm.view.numBvhNodes // 2 == case[0] and hm.nppl == case[1]
    if case == "tris300 nppl 1, 2^17 leaves":
        assert hm.view.numBvhNodes // 2 == 1 << 17
    mats = np.zeros(4, rt.material_dtype)
    mats["texId"] = -1
    cam = rt.make_camera((30, 18, 42), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.1, 50.0)
    _init_mesh(rt, hm, mats, [], cam, 8, 8)
    try:
        before = _nodes_match_twin(rt, hm, f"{case}: as built")
        if case == "signed zeros":
            new = hm.tris.copy()
            new["v"] = new["v"][:, ::-1, :]                     # the other vertex order: other zeros are met first
            _apply(rt, hm, 0, new)
            nodes = _nodes_match_twin(rt, hm, f"{case}: vertices reversed")
            assert np.array_equal(nodes["a"][1:], before["a"][1:]) and not np.array_equal(bits(nodes), bits(before))
            new = hm.tris.copy()
            real = S.is_real(new)
            new["v"][real] = -new["v"][real]
            _apply(rt, hm, 0, new)
            _nodes_match_twin(rt, hm, f"{case}: negated")
        elif case == "extremes":                                # NaN, near-FLT_MAX and denormal coordinates (scene_update_support.extremes)
            _apply(rt, hm, 0, S.extremes(hm.tris)[0])
            nodes = _nodes_match_twin(rt, hm, f"{case}: edited")
            want_nodes, want_bounds = S.numpy_refit(hm.tris, hm.bvh, hm.nppl)
            same(hm.bvh, want_nodes, f"{case}: the twin against the numpy restatement")
            same(S.view_bounds(hm), want_bounds, f"{case}: the twin's bounds against the numpy restatement")
            assert not np.array_equal(bits(nodes), bits(before)) and not np.isnan(nodes["a"][1:]).any() and not np.isnan(nodes["b"][1:]).any()
        else:
            _apply(rt, hm, 0, S.jitter(hm.tris, 50))
            nodes = _nodes_match_twin(rt, hm, f"{case}: jittered")
            assert not np.array_equal(bits(nodes), bits(before))
    finally:
        rt.cleanupRenderer()


# ---- 6. a relayout after an edit -----------------------------------------------------------------------------------------------------------

def test_relayout_keeps_the_edit(rt, O, tmp_path):
    """setRenderOptions with another stripe_rows builds new device states from the host mirrors: they must hold the edited scene."""
    f = G.mesh_frame(rt, O, "tris300")
    hm = S.fresh_copy(rt, f["hm"], tmp_path)
    args = (f["mats"], f["tex"], f["cam"], f["nx"], f["ny"])
    fb, o = _init_mesh(rt, hm, *args)
    try:
        _apply(rt, hm, 0, S.jitter(hm.tris, 33))
        rt.setRenderOptions(o, stripe_rows=16)
        _nodes_match_twin(rt, hm, "after the relayout")
        got = _collect(rt, fb, f["cam"], f["nx"], f["ny"], True)
        _apply(rt, hm, 7, S.jitter(hm.tris[7:90], 34))          # and an edit of the new device state
        rt.setRenderOptions(o, stripe_rows=8)
        got2 = _collect(rt, fb, f["cam"], f["nx"], f["ny"], True)
    finally:
        rt.cleanupRenderer()
    hm1 = S.fresh_copy(rt, f["hm"], tmp_path)
    hm1.tris[:] = S.jitter(hm1.tris, 33)
    hm1.refit()
    for mesh, rows, res, what in ((hm1, 16, got, "edit, relayout"), (hm, 8, got2, "edit, relayout, edit, relayout")):
        fb, o = _init_mesh(rt, mesh, *args, stripe_rows=rows)
        try:
            ref = _collect(rt, fb, f["cam"], f["nx"], f["ny"], True)
        finally:
            rt.cleanupRenderer()
        _same_all(res, ref, what + " against a fresh init")


# ---- 7. materials --------------------------------------------------------------------------------------------------------------------------

def test_materials(rt, O):
    """The back wall (13, diffuse) becomes glass - every material still plain, the lean kernel still runs -, then the floor (17) a checker preset, which takes
    the lean kernel away, then everything back."""
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    nx, ny = G.STAIR_NX, G.STAIR_NY
    cam = rt.staircase_camera(nx, ny)
    glass = mats.copy()
    glass["type"][13], glass["param"][13] = rt.RT_GLASS, 1.5
    checker = glass.copy()
    checker["type"][17] = rt.RT_FLOOR_CHECKER
    steps = [("wall to glass", glass), ("floor to checker", checker), ("back to the original", mats)]

    def lean(launches):
        return sorted({l["lean"] for l in launches})

    got, seen = [], []
    fb, o = _init_mesh(rt, hm, mats, [], cam, nx, ny)
    try:
        prim = rt.renderGuides(rt.RT_GUIDE_PRIM)["prim"]
        visible = set(hm.tris["meshID"][prim[prim >= 0]].tolist())
        assert {13, 17} <= visible
        for what, m in steps:
            rt.update_materials(m)
            rt.runRenderer(SPP)
            got.append((np.array(fb, copy=True), rt.renderGuides(rt.RT_GUIDE_ALBEDO)["albedo"]))
            seen.append(lean(rt.last_launches()))
    finally:
        rt.cleanupRenderer()
    assert seen[0] == seen[2] == [1] and seen[1] == [0], seen   # lean_ok followed the materials
    for (what, m), (frame, albedo), lean_seen in zip(steps, got, seen):
        fb, o = _init_mesh(rt, hm, m, [], cam, nx, ny)
        try:
            rt.runRenderer(SPP)
            same(frame, fb, what + ": frame against a fresh init")
            same(albedo, rt.renderGuides(rt.RT_GUIDE_ALBEDO)["albedo"], what + ": albedo against a fresh init")
            assert lean(rt.last_launches()) == lean_seen
        finally:
            rt.cleanupRenderer()
    assert not np.array_equal(bits(got[0][0]), bits(got[2][0])) and not np.array_equal(bits(got[1][1]), bits(got[0][1]))


# ---- 8. spheres ----------------------------------------------------------------------------------------------------------------------------

def _collect_spheres(rt, fb, cam, nx, ny):
    out = _collect(rt, fb, cam, nx, ny, False)
    rt.runRenderer(SPP)
    out["second frame"] = np.array(fb, copy=True)               # ordered by the cost map the first one recorded
    rt.runRendererProgressive(2)
    rt.runRendererProgressive(2)
    out["progressive 2 + 2"] = np.array(fb, copy=True)
    return out


@pytest.mark.parametrize("name", ["random_50x37", "cloud_hybrid"])
def test_spheres(rt, O, name):
    sp, mt, cam, nx, ny = G.sphere_frame(rt, name)
    rng = np.random.default_rng(61)
    sp2, mt2 = sp.copy(), mt.copy()
    movers = rng.choice(len(sp), 10, replace=False)
    sp2["center"][movers] = sp2["center"][movers] + rng.uniform(-1.5, 1.5, (10, 3)).astype(np.float32)
    a, b = int(np.flatnonzero(mt["type"] != mt["type"][0])[0]), 0           # the first sphere of another material type than sphere 0's, and sphere 0
    mt2[[a, b]] = mt[[b, a]]
    assert not np.array_equal(mt2, mt)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, DEPTH)
    try:
        rt.runRenderer(SPP)                                     # records a cost map of the OLD scene
        old = np.array(fb, copy=True)
        rt.runRendererProgressive(3)
        rt.update_spheres(sp2, mt2)
        assert rt.progressive_samples() == 0
        got = _collect_spheres(rt, fb, cam, nx, ny)
    finally:
        rt.cleanupRenderer()
    assert not np.array_equal(bits(got["frame"]), bits(old))
    fb = rt.initRendererSpheres(sp2, mt2, cam, nx, ny, DEPTH)
    try:
        ref = _collect_spheres(rt, fb, cam, nx, ny)
    finally:
        rt.cleanupRenderer()
    _same_all(got, ref, name + " edited against a fresh init")
    oracle = O.render(O.sphere_scene(sp2, mt2), cam, O.default_options(True), nx, ny, SPP, DEPTH)[0]
    for k in ("frame", "second frame", "progressive 2 + 2"):
        same(got[k], oracle, f"{name} edited: {k} against the oracle")


# ---- 9. what an edit leaves alone ----------------------------------------------------------------------------------------------------------

def _observed(rt, fb):
    return (bits(fb).copy(), stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.history_frames(), rt.preview_frames(), rt.last_exposure(),
            rt.last_guides_ms(), rt.last_denoise_ms(), rt.last_accumulate_ms(), rt.last_preview_ms(), rt.last_display_ms(), rt.last_rays_ms())


@pytest.mark.parametrize("kind", ["mesh", "spheres"])
def test_no_side_effects(rt, O, kind, tmp_path):
    if kind == "mesh":
        f = G.mesh_frame(rt, O, "tris300")
        hm = S.fresh_copy(rt, f["hm"], tmp_path)
        fb, o = _init_mesh(rt, hm, f["mats"], f["tex"], f["cam"], f["nx"], f["ny"])
        cam, nx, ny = f["cam"], f["nx"], f["ny"]
    else:
        sp, mt, cam, nx, ny = G.sphere_frame(rt, "random_50x37")
        fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, DEPTH)
    try:
        rt.runRenderer(SPP)
        rt.renderGuides()
        rt.denoiseFrame()
        rt.accumulateFrame()
        rt.previewFrame()
        rt.display_frame(flags=rt.RT_DISPLAY_AUTO_EXPOSURE)
        rt.trace_rays(*rt.centre_rays(cam, nx, ny, _all_pixels(nx, ny)))
        rt.runRendererProgressive(2)
        rt.runRenderer(SPP)
        before = _observed(rt, fb)
        assert before[2] and before[3] == 1 and before[4] == 1 and all(ms > 0.0 for ms in before[6:]) and rt.progressive_samples() == 2
        if kind == "mesh":
            nodes, ms = rt.mesh_bvh()[0], rt.last_update_ms()
            assert ms == 0.0
            rt.update_triangles(5, np.zeros(0, rt.triangle_dtype))          # count == 0: nothing at all
            assert rt.progressive_samples() == 2 and rt.last_update_ms() == 0.0
            assert np.array_equal(bits(rt.mesh_bvh()[0]), bits(nodes)) and _observed(rt, fb)[1:] == before[1:]
            rt.update_triangles(0, S.jitter(hm.tris, 35))
            assert rt.last_update_ms() > 0.0 and rt.progressive_samples() == 0
            after = _observed(rt, fb)
            assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
            rt.update_materials(f["mats"][::-1].copy())
        else:
            sp2 = sp.copy()
            sp2["center"][5:15] = sp2["center"][5:15] + np.float32(0.5)
            rt.update_spheres(sp2, mt)
        after = _observed(rt, fb)
        assert rt.progressive_samples() == 0
        assert np.array_equal(before[0], after[0])
        assert before[1:] == after[1:]
    finally:
        rt.cleanupRenderer()


# ---- 10. misuse ----------------------------------------------------------------------------------------------------------------------------

_MESH = ("sys.path.insert(0, %r); import scene_update_support as S\n"
         "hm = S.blob_mesh(rt, 8, 3); mats = np.zeros(4, rt.material_dtype); mats['texId'] = -1; t = hm.tris.copy(); real = S.is_real(t)\n"
         "ks, keep = rt.make_kernel_scene(hm, mats); rt.initRenderer(ks, rt.make_camera((30, 18, 42), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.1, 50.0), 8, 8, 4, keepalive=keep)\n"
         "r = rt.load_renderer(); i_real = int(np.flatnonzero(real)[0]); i_sent = int(np.flatnonzero(~real)[0]); one = t[i_real:i_real + 1].copy()\n"
         % __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
_SPHERES = "sp, mt, cam = rt.scene_random_spheres(32, 24); rt.initRendererSpheres(sp, mt, cam, 32, 24, 4); r = rt.load_renderer()\n"
_MISUSE = {
    "triangles_before_init": "rt.update_triangles(0, np.zeros(1, rt.triangle_dtype))\n",
    "materials_before_init": "rt.update_materials(np.zeros(1, rt.material_dtype))\n",
    "spheres_before_init": "rt.update_spheres(np.zeros(1, rt.sphere_dtype), np.zeros(1, rt.material_dtype))\n",
    "bvh_before_init": "rt.mesh_bvh()\n",
    "last_ms_before_init": "rt.last_update_ms()\n",
    "after_cleanup": _MESH + "rt.cleanupRenderer(); rt.update_triangles(0, one)\n",
    "triangles_on_spheres": _SPHERES + "rt.update_triangles(0, np.zeros(1, rt.triangle_dtype))\n",
    "materials_on_spheres": _SPHERES + "rt.update_materials(mt)\n",
    "bvh_on_spheres": _SPHERES + "rt.mesh_bvh()\n",
    "spheres_on_mesh": _MESH + "sp, mt, cam = rt.scene_three_spheres(8, 8); rt.update_spheres(sp, mt)\n",
    "first_negative": _MESH + "rt.update_triangles(-1, one)\n",
    "count_negative": _MESH + "r.updateTriangles(0, -1, one.ctypes.data)\n",
    "past_the_end": _MESH + "rt.update_triangles(len(t) - 1, t[-2:].copy())\n",
    "null_triangles": _MESH + "r.updateTriangles(0, 1, None)\n",
    "real_to_sentinel": _MESH + "one['v'][0, 0, 0] = np.inf; rt.update_triangles(i_real, one)\n",
    "real_to_negative_sentinel": _MESH + "one['v'][0, 0, 0] = -np.inf; rt.update_triangles(i_real, one)\n",
    "sentinel_to_real": _MESH + "rt.update_triangles(i_sent, one)\n",
    "mesh_id_out_of_range": _MESH + "one['meshID'] = 4; rt.update_triangles(i_real, one)\n",
    "materials_other_n": _MESH + "rt.update_materials(mats[:3].copy())\n",
    "materials_null": _MESH + "r.updateMaterials(None, 4)\n",
    "materials_bad_tex_id": _MESH + "mats['texId'][2] = 0; rt.update_materials(mats)\n",
    "spheres_other_n": _SPHERES + "rt.update_spheres(sp[:-1].copy(), mt[:-1].copy())\n",
    "spheres_null": _SPHERES + "r.updateSpheres(None, mt.ctypes.data, len(mt))\n",
    "spheres_bad_type": _SPHERES + "mt['type'][7] = 12; rt.update_spheres(sp, mt)\n",
    "bvh_null_nodes": _MESH + "r.getMeshBvh(None, 4, None)\n",
}


@pytest.mark.parametrize("case", sorted(_MISUSE))
def test_misuse_exits_99(case):
    """The library's misuse convention, each case in a child process of its own: 'rt error' on stderr and exit status 99 (a clean exit of a host-side check)."""
    exits_99(_MISUSE[case])
