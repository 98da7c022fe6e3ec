"""rebuildBvh (include/rt_api.h, "editing the scene") on the GPU.  The contract: after any sequence of edits and rebuilds everything the library computes is
bit-identical to cleanupRenderer + initRenderer with the mesh of the CPU twin (HostMesh.rebuild) and so, in PARITY mode, to the CPU oracle on that mesh.
Every comparison is np.array_equal on the raw 32-bit words.  Frames are 40x50 (staircase) and 48x40 (tris300) at 4 spp with 16 bounces; every test works on
a mesh of its own."""
import numpy as np
import pytest

import guides_reference as G
import rebuild_support as R
import scene_update_support as S
from preview_support import bits, exits_99, same, stats_tuple

pytestmark = pytest.mark.gpu
SPP, DEPTH = 4, 16
ALL_GUIDES = 1 | 2 | 4 | 8 | 16


def _init_mesh(rt, hm, mats, tex, cam, nx, ny, **opts):
    ks, keep = rt.make_kernel_scene(hm, mats, tex)
    fb = rt.initRenderer(ks, cam, nx, ny, DEPTH, keepalive=keep)
    o = rt.getDefaultRenderOptions(False)
    if opts:
        rt.setRenderOptions(o, **opts)
    return fb, o


def _all_pixels(nx, ny):
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny)), -1).reshape(-1, 2).astype(np.int32)


def _flat(t):
    for x in t:
        if isinstance(x, tuple):
            yield from _flat(x)
        else:
            yield x


def _collect(rt, fb, cam, nx, ny, o):
    """What a mesh scene yields: the frame and its launches, every guide plane, every plane of traceRays on the frame's centre rays, occludedRays, the
    counters = 1 frame with its statistics, the RT_FP_FAST frame and a progressive frame of 2 + 2 samples."""
    out = {}
    rt.runRenderer(SPP)
    out["frame"] = np.array(fb, copy=True)
    launches = rt.last_launches()
    for k, v in rt.renderGuides(ALL_GUIDES).items():
        out["guide " + k] = v
    org, d = rt.centre_rays(cam, nx, ny, _all_pixels(nx, ny))
    for k, v in rt.trace_rays(org, d).items():
        out["ray " + k] = v
    out["occluded"] = rt.occluded_rays(org, d).astype(np.uint32)
    rt.setRenderOptions(o, counters=1)
    rt.runRenderer(SPP)
    out["counted frame"] = np.array(fb, copy=True)
    out["stats"] = np.array([int(x) for x in _flat(stats_tuple(rt.getRenderStats())[2:])], np.uint64).view(np.uint32)
    rt.setRenderOptions(o, counters=0, fp=rt.RT_FP_FAST)
    rt.runRenderer(SPP)
    out["fast frame"] = np.array(fb, copy=True)
    rt.setRenderOptions(o, fp=rt.RT_FP_PARITY)
    rt.runRendererProgressive(2)
    rt.runRendererProgressive(2)
    out["progressive 2 + 2"] = np.array(fb, copy=True)
    return out, launches


def _same_all(got, ref, what):
    assert sorted(got[0]) == sorted(ref[0])
    for k in got[0]:
        same(got[0][k], ref[0][k], f"{what}: {k}")
    assert got[1] == ref[1] and got[1], what + ": rtLastLaunches"


def _fresh(rt, hm, mats, tex, cam, nx, ny, **opts):
    fb, o = _init_mesh(rt, hm, mats, tex, cam, nx, ny, **opts)
    try:
        return _collect(rt, fb, cam, nx, ny, o)
    finally:
        rt.cleanupRenderer()


def _rebuild_both(rt, hm, what):
    """rebuildBvh on the device and HostMesh.rebuild on the twin: old_slot, the device's triangles read through it, nodes and bounds must be the twin's."""
    before = hm.tris.copy()
    old = rt.rebuild_bvh()
    want = hm.rebuild()
    assert old.dtype == np.int32 and np.array_equal(old, want), (what, int((old != want).sum()), np.flatnonzero(old != want)[:8].tolist())
    moved = np.where(old >= 0, old, 0)
    device_tris = before[moved]
    device_tris[old < 0] = R.sentinels(rt, 1)[0]
    assert device_tris.tobytes() == hm.tris.tobytes(), what + ": triangles through old_slot"
    nodes, bounds = rt.mesh_bvh()
    assert len(nodes) == hm.view.numBvhNodes
    same(nodes, hm.bvh, what + ": nodes against the CPU twin")
    same(bounds, S.view_bounds(hm), what + ": bounds against the CPU twin")
    return old


def _scramble(rt, hm, seed=71):
    """The updateTriangles scramble: the real triangles permuted among the real slots on the device and on the twin, both refitted."""
    new = hm.tris.copy()
    real = np.flatnonzero(S.is_real(new))
    new[real] = new[real][np.random.default_rng(seed).permutation(len(real))]
    rt.update_triangles(0, new)
    hm.tris[:] = new
    hm.refit()


# ---- 1. the scrambled staircase ------------------------------------------------------------------------------------------------------------

def test_scrambled_staircase(rt, O):
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    nx, ny = G.STAIR_NX, G.STAIR_NY
    cam = rt.staircase_camera(nx, ny)
    fb, o = _init_mesh(rt, hm, mats, [], cam, nx, ny)
    try:
        assert rt.last_rebuild_ms() == 0.0
        _scramble(rt, hm)
        bad = int(rt.renderGuides(rt.RT_GUIDE_NODES)["nodes"].astype(np.int64).sum())
        _rebuild_both(rt, hm, "scrambled staircase")
        assert rt.last_rebuild_ms() > 0.0
        got = _collect(rt, fb, cam, nx, ny, o)
    finally:
        rt.cleanupRenderer()
    good = int(got[0]["guide nodes"].astype(np.int64).sum())
    print(f"node visits of the centre rays: scrambled {bad}, rebuilt {good}")
    assert good < bad
    oracle = O.render(O.mesh_scene(hm, mats, [], None), cam, O.default_options(False), nx, ny, SPP, DEPTH)[0]
    same(got[0]["frame"], oracle, "rebuilt staircase: frame against the oracle on the twin's mesh")
    same(got[0]["progressive 2 + 2"], oracle, "rebuilt staircase: progressive frame against the oracle")
    _same_all(got, _fresh(rt, hm, mats, [], cam, nx, ny), "rebuilt staircase against a fresh init")


# ---- 2. shapes -----------------------------------------------------------------------------------------------------------------------------

def _shape_mesh(rt, O, case):
    T = rt.RT_REBUILD_TILE
    if isinstance(case, tuple):
        return R.scrambled(S.blob_mesh(rt, *case))
    if case == "full tree":
        return R.scrambled(rt.HostMesh.build(S.blob_tris(rt, 64 * 3, 31), 3, extra_levels=0))
    if case == "one triangle":
        return rt.HostMesh.build(S.blob_tris(rt, 1, 21), 2)
    if case == "quantised":
        return R.scrambled(rt.HostMesh.build(R.quantised_tris(rt, 200), 3))
    if case == "2^17 mostly empty leaves":
        src = G.mesh_frame(rt, O, "tris300")["hm"].tris
        return R.scrambled(rt.HostMesh.build(src[S.is_real(src)], 1, extra_levels=8))
    if case == "sentinel before real":
        return S.sentinel_first_mesh(rt)
    if case in R.EXTREMES:
        return R.extreme_mesh(rt, case)
    n = {"T - 1": T - 1, "T": T, "T + 1": T + 1, "2 T + 3": 2 * T + 3}[case]
    hm = R.scrambled(rt.HostMesh.build(S.blob_tris(rt, n, 40 + n % 7), 5))
    assert int(S.is_real(hm.tris).sum()) == n
    return hm


SHAPES = [(2, 1), (4, 1), (4, 7), (256, 7), (512, 5), "full tree", "one triangle", "quantised", "2^17 mostly empty leaves", "sentinel before real",
          "T - 1", "T", "T + 1", "2 T + 3"] + list(R.EXTREMES)


@pytest.mark.parametrize("case", SHAPES, ids=[str(c) for c in SHAPES])
def test_shapes(rt, O, case):
    """getMeshBvh and old_slot against the twin, no render: the lowest trees, trees of several workgroups, every cut forced, one triangle, equal centroids and
    costs, a mostly empty tree, hidden triangles, triangle counts either side of one and two tiles of the scan kernels, and the float extremes of
    rebuild_support.EXTREMES (areas and costs that are +inf or NaN, nodes without a winner, costs of 0, infinite and denormal centroids: what each case holds is
    asserted on the CPU by tests/test_rebuild_api.py)."""
    hm = _shape_mesh(rt, O, case)
    if isinstance(case, tuple):
        assert hm.view.numBvhNodes // 2 == case[0] and hm.nppl == case[1]
    if case == "full tree":
        assert hm.view.numBvhNodes // 2 == 64 and S.is_real(hm.tris).all()
    if case == "2^17 mostly empty leaves":
        assert hm.view.numBvhNodes // 2 == 1 << 17
    mats = np.zeros(4, rt.material_dtype)
    mats["texId"] = -1
    mats["color"] = 0.7
    cam = rt.make_camera((30, 18, 42), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.1, 50.0)
    nx = ny = 16 if case == "sentinel before real" else 8
    fb, o = _init_mesh(rt, hm, mats, [], cam, nx, ny)
    try:
        if case == "sentinel before real":
            rt.runRenderer(SPP)
            without = rt.last_launches()
        _rebuild_both(rt, hm, str(case))
        if case == "sentinel before real":                      # the case in which compact leaf records appear
            rt.runRenderer(SPP)
            frame, launches = np.array(fb, copy=True), rt.last_launches()
    finally:
        rt.cleanupRenderer()
    if case == "sentinel before real":
        fb, o = _init_mesh(rt, hm, mats, [], cam, nx, ny)
        try:
            rt.runRenderer(SPP)
            same(frame, fb, "sentinel before real: frame against a fresh init")
            assert launches == rt.last_launches() and launches
        finally:
            rt.cleanupRenderer()
        print("lean before / after the rebuild:", sorted({l["lean"] for l in without}), sorted({l["lean"] for l in launches}))


# ---- 3. sequences --------------------------------------------------------------------------------------------------------------------------

def test_edit_rebuild_edit_rebuild(rt, O, tmp_path):
    f = G.mesh_frame(rt, O, "tris300")
    hm = S.fresh_copy(rt, f["hm"], tmp_path)
    args = (f["mats"], f["tex"], f["cam"], f["nx"], f["ny"])
    fb, o = _init_mesh(rt, hm, *args)
    try:
        _scramble(rt, hm, 81)
        _rebuild_both(rt, hm, "edit, rebuild")
        new = S.jitter(hm.tris, 82, amount=6.0)                 # an edit of the NEW slots
        rt.update_triangles(0, new)
        hm.tris[:] = new
        hm.refit()
        same(rt.mesh_bvh()[0], hm.bvh, "edit, rebuild, edit: nodes against the CPU twin")
        _rebuild_both(rt, hm, "edit, rebuild, edit, rebuild")
        got = _collect(rt, fb, f["cam"], f["nx"], f["ny"], o)
    finally:
        rt.cleanupRenderer()
    _same_all(got, _fresh(rt, hm, *args), "edit, rebuild, edit, rebuild against a fresh init")


def test_relayout_keeps_the_rebuild(rt, O, tmp_path):
    """setRenderOptions with another stripe_rows builds new device states from the host mirrors: they must hold the rebuilt scene, and rebuild again."""
    f = G.mesh_frame(rt, O, "tris300")
    hm = S.fresh_copy(rt, f["hm"], tmp_path)
    args = (f["mats"], f["tex"], f["cam"], f["nx"], f["ny"])
    fb, o = _init_mesh(rt, hm, *args)
    try:
        _scramble(rt, hm, 83)
        _rebuild_both(rt, hm, "rebuild")
        rt.setRenderOptions(o, stripe_rows=16)
        same(rt.mesh_bvh()[0], hm.bvh, "after the relayout: nodes against the CPU twin")
        got = _collect(rt, fb, f["cam"], f["nx"], f["ny"], o)
    finally:
        rt.cleanupRenderer()
    _same_all(got, _fresh(rt, hm, *args, stripe_rows=16), "rebuild, relayout against a fresh init")
    fb, o = _init_mesh(rt, hm, *args)
    try:
        rt.setRenderOptions(o, stripe_rows=16)
        _scramble(rt, hm, 84)
        _rebuild_both(rt, hm, "relayout, rebuild on the new device state")
    finally:
        rt.cleanupRenderer()


# ---- 4. what a rebuild leaves alone --------------------------------------------------------------------------------------------------------

def _observed(rt, fb):
    return (bits(fb).copy(), stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.history_frames(), rt.preview_frames(), rt.last_exposure(),
            rt.last_guides_ms(), rt.last_denoise_ms(), rt.last_accumulate_ms(), rt.last_preview_ms(), rt.last_display_ms(), rt.last_rays_ms(),
            rt.last_update_ms())


def test_no_side_effects(rt, O, tmp_path):
    f = G.mesh_frame(rt, O, "tris300")
    hm = S.fresh_copy(rt, f["hm"], tmp_path)
    cam, nx, ny = f["cam"], f["nx"], f["ny"]
    fb, o = _init_mesh(rt, hm, f["mats"], f["tex"], cam, nx, ny)
    try:
        rt.runRenderer(SPP)
        rt.renderGuides()
        rt.denoiseFrame()
        rt.accumulateFrame()
        rt.previewFrame()
        rt.display_frame(flags=rt.RT_DISPLAY_AUTO_EXPOSURE)
        rt.trace_rays(*rt.centre_rays(cam, nx, ny, _all_pixels(nx, ny)))
        _scramble(rt, hm, 85)
        rt.runRendererProgressive(2)
        rt.runRenderer(SPP)
        before = _observed(rt, fb)
        assert before[2] and before[3] == 1 and before[4] == 1 and all(ms > 0.0 for ms in before[6:]) and rt.progressive_samples() == 2
        assert rt.last_rebuild_ms() == 0.0
        rt.rebuild_bvh()
        assert rt.progressive_samples() == 0 and rt.last_rebuild_ms() > 0.0
        after = _observed(rt, fb)
        assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
        rt.accumulateFrame()
        rt.previewFrame()
        assert rt.history_frames() == 2 and rt.preview_frames() == 2       # the histories were kept
    finally:
        rt.cleanupRenderer()


# ---- 5. misuse -----------------------------------------------------------------------------------------------------------------------------

_MESH = ("sys.path.insert(0, %r); import scene_update_support as S\n"
         "hm = S.blob_mesh(rt, 8, 3); mats = np.zeros(4, rt.material_dtype); mats['texId'] = -1\n"
         "ks, keep = rt.make_kernel_scene(hm, mats); rt.initRenderer(ks, rt.make_camera((30, 18, 42), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.1, 50.0), 8, 8, 4, keepalive=keep)\n"
         % __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
_SPHERES = "sp, mt, cam = rt.scene_random_spheres(32, 24); rt.initRendererSpheres(sp, mt, cam, 32, 24, 4)\n"
_MISUSE = {
    "before_init": "rt.rebuild_bvh()\n",
    "last_ms_before_init": "rt.last_rebuild_ms()\n",
    "after_cleanup": _MESH + "rt.rebuild_bvh(); rt.cleanupRenderer(); rt.rebuild_bvh()\n",
    "on_spheres": _SPHERES + "rt.rebuild_bvh()\n",
}


@pytest.mark.parametrize("case", sorted(_MISUSE))
def test_misuse_exits_99(case):
    """The library's misuse convention, each case in a child process of its own: 'rt error' on stderr and exit status 99 (a clean exit of a host-side check)."""
    exits_99(_MISUSE[case])
