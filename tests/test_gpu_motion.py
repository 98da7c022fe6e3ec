"""rtMarkPose / renderMotion (include/rt_api.h) on the GPU against the test reference (tests/motion_reference.py): the motion planes of edited mesh and sphere
scenes, and accumulateFrame / previewFrame with a pose marked, every call, all pixels, bit for bit (np.array_equal on the raw 32-bit words).  The references
are fed the very framebuffers the GPU rendered (copied before the call) and the guide reference's planes of the edited scene.  Then: a mark without an edit
changes nothing, rebuildBvh carries the mark, a degenerate marked triangle, the lifetime of the mark, no side effects, the misuse exits and partitions."""
import numpy as np
import pytest

import accumulate_reference as A
import denoise_reference as D
import guides_reference as G
import motion_reference as M
from preview_support import NAN_CAP, bits as _bits, exits_99, init_frame as _init, same as _same, same_but_nan, stats_tuple, synthetic

pytestmark = pytest.mark.gpu


def _init_stairs(rt, O):
    """The unedited staircase_a on a HostMesh of the reference's own (frame 0 of motion_reference.stair_pose), under its camera."""
    f = G.mesh_frame(rt, O, "staircase_a")
    hm = M.stair_pose(rt, O, 0)[0]
    ks, keep = rt.make_kernel_scene(hm, f["mats"], f["tex"])
    return rt.initRenderer(ks, f["cam"], f["nx"], f["ny"], 16, keepalive=keep)


def _planes_same(got, ref, what, names=("prev_pos", "prev_normal", "screen")):
    for name in names:
        _same(got[name], ref[name], f"{what} {name}")


# ---- 1. the planes -----------------------------------------------------------------------------------------------------------

def test_planes_of_the_edited_staircase(rt, O):
    cam0 = A.sequence_camera(rt, "staircase_a", 0)
    cam, g, origin, dn, live, previous = M.stair_inputs(rt, O, 1)
    _init_stairs(rt, O)
    try:
        assert rt.last_motion_ms() == 0.0 and not rt.pose_marked()
        rt.setCamera(cam)
        unmarked = rt.renderMotion(cam0)
        rt.setCamera(cam0)
        rt.mark_pose()
        assert rt.pose_marked()
        rt.update_triangles(0, live)
        rt.setCamera(cam)
        with_prev, with_null, only_pos = rt.renderMotion(cam0), rt.renderMotion(None), rt.renderMotion(mask=M.POS)
        ms = rt.last_motion_ms()
    finally:
        rt.cleanupRenderer()
    assert ms > 0.0 and sorted(only_pos) == ["prev_pos"]
    g_plain = A.sequence_inputs(rt, O, "staircase_a", 1)[1]      # without a mark: the unedited mesh under camera 1 - P and the guide normal
    plain = M.motion_planes(g_plain, origin, dn, prev_cam=cam0)
    valid = g_plain["prim"] != G.PRIM_NONE
    _planes_same(unmarked, plain, "no mark")
    _same(unmarked["prev_pos"][valid], np.stack(M.hit_points(g_plain, origin, dn), axis=-1)[valid], "no mark: prev_pos = P")
    _same(unmarked["prev_normal"], g_plain["normal"], "no mark: prev_normal = the guide normal")
    _planes_same(with_prev, M.motion_planes(g, origin, dn, live, previous, prev_cam=cam0), "edited, previous camera")
    _planes_same(with_null, M.motion_planes(g, origin, dn, live, previous, prev_cam=cam), "edited, NULL camera")
    _same(only_pos["prev_pos"], with_prev["prev_pos"], "mask = POS")


@pytest.mark.parametrize("nx,ny", [(33, 9), (7, 3)])
def test_planes_of_the_tiny_mesh_with_floor_and_misses(rt, O, nx, ny):
    t = M.tiny_frame(rt, O, nx, ny)
    f = t["f"]
    hm0 = rt.HostMesh.build(f["hm"].tris[M.is_real(f["hm"].tris)].copy(), 5)
    assert hm0.tris.tobytes() == t["first"].tobytes()
    ks, keep = rt.make_kernel_scene(hm0, f["mats"], f["tex"], floor=f["floor"])
    rt.initRenderer(ks, t["cams"][0], nx, ny, 16, keepalive=keep)
    try:
        rt.setRenderOptions(rt.getDefaultRenderOptions(False), floor=1)
        rt.mark_pose()
        rt.update_triangles(0, t["live"])
        rt.setCamera(t["cams"][1])
        got = rt.renderMotion(t["cams"][0])
    finally:
        rt.cleanupRenderer()
    ref = M.motion_planes(t["g"], t["origin"], t["dn"], t["live"], t["first"], prev_cam=t["cams"][0])
    print(f"{nx} x {ny}: floor {int((t['g']['prim'] == G.PRIM_FLOOR).sum())}, miss {int((t['g']['prim'] == G.PRIM_NONE).sum())}, moved {int(ref['moved'].sum())}")
    assert (t["g"]["prim"] == G.PRIM_FLOOR).any() and (t["g"]["prim"] == G.PRIM_NONE).any() and ref["moved"].any()
    _planes_same(got, ref, f"tris300_floor {nx} x {ny}")


def test_planes_of_moved_and_resized_spheres(rt, O):
    cam0 = A.sequence_camera(rt, "random_50x37", 0)
    cam, g, origin, dn, live, previous, mt, idx = M.sphere_inputs(rt, O, 1)
    _init(rt, O, "random_50x37")
    try:
        rt.mark_pose()
        rt.update_spheres(live, mt)
        rt.setCamera(cam)
        got = rt.renderMotion(cam0)
    finally:
        rt.cleanupRenderer()
    ref = M.motion_planes(g, origin, dn, live, previous, prev_cam=cam0)
    resized = np.isin(g["prim"], idx[:2])
    print(f"random_50x37: {int(ref['moved'].sum())} pixels on moved spheres, {int(resized.sum())} of them on resized ones")
    assert ref["moved"].sum() >= 100 and resized.any() and (~ref["moved"] & (g["prim"] >= 0)).any()
    _planes_same(got, ref, "moved spheres")


# ---- 2., 3. the passes with a pose marked ------------------------------------------------------------------------------------

def _animate(rt, fb, inputs, edit, step, ref_step, marked=True, frames=3):
    """Frames 0 .. frames-1 on both sides: rtMarkPose (marked), the edit of frame k, setCamera, runRenderer(1), a copy of the framebuffer, the pass; the
    reference is fed the copy and the motion planes of frame k.  Returns per frame (got, ref, the reference's moved mask)."""
    res = []
    for k in range(frames):
        cam, g, origin, dn, live, previous = inputs(k)[:6]
        if marked:
            rt.mark_pose()
        edit(k, live)
        rt.setCamera(cam)
        rt.runRenderer(1)
        frame = np.array(fb, copy=True)
        got = step()
        mp = M.motion_planes(g, origin, dn, live, previous if marked else None)
        res.append((got, ref_step(frame, g, cam, origin, dn, mp["Pm"], mp["nm"]), M.motion_planes(g, origin, dn, live, previous)["moved"]))
    return res


def _mean_n(res):
    got, _, moved = res[-1]
    return float(got[1][moved].mean())


def test_accumulate_follows_the_moving_staircase(rt, O):
    flags = D.default_flags(True)
    runs = {}
    for marked in (True, False):
        fb = _init_stairs(rt, O)
        acc = M.MotionAccumulator()
        try:
            runs[marked] = _animate(rt, fb, lambda k: M.stair_inputs(rt, O, k), lambda k, live: rt.update_triangles(0, live),
                                    lambda: rt.accumulateFrame(history=True), lambda *a: acc.step(*a, flags=flags), marked)
        finally:
            rt.cleanupRenderer()
    for marked, res in runs.items():
        for k, (got, ref, _) in enumerate(res):
            _same(got[1], ref[1], f"accumulateFrame marked={marked} frame {k} history")
            _same(got[0], ref[0], f"accumulateFrame marked={marked} frame {k} out")
    print(f"mean N on the moved pixels of the last frame: {_mean_n(runs[True]):.3f} with rtMarkPose, {_mean_n(runs[False]):.3f} without")
    assert _mean_n(runs[True]) > _mean_n(runs[False])


def test_preview_follows_the_moving_staircase(rt, O):
    flags = D.default_flags(True)
    runs = {}
    for marked in (True, False):
        fb = _init_stairs(rt, O)
        pre = M.MotionPreviewer()
        try:
            runs[marked] = _animate(rt, fb, lambda k: M.stair_inputs(rt, O, k), lambda k, live: rt.update_triangles(0, live),
                                    lambda: rt.previewFrame(history=True, variance=True), lambda *a: pre.step(*a, flags=flags), marked)
        finally:
            rt.cleanupRenderer()
    for k, (got, ref, _) in enumerate(runs[True]):
        for a, b, what in zip(got, ref, ("out", "history", "variance")):
            _same(a, b, f"previewFrame frame {k} {what}")
    print(f"mean N on the moved pixels of the last frame: {_mean_n(runs[True]):.3f} with rtMarkPose, {_mean_n(runs[False]):.3f} without")
    assert _mean_n(runs[True]) > _mean_n(runs[False])


def test_preview_follows_moving_spheres_under_same_prim(rt, O):
    flags = D.default_flags(False)
    assert flags & M.SAME_PRIM
    mt = M.sphere_inputs(rt, O, 0)[6]
    runs = {}
    for marked in (True, False):
        fb = _init(rt, O, "random_50x37")[0]
        pre = M.MotionPreviewer()
        try:
            runs[marked] = _animate(rt, fb, lambda k: M.sphere_inputs(rt, O, k), lambda k, live: rt.update_spheres(live, mt),
                                    lambda: rt.previewFrame(history=True, variance=True), lambda *a: pre.step(*a, flags=flags), marked)
        finally:
            rt.cleanupRenderer()
    for k, (got, ref, _) in enumerate(runs[True]):
        for a, b, what in zip(got, ref, ("out", "history", "variance")):
            _same(a, b, f"previewFrame spheres frame {k} {what}")
    print(f"mean N on the moved spheres' pixels of the last frame: {_mean_n(runs[True]):.3f} with rtMarkPose, {_mean_n(runs[False]):.3f} without")
    assert _mean_n(runs[True]) > _mean_n(runs[False])


# ---- 4. a mark without an edit -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_spheres", "random_50x37", "tris300_floor", "staircase_a"])
def test_mark_without_an_edit_changes_nothing(rt, O, name):
    fb = _init(rt, O, name)[0]
    ny, nx = fb.shape[:2]
    res = {}
    try:
        for marked in (False, True):
            rt.reset_history(); rt.reset_preview(); rt.clear_pose()
            out = []
            for k in range(3):
                if marked:
                    rt.mark_pose()
                rt.setCamera(A.sequence_camera(rt, name, k))
                src = synthetic(70 + k, ny, nx)
                out.append(rt.accumulateFrame(src, history=True) + rt.previewFrame(src, history=True, variance=True))
            res[marked] = out
    finally:
        rt.cleanupRenderer()
    for k in range(3):
        for a, b, what in zip(res[True][k], res[False][k], ("accumulate out", "accumulate history", "preview out", "preview history", "preview variance")):
            _same(a, b, f"{name} call {k} {what}")
    assert float(res[True][2][1].max()) > 1.0


# ---- 5. rebuildBvh between mark and call -------------------------------------------------------------------------------------

def test_rebuild_carries_the_mark(rt, O):
    flags = D.default_flags(True)
    cam0, g0, o0, dn0 = M.stair_inputs(rt, O, 0)[:4]
    cam, g, origin, dn, live, previous = M.stair_inputs(rt, O, 1, True)
    old_ref = M.stair_pose(rt, O, 1, True)[3]
    fb = _init_stairs(rt, O)
    try:
        rt.runRenderer(1)
        f0 = np.array(fb, copy=True)
        a0 = rt.accumulateFrame(history=True)
        rt.mark_pose()
        rt.update_triangles(0, M.stair_pose(rt, O, 1)[1])
        old = rt.rebuild_bvh()
        assert rt.pose_marked()
        rt.setCamera(cam)
        planes = rt.renderMotion(cam0)
        rt.runRenderer(1)
        f1 = np.array(fb, copy=True)
        a1 = rt.accumulateFrame(history=True)
    finally:
        rt.cleanupRenderer()
    assert np.array_equal(old, old_ref) and (old_ref != np.arange(len(old_ref))).any()
    mp = M.motion_planes(g, origin, dn, live, previous, prev_cam=cam0)
    _planes_same(planes, mp, "after a rebuild")
    acc = M.MotionAccumulator()
    r0 = acc.step(f0, g0, cam0, o0, dn0, flags=flags)
    r1 = acc.step(f1, g, cam, origin, dn, mp["Pm"], mp["nm"], flags=flags)
    for got, ref, k in ((a0, r0, 0), (a1, r1, 1)):
        _same(got[1], ref[1], f"rebuild call {k} history"); _same(got[0], ref[0], f"rebuild call {k} out")
    assert float(r1[1][mp["moved"]].mean()) > 1.0


# ---- 6. one marked triangle of zero area ---------------------------------------------------------------------------------------

def test_degenerate_marked_triangle(rt, O):
    """The marked pose of the most seen moved triangle is made zero-area (never rendered: the edit that follows replaces it): its pixels get NaN planes, every
    comparison of the pass is false there and they start anew; the call returns and every other pixel is exact."""
    flags = D.default_flags(True)
    cam0, g0, o0, dn0 = M.stair_inputs(rt, O, 0)[:4]
    cam, g, origin, dn, live, previous = M.stair_inputs(rt, O, 1)
    moved = M.motion_planes(g, origin, dn, live, previous)["moved"]
    seen, counts = np.unique(g["prim"][moved], return_counts=True)
    slot = int(seen[np.argmax(counts)])
    flat = previous.copy()
    flat["v"][slot, 2] = flat["v"][slot, 1]
    fb = _init_stairs(rt, O)
    try:
        rt.runRenderer(1)
        f0 = np.array(fb, copy=True)
        rt.accumulateFrame()
        rt.update_triangles(slot, flat[slot:slot + 1])
        rt.mark_pose()
        rt.update_triangles(0, live)
        rt.setCamera(cam)
        planes = rt.renderMotion(cam0)
        rt.runRenderer(1)
        f1 = np.array(fb, copy=True)
        a1 = rt.accumulateFrame(history=True)
    finally:
        rt.cleanupRenderer()
    mp = M.motion_planes(g, origin, dn, live, flat, prev_cam=cam0)
    valid = g["prim"] != G.PRIM_NONE
    assert np.isnan(mp["prev_normal"]).any()
    for name in ("prev_pos", "prev_normal"):
        same_but_nan(planes[name], mp[name], f"degenerate {name}", valid, NAN_CAP)
    acc = M.MotionAccumulator()
    acc.step(f0, g0, cam0, o0, dn0, flags=flags)
    r1 = acc.step(f1, g, cam, origin, dn, mp["Pm"], mp["nm"], flags=flags)
    same_but_nan(a1[0], r1[0], "degenerate accumulate out", valid, NAN_CAP)
    same_but_nan(a1[1], r1[1], "degenerate accumulate history", valid, NAN_CAP)
    assert (r1[1][g["prim"] == slot] == 1.0).all()              # they start anew


# ---- 7. the lifetime of the mark -----------------------------------------------------------------------------------------------

def test_lifetime_of_the_mark(rt, O):
    fb, o, mesh = _init(rt, O, "random_50x37")
    sp, mt = G.sphere_frame(rt, "random_50x37")[:2]
    try:
        assert not rt.pose_marked()
        rt.mark_pose()
        rt.setCamera(A.sequence_camera(rt, "random_50x37", 1))
        rt.setRenderOptions(o, t_min=0.002)                      # a plain setRenderOptions
        rt.update_spheres(sp, mt)
        rt.runRenderer(1); rt.accumulateFrame(); rt.previewFrame(); rt.renderMotion()
        assert rt.pose_marked()
        rt.clear_pose()
        assert not rt.pose_marked()
        rt.mark_pose()
        rt.setRenderOptions(o, stripe_rows=16)                  # the device layout changes
        assert not rt.pose_marked()
        rt.mark_pose()
        _init(rt, O, "three_spheres")                           # a second init
        assert not rt.pose_marked()
        rt.mark_pose()
        rt.cleanupRenderer()
        _init(rt, O, "three_spheres")
        assert not rt.pose_marked()
    finally:
        rt.cleanupRenderer()


# ---- 8. no side effects --------------------------------------------------------------------------------------------------------

def test_no_side_effects(rt, O):
    def run(with_motion):
        fb = _init(rt, O, "random_50x37")[0]
        try:
            rt.runRenderer(2)
            rt.renderGuides()
            src = synthetic(5, *fb.shape[:2])
            a = rt.accumulateFrame(src, history=True)
            p = rt.previewFrame(src, history=True)
            before = (np.array(fb, copy=True), stats_tuple(rt.getRenderStats()), rt.last_launches(),
                      rt.last_guides_ms(), rt.last_accumulate_ms(), rt.last_preview_ms())
            if with_motion:
                rt.mark_pose(); rt.renderMotion(); rt.clear_pose(); rt.renderMotion(mask=M.SCREEN)
            after = (np.array(fb, copy=True), stats_tuple(rt.getRenderStats()), rt.last_launches(),
                     rt.last_guides_ms(), rt.last_accumulate_ms(), rt.last_preview_ms())
            assert _bits(before[0]).tobytes() == _bits(after[0]).tobytes() and before[1:] == after[1:]
            frames = (rt.history_frames(), rt.preview_frames())
            rt.runRendererProgressive(1)
            if with_motion:
                rt.renderMotion()
            rt.runRendererProgressive(1)
            prog = (np.array(fb, copy=True), rt.progressive_samples())
            den = rt.denoiseFrame(src)
            a2 = rt.accumulateFrame(src, history=True)        # both histories are where the calls above left them
            p2 = rt.previewFrame(src, history=True)
            return a, p, frames, prog, den, a2, p2
        finally:
            rt.cleanupRenderer()
    plain, motion = run(False), run(True)
    assert plain[2] == motion[2] == (1, 1) and plain[3][1] == motion[3][1] == 2
    _same(motion[3][0], plain[3][0], "the progressive frame")
    _same(motion[4], plain[4], "denoiseFrame")
    for k, what in ((5, "accumulateFrame"), (6, "previewFrame")):
        for a, b in zip(motion[k], plain[k]):
            _same(a, b, f"the next {what}")


# ---- 9. misuse -----------------------------------------------------------------------------------------------------------------

_SETUP = ("sp, mt, cam = rt.scene_three_spheres(16, 8)\nrt.initRendererSpheres(sp, mt, cam, 16, 8, 5)\n"
          "a = np.zeros((8, 16, 3), np.float32); p = a.ctypes.data_as(C.POINTER(C.c_float)); r = rt.load_renderer()\n")


@pytest.mark.parametrize("call", ["r.renderMotion(0, None, p, p, p)", "r.renderMotion(8, None, p, p, p)", "r.renderMotion(1 | 16, None, p, p, p)",
                                  "r.renderMotion(3, None, p, None, None)", "r.renderMotion(4, None, None, None, None)",
                                  "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); rt.renderMotion()",
                                  "rt.cleanupRenderer(); rt.mark_pose()", "rt.cleanupRenderer(); rt.renderMotion()"])
def test_misuse_exits_99(call):
    exits_99(_SETUP + call + "\n")


# ---- 10. partitions ------------------------------------------------------------------------------------------------------------

def test_partitioned_renderer_returns_whole_image_planes(rt, O):
    cam0 = A.sequence_camera(rt, "random_50x37", 0)
    cam, g, origin, dn, live, previous, mt, idx = M.sphere_inputs(rt, O, 1)
    _init(rt, O, "random_50x37", part_rank=1, part_world=2, stripe_rows=8)
    try:
        rt.mark_pose()
        rt.update_spheres(live, mt)
        rt.setCamera(cam)
        got = rt.renderMotion(cam0)
    finally:
        rt.cleanupRenderer()
    _planes_same(got, M.motion_planes(g, origin, dn, live, previous, prev_cam=cam0), "partitioned")
