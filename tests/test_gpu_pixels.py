"""GPU checks of renderPixels (include/rt_api.h) against the frame rendered in the same process and the CPU oracle's per-pixel region renders
(tests/pixels_reference.py): bit for bit in PARITY mode - the frame's pixels, per-pixel sample counts, continuation across calls, the smallest lists and
the refill path through one wave, a list that crosses RT_PIXEL_CHUNK, independence of the partition, the camera and scene edits - nothing another call observes changes, the FAST objects
within the tolerance the project states for the FAST frame, and misuse is the library's exit 99."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pixels_reference as PR
from preview_support import bits, exits_99, same, stats_tuple

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _at(plane, ij):
    return plane[ij[:, 1], ij[:, 0]]


# ---- 1. equals the frame and the oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,ns", [("S1", 5), ("S2", 4), ("M1", 3), ("M1_floor", 3), ("M1_tex", 3), ("M2_floor", 3)])
def test_equals_the_frame_and_the_oracle(rt, O, tag, ns):
    ij, first = PR.standard_list(tag)
    fb = PR.init(rt, tag, counters=1)
    try:
        rt.runRenderer(ns, 8, 8)
        frame = np.array(fb, copy=True)
        frame_rays = int(rt.getRenderStats().rays)
        out, _, rays = rt.render_pixels(ij, ns, rays=True)
    finally:
        rt.cleanupRenderer()
    ref_out, ref_rays = PR.oracle_pixels(rt, O, tag, ij, ns)
    same(out, _at(frame, ij), f"{tag}: the list against the frame of the same process")
    same(out, ref_out, f"{tag}: the list against the oracle's pixels")
    assert np.array_equal(rays, ref_rays), (tag, int((rays != ref_rays).sum()))
    assert int(rays[first].sum(dtype=np.uint64)) == frame_rays == int(PR.oracle_frame(rt, O, tag, ns)[1].rays)


# ---- 2. per-pixel counts ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["S2", "M1"])
def test_per_pixel_counts(rt, O, tag):
    """ns[k] cycles through 1, 2, 3, 7 over the standard list: entry k is the pixel of the frame of its own count."""
    ij, _ = PR.standard_list(tag)
    counts = np.array([1, 2, 3, 7], np.int32)[np.arange(len(ij)) % 4]
    fb = PR.init(rt, tag)
    try:
        out, _, rays = rt.render_pixels(ij, counts, rays=True)
        frames = {}
        for c in (1, 2, 3, 7):
            rt.runRenderer(c, 8, 8)
            frames[c] = np.array(fb, copy=True)
    finally:
        rt.cleanupRenderer()
    ref_out, ref_rays = PR.oracle_pixels(rt, O, tag, ij, counts)
    for c in (1, 2, 3, 7):
        m = counts == c
        same(out[m], _at(frames[c], ij[m]), f"{tag}: entries of {c} samples against runRenderer({c})")
    same(out, ref_out, f"{tag}: per-pixel counts against the oracle")
    assert np.array_equal(rays, ref_rays)


# ---- 3. continuation -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["S2", "M1"])
def test_continuation(rt, O, tag):
    ij, _ = PR.standard_list(tag)
    n = len(ij)
    PR.init(rt, tag)
    try:
        one_out, one_state, one_rays = rt.render_pixels(ij, 7, rays=True)
        a_out, a_state, a_rays = rt.render_pixels(ij, 3, rays=True)
        b_out, b_state, b_rays = rt.render_pixels(ij, 4, first=np.full(n, 3, np.int32), state=a_state, rays=True)
        st, total = None, np.zeros(n, np.uint64)
        for f, c in ((0, 1), (1, 1), (2, 5)):
            c_out, st, r = rt.render_pixels(ij, c, first=None if f == 0 else np.full(n, f, np.int32), state=st, rays=True)
            total += r
    finally:
        rt.cleanupRenderer()
    same(a_out, PR.oracle_pixels(rt, O, tag, ij, 3)[0], f"{tag}: the first three samples against the oracle")
    assert (bits(a_out) != bits(one_out)).any(axis=1).mean() > 0.5
    same(b_out, one_out, f"{tag}: 3 + 4 samples against 7 in one call, out")
    assert np.array_equal(b_state, one_state) and not np.array_equal(a_state, one_state)
    assert np.array_equal(a_rays.astype(np.uint64) + b_rays, one_rays)
    same(c_out, one_out, f"{tag}: 1 + 1 + 5 samples against 7 in one call, out")
    assert np.array_equal(st, one_state) and np.array_equal(total, one_rays)
    same(one_out, PR.oracle_pixels(rt, O, tag, ij, 7)[0], f"{tag}: 7 samples against the oracle")
    # the state is what the definition says: the bits of the colour sum, out = sum / 7
    assert np.array_equal(bits(one_state[:, :3].view(np.float32) / np.float32(7)), bits(one_out))


# ---- 4. smallest shapes, the refill path (a subprocess each: the switch is read per call) -----------------------------------------

_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import cuda_raytracing_optimized_amd as rt
import pixels_reference as PR
a = json.loads(sys.argv[1])
PR.init(rt, a["tag"])
out, state, rays = rt.render_pixels(np.load(a["ij"]), a["ns"], rays=True)
np.savez(a["out"], out=out, rays=rays, ms=rt.last_pixels_ms())
rt.cleanupRenderer()
""" % (ROOT, os.path.join(ROOT, "tests"))


def _in_child(tmp_path, tag, ij, ns, env):
    np.save(tmp_path / "ij.npy", np.ascontiguousarray(ij, dtype=np.int32))
    args = dict(tag=tag, ns=ns, ij=str(tmp_path / "ij.npy"), out=str(tmp_path / "res.npz"))
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(args)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.load(tmp_path / "res.npz")


def _extreme_pixels(rt, O):
    _, rays = PR.oracle_planes(rt, O, "S2", 4)
    lo, hi = np.unravel_index(int(rays.argmin()), rays.shape), np.unravel_index(int(rays.argmax()), rays.shape)
    return np.array([[lo[1], lo[0]]], np.int32), np.array([[hi[1], hi[0]]], np.int32)


@pytest.mark.parametrize("case", ["cheapest", "dearest", "n63", "n64", "n65", "waves1_S2", "waves1_M1", "waves3_200"])
def test_smallest_shapes_and_the_refill_path(rt, O, tmp_path, case):
    tag, env, ns = "S2", {}, 4
    if case in ("cheapest", "dearest"):
        ij = _extreme_pixels(rt, O)[0 if case == "cheapest" else 1]
    elif case.startswith("n6"):
        ij = PR.standard_list("S2")[0][: int(case[1:])]
    elif case == "waves1_S2":
        ij, env = PR.standard_list("S2")[0], {"RT_PIXELS_WAVES": "1"}
        assert len(ij) == 3109
    elif case == "waves1_M1":
        tag, ns, ij, env = "M1", 3, PR.standard_list("M1")[0], {"RT_PIXELS_WAVES": "1"}
    else:
        ij, env = PR.standard_list("S2")[0][100:300], {"RT_PIXELS_WAVES": "3"}
    got = _in_child(tmp_path, tag, ij, ns, env)
    ref_out, ref_rays = PR.oracle_pixels(rt, O, tag, ij, ns)
    print(case, "entries", len(ij), "kernel ms", float(got["ms"]))
    same(got["out"], ref_out, f"{case}: out against the oracle")
    assert np.array_equal(got["rays"], ref_rays)
    assert float(got["ms"]) > 0.0


def test_chunk_crossing(rt):
    """RT_PIXEL_CHUNK + 65 entries on S1 - 257 distinct pixels of the standard list, repeated in order: the second chunk holds 65 entries and starts in the
    middle of a repetition.  At one sample per entry out, state and rays equal, bit for bit, those of the 257 pixels alone, in the caller's order (the small
    list is tied to the frame and the oracle by test_equals_the_frame_and_the_oracle); so does the same list continued by one more sample from the returned
    states - the buffer that goes up and comes down at a chunk's offset.  Adjacent entries of the reference differ: an offset error cannot hide."""
    n, m = rt.RT_PIXEL_CHUNK + 65, 257
    assert n == (1 << 22) + 65
    idx = np.arange(n) % m
    every, first_seen = PR.standard_list("S1")
    small = np.ascontiguousarray(every[first_seen][:m])
    assert len(np.unique(small[:, 1] * 40 + small[:, 0])) == m
    ij = np.ascontiguousarray(small[idx])
    PR.init(rt, "S1")
    try:
        ref_out, ref_state, ref_rays = rt.render_pixels(small, 1, rays=True)
        ref2_out, ref2_state, ref2_rays = rt.render_pixels(small, 1, first=np.ones(m, np.int32), state=ref_state, rays=True)
        out, state, rays = rt.render_pixels(ij, 1, rays=True)
        ms = rt.last_pixels_ms()
        out2, state2, rays2 = rt.render_pixels(ij, 1, first=np.ones(n, np.int32), state=state, rays=True)
        ms2 = rt.last_pixels_ms()
    finally:
        rt.cleanupRenderer()
    print("entries", n, "kernel ms", ms, ms2)
    for ref in (ref_out, ref2_out):                         # entry k against entry k + 1, the last against the first of the next repetition
        assert (bits(ref) != bits(np.roll(ref, -1, axis=0))).any(axis=1).all()
    assert ms > 0.0 and ms2 > 0.0
    same(out, ref_out[idx], "one sample across the chunk boundary, out")
    assert np.array_equal(state, ref_state[idx]) and np.array_equal(rays, ref_rays[idx])
    same(out2, ref2_out[idx], "continued by one sample across the chunk boundary, out")
    assert np.array_equal(state2, ref2_state[idx]) and np.array_equal(rays2, ref2_rays[idx])
    assert not np.array_equal(ref2_state, ref_state) and (ref_rays > 0).all()


# ---- 5. independence -------------------------------------------------------------------------------------------------------------

def test_independent_of_partition_and_counters(rt, O):
    """The same bits under three stripes of 16 rows (stripe_rows must be a multiple of 8: setRenderOptions refuses 3), as member 1 of 2, with counters on."""
    ij, _ = PR.standard_list("S2")
    ref_out, ref_rays = PR.oracle_pixels(rt, O, "S2", ij, 4)
    PR.init(rt, "S2")
    try:
        for opts in (dict(stripe_rows=16), dict(part_world=2, part_rank=1), dict(counters=1)):
            rt.setRenderOptions(rt.getDefaultRenderOptions(True), **opts)
            out, _, rays = rt.render_pixels(ij, 4, rays=True)
            same(out, ref_out, f"S2 under {opts}")
            assert np.array_equal(rays, ref_rays), opts
    finally:
        rt.cleanupRenderer()


def test_follows_the_camera_and_scene_edits(rt, O):
    """After setCamera and after updateSpheres the list's result is that of a fresh init of the edited scene (and of the oracle on it)."""
    ij, _ = PR.standard_list("S2")
    s = PR.scene(rt, "S2")
    nx, ny, depth = s["nx"], s["ny"], s["depth"]
    cam2 = rt.make_camera((11, 3, 5), (0, 0.5, 0), (0, 1, 0), 30.0, nx / ny, 0.1, 10.0)
    sp2, mt2 = s["sp"].copy(), s["mt"].copy()
    sp2["center"][1:40, 1] += 0.35                          # lift a few dozen spheres, recolour them
    mt2["color"][1:40] = mt2["color"][1:40][:, ::-1]
    PR.init(rt, "S2")
    try:
        before, _, _ = rt.render_pixels(ij, 4)
        rt.setCamera(cam2)
        moved, _, _ = rt.render_pixels(ij, 4)
        rt.update_spheres(sp2, mt2)
        edited, _, _ = rt.render_pixels(ij, 4)
        rt.cleanupRenderer()
        rt.initRendererSpheres(s["sp"], s["mt"], cam2, nx, ny, depth)
        fresh_moved, _, _ = rt.render_pixels(ij, 4)
        rt.cleanupRenderer()
        rt.initRendererSpheres(sp2, mt2, cam2, nx, ny, depth)
        fresh_edited, _, _ = rt.render_pixels(ij, 4)
    finally:
        rt.cleanupRenderer()
    assert (bits(before) != bits(moved)).any(axis=1).mean() > 0.5 and (bits(moved) != bits(edited)).any(axis=1).mean() > 0.02
    same(moved, fresh_moved, "after setCamera against a fresh init")
    same(edited, fresh_edited, "after updateSpheres against a fresh init")
    ref, _ = O.render(O.sphere_scene(sp2, mt2), cam2, O.default_options(True), nx, ny, 4, depth)
    same(edited, _at(ref, ij), "after both against the oracle")


# ---- 6. leaves everything else alone ---------------------------------------------------------------------------------------------

def test_changes_nothing_another_call_observes(rt, O):
    ij, _ = PR.standard_list("S2")
    fb = PR.init(rt, "S2")
    try:
        rt.runRenderer(8, 8, 8)
        rt.runRenderer(8, 8, 8)                             # (the second frame is ordered by the first one's cost map)
        with_map = [l["phase"] for l in rt.last_launches()]
        rt.renderGuides()
        rt.trace_rays(*rt.centre_rays(PR.scene(rt, "S2")["cam"], 64, 48, ij[:100]))
        rt.runRendererProgressive(2, 8, 8)
        seen = lambda: (bits(np.array(fb, copy=True)).tobytes(), stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.last_sphere_form(),
                        rt.progressive_samples(), rt.last_rays_ms(), rt.last_guides_ms())
        was = seen()
        assert was[4] == 2 and was[5] > 0 and was[6] > 0
        out, _, _ = rt.render_pixels(ij, 4)
        assert rt.last_pixels_ms() > 0
        assert seen() == was
        rt.render_region(3, 5, 20, 9, 2)
        assert seen() == was
        rt.runRendererProgressive(2, 8, 8)                  # the next pass continues the progressive frame as if nothing had happened
        assert rt.progressive_samples() == 4
        same(np.array(fb, copy=True), PR.oracle_frame(rt, O, "S2", 4)[0], "the progressive frame after 2 + 2 samples around a renderPixels call")
        rt.runRenderer(8, 8, 8)                             # ... and the cost map is still the one the frames recorded
        assert [l["phase"] for l in rt.last_launches()] == with_map == [2]
    finally:
        rt.cleanupRenderer()
    same(out, PR.oracle_pixels(rt, O, "S2", ij, 4)[0], "the list in between")


def test_render_region_is_the_frames_rectangle(rt, O):
    fb = PR.init(rt, "M1")
    try:
        got = rt.render_region(5, 3, 31, 20, 3)
    finally:
        rt.cleanupRenderer()
    assert got.shape == (17, 26, 3)
    same(got, PR.oracle_frame(rt, O, "M1", 3)[0][3:20, 5:31], "render_region against the oracle's rectangle")


# ---- 7. FAST ---------------------------------------------------------------------------------------------------------------------

def _full_list(nx, ny):
    jj, ii = np.mgrid[0:ny, 0:nx]
    return np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.int32)


def test_fast_spheres_within_the_fast_frames_tolerance(rt, O):
    """S2's scene at 300x200x4, the configuration and the tolerance of test_fast_mode_within_tolerance (tests/test_gpu_parity_spheres.py): at least 97 % of
    the channels within 1e-4 of the oracle, mean |diff| <= 2e-3, RMSE <= 0.03.  The share bit-equal to the FAST frame is printed, not asserted."""
    nx, ny, ns = 300, 200, 4
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    ref, _ = O.render(O.sphere_scene(sp, mt), cam, O.default_options(True), nx, ny, ns, 50)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    try:
        rt.setRenderOptions(rt.getDefaultRenderOptions(True), fp=rt.RT_FP_FAST)
        rt.runRenderer(ns, 8, 8)
        frame = np.array(fb, copy=True)
        out, _, _ = rt.render_pixels(_full_list(nx, ny), ns)
    finally:
        rt.cleanupRenderer()
    got = out.reshape(ny, nx, 3)
    close = np.abs(got - ref) <= 1e-4
    print("FAST spheres: close", close.mean(), "mean abs", np.abs(got - ref).mean(), "rmse", rt.rmse(got, ref),
          "channels bit-equal to the FAST frame", float((bits(got) == bits(frame)).mean()))
    assert close.mean() >= 0.97
    assert np.abs(got - ref).mean() <= 2e-3
    assert rt.rmse(got, ref) <= 0.03


def test_fast_mesh_within_the_fast_frames_tolerance(rt, O):
    """The staircase at 96x120x4, depth 64, the configuration and the tolerance of test_mesh_fast_mode_within_tolerance (tests/test_gpu_parity_mesh.py): at
    least 90 % of the channels within 1e-3 of the oracle, RMSE <= 0.05.  The share bit-equal to the FAST frame is printed, not asserted."""
    nx, ny, ns = 96, 120, 4
    s = PR.scene(rt, "M1")
    cam = rt.staircase_camera(nx, ny)
    ref, _ = O.render(O.mesh_scene(s["hm"], s["mats"]), cam, O.default_options(False), nx, ny, ns, 64)
    ks, keep = rt.make_kernel_scene(s["hm"], s["mats"])
    fb = rt.initRenderer(ks, cam, nx, ny, 64, keepalive=keep)
    try:
        rt.setRenderOptions(rt.getDefaultRenderOptions(False), fp=rt.RT_FP_FAST)
        rt.runRenderer(ns, 8, 8)
        frame = np.array(fb, copy=True)
        out, _, _ = rt.render_pixels(_full_list(nx, ny), ns)
    finally:
        rt.cleanupRenderer()
    got = out.reshape(ny, nx, 3)
    close = np.abs(got - ref) <= 1e-3
    print("FAST mesh: close", close.mean(), "rmse", rt.rmse(got, ref), "channels bit-equal to the FAST frame", float((bits(got) == bits(frame)).mean()))
    assert close.mean() >= 0.90
    assert rt.rmse(got, ref) <= 0.05


# ---- 8. misuse -------------------------------------------------------------------------------------------------------------------

_INIT = ("import sys; sys.path.insert(0, %r); import pixels_reference as PR\n" % os.path.join(ROOT, "tests") +
         "PR.init(rt, 'S2'); r = rt.load_renderer(); ij = np.zeros((4, 2), np.int32)\n"
         "ip, up = C.POINTER(C.c_int32), C.POINTER(C.c_uint32); out = np.zeros((4, 3), np.float32); st = np.zeros((4, 4), np.uint32)\n"
         "p = lambda a, t: a.ctypes.data_as(t); o = p(out, C.POINTER(rt.vec3))\n")


@pytest.mark.parametrize("body", [
    "ij[2, 0] = 64; rt.render_pixels(ij, 2)",                                                                       # i = nx
    "rt.render_pixels(ij, 0)",                                                                                      # c = 0
    "r.renderPixels(4, p(ij, ip), 2, None, p(np.ones(4, np.int32), ip), None, o, None)",                            # first without state
    "r.renderPixels(4, p(ij, ip), 2, None, None, None, None, None)",                                                # all outputs NULL
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), rng=rt.RT_RNG_COUNTER); rt.render_pixels(ij, 2)",        # the counter stream
    "st[:, 3] = 1; rt.render_pixels(ij, 65536, first=np.ones(4, np.int32), state=st)",                              # f + c = 65537
    "st[:, 3] = 1; st[2, 3] = 0; rt.render_pixels(ij, 2, first=np.ones(4, np.int32), state=st)",                    # a stream word of 0: no state of any stream
    "r.renderPixels(-1, p(ij, ip), 2, None, None, None, o, None)",
    "r.renderPixels(4, None, 2, None, None, None, o, None)",
    "ij[1, 1] = -1; rt.render_pixels(ij, 2)",
    "st[:, 3] = 1; rt.render_pixels(ij, 2, first=-np.ones(4, np.int32), state=st)",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), variant=1); rt.render_pixels(ij, 2)",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); rt.render_pixels(ij, 2)",
])
def test_misuse_exits_99(body):
    exits_99(_INIT + body + "\n")


def test_the_largest_total_is_accepted_and_an_empty_list_writes_nothing(rt):
    """f + c = RT_PROGRESSIVE_MAX_SAMPLES passes the check that 65537 fails: 65535 samples of two pixels of S1 and then one more, continued from the state the
    first call returned, equal 65536 in one call; n = 0 returns and writes nothing."""
    PR.init(rt, "S1")
    try:
        r = rt.load_renderer()
        ip, up = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        out = np.full((2, 3), 7.0, np.float32)
        state = np.full((2, 4), 9, np.uint32)
        rays = np.full(2, 5, np.uint32)
        ij = np.array([[0, 0], [39, 23]], np.int32)
        before = rt.last_pixels_ms()
        r.renderPixels(0, ij.ctypes.data_as(ip), 2, None, None, state.ctypes.data_as(up), out.ctypes.data_as(C.POINTER(rt.vec3)), rays.ctypes.data_as(up))
        assert (out == 7.0).all() and (state == 9).all() and (rays == 5).all() and rt.last_pixels_ms() == before
        one, one_state, _ = rt.render_pixels(ij, 65536)
        _, st, _ = rt.render_pixels(ij, 65535)
        got, got_state, _ = rt.render_pixels(ij, 1, first=np.full(2, 65535, np.int32), state=st)
    finally:
        rt.cleanupRenderer()
    same(got, one, "65535 + 1 samples against 65536 in one call")
    assert np.array_equal(got_state, one_state) and (got_state[:, 3] != 0).all()
