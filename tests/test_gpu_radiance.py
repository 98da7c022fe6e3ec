"""GPU checks of radianceRays (include/rt_api.h) against the CPU oracle's one-pixel renders through the pinhole camera (tests/radiance_reference.py) and
against the library's own frame under that camera: bit for bit in PARITY mode - the standard lists with implicit and explicit seed ids, continuation across
calls, per-entry counts, the smallest lists and the refill path through one wave, a list that crosses RT_RAY_CHUNK, independence of the partition, the
counters and the camera, scene edits - nothing another call observes changes, the FAST objects within the tolerance the project states for the FAST frame,
and misuse is the library's exit 99 (the calls before init: tests/test_radiance_api.py, which needs no GPU)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pixels_reference as PR
import radiance_reference as RR
from preview_support import bits, exits_99, same, stats_tuple

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ns(tag):
    return 3 if PR.is_mesh(tag) else 4


# ---- 1. equals the oracle --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", sorted(RR.LIST_SEED))
def test_equals_the_oracle(rt, tag):
    org, _, d = RR.standard_list(tag)
    PR.init(rt, tag)
    try:
        out, _, rays = rt.radiance_rays(org, d, _ns(tag), rays=True)
        ms = rt.last_radiance_ms()
    finally:
        rt.cleanupRenderer()
    ref_out, ref_rays, _ = RR.oracle_standard(tag, _ns(tag))
    print(tag, "rays", len(org), "kernel ms", ms)
    same(out, ref_out, f"{tag}: the list against the oracle's pinhole pixels")
    assert np.array_equal(rays, ref_rays), (tag, int((rays != ref_rays).sum()))
    assert ms > 0.0


@pytest.mark.parametrize("tag", ["S2", "M1"])
def test_explicit_ids(rt, tag):
    """Shuffled explicit ids, most of them above nx * ny: the id alone chooses the stream, not the entry's place."""
    org, T, d = RR.standard_list(tag)
    nx, ny, _ = PR.SCENES[tag]
    ids = (np.random.default_rng(11).permutation(len(org)) * 37 + 5).astype(np.uint32)
    assert (ids > nx * ny).mean() > 0.9 and (ids < nx * ny).any()
    PR.init(rt, tag)
    try:
        out, _, rays = rt.radiance_rays(org, d, _ns(tag), ids=ids, rays=True)
    finally:
        rt.cleanupRenderer()
    ref_out, ref_rays = RR.oracle_rays(tag, org, T, ids, _ns(tag))
    same(out, ref_out, f"{tag}: explicit ids against the oracle")
    assert np.array_equal(rays, ref_rays)
    assert (bits(out) != bits(RR.oracle_standard(tag, _ns(tag))[0])).any(axis=1).mean() > 0.3      # (another id is another stream)


# ---- 2. a ray is the pixel of the pinhole frame -----------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["S2", "M1"])
def test_equals_the_frame_under_the_pinhole_camera(rt, tag):
    """setCamera(rtPinholeCamera(o, T)) and runRenderer(4): every pixel of the frame traces the one ray, pixel (i, j) with the seed id j * nx + i."""
    org, T, d = RR.standard_list(tag)
    _, ref_rays, _ = RR.oracle_standard(tag, _ns(tag))
    cam_o = np.array(list(PR.scene(rt, tag)["cam"].origin.e), np.float32)
    probes = np.flatnonzero((org != cam_o).any(axis=1))
    k = int(probes[np.argsort(ref_rays[probes])[len(probes) * 3 // 4]])         # a probe among the dearer ones: its paths draw
    nx, ny, _ = PR.SCENES[tag]
    fb = PR.init(rt, tag)
    try:
        rt.setCamera(rt.pinhole_camera(org[k], T[k]))
        rt.runRenderer(4, 8, 8)
        frame = np.array(fb, copy=True)
        out, _, _ = rt.radiance_rays(np.repeat(org[k:k + 1], nx * ny, axis=0), np.repeat(d[k:k + 1], nx * ny, axis=0), 4, ids=np.arange(nx * ny, dtype=np.uint32))
    finally:
        rt.cleanupRenderer()
    assert frame.shape == (ny, nx, 3)
    same(out, frame.reshape(-1, 3), f"{tag}: nx * ny copies of ray {k} against the frame under the pinhole camera")
    assert len(np.unique(bits(out), axis=0)) > nx * ny // 4                                     # (the ids are different streams)


# ---- 3. continuation -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["S2", "M1"])
def test_continuation(rt, tag):
    org, T, d = RR.standard_list(tag)
    n = len(org)
    PR.init(rt, tag)
    try:
        one_out, one_state, one_rays = rt.radiance_rays(org, d, 4, rays=True)
        got = {}
        for split in ((1, 3), (2, 2), (1, 1, 1, 1)):
            st, f, total = None, 0, np.zeros(n, np.uint64)
            for c in split:
                out, st, r = rt.radiance_rays(org, d, c, first=None if f == 0 else np.full(n, f, np.int32), state=st, rays=True)
                total += r
                f += c
            got[split] = (out, st, total)
        first_out, first_state, _ = rt.radiance_rays(org, d, 1)
    finally:
        rt.cleanupRenderer()
    for split, (out, st, total) in got.items():
        same(out, one_out, f"{tag}: {split} samples against 4 in one call, out")
        assert np.array_equal(st, one_state), split
        assert np.array_equal(total, one_rays), split
    assert not np.array_equal(first_state, one_state) and (bits(first_out) != bits(one_out)).any(axis=1).mean() > 0.3
    same(one_out, RR.oracle_rays(tag, org, T, None, 4)[0], f"{tag}: 4 samples against the oracle")
    # the state is what the definition says: the bits of the colour sum, out = sum / 4
    assert np.array_equal(bits(one_state[:, :3].view(np.float32) / np.float32(4)), bits(one_out))


@pytest.mark.parametrize("tag", ["S2", "M1"])
def test_per_entry_counts_and_first(rt, tag):
    """ns[k] and first[k] per entry, counts 1..5 mixed: a first call of a[k] samples, a second that continues entry k at a[k] by b[k] more."""
    org, T, d = RR.standard_list(tag)
    n = len(org)
    a = (1 + np.arange(n) % 5).astype(np.int32)
    b = (1 + (np.arange(n) // 5) % 4).astype(np.int32)
    PR.init(rt, tag)
    try:
        a_out, a_state, a_rays = rt.radiance_rays(org, d, a, rays=True)
        ab_out, ab_state, b_rays = rt.radiance_rays(org, d, b, first=a, state=a_state, rays=True)
        one_out, one_state, one_rays = rt.radiance_rays(org, d, a + b, rays=True)
    finally:
        rt.cleanupRenderer()
    ref_a, ref_a_rays = RR.oracle_rays(tag, org, T, None, a)
    ref_ab, ref_ab_rays = RR.oracle_rays(tag, org, T, None, a + b)
    same(a_out, ref_a, f"{tag}: per-entry counts against the oracle")
    assert np.array_equal(a_rays, ref_a_rays)
    same(ab_out, ref_ab, f"{tag}: per-entry first and counts against the oracle")
    same(ab_out, one_out, f"{tag}: a + b samples in two calls against one")
    assert np.array_equal(ab_state, one_state) and np.array_equal(a_rays.astype(np.uint64) + b_rays, one_rays) and np.array_equal(one_rays, ref_ab_rays)


# ---- 4. smallest shapes, the refill path (a subprocess each: the switch is read per call) -----------------------------------------

_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import cuda_raytracing_optimized_amd as rt
import pixels_reference as PR
a = json.loads(sys.argv[1])
z = np.load(a["in"])
PR.init(rt, a["tag"])
out, state, rays = rt.radiance_rays(z["org"], z["dir"], a["ns"], ids=z["ids"] if "ids" in z else None, rays=True)
np.savez(a["out"], out=out, rays=rays, ms=rt.last_radiance_ms())
rt.cleanupRenderer()
""" % (ROOT, os.path.join(ROOT, "tests"))


def _in_child(tmp_path, tag, org, d, ids, ns, env):
    arrays = dict(org=org, dir=d) if ids is None else dict(org=org, dir=d, ids=np.asarray(ids, np.uint32))
    np.savez(tmp_path / "in.npz", **arrays)
    args = dict(tag=tag, ns=ns, out=str(tmp_path / "res.npz"))
    args["in"] = str(tmp_path / "in.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(args)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.load(tmp_path / "res.npz")


@pytest.mark.parametrize("case", ["cheapest", "dearest", "n63", "n64", "n65", "waves1_S2", "waves1_M1", "waves3_200"])
def test_smallest_shapes_and_the_refill_path(rt, tmp_path, case):
    tag = "M1" if case == "waves1_M1" else "S2"
    ns, env, ids = _ns(tag), {}, None
    org, T, d = RR.standard_list(tag)
    ref_out, ref_rays, _ = RR.oracle_standard(tag, ns)
    if case in ("cheapest", "dearest"):                     # one ray, one wave, one lane: seed id 0
        k = int(ref_rays.argmin() if case == "cheapest" else ref_rays.argmax())
        sel = slice(k, k + 1)
        ref_out, ref_rays = RR.oracle_rays(tag, org[sel], T[sel], None, ns)
    elif case.startswith("n6"):
        sel = slice(0, int(case[1:]))
        ref_out, ref_rays = ref_out[sel], ref_rays[sel]
    elif case.startswith("waves1"):
        sel, env = slice(0, len(org)), {"RT_PIXELS_WAVES": "1"}
    else:
        sel, env, ids = slice(100, 300), {"RT_PIXELS_WAVES": "3"}, np.arange(100, 300)
        ref_out, ref_rays = ref_out[sel], ref_rays[sel]
    got = _in_child(tmp_path, tag, org[sel], d[sel], ids, ns, env)
    print(case, "entries", len(ref_out), "kernel ms", float(got["ms"]))
    same(got["out"], ref_out, f"{case}: out against the oracle")
    assert np.array_equal(got["rays"], ref_rays)
    assert float(got["ms"]) > 0.0


def test_chunk_crossing(rt):
    """RT_RAY_CHUNK + 65 rays on S1 at one sample - 257 distinct rays of the standard list, repeated in order, ids = NULL: entry k is seeded by k in the
    caller's list, so the second chunk's 65 entries are seeded from RT_RAY_CHUNK on, not from 0.  The 97 entries around the boundary equal a 97-ray call with
    those ids given, which equals the oracle; so does the same list continued by one more sample from the returned states - the buffer that goes up and comes
    down at a chunk's offset."""
    chunk, m = rt.RT_RAY_CHUNK, 257
    n = chunk + 65
    assert chunk == 1 << 22
    org257, T257, d257 = (a[:m] for a in RR.standard_list("S1"))
    idx = np.arange(n) % m
    org, d = np.ascontiguousarray(org257[idx]), np.ascontiguousarray(d257[idx])
    near = np.arange(chunk - 32, chunk + 65)
    PR.init(rt, "S1")
    try:
        out, state, rays = rt.radiance_rays(org, d, 1, rays=True)
        ms = rt.last_radiance_ms()
        out2, state2, rays2 = rt.radiance_rays(org, d, 1, first=np.ones(n, np.int32), state=state, rays=True)
        ms2 = rt.last_radiance_ms()
        ref_out, ref_state, ref_rays = rt.radiance_rays(org[near], d[near], 1, ids=near.astype(np.uint32), rays=True)
        ref2_out, ref2_state, ref2_rays = rt.radiance_rays(org[near], d[near], 1, ids=near.astype(np.uint32), first=np.ones(97, np.int32), state=ref_state,
                                                           rays=True)
    finally:
        rt.cleanupRenderer()
    print("entries", n, "kernel ms", ms, ms2)
    assert ms > 0.0 and ms2 > 0.0
    same(out[near], ref_out, "one sample across the chunk boundary, out")
    assert np.array_equal(state[near], ref_state) and np.array_equal(rays[near], ref_rays)
    same(out2[near], ref2_out, "continued by one sample across the chunk boundary, out")
    assert np.array_equal(state2[near], ref2_state) and np.array_equal(rays2[near], ref2_rays)
    T = T257[idx[near]]
    orc_out, orc_rays = RR.oracle_rays("S1", org[near], T, near, 1)
    orc2_out, orc2_rays = RR.oracle_rays("S1", org[near], T, near, 2)
    same(ref_out, orc_out, "the 97 rays against the oracle")
    same(ref2_out, orc2_out, "the 97 rays continued against the oracle")
    assert np.array_equal(ref_rays, orc_rays) and np.array_equal(ref_rays.astype(np.uint64) + ref2_rays, orc2_rays)
    assert (ref_state[:, 3] != ref2_state[:, 3]).all() and (ref_rays > 0).all() and (state[:, 3] != 0).all()


# ---- 5. independence -------------------------------------------------------------------------------------------------------------

def test_independent_of_partition_counters_and_camera(rt):
    """The same bits under three stripes of 16 rows, as member 1 of 2, with counters on, and after a setCamera."""
    org, _, d = RR.standard_list("S2")
    ref_out, ref_rays, _ = RR.oracle_standard("S2", 4)
    PR.init(rt, "S2")
    try:
        for opts in (dict(stripe_rows=16), dict(part_world=2, part_rank=1), dict(counters=1), dict()):
            rt.setRenderOptions(rt.getDefaultRenderOptions(True), **opts)
            out, _, rays = rt.radiance_rays(org, d, 4, rays=True)
            same(out, ref_out, f"S2 under {opts}")
            assert np.array_equal(rays, ref_rays), opts
        rt.setCamera(rt.make_camera((11, 3, 5), (0, 0.5, 0), (0, 1, 0), 30.0, 64 / 48, 0.1, 10.0))
        out, _, rays = rt.radiance_rays(org, d, 4, rays=True)
        same(out, ref_out, "S2 after setCamera")
        assert np.array_equal(rays, ref_rays)
    finally:
        rt.cleanupRenderer()


def test_follows_update_spheres(rt, O):
    org, T, d = RR.standard_list("S2")
    s = PR.scene(rt, "S2")
    sp2, mt2 = s["sp"].copy(), s["mt"].copy()
    sp2["center"][1:40, 1] += 0.35                          # lift a few dozen spheres, recolour them
    mt2["color"][1:40] = mt2["color"][1:40][:, ::-1]
    PR.init(rt, "S2")
    try:
        rt.update_spheres(sp2, mt2)
        out, _, rays = rt.radiance_rays(org, d, 4, rays=True)
    finally:
        rt.cleanupRenderer()
    ref_out, ref_rays = RR.oracle_rays_in(O.sphere_scene(sp2, mt2), O.default_options(True), s["depth"], org, T, None, 4)
    same(out, ref_out, "after updateSpheres against the oracle of the edited scene")
    assert np.array_equal(rays, ref_rays)
    assert (bits(out) != bits(RR.oracle_standard("S2", 4)[0])).any(axis=1).mean() > 0.02


def test_follows_update_triangles(rt, O):
    """The steel ball of the staircase (mesh id 12) moved by (25, 10, -30), as tests/test_gpu_scene_update.py moves it: the device refits, the rays follow."""
    org, T, d = RR.standard_list("M1")
    nx, ny, depth = PR.SCENES["M1"]
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)                         # (a mesh of this test's own: the cached scene is never edited)
    ks, keep = rt.make_kernel_scene(hm, mats, [])
    rt.initRenderer(ks, rt.staircase_camera(nx, ny), nx, ny, depth, keepalive=keep)
    try:
        real = np.isfinite(hm.tris["v"][:, 0, 0])
        sel = np.flatnonzero(real & (hm.tris["meshID"] == 12))
        first, last = int(sel.min()), int(sel.max())
        new = hm.tris[first:last + 1].copy()
        new["v"][sel - first] = new["v"][sel - first] + np.array([25, 10, -30], np.float32)
        rt.update_triangles(first, new)
        hm.tris[first:last + 1] = new
        hm.refit()
        out, _, rays = rt.radiance_rays(org, d, 3, rays=True)
    finally:
        rt.cleanupRenderer()
    ref_out, ref_rays = RR.oracle_rays_in(O.mesh_scene(hm, mats, []), O.default_options(False), depth, org, T, None, 3)
    same(out, ref_out, "after updateTriangles against the oracle of the edited mesh")
    assert np.array_equal(rays, ref_rays)
    assert (bits(out) != bits(RR.oracle_standard("M1", 3)[0])).any(axis=1).mean() > 0.02


# ---- 6. leaves everything else alone ---------------------------------------------------------------------------------------------

def test_changes_nothing_another_call_observes(rt, O):
    org, _, d = RR.standard_list("S2")
    ij, _ = PR.standard_list("S2")
    fb = PR.init(rt, "S2")
    try:
        rt.runRenderer(8, 8, 8)
        rt.runRenderer(8, 8, 8)                             # (the second frame is ordered by the first one's cost map)
        with_map = [l["phase"] for l in rt.last_launches()]
        rt.renderGuides()
        rt.trace_rays(*rt.centre_rays(PR.scene(rt, "S2")["cam"], 64, 48, ij[:100]))
        rt.render_pixels(ij[:200], 2)
        rt.runRendererProgressive(2, 8, 8)
        seen = lambda: (bits(np.array(fb, copy=True)).tobytes(), stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.last_sphere_form(),
                        rt.progressive_samples(), rt.last_rays_ms(), rt.last_guides_ms(), rt.last_pixels_ms())
        was = seen()
        assert was[4] == 2 and was[5] > 0 and was[6] > 0 and was[7] > 0
        out, _, _ = rt.radiance_rays(org, d, 4)
        assert rt.last_radiance_ms() > 0
        assert seen() == was
        rt.runRendererProgressive(2, 8, 8)                  # the next pass continues the progressive frame as if nothing had happened
        assert rt.progressive_samples() == 4
        same(np.array(fb, copy=True), PR.oracle_frame(rt, O, "S2", 4)[0], "the progressive frame after 2 + 2 samples around a radianceRays call")
        rt.runRenderer(8, 8, 8)                             # ... and the cost map is still the one the frames recorded
        assert [l["phase"] for l in rt.last_launches()] == with_map == [2]
    finally:
        rt.cleanupRenderer()
    same(out, RR.oracle_standard("S2", 4)[0], "the list in between")


# ---- 7. FAST ---------------------------------------------------------------------------------------------------------------------

def _centre_targets(cam, nx, ny):
    """(org, T) float32: the camera's origin and the pixel-centre points of its image plane, row by row from the bottom."""
    v = lambda x: np.array(list(x.e), np.float32)
    jj, ii = np.mgrid[0:ny, 0:nx]
    u = ((ii.ravel().astype(np.float32) + np.float32(0.5)) / np.float32(nx))[:, None]
    w = ((jj.ravel().astype(np.float32) + np.float32(0.5)) / np.float32(ny))[:, None]
    T = (v(cam.lower_left_corner) + u * v(cam.horizontal) + w * v(cam.vertical)).astype(np.float32) + np.float32(0)
    return np.repeat(v(cam.origin)[None] + np.float32(0), nx * ny, axis=0), np.ascontiguousarray(T)


def test_fast_spheres_within_the_fast_frames_tolerance(rt, O):
    """The pixel-centre targets of S2's camera at 96x64 from its origin, 4 samples, FAST objects, against the oracle's rays: the tolerance of
    test_fast_mode_within_tolerance (tests/test_gpu_parity_spheres.py) - at least 97 % of the channels within 1e-4, mean |diff| <= 2e-3, RMSE <= 0.03."""
    nx, ny, ns = 96, 64, 4
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    org, T = _centre_targets(cam, nx, ny)
    ref, _ = RR.oracle_rays_in(O.sphere_scene(sp, mt), O.default_options(True), 50, org, T, None, ns)
    rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    try:
        rt.setRenderOptions(rt.getDefaultRenderOptions(True), fp=rt.RT_FP_FAST)
        got, _, _ = rt.radiance_rays(org, T - org, ns)
    finally:
        rt.cleanupRenderer()
    close = np.abs(got - ref) <= 1e-4
    rmse = float(np.sqrt(((got.astype(np.float64) - ref) ** 2).mean()))
    print("FAST spheres: close", close.mean(), "mean abs", np.abs(got - ref).mean(), "rmse", rmse)
    assert close.mean() >= 0.97
    assert np.abs(got - ref).mean() <= 2e-3
    assert rmse <= 0.03


def test_fast_mesh_within_the_fast_frames_tolerance(rt, O):
    """The pixel-centre targets of the staircase camera at 48x60 from its origin, 4 samples, FAST objects, against the oracle's rays: the tolerance of
    test_mesh_fast_mode_within_tolerance (tests/test_gpu_parity_mesh.py) - at least 90 % of the channels within 1e-3, RMSE <= 0.05."""
    nx, ny, ns = 48, 60, 4
    s = PR.scene(rt, "M1")
    cam = rt.staircase_camera(nx, ny)
    org, T = _centre_targets(cam, nx, ny)
    ref, _ = RR.oracle_rays_in(O.mesh_scene(s["hm"], s["mats"]), O.default_options(False), s["depth"], org, T, None, ns)
    ks, keep = rt.make_kernel_scene(s["hm"], s["mats"])
    rt.initRenderer(ks, cam, nx, ny, s["depth"], keepalive=keep)
    try:
        rt.setRenderOptions(rt.getDefaultRenderOptions(False), fp=rt.RT_FP_FAST)
        got, _, _ = rt.radiance_rays(org, T - org, ns)
    finally:
        rt.cleanupRenderer()
    close = np.abs(got - ref) <= 1e-3
    rmse = float(np.sqrt(((got.astype(np.float64) - ref) ** 2).mean()))
    print("FAST mesh: close", close.mean(), "rmse", rmse)
    assert close.mean() >= 0.90
    assert rmse <= 0.05


# ---- 8. misuse -------------------------------------------------------------------------------------------------------------------

_INIT = ("import sys; sys.path.insert(0, %r); import pixels_reference as PR\n" % os.path.join(ROOT, "tests") +
         "PR.init(rt, 'S2'); r = rt.load_renderer(); org = np.zeros((4, 3), np.float32); d = np.ones((4, 3), np.float32)\n"
         "fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32); out = np.zeros((4, 3), np.float32); st = np.zeros((4, 4), np.uint32)\n"
         "p = lambda a, t: a.ctypes.data_as(t); o = p(out, C.POINTER(rt.vec3)); ones = np.ones(4, np.int32)\n")


@pytest.mark.parametrize("body", [
    "r.radianceRays(-1, p(org, fp), p(d, fp), None, 2, None, None, None, o, None)",                                     # n < 0
    "r.radianceRays(4, None, p(d, fp), None, 2, None, None, None, o, None)",                                            # org NULL
    "r.radianceRays(4, p(org, fp), None, None, 2, None, None, None, o, None)",                                          # dir NULL
    "r.radianceRays(4, p(org, fp), p(d, fp), None, 2, None, None, None, None, None)",                                   # all outputs NULL
    "rt.radiance_rays(org, d, 0)",                                                                                      # c = 0
    "rt.radiance_rays(org, d, np.array([1, 2, 0, 1], np.int32))",                                                       # one c = 0
    "st[:, 3] = 1; rt.radiance_rays(org, d, 2, first=-ones, state=st)",                                                 # f < 0
    "st[:, 3] = 1; rt.radiance_rays(org, d, 65536, first=ones, state=st)",                                              # f + c = 65537
    "rt.radiance_rays(org, d, 65537)",
    "r.radianceRays(4, p(org, fp), p(d, fp), None, 2, None, p(ones, ip), None, o, None)",                               # first without state
    "st[:, 3] = 1; st[2, 3] = 0; rt.radiance_rays(org, d, 2, first=ones, state=st)",                                    # a stream word of 0
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), rng=rt.RT_RNG_COUNTER); rt.radiance_rays(org, d, 2)",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), variant=1); rt.radiance_rays(org, d, 2)",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); rt.radiance_rays(org, d, 2)",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), nee=1); rt.radiance_rays(org, d, 2)",
])
def test_misuse_exits_99(body):
    exits_99(_INIT + body + "\n")


def test_the_largest_total_is_accepted_and_an_empty_list_writes_nothing(rt):
    """f + c = RT_PROGRESSIVE_MAX_SAMPLES passes the check that 65537 fails: 65535 samples of two rays of S1 and then one more, continued from the state the
    first call returned, equal 65536 in one call; n = 0 returns, writes nothing and leaves rtLastRadianceMs as it was."""
    org, _, d = (np.ascontiguousarray(a[:2]) for a in RR.standard_list("S1"))
    PR.init(rt, "S1")
    try:
        r = rt.load_renderer()
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        out = np.full((2, 3), 7.0, np.float32)
        state = np.full((2, 4), 9, np.uint32)
        rays = np.full(2, 5, np.uint32)
        rt.radiance_rays(org, d, 1)
        before = rt.last_radiance_ms()
        assert before > 0.0
        r.radianceRays(0, org.ctypes.data_as(fp), d.ctypes.data_as(fp), None, 2, None, None, state.ctypes.data_as(up), out.ctypes.data_as(C.POINTER(rt.vec3)),
                       rays.ctypes.data_as(up))
        assert (out == 7.0).all() and (state == 9).all() and (rays == 5).all() and rt.last_radiance_ms() == before
        one, one_state, _ = rt.radiance_rays(org, d, 65536)
        _, st, _ = rt.radiance_rays(org, d, 65535)
        got, got_state, _ = rt.radiance_rays(org, d, 1, first=np.full(2, 65535, np.int32), state=st)
    finally:
        rt.cleanupRenderer()
    same(got, one, "65535 + 1 samples against 65536 in one call")
    assert np.array_equal(got_state, one_state) and (got_state[:, 3] != 0).all()
