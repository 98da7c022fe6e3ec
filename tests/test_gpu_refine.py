"""GPU checks of refineFrame (include/rt_api.h) against its numpy reference over the CPU oracle's frames (tests/refine_reference.py) and against frames rendered
in the same process: bit for bit in PARITY mode after every call - the planes, the return value, the sample total, the list of a pass and its cost order,
delivery on demand, parameters that change between calls, every reset, the smallest image and a single wave, independence of the partition - nothing another
call observes changes, the FAST objects within the tolerance tests/test_gpu_pixels.py states for FAST lists, and misuse is the library's exit 99.
tests/test_refine_api.py shows on the reference alone that the parameters used here exercise the selection, the cap and the dilation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pixels_reference as PR
import refine_reference as RR
from preview_support import bits, exits_99, same, stats_tuple

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DILATE = RR.DILATE


def _check_call(got, ref, what):
    sampled, out, samples, error = got
    assert sampled == ref[0], (what, sampled, ref[0])
    assert np.array_equal(samples, ref[2]), (what, int((samples != ref[2]).sum()))
    same(error, ref[3], f"{what}: error")
    same(out, ref[1], f"{what}: out")


# ---- 1. to completion, every call ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,flags", [("S2", 0), ("S2", DILATE), ("M1", 0), ("M1", DILATE), ("S1_13x5", 0), ("S1_13x5", DILATE)])
def test_to_completion_every_call(rt, O, tag, flags):
    batch, min_batches, max_samples, threshold = RR.CASES[tag]
    ref = RR.run(rt, O, tag, flags)
    fb = RR.init(rt, tag)
    try:
        assert rt.refine_samples() == 0 and rt.last_refine_ms() == 0.0 and len(rt.refine_last_list()) == 0
        got, totals = [], []
        for _ in ref:
            got.append(rt.refine_frame(batch, min_batches, max_samples, threshold, flags))
            totals.append(rt.refine_samples())
            assert rt.last_refine_ms() > 0.0 and len(rt.refine_last_list()) == got[-1][0]
        further = rt.refine_frame(batch, min_batches, max_samples, threshold, flags)
        total_after = rt.refine_samples()
        frames = {}
        for n in np.unique(got[-1][2]).tolist():
            rt.runRenderer(n, 8, 8)
            frames[n] = np.array(fb, copy=True)
    finally:
        rt.cleanupRenderer()
    print(tag, "dilate", flags, "sampled per call", [g[0] for g in got])
    traced = 0
    for k, (g, r) in enumerate(zip(got, ref)):
        _check_call(g, r, f"{tag} dilate {flags} call {k + 1}")
        traced += r[0] * batch
        assert totals[k] == traced
    assert got[-1][0] == 0 and further[0] == 0 and total_after == traced
    for a, b in zip(further[1:], got[-1][1:]):
        assert np.array_equal(bits(a), bits(b))
    out, samples = got[-1][1], got[-1][2]
    for n, frame in frames.items():
        m = samples == n
        same(out[m], frame[m], f"{tag}: the pixels that stopped at {n} samples against runRenderer({n})")
        same(out[m], RR.oracle_frame(rt, O, tag, n)[m], f"{tag}: ... and against the oracle")


# ---- 2. smallest shapes: a single wave (a subprocess each: the switch is read per call) -------------------------------------------

_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import cuda_raytracing_optimized_amd as rt
import refine_reference as RR
a = json.loads(sys.argv[1])
RR.init(rt, a["tag"])
res = {}
for k in range(a["calls"]):
    sampled, out, samples, error = rt.refine_frame(*a["params"], a["flags"])
    res.update({"sampled%%d" %% k: sampled, "out%%d" %% k: out, "samples%%d" %% k: samples, "error%%d" %% k: error})
np.savez(a["out"], total=rt.refine_samples(), **res)
rt.cleanupRenderer()
""" % (ROOT, os.path.join(ROOT, "tests"))


@pytest.mark.parametrize("tag,flags", [("S1_13x5", DILATE), ("M1", DILATE), ("S2", 0)])
def test_one_wave_gives_the_same_bits(rt, O, tmp_path, tag, flags):
    ref = RR.run(rt, O, tag, flags)
    args = dict(tag=tag, flags=flags, params=list(RR.CASES[tag]), calls=len(ref), out=str(tmp_path / "res.npz"))
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(args)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, RT_PIXELS_WAVES="1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.load(tmp_path / "res.npz")
    for k, c in enumerate(ref):
        _check_call((int(got[f"sampled{k}"]), got[f"out{k}"], got[f"samples{k}"], got[f"error{k}"]), c, f"{tag} through one wave, call {k + 1}")
    assert int(got["total"]) == sum(c[0] for c in ref) * RR.CASES[tag][0]


# ---- 3. the list and its order ---------------------------------------------------------------------------------------------------

_classes = RR.classes           # 31 - clz(max(rays, 1))


def test_the_list_is_the_active_set_in_cost_order(rt, O):
    batch, min_batches, max_samples, threshold = RR.CASES["S2"]
    nx, ny = RR.size("S2")
    ref = RR.run(rt, O, "S2", 0)
    rays2, rays4 = PR.oracle_planes(rt, O, "S2", 2)[1], PR.oracle_planes(rt, O, "S2", 4)[1]
    last_batch = {1: np.zeros_like(rays2), 2: rays2, 3: rays4 - rays2}                       # the rays of a pixel's last batch before pass 1, 2, 3
    RR.init(rt, "S2")
    try:
        lists = {}
        for k in (1, 2, 3):
            sampled = rt.refine_frame(batch, min_batches, max_samples, threshold, 0, want=())[0]
            lists[k] = rt.refine_last_list()
            assert len(lists[k]) == sampled == ref[k - 1][0]
    finally:
        rt.cleanupRenderer()
    for k in (1, 2, 3):
        ij = lists[k]
        ids = ij[:, 1].astype(np.int64) * nx + ij[:, 0]
        assert np.array_equal(np.sort(ids), np.flatnonzero(ref[k - 1][4].ravel())), f"pass {k}: the list is not the reference's active set"
        cls = _classes(last_batch[k][ij[:, 1], ij[:, 0]])
        print("pass", k, "entries", len(ij), "classes", np.unique(cls).tolist())
        assert (np.diff(cls) <= 0).all(), f"pass {k}: the classes increase somewhere"
        if k > 1:
            assert len(np.unique(cls)) >= 3


# ---- 4. delivery and late parameter changes --------------------------------------------------------------------------------------

def test_delivery_on_demand_equals_delivering_every_call(rt, O):
    batch, min_batches, max_samples, threshold = RR.CASES["S2"]
    ref = RR.run(rt, O, "S2", DILATE)
    RR.init(rt, "S2")
    try:
        quiet = [rt.refine_frame(batch, min_batches, max_samples, threshold, DILATE, want=()) for _ in range(4)]
        fifth = rt.refine_frame(batch, min_batches, max_samples, threshold, DILATE)
        only_samples = rt.refine_frame(batch, min_batches, max_samples, threshold, DILATE, want="samples")
    finally:
        rt.cleanupRenderer()
    assert [q[0] for q in quiet] == [c[0] for c in ref[:4]] and all(q[1] is None and q[2] is None and q[3] is None for q in quiet)
    _check_call(fifth, ref[4], "S2: four calls without planes, then one with")
    assert only_samples[0] == ref[5][0] and only_samples[1] is None and only_samples[3] is None and np.array_equal(only_samples[2], ref[5][2])


def test_parameters_that_change_between_calls_follow_the_reference(rt, O):
    """The threshold lowered and raised, min_batches raised, dilation switched, and max_samples raised after a 0 return."""
    batch = RR.CASES["S2"][0]
    #        min_batches, max_samples, threshold, flags
    plan = [(2, 6, 0.1, 0), (2, 6, 0.1, 0), (2, 6, 0.02, 0), (2, 6, 0.02, 0), (2, 12, 0.02, 0), (2, 12, 0.5, DILATE), (4, 12, 0.5, 0), (2, 12, 0.05, DILATE),
            (2, 12, 0.05, DILATE), (2, 12, 1.0, 0), (2, 14, 0.0, 0)]
    f = RR.Frame(rt, O, "S2", batch)
    ref = [f.call(*p) for p in plan]
    assert ref[3][0] == 0 and ref[4][0] > 0 and ref[9][0] == 0 and ref[10][0] > 0 and all(r[0] > 0 for k, r in enumerate(ref) if k not in (3, 9))
    RR.init(rt, "S2")
    try:
        got = [rt.refine_frame(batch, *p) for p in plan]
        total = rt.refine_samples()
    finally:
        rt.cleanupRenderer()
    print("sampled per call", [g[0] for g in got])
    for k, (g, r) in enumerate(zip(got, ref)):
        _check_call(g, r, f"S2 plan call {k + 1} {plan[k]}")
    assert total == f.total


# ---- 5. resets -------------------------------------------------------------------------------------------------------------------

def _fresh(rt, ref, params, what):
    """The next two calls are the first two of a frame."""
    for k in (0, 1):
        _check_call(rt.refine_frame(*params), ref[k], f"{what}: call {k + 1} of the new frame")
    assert rt.refine_samples() == (ref[0][0] + ref[1][0]) * params[0]


def test_every_reset_starts_a_fresh_frame(rt, O):
    params = RR.CASES["S2"]
    ref = RR.run(rt, O, "S2", 0)
    s = PR.scene(rt, "S2")
    RR.init(rt, "S2")
    try:
        for what, reset in (("setCamera", lambda: rt.setCamera(s["cam"])),
                            ("setRenderOptions", lambda: rt.setRenderOptions(rt.getDefaultRenderOptions(True))),
                            ("updateSpheres", lambda: rt.update_spheres(s["sp"], s["mt"])),
                            ("rtResetRefine", rt.reset_refine),
                            ("re-init", lambda: RR.init(rt, "S2"))):
            for _ in range(3):
                rt.refine_frame(*params, want=())
            assert rt.refine_samples() > 0
            reset()
            assert rt.refine_samples() == 0 and len(rt.refine_last_list()) == 0, what
            _fresh(rt, ref, params, what)
        # a new frame may take another batch; the old one may not (test_misuse_exits_99)
        rt.reset_refine()
        assert rt.refine_frame(3, 2, 12, 0.1, want=())[0] == s["nx"] * s["ny"] and rt.refine_samples() == 3 * s["nx"] * s["ny"]
    finally:
        rt.cleanupRenderer()


def test_mesh_edits_start_a_fresh_frame(rt, O):
    params = RR.CASES["M1"]
    ref = RR.run(rt, O, "M1", 0)
    s = PR.scene(rt, "M1")
    RR.init(rt, "M1")
    try:
        for what, reset in (("updateTriangles", lambda: rt.update_triangles(0, np.array(s["hm"].tris[:4], copy=True))),
                            ("updateMaterials", lambda: rt.update_materials(s["mats"]))):
            for _ in range(3):
                rt.refine_frame(*params, want=())
            reset()
            assert rt.refine_samples() == 0, what
            _fresh(rt, ref, params, what)
    finally:
        rt.cleanupRenderer()


# ---- 6. leaves everything else alone ---------------------------------------------------------------------------------------------

def test_changes_nothing_another_call_observes(rt, O):
    params = RR.CASES["S2"]
    ref = RR.run(rt, O, "S2", 0)
    ij, _ = PR.standard_list("S2")
    fb = PR.init(rt, "S2")
    try:
        rt.runRenderer(8, 8, 8)
        rt.runRenderer(8, 8, 8)                             # (the second frame is ordered by the first one's cost map)
        with_map = [l["phase"] for l in rt.last_launches()]
        rt.renderGuides()
        rt.trace_rays(*rt.centre_rays(PR.scene(rt, "S2")["cam"], 64, 48, ij[:100]))
        rt.render_pixels(ij, 2)
        rt.accumulateFrame()
        rt.previewFrame()
        rt.denoiseFrame()
        rt.display_frame()
        rt.runRendererProgressive(2, 8, 8)
        seen = lambda: (bits(np.array(fb, copy=True)).tobytes(), stats_tuple(rt.getRenderStats()), rt.last_launches(), rt.last_sphere_form(),
                        rt.progressive_samples(), rt.history_frames(), rt.preview_frames(), rt.last_exposure(), rt.last_rays_ms(), rt.last_guides_ms(),
                        rt.last_pixels_ms(), rt.last_accumulate_ms(), rt.last_preview_ms(), rt.last_denoise_ms(), rt.last_display_ms())
        was = seen()
        assert was[4] == 2 and was[5] == 1 and was[6] == 1 and all(ms > 0 for ms in was[8:])
        got = [rt.refine_frame(*params) for _ in range(3)]
        assert rt.last_refine_ms() > 0 and seen() == was
        rt.refine_last_list()
        rt.reset_refine()
        assert seen() == was
        rt.runRendererProgressive(2, 8, 8)                  # the next pass continues the progressive frame as if nothing had happened
        assert rt.progressive_samples() == 4
        same(np.array(fb, copy=True), PR.oracle_frame(rt, O, "S2", 4)[0], "the progressive frame after 2 + 2 samples around three refineFrame calls")
        rt.runRenderer(8, 8, 8)                             # ... and the cost map is still the one the frames recorded
        assert [l["phase"] for l in rt.last_launches()] == with_map == [2]
    finally:
        rt.cleanupRenderer()
    for k in range(3):
        _check_call(got[k], ref[k], f"the adaptive frame in between, call {k + 1}")


# ---- 7. partition ----------------------------------------------------------------------------------------------------------------

def test_independent_of_the_partition(rt, O):
    params = RR.CASES["S2"]
    ref = RR.run(rt, O, "S2", DILATE)
    PR.init(rt, "S2")
    try:
        for opts in (dict(stripe_rows=16), dict(part_world=2, part_rank=1), dict(stripe_rows=24, part_world=3, part_rank=2)):
            rt.setRenderOptions(rt.getDefaultRenderOptions(True), **opts)
            for k in range(4):
                _check_call(rt.refine_frame(*params, DILATE), ref[k], f"S2 under {opts}, call {k + 1}")
    finally:
        rt.cleanupRenderer()


# ---- 8. FAST ---------------------------------------------------------------------------------------------------------------------

def _to_completion(rt, params, flags, limit=64):
    calls = 0
    while rt.refine_frame(*params, flags, want=())[0]:
        calls += 1
        assert calls < limit
    return rt.refine_frame(*params, flags)


def _oracle_at(samples, frame_at):
    ref = np.zeros(samples.shape + (3,), np.float32)
    for n in np.unique(samples).tolist():
        ref[samples == n] = frame_at(n)[samples == n]
    return ref


def test_fast_spheres_within_the_fast_lists_tolerance(rt, O):
    """S2's scene at 300x200, the configuration and the tolerance of test_fast_spheres_within_the_fast_frames_tolerance (tests/test_gpu_pixels.py): at least
    97 % of the channels within 1e-4 of the oracle at the reported samples(p), mean |diff| <= 2e-3, RMSE <= 0.03.  The samples plane is not compared."""
    nx, ny = 300, 200
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    try:
        rt.setRenderOptions(rt.getDefaultRenderOptions(True), fp=rt.RT_FP_FAST)
        sampled, got, samples, error = _to_completion(rt, (2, 2, 8, 0.1), DILATE)
    finally:
        rt.cleanupRenderer()
    assert sampled == 0 and samples.min() >= 4 and samples.max() <= 8 and (samples % 2 == 0).all()
    ref = _oracle_at(samples, lambda n: O.render(O.sphere_scene(sp, mt), cam, O.default_options(True), nx, ny, n, 50)[0])
    close = np.abs(got - ref) <= 1e-4
    print("FAST spheres: samples", np.unique(samples, return_counts=True), "close", close.mean(), "mean abs", np.abs(got - ref).mean(), "rmse", rt.rmse(got, ref))
    assert close.mean() >= 0.97
    assert np.abs(got - ref).mean() <= 2e-3
    assert rt.rmse(got, ref) <= 0.03


def test_fast_mesh_within_the_fast_lists_tolerance(rt, O):
    """The staircase at 96x120, depth 64, the configuration and the tolerance of test_fast_mesh_within_the_fast_frames_tolerance (tests/test_gpu_pixels.py): at
    least 90 % of the channels within 1e-3 of the oracle at the reported samples(p), RMSE <= 0.05."""
    nx, ny = 96, 120
    s = PR.scene(rt, "M1")
    cam = rt.staircase_camera(nx, ny)
    ks, keep = rt.make_kernel_scene(s["hm"], s["mats"])
    rt.initRenderer(ks, cam, nx, ny, 64, keepalive=keep)
    try:
        rt.setRenderOptions(rt.getDefaultRenderOptions(False), fp=rt.RT_FP_FAST)
        sampled, got, samples, error = _to_completion(rt, (2, 2, 8, 0.8), 0)
    finally:
        rt.cleanupRenderer()
    assert sampled == 0 and samples.min() >= 4 and samples.max() <= 8 and (samples % 2 == 0).all()
    ref = _oracle_at(samples, lambda n: O.render(O.mesh_scene(s["hm"], s["mats"]), cam, O.default_options(False), nx, ny, n, 64)[0])
    close = np.abs(got - ref) <= 1e-3
    print("FAST mesh: samples", np.unique(samples, return_counts=True), "close", close.mean(), "rmse", rt.rmse(got, ref))
    assert close.mean() >= 0.90
    assert rt.rmse(got, ref) <= 0.05


# ---- 9. misuse -------------------------------------------------------------------------------------------------------------------

_INIT = ("import sys; sys.path.insert(0, %r); import pixels_reference as PR\n" % os.path.join(ROOT, "tests") +
         "PR.init(rt, 'S2'); r = rt.load_renderer()\n")


@pytest.mark.parametrize("body", [
    "rt.refine_frame(0, 2, 8, 0.1)",                                                                                # batch < 1
    "rt.refine_frame(2, 1, 8, 0.1)",                                                                                # min_batches < 2
    "rt.refine_frame(4, 2, 3, 0.1)",                                                                                # max_samples < batch
    "rt.refine_frame(2, 2, 65537, 0.1)",                                                                            # above RT_PROGRESSIVE_MAX_SAMPLES
    "rt.refine_frame(2, 2, 8, float('nan'))",
    "rt.refine_frame(2, 2, 8, float('inf'))",
    "rt.refine_frame(2, 2, 8, -0.5)",
    "rt.refine_frame(2, 2, 8, 0.1, flags=2)",                                                                       # unknown flag bits
    "rt.refine_frame(2, 2, 8, 0.1, want=()); rt.refine_frame(4, 2, 8, 0.1)",                                        # another batch than the frame's
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), rng=rt.RT_RNG_COUNTER); rt.refine_frame(2, 2, 8, 0.1)",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), variant=1); rt.refine_frame(2, 2, 8, 0.1)",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), floor=1); rt.refine_frame(2, 2, 8, 0.1)",
    "rt.setRenderOptions(rt.getDefaultRenderOptions(True), nee=1); rt.refine_frame(2, 2, 8, 0.1)",
    "rt.cleanupRenderer(); rt.refine_frame(2, 2, 8, 0.1)",
])
def test_misuse_exits_99(body):
    exits_99(_INIT + body + "\n")


def test_the_limits_of_the_arguments_are_accepted(rt, O):
    """batch = max_samples (one pass, then the cap), threshold 0 (a pixel converges only where its batch means are equal), max_samples =
    RT_PROGRESSIVE_MAX_SAMPLES as a cap that is not reached."""
    f = RR.Frame(rt, O, "S1_13x5", 2)
    ref = [f.call(2, 65536, 0.0) for _ in range(3)] + [f.call(2, 6, 0.0)]
    RR.init(rt, "S1_13x5")
    try:
        assert rt.refine_frame(3, 2, 3, 0.0, want=())[0] == 65 and rt.refine_frame(3, 2, 3, 0.0, want=())[0] == 0
        rt.reset_refine()
        got = [rt.refine_frame(2, 2, 65536, 0.0) for _ in range(3)] + [rt.refine_frame(2, 2, 6, 0.0)]
    finally:
        rt.cleanupRenderer()
    assert ref[2][0] > 32 and ref[3][0] == 0
    for k in range(4):
        _check_call(got[k], ref[k], f"S1_13x5 threshold 0, call {k + 1}")
