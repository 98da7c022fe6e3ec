"""CPU checks of refineFrame (include/rt_api.h): the five calls are declared, exported and bound with their argument types, the constants agree between
header and Python, the ABI version and struct sizes are the parent's, every call before init is the library's misuse exit, the binding refuses wrong
arguments, and the test reference (tests/refine_reference.py) shows on the parameters of the GPU tests what they are there to cover, so that none of them
can pass vacuously - conditions on the reference alone, no tolerance.

The thresholds of refine_reference.CASES were chosen here, on the CPU oracle, from the candidates 0.02 .. 0.2 (S2), 0.1 .. 0.8 (M1), 0.005 .. 0.1 (S1_13x5),
as the first under which every condition below holds with RT_REFINE_DILATE off and on.  Observed (share of the pixels pass 3 samples, off / on; the values
of the final samples plane, off / on; pixels whose final count differs between off and on):
  S2       batch 2, min_batches 2, max 12, threshold 0.1:  0.334 / 0.681;  {4, 6, 8, 10, 12} both;    1358 of 3072
  M1       batch 2, min_batches 2, max 8,  threshold 0.8:  0.135 / 0.596;  {4, 6, 8} both;             783 of 1536
  S1_13x5  batch 2, min_batches 2, max 10, threshold 0.1:  0.108 / 0.631;  {4, 6, 8, 10} both;          34 of 65
  S1_523x503  batch 2, min_batches 2, max 8, threshold 0.0003:  0.558 / 0.821;  {4, 6, 8} both;  73531 of 263069  (chosen by tests/test_capped_grids_api.py)
A pass that stops early with dilation on starts again later (S2: 11 calls instead of 7): a neighbour's new samples can move its error above the threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import refine_reference as RR
from preview_support import exits_99

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
NEW = ("refineFrame", "rtResetRefine", "rtRefineSamples", "rtRefineLastList", "rtLastRefineMs")


def test_declared_exported_and_bound(rt):
    assert re.search(r"int\s+refineFrame\s*\(\s*rt_vec3\s*\*\s*out\s*,\s*int32_t\s*\*\s*samples\s*,\s*float\s*\*\s*error\s*,\s*int\s+batch\s*,\s*int\s+min_batches\s*,"
                     r"\s*int\s+max_samples\s*,\s*float\s+threshold\s*,\s*int\s+flags\s*\)\s*;", API)
    assert re.search(r"void\s+rtResetRefine\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"long long\s+rtRefineSamples\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"int\s+rtRefineLastList\s*\(\s*int32_t\s*\*\s*ij\s*,\s*int\s+cap\s*\)\s*;", API)
    assert re.search(r"double\s+rtLastRefineMs\s*\(\s*void\s*\)\s*;", API)
    assert API.index("double rtLastPixelsMs") < API.index("refineFrame(rt_vec3* out") < API.index("--- editing the scene")       # the section's place
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    r = rt.load_renderer()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    assert r.refineFrame.argtypes == [C.POINTER(rt.vec3), ip, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int] and r.refineFrame.restype is C.c_int
    assert r.rtResetRefine.argtypes == [] and r.rtResetRefine.restype is None
    assert r.rtRefineSamples.argtypes == [] and r.rtRefineSamples.restype is C.c_longlong
    assert r.rtRefineLastList.argtypes == [ip, C.c_int] and r.rtRefineLastList.restype is C.c_int
    assert r.rtLastRefineMs.argtypes == [] and r.rtLastRefineMs.restype is C.c_double
    for name in ("refine_frame", "reset_refine", "refine_samples", "refine_last_list", "last_refine_ms"):
        assert callable(getattr(rt, name)), name


def test_constants_agree_between_header_and_python(rt):
    assert re.search(r"^enum \{ RT_REFINE_DILATE = 1 \};$", API, re.M) and rt.RT_REFINE_DILATE == 1 == RR.DILATE
    assert re.search(r"^#define RT_REFINE_LUM_EPS 1e-3f$", API, re.M)
    assert np.float32(rt.RT_REFINE_LUM_EPS) == RR.LUM_EPS == np.float32(1e-3)


def test_abi_unchanged(rt):
    assert rt.load_renderer().rtApiVersion() == 1002 == rt.RT_API_VERSION
    assert re.search(r"#define RT_API_VERSION 1002\b", API)
    sizes = (C.c_int32 * 32)()
    n = rt.load_renderer().rtStructSizes(sizes, 32)
    assert n == 13 and [sizes[k] for k in range(n)] == [C.sizeof(s) for s in rt.ABI_STRUCTS]


@pytest.mark.parametrize("call", ["rt.load_renderer().refineFrame(None, None, None, 2, 2, 8, 0.1, 0)", "rt.reset_refine()", "rt.refine_samples()",
                                  "rt.refine_last_list()", "rt.last_refine_ms()"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99(call + "\n")


def test_the_binding_refuses_wrong_arguments(rt):
    for args, kw in (((2.0, 2, 8, 0.1), {}), ((2, 2.5, 8, 0.1), {}), ((2, 2, "8", 0.1), {}), ((2, 2, 8, "0.1"), {}), ((2, 2, 8, None), {}),
                     ((True, 2, 8, 0.1), {}), ((2, 2, 8, 0.1), dict(flags=1.0)), ((2, 2, 8, 0.1), dict(want=("out", "variance"))),
                     ((2, 2, 8, 0.1), dict(want="mean"))):
        with pytest.raises(ValueError):
            rt.refine_frame(*args, **kw)


# ---- the parameters of the GPU tests: conditions, from the reference alone ---------------------------------------------------------

@pytest.mark.parametrize("tag", sorted(RR.CASES))
def test_the_cases_exercise_selection_cap_and_dilation(rt, O, tag):
    nx, ny = RR.size(tag)
    batch, min_batches, max_samples, threshold = RR.CASES[tag]
    final = {}
    for flags in (0, RR.DILATE):
        calls = RR.run(rt, O, tag, flags)
        share3 = calls[2][0] / (nx * ny)
        values = np.unique(calls[-1][2]).tolist()
        print(tag, "threshold", threshold, "dilate", flags, "calls", len(calls), "share of pass 3", round(share3, 3), "final samples", values)
        assert calls[0][0] == calls[1][0] == nx * ny                   # min_batches = 2: the first two passes sample every pixel
        assert 0.10 <= share3 <= 0.90
        assert len(values) >= 3 and values[0] == min_batches * batch and values[-1] == max_samples     # converged early, and stopped by the cap
        assert calls[-1][0] == 0 and all(c[0] > 0 for c in calls[:-1])
        assert all(c[0] == int(c[4].sum()) for c in calls)
        before = np.zeros((ny, nx), np.int32)
        for c in calls:                                                 # a pass adds one batch to its active pixels and nothing elsewhere
            assert np.array_equal(c[2] - before, np.where(c[4], batch, 0))
            before = c[2]
        final[flags] = calls[-1][2]
    differ = int((final[0] != final[RR.DILATE]).sum())
    print(tag, "pixels whose final count differs between dilation off and on", differ)
    assert differ > 0 and (final[RR.DILATE] >= final[0]).mean() > 0.9


def test_the_small_image_clips_every_window_and_is_one_wave_plus_one():
    nx, ny = RR.size("S1_13x5")
    assert nx * ny == 65
    m = np.zeros((ny, nx), bool)
    m[0, 0] = m[ny - 1, nx - 1] = True
    d = RR.dilate(m)
    assert int(d.sum()) == 8 and d[:2, :2].all() and d[-2:, -2:].all()             # the corners' windows are 2 x 2


def test_a_pixel_without_a_finite_mean_never_converges_and_stops_at_the_cap():
    """The reference on synthetic frames: a constant image (its error is exactly 0) with one NaN and one +inf pixel."""
    def frames(n):
        f = np.full((4, 6, 3), 0.5, np.float32)
        f[1, 2] = np.nan
        f[2, 4, 1] = np.inf
        return f
    f = RR.Frame(None, None, None, 2, frames=frames, shape=(4, 6))
    calls = []
    while not calls or calls[-1][0]:
        calls.append(f.call(2, 10, 1.0))
    assert [c[0] for c in calls] == [24, 24, 2, 2, 2, 0]
    n, err = calls[-1][2], calls[-1][3]
    assert n[1, 2] == n[2, 4] == 10 and (np.delete(n.ravel(), [1 * 6 + 2, 2 * 6 + 4]) == 4).all()
    assert np.isnan(err[1, 2]) and np.isnan(err[2, 4]) and (np.delete(err.ravel(), [8, 16]) == 0).all()


def test_raising_the_cap_after_a_zero_return_continues_the_frame(rt, O):
    """What the GPU test of late parameter changes relies on: under S2's parameters with max_samples 6 the frame finishes, and 12 starts it again."""
    batch, min_batches, _, threshold = RR.CASES["S2"]
    f = RR.Frame(rt, O, "S2", batch)
    counts = []
    while not counts or counts[-1]:
        counts.append(f.call(min_batches, 6, threshold)[0])
    assert len(counts) == 4 and counts[2] > 0
    assert f.call(min_batches, 12, threshold)[0] > 0
