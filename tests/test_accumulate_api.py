"""CPU checks of the temporal accumulation's interface (include/rt_api.h): accumulateFrame / rtResetHistory / rtHistoryFrames / rtLastAccumulateMs are declared,
exported and bound, the constants agree between header and Python, the ABI version and the struct sizes are the parent's, a call before init is the library's
misuse exit, the new translation unit is built once with the denoiser's flags; and, from the test reference alone (tests/accumulate_reference.py): its
vectorisation agrees bit for bit with a per-pixel scalar restatement, the sequences of the GPU tests exercise every way a tap and a pixel can be rejected, and
accumulation over a camera move reduces the error of 1 spp frames."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import accumulate_reference as A
import denoise_reference as D
import guides_reference as R
from preview_support import bits as _bits, exits_99, oracle_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
NEW = ("accumulateFrame", "rtResetHistory", "rtHistoryFrames", "rtLastAccumulateMs")


def test_declared_exported_and_bound(rt):
    assert re.search(r"void\s+accumulateFrame\s*\(\s*const\s+rt_vec3\s*\*\s*in\s*,\s*rt_vec3\s*\*\s*out\s*,\s*float\s*\*\s*history\s*,\s*int\s+flags\s*,"
                     r"\s*int\s+max_history\s*,\s*float\s+sigma_z\s*,\s*float\s+normal_min\s*\)\s*;", API)
    assert re.search(r"void\s+rtResetHistory\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"int\s+rtHistoryFrames\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"double\s+rtLastAccumulateMs\s*\(\s*void\s*\)\s*;", API)
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    r = rt.load_renderer()
    assert r.accumulateFrame.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float] and r.accumulateFrame.restype is None
    assert r.rtResetHistory.argtypes == [] and r.rtResetHistory.restype is None
    assert r.rtHistoryFrames.argtypes == [] and r.rtHistoryFrames.restype is C.c_int
    assert r.rtLastAccumulateMs.argtypes == [] and r.rtLastAccumulateMs.restype is C.c_double
    assert callable(rt.accumulateFrame) and callable(rt.reset_history) and callable(rt.history_frames) and callable(rt.last_accumulate_ms)
    assert r.rtLastAccumulateMs() == 0.0                        # before the first call; no device is touched


def test_constants_agree_between_header_and_python(rt):
    assert dict(re.findall(r"#define\s+(RT_ACCUM_[A-Z_]+)\s+(\d+)\b", API)) == {"RT_ACCUM_MAX_HISTORY": "1024"}
    assert rt.RT_ACCUM_MAX_HISTORY == 1024
    assert (A.DEMODULATE, A.SAME_PRIM) == (rt.RT_DENOISE_DEMODULATE, rt.RT_DENOISE_SAME_PRIM)
    assert np.float32(rt.RT_DENOISE_ALBEDO_FLOOR) == A.ALBEDO_FLOOR
    sig = inspect.signature(rt.accumulateFrame).parameters
    assert list(sig) == ["fb", "out", "history", "flags", "max_history", "sigma_z", "normal_min"]
    assert [sig[k].default for k in sig] == [None, None, False, None, 32, 0.01, 0.9]
    assert A.DEFAULTS == dict(max_history=32, sigma_z=0.01, normal_min=0.9)


def test_abi_unchanged(rt):
    assert rt.load_renderer().rtApiVersion() == 1002 == rt.RT_API_VERSION
    assert re.search(r"#define RT_API_VERSION 1002\b", API)
    sizes = (C.c_int32 * 32)()
    n = rt.load_renderer().rtStructSizes(sizes, 32)
    assert n == 13 and [sizes[k] for k in range(n)] == [C.sizeof(s) for s in rt.ABI_STRUCTS]


@pytest.mark.parametrize("call", ["rt.accumulateFrame(np.zeros((4, 4, 3), np.float32), flags=3)",
                                  "a = np.zeros((4, 4, 3), np.float32); rt.load_renderer().accumulateFrame(a.ctypes.data, a.ctypes.data, None, 3, 32, 0.01, 0.9)",
                                  "rt.reset_history()", "rt.history_frames()"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99("rt._state.update(nx=4, ny=4)\n%s\n" % call)


def test_translation_unit_is_built_once_with_the_denoiser_s_flags():
    """One arithmetic, defined bit for bit: one object, compiled like denoise.o and appended to RT_OBJS; renderer.o depends on the new header and no other
    kernel file sees it; the kernel names keep away from the strings the production-form tripwires scan for."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    rules = re.findall(r"^\$\(OBJ\)/(\S+)\.o:\s*\$\(CSRC\)/rt_kernels_accumulate\.hip([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert len(rules) == 1 and rules[0][0] == "accumulate", rules
    assert "$(CSRC)/rt_accumulate.h" in rules[0][1].split()
    line = rules[0][2]
    for flag in ("-ffp-contract=off", "-fno-slp-vectorize", "-fno-vectorize"):
        assert flag in line.split(), (flag, line)
    assert "-fno-hip-fp32-correctly-rounded-divide-sqrt" not in line and "-ffast-math" not in line and "-fgpu-flush-denormals-to-zero" not in line
    assert "RT_MODE_" not in line
    denoise = re.search(r"^\$\(OBJ\)/denoise\.o:[^\n]*\n\t([^\n]+)", mk, re.M).group(1)
    assert line.split()[:-4] == denoise.split()[:-4]            # the same command up to `-c $< -o $@`
    assert re.search(r"^RT_OBJS\s*:=.*\$\(OBJ\)/denoise\.o \$\(OBJ\)/accumulate\.o\s*$", mk, re.M)
    renderer = re.search(r"^\$\(OBJ\)/renderer\.o:([^\n]*)", mk, re.M).group(1)
    assert "$(CSRC)/rt_accumulate.h" in renderer.split()
    csrc = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")
    for name in ("rt_kernels_spheres.hip", "rt_kernels_mesh.hip", "rt_probe.hip", "rt_params.h", "rt_device.h", "rt_kernels_denoise.hip", "rt_denoise.h"):
        assert "rt_accumulate" not in open(os.path.join(csrc, name)).read().lower(), name
    src = open(os.path.join(csrc, "rt_kernels_accumulate.hip")).read()
    for scanned in ("launch_mesh_queue<", "k_render_mesh<", "k_render_spheres_tiles<", "launch_queue_form", "launch_kind_of", "launch_with_lds", "k_render_spheres_queue<", "k_render_mesh_queue<"):
        assert scanned not in src, scanned
    assert "fmaf" not in src and "__fmaf" not in src and "expf" not in src
    assert '#include "rt_accumulate.h"' in src and "__shared__" not in src and "atomic" not in src.split("#include", 1)[1]


# ---- the reference itself --------------------------------------------------------------------------------------------

def _run_sequence(rt, O, name, calls, spp=1, scalar=False, counts=None, still=False, **kw):
    """`calls` accumulateFrame calls of the reference along a sequence on the oracle's frames; returns the list of (noisy, out, N) and the last camera."""
    kw = dict(dict(A.DEFAULTS, flags=D.default_flags(name in R.MESH_FRAMES)), **kw)
    acc = A.Accumulator(scalar=scalar)
    res = []
    for k in range(calls):
        cam, g, origin, dn = A.sequence_inputs(rt, O, name, k, still)
        noisy = oracle_frame(rt, O, name, spp, cam)
        out, N = acc.step(noisy, g, cam, origin, dn, counts=counts, **kw)
        res.append((noisy, out, N))
    return res, cam


@pytest.mark.parametrize("kw", [dict(), dict(flags=0, max_history=2, sigma_z=10.0, normal_min=-1.0), dict(flags=1, max_history=1, sigma_z=1e-3, normal_min=0.99),
                                dict(flags=2, max_history=1024, sigma_z=0.05, normal_min=0.5)])
def test_scalar_restatement_agrees_with_the_vectorised_reference(rt, O, kw):
    """`tie` (40 x 24: hits, misses, five objects), three calls along an orbit of 4 degrees per frame: one pixel and one tap at a time on float32 scalars gives
    the bits of the vectorised reference, for out and for N, in every call."""
    a, _ = _run_sequence(rt, O, "tie", 3, **kw)
    b, _ = _run_sequence(rt, O, "tie", 3, scalar=True, **kw)
    valid = A.sequence_inputs(rt, O, "tie", 2)[1]["prim"] != R.PRIM_NONE
    assert 0 < valid.sum() < valid.size
    for k in range(3):
        for what in (1, 2):
            assert np.array_equal(_bits(a[k][what]), _bits(b[k][what])), (k, what, int((_bits(a[k][what]) != _bits(b[k][what])).sum()))
    noisy, out, N = a[2]
    assert np.array_equal(_bits(out[~valid]), _bits(noisy[~valid])) and np.all(N[~valid] == 0.0) and np.all(N[valid] >= 1.0)
    assert np.array_equal(_bits(a[0][1][valid]), _bits(a[0][0][valid])) or kw.get("flags", 3) & 1        # a first call without DEMODULATE returns its input
    assert abs(float(N.max()) - min(3.0, float(kw.get("max_history", 32)))) < 1e-5       # three calls: a history of at most three frames
    if kw.get("max_history", 32) > 1:
        assert (D.ulp_distance(out, noisy).max(axis=-1) > 1)[valid].mean() > 0.5


# ---- coverage: what the sequences of the GPU tests exercise, from the reference alone -------------------------------------

def test_sequences_exercise_every_rejection(rt, O):
    """The three sequences of the GPU tests, three calls each, default parameters (SAME_PRIM on the sphere scenes only).  Over their union: pixels that are no
    candidate, candidate pixels' taps outside the image, on a pixel without a hit, rejected by the plane test, by the normal test, by SAME_PRIM alone, and valid
    candidates without any accepted tap - each above 0 - and the accepted taps the majority.  A tap is counted in the first class that rejects it."""
    total = {}
    for name in A.SEQUENCES:
        cnt = {}
        _run_sequence(rt, O, name, 3, counts=cnt)
        print(name, {k: cnt[k] for k in A.COUNTS})
        assert sum(cnt[k] for k in A.TAP_COUNTS) == 4 * cnt["candidate"] and cnt["valid"] == cnt["candidate"] + cnt["no_candidate"]
        assert cnt["candidate"] == cnt["blended"] + cnt["candidate_without_tap"]
        for k in A.COUNTS:
            total[k] = total.get(k, 0) + cnt[k]
    print("union", total)
    for k in ("no_candidate", "outside", "no_hit", "plane", "normal", "prim_alone", "candidate_without_tap"):
        assert total[k] > 0, k
    assert 2 * total["accepted"] > sum(total[k] for k in A.TAP_COUNTS)


# ---- quality, from the reference alone -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_spheres", "random_50x37"])
def test_accumulation_reduces_the_error_of_a_camera_move(rt, O, name):
    """Four frames at 1 spp along the sequence: RMSE(accumulated, target) / RMSE(last noisy frame, target) < 1, the target the oracle's frame of the last camera
    at 256 spp (DESIGN.md 3.12 records the ratios this prints).  The still camera is printed, not asserted: the noise of a pixel depends on the pixel alone, so
    every frame of a camera that does not move is the same and the ratio is 1."""
    res, cam = _run_sequence(rt, O, name, 4)
    target = oracle_frame(rt, O, name, 256, cam)
    noisy, out, N = res[-1]
    assert np.isfinite(noisy).all() and np.isfinite(target).all() and np.isfinite(out).all()
    ratio = D.rmse(out, target) / D.rmse(noisy, target)
    print(f"{name}: 4 frames at 1 spp, RMSE noisy {D.rmse(noisy, target):.5f}, accumulated {D.rmse(out, target):.5f}, ratio {ratio:.3f}, mean N {float(N[N > 0].mean()):.2f}")
    still, cam0 = _run_sequence(rt, O, name, 4, still=True)
    target0 = oracle_frame(rt, O, name, 256, cam0)
    print(f"{name}: camera still, ratio {D.rmse(still[-1][1], target0) / D.rmse(still[-1][0], target0):.4f}")
    assert ratio < 1.0
