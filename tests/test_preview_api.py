"""CPU checks of previewFrame's interface (include/rt_api.h): previewFrame / rtResetPreview / rtPreviewFrames / rtLastPreviewMs are declared, exported and bound,
the constants agree between header and Python, the ABI version and the struct sizes are the parent's, a call before init is the library's misuse exit, the new
translation unit is built once with the denoiser's flags, the host function keeps to the shared path of the whole-image passes; and, from the test reference
alone (tests/preview_reference.py): its vectorisation agrees bit for bit with a per-pixel scalar restatement, the sequences of the GPU tests exercise both
branches of the variance, every weight of the spatial estimate and the luminance weight, and the result is closer to the converged frame than the existing
accumulateFrame -> denoiseFrame chain at its defaults.

A history reaches RT_PREVIEW_MIN_HISTORY = 4 with the FOURTH call (N grows by one per call from 1), so wherever the temporal branch of the variance has to be
reached the sequences run four calls, one more than the three the first and the spatial branch need."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import accumulate_reference as A
import denoise_reference as D
import guides_reference as R
import preview_reference as V
import test_renderer_host_structure as H
from preview_support import bits as _bits, exits_99, oracle_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
NEW = ("previewFrame", "rtResetPreview", "rtPreviewFrames", "rtLastPreviewMs")


def test_declared_exported_and_bound(rt):
    assert re.search(r"void\s+previewFrame\s*\(\s*const\s+rt_vec3\s*\*\s*in\s*,\s*rt_vec3\s*\*\s*out\s*,\s*float\s*\*\s*history\s*,\s*float\s*\*\s*variance\s*,"
                     r"\s*int\s+flags\s*,\s*int\s+max_history\s*,\s*int\s+iterations\s*,\s*int\s+normal_squarings\s*,\s*float\s+sigma_z\s*,"
                     r"\s*float\s+normal_min\s*,\s*float\s+sigma_l\s*\)\s*;", API)
    assert re.search(r"void\s+rtResetPreview\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"int\s+rtPreviewFrames\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"double\s+rtLastPreviewMs\s*\(\s*void\s*\)\s*;", API)
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    r = rt.load_renderer()
    assert r.previewFrame.argtypes == [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_float] * 3 and r.previewFrame.restype is None
    assert r.rtResetPreview.argtypes == [] and r.rtResetPreview.restype is None
    assert r.rtPreviewFrames.argtypes == [] and r.rtPreviewFrames.restype is C.c_int
    assert r.rtLastPreviewMs.argtypes == [] and r.rtLastPreviewMs.restype is C.c_double
    assert callable(rt.previewFrame) and callable(rt.reset_preview) and callable(rt.preview_frames) and callable(rt.last_preview_ms)
    assert r.rtLastPreviewMs() == 0.0                           # before the first call; no device is touched


def test_constants_agree_between_header_and_python(rt):
    assert dict(re.findall(r"#define\s+(RT_PREVIEW_[A-Z_]+)\s+([0-9.e-]+)f\b", API)) == {"RT_PREVIEW_MIN_HISTORY": "4.0", "RT_PREVIEW_LUM_EPS": "1e-4"}
    assert np.float32(rt.RT_PREVIEW_MIN_HISTORY) == V.MIN_HISTORY == np.float32(4.0)
    assert np.float32(rt.RT_PREVIEW_LUM_EPS) == V.LUM_EPS == np.float32(1e-4)
    assert (V.DEMODULATE, V.SAME_PRIM) == (rt.RT_DENOISE_DEMODULATE, rt.RT_DENOISE_SAME_PRIM)
    sig = inspect.signature(rt.previewFrame).parameters
    assert list(sig) == ["fb", "out", "history", "variance", "flags", "max_history", "iterations", "normal_squarings", "sigma_z", "normal_min", "sigma_l"]
    assert [sig[k].default for k in sig] == [None, None, False, False, None, 32, 5, 5, 0.01, 0.9, 4.0]
    assert V.DEFAULTS == dict(max_history=32, iterations=5, normal_squarings=5, sigma_z=0.01, normal_min=0.9, sigma_l=4.0)


def test_abi_unchanged(rt):
    assert rt.load_renderer().rtApiVersion() == 1002 == rt.RT_API_VERSION
    assert re.search(r"#define RT_API_VERSION 1002\b", API)
    sizes = (C.c_int32 * 32)()
    n = rt.load_renderer().rtStructSizes(sizes, 32)
    assert n == 13 and [sizes[k] for k in range(n)] == [C.sizeof(s) for s in rt.ABI_STRUCTS]


@pytest.mark.parametrize("call", ["rt.previewFrame(np.zeros((4, 4, 3), np.float32), flags=3)",
                                  "a = np.zeros((4, 4, 3), np.float32); rt.load_renderer().previewFrame(a.ctypes.data, a.ctypes.data, None, None, 3, 32, 5, 5, 0.01, 0.9, 4.0)",
                                  "rt.reset_preview()", "rt.preview_frames()"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99("rt._state.update(nx=4, ny=4)\n%s\n" % call)


def test_translation_unit_is_built_once_with_the_denoiser_s_flags():
    """One arithmetic, defined bit for bit: one object, compiled like denoise.o and appended to RT_OBJS; renderer.o depends on the new header and no other
    kernel file sees it; the kernel names keep away from the strings the production-form tripwires scan for."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    rules = re.findall(r"^\$\(OBJ\)/(\S+)\.o:\s*\$\(CSRC\)/rt_kernels_preview\.hip([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert len(rules) == 1 and rules[0][0] == "preview", rules
    assert "$(CSRC)/rt_preview.h" in rules[0][1].split()
    line = rules[0][2]
    for flag in ("-ffp-contract=off", "-fno-slp-vectorize", "-fno-vectorize"):
        assert flag in line.split(), (flag, line)
    assert "-fno-hip-fp32-correctly-rounded-divide-sqrt" not in line and "-ffast-math" not in line and "-fgpu-flush-denormals-to-zero" not in line
    assert "RT_MODE_" not in line
    denoise = re.search(r"^\$\(OBJ\)/denoise\.o:[^\n]*\n\t([^\n]+)", mk, re.M).group(1)
    assert line.split() == denoise.split()                      # the same command
    objs = " ".join(re.findall(r"^RT_OBJS\s*[:+]=([^\n]*)", mk, re.M)).split()
    assert objs[-3:] == ["$(OBJ)/denoise.o", "$(OBJ)/accumulate.o", "$(OBJ)/preview.o"] and objs.count("$(OBJ)/preview.o") == 1
    renderer = re.search(r"^\$\(OBJ\)/renderer\.o:([^\n]*)", mk, re.M).group(1)
    assert "$(CSRC)/rt_preview.h" in renderer.split()
    csrc = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")
    for name in ("rt_kernels_spheres.hip", "rt_kernels_mesh.hip", "rt_probe.hip", "rt_params.h", "rt_device.h", "rt_kernels_denoise.hip", "rt_denoise.h",
                 "rt_kernels_accumulate.hip", "rt_accumulate.h"):
        assert "rt_preview" not in open(os.path.join(csrc, name)).read().lower(), name
    src = open(os.path.join(csrc, "rt_kernels_preview.hip")).read()
    for scanned in ("launch_mesh_queue<", "k_render_mesh<", "k_render_spheres_tiles<", "launch_queue_form", "launch_kind_of", "launch_with_lds", "k_render_spheres_queue<", "k_render_mesh_queue<"):
        assert scanned not in src, scanned
    assert "fmaf" not in src and "__fmaf" not in src and "expf" not in src
    assert '#include "rt_preview.h"' in src and "__shared__" not in src and "atomic" not in src.split("#include", 1)[1]
    for other in ("rt_denoise.h", "rt_accumulate.h", "rt_params.h", "rt_device.h"):
        assert not re.search(r'#include\s+"[^"\n]*%s"' % re.escape(other), src + open(os.path.join(csrc, "rt_preview.h")).read()), other


def test_the_host_function_keeps_to_the_shared_path_of_the_passes():
    """What tests/test_renderer_host_structure.py enforces for denoiseFrame and accumulateFrame, for previewFrame: no allocation, release, event creation or
    device switch of its own, no partition; it goes through begin_pass / pass_params / end_pass, its state is a PassState released by free_pass where the
    other two are."""
    src = H._source()
    funcs = H._functions(src)
    body = [src[a:b] for n, a, b in funcs if n == "previewFrame"]
    assert len(body) == 1
    body = body[0]
    for call in ("hipMalloc", "hipFree", "hipEventCreate", "hipGetDevice", "hipSetDevice"):
        assert "previewFrame" not in H._callers(src, call), call
        assert not re.search(r"\b%s\b" % call, body), call
    assert "RtPartition" not in body
    for call in (r"begin_pass\(", r"pass_params<RtPreviewParams>\(", r"end_pass\("):
        assert len(re.findall(r"\b" + call, body)) == 1, call
    assert re.search(r"^struct PreviewState\s*:\s*PassState\s*\{", src, re.M)
    for fn in ("setup_devices", "cleanup_impl"):
        text = "".join(src[a:b] for n, a, b in funcs if n == fn)
        for g in ("g_denoise", "g_accumulate", "g_preview"):
            assert "free_pass(%s)" % g in text, (fn, g)
    options = "".join(src[a:b] for n, a, b in funcs if n == "setRenderOptions")
    assert "g_accumulate.frames = 0" in options and "g_preview.frames = 0" in options
    assert len(re.findall(r"^double end_pass\(", src, re.M)) == 1 and len(re.findall(r"\bhipMemcpyAsync\s*\(\s*variance\b", src)) == 1


# ---- the reference itself --------------------------------------------------------------------------------------------

def _run_sequence(rt, O, name, calls, spp=1, scalar=False, counts=None, **kw):
    """`calls` previewFrame calls of the reference along a sequence on the oracle's frames; returns the list of (noisy, out, N, variance) and the last camera."""
    kw = dict(dict(V.DEFAULTS, flags=D.default_flags(name in R.MESH_FRAMES)), **kw)
    pre = V.Previewer(scalar=scalar)
    res = []
    for k in range(calls):
        cam, g, origin, dn = A.sequence_inputs(rt, O, name, k)
        noisy = oracle_frame(rt, O, name, spp, cam)
        res.append((noisy,) + pre.step(noisy, g, cam, origin, dn, counts=counts, **kw))
    return res, cam


@pytest.mark.parametrize("kw", [dict(), dict(flags=0, iterations=1, normal_squarings=0, max_history=2, sigma_z=10.0, normal_min=-1.0, sigma_l=0.5),
                                dict(flags=1, max_history=1, iterations=2, sigma_z=1e-3, normal_min=0.99, sigma_l=64.0),
                                dict(flags=2, max_history=1024, iterations=3, normal_squarings=2, sigma_z=0.05, normal_min=0.5)])
def test_scalar_restatement_agrees_with_the_vectorised_reference(rt, O, kw):
    """`tie` (40 x 24: hits, misses, five objects), four calls along an orbit of 4 degrees per frame: one pixel and one tap at a time on float32 scalars gives
    the bits of the vectorised reference, for out, N and the variance, in every call.  The fourth call takes the temporal variance where max_history allows."""
    cnt = {}
    a, _ = _run_sequence(rt, O, "tie", 4, counts=cnt, **kw)
    b, _ = _run_sequence(rt, O, "tie", 4, scalar=True, **kw)
    valid = A.sequence_inputs(rt, O, "tie", 3)[1]["prim"] != R.PRIM_NONE
    assert 0 < valid.sum() < valid.size
    for k in range(4):
        for what in (1, 2, 3):
            assert np.array_equal(_bits(a[k][what]), _bits(b[k][what])), (k, what, int((_bits(a[k][what]) != _bits(b[k][what])).sum()))
    noisy, out, N, var = a[3]
    assert np.array_equal(_bits(out[~valid]), _bits(noisy[~valid])) and np.all(N[~valid] == 0.0) and np.all(N[valid] >= 1.0) and np.all(var[~valid] == 0.0)
    assert np.all(var[valid] >= 0.0) and float(var.max()) > 0.0
    assert abs(float(N.max()) - min(4.0, float(kw.get("max_history", 32)))) < 1e-5       # four calls: a history of at most four frames
    print(kw, {k: cnt.get(k, 0) for k in V.COUNTS})
    assert cnt["spatial_variance"] > 0 and (cnt.get("temporal_variance", 0) > 0) == (kw.get("max_history", 32) >= 4)
    assert (D.ulp_distance(out, noisy).max(axis=-1) > 1)[valid].mean() > 0.5


# ---- coverage: what the sequences of the GPU tests exercise, from the reference alone -------------------------------------

def test_sequences_exercise_both_variances_and_every_weight(rt, O):
    """The three sequences of the GPU tests, default parameters (SAME_PRIM on the sphere scenes only), four calls each: three calls keep every history below
    RT_PREVIEW_MIN_HISTORY, the fourth reaches it.  Over their union each of these is above 0: pixels taking the temporal variance, pixels taking the spatial
    one, taps of the spatial estimate rejected by the normal weight, by the plane weight and by SAME_PRIM, a-trous taps with wl < 1."""
    total = {}
    for name in A.SEQUENCES:
        three, cnt = {}, {}
        _run_sequence(rt, O, name, 3, counts=three)
        _run_sequence(rt, O, name, 4, counts=cnt)
        print(name, "three calls", {k: three.get(k, 0) for k in V.COUNTS})
        print(name, "four calls", {k: cnt.get(k, 0) for k in V.COUNTS})
        assert three.get("temporal_variance", 0) == 0 and three["spatial_variance"] == three["valid"]
        assert cnt["valid"] == cnt["temporal_variance"] + cnt["spatial_variance"]
        for k in V.COUNTS:
            total[k] = total.get(k, 0) + cnt.get(k, 0)
    print("union", total)
    for k in ("temporal_variance", "spatial_variance", "spatial_wn_zero", "spatial_wz_zero", "spatial_prim_mismatch", "atrous_wl_lt1", "blended"):
        assert total[k] > 0, k


# ---- quality, from the reference alone -------------------------------------------------------------------------------

def _ratios(rt, O, name, frames):
    """RMSE(result, oracle 256 spp) / RMSE(last noisy 1 spp frame, same target) over the whole image after `frames` frames of the sequence, for the existing
    chain at its defaults (Accumulator.step, then D.denoise with D.DEFAULTS), the chain's best fixed sigma_c of {2, 1, 0.5, 0.25}, and previewFrame."""
    flags = D.default_flags(name in R.MESH_FRAMES)
    acc, pre = A.Accumulator(), V.Previewer()
    for k in range(frames):
        cam, g, origin, dn = A.sequence_inputs(rt, O, name, k)
        noisy = oracle_frame(rt, O, name, 1, cam)
        accumulated, _ = acc.step(noisy, g, cam, origin, dn, flags=flags, **A.DEFAULTS)
        preview = pre.step(noisy, g, cam, origin, dn, flags=flags, **V.DEFAULTS)[0]
    target = oracle_frame(rt, O, name, 256, cam)
    assert np.isfinite(noisy).all() and np.isfinite(target).all() and np.isfinite(preview).all()
    base = D.rmse(noisy, target)
    chain = {sc: D.rmse(D.denoise(accumulated, g, origin, dn, flags=flags, **dict(D.DEFAULTS, sigma_c=sc)), target) / base for sc in (2.0, 1.0, 0.5, 0.25)}
    return chain[1.0], min(chain.values()), D.rmse(preview, target) / base


@pytest.mark.parametrize("name,frames,gate", [("three_spheres", 1, True), ("random_50x37", 1, True), ("tris300_floor", 1, True), ("three_spheres", 4, True),
                                              ("random_50x37", 4, True), ("three_spheres", 8, False), ("random_50x37", 8, False)])
def test_preview_beats_the_two_call_chain_at_its_defaults(rt, O, name, frames, gate):
    """The seven rows DESIGN.md 3.13 records.  For 1 and 4 frames the previewFrame ratio is strictly below the existing chain's at its defaults on the same
    inputs, and below 1; the rows of 8 frames are printed."""
    chain, best, preview = _ratios(rt, O, name, frames)
    print(f"{name}, {frames} frame(s): accumulate -> denoise at defaults {chain:.3f}, best fixed sigma_c {best:.3f}, previewFrame {preview:.3f}")
    if gate:
        assert preview < chain, (name, frames, preview, chain)
        assert preview < 1.0, (name, frames, preview)
