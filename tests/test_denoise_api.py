"""CPU checks of the preview denoiser's interface (include/rt_api.h): denoiseFrame / rtDefaultDenoiseFlags / rtLastDenoiseMs are declared, exported and bound,
the constants agree between header and Python, the ABI version and the struct sizes are the parent's, a call before init is the library's misuse exit, the new
translation unit is built once with contraction off; and, from the test reference alone (tests/denoise_reference.py): its vectorisation agrees bit for bit with
a per-pixel scalar restatement, the frames of the GPU tests exercise every weight and both ways of skipping a tap, and the filter with its default parameters
reduces the error of 4 spp frames."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_reference as D
import guides_reference as R
from preview_support import bits as _bits, exits_99

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
NEW = ("rtDefaultDenoiseFlags", "denoiseFrame", "rtLastDenoiseMs")


def test_declared_exported_and_bound(rt):
    assert re.search(r"void\s+denoiseFrame\s*\(\s*const\s+rt_vec3\s*\*\s*in\s*,\s*rt_vec3\s*\*\s*out\s*,\s*int\s+iterations\s*,\s*int\s+flags\s*,"
                     r"\s*int\s+normal_squarings\s*,\s*float\s+sigma_z\s*,\s*float\s+sigma_c\s*\)\s*;", API)
    assert re.search(r"int\s+rtDefaultDenoiseFlags\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"double\s+rtLastDenoiseMs\s*\(\s*void\s*\)\s*;", API)
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    r = rt.load_renderer()
    assert r.denoiseFrame.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float] and r.denoiseFrame.restype is None
    assert r.rtDefaultDenoiseFlags.argtypes == [] and r.rtDefaultDenoiseFlags.restype is C.c_int
    assert r.rtLastDenoiseMs.argtypes == [] and r.rtLastDenoiseMs.restype is C.c_double
    assert callable(rt.denoiseFrame) and callable(rt.last_denoise_ms) and callable(rt.default_denoise_flags)
    assert r.rtLastDenoiseMs() == 0.0                           # before the first call; no device is touched


def test_constants_agree_between_header_and_python(rt):
    enums = {k: int(v) for k, v in re.findall(r"\b(RT_DENOISE_[A-Z_]+)\s*=\s*(\d+)", API)}
    assert enums == {"RT_DENOISE_DEMODULATE": 1, "RT_DENOISE_SAME_PRIM": 2}
    defines = dict(re.findall(r"#define\s+(RT_DENOISE_[A-Z_]+)\s+([0-9.]+)f?\b", API))
    assert defines == {"RT_DENOISE_MAX_ITERATIONS": "8", "RT_DENOISE_MAX_SQUARINGS": "7", "RT_DENOISE_ALBEDO_FLOOR": "0.01"}
    for name, value in enums.items():
        assert getattr(rt, name) == value, name
    assert (rt.RT_DENOISE_MAX_ITERATIONS, rt.RT_DENOISE_MAX_SQUARINGS) == (8, 7)
    assert np.float32(rt.RT_DENOISE_ALBEDO_FLOOR) == np.float32(0.01) == D.ALBEDO_FLOOR
    assert (D.DEMODULATE, D.SAME_PRIM) == (rt.RT_DENOISE_DEMODULATE, rt.RT_DENOISE_SAME_PRIM)
    import inspect
    sig = inspect.signature(rt.denoiseFrame).parameters
    assert [sig[k].default for k in ("fb", "iterations", "flags", "normal_squarings", "sigma_z", "sigma_c")] == [None, 5, None, 5, 0.01, 1.0]
    assert D.DEFAULTS == dict(iterations=5, normal_squarings=5, sigma_z=0.01, sigma_c=1.0)


def test_abi_unchanged(rt):
    assert rt.load_renderer().rtApiVersion() == 1002 == rt.RT_API_VERSION
    assert re.search(r"#define RT_API_VERSION 1002\b", API)
    sizes = (C.c_int32 * 32)()
    n = rt.load_renderer().rtStructSizes(sizes, 32)
    assert n == 13 and [sizes[k] for k in range(n)] == [C.sizeof(s) for s in rt.ABI_STRUCTS]


@pytest.mark.parametrize("call", ["rt.denoiseFrame(np.zeros((4, 4, 3), np.float32))", "rt.load_renderer().denoiseFrame(None, None, 5, 3, 5, 0.01, 1.0)",
                                  "rt.default_denoise_flags()"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99("rt._state.update(nx=4, ny=4)\n%s\n" % call)


def test_translation_unit_is_built_once_with_contraction_off():
    """One arithmetic, defined bit for bit: one object, compiled like the PARITY objects; the existing kernel files do not see the new header; the kernel
    names keep away from the strings the production-form tripwires scan for."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    rules = re.findall(r"^\$\(OBJ\)/(\S+)\.o:\s*\$\(CSRC\)/rt_kernels_denoise\.hip[^\n]*\n\t([^\n]+)", mk, re.M)
    assert len(rules) == 1 and rules[0][0] == "denoise", rules
    line = rules[0][1]
    for flag in ("-ffp-contract=off", "-fno-slp-vectorize", "-fno-vectorize"):
        assert flag in line.split(), (flag, line)
    assert "-fno-hip-fp32-correctly-rounded-divide-sqrt" not in line and "-ffast-math" not in line and "-fgpu-flush-denormals-to-zero" not in line
    assert "RT_MODE_" not in line
    assert re.search(r"^RT_OBJS\s*:=.*\$\(OBJ\)/denoise\.o", mk, re.M)
    csrc = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")
    for name in ("rt_kernels_spheres.hip", "rt_kernels_mesh.hip", "rt_probe.hip", "rt_params.h", "rt_device.h"):
        assert "denoise" not in open(os.path.join(csrc, name)).read().lower(), name
    src = open(os.path.join(csrc, "rt_kernels_denoise.hip")).read()
    for scanned in ("launch_mesh_queue<", "k_render_mesh<", "k_render_spheres_tiles<", "launch_queue_form", "launch_kind_of", "launch_with_lds", "k_render_spheres_queue<", "k_render_mesh_queue<"):
        assert scanned not in src, scanned
    assert "fmaf" not in src and "__fmaf" not in src and "expf" not in src


# ---- the reference itself --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(iterations=3, flags=0, normal_squarings=0, sigma_c=0.0), dict(iterations=2, flags=2, normal_squarings=7, sigma_z=1e-3, sigma_c=0.25),
                                dict(iterations=4, flags=1, normal_squarings=2, sigma_z=10.0)])
def test_scalar_restatement_agrees_with_the_vectorised_reference(rt, O, kw):
    """`tie` (40 x 24: hits, misses, five objects) at 4 spp: one pixel and one tap at a time on float32 scalars gives the bits of the vectorised reference."""
    g, origin, dn, mesh = D.frame_inputs(rt, O, "tie")
    noisy = D.oracle_frame(rt, O, "tie", 4)
    kw = dict(dict(flags=D.default_flags(mesh)), **kw)
    a = D.denoise(noisy, g, origin, dn, **kw)
    b = D.denoise_scalar(noisy, g, origin, dn, **kw)
    valid = g["prim"] != R.PRIM_NONE
    assert 0 < valid.sum() < valid.size
    assert np.array_equal(_bits(a), _bits(b)), int((_bits(a) != _bits(b)).sum())
    assert np.array_equal(_bits(a[~valid]), _bits(noisy[~valid]))           # pass-through of the pixels without a hit
    assert (D.ulp_distance(a, noisy).max(axis=-1) > 1)[valid].mean() > 0.5


def test_vectorised_centre_ray_is_the_oracle_s(rt, O):
    """The numpy restatement of the centre ray (the large frame of the GPU test uses it) against orc_get_ray, on random_96x64 and the staircase camera."""
    sp, mt, cam, nx, ny = R.sphere_frame(rt, "random_96x64")
    for cam, nx, ny in ((cam, nx, ny), (rt.staircase_camera(R.STAIR_NX, R.STAIR_NY), R.STAIR_NX, R.STAIR_NY)):
        o1, d1 = D.centre_dirs(rt, O, cam, nx, ny)
        o2, d2 = D.centre_dirs_numpy(cam, nx, ny)
        assert np.array_equal(_bits(o1), _bits(o2)) and np.array_equal(_bits(d1), _bits(d2))


# ---- coverage: what the frames of the GPU tests exercise, from the reference alone -------------------------------------

@pytest.mark.parametrize("name", ["random_96x64", "staircase_a"])
def test_frames_exercise_every_weight(rt, O, name):
    """4 spp, default parameters.  Shares are of the 24 x iterations non-centre taps of the valid pixels.  At least 10 % of the valid pixels change by more than
    1 ulp; wn < 1, wz < 1, wc < 1 (and a primitive mismatch on spheres) each on at least 1 % of the taps; on random_96x64 taps are skipped both for lying outside
    the image and for having no first hit."""
    g, origin, dn, mesh = D.frame_inputs(rt, O, name)
    noisy = D.oracle_frame(rt, O, name, 4)
    assert np.isfinite(noisy).all()
    cnt = {}
    out = D.denoise(noisy, g, origin, dn, flags=D.default_flags(mesh), counts=cnt, **D.DEFAULTS)
    valid = g["prim"] != R.PRIM_NONE
    changed = float((D.ulp_distance(out, noisy).max(axis=-1) > 1)[valid].mean())
    share = {k: cnt[k] / cnt["taps"] for k in D.COUNTS}
    print(name, "valid pixels changed by more than 1 ulp: %.3f" % changed, {k: round(v, 4) for k, v in share.items()})
    assert cnt["taps"] == 24 * 5 * int(valid.sum()) and cnt["outside"] + cnt["invalid"] + cnt["accepted"] == cnt["taps"]
    assert changed >= 0.10
    for k in ("wn_lt1", "wz_lt1", "wc_lt1"):
        assert share[k] >= 0.01, k
    if mesh:
        assert cnt["prim_mismatch"] == 0                        # SAME_PRIM is off for meshes: not counted
    else:
        assert share["prim_mismatch"] >= 0.01
        assert cnt["outside"] > 0 and cnt["invalid"] > 0


def test_small_frame_loses_most_taps_from_stride_16_on(rt, O):
    """cloud_hybrid is 32 x 24: at stride 16 a tap with |dx| = 2 or |dy| = 2 is always outside and |dx| = 1 for half the columns, |dy| = 1 for two thirds of
    the rows - 1 - (2 * 5/3 - 1) / 24 = 90 % of the non-centre taps of uniformly spread pixels; the frame must show more than half."""
    g, origin, dn, mesh = D.frame_inputs(rt, O, "cloud_hybrid")
    noisy = D.oracle_frame(rt, O, "cloud_hybrid", 4)
    cnt = {}
    D.denoise(noisy, g, origin, dn, flags=D.default_flags(mesh), counts=cnt, **D.DEFAULTS)
    per = cnt["per_iteration"]
    print("cloud_hybrid: outside share per iteration", [round(p["outside"] / p["taps"], 3) for p in per], "all", round(cnt["outside"] / cnt["taps"], 3))
    assert per[4]["outside"] / per[4]["taps"] > 0.5
    assert per[0]["outside"] / per[0]["taps"] < 0.2


# ---- quality, from the reference alone -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["random_96x64", "three_spheres", "staircase_a", "tris300_floor"])
def test_default_parameters_reduce_the_error_at_4_spp(rt, O, name):
    """RMSE(denoised, target) / RMSE(noisy, target) < 1, the noisy frame the oracle's at 4 spp, the target the same frame at 1024 spp (DESIGN.md 3.11 records
    the ratios this prints)."""
    g, origin, dn, mesh = D.frame_inputs(rt, O, name)
    noisy, target = D.oracle_frame(rt, O, name, 4), D.oracle_frame(rt, O, name, 1024)
    assert np.isfinite(noisy).all() and np.isfinite(target).all()
    out = D.denoise(noisy, g, origin, dn, flags=D.default_flags(mesh), **D.DEFAULTS)
    ratio = D.rmse(out, target) / D.rmse(noisy, target)
    print(f"{name}: 4 spp, RMSE noisy {D.rmse(noisy, target):.5f}, denoised {D.rmse(out, target):.5f}, ratio {ratio:.3f}")
    assert ratio < 1.0
