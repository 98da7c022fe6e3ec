"""CPU checks of displayFrame's interface (include/rt_api.h) and of everything of it that runs without a GPU: the new symbols are declared, exported and bound,
the constants agree between header and Python, the ABI version and the struct sizes are the parent's, a call before init is the library's misuse exit; the
device's powf (csrc/rt_glibc_powf_pos.h) compiled for the host is libm's powf(x, 0.416666667f) bit for bit, and the 8-bit code built on it is rtLinearToSRGB's;
the CPU twin rtDisplayFrameHost equals the numpy reference (tests/display_reference.py) byte for byte on the cases the GPU tests hold displayFrame to, and
rtLinearToSRGB on the fixtures minted from the reference renderer."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import display_reference as D
import test_renderer_host_structure as H
from preview_support import exits_99

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-raytracing-optimized_amd")
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("displayFrame", "rtLastExposure", "rtDisplayHistogram", "rtResetDisplay", "rtLastDisplayMs")


def test_declared_exported_and_bound(rt):
    assert re.search(r"void\s+displayFrame\s*\(\s*const\s+rt_vec3\s*\*\s*in\s*,\s*uint8_t\s*\*\s*out_rgba\s*,\s*int\s+flags\s*,\s*int\s+tonemap\s*,"
                     r"\s*float\s+exposure\s*,\s*float\s+adapt\s*\)\s*;", API)
    assert re.search(r"float\s+rtLastExposure\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"int\s+rtDisplayHistogram\s*\(\s*uint32_t\s*\*\s*out\s*,\s*int\s+cap\s*\)\s*;", API)
    assert re.search(r"void\s+rtResetDisplay\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"double\s+rtLastDisplayMs\s*\(\s*void\s*\)\s*;", API)
    lib = C.CDLL(os.path.join(PKG, "librt_mi355x.so"))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    r = rt.load_renderer()
    assert r.displayFrame.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float] and r.displayFrame.restype is None
    assert r.rtLastExposure.argtypes == [] and r.rtLastExposure.restype is C.c_float
    assert r.rtDisplayHistogram.argtypes == [C.POINTER(C.c_uint32), C.c_int] and r.rtDisplayHistogram.restype is C.c_int
    assert r.rtResetDisplay.argtypes == [] and r.rtResetDisplay.restype is None
    assert r.rtLastDisplayMs.argtypes == [] and r.rtLastDisplayMs.restype is C.c_double
    for fn in ("display_frame", "last_exposure", "display_histogram", "reset_display", "last_display_ms", "display_frame_host"):
        assert callable(getattr(rt, fn)), fn
    sig = inspect.signature(rt.display_frame).parameters
    assert list(sig) == ["src", "out", "flags", "tonemap", "exposure", "adapt"] and [sig[k].default for k in sig] == [None, None, 0, 0, 1.0, 1.0]
    # the host twin: declared in rt_host.h, exported by librt_host.so, bound
    host_h = open(os.path.join(ROOT, "include", "rt_host.h")).read()
    assert re.search(r"\brtDisplayFrameHost\s*\(\s*const\s+rt_vec3\s*\*\s*in\s*,\s*uint8_t\s*\*\s*out_rgba\s*,\s*int\s+nx\s*,\s*int\s+ny\s*,\s*int\s+flags\s*,"
                     r"\s*int\s+tonemap\s*,\s*float\s+exposure\s*,\s*float\s+adapt\s*,\s*float\s*\*\s*E_state\s*,\s*uint32_t\s*\*\s*hist\s*\)\s*;", host_h)
    assert "rtDisplayFrameHost" in rt.HOST_SYMBOLS and hasattr(C.CDLL(os.path.join(PKG, "librt_host.so")), "rtDisplayFrameHost")
    assert rt.load_host().rtDisplayFrameHost.argtypes[:8] == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]


def test_constants_agree_between_header_reference_and_python(rt):
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(RT_(?:DISPLAY|TONEMAP)_[A-Z_]+)\s*=\s*(\d+)", API))
    assert enums == dict(RT_DISPLAY_TOP_DOWN=rt.RT_DISPLAY_TOP_DOWN, RT_DISPLAY_DITHER=rt.RT_DISPLAY_DITHER, RT_DISPLAY_AUTO_EXPOSURE=rt.RT_DISPLAY_AUTO_EXPOSURE,
                         RT_DISPLAY_FROM_PREVIEW=rt.RT_DISPLAY_FROM_PREVIEW, RT_TONEMAP_NONE=rt.RT_TONEMAP_NONE, RT_TONEMAP_REINHARD=rt.RT_TONEMAP_REINHARD,
                         RT_TONEMAP_ACES=rt.RT_TONEMAP_ACES)
    flags = [rt.RT_DISPLAY_TOP_DOWN, rt.RT_DISPLAY_DITHER, rt.RT_DISPLAY_AUTO_EXPOSURE, rt.RT_DISPLAY_FROM_PREVIEW]
    assert all(f > 0 and f & (f - 1) == 0 for f in flags) and len(set(flags)) == 4
    assert (D.TOP_DOWN, D.DITHER, D.AUTO_EXPOSURE, D.FROM_PREVIEW) == tuple(flags)
    assert (D.NONE, D.REINHARD, D.ACES) == (rt.RT_TONEMAP_NONE, rt.RT_TONEMAP_REINHARD, rt.RT_TONEMAP_ACES)
    assert re.search(r"#define\s+RT_DISPLAY_BINS\s+256\b", API) and rt.RT_DISPLAY_BINS == D.BINS == 256
    assert re.search(r"#define\s+RT_DISPLAY_KEY\s+0\.18f\b", API) and np.float32(rt.RT_DISPLAY_KEY) == D.KEY
    m = re.search(r"#define\s+RT_DISPLAY_BAYER8\s+(.*?)\n[^\n]*\n[^\n]*\n", API, re.S)
    bayer = np.array([int(x) for x in re.findall(r"\d+", m.group(0).split("BAYER8", 1)[1])]).reshape(8, 8)
    assert np.array_equal(bayer, D.BAYER8) and np.array_equal(bayer, np.array(rt.RT_DISPLAY_BAYER8)) and sorted(bayer.ravel()) == list(range(64))
    # an ordered-dither matrix: every 2 x 2 block of every quadrant level is spread, the classic recursion B(2n) = [[4B, 4B+2], [4B+3, 4B+1]]
    b2 = np.array([[0, 2], [3, 1]])
    b4 = np.block([[4 * b2, 4 * b2 + 2], [4 * b2 + 3, 4 * b2 + 1]])
    assert np.array_equal(bayer, np.block([[4 * b4, 4 * b4 + 2], [4 * b4 + 3, 4 * b4 + 1]]))


def test_abi_unchanged(rt):
    assert rt.load_renderer().rtApiVersion() == 1002 == rt.RT_API_VERSION
    assert re.search(r"#define RT_API_VERSION 1002\b", API)
    sizes = (C.c_int32 * 32)()
    n = rt.load_renderer().rtStructSizes(sizes, 32)
    assert n == 13 and [sizes[k] for k in range(n)] == [C.sizeof(s) for s in rt.ABI_STRUCTS]


@pytest.mark.parametrize("call", ["rt.display_frame(np.zeros((4, 4, 3), np.float32))",
                                  "a = np.zeros((4, 4, 3), np.float32); o = np.zeros((4, 4, 4), np.uint8); rt.load_renderer().displayFrame(a.ctypes.data, o.ctypes.data, 0, 0, 1.0, 1.0)",
                                  "rt.last_exposure()", "rt.display_histogram()", "rt.reset_display()", "rt.last_display_ms()"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99("rt._state.update(nx=4, ny=4)\n%s\n" % call)


def test_translation_unit_and_host_path():
    """One object with the denoiser's command, linked into the library beside RT_OBJS; rt_glibc_powf.h and the render kernels' sources do not know the new
    headers; the host function keeps to the shared path of the passes: no allocation, release, event or device switch of its own."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    rules = re.findall(r"^\$\(OBJ\)/(\S+)\.o:\s*\$\(CSRC\)/rt_kernels_display\.hip([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert len(rules) == 1 and rules[0][0] == "display", rules
    for dep in ("$(CSRC)/rt_display.h", "$(CSRC)/rt_glibc_powf_pos.h", "$(CSRC)/rt_glibc_powf.h"):
        assert dep in rules[0][1].split(), dep
    denoise = re.search(r"^\$\(OBJ\)/denoise\.o:[^\n]*\n\t([^\n]+)", mk, re.M).group(1)
    assert rules[0][2].split() == denoise.split() and "-ffp-contract=off" in denoise.split()
    link = re.search(r"^\$\(PKG\)/librt_mi355x\.so:([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert "$(DISPLAY_OBJS)" in link.group(1).split() and "$(DISPLAY_OBJS)" in link.group(2).split()
    assert re.search(r"^DISPLAY_OBJS\s*:=\s*\$\(OBJ\)/display\.o\s*$", mk, re.M)
    host = re.search(r"^\$\(PKG\)/librt_host\.so:([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert "$(HOST)/rt_display_host.cpp" in host.group(1).split() and "$(HOST)/rt_display_host.cpp" in host.group(2).split() and "-ffp-contract=off" in host.group(2).split()
    csrc = os.path.join(PKG, "csrc")
    for name in ("rt_kernels_spheres.hip", "rt_kernels_mesh.hip", "rt_probe.hip", "rt_params.h", "rt_device.h", "rt_glibc_powf.h", "rt_kernels_denoise.hip",
                 "rt_kernels_accumulate.hip", "rt_kernels_preview.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert "rt_display" not in text and "powf_pos" not in text, name
    src = open(os.path.join(csrc, "rt_kernels_display.hip")).read()
    assert "fmaf" not in src and "expf" not in src and "__powf" not in src and "__shared__" in src and "atomicAdd" in src
    twin = open(os.path.join(csrc, "rt_glibc_powf_pos.h")).read()
    assert '#include "rt_glibc_powf.h"' in twin and "(double)y *" in twin and "rt_powf_log2_tab[32]" not in twin      # the tables are the other header's
    rsrc = H._source()
    funcs = H._functions(rsrc)
    body = [rsrc[a:b] for n, a, b in funcs if n == "displayFrame"]
    assert len(body) == 1
    for call in ("hipMalloc", "hipFree", "hipEventCreate", "hipGetDevice", "hipSetDevice", "hipStreamSynchronize", "hipDeviceSynchronize"):
        assert not re.search(r"\b%s\b" % call, body[0]), call
    assert "RtPartition" not in body[0] and "launch_guides" not in body[0]
    for call in (r"begin_pass\(", r"end_pass\("):
        assert len(re.findall(r"\b" + call, body[0])) == 1, call
    assert re.search(r"^struct DisplayState\s*:\s*PassState\s*\{", rsrc, re.M)
    for fn in ("setup_devices", "cleanup_impl"):
        assert "free_pass(g_display)" in "".join(rsrc[a:b] for n, a, b in funcs if n == fn), fn
    assert "reset_display()" in "".join(rsrc[a:b] for n, a, b in funcs if n == "setRenderOptions")


# ---- the device's powf, compiled for the host ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """tests/display_powf_twin.c (which includes csrc/rt_glibc_powf_pos.h) as a shared object in a temporary directory, linked against librt_host.so."""
    so = str(tmp_path_factory.mktemp("display_twin") / "libdisplay_twin.so")
    r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", os.path.join(ROOT, "tests", "display_powf_twin.c"), "-o", so,
                        "-L" + PKG, "-lrt_host", "-Wl,-rpath," + PKG, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(so)
    lib.display_twin_mismatches.restype = C.c_long
    lib.display_twin_mismatches.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_long)]
    lib.display_twin_powf.restype = C.c_float
    lib.display_twin_powf.argtypes = [C.c_float, C.c_float]
    lib.display_twin_code.restype = C.c_uint32
    lib.display_twin_code.argtypes = [C.c_float]
    return lib


def test_powf_twin_is_libm(twin):
    """rt_glibc_powf_pos.h compiled for the host equals this machine's libm powf(x, 0.416666667f) in every bit on ALL floats of [0, 1.0000002] - everything a
    frame in [0, 1] encodes - on every 61st bit pattern of [0, +inf], and for NaN; over the same ranges (the stride's below 2^40: the C conversion of
    rtLinearToSRGB is undefined above) the 8-bit code built on the twin is rtLinearToSRGB's."""
    bad, codes = C.c_uint32(0), C.c_long(0)
    threads = min(8, os.cpu_count() or 1)
    one_plus = int(np.float32(1.0000002).view(np.uint32))
    assert one_plus == 0x3F800002
    assert twin.display_twin_mismatches(0, one_plus + 1, 1, threads, 1, C.byref(bad), C.byref(codes)) == 0, hex(bad.value)
    assert codes.value == 0, hex(bad.value)
    two40 = int(np.float32(2.0 ** 40).view(np.uint32))
    assert twin.display_twin_mismatches(0, two40, 61, threads, 1, C.byref(bad), C.byref(codes)) == 0, hex(bad.value)
    assert codes.value == 0, hex(bad.value)
    first = two40 - two40 % 61                                  # (the same lattice of bit patterns, continued to +inf inclusive)
    assert twin.display_twin_mismatches(first, 0x7F800001, 61, threads, 0, C.byref(bad), C.byref(codes)) == 0, hex(bad.value)
    assert twin.display_twin_mismatches(0x7F800000, 0x7F800001, 1, 1, 0, C.byref(bad), C.byref(codes)) == 0          # +inf itself
    for nan in (0x7FC00000, 0x7F800001, 0xFFC12345):
        assert twin.display_twin_mismatches(nan, nan + 1, 1, 1, 0, C.byref(bad), C.byref(codes)) == 0, hex(nan)
        assert np.isnan(twin.display_twin_powf(float(np.uint32(nan).view(np.float32)), 0.416666667))
    assert twin.display_twin_powf(0.0, 0.416666667) == 0.0 and twin.display_twin_powf(1.0, 0.416666667) == 1.0 and twin.display_twin_powf(float("inf"), 0.416666667) == float("inf")
    # the exponent is a variable: other positive exponents are libm's as well (a spot check of the generalisation, not of displayFrame)
    x = np.random.default_rng(5).uniform(0, 4, 2000).astype(np.float32)
    for y in (0.416666667, 0.5, 1.0, 2.2, 5.0, 0.001):
        got = np.array([twin.display_twin_powf(float(v), y) for v in x], np.float32)
        assert np.array_equal(got.view(np.uint32), D.powf(x, np.float32(y)).view(np.uint32)), y
    # where the definitions part: the device's clamp gives 255, the C conversion of rtLinearToSRGB is undefined (rt_api.h)
    assert twin.display_twin_code(float("inf")) == 255 and twin.display_twin_code(1e30) == 255 and twin.display_twin_code(float("nan")) == 0
    assert twin.display_twin_code(float("-inf")) == 0


# ---- the CPU twin against the numpy reference ---------------------------------------------------------------------------

def _host_sequence(rt, frames, calls):
    """rtDisplayFrameHost and the reference side by side over `calls` = [(frame index, flags, tonemap, exposure, adapt)], one state each."""
    ref, state = D.Display(), np.array([np.nan], np.float32)
    for k, (f, flags, tonemap, exposure, adapt) in enumerate(calls):
        frame = np.ascontiguousarray(frames[f])
        before = state.copy()
        got, hist = rt.display_frame_host(frame, flags=flags, tonemap=tonemap, exposure=exposure, adapt=adapt, state=state, histogram=True)
        want, E_used, want_hist = ref.step(frame, flags, tonemap, exposure, adapt)
        assert np.array_equal(got, want), (k, flags, tonemap, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        if flags & D.AUTO_EXPOSURE:
            assert np.array_equal(hist, want_hist), k
            assert state.view(np.uint32)[0] == np.float32(ref.E).view(np.uint32), (k, state, ref.E)
        else:
            assert np.array_equal(state.view(np.uint32), before.view(np.uint32)) and not hist.any()


@pytest.mark.parametrize("nx,ny", D.SIZES)
def test_host_twin_equals_the_reference_on_synthetic_frames(rt, nx, ny):
    """Every tone map with each flag alone and all together, at every size of the GPU tests, on the frames those use."""
    frame = D.synthetic(100 + nx, nx, ny)
    for tonemap, flags in D.CASES:
        _host_sequence(rt, [frame], [(0, flags, tonemap, 1.0, 1.0), (0, flags, tonemap, 0.37, 0.5)])


def test_synthetic_frames_cover_the_edges():
    """What the largest synthetic frame holds, from the reference alone: luminances exactly on bin edges, in the first and in the last bin, beyond both ends,
    negative channels and negative luminance, values over 2^-20 .. 2^20, more than one histogram workgroup of 256 pixels."""
    frame = D.synthetic(100 + 130, 130, 67)
    assert frame.shape == (67, 130, 3) and frame.shape[0] * frame.shape[1] > 4 * 256
    l = np.ascontiguousarray(D.lum(frame))
    b, counted = D.bins_of(frame)
    on_edge = counted & ((l.view(np.uint32) & 0xFFFFF) == 0)
    assert on_edge.sum() >= 5 and (b[counted] == 0).any() and (b[counted] >= 255).sum() >= 2 and (b[counted] > 255).any()
    assert ((b == -1) & (l > 0)).any() and (l < 0).any() and (frame < 0).any() and (l == 0).any()
    assert np.abs(frame).max() > 2.0 ** 19 and np.abs(frame[frame != 0]).min() < 2.0 ** -19
    hist = D.histogram(frame)
    assert hist.sum() == counted.sum() and hist[0] > 0 and hist[255] >= 2 and 0 < counted.sum() < counted.size
    assert (D.bins_of(D.special_frame())[1]).sum() < D.special_frame().shape[0] * D.special_frame().shape[1]


def test_host_twin_special_pixels(rt):
    """NaN and -inf encode to 0, +inf, 1e30 and FLT_MAX to 255 (the clamp before the conversion), denormals and both zeros to 0; non-finite and non-positive
    luminance stays out of the histogram; an all-black frame has T = 0 and E = 1.  And the twin equals the reference on all of it, every tone map."""
    frame = D.special_frame()
    for tonemap, flags in D.CASES:
        _host_sequence(rt, [frame], [(0, flags, tonemap, 1.0, 1.0)])
    out, hist = rt.display_frame_host(np.ascontiguousarray(frame), flags=D.AUTO_EXPOSURE, exposure=1.0, histogram=True)
    plain = rt.display_frame_host(np.ascontiguousarray(frame))
    code = {v: [int(plain[k, col, k]) for k in range(3)] for col, v in enumerate(map(repr, D.SPECIAL_VALUES))}
    assert code["nan"] == [0] * 3 and code["-inf"] == [0] * 3 and code["-1e+30"] == [0] * 3 and code["1e-40"] == [0] * 3 and code["-0.0"] == [0] * 3
    assert code["inf"] == [255] * 3 and code["1e+30"] == [255] * 3 and code["3.4028234e+38"] == [255] * 3 and code["1.0"] == [255] * 3
    assert (plain[..., 3] == 255).all()
    l = D.lum(frame)
    assert hist.sum() == int((np.isfinite(l) & (l > 0)).sum()) < l.size          # (every finite positive luminance of this frame lies above 2^-16)
    black = np.zeros((5, 7, 3), np.float32)
    state = np.array([np.nan], np.float32)
    out, hist = rt.display_frame_host(black, flags=D.AUTO_EXPOSURE, exposure=2.0, state=state, histogram=True)
    assert not hist.any() and state[0] == 1.0 and not out[..., :3].any()


def test_host_twin_adaptation(rt):
    """Four AUTO_EXPOSURE calls with adapt = 0.25 on frames of different brightness follow the reference's E bit for bit, a call without the flag in between
    leaves the state alone, and a NaN state (a reset) adapts from nothing."""
    frames = [D.synthetic(7, 50, 37, scale) for scale in (1.0, 16.0, 0.01, 300.0)]
    A = D.AUTO_EXPOSURE
    _host_sequence(rt, frames, [(0, A, D.NONE, 1.0, 0.25), (1, A, D.REINHARD, 1.0, 0.25), (2, D.DITHER, D.ACES, 3.0, 0.25), (2, A, D.ACES, 0.5, 0.25),
                                (3, A | D.TOP_DOWN, D.NONE, 1.0, 0.25)])
    targets = [D.target_of(D.histogram(f)) for f in frames]
    assert len({float(t) for t in targets}) == 4                # the frames do differ in their median bin
    for bad in (dict(flags=16), dict(flags=D.FROM_PREVIEW), dict(tonemap=3), dict(tonemap=-1), dict(exposure=0.0), dict(exposure=float("nan")), dict(exposure=float("inf")),
                dict(adapt=0.0), dict(adapt=1.5), dict(adapt=float("nan"))):
        with pytest.raises(ValueError):
            rt.display_frame_host(np.ascontiguousarray(frames[0]), **bad)


def test_host_twin_equals_rtLinearToSRGB_on_the_fixtures(rt):
    """NONE, E = 1, no dither: the RGB bytes are rtLinearToSRGB's on the seeded framebuffer of tests/golden/hostio.npz (finite, up to 1e9) and on the
    srgb_in / srgb vectors of tests/golden/materials.npz, minted from the reference renderer's own linearToSRGB."""
    h = rt.load_host()
    fb = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "hostio.npz"))["fb"], np.float32)
    assert fb.ndim == 3 and np.isfinite(fb).all() and float(np.abs(fb).max()) < 2.0 ** 40
    got = rt.display_frame_host(fb)
    want = np.array([h.rtLinearToSRGB(float(x)) for x in fb.ravel()], np.uint32).reshape(fb.shape)
    assert np.array_equal(got[..., :3], want) and (got[..., 3] == 255).all()
    assert np.array_equal(rt.display_frame_host(fb, flags=D.TOP_DOWN), got[::-1])
    g = np.load(os.path.join(GOLDEN, "materials.npz"))
    x = np.ascontiguousarray(g["srgb_in"], np.float32)
    row = np.ascontiguousarray(np.repeat(x[None, :, None], 3, axis=2))
    got = rt.display_frame_host(row)
    for k in range(3):
        assert np.array_equal(got[0, :, k].astype(np.uint32), g["srgb"])
    assert np.array_equal(D.transform(row, 1.0)[0, :, 0].astype(np.uint32), g["srgb"])           # and the numpy reference
