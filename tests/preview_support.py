"""What the tests of the preview calls (renderGuides, denoiseFrame, accumulateFrame) share.  No test: a plain module, imported as guides_reference is, by
tests/test_gpu_{guides,denoise,accumulate,preview_edges}.py, tests/test_{guides,denoise,accumulate}_api.py, tests/test_preview_edges_reference.py and the two references of the whole-image passes
(tests/denoise_reference.py and tests/accumulate_reference.py take default_flags and oracle_frame from here)."""
import functools
import os
import subprocess
import sys

import numpy as np

import guides_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMODULATE, SAME_PRIM = 1, 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, ref, what):
    """Bit for bit: np.array_equal on the raw 32-bit words."""
    diff = bits(got) != bits(ref)
    print(f"{what}: {int(diff.sum())} of {diff.size} words differ")
    assert np.array_equal(bits(got), bits(ref)), (what, int(diff.sum()), np.argwhere(diff)[:5].tolist())


def stats_tuple(st):
    return (st.kernel_ms, st.total_ms, st.samples, st.num_launches, st.rays, st.prim_tests, st.node_visits, st.exec_tests, st.shadow_rays, st.box_tests,
            tuple(st.ref_stats))


def init_frame(rt, O, name, **opts):
    """Initialises the named frame of guides_reference (a sequence: its frame-0 camera); returns (framebuffer view, options, is-mesh)."""
    mesh = name in G.MESH_FRAMES
    if mesh:
        f = G.mesh_frame(rt, O, name)
        ks, keep = rt.make_kernel_scene(f["hm"], f["mats"], f["tex"], floor=f["floor"])
        fb = rt.initRenderer(ks, f["cam"], f["nx"], f["ny"], 16, keepalive=keep)
        if f["floor"] is not None:
            opts = dict(opts, floor=1)
    else:
        sp, mt, cam, nx, ny = G.sphere_frame(rt, name)
        fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 20)
    o = rt.getDefaultRenderOptions(not mesh)
    if opts:
        rt.setRenderOptions(o, **opts)
    return fb, o, mesh


def exits_99(body):
    """The library's misuse convention: `body` (after the imports: C, np, rt) in a child process of its own ends with 'rt error' on stderr and exit status 99
    (a clean exit of a host-side check)."""
    code = ("import sys; sys.path.insert(0, %r); import ctypes as C; import numpy as np; import cuda_raytracing_optimized_amd as rt\n" % ROOT) + body
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 99, (r.returncode, r.stderr[-1000:])
    assert "rt error" in r.stderr


def default_flags(mesh):
    return DEMODULATE if mesh else DEMODULATE | SAME_PRIM


def oracle_frame(rt, O, name, spp, cam=None):
    """The CPU oracle's render of a named frame with the default options (and the floor of the *_floor frame), from `cam` or the frame's own camera."""
    if name in G.MESH_FRAMES:
        f = G.mesh_frame(rt, O, name)
        opt = O.default_options(False)
        if f["floor"] is not None:
            opt.floor = 1
        fb, _ = O.render(O.mesh_scene(f["hm"], f["mats"], f["tex"], f["floor"]), f["cam"] if cam is None else cam, opt, f["nx"], f["ny"], spp, 16)
        return fb
    sp, mt, own, nx, ny = G.sphere_frame(rt, name)
    fb, _ = O.render(O.sphere_scene(sp, mt), own if cam is None else cam, O.default_options(True), nx, ny, spp, 20)
    return fb


# ---------------------------------------------------------------------------------------------
# non-finite and extreme pixel values, images smaller than a tile (tests/test_preview_edges_reference.py, tests/test_gpu_preview_edges.py)
# ---------------------------------------------------------------------------------------------

FLT_MAX = float(np.finfo(np.float32).max)
POISON = (float("nan"), float("inf"), float("-inf"), FLT_MAX, -FLT_MAX, 1e30)
FINITE_EXTREMES = (1e-40, -1e-40, 1.4e-45, 0.0, -0.0, -2.5, 1e-30, 1e15, -1e15, 6e4)      # denormals of both signs, the smallest one, both zeros, negative radiance
PAYLOAD_NANS = (np.uint32(0x7F800001), np.uint32(0xFFC12345))       # bit patterns: a signalling NaN and a negative quiet one with a payload (copy-through only)
NAN_CAP = 0.5                                                   # the largest NaN share of the first-hit pixels at which same_but_nan still says something


def nan_share(a, first_hit):
    """The share of the first-hit pixels with a NaN in any channel."""
    nan = np.isnan(a)
    if nan.ndim > first_hit.ndim:
        nan = nan.any(axis=-1)
    return float(nan[first_hit].mean()) if first_hit.any() else 0.0


def same_but_nan(got, ref, what, first_hit, cap):
    """As `same` where the reference holds a NaN the definition computed: the reference's own NaN share of the first-hit pixels is at most `cap` (or the
    comparison is hollow: choose other inputs), the NaNs lie in the same words, and every word that is no NaN in the reference - +-Inf, denormals and the sign
    of a zero included - is bit-equal.  Payload and sign of a computed NaN are not compared: x86 and the GPU generate different default NaNs."""
    share = nan_share(ref, first_hit)
    assert share <= cap, (what, "the reference's NaN share of the first-hit pixels", share, cap)
    nan_got, nan_ref = np.isnan(got), np.isnan(ref)
    where = nan_got != nan_ref
    diff = (bits(got) != bits(ref)) & ~nan_ref & ~where
    print(f"{what}: NaN share of the first-hit pixels {share:.4f}, {int(nan_ref.sum())} NaN words, {int(where.sum())} of them elsewhere; "
          f"{int(diff.sum())} of {int((~nan_ref).sum())} other words differ")
    assert np.array_equal(nan_got, nan_ref), (what, "NaN words", int(where.sum()), np.argwhere(where)[:5].tolist())
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:5].tolist())


def inject(src, mask, rng, values, reps=1):
    """Writes every value of `values`, `reps` times, into one randomly chosen channel of a pixel of `mask` (ny, nx) of its own, in place; a float as its float32,
    a np.uint32 as that bit pattern.  rng: a seed or a seeded np.random.Generator.  Returns the (ny, nx) mask of the pixels written."""
    rng = np.random.default_rng(rng)
    values = list(values) * reps
    at = np.argwhere(mask)
    assert len(at) >= len(values), (len(at), len(values))
    words, hit = bits(src), np.zeros(mask.shape, bool)
    assert words.base is not None and np.shares_memory(words, src)
    for (j, i), v, a in zip(at[rng.permutation(len(at))[:len(values)]], values, rng.integers(0, 3, len(values))):
        words[j, i, a] = v if isinstance(v, np.uint32) else np.float32(v).view(np.uint32)
        hit[j, i] = True
    return hit


TINY_SIZES = ((1, 1), (1, 9), (9, 1), (2, 2), (7, 3), (31, 8), (32, 8), (33, 9), (65, 17))       # around the 32 x 8 tile of the preview kernels, and below it
TINY_MESH_SIZES = ((7, 3), (33, 9))
# the sequence frames of the accumulate edge test's calls: three with special values, a finite fourth (the camera moves back: no further guide reference)
EDGE_CALLS = {"random_50x37": (0, 1, 2, 1), "staircase_a": (0, 1, 0, 1)}


@functools.lru_cache(maxsize=None)
def tiny_spheres(rt, O, nx, ny):
    """The random-spheres scene at nx x ny under its own camera and the same camera orbited by 2 degrees, both at the image's aspect:
    (spheres, materials, [(camera, guide planes, origin, centre directions)] * 2), from the references alone."""
    import accumulate_reference as A
    import denoise_reference as D
    sp, mt, cam0 = rt.scene_random_spheres(nx, ny)
    cams = [cam0, rt.make_camera(A.orbit((13, 2, 3), (0, 0, 0), 2.0), (0, 0, 0), (0, 1, 0), 30.0, nx / ny, 0.1, 10.0)]
    return sp, mt, [(cam, G.sphere_guides(rt, O, sp, mt, cam, nx, ny)) + D.centre_dirs(rt, O, cam, nx, ny) for cam in cams]


@functools.lru_cache(maxsize=None)
def tiny_mesh(rt, O, nx, ny):
    """The tris300_floor scene at nx x ny under two cameras of that aspect, the second moved as the sequence's: (frame dict, [(camera, planes, origin, dn)] * 2)."""
    import denoise_reference as D
    f = G.mesh_frame(rt, O, "tris300_floor")
    cams = [rt.make_camera((30 + 2 * k, 18, 42 - 2 * k), (0, 0, 0), (0, 1, 0), 40.0, nx / ny, 0.1, 50.0) for k in range(2)]
    return f, [(cam, G.mesh_guides(rt, O, f["hm"], f["mats"], f["tex"], cam, nx, ny, floor=f["floor"])) + D.centre_dirs(rt, O, cam, nx, ny) for cam in cams]


def synthetic(seed, ny, nx):
    """A seeded random image, uniform in [0, 4)."""
    return np.random.default_rng(seed).uniform(0, 4, (ny, nx, 3)).astype(np.float32)


def edge_image(kind, valid, seed):
    """The input images of the edge tests over a frame whose first-hit pixels are `valid`, a seeded uniform [0, 4) image with:
    no_hit_poison    POISON and the payload NaNs, five times over, in 40 pixels without a first hit;
    finite_extremes  FINITE_EXTREMES, three times over, in 30 first-hit pixels;
    denormal         every word scaled by 1e-39 (all of them fp32 denormals);
    poison           each value of POISON in one first-hit pixel;
    everything       POISON, FINITE_EXTREMES and the payload NaNs in one first-hit pixel each, and again in pixels without a first hit where the frame has
                     that many."""
    ny, nx = valid.shape
    rng = np.random.default_rng(seed)
    src = rng.uniform(0, 4, (ny, nx, 3)).astype(np.float32)
    if kind == "no_hit_poison":
        inject(src, ~valid, rng, POISON + PAYLOAD_NANS, reps=5)
    elif kind == "finite_extremes":
        inject(src, valid, rng, FINITE_EXTREMES, reps=3)
    elif kind == "denormal":
        src = src * np.float32(1e-39)
    elif kind == "poison":
        inject(src, valid, rng, POISON)
    elif kind == "everything":
        values = POISON + FINITE_EXTREMES + PAYLOAD_NANS
        inject(src, valid, rng, values)
        if int((~valid).sum()) >= len(values):
            inject(src, ~valid, rng, values)
    else:
        raise KeyError(kind)
    return src


def is_denormal(a):
    """Words that are non-zero fp32 denormals."""
    w = bits(a)
    return ((w & np.uint32(0x7F800000)) == 0) & ((w & np.uint32(0x007FFFFF)) != 0)
