"""The preview calls (renderGuides, denoiseFrame, accumulateFrame) on the GPU where the other GPU tests do not go: pixel values that are not well-behaved - NaN,
+-Inf, +-FLT_MAX, fp32 denormals, signed zeros, negative radiance - and images smaller than the kernels' 32 x 8 tile.  Every pixel against the test references
(tests/denoise_reference.py, tests/accumulate_reference.py, tests/guides_reference.py), bit for bit; where the definition itself computes NaNs, the NaN words
must be the reference's and every other word bit-equal (preview_support.same_but_nan: payload and sign of a computed NaN differ between x86 and the GPU).
tests/test_preview_edges_reference.py pins, on the CPU, the conditions these inputs rely on.

What the special values are for: a tap that is outside the image or has no first hit is loaded and then dropped by a select, not multiplied by a zero weight
(0 * NaN and 0 * Inf are NaN); fp32 denormals are kept; max(x, 0) of a NaN is 0; a comparison with a NaN is false."""
import numpy as np
import pytest

import accumulate_reference as A
import denoise_reference as D
import guides_reference as R
import preview_support as S
from preview_support import bits as _bits, init_frame as _init, same as _same

pytestmark = pytest.mark.gpu
DENOISE_FRAMES = ("random_96x64", "staircase_a")
ACCUMULATE_SEQUENCES = ("random_50x37", "staircase_a")
POISON_CASES = [dict(iterations=it, sigma_c=sc, normal_squarings=sq) for it in (1, 2) for sc in (1.0, 0.0) for sq in (0, 5)]


def _denoise_kw(mesh, **kw):
    return dict(dict(D.DEFAULTS, flags=D.default_flags(mesh)), **kw)


def _denoise_cases(rt, O, name, cases):
    """One init; per (what, src, parameters): denoiseFrame with src passed explicitly and out == in.  Returns (first-hit mask, [(what, src, got, ref)])."""
    g, origin, dn, mesh = D.frame_inputs(rt, O, name)
    valid = g["prim"] != R.PRIM_NONE
    res = []
    _init(rt, O, name)
    try:
        for what, src, kw in cases(valid, mesh):
            buf = src.copy()
            got = rt.denoiseFrame(buf, out=buf, **kw)
            assert got is buf
            res.append((what, src, got, D.denoise(src, g, origin, dn, **kw)))
    finally:
        rt.cleanupRenderer()
    return valid, res


# ---- 1. denoiseFrame: special pixel values ---------------------------------------------------------------------------

def test_denoise_poison_in_pixels_without_a_first_hit(rt, O):
    """random_96x64 (staircase_a has no such pixel): NaN, +-Inf, +-FLT_MAX, 1e30 and two NaNs with payloads in 40 pixels without a first hit, the default 5
    iterations, with and without the colour weight.  No first-hit pixel of the reference holds a non-finite word, so this is plain bit equality; the poisoned
    pixels come back with their exact bits.  A rejected tap multiplied by a zero weight instead of selected away fails here."""
    valid, res = _denoise_cases(rt, O, "random_96x64", lambda valid, mesh: [
        (f"no-hit poison {kw}", S.edge_image("no_hit_poison", valid, 70), _denoise_kw(mesh, **kw)) for kw in (dict(), dict(sigma_c=0.0))])
    for what, src, got, ref in res:
        _same(got, ref, what)
        assert np.isfinite(got[valid]).all() and np.array_equal(_bits(got[~valid]), _bits(src[~valid]))


def test_denoise_stale_records_of_pixels_that_lost_their_first_hit(rt, O):
    """The second colour buffer of the iterations is written for first-hit pixels only, so a pixel without a first hit keeps whatever an earlier call left there,
    and a tap on it loads that before the select drops it.  random_50x37: an all-NaN frame under the sequence's camera 0 (2 iterations) leaves NaN in every
    first-hit entry of both buffers; under camera 2 some of those pixels have no first hit any more and lie in the tap sets of pixels that have.  A finite
    frame there comes out as the reference's, without a NaN."""
    name = "random_50x37"
    (cam0, g0, _, _), (cam2, g2, origin, dn) = (A.sequence_inputs(rt, O, name, k) for k in (0, 2))
    was, valid = g0["prim"] != R.PRIM_NONE, g2["prim"] != R.PRIM_NONE
    assert (was & ~valid).sum() > 0
    src = S.synthetic(74, *valid.shape)
    _init(rt, O, name)
    try:
        first = rt.denoiseFrame(np.full(src.shape, np.nan, np.float32), iterations=2)
        rt.setCamera(cam2)
        got = [rt.denoiseFrame(src, **kw) for kw in (dict(), dict(iterations=2))]
    finally:
        rt.cleanupRenderer()
    assert np.isnan(first[was]).all()
    for out, kw in zip(got, (dict(), dict(iterations=2))):
        _same(out, D.denoise(src, g2, origin, dn, **_denoise_kw(False, **kw)), f"stale records {kw}")
        assert np.isfinite(out).all()


@pytest.mark.parametrize("name", DENOISE_FRAMES)
def test_denoise_finite_extremes(rt, O, name):
    """Denormals of both signs, the smallest denormal, both zeros, negative radiance, 1e-30, +-1e15 and 6e4 in 30 first-hit pixels, flags 0 and 3, 5 iterations."""
    valid, res = _denoise_cases(rt, O, name, lambda valid, mesh: [
        (f"{name} finite extremes, flags {flags}", S.edge_image("finite_extremes", valid, 71), _denoise_kw(mesh, flags=flags)) for flags in (0, 3)])
    for what, src, got, ref in res:
        _same(got, ref, what)
        assert np.isfinite(got).all()


@pytest.mark.parametrize("name", DENOISE_FRAMES)
def test_denoise_all_denormal_image(rt, O, name):
    """uniform(0, 4) * 1e-39: every input word a denormal.  Bit equality, and every first-hit word of the GPU's result a non-zero denormal - but for staircase_a
    with DEMODULATE, where albedos at the floor of 0.01 lift demodulated neighbours a hundredfold and the filter carries them to pixels of albedo near 1: there
    every word is non-zero and more than nine in ten are denormals (tests/test_preview_edges_reference.py has the reference's share)."""
    valid, res = _denoise_cases(rt, O, name, lambda valid, mesh: [
        (flags, S.edge_image("denormal", valid, 72), _denoise_kw(mesh, flags=flags)) for flags in (3, 0)])
    for flags, src, got, ref in res:
        _same(got, ref, f"{name} all-denormal image, flags {flags}")
        share = float(S.is_denormal(got[valid]).mean())
        print(f"{name} flags {flags}: denormal share of the first-hit words {share}")
        assert (got[valid] != 0).all()
        assert share == 1.0 or (name == "staircase_a" and flags & D.DEMODULATE and share > 0.9)


@pytest.mark.parametrize("name", DENOISE_FRAMES)
def test_denoise_poison_in_first_hit_pixels(rt, O, name):
    """NaN, +-Inf, +-FLT_MAX and 1e30 in one first-hit pixel each, 1 and 2 iterations, with and without the colour weight, 0 and 5 squarings of the normal
    weight: the definition carries a non-finite value to every pixel whose tap set holds it, whatever the tap's weight (0 * NaN).  The NaN words are the
    reference's, every other word is bit-equal."""
    valid, res = _denoise_cases(rt, O, name, lambda valid, mesh: [
        (f"{name} poison {kw}", S.edge_image("poison", valid, 73), _denoise_kw(mesh, **kw)) for kw in POISON_CASES])
    for what, src, got, ref in res:
        S.same_but_nan(got, ref, what, valid, S.NAN_CAP)


# ---- 2. accumulateFrame: special pixel values --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ACCUMULATE_SEQUENCES)
@pytest.mark.parametrize("flags", [3, 0])
def test_accumulate_special_values_over_a_sequence(rt, O, name, flags):
    """Three calls along the sequence, each with NaN, +-Inf, +-FLT_MAX, 1e30, the finite extremes and two NaNs with payloads in one first-hit pixel each and
    (random_50x37) again in pixels without a first hit, injected afresh per call; then a fourth call with a finite image, which must still equal the reference:
    a NaN in the history stays where the definition says it stays; then rtResetHistory and a finite call, which holds no NaN at all.  out: the reference's NaN
    words, every other word bit-equal; N: bit-equal and finite; pixels without a first hit: the input's bits, payloads included."""
    res = []
    _init(rt, O, name)
    try:
        acc = A.Accumulator()
        for n, k in enumerate(S.EDGE_CALLS[name] + (S.EDGE_CALLS[name][-1],)):
            cam, g, origin, dn = A.sequence_inputs(rt, O, name, k)
            valid = g["prim"] != R.PRIM_NONE
            src = S.edge_image("everything", valid, 80 + n) if n < 3 else S.synthetic(80 + n, *valid.shape)
            if n == 4:
                rt.reset_history()
                acc.reset()
            rt.setCamera(cam)
            buf = src.copy()
            got, hist = rt.accumulateFrame(buf, out=buf, history=True, flags=flags)
            assert got is buf
            res.append((valid, src, got, hist) + acc.step(src, g, cam, origin, dn, flags=flags))
    finally:
        rt.cleanupRenderer()
    for n, (valid, src, got, hist, ref, N) in enumerate(res):
        S.same_but_nan(got, ref, f"{name} flags {flags} call {n} out", valid, S.NAN_CAP)
        _same(hist, N, f"{name} flags {flags} call {n} history")
        assert np.isfinite(hist).all()
        assert np.array_equal(_bits(got[~valid]), _bits(src[~valid]))
    assert np.isnan(res[3][2]).any() and np.isfinite(res[3][1]).all()          # the fourth call: a finite input, the history's NaNs
    assert not np.isnan(res[4][2]).any() and float(res[4][3].max()) == 1.0     # after the reset: a first call


# ---- 3. images smaller than a tile -------------------------------------------------------------------------------------

def _guide_planes(rt, mesh):
    mask = rt.RT_GUIDE_ALBEDO | rt.RT_GUIDE_NORMAL | rt.RT_GUIDE_DEPTH | rt.RT_GUIDE_PRIM
    return rt.renderGuides(mask | rt.RT_GUIDE_NODES if mesh else mask)


def _tiny_calls(rt, frames, mesh, nx, ny):
    """After init: renderGuides under both cameras, denoiseFrame with the defaults and with 8 iterations under the first, two accumulateFrame calls along the
    cameras, all inputs explicit.  Returns the (what, got, reference, is a dict of planes) list."""
    res = []
    kw = _denoise_kw(mesh)
    for k, (cam, g, origin, dn) in enumerate(frames):
        rt.setCamera(cam)
        res.append((f"guides, camera {k}", _guide_planes(rt, mesh), g))
    cam, g, origin, dn = frames[0]
    rt.setCamera(cam)
    for n, more in enumerate((dict(), dict(iterations=8))):
        src = S.synthetic(90 + n, ny, nx)
        buf = src.copy()
        rt.denoiseFrame(buf, out=buf, **dict(kw, **more))
        res.append((f"denoise {more}", buf, D.denoise(src, g, origin, dn, **dict(kw, **more))))
    acc = A.Accumulator()
    for k, (cam, g, origin, dn) in enumerate(frames):
        rt.setCamera(cam)
        src = S.synthetic(92 + k, ny, nx)
        buf = src.copy()
        got, hist = rt.accumulateFrame(buf, out=buf, history=True)
        ref, N = acc.step(src, g, cam, origin, dn, flags=D.default_flags(mesh))
        res += [(f"accumulate call {k} out", got, ref), (f"accumulate call {k} history", hist, N)]
    return res


def _compare(res, size):
    for what, got, ref in res:
        if isinstance(ref, dict):
            assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
            for plane in ref:
                _same(got[plane], ref[plane], f"{size} {what}: plane {plane}")
        else:
            _same(got, ref, f"{size} {what}")


@pytest.mark.parametrize("nx,ny", S.TINY_SIZES)
def test_tiny_sphere_frames(rt, O, nx, ny):
    """The random-spheres scene at sizes below one tile, a 1-pixel row and column, a tile minus one, one tile, a tile plus one in both directions, two tiles
    plus one: the accumulate kernel's x >= -1 / i0 = -1 / inside[k] paths and the denoiser's read of the pixel's own record carry most of the taps; the guide
    launch's one partition of ny rows is shorter than a stripe.  At 9 x 1 also the NULL input: the framebuffer of runRenderer(1)."""
    sp, mt, frames = S.tiny_spheres(rt, O, nx, ny)
    fb = rt.initRendererSpheres(sp, mt, frames[0][0], nx, ny, 20)
    try:
        res = _tiny_calls(rt, frames, False, nx, ny)
        if (nx, ny) == (9, 1):
            rt.reset_history()
            acc = A.Accumulator()
            for k, (cam, g, origin, dn) in enumerate(frames):
                rt.setCamera(cam)
                rt.runRenderer(1)
                frame = np.array(fb, copy=True)
                got, hist = rt.accumulateFrame(history=True)
                den = rt.denoiseFrame()
                assert np.array_equal(_bits(fb), _bits(frame))
                ref, N = acc.step(frame, g, cam, origin, dn, flags=D.default_flags(False))
                res += [(f"NULL input, accumulate call {k} out", got, ref), (f"NULL input, accumulate call {k} history", hist, N),
                        (f"NULL input, denoise {k}", den, D.denoise(frame, g, origin, dn, **_denoise_kw(False)))]
    finally:
        rt.cleanupRenderer()
    _compare(res, f"{nx}x{ny}")


@pytest.mark.parametrize("nx,ny", S.TINY_MESH_SIZES)
def test_tiny_mesh_frames(rt, O, nx, ny):
    """The 300 loose triangles over the floor plane at 7 x 3 and 33 x 9: the same three checks through the mesh guide kernel (the node plane included)."""
    f, frames = S.tiny_mesh(rt, O, nx, ny)
    ks, keep = rt.make_kernel_scene(f["hm"], f["mats"], f["tex"], floor=f["floor"])
    rt.initRenderer(ks, frames[0][0], nx, ny, 16, keepalive=keep)
    try:
        rt.setRenderOptions(rt.getDefaultRenderOptions(False), floor=1)
        res = _tiny_calls(rt, frames, True, nx, ny)
    finally:
        rt.cleanupRenderer()
    _compare(res, f"{nx}x{ny} mesh")
