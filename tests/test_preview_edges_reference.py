"""CPU checks that the references of denoiseFrame and accumulateFrame (tests/denoise_reference.py, tests/accumulate_reference.py) are fit to judge the kernels
on the inputs of tests/test_gpu_preview_edges.py: non-finite and extreme pixel values, and images smaller than the kernels' 32 x 8 tile.  The vectorised
references against their per-pixel scalar restatements on such inputs, and - from the references alone - the conditions the GPU module relies on, so that a
change of scene or seed that breaks one of them fails here."""
import numpy as np
import pytest

import accumulate_reference as A
import denoise_reference as D
import guides_reference as R
import preview_support as S
from preview_support import bits as _bits, same as _same

SCALAR_SIZES = ((1, 1), (1, 9), (9, 1), (7, 3), (33, 9))
DENOISE_FRAMES = ("random_96x64", "staircase_a")
ACCUMULATE_SEQUENCES = ("random_50x37", "staircase_a")
POISON_CASES = [dict(iterations=it, sigma_c=sc, normal_squarings=sq) for it in (1, 2) for sc in (1.0, 0.0) for sq in (0, 5)]


def _denoise_kw(mesh, **kw):
    return dict(dict(D.DEFAULTS, flags=D.default_flags(mesh)), **kw)


# ---- the vectorised references against the scalar restatements ---------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 3])
def test_denoise_scalar_restatement_agrees_on_special_values(rt, O, flags):
    """`tie` with POISON and FINITE_EXTREMES in one first-hit pixel each, 2 iterations: the same NaN words, every other word bit-equal.  (No cap on the NaN
    share here: two iterations carry each of the six non-finite values over up to 13 x 13 of the frame's 40 x 24 pixels, and the words that are left - about
    half - are still compared.)"""
    g, origin, dn, mesh = D.frame_inputs(rt, O, "tie")
    valid = g["prim"] != R.PRIM_NONE
    src = S.synthetic(21, *valid.shape)
    S.inject(src, valid, 22, S.POISON + S.FINITE_EXTREMES)
    a = D.denoise(src, g, origin, dn, **_denoise_kw(mesh, iterations=2, flags=flags))
    b = D.denoise_scalar(src, g, origin, dn, **_denoise_kw(mesh, iterations=2, flags=flags))
    assert np.isnan(a).any() and 0 < valid.sum() < valid.size
    S.same_but_nan(b, a, f"tie flags {flags}", valid, 1.0)
    assert S.nan_share(a, valid) < 0.75


@pytest.mark.parametrize("flags", [0, 3])
def test_accumulate_scalar_restatement_agrees_on_special_values(rt, O, flags):
    """Three calls of the `tie` sequence, the values injected afresh per call: out and N of every call, the same way."""
    acc, ref = A.Accumulator(scalar=True), A.Accumulator()
    nans = 0
    for k in range(3):
        cam, g, origin, dn = A.sequence_inputs(rt, O, "tie", k)
        valid = g["prim"] != R.PRIM_NONE
        src = S.synthetic(30 + k, *valid.shape)
        S.inject(src, valid, 40 + k, S.POISON + S.FINITE_EXTREMES)
        a, Na = ref.step(src, g, cam, origin, dn, flags=flags)
        b, Nb = acc.step(src, g, cam, origin, dn, flags=flags)
        S.same_but_nan(b, a, f"tie flags {flags} call {k} out", valid, 1.0)
        S.same_but_nan(Nb, Na, f"tie flags {flags} call {k} history", valid, 0.0)
        nans += int(np.isnan(a).sum())
    assert nans > 0


@pytest.mark.parametrize("nx,ny", SCALAR_SIZES)
def test_scalar_restatements_agree_at_tiny_sizes(rt, O, nx, ny):
    """Finite uniform [0, 4) input below and around one tile: plain bit equality of both pairs."""
    sp, mt, frames = S.tiny_spheres(rt, O, nx, ny)
    cam, g, origin, dn = frames[0]
    src = S.synthetic(50, ny, nx)
    for kw in (dict(), dict(iterations=8, flags=0)):
        _same(D.denoise_scalar(src, g, origin, dn, **_denoise_kw(False, **kw)), D.denoise(src, g, origin, dn, **_denoise_kw(False, **kw)), f"{nx}x{ny} denoise {kw}")
    acc, ref = A.Accumulator(scalar=True), A.Accumulator()
    for k, (cam, g, origin, dn) in enumerate(frames):
        src = S.synthetic(51 + k, ny, nx)
        a, Na = ref.step(src, g, cam, origin, dn)
        b, Nb = acc.step(src, g, cam, origin, dn)
        _same(b, a, f"{nx}x{ny} accumulate call {k} out")
        _same(Nb, Na, f"{nx}x{ny} accumulate call {k} history")


# ---- the conditions the GPU module relies on ---------------------------------------------------------------------------

def _tiny_conditions(frames, mesh, nx, ny):
    """Every call with a history has candidates and taps outside the image, the last call blends, the denoiser has taps outside the image."""
    assert (frames[0][1]["prim"] != R.PRIM_NONE).any()
    acc = A.Accumulator()
    for k, (cam, g, origin, dn) in enumerate(frames):
        cnt = {}
        acc.step(S.synthetic(60 + k, ny, nx), g, cam, origin, dn, flags=D.default_flags(mesh), counts=cnt)
        if k:
            print(f"{nx}x{ny} call {k}", {key: cnt[key] for key in A.COUNTS})
            assert cnt["candidate"] > 0 and cnt["outside"] > 0, cnt
    assert cnt["blended"] > 0, cnt
    cnt = {}
    cam, g, origin, dn = frames[0]
    D.denoise(S.synthetic(62, ny, nx), g, origin, dn, counts=cnt, **_denoise_kw(mesh))
    print(f"{nx}x{ny} denoise", {key: cnt[key] for key in D.COUNTS})
    assert cnt["outside"] > 0, cnt


@pytest.mark.parametrize("nx,ny", S.TINY_SIZES)
def test_tiny_sphere_frames_exercise_the_image_border(rt, O, nx, ny):
    _tiny_conditions(S.tiny_spheres(rt, O, nx, ny)[2], False, nx, ny)


@pytest.mark.parametrize("nx,ny", S.TINY_MESH_SIZES)
def test_tiny_mesh_frames_exercise_the_image_border(rt, O, nx, ny):
    _tiny_conditions(S.tiny_mesh(rt, O, nx, ny)[1], True, nx, ny)


def test_poison_in_no_hit_pixels_stays_there(rt, O):
    """random_96x64, 40 poisoned pixels without a first hit, 5 iterations, with and without the colour weight: no non-finite word in a first-hit pixel of the
    reference, and the pixels without a first hit are the input's bits, payloads included.  (staircase_a has no pixel without a first hit.)"""
    g, origin, dn, mesh = D.frame_inputs(rt, O, "random_96x64")
    valid = g["prim"] != R.PRIM_NONE
    assert (D.frame_inputs(rt, O, "staircase_a")[0]["prim"] != R.PRIM_NONE).all()
    src = S.edge_image("no_hit_poison", valid, 70)
    assert int((~np.isfinite(src)).any(axis=-1)[~valid].sum()) == 25 and np.isfinite(src[valid]).all()       # (+-FLT_MAX and 1e30 are finite: 15 of the 40)
    for kw in (dict(), dict(sigma_c=0.0)):
        ref = D.denoise(src, g, origin, dn, **_denoise_kw(mesh, **kw))
        assert np.isfinite(ref[valid]).all()
        assert np.array_equal(_bits(ref[~valid]), _bits(src[~valid]))


def test_camera_move_takes_the_first_hit_from_pixels_next_to_others(rt, O):
    """random_50x37, cameras 0 and 2 of the sequence: pixels with a first hit under the first and none under the second exist, and some are taps of the second
    iteration (stride 2: the first to read the buffer the prologue does not write) of a pixel that has one (the stale-record test of the GPU module relies on
    it)."""
    was, valid = (A.sequence_inputs(rt, O, "random_50x37", k)[1]["prim"] != R.PRIM_NONE for k in (0, 2))
    lost = was & ~valid
    ny, nx = valid.shape
    reached = np.zeros_like(valid)
    for j, i in np.argwhere(lost):
        for dy in (-4, -2, 0, 2, 4):
            for dx in (-4, -2, 0, 2, 4):
                if 0 <= j + dy < ny and 0 <= i + dx < nx:
                    reached[j + dy, i + dx] = True
    print(int(lost.sum()), "pixels lost their first hit,", int((reached & valid).sum()), "first-hit pixels have one among their stride-2 taps")
    assert lost.sum() > 0 and (reached & valid).sum() > 0


@pytest.mark.parametrize("name", DENOISE_FRAMES)
def test_finite_extremes_and_denormals_stay_finite(rt, O, name):
    """FINITE_EXTREMES in 30 first-hit pixels: no non-finite output word and at least one denormal one, with flags 0 and 3.  The all-denormal image comes out
    with every first-hit word non-zero, and a denormal - but for staircase_a with DEMODULATE, where a neighbour's albedo at the floor of 0.01 lifts the
    demodulated value a hundredfold and the filter carries it to pixels of albedo near 1: there most words are denormals."""
    g, origin, dn, mesh = D.frame_inputs(rt, O, name)
    valid = g["prim"] != R.PRIM_NONE
    for flags in (0, 3):
        src = S.edge_image("finite_extremes", valid, 71)
        ref = D.denoise(src, g, origin, dn, **_denoise_kw(mesh, flags=flags))
        print(name, flags, "denormal words in", int(S.is_denormal(src).sum()), "out", int(S.is_denormal(ref).sum()))
        assert np.isfinite(ref).all() and S.is_denormal(ref).any()
        src = S.edge_image("denormal", valid, 72)
        assert S.is_denormal(src).all()
        ref = D.denoise(src, g, origin, dn, **_denoise_kw(mesh, flags=flags))
        share = float(S.is_denormal(ref[valid]).mean())
        print(name, flags, "denormal share of the first-hit words", share)
        assert (ref[valid] != 0).all() and np.isfinite(ref).all()
        assert share == 1.0 or (name == "staircase_a" and flags & D.DEMODULATE and share > 0.9)


@pytest.mark.parametrize("name", DENOISE_FRAMES)
def test_poison_in_first_hit_pixels_spreads_but_stays_under_the_cap(rt, O, name):
    """Each value of POISON in one first-hit pixel: in every parameter set of the GPU test the reference has a first-hit pixel that is NaN with a finite
    input (spreading is exercised), and its NaN share stays under the cap."""
    g, origin, dn, mesh = D.frame_inputs(rt, O, name)
    valid = g["prim"] != R.PRIM_NONE
    src = S.edge_image("poison", valid, 73)
    for kw in POISON_CASES:
        ref = D.denoise(src, g, origin, dn, **_denoise_kw(mesh, **kw))
        spread = int((np.isnan(ref).any(axis=-1) & np.isfinite(src).all(axis=-1) & valid).sum())
        print(name, kw, "NaN share %.4f, %d pixels NaN with a finite input" % (S.nan_share(ref, valid), spread))
        assert spread > 0 and S.nan_share(ref, valid) <= S.NAN_CAP


@pytest.mark.parametrize("name", ACCUMULATE_SEQUENCES)
@pytest.mark.parametrize("flags", [3, 0])
def test_accumulated_poison_spreads_but_stays_under_the_cap(rt, O, name, flags):
    """The calls of the GPU test from the reference alone: three poisoned calls, a finite fourth and a finite call after a reset.  The NaN share of every call
    stays under the cap, N stays finite, some first-hit pixel is NaN where its input is finite, a NaN of the history is still there in the fourth call and
    none after the reset."""
    acc = A.Accumulator()
    spread = 0
    for n, k in enumerate(S.EDGE_CALLS[name]):
        cam, g, origin, dn = A.sequence_inputs(rt, O, name, k)
        valid = g["prim"] != R.PRIM_NONE
        src = S.edge_image("everything", valid, 80 + n) if n < 3 else S.synthetic(80 + n, *valid.shape)
        out, N = acc.step(src, g, cam, origin, dn, flags=flags)
        here = int((np.isnan(out).any(axis=-1) & np.isfinite(src).all(axis=-1) & valid).sum())
        print(name, flags, f"call {n}: NaN share {S.nan_share(out, valid):.4f}, {here} pixels NaN with a finite input, N max {float(N.max())}")
        assert S.nan_share(out, valid) <= S.NAN_CAP and np.isfinite(N).all()
        assert np.array_equal(_bits(out[~valid]), _bits(src[~valid]))
        spread += here
    assert spread > 0 and here > 0                              # (the fourth call's input is finite: its NaNs are the history's)
    out, N = A.Accumulator().step(src, g, cam, origin, dn, flags=flags)
    assert not np.isnan(out).any()
