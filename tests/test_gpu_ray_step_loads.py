"""The loads of the ray step in the folded sphere kinds (k_render_spheres_queue with FORM = 1): scan_single reads the eight rounds of a
512-slot scene in one burst at immediate offsets and keeps its loop for every other round count, its exact tail reads orig[] beside the slot, shade
reads a hit's four records together, and the hit normal divides by the radius through the refined reciprocal stored beside it when the scene is staged
(rt_exactdiv.h rt_exdiv3_y), with the plain division behind one branch for a radius outside the form's window and for a numerator that is zero, tiny
or huge.  None of it may move a bit.  Every frame here is rendered twice in a row - measured, then ordered by the first frame's cost map - must report
the folded form both times and must be the CPU oracle's frame, word for word, free of NaN.  The stored-reciprocal form itself is held on the device by
the probe rtProbeExactDivStored beside the plain operator.  Helpers: tests/ray_step_support.py (the idioms of tests/test_gpu_single_ray_step.py)."""
import ctypes as C

import numpy as np
import pytest

import radiance_reference as RR
import ray_step_support as S

pytestmark = pytest.mark.gpu
FLT_MAX = 3.4028234663852886e38


# ---- sphere counts: the eight-read burst and the loop on both sides of it ------------------------------------------------------------

def _n_with_rounds(rt, want):
    """The smallest n whose first n spheres (S.first_n) make `want` rounds of 64 slots, by the padding rule restated on the CPU."""
    for n in range(2, 600):
        if S.rounds(S.first_n(rt, n)[0]) == want:
            return n
    raise AssertionError(want)


def _frame_and_one_pixel(rt, O, sp, mt, what):
    """32x24 at 8 samples, one workgroup.  Where the oracle cannot show that a wave of that frame ends on one live lane, the scene is rendered as a frame
    of ONE pixel as well: its wave has one live lane for every ray of the frame."""
    nx, ny, ns = 32, 24, 8
    alone = S.a_wave_ends_on_one_lane(O, sp, mt, S.camera(rt, nx, ny), nx, ny, ns)
    S.check(rt, O, sp, mt, nx, ny, ns, what=what)
    if not alone:
        S.check(rt, O, sp, mt, 1, 1, ns, what=what + ", one pixel")


@pytest.mark.parametrize("want", [7, 8, 9])
def test_round_counts_around_the_burst(rt, O, want):
    """n chosen on the CPU so that n_padded >> 6 is 7, 8 and 9: the loop below the burst, the burst, the loop above it."""
    n = _n_with_rounds(rt, want)
    sp, mt = S.first_n(rt, n)
    assert len(sp) == n and S.n_padded(sp) >> 6 == want, (n, S.n_padded(sp))
    _frame_and_one_pixel(rt, O, sp, mt, f"{n} spheres, {want} rounds")


def test_the_three_round_counts_are_distinct_scenes(rt):
    ns = [_n_with_rounds(rt, w) for w in (7, 8, 9)]
    assert [S.rounds(S.first_n(rt, n)[0]) for n in ns] == [7, 8, 9] and len(set(ns)) == 3, ns


@pytest.mark.parametrize("n,want", [(1, 1), (64, 2), (65, 2), (488, 8)])
def test_named_sphere_counts(rt, O, n, want):
    """One sphere, a full round of small spheres and one more, and the whole scene (the benchmark's: eight rounds, the burst)."""
    sp, mt = S.first_n(rt, n)
    assert len(sp) == n and S.rounds(sp) == want, (n, S.n_padded(sp))
    _frame_and_one_pixel(rt, O, sp, mt, f"{n} spheres")


# ---- lone-wave steps ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny,ns", [(96, 64, 16), (13, 7, 16), (1, 1, 16)])
def test_close_up(rt, O, nx, ny, ns):
    """The close-up (tests/test_gpu_sphere_form.py holds, with the oracle, that 96x64 puts pixels on chain list 0: one-pixel waves trace whole pixels in
    the single-ray step), one workgroup with partial tiles, and one pixel: a wave that has one live lane from its first ray to its last."""
    sp, mt = S.scene(rt)
    assert S.rounds(sp) == 8
    S.check(rt, O, sp, mt, nx, ny, ns, lean=3, what=f"{nx}x{ny}")


# ---- every branch behind the hoisted loads -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,param", [("diffuse", 0.0), ("metal", 0.0), ("metal", 0.3), ("glass", 1.5)], ids=["diffuse", "metal_mirror", "metal_fuzz", "glass"])
def test_single_material_scenes(rt, O, name, param):
    """16x16 of the close-up with every sphere but the ground made diffuse / metal without and with fuzz / glass: each material's branch reads the records
    that shade loaded ahead of the hit point.  Where the oracle cannot show that a wave of the frame ends on one live lane, the scene is rendered as a frame
    of one pixel as well."""
    nx, ny, ns = 16, 16, 8
    sp, mt = S.scene(rt)
    m2 = mt.copy()
    m2["type"][1:] = {"diffuse": rt.RT_DIFFUSE, "metal": rt.RT_METAL, "glass": rt.RT_GLASS}[name]
    m2["param"][1:] = param
    alone = S.a_wave_ends_on_one_lane(O, sp, m2, S.camera(rt, nx, ny), nx, ny, ns)
    S.check(rt, O, sp, m2, nx, ny, ns, what=name)
    if not alone:
        S.check(rt, O, sp, m2, 1, 1, ns, what=name + ", one pixel")


# ---- the plain-division branch of the stored reciprocal --------------------------------------------------------------------------------

def test_radii_outside_the_window_take_the_marker(rt, O):
    """A sphere of radius 2^45 (above the window: its slot holds the marker, every hit on it divides plainly) and one of 2^-45 (below it) beside the
    scene's ordinary spheres (radii 0.2 to 1000: the stored reciprocal).  The oracle says that both kinds of hit are in the frame: it differs from the
    frame without the giant sphere and from the frame of the giant alone.  (Nothing hits the tiny sphere - the frame is the oracle's frame without it;
    below the window the device is held by the probe, test_stored_reciprocal_probe.)"""
    nx, ny, ns = 32, 24, 8
    sp, mt = S.scene(rt)
    n = len(sp)
    s2, m2 = np.concatenate([sp, sp[:2]]), np.concatenate([mt, mt[:2]])
    s2["center"][n], s2["radius"][n] = (0.9, 0.45, 0.8), 2.0 ** -45
    s2["center"][n + 1], s2["radius"][n + 1] = (-2.0 ** 45, 0.0, 0.0), 2.0 ** 45
    m2["type"][n:] = rt.RT_DIFFUSE
    m2["color"][n:] = (0.9, 0.2, 0.2)
    m2["param"][n:] = 0.0
    cam = S.camera(rt, nx, ny)
    full = S.oracle(O, s2, m2, cam, nx, ny, ns)
    assert not np.array_equal(S.bits(full), S.bits(S.oracle(O, s2[:n + 1], m2[:n + 1], cam, nx, ny, ns)))      # the giant sphere is hit
    assert not np.array_equal(S.bits(full), S.bits(S.oracle(O, s2[n:], m2[n:], cam, nx, ny, ns)))              # ordinary spheres are hit
    assert np.array_equal(S.bits(full), S.bits(S.oracle(O, np.delete(s2, n), np.delete(m2, n), cam, nx, ny, ns)))   # the tiny one is not
    S.check(rt, O, s2, m2, nx, ny, ns, what="radii 2^-45 and 2^45")


def _axis_scene(rt):
    """A diffuse sphere on the z axis above a ground sphere, and a metal one beside it."""
    sp = np.zeros(3, rt.sphere_dtype)
    mt = np.zeros(3, rt.material_dtype)
    sp["center"] = [(0, -100.5, 2), (0, 0, 2), (1.1, 0, 2.2)]
    sp["radius"] = [100, 0.5, 0.5]
    mt["type"] = [rt.RT_DIFFUSE, rt.RT_DIFFUSE, rt.RT_METAL]
    mt["color"] = [(0.8, 0.8, 0.0), (0.7, 0.3, 0.3), (0.8, 0.8, 0.8)]
    mt["param"] = [0.0, 0.0, 0.1]
    return sp, mt


def test_a_hit_offset_with_zero_components(rt, O):
    """A caller's ray along +z through the centre of a sphere on the z axis (radianceRays, 4 samples): the first hit's offset hp - c has two components
    that are exactly zero - shown first with the oracle's own sphereHit - which is outside the window of the shared-reciprocal forms: the quotient is the
    plain division's.  The result is the oracle's, bit for bit."""
    sp, mt = _axis_scene(rt)
    org = np.array([[0.0, 0.0, -1.0]], np.float32)
    d = np.array([[0.0, 0.0, 1.0]], np.float32)
    T = org + d
    # on the CPU: the oracle's t of that ray on sphere 1, the hit point as ray.h:12 rounds it, the offset
    lib = O.load_oracle()
    fp = C.POINTER(C.c_float)
    s1 = np.ascontiguousarray(sp[1:2], dtype=rt.sphere_dtype)
    t = np.float32(lib.orc_sphere_hit(C.cast(s1.ctypes.data, C.POINTER(rt.sphere)), org[0].ctypes.data_as(fp), d[0].ctypes.data_as(fp), C.c_float(0.001), C.c_float(FLT_MAX)))
    assert 0.0 < t < FLT_MAX
    hp = np.array([org[0][a] + t * d[0][a] for a in range(3)], np.float32)
    off = hp - sp["center"][1].astype(np.float32)
    assert off[0] == 0.0 and off[1] == 0.0 and off[2] != 0.0, off
    ref_out, ref_rays = RR.oracle_rays_in(O.sphere_scene(sp, mt), O.default_options(True), S.DEPTH, org, T, None, 4)
    assert ref_rays[0] >= 8                                          # every sample hits the sphere first and bounces
    rt.initRendererSpheres(sp, mt, S.camera(rt, 8, 8), 8, 8, S.DEPTH)
    try:
        out, _, rays = rt.radiance_rays(org, d, 4, rays=True)
    finally:
        rt.cleanupRenderer()
    S.same(out, ref_out, "the axis ray against the oracle")
    assert np.array_equal(rays, ref_rays)


def test_the_axis_scene_as_folded_frames(rt, O):
    """The same three spheres as frames of the folded kinds (16x16 and one pixel, 8 samples): a scene of one round."""
    sp, mt = _axis_scene(rt)
    assert S.rounds(sp) == 1
    cam = rt.make_camera((0, 0, -1), (0, 0, 2), (0, 1, 0), 40.0, 1.0, 0.0, 3.0)
    for nx, ny in ((16, 16), (1, 1)):
        ref = S.oracle(O, sp, mt, cam, nx, ny, 8)
        measured, ordered = S.two_frames(rt, sp, mt, cam, nx, ny, 8)
        S.same(measured, ref, f"{nx}x{ny} measured")
        S.same(ordered, ref, f"{nx}x{ny} ordered by the map")


# ---- the stored-reciprocal form on the device ----------------------------------------------------------------------------------------

def _probe_operands():
    """2^16 operand sets (x, y, z, radius): numerators and radii with exponents spread over and beyond the window [2^-40, 2^40], then rows with the radius
    at, next to and beyond both ends of the window, and rows with denormal, zero, infinite and NaN numerators."""
    n = 1 << 16
    rng = np.random.default_rng(328)
    v = np.empty((n, 4), np.float32)
    mant = rng.uniform(1.0, 2.0, (n, 4))
    expo = np.concatenate([rng.integers(-44, 45, (n, 3)), rng.integers(-44, 45, (n, 1))], axis=1)
    sign = np.where(rng.random((n, 4)) < 0.5, -1.0, 1.0)
    sign[:, 3] = 1.0
    v[:] = (sign * np.ldexp(mant, expo)).astype(np.float32)
    v[: n // 2, :3] = (sign[: n // 2, :3] * rng.uniform(1e-3, 1e3, (n // 2, 3))).astype(np.float32)     # half: numerators of a scene's size
    v[: n // 4, 3] = rng.uniform(0.05, 1000.0, n // 4).astype(np.float32)                                # a quarter: radii of a scene's size too
    lo, hi = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
    ends = [lo, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(1)), hi, np.nextafter(hi, np.float32(0)), np.nextafter(hi, np.float32(np.inf)),
            np.float32(0.0), np.float32(np.inf), np.float32(np.nan), np.float32(-1.0), np.float32(1e-42), np.float32(2.0 ** 45), np.float32(2.0 ** -45)]
    for k, r in enumerate(ends * 16):
        v[n // 2 + k, 3] = r
    special = [np.float32(0.0), np.float32(-0.0), np.float32(1e-42), np.float32(-1e-45), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)]
    for k in range(7 * 3 * 8):
        row = n // 2 + 4096 + k
        v[row, (k // 7) % 3] = special[k % 7]
        if k >= 7 * 3 * 4:
            v[row, 3] = np.float32(0.5)                                # ... half of them over a radius inside the window
    return v


def test_stored_reciprocal_probe(rt):
    """rtProbeExactDivStored: the reciprocal from one kernel launch, the quotients from a second launch that reads it back, the plain operator beside them.
    Bit-equal on every row; the stored word is the marker exactly for the radii outside the window."""
    v = _probe_operands()
    assert len(v) == 1 << 16
    out = rt.Probe("parity").exactdiv_stored(v)
    q, plain, y = S.bits(out[:, 0:3]), S.bits(out[:, 3:6]), out[:, 6]
    bad = np.flatnonzero((q != plain).any(axis=1))
    assert bad.size == 0, (bad.size, v[bad[:4]], out[bad[:4]])
    r = v[:, 3]
    inside = (r >= np.float32(2.0 ** -40)) & (r <= np.float32(2.0 ** 40))
    assert np.array_equal(np.isnan(y), ~inside)
    a = np.abs(v[:, :3])
    taken = inside & (a.sum(axis=1, dtype=np.float32) <= np.float32(2.0 ** 40)) & (a.min(axis=1) >= np.float32(2.0 ** -40))
    assert taken.mean() > 0.4 and (~taken).mean() > 0.1, (taken.mean(),)       # both sides of the guard are populated
