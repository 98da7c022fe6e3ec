"""The bounce's divisions by a special divisor (csrc/rt_exactdiv.h) on the device: the probe holds each form against the plain operators on the same operands,
bit for bit ("bits" = float32 words), and whole frames are held against the CPU oracle as the other sphere tests do - the benchmark scene, radii of every
size, a camera whose rays lie in a plane through the spheres' centres (hit normals and reflections with a zero component: the plain path), scenes scaled
out of the operand window, t_min = 0, a grid of six workgroups and a mesh frame (material_scatter is shared with the mesh kernel, which keeps unit()).
The frames take the cost-ordered dispatch (8 spp), whose folded kinds are the kernels that use the header."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ONE = 0x3F800000
NS = 8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_words(a, b):
    a, b = _bits(a), _bits(b)
    nan = lambda w: (w & 0x7FFFFFFF) > 0x7F800000
    return (a == b) | (nan(a) & nan(b))                                   # (a NaN's payload is never looked at)


def _same(got, ref, what=""):
    assert not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    assert np.array_equal(_bits(got), _bits(ref)), (what, int(np.count_nonzero(_bits(got) != _bits(ref))))


# ---- the probe ---------------------------------------------------------------------------------------------------------------------------------------

def _operand_sets():
    """About 2^20 sets (x, y, z, l): bounce vectors over the benchmark's radii, hit offsets over their radius, numerators over every a next to 1, operands on
    both sides of each guard and the special values, and raw bit patterns."""
    rng = np.random.default_rng(20261019)
    f32 = np.float32
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    sets = []
    n = 300_000                                                            # normal + point in the unit ball, divided by a radius
    v = unit(rng.normal(size=(n, 3))) + unit(rng.normal(size=(n, 3))) * rng.random((n, 1)) ** (1 / 3)
    sets.append(np.column_stack([v, rng.choice([0.2, 0.5, 1.0, 1000.0], n)]))
    n = 300_000                                                            # hit point - centre over the radius
    r = np.concatenate([rng.choice([0.2, 0.5, 1.0, 1000.0], n // 2), rng.uniform(0.05, 3.0, n - n // 2)])
    sets.append(np.column_stack([unit(rng.normal(size=(n, 3))) * r[:, None] * (1 + rng.normal(size=(n, 1)) * 1e-6), r]))
    n = 330_000                                                            # roots over a = 1 + k ulp, k = -6 .. 4, numerators of every size and the special values
    a = (np.uint32(ONE) + rng.integers(-6, 5, n).astype(np.int64)).astype(np.uint32).view(f32)
    x = (rng.normal(size=(n, 3)) * np.exp2(rng.integers(-30, 30, (n, 1)))).astype(f32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-38, 3.4e38, -3.4e38, 1.1754944e-38], f32)
    x[::50, 0] = special[np.arange(len(x[::50])) % len(special)]
    sets.append(np.column_stack([x, a]))
    n = 20_000                                                             # the guards from both sides: magnitudes around 2^-40, 2^-30, 2^30, 2^40, divisors alike
    edge = np.exp2(rng.choice([-45.0, -41.0, -40.0, -39.0, -30.0, 0.0, 30.0, 38.0, 39.0, 40.0, 41.0, 45.0], (n, 4))).astype(f32)
    edge = (edge.view(np.uint32) + rng.integers(-2, 3, (n, 4)).astype(np.uint32)).view(f32) * rng.choice([-1.0, 1.0], (n, 4)).astype(f32)
    sets.append(edge)
    n = 5_000                                                              # a special value in one operand
    sp = rng.normal(size=(n, 4)).astype(f32)
    sp[np.arange(n), rng.integers(0, 4, n)] = special[rng.integers(0, len(special), n)]
    sets.append(sp)
    sets.append(rng.integers(0, 2 ** 32, (90_000, 4), dtype=np.uint64).astype(np.uint32).view(f32))      # raw bit patterns
    return np.concatenate([np.ascontiguousarray(s, dtype=f32) for s in sets])


def test_probe_every_form_against_the_plain_operators(rt):
    v = _operand_sets()
    assert 2 ** 20 - 2 ** 16 <= len(v) <= 2 ** 20 + 2 ** 16
    out = rt.Probe("parity").exactdiv(v)
    x, l = v[:, 0:3], v[:, 3]
    # form C over a divisor of any size and as unit(): the device's plain operators on the same operands, and IEEE division on the host
    bad = ~_same_words(out[:, 0:3], out[:, 3:6]).all(axis=1)
    assert not bad.any(), ("vec3 / float", int(bad.sum()), v[bad][:3], out[bad][:3])
    with np.errstate(all="ignore"):
        host = x / l[:, None]
    bad = ~_same_words(out[:, 0:3], host).all(axis=1)
    assert not bad.any(), ("vec3 / float against the host", int(bad.sum()), v[bad][:3], out[bad][:3])
    bad = ~_same_words(out[:, 6:9], out[:, 9:12]).all(axis=1)
    assert not bad.any(), ("unit", int(bad.sum()), v[bad][:3], out[bad][:3])
    # the guards as the header states them: both sides are well populated
    ax = np.abs(x)
    with np.errstate(all="ignore"):
        inside = (ax.sum(axis=1, dtype=np.float32) <= 2.0 ** 40) & (ax.min(axis=1) >= 2.0 ** -40) & (l >= 2.0 ** -40) & (l <= 2.0 ** 40)
        xx = x * x
        s2 = (xx[:, 0] + xx[:, 1]) + xx[:, 2]
        inside_unit = (s2 >= 2.0 ** -60) & (s2 <= 2.0 ** 60) & (xx.min(axis=1) >= 2.0 ** -80)
    assert inside.sum() > 500_000 and (~inside).sum() > 50_000 and inside_unit.sum() > 500_000 and (~inside_unit).sum() > 50_000
    # form B: the two roots over a, against the host's IEEE quotient.  Handled a (k = -4 .. 2): the same word, bar the header's two exceptions - a zero numerator (either zero) and an infinite
    # one (inf or NaN) - which sphere_hit_exact's range test rejects alike
    k = _bits(l).astype(np.int64) - ONE
    handled = (k >= -4) & (k <= 2)
    assert all((k == kk).sum() > 20_000 for kk in range(-6, 5))
    zero_n = inf_n = 0
    for col, root in ((0, 12), (1, 13)):                                   # the two roots ride on one multiplier and one branch
        num = v[:, col]
        same = _same_words(out[:, root], host[:, col])
        zero, infinite = num == 0, np.isinf(num)
        bad = ~same & ~(handled & (zero | infinite))
        assert not bad.any(), ("root / a", col, int(bad.sum()), v[bad][:3], out[bad][:3])
        assert (out[handled & zero, root] == 0).all()
        assert not np.isfinite(out[handled & infinite, root]).any()
        zero_n, inf_n = zero_n + int((handled & zero).sum()), inf_n + int((handled & infinite).sum())
    assert zero_n > 100 and inf_n > 100


# ---- frames ------------------------------------------------------------------------------------------------------------------------------------------

_FORMS = []           # rtLastSphereForm() of every frame _frames rendered: 1 = the folded form, whose kernels use the header


def _frames(rt, O, sp, mt, cam, nx, ny, ns=NS, **opts):
    """(device frame, oracle frame) of a sphere scene at depth 50 under the same options."""
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    o = rt.getDefaultRenderOptions(True)
    rt.setRenderOptions(o, **opts)
    rt.runRenderer(ns, 8, 8)
    got = np.array(fb, copy=True)
    _FORMS.append(rt.last_sphere_form())
    rt.cleanupRenderer()
    oo = O.default_options(True)
    for key, val in opts.items():
        setattr(oo, key, val)
    ref, _ = O.render(O.sphere_scene(sp, mt), cam, oo, nx, ny, ns, 50)
    return got, ref


def test_benchmark_scene(rt, O):
    nx, ny = 64, 48
    _same(*_frames(rt, O, *rt.scene_random_spheres(nx, ny), nx, ny), "benchmark scene")


def test_benchmark_scene_in_the_folded_form(rt, O):
    """128x64 reaches every XCD: the cost-ordered dispatch runs the folded kind, the one compiled with the header's forms."""
    nx, ny = 128, 64
    got, ref = _frames(rt, O, *rt.scene_random_spheres(nx, ny), nx, ny)
    assert _FORMS[-1] == 1, _FORMS[-1]
    _same(got, ref, "benchmark scene, folded form")


def test_benchmark_scene_with_t_min_zero(rt, O):
    nx, ny = 64, 48
    _same(*_frames(rt, O, *rt.scene_random_spheres(nx, ny), nx, ny, t_min=0.0), "t_min = 0")


def test_six_workgroups(rt, O):
    nx, ny = 96, 64
    _same(*_frames(rt, O, *rt.scene_random_spheres(nx, ny), nx, ny), "96x64")


def _radii_scene(rt, nx, ny):
    """81 spheres with pseudo-random radii in [0.05, 3] of all three materials on a ground sphere."""
    rng = np.random.default_rng(7)
    n = 82
    sp = np.zeros(n, rt.sphere_dtype)
    mt = np.zeros(n, rt.material_dtype)
    sp["center"][0], sp["radius"][0] = (0, -1000, 0), 1000
    mt["type"][0], mt["color"][0] = rt.RT_DIFFUSE, (0.5, 0.5, 0.5)
    gx, gz = np.meshgrid(np.arange(-4, 5), np.arange(-4, 5))
    r = rng.uniform(0.05, 3.0, n - 1).astype(np.float32)
    sp["radius"][1:] = r
    sp["center"][1:, 0] = gx.ravel() * 2.5 + rng.uniform(-0.5, 0.5, n - 1)
    sp["center"][1:, 1] = r
    sp["center"][1:, 2] = gz.ravel() * 2.5 + rng.uniform(-0.5, 0.5, n - 1)
    mt["type"][1:] = np.array([rt.RT_DIFFUSE, rt.RT_METAL, rt.RT_GLASS])[np.arange(n - 1) % 3]
    mt["color"][1:] = rng.uniform(0.2, 0.95, (n - 1, 3))
    mt["param"][1:] = np.where(mt["type"][1:] == rt.RT_GLASS, 1.5, np.where(np.arange(n - 1) % 2 == 0, 0.0, 0.3))
    cam = rt.make_camera((13, 4, 9), (0, 1, 0), (0, 1, 0), 35.0, nx / ny, 0.05, 14.0)
    return sp, mt, cam


def test_radii_of_every_size_and_all_three_materials(rt, O):
    nx, ny = 64, 48
    _same(*_frames(rt, O, *_radii_scene(rt, nx, ny), nx, ny), "radii in [0.05, 3]")


def test_rays_in_a_plane_through_the_centres(rt, O):
    """A camera of aspect 0 on the z axis: `horizontal` is (0, 0, 0), so every primary ray lies in the plane x = 0, which holds the centres of a diffuse, a
    mirror and a glass sphere and of the ground.  Every first hit's normal, and every reflection and refraction off it, has an x of exactly zero: the guards
    send them down the plain path, inside a frame."""
    nx, ny = 64, 48
    sp = np.zeros(4, rt.sphere_dtype)
    mt = np.zeros(4, rt.material_dtype)
    sp["center"][:] = ((0, -100.5, 0), (0, 0, 0), (0, 0.1, -1.3), (0, 0, 1.2))
    sp["radius"][:] = (100, 0.5, 0.6, 0.5)
    mt["type"][:] = (rt.RT_DIFFUSE, rt.RT_METAL, rt.RT_DIFFUSE, rt.RT_GLASS)
    mt["color"][:] = ((0.8, 0.8, 0.0), (0.8, 0.6, 0.2), (0.1, 0.2, 0.5), (1, 1, 1))
    mt["param"][:] = (0.0, 0.0, 0.0, 1.5)
    cam = rt.make_camera((0, 0.3, 6), (0, 0.0, 0), (0, 1, 0), 40.0, 0.0, 0.0, 6.0)
    assert tuple(cam.horizontal.e) == (0.0, 0.0, 0.0) and cam.lower_left_corner.e[0] == 0.0 and cam.vertical.e[0] == 0.0 and cam.origin.e[0] == 0.0
    got, ref = _frames(rt, O, sp, mt, cam, nx, ny)
    assert len(np.unique(_bits(ref).reshape(-1, 3), axis=0)) > 100         # (a picture, not one colour)
    _same(got, ref, "plane x = 0")


@pytest.mark.parametrize("exponent", [-45, 45])
def test_scenes_scaled_out_of_the_window(rt, O, exponent):
    """The three spheres and their camera scaled by 2^-45 and 2^45: every radius and every hit offset lies outside the window of the shared reciprocal, the
    normal's division takes the plain path.  t_min = 0: at 2^-45 every distance of the scene is below the default."""
    nx, ny = 64, 48
    s = np.float32(2.0) ** exponent
    sp, mt, cam = rt.scene_three_spheres(nx, ny)
    sp["center"] *= s
    sp["radius"] *= s
    for v in (cam.origin, cam.lower_left_corner, cam.horizontal, cam.vertical):
        for q in range(3):
            v.e[q] = float(np.float32(v.e[q]) * s)
    cam.lens_radius = float(np.float32(cam.lens_radius) * s)
    assert sp["radius"].min() < 2.0 ** -40 if exponent < 0 else sp["radius"].min() > 2.0 ** 40
    got, ref = _frames(rt, O, sp, mt, cam, nx, ny, t_min=0.0)
    assert len(np.unique(_bits(ref).reshape(-1, 3), axis=0)) > 100
    _same(got, ref, f"scale 2^{exponent}")


def test_staircase_mesh(rt, O):
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    nx, ny = 96, 64
    cam = rt.staircase_camera(nx, ny)
    ks, keep = rt.make_kernel_scene(hm, mats)
    fb = rt.initRenderer(ks, cam, nx, ny, 16, keepalive=keep)
    rt.runRenderer(NS, 8, 8)
    got = np.array(fb, copy=True)
    rt.cleanupRenderer()
    ref, _ = O.render(O.mesh_scene(hm, mats), cam, O.default_options(False), nx, ny, NS, 16)
    _same(got, ref, "staircase")
