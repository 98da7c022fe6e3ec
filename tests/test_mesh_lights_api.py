"""CPU only: the lights of tests/mesh_lights_support.py do what they are named for.  Everything here is the CPU oracle's own output - nothing of the code
under test runs - at the 4 samples per pixel the GPU tests use.  These are conditions on the fixtures, each with the figure it had when the table was
fixed (frames in the order stair_exact, soup_exact, stair_plain); every figure is printed.

Why the file exists: under the default light of getDefaultRenderOptions three kinds of kernel error cannot be seen.
  1. Of the shadow rays from the first hits that are free up to the light, NONE has an occluder behind the light (0 of 187, 0 of 381, 0 of 187): a
     shadow traversal that ran to FLT_MAX instead of lightDist renders the same frame.  Under `inside` 1357 of the 1808 generated rays are such rays on
     the staircase and 101 of 802 on the soup; under `inside_big` 1152 of 1568 and 275 of 837.
  2. The default colour (20, 20, 20) has three equal channels: a kernel that used lightColor.x for every channel renders the same frame (0 pixels).
     Under (30, 12, 3) against (30, 30, 30), of 2000 / 4032 / 2000 pixels: inside 1858 / 1330 / 1987, inside_big 1824 / 2613 / 1986, low 3125,
     sky 1908 / 3346 / 1987, huge 359 / 2179 / 785.
  3. With nee = 0 a specular path that leaves the scene and meets the light sphere adds atten * lightColor.  The default light decides 1 / 18 / 0 pixels
     that way; `sky` decides 248 / 271 / 59.
The other lights: `low` fails the scene-bounds test of 11222 of its 16420 shadow rays, and of the shadow rays from a grid of 400 floor points 187 miss
the bounds by t_max = lightDist alone (the light lies between the bounds and the floor); `tiny` traces 9662 / 17172 / 23658 shadow rays (9075 / 775 /
22629 of them free) whose contribution is exactly 0; `inside_big` has 317 / 34 / 317 first hits inside the light, and `inside_big` and `huge` have fewer
shadow rays than `inside` (staircase 8183 and 995 against 9165, soup 16199 and 5005 against 16312, plain staircase 22464 and 1757 against 23219), with
values up to 32.6 and no NaN.

Three values moved from the first proposal because a condition failed with them: the soup's `tiny` radius 1e-3 -> 1e-5 (cosAMax is exactly 1 only
where R^2 / d^2 < 2^-25, d > 5.8 at 1e-3: 304 pixels differed from the black light's frame), the staircase's `inside_big` radius 66 -> 120 (at 66 only
9 first hits lie inside and the frame has MORE shadow rays than `inside`, 9315 against 9165) and the staircase's `huge` radius 400 -> 370 (at 400 the
49 / 79 shadow rays that are left change 24 / 56 pixels with the colour, below 5 %; at 370, 1772 of the 2000 first hits are still inside)."""
import numpy as np
import pytest

import mesh_lights_support as L
from mesh_materials_support import bits

SPP = 4
FRAME_LIGHTS = [(f, n) for f in L.FRAMES for n in L.names(f)]


def _differ(a, b):
    return int((bits(a) != bits(b)).any(axis=2).sum())


def test_the_default_light_is_the_renderers(rt, O):
    """DEFAULT_LIGHT is the light of the default options, float for float, and grey."""
    o = O.default_options(False)
    centre, radius, colour = L.DEFAULT_LIGHT
    f = np.float32
    assert [f(x) for x in centre] == [f(x) for x in o.light.center.e[:]] and f(radius) == f(o.light.radius)
    assert [f(x) for x in colour] == [f(x) for x in o.lightColor.e[:]] and len(set(colour)) == 1
    assert L.light_of("stair_exact", L.DEFAULT) is None
    for frame in L.FRAMES:
        a = L.oracle_frame(rt, O, frame, L.DEFAULT, SPP)[0]
        b = L.oracle_frame(rt, O, frame, L.DEFAULT, SPP, colour=colour)[0]               # the same light, spelled out
        assert np.array_equal(bits(a), bits(b))


def test_the_table(rt, O):
    """Every staircase light lies inside the mesh bounds or is `sky`; the soup's `low` lies between the floor plane and the bounds."""
    import mesh_materials_support as M
    assert set(L.names("soup_exact")) == {"inside", "inside_big", "low", "sky", "tiny", "huge"}
    assert set(L.names("stair_exact")) == set(L.names("stair_plain")) == {"inside", "inside_big", "sky", "tiny", "huge"}
    for frame in ("stair_exact", "soup_exact"):
        b = M.frame(rt, O, frame)["hm"].view.bounds
        lo, hi = np.array(b.min.e[:]), np.array(b.max.e[:])
        for name in L.names(frame):
            c = np.array(L.light_of(frame, name)[0])
            inside = bool(((c > lo) & (c < hi)).all())
            print(f"{frame} {name}: centre {c.tolist()} inside the bounds {inside}")
            assert inside == (name not in ("sky", "low")), (frame, name)
        d = np.array(L.DEFAULT_LIGHT[0])
        assert not ((d > lo) & (d < hi)).all()
    lo_y = M.frame(rt, O, "soup_exact")["hm"].view.bounds.min.e[1]
    c, r = L.LIGHTS["soup"]["low"]
    assert M.SOUP_FLOOR[4] < c[1] - r and c[1] + r < lo_y


@pytest.mark.parametrize("frame", L.FRAMES)
def test_occluders_behind_the_light(rt, O, frame):
    """inside, inside_big: at least 5 % of the shadow rays generated from the first hits are free up to the light and blocked beyond it; the default
    light has fewer such rays than either (none)."""
    res = {name: L.shadow_witness(rt, O, frame, name) for name in ("inside", "inside_big", L.DEFAULT)}
    for name, w in res.items():
        print(f"{frame} {name}: {w}")
    for name in ("inside", "inside_big"):
        w = res[name]
        assert w["generated"] >= 500 and w["behind"] >= 0.05 * w["generated"], (frame, name, w)
        assert res[L.DEFAULT]["behind"] < w["behind"]
    assert res[L.DEFAULT]["generated"] >= 100 and res[L.DEFAULT]["free"] >= 100
    assert res["inside"]["no_draws"] == 0 and res["inside_big"]["no_draws"] >= 20      # first hits inside the light: 317, 34, 317


@pytest.mark.parametrize("frame,name", [(f, n) for f, n in FRAME_LIGHTS if n != "tiny"])
def test_colour_matters(rt, O, frame, name):
    """(30, 12, 3) against (30, 30, 30) - what a kernel that read lightColor.x for every channel would render: at least 5 % of the pixels differ.  Under
    the default light that kernel renders the default frame: its colour has three equal channels (test_the_default_light_is_the_renderers)."""
    a = L.oracle_frame(rt, O, frame, name, SPP)[0]
    g = L.oracle_frame(rt, O, frame, name, SPP, colour=L.GREY)[0]
    n = _differ(a, g)
    print(f"{frame} {name}: {n} of {a.shape[0] * a.shape[1]} pixels differ between {L.COLOUR} and {L.GREY}")
    assert n >= 0.05 * a.shape[0] * a.shape[1]
    x_only = (L.DEFAULT_LIGHT[2][0],) * 3
    assert _differ(L.oracle_frame(rt, O, frame, L.DEFAULT, SPP)[0], L.oracle_frame(rt, O, frame, L.DEFAULT, SPP, colour=x_only)[0]) == 0 < n


@pytest.mark.parametrize("frame", L.FRAMES)
def test_the_light_seen_directly(rt, O, frame):
    """sky, nee = 0: the frame under (30, 12, 3) differs from the frame under a black light in at least 40 pixels; the default light in fewer."""
    n = _differ(L.oracle_frame(rt, O, frame, "sky", SPP, nee=0)[0], L.oracle_frame(rt, O, frame, "sky", SPP, nee=0, colour=L.BLACK)[0])
    d = _differ(L.oracle_frame(rt, O, frame, L.DEFAULT, SPP, nee=0)[0], L.oracle_frame(rt, O, frame, L.DEFAULT, SPP, nee=0, colour=L.BLACK)[0])
    print(f"{frame}: pixels a directly seen light decides, sky {n}, default light {d}")
    assert n >= 40 and d < n


def test_low_fails_the_bounds_test_by_the_light_distance(rt, O):
    """soup_exact under `low`: some shadow rays, not all, miss the scene bounds.  From a grid of floor points, at least 5 % of the generated shadow rays
    miss the bounds with t_max = lightDist and meet them with FLT_MAX: the distance is what rejects them."""
    import mesh_materials_support as M
    cnt =L.oracle_frame(rt, O, "soup_exact", "low", SPP)[1]
    nohits, shadows = int(cnt.ref_stats[rt.RT_STAT_SHADOWS_BBOX_NOHITS]), int(cnt.ref_stats[rt.RT_STAT_SHADOWS])
    print(f"soup_exact low: {nohits} of {shadows} shadow rays miss the bounds")
    assert 0 < nohits < shadows == cnt.shadow_rays
    lib, opt = O.load_oracle(), L.frame_options(rt, O, "soup_exact", "low")
    b = M.frame(rt, O, "soup_exact")["hm"].view.bounds
    lo, hi = O.f3(b.min.e[:]), O.f3(b.max.e[:])
    generated = by_distance = 0
    for k, (x, z) in enumerate((x, z) for x in np.linspace(-4, 4, 20) for z in np.linspace(-4, 4, 20)):
        p = (x, M.SOUP_FLOOR[4], z)
        ok, sdir, _, dist, _, _, _ = O.generate_shadow_ray(opt, p, (1.0, 1.0, 1.0), M.SOUP_FLOOR[:3], lib.orc_pixel_seed(k))
        if ok:
            generated += 1
            by_distance += bool(not lib.orc_hit_bbox(lo, hi, O.f3(p), O.f3(sdir), float(dist)) and lib.orc_hit_bbox(lo, hi, O.f3(p), O.f3(sdir), 3.0e38))
    print(f"soup_exact low: {by_distance} of {generated} shadow rays from 400 floor points miss the bounds by their distance alone")
    assert generated >= 100 and by_distance >= 0.05 * generated
    for frame in ("stair_exact", "stair_plain"):
        assert L.oracle_frame(rt, O, frame, L.DEFAULT, SPP)[1].ref_stats[rt.RT_STAT_SHADOWS_BBOX_NOHITS] == 0


@pytest.mark.parametrize("frame", L.FRAMES)
def test_tiny_contributes_exactly_nothing(rt, O, frame):
    """Shadow rays are traced and counted - some free, some blocked - and the frame is bit-equal to the black light's."""
    a, ca = L.oracle_frame(rt, O, frame, "tiny", SPP)
    k, ck = L.oracle_frame(rt, O, frame, "tiny", SPP, colour=L.BLACK)
    free = int(ca.ref_stats[rt.RT_STAT_SHADOWS_NOHITS])
    print(f"{frame} tiny: {ca.shadow_rays} shadow rays, {free} of them free")
    assert ca.shadow_rays > 0 and 0 < free < ca.shadow_rays
    assert np.array_equal(bits(a), bits(k)) and ca.shadow_rays == ck.shadow_rays


@pytest.mark.parametrize("frame", L.FRAMES)
def test_big_lights_swallow_origins(rt, O, frame):
    """huge, inside_big: fewer shadow rays than `inside` (origins inside the light draw nothing), and no NaN reaches the frame."""
    base = L.oracle_frame(rt, O, frame, "inside", SPP)[1].shadow_rays
    for name in ("inside_big", "huge"):
        a, cnt = L.oracle_frame(rt, O, frame, name, SPP)
        print(f"{frame} {name}: {cnt.shadow_rays} shadow rays against {base} under inside, largest value {float(a.max()):.3g}")
        assert 0 < cnt.shadow_rays < base
        assert not np.isnan(a).any() and cnt.ref_stats[rt.RT_STAT_NAN] == 0 and np.isfinite(a).all()


@pytest.mark.parametrize("frame,name", FRAME_LIGHTS)
def test_no_nan_and_a_different_frame(rt, O, frame, name):
    """Every light renders a finite frame that differs from the default light's (tiny: its light adds nothing, the default's does)."""
    for nee in (1, 0):
        a = L.oracle_frame(rt, O, frame, name, SPP, nee=nee)[0]
        assert np.isfinite(a).all()
    assert _differ(L.oracle_frame(rt, O, frame, name, SPP)[0], L.oracle_frame(rt, O, frame, L.DEFAULT, SPP)[0]) > 100
