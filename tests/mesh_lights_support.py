"""Named lights for the path-traced mesh frames of tests/mesh_materials_support.py, and the CPU oracle's renders under them.  No test: a plain module,
read by tests/test_mesh_lights_api.py (CPU: each light does what it is named for, on the oracle alone) and tests/test_gpu_mesh_lights.py (GPU: every mesh
kernel against the oracle under every light).

rt_render_options.light (centre, radius) and .lightColor drive next-event estimation in every mesh kernel.  The default light of getDefaultRenderOptions -
centre (52.5, 715.7, -272.6), radius 50, colour (20, 20, 20) - lies outside the bounds of every test scene and is grey: no shadow ray can meet an occluder
BEHIND it, no channel can be told from another, cosAMax never leaves [0.998, 1).  The lights below do.

Frames: stair_exact and soup_exact of mesh_materials_support (taken from there, not copied), and stair_plain = the staircase with its own plain table
(mesh_materials_support.plain_stair_table), the scene of the LEAN instantiations.

Lights (name: purpose; centre and radius per scene kind in LIGHTS):
  inside      in the middle of the scene, small: occluders behind the light (a shadow traversal that ignored lightDist would find them)
  inside_big  the same centre, a radius that reaches the geometry: near regime (cosAMax towards 0), origins inside give cosAMax = NaN and no draws
  low         soup only: between the floor plane and the mesh bounds - the scene-bounds test of a shadow ray fails by t_max = lightDist
  sky         large and above the scene: specular paths that leave the scene see it directly (the nee = 0 branch adds atten * lightColor)
  tiny        1 - R^2 / d^2 rounds to 1: cosAMax = 1, sinA = 0, omega = 0 - shadow rays are traced and counted, the contribution is exactly 0
  huge        most origins inside the light: few shadow rays, a finite frame
  default     the light of getDefaultRenderOptions, colour included (light_of returns None)
Every light but `default` has the colour COLOUR = (30, 12, 3) unless another is asked for."""
import functools

import numpy as np

import mesh_materials_support as M

FRAMES = ("stair_exact", "soup_exact", "stair_plain")
COLOUR = (30.0, 12.0, 3.0)
GREY = (30.0, 30.0, 30.0)
BLACK = (0.0, 0.0, 0.0)
LIGHTS = {
    "soup": {"inside": ((0.0, 0.0, 0.0), 0.25), "inside_big": ((0.0, 0.0, 0.0), 1.0), "low": ((0.0, -2.8, 0.0), 0.1), "sky": ((0.0, 8.0, 0.0), 5.0),
             "tiny": ((0.5, 1.0, 0.5), 1e-5), "huge": ((0.0, 0.0, 0.0), 6.0)},
    "stair": {"inside": ((5.0, 210.0, 200.0), 16.0), "inside_big": ((5.0, 210.0, 200.0), 120.0), "sky": ((5.0, 700.0, 200.0), 250.0),
              "tiny": ((5.0, 300.0, 250.0), 0.01), "huge": ((5.0, 210.0, 200.0), 370.0)},
}
DEFAULT = "default"
DEFAULT_LIGHT = ((52.514355, 715.686951, -272.620972), 50.0, (20.0, 20.0, 20.0))      # getDefaultRenderOptions' (tests/test_mesh_lights_api.py holds it to that)


def scene_kind(frame):
    return "soup" if M.is_soup(frame) else "stair"


def names(frame):
    """The named lights of a frame (without `default`)."""
    return tuple(LIGHTS[scene_kind(frame)])


def base(frame):
    """(frame name of mesh_materials_support, table argument of its oracle_frame)."""
    return ("stair_exact", "plain") if frame == "stair_plain" else (frame, "own")


def table(rt, O, frame):
    """The material table of a frame."""
    return M.plain_stair_table(rt) if frame == "stair_plain" else M.frame(rt, O, frame)["mats"]


def light_of(frame, name, colour=None, radius=None):
    """((centre), radius, (colour)) of a named light; colour / radius replace the table's.  `default` with neither: None (the options keep every
    default); with one of them: DEFAULT_LIGHT with it replaced."""
    if name == DEFAULT:
        if colour is None and radius is None:
            return None
        centre, r = DEFAULT_LIGHT[:2]
        colour = DEFAULT_LIGHT[2] if colour is None else colour
    else:
        centre, r = LIGHTS[scene_kind(frame)][name]
    return (tuple(float(x) for x in centre), float(r if radius is None else radius), tuple(float(x) for x in (COLOUR if colour is None else colour)))


def frame_options(rt, O, frame, name, nee=1, floor=None, colour=None, radius=None):
    """The oracle's options of a frame under a named light."""
    return M.frame_options(rt, O, base(frame)[0], nee, floor, light_of(frame, name, colour, radius))


def device_options(rt, frame, name, nee=1, floor=None, colour=None, radius=None, **more):
    """The same as setRenderOptions keywords: nee, floor and - for every light but `default` - light and lightColor."""
    opts = M.device_options(base(frame)[0], nee, floor, **more)
    light = light_of(frame, name, colour, radius)
    if light is not None:
        opts["light"], opts["lightColor"] = M.light_structs(rt, light)
    return opts


def oracle_frame(rt, O, frame, name, ns, nee=1, floor=None, colour=None, radius=None):
    """(frame, counters) of the oracle under a named light, computed once and read-only (mesh_materials_support.oracle_frame's cache)."""
    b, tab = base(frame)
    return M.oracle_frame(rt, O, b, ns, nee, floor, tab, False, light_of(frame, name, colour, radius))


def init(rt, O, frame, name=DEFAULT, **opts):
    """initRenderer of the frame's scene and setRenderOptions(defaults + the named light + opts); returns the framebuffer view."""
    nee, floor = opts.pop("nee", 1), opts.pop("floor", None)
    return M.init(rt, O, base(frame)[0], table(rt, O, frame) if frame == "stair_plain" else None, **device_options(rt, frame, name, nee, floor, **opts))


def set_light(rt, frame, name, nee=1, floor=None, colour=None, radius=None, **more):
    """setRenderOptions(defaults + the named light + more) on the renderer that is up: no new init."""
    rt.setRenderOptions(rt.getDefaultRenderOptions(False), **device_options(rt, frame, name, nee, floor, colour, radius, **more))


@functools.lru_cache(maxsize=None)
def first_hits(rt, O, frame):
    """(p (n, 3), normal (n, 3)) float32: hit point and facing normal of the centre ray of every pixel that meets a triangle, from the planes of
    tests/guides_reference.py (the oracle's own functions)."""
    import guides_reference as G
    f = M.frame(rt, O, base(frame)[0])
    g = G.mesh_guides(rt, O, f["hm"], table(rt, O, frame), f["tex"], f["cam"], f["nx"], f["ny"], floor=None)
    lib, cam0 = O.load_oracle(), G._camera_without_lens(rt, f["cam"])
    sel = np.argwhere(g["prim"] >= 0)
    p = np.zeros((len(sel), 3), np.float32)
    for k, (j, i) in enumerate(sel):
        org, d = G._centre_ray(lib, rt, cam0, int(i), int(j), f["nx"], f["ny"])
        o, dn = G._f3(org), G._unit(G._f3(d))
        p[k] = [o[a] + g["depth"][j, i] * dn[a] for a in range(3)]
    n = g["normal"][sel[:, 0], sel[:, 1]].astype(np.float32)
    p.setflags(write=False)
    n.setflags(write=False)
    return p, n


def shadow_witness(rt, O, frame, name):
    """dict(generated, no_draws, free, behind) of the frame's first hits under the light (attenuation 1, a seeded stream per pixel): the shadow rays
    generate_shadow_ray makes; the hits inside the light (cosAMax = NaN, nothing drawn); of the generated rays, how many are free up to the light (no
    any-hit below lightDist) and, of those, how many have an occluder BEHIND the light (an any-hit below FLT_MAX) - the rays a shadow traversal that
    ignored lightDist would get wrong."""
    import ctypes as C
    lib = O.load_oracle()
    f = M.frame(rt, O, base(frame)[0])
    scene = O.mesh_scene(f["hm"], table(rt, O, frame), f["tex"], floor=f["floor"])
    opt = frame_options(rt, O, frame, name)
    p, n = first_hits(rt, O, frame)
    flt_max = float(np.finfo(np.float32).max)
    res = dict(generated=0, no_draws=0, free=0, behind=0)
    tri, hu, hv = C.c_uint32(0), C.c_float(0), C.c_float(0)
    for k in range(len(p)):
        ok, sdir, _, dist, _, draws, _ = O.generate_shadow_ray(opt, p[k], (1.0, 1.0, 1.0), n[k], lib.orc_pixel_seed(k))
        if not ok:
            res["no_draws"] += draws == 0
            continue
        res["generated"] += 1
        near = lib.orc_hit_bvh(C.byref(scene), O.f3(p[k]), O.f3(sdir), opt.t_min, float(dist), 1, C.byref(tri), C.byref(hu), C.byref(hv), None)
        if near < float(dist):
            continue
        res["free"] += 1
        far = lib.orc_hit_bvh(C.byref(scene), O.f3(p[k]), O.f3(sdir), opt.t_min, flt_max, 1, C.byref(tri), C.byref(hu), C.byref(hv), None)
        res["behind"] += bool(far < flt_max)
    return res


# ---- generateShadowRay by itself: the regimes the frames above put a light into, and the edges beside them --------------------------------------------

REGIME_CASES = 1000
ODD_COLOURS = ((30.0, 12.0, 3.0), (0.0, 5.0, 0.0), (-1.0, 2.0, 3.0), (1e30, 1.0, 1e-40))       # (the last one: a huge channel beside a subnormal one)


def _unit_rows(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def shadow_regimes():
    """Tabulated inputs of generateShadowRay, one light and one colour per regime: a tuple of dict(name, centre, radius, colour, org, att, nrm, seeds,
    expect) with org / att / nrm (REGIME_CASES, 3) float32 and seeds (REGIME_CASES,) uint32, all read-only.  expect: outcome -> the least number of cases
    that must have it ("generated", "nan" = cosAMax is NaN and nothing is drawn, "rejected" = dotl <= 0 after two draws); tests/test_oracle_vs_ref.py holds
    the oracle to these counts on the CPU.  A third of the normals face the light, the others are random.
      near      |org - c| / R in (1, 2]: cosAMax from 0 to 0.87
      near_one  R = 1e-3 at a distance of 0.5 .. 2: cosAMax within 32 ulp below 1
      small     R = 1e-4 at a distance of 0.7 .. 2: R^2 / d^2 < 2^-25, so 1 - R^2 / d^2 rounds to 1: cosAMax = 1, sinA = 0, omega = 0
      zero      R = 0: the same by an exact 0
      surface   the origin's distance from c is the next float above R (even cases) or below R (odd cases), up to the rounding of the three coordinates
      centre    org = c: the direction is 0 / 0; R = 0 in the odd cases (0 / 0 inside cosAMax too)
      switch    the direction to the light has |sw.x| within 0.01 -+ 0.005: both sides of the switch of the tangent frame's helper axis
      colour_k  ordinary distances (3 .. 10 R) under ODD_COLOURS[k]"""
    rng = np.random.default_rng(4242)
    n = REGIME_CASES
    f = np.float32
    out = []

    def add(name, centre, radius, colour, org, expect, face_all=False):
        centre = np.asarray(centre, np.float64)
        org = np.asarray(org, f)
        nrm = _unit_rows(rng.normal(size=(n, 3)))
        with np.errstate(all="ignore"):
            to_l = _unit_rows(centre - org.astype(np.float64))
        facing = np.isfinite(to_l).all(axis=1) & ((np.arange(n) % 3 == 0) | face_all)
        nrm[facing] = to_l[facing]
        d = dict(name=name, centre=tuple(float(x) for x in centre), radius=float(radius), colour=tuple(colour), org=org,
                 att=rng.uniform(0, 1, (n, 3)).astype(f), nrm=nrm.astype(f), seeds=(rng.integers(1, 2 ** 32, n, dtype=np.uint64) | 1).astype(np.uint32),
                 expect=dict(expect))
        for k in ("org", "att", "nrm", "seeds"):
            d[k].setflags(write=False)
        out.append(d)

    dirs = lambda: _unit_rows(rng.normal(size=(n, 3)))
    c, r = np.array((3.0, -2.0, 5.0)), 2.0
    add("near", c, r, COLOUR, c + dirs() * (r * (2.0 - rng.uniform(0, 1, (n, 1)))), dict(generated=100, rejected=100))
    c = np.array((0.5, 1.0, 0.5))
    add("near_one", c, 1e-3, COLOUR, c + dirs() * rng.uniform(0.5, 2.0, (n, 1)), dict(generated=100, rejected=100))
    add("small", c, 1e-4, COLOUR, c + dirs() * rng.uniform(0.7, 2.0, (n, 1)), dict(generated=100, rejected=100))
    add("zero", c, 0.0, COLOUR, c + dirs() * rng.uniform(0.5, 2.0, (n, 1)), dict(generated=100, rejected=100))
    c, r = np.array((5.0, 210.0, 200.0)), 16.0
    dist = np.where(np.arange(n) % 2 == 0, np.nextafter(f(r), f(np.inf)), np.nextafter(f(r), f(0))).astype(np.float64)
    add("surface", c, r, COLOUR, c + dirs() * dist[:, None], dict(generated=100, nan=100), face_all=True)
    add("centre", c, r, COLOUR, np.tile(c, (n, 1)), dict(nan=n))
    out[-1]["radius_odd"] = 0.0
    sx = rng.uniform(0.005, 0.015, n) * rng.choice([-1.0, 1.0], n)
    rest = _unit_rows(rng.normal(size=(n, 2))) * np.sqrt(1.0 - sx * sx)[:, None]
    sw = np.stack([sx, rest[:, 0], rest[:, 1]], axis=1)
    add("switch", c, r, COLOUR, c - sw * rng.uniform(40.0, 400.0, (n, 1)), dict(generated=100, rejected=100))
    c, r = np.array((0.0, 8.0, 0.0)), 1.5
    for k, colour in enumerate(ODD_COLOURS):
        add(f"colour_{k}", c, r, colour, c + dirs() * rng.uniform(3 * r, 10 * r, (n, 1)), dict(generated=100, rejected=100))
    return tuple(out)


def regime_lights(rt, reg):
    """[(rows, rt.sphere, rt.vec3)] of a regime: the light and colour of each group of cases (one group, or - `centre` - the even and the odd cases)."""
    rows = np.arange(REGIME_CASES)
    groups = [(rows, reg["radius"])] if "radius_odd" not in reg else [(rows[0::2], reg["radius"]), (rows[1::2], reg["radius_odd"])]
    return [(sel,) + M.light_structs(rt, (reg["centre"], radius, reg["colour"])) for sel, radius in groups]


def regime_oracle(rt, O, reg, which="orc"):
    """The outputs of O.generate_shadow_ray (which: "orc", or "ref" for the reference-header twin) on a regime's cases, as a dict of arrays."""
    n = REGIME_CASES
    r = {"generated": np.zeros(n, np.int32), "draws": np.zeros(n, np.int32), "rng_after": np.zeros(n, np.uint32), "dir": np.zeros((n, 3), np.float32),
         "contribution": np.zeros((n, 3), np.float32), "dist": np.zeros(n, np.float32), "cos_a_max": np.zeros(n, np.float32)}
    opt = O.default_options(False)
    for sel, light, colour in regime_lights(rt, reg):
        opt.light, opt.lightColor = light, colour
        for k in sel:
            g = O.generate_shadow_ray(opt, reg["org"][k], reg["att"][k], reg["nrm"][k], int(reg["seeds"][k]), which)
            r["generated"][k], r["dir"][k], r["contribution"][k], r["dist"][k], r["cos_a_max"][k], r["draws"][k], r["rng_after"][k] = g
    return r


def regime_outcomes(res):
    """dict(generated, nan, rejected) counts of regime_oracle's result; every case has exactly one of the three."""
    gen = res["generated"] != 0
    nan = ~gen & (res["draws"] == 0)
    rej = ~gen & (res["draws"] == 2)
    assert (gen | nan | rej).all() and np.isnan(res["cos_a_max"][nan]).all() and (res["draws"][gen] == 2).all()
    return dict(generated=int(gen.sum()), nan=int(nan.sum()), rejected=int(rej.sum()))
