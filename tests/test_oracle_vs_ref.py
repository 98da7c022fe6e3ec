"""CPU: our restatement (oracle/liboracle.so) against the reference's own header-only code, function by function and on whole
frames.  The reference side comes from the reference compiled where its sources exist (oracle/_ref/libref.so, libref_main.so);
elsewhere from tests/golden/vs_ref.npz: the same reference calls on the same seeded inputs, frozen.  Where the shims exist the live
outputs must also equal the frozen ones, so the file cannot go stale.  To re-mint it where the shims exist:
RT_MINT_VS_REF=tests/golden/vs_ref.npz python -m pytest tests/test_oracle_vs_ref.py
The keys of the lights of tests/mesh_lights_support.py live in a second file, tests/golden/vs_ref_lights.npz (one file would pass the size limit of a
committed file); the same command writes it beside the first, as <the given name>_lights.npz."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import mesh_lights_support as L
import mesh_materials_support as M
from oracle import oracle as O

FLT_MAX = float(np.finfo(np.float32).max)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vs_ref.npz")
GOLDEN_LIGHTS = GOLDEN[:-len(".npz")] + "_lights.npz"
MINT = os.environ.get("RT_MINT_VS_REF")
_minted = {}
_golden = {}


def _reference(key, live, have=O.have_ref, golden=GOLDEN):
    """The reference's outputs for `key` as a dict of arrays: live() where the shim was built (checked against the frozen copy in `golden`,
    or recorded into RT_MINT_VS_REF), else the frozen copy."""
    if golden not in _golden:
        _golden[golden] = {}
        if os.path.exists(golden):
            with np.load(golden) as z:
                _golden[golden] = {k: z[k] for k in z.files}
    frozen = {k[len(key) + 1:]: v for k, v in _golden[golden].items() if k.startswith(key + "/")}
    if not have():
        assert frozen, f"{key}: no reference shim and no frozen outputs in {golden}"
        return frozen
    out = {k: np.asarray(v) for k, v in live().items()}
    if MINT:
        minted = _minted.setdefault(golden, {})
        minted.update({f"{key}/{k}": v for k, v in out.items()})
        np.savez_compressed(MINT if golden == GOLDEN else MINT[:-len(".npz")] + "_lights.npz", **minted)
    else:
        assert set(out) == set(frozen) and all(out[k].tobytes() == frozen[k].tobytes() for k in out), f"{key}: {golden} is stale"
    return out


def _sha(b):
    return np.frombuffer(hashlib.sha256(bytes(b)).digest(), np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def test_struct_layouts_match_reference(rt):
    def live():
        sizes = (C.c_int * 32)()
        n = O.load_ref().ref_struct_sizes(sizes, 32)
        return {"sizes": np.array(sizes[:n], np.int32)}
    sizes = _reference("struct_sizes", live)["sizes"]
    names = ["vec3", "ray", "camera", "sphere", "plane", "bbox", "triangle", "bvh_node", "material", "stexture", "mesh", "scene",
             "kernel_scene", "intersection", "scatter_info", "path", "tri_hit"]
    got = dict(zip(names, sizes.tolist()))
    # SURVEY.md §8b table
    assert got == {"vec3": 12, "ray": 24, "camera": 88, "sphere": 16, "plane": 24, "bbox": 24, "triangle": 64, "bvh_node": 24,
                   "material": 24, "stexture": 16, "mesh": 56, "scene": 96, "kernel_scene": 64, "intersection": 56,
                   "scatter_info": 36, "path": 88, "tri_hit": 12}
    for nm in ("vec3", "camera", "sphere", "plane", "bbox", "triangle", "bvh_node", "material", "stexture", "mesh", "kernel_scene"):
        assert C.sizeof(getattr(rt, nm)) == got[nm], nm


def _function_cases(rt):
    """The seeded inputs of test_functions_random: rng seed, a ray, a sphere, a box (some ray directions with a zero
    component), a triangle with a ray towards a point inside it, a floor plane."""
    rng = np.random.default_rng(99)
    cases = []
    for k in range(1500):
        c = {"seed": int(rng.integers(1, 2 ** 32)) | 1}
        c["org"] = rng.uniform(-3, 3, 3); c["d"] = rng.normal(size=3)
        sp = rt.sphere(); sp.center.e[:] = rng.uniform(-2, 2, 3); sp.radius = rng.uniform(0.1, 2.5)
        c["sphere"] = sp
        c["lo"] = rng.uniform(-2, 1, 3); c["hi"] = c["lo"] + rng.uniform(0, 2, 3)
        c["d_box"] = c["d"].copy()
        if k % 7 == 0:
            c["d_box"][k % 3] = 0.0
        tri = rt.triangle()
        for q in range(3):
            tri.v[q].e[:] = rng.uniform(-2, 2, 3)
        target = sum(np.array(tri.v[q].e[:]) * w for q, w in enumerate(rng.dirichlet([1, 1, 1])))
        c["tri"], c["dd"] = tri, target - c["org"]
        pl = rt.plane(); pl.norm.e[:] = (0.0, 1.0, 0.0); pl.point.e[:] = (0.0, float(rng.uniform(-1, 1)), 0.0)
        c["plane"] = pl
        cases.append(c)
    return cases + _edge_cases(rt, rng)


def _edge_cases(rt, rng):
    """480 more cases at the edges the ray queries reach (tests/rays_reference.py: mesh_axis, the _inf sets), drawn after the random ones so that those keep
    their inputs.  Every coordinate is rounded to float32 first, so that "on the plane" survives the conversion.  Kind k % 6:
    0: a box flat on one axis, the origin in its plane, that direction component zero (both slab products of the axis are 0 * inf);
    1: the same flat box with the origin off the plane (the axis alone rejects the ray: -inf, -inf or +inf, +inf);
    2: an ordinary box, the origin exactly on its lo or hi plane of an axis whose direction component is zero (one product is NaN, the other +-inf);
    3: as 2 with two zero components and the origin on a plane of each of the two axes;
    4: as 2 but a non-zero component on the plane's axis (t0 or t1 is exactly 0, below the test's t_min of 0.001);
    5: an ordinary box, no zero component, the origin inside it.
    Zeros are +0.0 in the first half of the cases and -0.0 in the second (1 / -0 = -inf takes the swap branch).  Every other case takes FLT_MAX as the box's
    and the triangle's t_max.  Triangles: the ray lies in the triangle's plane - from a point of the plane towards another one - in the kinds 0 to 2 (the
    determinant is 0 up to rounding: either side of the EPS test), starts on a vertex or an edge in the kinds 3 and 4, and is an ordinary hit in kind 5."""
    f = np.float32
    cases = []
    n = 480
    for k in range(n):
        kind = k % 6
        zero = f(0.0) if k < n // 2 else f(-0.0)
        c = {"seed": int(rng.integers(1, 2 ** 32)) | 1}
        lo = rng.uniform(-2, 1, 3).astype(f)
        hi = (lo + rng.uniform(0.1, 2, 3).astype(f)).astype(f)
        a, b = (int(x) for x in rng.permutation(3)[:2])
        d = rng.normal(size=3).astype(f)
        org = rng.uniform(lo, hi).astype(f)
        if kind in (0, 1):
            hi[a] = lo[a]
            org = (rng.uniform(lo, hi) + rng.normal(size=3) * (0 if k % 4 < 2 else 1.5)).astype(f)       # inside the flat box's rectangle, or around it
            org[a] = lo[a] if kind == 0 else lo[a] + f(rng.choice([-0.5, 0.5]))
            d[a] = zero
        elif kind in (2, 3, 4):
            org[a] = (lo if rng.integers(0, 2) else hi)[a]
            if kind != 4:
                d[a] = zero
            if kind == 3:
                org[b] = (lo if rng.integers(0, 2) else hi)[b]
                d[b] = zero
        c["lo"], c["hi"], c["org"], c["d"], c["d_box"] = lo, hi, org, d, d
        sp = rt.sphere(); sp.center.e[:] = rng.uniform(-2, 2, 3); sp.radius = rng.uniform(0.1, 2.5)
        c["sphere"] = sp
        tri = rt.triangle()
        v = rng.uniform(-2, 2, (3, 3)).astype(f)
        for q in range(3):
            tri.v[q].e[:] = v[q]
        inside = (v * rng.dirichlet([1, 1, 1])[:, None]).sum(axis=0)
        if kind in (0, 1, 2):                                       # in the plane: from one affine combination of the vertices towards another
            w = rng.normal(size=3); w += (1 - w.sum()) / 3
            start = (v * w[:, None]).sum(axis=0)
            c["tri_org"], c["dd"] = start.astype(f), ((inside - start) * 10.0 ** rng.uniform(-1, 1)).astype(f)
        elif kind == 3:                                             # from a vertex
            c["tri_org"], c["dd"] = v[k % 3].copy(), rng.normal(size=3).astype(f)
        elif kind == 4:                                             # from a point of an edge, to the rounding of the midpoint
            c["tri_org"], c["dd"] = ((v[0] + v[1]) * f(0.5)).astype(f), rng.normal(size=3).astype(f)
        else:
            c["tri_org"] = org
            c["dd"] = (inside - org).astype(f)
        c["tri"] = tri
        pl = rt.plane(); pl.norm.e[:] = (0.0, 1.0, 0.0); pl.point.e[:] = (0.0, float(rng.uniform(-1, 1)), 0.0)
        c["plane"] = pl
        if k % 2:
            c["box_tmax"] = c["tri_tmax"] = FLT_MAX
        cases.append(c)
    return cases


def _functions(lib, p, cases):
    """Every function of test_functions_random on every case through `lib` (prefix `p`: "orc_" or "ref_")."""
    n = len(cases)
    r = {k: np.zeros(n, np.float32) for k in ("sphere_t", "box_dist", "tri_t", "tri_u", "tri_v", "plane_t")}
    r["unit_sphere"] = np.zeros((n, 3), np.float32); r["rng_after"] = np.zeros(n, np.uint32); r["box_hit"] = np.zeros(n, np.int32)
    o = (C.c_float * 3)()
    for k, c in enumerate(cases):
        s = C.c_uint32(c["seed"])
        getattr(lib, p + "random_in_unit_sphere")(C.byref(s), o)
        r["unit_sphere"][k], r["rng_after"][k] = o[:], s.value
        org, d, db = f3(c["org"]), f3(c["d"]), f3(c["d_box"])
        r["sphere_t"][k] = getattr(lib, p + "sphere_hit")(C.byref(c["sphere"]), org, d, 0.001, 3.0e38)
        box_tmax, tri_tmax = c.get("box_tmax", 10.0), c.get("tri_tmax", 3.0e38)                # (the edge cases: FLT_MAX for every other one)
        r["box_dist"][k] = getattr(lib, p + "hit_bbox_dist")(f3(c["lo"]), f3(c["hi"]), org, db, box_tmax)
        r["box_hit"][k] = getattr(lib, p + "hit_bbox")(f3(c["lo"]), f3(c["hi"]), org, db, box_tmax)
        u = C.c_float(); v = C.c_float()
        tri_org = f3(c["tri_org"]) if "tri_org" in c else org
        r["tri_t"][k] = getattr(lib, p + "triangle_hit")(C.byref(c["tri"]), tri_org, f3(c["dd"]), 0.01, tri_tmax, C.byref(u), C.byref(v))
        r["tri_u"][k], r["tri_v"][k] = u.value, v.value
        r["plane_t"][k] = getattr(lib, p + "plane_hit")(C.byref(c["plane"]), org, db, 0.01, 3.0e38)
    return r


def test_functions_random(rt):
    cases = _function_cases(rt)
    ref = _reference("functions", lambda: _functions(O.load_ref(), "ref_", cases))
    orc = _functions(O.load_oracle(), "orc_", cases)
    assert np.array_equal(orc["unit_sphere"], ref["unit_sphere"]) and np.array_equal(orc["rng_after"], ref["rng_after"])
    for k in ("sphere_t", "box_dist", "tri_t", "plane_t"):
        assert np.array_equal(_bits(orc[k]), _bits(ref[k])), k
    assert np.array_equal(orc["box_hit"], ref["box_hit"])
    hit = orc["tri_t"] < 1e30
    assert np.array_equal(orc["tri_u"][hit], ref["tri_u"][hit]) and np.array_equal(orc["tri_v"][hit], ref["tri_v"][hit])
    # the edge cases are what they claim: NaN slab products that leave a hit standing, boxes rejected and accepted under FLT_MAX, in-plane rays on both
    # sides of the determinant test
    edge = np.arange(1500, len(cases))
    assert len(edge) == 480
    kind = (edge - 1500) % 6
    with np.errstate(all="ignore"):
        nan_slab = np.array([np.isnan(np.stack([c["lo"] - c["org"], c["hi"] - c["org"]]) * (np.float32(1) / c["d_box"])).any() for c in cases[1500:]])
    neg_zero = np.array([(np.float32(c["d_box"]).view(np.uint32) == 0x80000000).any() for c in cases[1500:]])
    print("edge cases: NaN slab products", int(nan_slab.sum()), "of them box hits", int(orc["box_hit"][edge][nan_slab].sum()), "-0.0 directions", int(neg_zero.sum()),
          "box hits per kind", [int(orc["box_hit"][edge][kind == q].sum()) for q in range(6)], "triangle hits per kind", [int(hit[edge][kind == q].sum()) for q in range(6)])
    assert np.all(nan_slab == ((kind == 0) | (kind == 2) | (kind == 3)))
    assert orc["box_hit"][edge][nan_slab].sum() >= 40 and (orc["box_hit"][edge][nan_slab] == 0).sum() >= 30
    assert neg_zero.sum() >= 150 and orc["box_hit"][edge][neg_zero].sum() >= 20
    assert orc["box_hit"][edge][kind == 1].sum() == 0 and orc["box_hit"][edge][kind == 5].all()
    assert hit[edge][kind == 5].all() and 0 < hit[edge][kind <= 2].sum() < (kind <= 2).sum()


def test_light_sampling_expressions(rt):
    """kernels.cu:378-387: the two vec3 expressions of generateShadowRay, restated in rt_oracle.c, against the
    same expressions evaluated with the reference's own vec3 operators (tests/golden/light.npz)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "light.npz"))
    f = np.float32
    for k in range(len(g["eps2"])):
        phi = f(2 * np.pi * np.float64(g["eps2"][k]))
        assert phi == g["phi"][k]
        su, sv, sw = g["su"][k], g["sv"][k], g["sw"][k]
        c, s = f(np.cos(phi, dtype=f)), f(np.sin(phi, dtype=f))
        # numpy's float32 cos/sin may differ from glibc's cosf/sinf in the last ulp; compare loosely here —
        # the oracle itself calls cosf/sinf like the reference and is frame-checked in test_oracle_golden
        l = g["sinA"][k] * (c * su) + g["sinA"][k] * (s * sv) + g["cosA"][k] * sw
        assert np.allclose(l, g["ldir"][k], rtol=1e-5, atol=1e-6)
        omega = f(2 * np.pi * np.float64(f(1.0) - g["cosAMax"][k]))
        con = (omega * (g["dotl"][k] * (g["att"][k] * f(20.0)))) / f(np.pi)
        assert np.array_equal(_bits(con.astype(f)), _bits(g["lcon"][k]))


@pytest.mark.parametrize("scene,nx,ny,ns,kw", [("c1", 160, 80, 3, {}), ("rs", 120, 80, 3, {}), ("rs", 64, 48, 4, {"rr": 1, "sky": 0}),
                                               ("rs", 64, 48, 4, {"rng": 1}), ("c1", 97, 33, 2, {"t_min": 0.01})])
def test_frames_random_configs(rt, scene, nx, ny, ns, kw):
    sp, mt, cam = rt.scene_three_spheres(nx, ny) if scene == "c1" else rt.scene_random_spheres(nx, ny)
    opt = O.default_options(True)
    for k, v in kw.items():
        setattr(opt, k, v)
    a, ca = O.render(O.sphere_scene(sp, mt), cam, opt, nx, ny, ns, 50, counters=True)

    def live():
        b, cb = O.ref_render_spheres(sp, mt, cam, opt, nx, ny, ns, 50, counters=True)
        return {"frame": b, "counters": np.array([cb.rays, cb.prim_tests, cb.hits], np.int64)}
    ref = _reference(f"frames_{scene}_{nx}x{ny}x{ns}_" + "_".join(f"{k}{v}" for k, v in kw.items()), live)
    assert np.array_equal(_bits(a), _bits(ref["frame"]))
    assert [ca.rays, ca.prim_tests, ca.hits] == ref["counters"].tolist()


# ---- the MESH path: oracle restatement vs the reference-arithmetic twin (oracle/ref_driver.cpp ref_render_mesh) ------------

def _triangle_soup(rt, rng, n, n_mats=6):
    tris = np.zeros(n, rt.triangle_dtype)
    c = rng.uniform(-2, 2, (n, 1, 3)).astype(np.float32)
    tris["v"] = c + rng.uniform(-0.7, 0.7, (n, 3, 3)).astype(np.float32)
    tris["texCoords"] = rng.uniform(-1, 2, (n, 6))
    tris["meshID"] = rng.integers(0, n_mats, n)
    mats = np.zeros(n_mats, rt.material_dtype)
    mats["type"] = [rt.RT_DIFFUSE, rt.RT_METAL, rt.RT_GLASS, rt.RT_DIFFUSE, rt.RT_METAL, rt.RT_MODEL_COAT][:n_mats]
    mats["color"] = rng.uniform(0.2, 1, (n_mats, 3))
    mats["param"] = [0.0, 0.1, 1.5, 0.0, 0.0, 0.0][:n_mats]
    mats["texId"] = -1
    return tris, mats


def _counters(c):
    return np.array([c.samples, c.rays, c.shadow_rays, c.prim_tests, c.node_visits, c.hits] + list(c.ref_stats), np.int64)


def _mesh_frame_and_counters(sc, cam, opt, nx, ny, ns, depth):
    b, cb = O.ref_render_mesh(sc, cam, opt, nx, ny, ns, depth, counters=True)
    return {"frame": b, "counters": _counters(cb)}


@pytest.mark.parametrize("kw", [{}, {"nee": 0}, {"nee": 0, "rr": 0}, {"sky": 1}, {"floor": 1}, {"floor": 1, "nee": 0}, {"rng": 1},
                                {"light_radius": 900.0}, {"light": "inside"}])
def test_mesh_frames_oracle_equals_reference_twin_staircase(rt, kw):
    """Frames + every counter, NEE on and off, RR on and off, gradient sky, the floor call site re-enabled (kernels.cu:341-345),
    counter RNG, a light so big that cosAMax is NaN for part of the scene (kernels.cu:371-372), and the coloured light `inside` of
    tests/mesh_lights_support.py: in the middle of the scene, with occluders behind it."""
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    nx, ny, ns = 64, 80, 2
    cam = rt.staircase_camera(nx, ny)
    opt = O.default_options(False)
    key = "mesh_staircase_" + "_".join(f"{k}{v}" for k, v in kw.items())
    kw = dict(kw)
    if "light_radius" in kw:
        opt.light.radius = kw.pop("light_radius")
    golden = GOLDEN_LIGHTS if "light" in kw else GOLDEN
    if "light" in kw:
        opt.light, opt.lightColor = M.light_structs(rt, L.light_of("stair_exact", kw.pop("light")))
    for k, v in kw.items():
        setattr(opt, k, v)
    lo = np.array(hm.view.bounds.min.e[:])
    floor = (0.0, 1.0, 0.0, 0.0, float(lo[1]) - 5.0, 0.0)                 # plane(point, norm): norm first (helper_structs.h:165-171)
    sc = O.mesh_scene(hm, mats, floor=floor)
    a, ca = O.render(sc, cam, opt, nx, ny, ns, 64, counters=True)
    ref = _reference(key, lambda: _mesh_frame_and_counters(sc, cam, opt, nx, ny, ns, 64), golden=golden)
    assert np.array_equal(_bits(a), _bits(ref["frame"])), np.count_nonzero(_bits(a) != _bits(ref["frame"]))
    assert np.array_equal(_counters(ca), ref["counters"])
    assert ca.ref_stats[rt.RT_STAT_PRIMARY] == nx * ny * ns and ca.ref_stats[rt.RT_STAT_PRIMARY] + ca.ref_stats[rt.RT_STAT_SECONDARY] == ca.rays
    if opt.nee:
        assert ca.ref_stats[rt.RT_STAT_SHADOWS] == ca.shadow_rays > 0


@pytest.mark.parametrize("n,nppl,nee,floor", [(1, 1, 1, 0), (7, 5, 1, 1), (65, 3, 0, 1), (1000, 5, 1, 0), (1000, 16, 0, 0), (300, 20, 1, 1)])
def test_mesh_frames_oracle_equals_reference_twin_soups(rt, n, nppl, nee, floor):
    _soup_frame_equals_reference_twin(rt, n, nppl, nee, floor, None)


@pytest.mark.parametrize("n,nppl,nee,floor,light", [(1000, 5, 1, 1, "inside"), (300, 20, 1, 1, "inside"), (1000, 5, 1, 1, "low"), (1000, 16, 0, 1, "sky")])
def test_mesh_frames_oracle_equals_reference_twin_soups_lights(rt, n, nppl, nee, floor, light):
    """The same soups under a coloured light of tests/mesh_lights_support.py (they fill the same box over the same floor as its soup_exact): `inside`
    among the triangles, `low` between the floor and the bounds (shadow rays from the floor end before they reach the bounds), `sky` with nee = 0 (seen
    directly by specular paths that leave the scene)."""
    _soup_frame_equals_reference_twin(rt, n, nppl, nee, floor, light)


def _soup_frame_equals_reference_twin(rt, n, nppl, nee, floor, light):
    """light: None = a light above the soup, outside its bounds; else the name of a light of tests/mesh_lights_support.py."""
    rng = np.random.default_rng(777 + 13 * n + nppl)
    tris, mats = _triangle_soup(rt, rng, n)
    tex = [rng.uniform(0, 1, (9, 13, 3)).astype(np.float32)]
    mats["texId"][3] = 0
    hm = rt.HostMesh.build(tris, nppl)
    nx, ny, ns = 56, 40, 3
    cam = rt.make_camera((4.5, 2.5, 6.0), (0, 0, 0), (0, 1, 0), 40.0, nx / ny, 0.02, 8.0)
    opt = O.default_options(False)
    opt.nee = nee
    opt.light.center.e[:] = (3.0, 9.0, 2.0); opt.light.radius = 1.5       # a light the soup can actually shadow
    opt.floor = floor
    key, golden = f"mesh_soup_{n}_{nppl}_{nee}_{floor}", GOLDEN
    if light is not None:
        opt.light, opt.lightColor = M.light_structs(rt, L.light_of("soup_exact", light))
        key, golden = f"{key}_{light}", GOLDEN_LIGHTS
    sc = O.mesh_scene(hm, mats, tex, floor=(0.0, 1.0, 0.0, 0.0, -3.0, 0.0))   # plane {norm, point} (helper_structs.h:165-171)
    a, ca = O.render(sc, cam, opt, nx, ny, ns, 12, counters=True)
    ref = _reference(key, lambda: _mesh_frame_and_counters(sc, cam, opt, nx, ny, ns, 12), golden=golden)
    assert np.array_equal(_bits(a), _bits(ref["frame"])), np.count_nonzero(_bits(a) != _bits(ref["frame"]))
    assert np.array_equal(_counters(ca), ref["counters"])
    if floor:       # primary rays that hit only the floor count as "primary nohit" (kernels.cu:430); paths leaving the floor into the sky as "secondary no hit"
        assert ca.ref_stats[rt.RT_STAT_SECONDARY_NOHIT] > 0 and ca.ref_stats[rt.RT_STAT_PRIMARY_NOHITS] > 0
    else:
        assert ca.ref_stats[rt.RT_STAT_SECONDARY_NOHIT] == 0
    if light == "low":
        assert 0 < ca.ref_stats[rt.RT_STAT_SHADOWS_BBOX_NOHITS] < ca.ref_stats[rt.RT_STAT_SHADOWS]
    if light == "inside":
        assert 0 < ca.ref_stats[rt.RT_STAT_SHADOWS_NOHITS] < ca.ref_stats[rt.RT_STAT_SHADOWS] and ca.ref_stats[rt.RT_STAT_SHADOWS_BBOX_NOHITS] == 0
    if light == "sky":
        black = rt.vec3()
        opt.lightColor = black
        assert np.count_nonzero((_bits(O.render(sc, cam, opt, nx, ny, ns, 12)[0]) != _bits(a)).any(axis=2)) >= 20       # the light is seen directly


def _shadow_rays(opt, cases, which):
    n = len(cases)
    r = {"generated": np.zeros(n, np.int32), "draws": np.zeros(n, np.int32), "rng_after": np.zeros(n, np.uint32),
         "dir": np.zeros((n, 3), np.float32), "contribution": np.zeros((n, 3), np.float32), "dist": np.zeros(n, np.float32),
         "cos_a_max": np.zeros(n, np.float32)}
    for k, (org, att, nrm, seed) in enumerate(cases):
        g = O.generate_shadow_ray(opt, org, att, nrm, seed, which)
        r["generated"][k], r["dir"][k], r["contribution"][k], r["dist"][k], r["cos_a_max"][k], r["draws"][k], r["rng_after"][k] = g
    return r


def test_generate_shadow_ray_oracle_equals_reference_twin(rt):
    """generateShadowRay as a whole (kernels.cu:363-393) on tabulated (origin, attenuation, normal, rng): every output bit-equal,
    incl. the NaN early-out before any draw and the dotl <= 0 rejection after two draws."""
    rng = np.random.default_rng(5)
    opt = O.default_options(False)
    cases = []
    for k in range(3000):
        if k % 10 == 9:                                   # inside the light's sphere: cosAMax = NaN
            org = np.array(opt.light.center.e[:]) + rng.normal(size=3) * 20.0
        else:
            org = rng.uniform(-300, 300, 3) + (0, 100, 0)
        att = rng.uniform(0, 1, 3)
        nrm = rng.normal(size=3); nrm /= np.linalg.norm(nrm)
        if k % 3 == 0:                                    # facing the light more often than not
            nrm = np.array(opt.light.center.e[:]) - org; nrm /= np.linalg.norm(nrm)
        cases.append((org, att, nrm, int(rng.integers(1, 2 ** 32)) | 1))
    ra = _shadow_rays(opt, cases, "orc")
    rb = _reference("shadow_rays", lambda: _shadow_rays(opt, cases, "ref"))
    n_gen = n_nan = n_rej = 0
    for k in range(len(cases)):
        assert ra["generated"][k] == rb["generated"][k] and ra["draws"][k] == rb["draws"][k] and ra["rng_after"][k] == rb["rng_after"][k], k
        assert _bits(ra["cos_a_max"][k]) == _bits(rb["cos_a_max"][k])                                   # cosAMax (NaN included: same bits)
        if ra["generated"][k]:
            n_gen += 1
            assert np.array_equal(_bits(ra["dir"][k]), _bits(rb["dir"][k])) and np.array_equal(_bits(ra["contribution"][k]), _bits(rb["contribution"][k])) \
                and _bits(ra["dist"][k]) == _bits(rb["dist"][k]), k
        elif ra["draws"][k] == 0:
            n_nan += 1
            assert np.isnan(ra["cos_a_max"][k])
        else:
            n_rej += 1
            assert ra["draws"][k] == 2
    assert n_gen > 500 and n_nan > 100 and n_rej > 100


@pytest.mark.parametrize("regime", [r["name"] for r in L.shadow_regimes()])
def test_generate_shadow_ray_regimes_oracle_equals_reference_twin(rt, regime):
    """The same on the regimes of tests/mesh_lights_support.py (shadow_regimes: a light of its own per regime - near, cosAMax = 1 by a small and by a
    zero radius, origins a float off the sphere's surface and at its centre, both sides of the tangent frame's switch, odd colours), and each regime
    yields the outcomes it is named for: the counts tests/test_gpu_probe_functions.py relies on."""
    reg = next(r for r in L.shadow_regimes() if r["name"] == regime)
    ra = L.regime_oracle(rt, O, reg)
    rb = _reference(f"shadow_regime_{regime}", lambda: L.regime_oracle(rt, O, reg, "ref"), golden=GOLDEN_LIGHTS)
    for k in ("generated", "draws", "rng_after"):
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(_bits(ra["cos_a_max"]), _bits(rb["cos_a_max"]))
    gen = ra["generated"] != 0
    for k in ("dir", "contribution", "dist"):
        assert np.array_equal(_bits(ra[k][gen]), _bits(rb[k][gen])), k
    got = L.regime_outcomes(ra)
    print(regime, got, "cosAMax", float(np.nanmin(ra["cos_a_max"])) if not np.isnan(ra["cos_a_max"]).all() else None, "to",
          float(np.nanmax(ra["cos_a_max"])) if not np.isnan(ra["cos_a_max"]).all() else None)
    for outcome, least in reg["expect"].items():
        assert got[outcome] >= least, (regime, outcome, got)
    cam = ra["cos_a_max"]
    if regime == "near":
        assert cam.min() < 0.1 and cam.max() < 0.87
    if regime in ("small", "zero"):
        assert (cam == 1.0).all() and (ra["contribution"][gen] == 0).all() and not np.signbit(ra["contribution"][gen]).any()
    if regime == "near_one":
        assert (cam < 1.0).all() and (cam > 0.99999).all()
    if regime == "surface":
        assert gen[0::2].sum() >= 100 and gen[1::2].sum() >= 100 and (~gen)[0::2].sum() >= 100 and (~gen)[1::2].sum() >= 100
    if regime == "switch":
        sw = np.array(reg["centre"]) - reg["org"].astype(np.float64)
        x = np.abs(sw[:, 0] / np.linalg.norm(sw, axis=1))
        assert (gen & (x > 0.0101)).sum() >= 100 and (gen & (x < 0.0099)).sum() >= 100
    if regime == "colour_3":
        c = ra["contribution"][gen]
        assert c[:, 0].max() > 1e28 and ((c[:, 2] != 0) & (np.abs(c[:, 2]) < 1.2e-38)).sum() >= 100       # subnormal results


# ---- the host I/O either side of the path, against the reference's own code -----------------------------------------

def test_bvh_file_written_here_loads_through_the_reference_loader(rt, tmp_path):
    """rtSaveBvhFile -> the reference's loadBVH (staircase_scene.h:75-101): triangles, nodes, bounds and the leaf size come back byte for byte;
    rtLoadBvhFile of the same file returns what loadBVH returns; both refuse a wrong header and a missing file.
    (Frozen: the sha256 of the file loadBVH read and of the arrays it returned.)"""
    cases = [(rt.scene_staircase_procedural(1)[0], 5, None), (rt.scene_staircase_procedural(1)[0][:333], 3, 2)]
    rng = np.random.default_rng(9)
    soup = np.zeros(57, rt.triangle_dtype)
    soup["v"] = rng.uniform(-3, 3, (57, 3, 3)).astype(np.float32)
    soup["meshID"] = rng.integers(0, 20, 57)
    cases.append((soup, 1, None))
    meshes, paths = [], []
    for k, (tris, nppl, levels) in enumerate(cases):
        hm = rt.HostMesh.build(tris, nppl, levels)
        path = str(tmp_path / f"m{k}.bvh")
        assert hm.save(path) == 0
        meshes.append(hm); paths.append(path)
    bad = str(tmp_path / "bad.bvh")
    open(bad, "wb").write(b"BVH_00.03\x00" + open(paths[0], "rb").read()[10:])

    def live():
        out = {"bad_refused": np.int32(O.ref_load_bvh(bad) is None), "missing_refused": np.int32(O.ref_load_bvh(str(tmp_path / "missing.bvh")) is None)}
        for k, path in enumerate(paths):
            got = O.ref_load_bvh(path)
            assert got is not None
            rtris, rbvh, rbounds, rnppl = got
            out.update({f"file_sha{k}": _sha(open(path, "rb").read()), f"tris_sha{k}": _sha(rtris.tobytes()), f"bvh_sha{k}": _sha(rbvh.tobytes()),
                        f"bounds{k}": np.frombuffer(rbounds.tobytes(), np.uint8), f"nppl{k}": np.int32(rnppl)})
        return out
    ref = _reference("bvh_loader", live)
    for k, hm in enumerate(meshes):
        assert np.array_equal(_sha(open(paths[k], "rb").read()), ref[f"file_sha{k}"])        # the very file the reference's loader read
        assert int(ref[f"nppl{k}"]) == cases[k][1] == hm.nppl
        assert np.array_equal(_sha(hm.tris.tobytes()), ref[f"tris_sha{k}"]) and np.array_equal(_sha(hm.bvh.tobytes()), ref[f"bvh_sha{k}"])
        assert bytes(hm.view.bounds) == ref[f"bounds{k}"].tobytes()
        hm2 = rt.HostMesh.load(paths[k])                               # our reader on the same file: what the reference's reader returned
        assert hm2.nppl == int(ref[f"nppl{k}"]) and np.array_equal(_sha(hm2.tris.tobytes()), ref[f"tris_sha{k}"])
        assert np.array_equal(_sha(hm2.bvh.tobytes()), ref[f"bvh_sha{k}"]) and bytes(hm2.view.bounds) == ref[f"bounds{k}"].tobytes()
        hm.close(); hm2.close()
    assert int(ref["bad_refused"]) == 1 and int(ref["missing_refused"]) == 1
    with pytest.raises(ValueError):
        rt.HostMesh.load(bad)


def test_ppm_bytes_equal_the_reference_writer(rt, tmp_path):
    """rtWritePPM's file = the bytes the reference's writePPM (staircase_scene.h:32-43) sends to std::cout: header, row order (top row first), sRGB
    quantisation of every channel, separators - on random frames incl. negative, > 1, NaN-free extremes."""
    rng = np.random.default_rng(11)
    fbs = []
    for (ny, nx) in ((1, 1), (7, 5), (33, 64)):
        fb = rng.uniform(-0.2, 1.4, (ny, nx, 3)).astype(np.float32)
        fb[0, 0] = (0.0, 1.0, 0.5)
        if ny > 1:
            fb[1, 0] = (1e-9, 1e9, 0.0031308)
        fbs.append(fb)
    ref = _reference("ppm", lambda: {f"ppm{k}": np.frombuffer(O.ref_write_ppm(fb), np.uint8) for k, fb in enumerate(fbs)})
    for k, fb in enumerate(fbs):
        path = str(tmp_path / "o.ppm")
        assert rt.write_ppm(path, fb) == 0
        assert open(path, "rb").read() == ref[f"ppm{k}"].tobytes()


def test_staircase_camera_equals_the_reference_setup_camera(rt):
    """rtStaircaseCamera = setup_camera (staircase_scene.h:62-73), every one of the 22 floats, for several image sizes."""
    sizes = ((640, 800), (1920, 1080), (160, 200), (48, 60), (1, 1), (1234, 567))
    ref = _reference("camera", lambda: {f"{nx}x{ny}": np.frombuffer(bytes(O.ref_setup_camera(nx, ny)), np.uint8) for nx, ny in sizes})
    for (nx, ny) in sizes:
        assert bytes(rt.staircase_camera(nx, ny)) == ref[f"{nx}x{ny}"].tobytes(), (nx, ny)


def test_ref_files_against_the_reference_main_cpp(rt, tmp_path):
    """REF_00.01 images (main.cpp:25-60): a file rtSaveReference writes loads through the reference's loadReference into the same floats, the file the
    reference's saveReference writes is byte-identical to ours and loads through rtLoadReference; a size mismatch and a missing file are refused by both."""
    rng = np.random.default_rng(13)
    nx, ny = 9, 6
    fb = rng.uniform(0, 1.3, (ny, nx, 3)).astype(np.float32)
    ours, theirs = str(tmp_path / "ours.ref"), str(tmp_path / "theirs.ref")
    assert rt.save_reference(ours, fb) == 0
    bad = str(tmp_path / "bad.ref")
    open(bad, "wb").write(b"REF_00.02\x00" + open(ours, "rb").read()[10:])

    def live():
        rm = O.load_ref_main()
        rm.ref_save_reference(theirs.encode(), nx, ny, fb.ctypes.data)
        back = np.zeros_like(fb)
        rc = rm.ref_load_reference(ours.encode(), back.ctypes.data, nx, ny)
        return {"theirs": np.frombuffer(open(theirs, "rb").read(), np.uint8), "ours_sha": _sha(open(ours, "rb").read()),
                "load_rc": np.int32(rc), "loaded": back.copy(),
                "transposed_rc": np.int32(rm.ref_load_reference(ours.encode(), back.ctypes.data, ny, nx)),
                "missing_rc": np.int32(rm.ref_load_reference(str(tmp_path / "none.ref").encode(), back.ctypes.data, nx, ny)),
                "bad_rc": np.int32(rm.ref_load_reference(bad.encode(), back.ctypes.data, nx, ny))}
    ref = _reference("ref_files", live, O.have_ref_main)
    assert np.array_equal(_sha(open(ours, "rb").read()), ref["ours_sha"])          # the very file the reference's loader read
    assert open(ours, "rb").read() == ref["theirs"].tobytes()
    assert int(ref["load_rc"]) == 0 and ref["loaded"].tobytes() == fb.tobytes()
    open(theirs, "wb").write(ref["theirs"].tobytes())
    rc, back2 = rt.load_reference(theirs, nx, ny)
    assert rc == 0 and back2.tobytes() == fb.tobytes()
    assert int(ref["transposed_rc"]) != 0 and rt.load_reference(ours, ny, nx)[0] != 0
    assert int(ref["missing_rc"]) != 0
    assert int(ref["bad_rc"]) != 0 and rt.load_reference(bad, nx, ny)[0] != 0
