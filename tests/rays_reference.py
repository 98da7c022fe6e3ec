"""The test reference of traceRays / occludedRays (include/rt_api.h) and the ray sets the ray tests send.  No test: read by tests/test_rays_api.py (CPU: the
conditions every set is there to meet, the reference against the guide reference) and tests/test_gpu_rays.py (GPU: every plane of every set, bit for bit).

The reference is built from the CPU oracle's own functions through ctypes, the way tests/guides_reference.py is, and from nothing of the code under test:
orc_sphere_hit in the caller's order against the running closest t (which starts at the ray's t_max), orc_hit_bbox + orc_hit_bvh with is_shadow 0 and 1 and
orc_counters.node_visits, orc_plane_hit against the ray's own t_max.  The oracle's functions normalise the direction they are given once (ray.h:9), as
traceRays does.  A t_max above FLT_MAX is taken as FLT_MAX before any of them is called, as the contract says (clamp_t_max; tests/test_rays_api.py records
what the unclamped calls answer).  Hit point and normal are restated in numpy float32, operation by operation (guides_reference's _unit / _dot / _cross).

The scenes are frames of guides_reference (the ray calls do not depend on the camera or the image size; the frame only names the scene to initialise).
Every set is seeded."""
import ctypes as C
import functools

import numpy as np

import guides_reference as G
from guides_reference import F, FLT_MAX, PRIM_FLOOR, PRIM_NONE, _cross, _dot, _f3, _unit

PLANES = ("t", "prim", "normal", "uv", "nodes")
CENTRE_FRAMES = ("random_50x37", "tie_mirror", "cloud_hybrid", "cloud_global", "staircase_a", "tris300_floor")
SETS = tuple("centre:" + f for f in CENTRE_FRAMES) + ("sph_random:three_spheres", "sph_random:random_50x37", "sph_axis:tie_mirror",
                                                      "mesh_random:tris300", "mesh_random:tris300_floor", "mesh_random:staircase_a",
                                                      "mesh_axis:tris300", "mesh_axis:staircase_a", "mesh_surface:staircase_a", "mesh_surface:tris300",
                                                      "sph_surface:random_50x37", "sph_axis:cloud_hybrid", "sph_axis:cloud_global",
                                                      "mesh_inf:tris300", "sph_inf:three_spheres")
RANDOM_SETS = tuple(s for s in SETS if "_random:" in s)
OWN_BOUNDS_SHARE = 0.3                                          # of the rays of a random set draw their own t_min / t_max


def is_mesh(frame):
    return frame in G.MESH_FRAMES


def default_t_min(frame):
    return 0.01 if is_mesh(frame) else 0.001                    # getDefaultRenderOptions (kernels.cu:19 for meshes)


def frame_of(name):
    return name.split(":")[1]


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------

def _c3(v):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))


def clamp_t_max(t_max):
    """The contract's reading of the upper bounds: a t_max above FLT_MAX (+inf) is taken as FLT_MAX."""
    return np.minimum(np.asarray(t_max, np.float32), np.float32(FLT_MAX))


def _empty(n, mesh):
    out = {"t": np.full(n, FLT_MAX, np.float32), "prim": np.full(n, PRIM_NONE, np.int32), "normal": np.zeros((n, 3), np.float32),
           "uv": np.zeros((n, 2), np.float32), "occluded": np.zeros(n, np.uint8)}
    if mesh:
        out["nodes"] = np.zeros(n, np.int32)
    return out


def sphere_rays(rt, O, spheres, org, dir, t_min, t_max, clamp=True):
    """t, prim, normal, uv and occluded of rays against a sphere scene; t_min, t_max: one float32 per ray.  clamp = False: the oracle's calls on the raw
    t_max, which is not the contract (only the test that records why the clamp exists asks for it)."""
    lib = O.load_oracle()
    spheres = np.ascontiguousarray(spheres, dtype=rt.sphere_dtype)
    sp_ptr = [C.cast(spheres.ctypes.data + 16 * k, C.POINTER(rt.sphere)) for k in range(len(spheres))]
    hit = lib.orc_sphere_hit
    n = len(org)
    out = _empty(n, False)
    t_max = clamp_t_max(t_max) if clamp else np.asarray(t_max, np.float32)
    for r in range(n):
        o, d = _c3(org[r]), _c3(dir[r])
        tmin, tmax = C.c_float(t_min[r]), float(np.float32(t_max[r]))
        closest, sid = tmax, -1
        for k, sp in enumerate(sp_ptr):                         # strict <: the lower index keeps an equal t, and a hit at t_max is none
            t = hit(sp, o, d, tmin, closest)
            if t < closest:
                closest, sid = t, k
        # occluded: some sphere with sphereHit(s, ray, tmin, tmax) < FLT_MAX.  Up to the first accepted hit `closest` is still tmax, so the calls above ARE
        # that definition's calls: it holds iff one of them was accepted.
        if sid < 0:
            continue
        out["occluded"][r] = 1
        of, dn = _f3(org[r]), _unit(_f3(dir[r]))                # mkray: the ray's direction
        t = F(closest)
        p = [of[a] + t * dn[a] for a in range(3)]
        c, rad = _f3(spheres["center"][sid]), F(spheres["radius"][sid])
        nrm = [(p[a] - c[a]) / rad for a in range(3)]
        if _dot(dn, nrm) > F(0.0):
            nrm = [-x for x in nrm]
        out["t"][r] = t
        out["prim"][r] = sid
        out["normal"][r] = nrm
    return out


def sphere_occluded_by_definition(rt, O, spheres, org, dir, t_min, t_max):
    """occludedRays' definition word for word, every sphere against the ray's own t_max (the self-consistency test holds sphere_rays' shortcut to it)."""
    lib = O.load_oracle()
    spheres = np.ascontiguousarray(spheres, dtype=rt.sphere_dtype)
    sp_ptr = [C.cast(spheres.ctypes.data + 16 * k, C.POINTER(rt.sphere)) for k in range(len(spheres))]
    out = np.zeros(len(org), np.uint8)
    for r in range(len(org)):
        o, d, tmin, tmax = _c3(org[r]), _c3(dir[r]), C.c_float(t_min[r]), C.c_float(t_max[r])
        out[r] = any(lib.orc_sphere_hit(sp, o, d, tmin, tmax) < FLT_MAX for sp in sp_ptr)
    return out


def mesh_rays(rt, O, hm, materials, textures, floor, org, dir, t_min, t_max, clamp=True):
    """The five planes and occluded of rays against a mesh scene; floor = (norm xyz, point xyz) with rt_render_options.floor = 1, None without.
    clamp = False: as in sphere_rays."""
    lib = O.load_oracle()
    scene = O.mesh_scene(hm, materials, textures, floor)
    tris = hm.tris
    bmin = (C.c_float * 3)(*[hm.view.bounds.min.e[a] for a in range(3)])
    bmax = (C.c_float * 3)(*[hm.view.bounds.max.e[a] for a in range(3)])
    plane = rt.plane()
    if floor is not None:
        for a in range(3):
            plane.norm.e[a] = float(floor[a]); plane.point.e[a] = float(floor[3 + a])
    n = len(org)
    out = _empty(n, True)
    t_max = clamp_t_max(t_max) if clamp else np.asarray(t_max, np.float32)
    for r in range(n):
        o, d = _c3(org[r]), _c3(dir[r])
        tmin, tmax = C.c_float(t_min[r]), C.c_float(t_max[r])
        of, dn = _f3(org[r]), _unit(_f3(dir[r]))
        t, prim, nrm = FLT_MAX, PRIM_NONE, None
        if lib.orc_hit_bbox(bmin, bmax, o, d, tmax):                # hitMesh: the scene bounds first, against the ray's own t_max
            cnt = O.orc_counters()
            tri_id, hu, hv = C.c_uint32(0), C.c_float(0), C.c_float(0)
            x = lib.orc_hit_bvh(C.byref(scene), o, d, tmin, tmax, 0, C.byref(tri_id), C.byref(hu), C.byref(hv), C.byref(cnt))
            out["nodes"][r] = cnt.node_visits
            if x < tmax.value:
                t, prim = x, int(tri_id.value)
                tri = tris[prim]
                v0, v1, v2 = _f3(tri["v"][0]), _f3(tri["v"][1]), _f3(tri["v"][2])
                nrm = _unit(_cross([v1[a] - v0[a] for a in range(3)], [v2[a] - v0[a] for a in range(3)]))
                out["uv"][r] = (hu.value, hv.value)
            cnt2 = O.orc_counters()
            tri2, u2, v2_ = C.c_uint32(0), C.c_float(0), C.c_float(0)
            y = lib.orc_hit_bvh(C.byref(scene), o, d, tmin, tmax, 1, C.byref(tri2), C.byref(u2), C.byref(v2_), C.byref(cnt2))
            out["occluded"][r] = 1 if y < tmax.value else 0
        if prim == PRIM_NONE and floor is not None:
            x = lib.orc_plane_hit(C.byref(plane), o, d, tmin, tmax)        # against the ray's own t_max
            if x < FLT_MAX:
                t, prim, nrm = x, PRIM_FLOOR, _f3(floor[:3])
        if prim == PRIM_NONE:
            continue
        if _dot(dn, nrm) > F(0.0):
            nrm = [-x for x in nrm]
        out["t"][r] = F(t)
        out["prim"][r] = prim
        out["normal"][r] = nrm
    return out


# ---------------------------------------------------------------------------------------------
# the ray sets
# ---------------------------------------------------------------------------------------------

def _directions(rng, n, min_comp=0.0):
    """Uniform on the sphere (every component of the unit direction at least min_comp in magnitude), scaled by 10**U(-2, 2): normalisation is exercised."""
    out = np.zeros((n, 3))
    for k in range(n):
        while True:
            v = rng.normal(size=3)
            v /= np.sqrt((v * v).sum())
            if np.abs(v).min() >= min_comp:
                break
        out[k] = v
    return (out * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)


def _own_bounds(rng, n, frame):
    """30 % of the rays draw t_min in [0.001, 2] and t_max in [t_min + 0.1, 30]; the others carry the default t_min of the scene kind and FLT_MAX."""
    t_min = np.full(n, default_t_min(frame), np.float32)
    t_max = np.full(n, FLT_MAX, np.float32)
    own = rng.uniform(size=n) < OWN_BOUNDS_SHARE
    lo = rng.uniform(0.001, 2.0, n)
    hi = rng.uniform(lo + 0.1, 30.0)
    t_min[own] = lo[own].astype(np.float32)
    t_max[own] = hi[own].astype(np.float32)
    return t_min, t_max, own


def _centre_set(rt, O, frame):
    lib = O.load_oracle()
    if is_mesh(frame):
        f = G.mesh_frame(rt, O, frame)
        cam, nx, ny = f["cam"], f["nx"], f["ny"]
    else:
        _, _, cam, nx, ny = G.sphere_frame(rt, frame)
    cam0 = G._camera_without_lens(rt, cam)
    org, d = np.zeros((ny * nx, 3), np.float32), np.zeros((ny * nx, 3), np.float32)
    for j in range(ny):
        for i in range(nx):
            o, dd = G._centre_ray(lib, rt, cam0, i, j, nx, ny)
            org[j * nx + i] = [o[a] for a in range(3)]
            d[j * nx + i] = [dd[a] for a in range(3)]
    return org, d, None, None


def _sph_random_set(rt, O, frame):
    """1000 rays: origins through the scene's extent (a quarter of the box lies inside the ground sphere), 150 more of them put strictly inside a sphere
    chosen at random."""
    n, inside = 1000, 150
    sp = np.ascontiguousarray(G.sphere_frame(rt, frame)[0], dtype=rt.sphere_dtype)
    rng = np.random.default_rng(101 if frame == "three_spheres" else 102)
    if frame == "three_spheres":
        lo, hi = np.array([-2.5, -1.5, -3.0]), np.array([2.5, 1.5, 1.5])
    else:
        lo, hi = np.array([-12.0, -1.0, -12.0]), np.array([12.0, 3.0, 12.0])
    org = rng.uniform(lo, hi, (n, 3))
    pick = rng.integers(0, len(sp), inside)
    off = rng.normal(size=(inside, 3))
    off /= np.sqrt((off * off).sum(axis=1, keepdims=True))
    org[:inside] = sp["center"][pick] + off * (sp["radius"][pick] * rng.uniform(0.05, 0.9, inside))[:, None]
    org = org.astype(np.float32)
    d = _directions(rng, n)
    t_min, t_max, _ = _own_bounds(rng, n, frame)
    return org, d, t_min, t_max


def _sph_axis_set(rt, O, frame):
    """48 rays with one or two direction components exactly 0.  The clouds: _sph_axis_cloud_set.  tie_mirror: 16 in the plane x = 0 aimed into the lens the overlapping pair (indices 1, 2 at
    x = +-0.2) shares - both spheres at the same t bit for bit -, 16 along an axis through a sphere's centre, 16 with one zero component elsewhere."""
    if frame != "tie_mirror":
        return _sph_axis_cloud_set(rt, O, frame)
    sp = np.ascontiguousarray(G.sphere_frame(rt, frame)[0], dtype=rt.sphere_dtype)
    rng = np.random.default_rng(103)
    org, d = np.zeros((48, 3), np.float32), np.zeros((48, 3), np.float32)
    for k in range(16):                                         # x = 0 plane: origin and target both on it
        o = np.array([0.0, rng.uniform(0.2, 3.0), rng.choice([-1.0, 1.0]) * rng.uniform(3.0, 6.0)], np.float32)
        target = np.array([0.0, 0.5 + rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)], np.float32)
        v = (target - o) * np.float32(rng.choice([0.03, 1.0, 7.0]))
        if k < 6:
            o[1] = target[1]; v = np.array([0.0, 0.0, -np.sign(o[2]) * rng.uniform(0.1, 5.0)], np.float32)      # two zero components
        org[k], d[k] = o, v
    for k in range(16):                                         # along an axis through a centre
        c = sp["center"][1 + int(rng.integers(0, 24))]
        axis, sign = int(rng.integers(0, 3)), float(rng.choice([-1.0, 1.0]))
        v = np.zeros(3, np.float32); v[axis] = sign * rng.uniform(0.05, 20.0)
        o = c.copy(); o[axis] -= np.float32(sign * rng.uniform(2.0, 8.0))
        org[16 + k], d[16 + k] = o, v
    for k in range(16):                                         # one zero component
        v = rng.normal(size=3) * 10.0 ** rng.uniform(-1, 1); v[int(rng.integers(0, 3))] = 0.0
        org[32 + k] = rng.uniform([-6, 0.1, -4], [6, 2.0, 5])
        d[32 + k] = v
    return org, d, None, None


def _mesh_random_set(rt, O, frame):
    """tris300 and tris300_floor share their rays (the floor is an option, not geometry).  Origins: half inside the bounds; a quarter outside aimed
    at a triangle; a quarter outside pointing away from the centre (these miss the bounds).  Every component of every unit direction is at least 1e-3 in magnitude:
    a ray lying in a slab plane puts 0 * inf into the box test, whose device form belongs to the render path (csrc/rt_device.h).  Those rays are the mesh_axis
    sets' (mesh_axis_build)."""
    n = 600 if frame == "staircase_a" else 1000
    f = G.mesh_frame(rt, O, "tris300" if frame.startswith("tris300") else frame)
    b = f["hm"].view.bounds
    lo, hi = np.array([b.min.e[a] for a in range(3)], np.float64), np.array([b.max.e[a] for a in range(3)], np.float64)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    rng = np.random.default_rng(104 if frame == "staircase_a" else 105)
    tris = f["hm"].tris
    tris = tris[np.isfinite(tris["v"]).all(axis=(1, 2))]         # (not the leaves' sentinel triangles)
    org = rng.uniform(lo, hi, (n, 3))
    d = _directions(rng, n, 2e-3).astype(np.float64)
    n_in, n_aim = n // 2, n // 4
    for k in range(n_in, n):                                    # outside the bounds
        while True:
            p = centre + half * rng.uniform(-3, 3, 3)
            if np.any(np.abs(p - centre) > half * 1.05):
                break
        org[k] = p
        scale = 10.0 ** rng.uniform(-2, 2)
        while True:
            if k < n_in + n_aim:
                v = tris["v"][int(rng.integers(0, len(tris)))].mean(axis=0) + rng.normal(size=3) * 0.2 - p       # at a triangle, roughly
            else:
                v = (p - centre) / half + rng.normal(size=3) * 0.05      # away
            v /= np.sqrt((v * v).sum())
            if np.abs(v).min() >= 2e-3:
                break
        d[k] = v * scale
    t_min, t_max, _ = _own_bounds(rng, n, frame)
    return org.astype(np.float32), d.astype(np.float32), t_min, t_max


def _zero(kind):
    """The zero of a ray kind: +0.0 for the even kinds, -0.0 for the odd ones (1 / -0 = -inf takes the swap branch of the slab test)."""
    return np.float32(-0.0) if kind % 2 else np.float32(0.0)


def _in_plane_direction(rng, axis, zero):
    """A direction with `zero` on `axis` and the other two components at least 2e-3 of its length in magnitude, scaled by 10**U(-2, 2)."""
    while True:
        v = rng.normal(size=2)
        v /= np.sqrt((v * v).sum())
        if np.abs(v).min() >= 2e-3:
            break
    d = np.zeros(3, np.float32)
    d[[a for a in range(3) if a != axis]] = (v * 10.0 ** rng.uniform(-2, 2)).astype(np.float32)
    d[axis] = zero
    return d


@functools.lru_cache(maxsize=None)
def mesh_axis_build(rt, O, frame):
    """(org, dir, t_min, t_max, info) of mesh_axis:<frame>: 600 rays, six kinds of 100, every ray with at least one direction component exactly zero (+0.0 in
    the even kinds, -0.0 in the odd ones) and own bounds drawn by _own_bounds.
    0, 1: two zero components - along one axis from 1.0 outside the scene bounds, the other two origin coordinates inside them.
    2, 3: one zero component, the origin anywhere in the bounds widened by half their extent.
    4:    one zero component on axis a and org[a] exactly on a plane of a node box: on staircase_a a box that is flat on a (lo[a] == hi[a]), the origin displaced
          inside that plane and the ray aimed at a point of the flat box - both slab products of that axis are 0 * inf = NaN -; on tris300, which has no flat
          box, either plane of one of the nodes 1 to 64, the ray aimed at a point of that box.
    5:    as 4 with a plane of the scene bounds (node 1): the root test itself meets the NaN.  The ray is aimed at a point of the bounds.
    info: kind, axis (the zero axis of kinds 2 to 5, the ray's axis of kinds 0 and 1), node and side (0: lo, 1: hi) of kinds 4 and 5, one entry per ray."""
    n, per = 600, 100
    hm = G.mesh_frame(rt, O, frame)["hm"]
    nodes = hm.bvh
    first_leaf = hm.view.numBvhNodes // 2
    lo, hi = nodes["a"][1].astype(np.float64), nodes["b"][1].astype(np.float64)
    assert np.array_equal(nodes["a"][1], [hm.view.bounds.min.e[a] for a in range(3)]) and np.array_equal(nodes["b"][1], [hm.view.bounds.max.e[a] for a in range(3)])
    ext = hi - lo
    rng = np.random.default_rng(106 if frame == "staircase_a" else 107)
    real = np.isfinite(nodes["a"]).all(axis=1) & np.isfinite(nodes["b"]).all(axis=1)
    real[0] = False
    flat = [np.flatnonzero(real & (nodes["a"][:, a] == nodes["b"][:, a])) for a in range(3)]
    org, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    info = {k: np.full(n, -1, np.int32) for k in ("kind", "axis", "node", "side")}
    for k in range(n):
        kind = k // per
        zero = _zero(kind)
        a = int(rng.integers(0, 3))
        others = [b for b in range(3) if b != a]
        node = side = -1
        if kind < 2:
            sign = float(rng.choice([-1.0, 1.0]))
            o = rng.uniform(lo, hi)
            o[a] = lo[a] - 1.0 if sign > 0 else hi[a] + 1.0
            v = np.full(3, zero, np.float32)
            v[a] = np.float32(sign * 10.0 ** rng.uniform(-2, 2))
        elif kind < 4:
            o = rng.uniform(lo - ext / 2, hi + ext / 2)
            v = _in_plane_direction(rng, a, zero)
        else:
            if kind == 5:
                node = 1
            elif frame == "staircase_a":
                assert all(len(f) >= 100 for f in flat), [len(f) for f in flat]
                node = int(rng.choice(flat[a]))
            else:
                assert not any(len(f) for f in flat) and first_leaf > 64
                node = int(rng.integers(1, 65))
            side = int(rng.integers(0, 2))
            blo, bhi = nodes["a"][node].astype(np.float64), nodes["b"][node].astype(np.float64)
            target = rng.uniform(blo, bhi)
            o = target + rng.normal(size=3) * np.maximum(bhi - blo, 0.05 * ext)        # displaced inside the plane: axis a is overwritten below
            v = ((target - o) * 10.0 ** rng.uniform(-2, 2)).astype(np.float32)
            assert np.all(v[others] != 0)
            v[a] = zero
            o = o.astype(np.float32)
            o[a] = (nodes["a"] if side == 0 else nodes["b"])[node][a]                   # the plane's own float32
        org[k], d[k] = o, v
        info["kind"][k], info["axis"][k], info["node"][k], info["side"][k] = kind, a, node, side
    t_min, t_max, _ = _own_bounds(rng, n, frame)
    for arr in info.values():
        arr.setflags(write=False)
    return org, d, t_min, t_max, info


def _mesh_axis_set(rt, O, frame):
    return mesh_axis_build(rt, O, frame)[:4]


SURFACE_T_MIN = {"mesh": (0.0, 1e-42, 1e-6, 0.01), "sph": (0.0, 1e-42, 1e-6, 0.001)}      # cycled over the rays; 1e-42 is a denormal


@functools.lru_cache(maxsize=None)
def surface_build(rt, O, name):
    """(org, dir, t_min, t_max, prim) of mesh_surface:<frame> / sph_surface:<frame>: the origins are the float32 hit points org + t * unit(dir) of the
    NULL-bounds reference of the frame's random set (triangles and spheres only, not the floor; the first 600 of them), prim the primitive each origin lies on; new directions from
    _directions(rng, m, 2e-3); t_min cycles through SURFACE_T_MIN, t_max is FLT_MAX."""
    kind, frame = name.split(":")
    src = ("mesh_random:" if kind == "mesh_surface" else "sph_random:") + frame
    o, dd, _, _ = ray_set(rt, O, src)
    ref = reference(rt, O, src, own=False)
    hit = np.flatnonzero(ref["prim"] >= 0)[:600]                    # (a set holds at most 600 rays)
    org = np.zeros((len(hit), 3), np.float32)
    for k, r in enumerate(hit):
        of, dn, t = _f3(o[r]), _unit(_f3(dd[r])), F(ref["t"][r])
        org[k] = [of[a] + t * dn[a] for a in range(3)]
    rng = np.random.default_rng({"mesh_surface:staircase_a": 108, "mesh_surface:tris300": 109, "sph_surface:random_50x37": 110}[name])
    d = _directions(rng, len(hit), 2e-3)
    cycle = np.array(SURFACE_T_MIN["mesh" if kind == "mesh_surface" else "sph"], np.float32)
    t_min = cycle[np.arange(len(hit)) % 4]
    t_max = np.full(len(hit), FLT_MAX, np.float32)
    prim = ref["prim"][hit].copy()
    prim.setflags(write=False)
    return org, d, t_min, t_max, prim


def _surface_set(name):
    return lambda rt, O, frame: surface_build(rt, O, name)[:4]


def _sph_axis_cloud_set(rt, O, frame):
    """48 rays against a cloud (the hybrid and the global scene copy, whose culling must keep a node on the NaN of an axis-parallel ray): 16 along an axis
    through a sphere's centre, 16 with two zero components through random points of the scene's extent, 16 with one zero component; every other zero is -0.0."""
    sp = np.ascontiguousarray(G.sphere_frame(rt, frame)[0], dtype=rt.sphere_dtype)
    rng = np.random.default_rng(116 if frame == "cloud_hybrid" else 112)
    c = sp["center"].astype(np.float64)
    small = sp["radius"] < 10.0                                    # (not a ground sphere, should the scene have one)
    lo, hi = c[small].min(axis=0), c[small].max(axis=0)
    org, d = np.zeros((48, 3), np.float32), np.zeros((48, 3), np.float32)
    zeros = 0

    def zero():
        nonlocal zeros
        zeros += 1
        return np.float32(-0.0) if zeros % 2 else np.float32(0.0)

    for k in range(32):
        axis, sign = int(rng.integers(0, 3)), float(rng.choice([-1.0, 1.0]))
        v = np.array([zero() if a != axis else 0.0 for a in range(3)], np.float32)
        v[axis] = sign * rng.uniform(0.05, 20.0)
        if k < 16:                                                  # through a centre, from outside the sphere
            pick = int(rng.choice(np.flatnonzero(small)))
            o = sp["center"][pick].copy()
            o[axis] -= np.float32(sign * (sp["radius"][pick] + rng.uniform(0.5, 4.0)))
        else:                                                       # through a random point of the extent
            o = rng.uniform(lo, hi).astype(np.float32)
        org[k], d[k] = o, v
    for k in range(32, 48):                                         # one zero component
        v = (rng.normal(size=3) * 10.0 ** rng.uniform(-1, 1)).astype(np.float32)
        v[int(rng.integers(0, 3))] = zero()
        org[k] = rng.uniform(lo, hi)
        d[k] = v
    return org, d, None, None


def _inf_set(src):
    """The rays of `src` with the t_max of every ray k % 3 == 0 replaced by +inf and of every ray k % 3 == 1 by FLT_MAX."""
    def build(rt, O, frame):
        org, d, t_min, t_max = ray_set(rt, O, src)
        t_max = t_max.copy()
        k = np.arange(len(t_max))
        t_max[k % 3 == 0] = np.inf
        t_max[k % 3 == 1] = FLT_MAX
        return org, d, t_min, t_max
    return build


@functools.lru_cache(maxsize=None)
def ray_set(rt, O, name):
    """(org (n, 3), dir (n, 3), t_min (n,) or None, t_max (n,) or None) of a named set; None: the set has no bounds of its own."""
    kind, frame = name.split(":")
    builders = {"centre": _centre_set, "sph_random": _sph_random_set, "mesh_random": _mesh_random_set, "mesh_axis": _mesh_axis_set,
                "sph_axis": _sph_axis_set, "mesh_surface": _surface_set(name), "sph_surface": _surface_set(name),
                "mesh_inf": _inf_set("mesh_random:" + frame), "sph_inf": _inf_set("sph_random:" + frame)}
    org, d, t_min, t_max = builders[kind](rt, O, frame)
    for a in (org, d, t_min, t_max):
        if a is not None:
            a.setflags(write=False)
    return org, d, t_min, t_max


def bounds_of(rt, O, name, own=True, t_min=None):
    """The per-ray bounds a call works with: the set's own arrays (own, where the set has them), else t_min (default: the scene kind's) and FLT_MAX."""
    org, _, tmin_a, tmax_a = ray_set(rt, O, name)
    if own and tmin_a is not None:
        return tmin_a, tmax_a
    n = len(org)
    return np.full(n, default_t_min(frame_of(name)) if t_min is None else t_min, np.float32), np.full(n, FLT_MAX, np.float32)


@functools.lru_cache(maxsize=None)
def reference(rt, O, name, own=True, t_min=None, floor=None):
    """The planes and `occluded` of a named set: with its own bounds, or (own = False) with t_min - default: the scene kind's - and FLT_MAX for every ray.
    floor: None = the frame's (on for tris300_floor), True / False = the option toggled on a tris300 frame."""
    frame = frame_of(name)
    org, d, _, _ = ray_set(rt, O, name)
    tmin_a, tmax_a = bounds_of(rt, O, name, own, t_min)
    if is_mesh(frame):
        f = G.mesh_frame(rt, O, frame)
        fl = f["floor"]
        if floor is not None:
            fl = G.mesh_frame(rt, O, "tris300_floor")["floor"] if floor else None
        out = mesh_rays(rt, O, f["hm"], f["mats"], f["tex"], fl, org, d, tmin_a, tmax_a)
    else:
        out = sphere_rays(rt, O, G.sphere_frame(rt, frame)[0], org, d, tmin_a, tmax_a)
    for a in out.values():
        a.setflags(write=False)
    return out


def material_kinds(rt, O, name, prim):
    """The (type, textured) pairs of the materials of the triangles in `prim` (mesh sets)."""
    f = G.mesh_frame(rt, O, frame_of(name))
    ids = f["hm"].tris["meshID"][prim[prim >= 0]]
    return sorted({(int(f["mats"]["type"][m]), bool(f["mats"]["texId"][m] != -1)) for m in np.unique(ids)})
