"""CPU checks of the batched ray queries (include/rt_api.h): traceRays / occludedRays / rtLastRaysMs and rtCentreRays are declared, exported and bound with
their argument types, the constants agree between header and Python, the ABI version and struct sizes are the parent's, every call before init is the
library's misuse exit, rt.centre_rays is orc_get_ray on the lens-less camera bit for bit, and the test reference (tests/rays_reference.py) shows on every
ray set of the GPU tests what that set is there to cover - a set that exercises nothing fails here, without a GPU - and agrees with the guide reference.
The edge sets (exactly-zero direction components, origins on box planes and on surfaces, t_max = +inf) carry conditions on their inputs, not tolerances: a
seed that misses one is changed, never the threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import guides_reference as G
import rays_reference as R
from preview_support import bits, exits_99, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
HOST_H = open(os.path.join(ROOT, "include", "rt_host.h")).read()
NEW = ("traceRays", "occludedRays", "rtLastRaysMs")
FLT_MAX = R.FLT_MAX


def test_declared_exported_and_bound(rt):
    assert re.search(r"void\s+traceRays\s*\(\s*int\s+n\s*,\s*const\s+float\s*\*\s*org\s*,\s*const\s+float\s*\*\s*dir\s*,\s*const\s+float\s*\*\s*t_min\s*,"
                     r"\s*const\s+float\s*\*\s*t_max\s*,\s*int\s+mask\s*,\s*float\s*\*\s*t\s*,\s*int32_t\s*\*\s*prim\s*,\s*float\s*\*\s*normal\s*,"
                     r"\s*float\s*\*\s*uv\s*,\s*int32_t\s*\*\s*nodes\s*\)\s*;", API)
    assert re.search(r"void\s+occludedRays\s*\(\s*int\s+n\s*,\s*const\s+float\s*\*\s*org\s*,\s*const\s+float\s*\*\s*dir\s*,\s*const\s+float\s*\*\s*t_min\s*,"
                     r"\s*const\s+float\s*\*\s*t_max\s*,\s*uint8_t\s*\*\s*occluded\s*\)\s*;", API)
    assert re.search(r"double\s+rtLastRaysMs\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"void\s+rtCentreRays\s*\(\s*const\s+rt_camera\s*\*\s*cam\s*,\s*int\s+nx\s*,\s*int\s+ny\s*,\s*const\s+int32_t\s*\*\s*ij\s*,\s*int\s+n\s*,"
                     r"\s*float\s*\*\s*org\s*,\s*float\s*\*\s*dir\s*\)\s*;", HOST_H)
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    host = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_host.so"))
    assert hasattr(host, "rtCentreRays") and "rtCentreRays" in rt.HOST_SYMBOLS
    r, h = rt.load_renderer(), rt.load_host()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert r.traceRays.argtypes == [C.c_int, fp, fp, fp, fp, C.c_int, fp, ip, fp, fp, ip] and r.traceRays.restype is None
    assert r.occludedRays.argtypes == [C.c_int, fp, fp, fp, fp, C.POINTER(C.c_uint8)] and r.occludedRays.restype is None
    assert r.rtLastRaysMs.argtypes == [] and r.rtLastRaysMs.restype is C.c_double
    assert h.rtCentreRays.argtypes == [C.POINTER(rt.camera), C.c_int, C.c_int, ip, C.c_int, fp, fp] and h.rtCentreRays.restype is None
    for name in ("trace_rays", "occluded_rays", "last_rays_ms", "centre_rays"):
        assert callable(getattr(rt, name)), name


def test_constants_agree_between_header_and_python(rt):
    line = re.search(r"^enum \{ (RT_RAY_T = [^}]*)\};", API, re.M).group(1)
    enums = dict(re.findall(r"\b(RT_RAY_[A-Z_]+)\s*=\s*(-?\d+)", line))
    assert {k: int(v) for k, v in enums.items()} == {"RT_RAY_T": 1, "RT_RAY_PRIM": 2, "RT_RAY_NORMAL": 4, "RT_RAY_UV": 8, "RT_RAY_NODES": 16}
    for name, value in enums.items():
        assert getattr(rt, name) == int(value), name
    assert re.search(r"#define RT_RAY_CHUNK \(1 << 22\)", API) and rt.RT_RAY_CHUNK == 1 << 22
    assert [(n, b) for n, b, _, _ in rt.RAY_PLANES] == [("t", 1), ("prim", 2), ("normal", 4), ("uv", 8), ("nodes", 16)]
    assert tuple(n for n, _, _, _ in rt.RAY_PLANES) == R.PLANES


def test_abi_unchanged(rt):
    assert rt.load_renderer().rtApiVersion() == 1002 == rt.RT_API_VERSION
    assert re.search(r"#define RT_API_VERSION 1002\b", API)
    sizes = (C.c_int32 * 32)()
    n = rt.load_renderer().rtStructSizes(sizes, 32)
    assert n == 13 and [sizes[k] for k in range(n)] == [C.sizeof(s) for s in rt.ABI_STRUCTS]


_RAYS = "o = np.zeros((4, 3), np.float32); d = np.ones((4, 3), np.float32)\n"


@pytest.mark.parametrize("call", ["rt.trace_rays(o, d, mask=rt.RT_RAY_T)", "rt.occluded_rays(o, d)", "rt.last_rays_ms()",
                                  "rt.trace_rays(o[:0], d[:0], mask=rt.RT_RAY_T)"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99(_RAYS + call + "\n")


def test_wrong_shapes_are_value_errors(rt):
    o, d = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    for args in ((o[:, :2], d), (o, d[:3]), (o.ravel(), d.ravel())):
        with pytest.raises(ValueError):
            rt.trace_rays(*args)
        with pytest.raises(ValueError):
            rt.occluded_rays(*args)
    with pytest.raises(ValueError):
        rt.trace_rays(o, d, t_min=np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        rt.occluded_rays(o, d, t_max=np.zeros((4, 1), np.float32))
    with pytest.raises(ValueError):
        rt.trace_rays(o, d, mask=rt.RT_RAY_T, out={"t": np.zeros(5, np.float32)})
    with pytest.raises(ValueError):
        rt.occluded_rays(o, d, out=np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        rt.centre_rays(rt.camera(), 4, 4, np.zeros((4, 3), np.int32))


@pytest.mark.parametrize("frame", ["random_50x37", "tie_mirror"])
def test_centre_rays_are_the_oracles(rt, O, frame):
    """rt.centre_rays equals orc_get_ray on the lens-less camera bit for bit, every pixel of a 50x37 and a 41x24 frame (both cameras have a lens)."""
    _, _, cam, nx, ny = G.sphere_frame(rt, frame)
    assert (nx, ny) in ((50, 37), (41, 24)) and cam.lens_radius > 0
    ij = np.array([(i, j) for j in range(ny) for i in range(nx)], np.int32)
    org, d = rt.centre_rays(cam, nx, ny, ij)
    ref_org, ref_d, _, _ = R.ray_set(rt, O, "centre:" + frame)
    same(org, ref_org, frame + " origins")
    same(d, ref_d, frame + " directions")


# ---- the ray sets: conditions, from the reference alone ----------------------------------------------------------------------

def _hit(ref):
    return ref["prim"] != R.PRIM_NONE


def _changed(a, b):
    """Rays whose result differs in any plane or in occluded."""
    ch = np.zeros(len(a["t"]), bool)
    for k in a:
        d = bits(a[k]) != bits(b[k]) if a[k].dtype != np.uint8 else a[k] != b[k]
        ch |= d.reshape(len(ch), -1).any(axis=1)
    return ch


@pytest.mark.parametrize("name", R.RANDOM_SETS)
def test_random_sets_meet_their_conditions(rt, O, name):
    """At least 15 % hits and 15 % misses; at least 20 rays whose own bounds change the result against the default bounds; 30 % (+-5) of the rays have bounds
    of their own; directions are scaled over four decades.  Figures (hit share, changed by own bounds):
    sph_random:three_spheres 0.582, 124; sph_random:random_50x37 0.560, 126; mesh_random:tris300 0.225, 97; mesh_random:tris300_floor 0.460, 136;
    mesh_random:staircase_a 0.470, 122."""
    org, d, t_min, t_max = R.ray_set(rt, O, name)
    n = len(org)
    assert n == (600 if name.endswith("staircase_a") else 1000) and d.shape == org.shape == (n, 3) and t_min.shape == t_max.shape == (n,)
    ref, dflt = R.reference(rt, O, name), R.reference(rt, O, name, own=False)
    share = float(_hit(ref).mean())
    changed = int(_changed(ref, dflt).sum())
    own = t_max < FLT_MAX
    print(name, "hit share", round(share, 3), "changed by own bounds", changed, "own", int(own.sum()))
    assert 0.15 <= share <= 0.85
    assert changed >= 20
    assert 0.25 <= own.mean() <= 0.35
    assert np.all((t_min[own] >= 0.001) & (t_min[own] <= 2.0) & (t_max[own] >= t_min[own] + np.float32(0.0999)) & (t_max[own] <= 30.0))
    assert np.all(t_min[~own] == np.float32(R.default_t_min(R.frame_of(name))))
    length = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
    assert length.min() < 0.02 and length.max() > 50.0


@pytest.mark.parametrize("name", ["sph_random:three_spheres", "sph_random:random_50x37"])
def test_sphere_sets_start_inside_spheres(rt, O, name):
    """At least 100 origins strictly inside a sphere; at least 20 rays start inside a sphere and hit that same sphere.
    Figures (inside, hit their own sphere): three_spheres 420, 333; random_50x37 164, 116."""
    org, d, _, _ = R.ray_set(rt, O, name)
    sp = G.sphere_frame(rt, R.frame_of(name))[0]
    dist = np.sqrt(((org[:, None, :].astype(np.float64) - sp["center"][None].astype(np.float64)) ** 2).sum(axis=2))
    inside = dist < sp["radius"][None] * 0.999
    ref = R.reference(rt, O, name)
    own = np.array([ref["prim"][r] >= 0 and inside[r, ref["prim"][r]] for r in range(len(org))])
    print(name, "inside a sphere", int(inside.any(axis=1).sum()), "hit their own sphere", int(own.sum()))
    assert inside.any(axis=1).sum() >= 100
    assert own.sum() >= 20


def test_axis_set_meets_coincident_spheres(rt, O):
    """48 rays with one or two direction components exactly 0; at least 4 where two spheres give the same finite t (each tested on its own) and the reference
    reports the lower index; some pass through a sphere's centre.  Figures: 16 rays tie on the pair (1, 2), all reported as 1; 22 have two zero components, 16 pass through a centre, 38 hit."""
    name = "sph_axis:tie_mirror"
    lib = O.load_oracle()
    org, d, t_min, t_max = R.ray_set(rt, O, name)
    assert len(org) == 48 and t_min is None and t_max is None
    zeros = (d == 0).sum(axis=1)
    assert np.all((zeros == 1) | (zeros == 2)) and (zeros == 2).sum() >= 8 and (zeros == 1).sum() >= 8
    sp = np.ascontiguousarray(G.sphere_frame(rt, "tie_mirror")[0], dtype=rt.sphere_dtype)
    ref = R.reference(rt, O, name)
    ties = 0
    for r in range(48):
        o, dd = (C.c_float * 3)(*org[r]), (C.c_float * 3)(*d[r])
        t = [lib.orc_sphere_hit(C.cast(sp.ctypes.data + 16 * k, C.POINTER(rt.sphere)), o, dd, C.c_float(0.001), C.c_float(FLT_MAX)) for k in range(len(sp))]
        best = min(t)
        if best < FLT_MAX and t.count(best) >= 2 and float(ref["t"][r]) == best:
            assert ref["prim"][r] == t.index(best)
            ties += 1
    centre = 0
    for r in range(16, 32):                                     # the axis rays: the line passes through a centre exactly
        c = sp["center"][1:]
        axis = int(np.flatnonzero(d[r])[0])
        other = [a for a in range(3) if a != axis]
        centre += bool(np.any(np.all(c[:, other] == org[r][other], axis=1)))
    print("sph_axis: ties", ties, "two zero components", int((zeros == 2).sum()), "through a centre", centre, "hits", int(_hit(ref).sum()))
    assert ties >= 4 and centre >= 8 and _hit(ref).sum() >= 24


@pytest.mark.parametrize("name", ["mesh_random:tris300", "mesh_random:tris300_floor", "mesh_random:staircase_a"])
def test_mesh_sets_meet_their_conditions(rt, O, name):
    """At least 50 rays miss the bounds (nodes == 0) and at least 50 miss inside them (nodes > 0); at least 100 start outside and point away; at least 3
    material kinds are hit; tris300_floor has at least 30 floor hits; every component of every unit direction is at least 1e-3 in magnitude; tris300 and
    tris300_floor share their rays.  Figures (bounds misses, inside misses, floor hits, kinds): tris300 300, 475, 0, 4; tris300_floor 258, 282, 235, 4;
    staircase_a 203, 115, 0, 8."""
    org, d, _, _ = R.ray_set(rt, O, name)
    ref = R.reference(rt, O, name)
    miss = ~_hit(ref)
    bounds_miss, inside_miss = int((miss & (ref["nodes"] == 0)).sum()), int((miss & (ref["nodes"] > 0)).sum())
    floor = int((ref["prim"] == R.PRIM_FLOOR).sum())
    kinds = R.material_kinds(rt, O, name, ref["prim"])
    f = G.mesh_frame(rt, O, R.frame_of(name))
    b = f["hm"].view.bounds
    lo, hi = np.array([b.min.e[a] for a in range(3)]), np.array([b.max.e[a] for a in range(3)])
    outside = np.any((org < lo) | (org > hi), axis=1)
    away = outside & (((org - (lo + hi) / 2) * d).sum(axis=1) > 0) & (ref["nodes"] == 0)
    print(name, "bounds misses", bounds_miss, "inside misses", inside_miss, "floor", floor, "kinds", len(kinds), "outside and away", int(away.sum()))
    assert bounds_miss >= 50 and inside_miss >= 50
    assert away.sum() >= 100
    assert len(kinds) >= 3
    d64 = d.astype(np.float64)
    assert np.abs(d64 / np.sqrt((d64 * d64).sum(axis=1, keepdims=True))).min() >= 1e-3
    if name.endswith("tris300_floor"):
        assert floor >= 30
        other = R.ray_set(rt, O, "mesh_random:tris300")
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(R.ray_set(rt, O, name), other))
    else:
        assert floor == 0


# ---- the edge sets: exactly-zero direction components, origins on a surface, t_max = +inf ------------------------------------------------

def _zero_bits(d):
    w = bits(d)
    return w == 0, w == 0x80000000


@pytest.mark.parametrize("frame", ["tris300", "staircase_a"])
def test_mesh_axis_sets_meet_their_conditions(rt, O, frame):
    """600 rays, six kinds of 100; every ray has a direction component whose bits are 0 or 0x80000000, at least 250 rays of each sign, kinds 0 and 1 two of
    them; kinds 4 and 5 have org[a] bit-equal to the named plane of the named node (kind 5: node 1, the scene bounds; kind 4 on staircase_a: a box flat on a)
    and every kind-5 ray whose other two slabs overlap visits nodes.  tris300: at least 40 hits and 150 rays that pass the bounds and hit nothing;
    staircase_a: at least 200 hits, 50 misses and 60 hits among kind 4.
    Figures (hits, nodes > 0 without a hit, hits among kind 4, kind-5 rays past the bounds): tris300 74, 353, 14, 86; staircase_a 338, 76, 78, 81."""
    name = "mesh_axis:" + frame
    lib = O.load_oracle()
    org, d, t_min, t_max, info = R.mesh_axis_build(rt, O, frame)
    assert all(a is b for a, b in zip(R.ray_set(rt, O, name), (org, d, t_min, t_max)))
    assert len(org) == 600 and np.array_equal(info["kind"], np.arange(600) // 100)
    pos, neg = _zero_bits(d)
    assert np.all((pos | neg).any(axis=1))
    assert pos.any(axis=1).sum() >= 250 and neg.any(axis=1).sum() >= 250
    even = info["kind"] % 2 == 0
    assert not neg[even].any() and not pos[~even].any()
    zeros = (pos | neg).sum(axis=1)
    assert np.all(zeros[info["kind"] < 2] == 2) and np.all(zeros[info["kind"] >= 2] == 1)
    rows = np.arange(600)
    assert np.all((pos | neg)[rows, info["axis"]] == (info["kind"] >= 2)) and np.all(d[rows, info["axis"]][info["kind"] < 2] != 0)
    own = t_max < FLT_MAX
    assert 0.25 <= own.mean() <= 0.35
    hm = G.mesh_frame(rt, O, frame)["hm"]                       # (held: the node array is a view of the mesh's memory)
    nodes = hm.bvh
    ref = R.reference(rt, O, name)
    past = 0
    for r in np.flatnonzero(info["kind"] >= 4):
        a, node, side = int(info["axis"][r]), int(info["node"][r]), int(info["side"][r])
        plane = (nodes["a"] if side == 0 else nodes["b"])[node][a]
        assert bits(org[r, a:a + 1])[0] == bits(np.array([plane], np.float32))[0], r
        if info["kind"][r] == 5:
            assert node == 1
            lo, hi = nodes["a"][1].copy(), nodes["b"][1].copy()
            lo[a], hi[a] = org[r, a] - np.float32(1.0), org[r, a] + np.float32(1.0)         # axis a no longer constrains: the other two slabs alone
            if lib.orc_hit_bbox((C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_float * 3)(*org[r]), (C.c_float * 3)(*d[r]), C.c_float(t_max[r])):
                past += 1
                assert ref["nodes"][r] > 0, r
        elif frame == "staircase_a":
            assert nodes["a"][node][a] == nodes["b"][node][a]
        else:
            assert 1 <= node <= 64
    hit = _hit(ref)
    inside_miss = int((~hit & (ref["nodes"] > 0)).sum())
    kind4 = int(hit[info["kind"] == 4].sum())
    print(name, "hits", int(hit.sum()), "nodes > 0 without a hit", inside_miss, "hits among kind 4", kind4, "kind-5 rays past the bounds", past)
    assert past >= 50
    if frame == "tris300":
        assert hit.sum() >= 40 and inside_miss >= 150
    else:
        assert hit.sum() >= 200 and (~hit).sum() >= 50 and kind4 >= 60


@pytest.mark.parametrize("name", ["mesh_surface:staircase_a", "mesh_surface:tris300", "sph_surface:random_50x37"])
def test_surface_sets_start_on_a_surface(rt, O, name):
    """The origins are the float32 hit points of the random set's NULL-bounds reference; t_min cycles through 0, 1e-42 (a denormal), 1e-6 and the scene
    kind's default, t_max is FLT_MAX.  With t_min = 0 for every ray and with the default for every ray the reference differs in at least 4 rays, and at least 3
    rays with t_min in {0, 1e-42} hit the primitive they start on again below the default t_min: a device that started such rays at its own epsilon would
    differ.  Figures (rays, differ between t_min 0 and the default, re-hits below the default among t_min in {0, 1e-42}):
    mesh_surface:staircase_a 396, 13, 5; mesh_surface:tris300 283, 141, 71; sph_surface:random_50x37 600 (the first 600 of 675 hit points), 214, 107."""
    org, d, t_min, t_max, prim = R.surface_build(rt, O, name)
    frame = R.frame_of(name)
    dflt = np.float32(R.default_t_min(frame))
    n = len(org)
    assert n <= 600
    if name == "mesh_surface:staircase_a":
        assert n == 396
    src = R.reference(rt, O, ("mesh_random:" if R.is_mesh(frame) else "sph_random:") + frame, own=False)
    assert n == min(600, int((src["prim"] >= 0).sum())) >= 200 and np.all(prim >= 0)
    cycle = np.array([0.0, 1e-42, 1e-6, dflt], np.float32)
    assert 0 < cycle[1] < np.finfo(np.float32).tiny and np.array_equal(bits(t_min), bits(cycle[np.arange(n) % 4])) and np.all(t_max == np.float32(FLT_MAX))
    d64 = d.astype(np.float64)
    assert np.abs(d64 / np.sqrt((d64 * d64).sum(axis=1, keepdims=True))).min() >= 1e-3
    at0, at_default = R.reference(rt, O, name, own=False, t_min=0.0), R.reference(rt, O, name, own=False)
    differ = int(_changed(at0, at_default).sum())
    ref = R.reference(rt, O, name)
    early = (t_min < np.float32(1e-30)) & (ref["prim"] == prim) & (ref["t"] < dflt)
    print(name, "rays", n, "differ between t_min 0 and the default", differ, "re-hits below the default", int(early.sum()))
    assert differ >= 4
    assert early.sum() >= 3


@pytest.mark.parametrize("frame", ["cloud_hybrid", "cloud_global"])
def test_cloud_axis_sets_meet_their_conditions(rt, O, frame):
    """48 rays: 32 with two zero components (16 of them through a sphere's centre), 16 with one; half of the zeros are -0.0; at least 10 hits and 10 misses.
    Figures (hits, misses): cloud_hybrid 33, 15; cloud_global 34, 14."""
    name = "sph_axis:" + frame
    org, d, t_min, t_max = R.ray_set(rt, O, name)
    assert len(org) == 48 and t_min is None and t_max is None
    pos, neg = _zero_bits(d)
    zeros = (pos | neg).sum(axis=1)
    assert np.all(zeros[:32] == 2) and np.all(zeros[32:] == 1)
    assert pos.sum() == neg.sum() == 40
    sp = G.sphere_frame(rt, frame)[0]
    for r in range(16):
        axis = int(np.flatnonzero(d[r])[0])
        other = [a for a in range(3) if a != axis]
        assert np.any(np.all(sp["center"][:, other] == org[r][other], axis=1)), r
    hit = _hit(R.reference(rt, O, name))
    print(name, "hits", int(hit.sum()), "misses", int((~hit).sum()))
    assert hit.sum() >= 10 and (~hit).sum() >= 10


@pytest.mark.parametrize("name", ["mesh_inf:tris300", "sph_inf:three_spheres"])
def test_inf_sets_are_the_flt_max_sets(rt, O, name):
    """Every third ray of the random set carries t_max = +inf and every third FLT_MAX; among the +inf rays at least 30 hits and 30 misses; the reference on
    +inf equals the reference with those entries set to FLT_MAX.  Figures (+inf rays, hits, misses): mesh_inf:tris300 334, 83, 251; sph_inf:three_spheres
    334, 223, 111."""
    org, d, t_min, t_max = R.ray_set(rt, O, name)
    src = R.ray_set(rt, O, name.replace("_inf:", "_random:"))
    k = np.arange(len(org))
    inf = k % 3 == 0
    assert np.all(np.isposinf(t_max[inf])) and np.all(t_max[k % 3 == 1] == np.float32(FLT_MAX)) and np.array_equal(bits(t_max[k % 3 == 2]), bits(src[3][k % 3 == 2]))
    assert org is src[0] and d is src[1] and t_min is src[2]
    ref = R.reference(rt, O, name)
    hit = _hit(ref)
    print(name, "+inf rays", int(inf.sum()), "hits", int(hit[inf].sum()), "misses", int((~hit[inf]).sum()))
    assert hit[inf].sum() >= 30 and (~hit[inf]).sum() >= 30
    finite = np.where(inf, np.float32(FLT_MAX), t_max)
    frame = R.frame_of(name)
    if R.is_mesh(frame):
        f = G.mesh_frame(rt, O, frame)
        want = R.mesh_rays(rt, O, f["hm"], f["mats"], f["tex"], f["floor"], org, d, t_min, finite, clamp=False)
    else:
        want = R.sphere_rays(rt, O, G.sphere_frame(rt, frame)[0], org, d, t_min, finite, clamp=False)
    assert sorted(want) == sorted(ref)
    for key in ref:
        same(ref[key], want[key], f"{name}: {key}, +inf against FLT_MAX")


def test_why_t_max_is_clamped(rt, O):
    """The record of why "a tmax above FLT_MAX is taken as FLT_MAX" is in the contract: the oracle's calls on the raw +inf turn a miss into a hit.  A miss
    returns FLT_MAX, and FLT_MAX < inf accepts it: on three_spheres every +inf ray that misses everything comes back as prim 0, t = FLT_MAX, occluded 1 (the
    first three of them are pinned below); on tris300 a box the ray missed (leftHit = FLT_MAX < closest = inf) is walked into, so +inf rays that miss inside
    the bounds visit more nodes, and every +inf ray that passes the bounds without a hit is reported as prim >= 0 and occluded."""
    name = "sph_inf:three_spheres"
    org, d, t_min, t_max = R.ray_set(rt, O, name)
    ref = R.reference(rt, O, name)
    raw = R.sphere_rays(rt, O, G.sphere_frame(rt, "three_spheres")[0], org, d, t_min, t_max, clamp=False)
    inf = np.isinf(t_max)
    miss = inf & ~_hit(ref)
    assert miss.sum() >= 30
    assert np.all(raw["prim"][miss] == 0) and np.all(raw["t"][miss] == np.float32(FLT_MAX)) and np.all(raw["occluded"][miss] == 1)
    assert not ref["occluded"][miss].any() and np.all(ref["t"][miss] == np.float32(FLT_MAX))
    three = np.flatnonzero(miss)[:3]
    print("three_spheres, the first three +inf rays that miss:", three.tolist(), "raw prim", raw["prim"][three].tolist(), "occluded", raw["occluded"][three].tolist())
    assert three.tolist() == THREE_MISSES
    assert not _changed({k: v[~miss] for k, v in raw.items()}, {k: v[~miss] for k, v in ref.items()}).any()      # nothing else differs
    name = "mesh_inf:tris300"
    f = G.mesh_frame(rt, O, "tris300")
    org, d, t_min, t_max = R.ray_set(rt, O, name)
    ref = R.reference(rt, O, name)
    raw = R.mesh_rays(rt, O, f["hm"], f["mats"], f["tex"], f["floor"], org, d, t_min, t_max, clamp=False)
    inf = np.isinf(t_max)
    miss = inf & ~_hit(ref) & (ref["nodes"] > 0)
    assert miss.sum() >= 30
    assert np.all(raw["prim"][miss] >= 0) and np.all(raw["occluded"][miss] == 1)
    more = int((raw["nodes"][miss] > ref["nodes"][miss]).sum())
    print("tris300: +inf rays that miss inside the bounds", int(miss.sum()), "of which the raw calls visit more nodes on", more)
    assert np.all(raw["nodes"][miss] >= ref["nodes"][miss]) and more >= 10


THREE_MISSES = [36, 123, 162]


# ---- the reference against itself and against the guide reference ---------------------------------------------------------------

@pytest.mark.parametrize("frame", R.CENTRE_FRAMES)
def test_centre_reference_is_the_guide_reference(rt, O, frame):
    """On the centre rays t, prim, normal and nodes are guides_reference's depth, prim, normal and nodes (two normalisations there, one of a unit vector's
    bits here: the same direction); uv is zero off the triangles."""
    name = "centre:" + frame
    ref, g = R.reference(rt, O, name), G.reference(rt, O, frame)
    same(ref["t"], g["depth"].reshape(-1), frame + " t")
    same(ref["prim"], g["prim"].reshape(-1), frame + " prim")
    same(ref["normal"], g["normal"].reshape(-1, 3), frame + " normal")
    if R.is_mesh(frame):
        same(ref["nodes"], g["nodes"].reshape(-1), frame + " nodes")
        assert np.any(ref["uv"][ref["prim"] >= 0] != 0)
    assert np.all(ref["uv"][ref["prim"] < 0] == 0)


@pytest.mark.parametrize("name", [s for s in R.SETS if not s.endswith("_floor")])
def test_occluded_is_a_hit_without_a_floor(rt, O, name):
    """Without a floor occluded equals t < FLT_MAX: the any-hit and the closest-hit query visit the same nodes until the first hit."""
    for own in (True, False):
        ref = R.reference(rt, O, name, own=own)
        assert np.array_equal(ref["occluded"], (ref["t"] < FLT_MAX).astype(np.uint8)), (name, own)


def test_floor_never_occludes(rt, O):
    ref, plain = R.reference(rt, O, "mesh_random:tris300_floor"), R.reference(rt, O, "mesh_random:tris300")
    assert np.array_equal(ref["occluded"], plain["occluded"])
    floor = ref["prim"] == R.PRIM_FLOOR
    assert floor.sum() >= 30 and not ref["occluded"][floor].any()
    assert np.array_equal(bits(ref["t"][~floor]), bits(plain["t"][~floor]))


@pytest.mark.parametrize("name", ["sph_random:three_spheres", "sph_axis:tie_mirror"])
def test_sphere_occluded_shortcut_is_the_definition(rt, O, name):
    """sphere_rays takes occluded from its closest-hit scan; the definition - every sphere against the ray's own t_max - gives the same bytes."""
    org, d, _, _ = R.ray_set(rt, O, name)
    t_min, t_max = R.bounds_of(rt, O, name)
    sp = G.sphere_frame(rt, R.frame_of(name))[0]
    assert np.array_equal(R.sphere_occluded_by_definition(rt, O, sp, org, d, t_min, t_max), R.reference(rt, O, name)["occluded"])
