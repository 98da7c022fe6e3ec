"""The test reference of renderGuides (include/rt_api.h) and the frames the guide tests render.  No test: read by tests/test_guides_api.py (CPU: the
coverage conditions of every frame) and tests/test_gpu_guides.py (GPU: every plane of every frame, bit for bit).

The reference is built from the CPU oracle's own functions through ctypes and from nothing of the code under test: orc_get_ray on a copy of the camera
with lens_radius = 0 (the centre ray), orc_sphere_hit against the running closest t in the caller's order (hit_spheres of oracle/rt_oracle.c),
orc_hit_bbox + orc_hit_bvh with orc_counters.node_visits, orc_plane_hit; the diffuse / checker / coat / floor albedos are the throughput
orc_material_scatter_p returns for a diffuse bounce.  Hit point, normal and sky are restated in fp32 in the operation order of hit() / color() in
oracle/rt_oracle.c: numpy float32 scalars, every product and sum written out (no np.dot, nothing fused).  hit() builds its ray with mkray, which
normalises the path's (already unit) direction once more: the intersection tests, the hit point and the orientation of the normal use that direction,
the sky uses the path's."""
import ctypes as C
import functools

import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
PRIM_NONE, PRIM_FLOOR = -1, -2
PLANES = ("albedo", "normal", "depth", "prim", "nodes")


def _unit(v):
    s = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    l = np.sqrt(s)
    return [v[0] / l, v[1] / l, v[2] / l]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]]


def _f3(a):
    return [F(a[0]), F(a[1]), F(a[2])]


def _sky(sky_gradient, d):
    if not sky_gradient:
        return [F(0.5), F(0.5), F(0.5)]
    t = F(0.5) * (d[1] + F(1.0))
    w = F(1.0) - t
    return [w * F(1.0) + t * F(0.5), w * F(1.0) + t * F(0.7), w * F(1.0) + t * F(1.0)]


def _centre_ray(lib, rt, cam0, i, j, nx, ny):
    u = (F(i) + F(0.5)) / F(nx)
    v = (F(j) + F(0.5)) / F(ny)
    st = C.c_uint32(12345)
    org = (C.c_float * 3)()
    d = (C.c_float * 3)()
    lib.orc_get_ray(C.byref(cam0), C.c_float(u), C.c_float(v), C.byref(st), org, d)
    return org, d


def _camera_without_lens(rt, cam):
    cam0 = rt.camera()
    C.memmove(C.byref(cam0), C.byref(cam), C.sizeof(cam))
    cam0.lens_radius = 0.0
    return cam0


def _empty(nx, ny, mesh):
    out = {"albedo": np.zeros((ny, nx, 3), np.float32), "normal": np.zeros((ny, nx, 3), np.float32),
           "depth": np.full((ny, nx), FLT_MAX, np.float32), "prim": np.full((ny, nx), PRIM_NONE, np.int32)}
    if mesh:
        out["nodes"] = np.zeros((ny, nx), np.int32)
    return out


def sphere_guides(rt, O, spheres, materials, cam, nx, ny, t_min=0.001, sky=1):
    """The four planes of a sphere scene."""
    lib = O.load_oracle()
    spheres = np.ascontiguousarray(spheres, dtype=rt.sphere_dtype)
    cam0 = _camera_without_lens(rt, cam)
    sp_ptr = [C.cast(spheres.ctypes.data + 16 * k, C.POINTER(rt.sphere)) for k in range(len(spheres))]
    out = _empty(nx, ny, False)
    hit = lib.orc_sphere_hit
    tmin = C.c_float(t_min)
    for j in range(ny):
        for i in range(nx):
            org, d = _centre_ray(lib, rt, cam0, i, j, nx, ny)
            assert [org[a] for a in range(3)] == [cam.origin.e[a] for a in range(3)]
            closest, sid = FLT_MAX, -1
            for k, sp in enumerate(sp_ptr):                     # hit_spheres: strict <, the lower index keeps an equal t
                t = hit(sp, org, d, tmin, closest)
                if t < closest:
                    closest, sid = t, k
            if sid < 0:
                out["albedo"][j, i] = _sky(sky == rt.RT_SKY_GRADIENT, _f3(d))
                continue
            o, dn = _f3(org), _unit(_f3(d))                     # mkray: the ray's direction
            t = F(closest)
            p = [o[a] + t * dn[a] for a in range(3)]
            c, r = _f3(spheres["center"][sid]), F(spheres["radius"][sid])
            n = [(p[a] - c[a]) / r for a in range(3)]
            if _dot(dn, n) > F(0.0):
                n = [-x for x in n]
            out["albedo"][j, i] = materials["color"][sid]
            out["normal"][j, i] = n
            out["depth"][j, i] = t
            out["prim"][j, i] = sid
    return out


def _diffuse_throughput(lib, rt, O, mtype, p, n, wo):
    """The albedo of a preset with a diffuse lobe: the throughput of a bounce that took it (the coats choose their layer with one random draw)."""
    mat = rt.material()
    mat.type = int(mtype)
    mat.texId = -1
    col = (C.c_float * 3)(0.25, 0.5, 0.75)
    for seed in range(1, 200):
        st = C.c_uint32(seed * 2654435761 & 0xFFFFFFFF | 1)
        sc = O.orc_scatter()
        lib.orc_material_scatter_p(C.c_float(1.0), (C.c_float * 3)(*p), (C.c_float * 3)(*n), 0, (C.c_float * 3)(*wo), C.byref(mat), col, C.byref(st), C.byref(sc))
        if not sc.specular:
            return [F(sc.throughput[a]) for a in range(3)]
    raise AssertionError("no diffuse bounce in 200 draws")


def mesh_guides(rt, O, hm, materials, textures, cam, nx, ny, t_min=0.01, sky=0, floor=None):
    """The five planes of a mesh scene; floor = (norm xyz, point xyz) with rt_render_options.floor = 1, None without."""
    lib = O.load_oracle()
    scene = O.mesh_scene(hm, materials, textures, floor)
    cam0 = _camera_without_lens(rt, cam)
    tris = hm.tris
    bmin = (C.c_float * 3)(*[hm.view.bounds.min.e[a] for a in range(3)])
    bmax = (C.c_float * 3)(*[hm.view.bounds.max.e[a] for a in range(3)])
    plane = rt.plane()
    if floor is not None:
        for a in range(3):
            plane.norm.e[a] = float(floor[a]); plane.point.e[a] = float(floor[3 + a])
    basic = (rt.RT_DIFFUSE, rt.RT_METAL, rt.RT_GLASS)
    lobe = (rt.RT_FLOOR_COAT, rt.RT_FLOOR_DIFFUSE, rt.RT_FLOOR_CHECKER, rt.RT_MODEL_COAT, rt.RT_MODEL_DIFFUSE)
    out = _empty(nx, ny, True)
    tmin = C.c_float(t_min)
    for j in range(ny):
        for i in range(nx):
            org, d = _centre_ray(lib, rt, cam0, i, j, nx, ny)
            o, dn = _f3(org), _unit(_f3(d))
            t, prim, n, albedo = FLT_MAX, PRIM_NONE, None, None
            if lib.orc_hit_bbox(bmin, bmax, org, d, C.c_float(FLT_MAX)):       # hit_mesh: the scene bounds first
                cnt = O.orc_counters()
                tri_id, hu, hv = C.c_uint32(0), C.c_float(0), C.c_float(0)
                t = lib.orc_hit_bvh(C.byref(scene), org, d, tmin, C.c_float(FLT_MAX), 0, C.byref(tri_id), C.byref(hu), C.byref(hv), C.byref(cnt))
                out["nodes"][j, i] = cnt.node_visits
            if t < FLT_MAX:
                prim = tri_id.value
                tri = tris[prim]
                v0, v1, v2 = _f3(tri["v"][0]), _f3(tri["v"][1]), _f3(tri["v"][2])
                n = _unit(_cross([v1[a] - v0[a] for a in range(3)], [v2[a] - v0[a] for a in range(3)]))
                p = [o[a] + F(t) * dn[a] for a in range(3)]
                mat = materials[int(tri["meshID"])]
                if mat["type"] in basic:
                    if mat["texId"] != -1:
                        tc, u, v = [F(x) for x in tri["texCoords"]], F(hu.value), F(hv.value)
                        w0 = F(1.0) - u - v
                        tu = u * tc[2] + v * tc[4] + w0 * tc[0]
                        tv = u * tc[3] + v * tc[5] + w0 * tc[1]
                        tu = tu - np.floor(tu)
                        tv = tv - np.floor(tv)
                        tex = textures[int(mat["texId"])]
                        height, width = tex.shape[0], tex.shape[1]
                        tx, ty = int(F(width - 1) * tu), int(F(height - 1) * tv)
                        albedo = tex.reshape(-1)[(ty * width + tx) * 3:(ty * width + tx) * 3 + 3]
                    else:
                        albedo = mat["color"]
                elif mat["type"] in lobe:
                    nf = n if not _dot(dn, n) > F(0.0) else [-x for x in n]
                    albedo = _diffuse_throughput(lib, rt, O, mat["type"], p, nf, _f3(d))
                else:
                    albedo = [F(1.0)] * 3
            elif floor is not None:
                t = lib.orc_plane_hit(C.byref(plane), org, d, tmin, C.c_float(FLT_MAX))
                if t < FLT_MAX:
                    prim = PRIM_FLOOR
                    n = _f3(floor[:3])
                    p = [o[a] + F(t) * dn[a] for a in range(3)]
                    nf = n if not _dot(dn, n) > F(0.0) else [-x for x in n]
                    albedo = _diffuse_throughput(lib, rt, O, rt.RT_FLOOR_DIFFUSE, p, nf, _f3(d))      # kernels.cu:481-482
            if prim == PRIM_NONE:
                out["albedo"][j, i] = _sky(sky == rt.RT_SKY_GRADIENT, _f3(d))
                continue
            if _dot(dn, n) > F(0.0):
                n = [-x for x in n]
            out["albedo"][j, i] = albedo
            out["normal"][j, i] = n
            out["depth"][j, i] = F(t)
            out["prim"][j, i] = prim
    return out


# ---------------------------------------------------------------------------------------------
# the frames
# ---------------------------------------------------------------------------------------------

def _cloud(rt, n, nx, ny):
    import kernel_forms as K
    _, sp, mt, cam = K.build_scene(rt, ("cloud", n, "volume", False), nx, ny)
    return sp, mt, cam


def _tie_scene(rt, nx, ny):
    """Five spheres, two of them coincident (indices 1 and 3, different colours): the lower caller index must win every pixel of the pair."""
    sp = np.zeros(5, rt.sphere_dtype)
    mt = np.zeros(5, rt.material_dtype)
    sp["center"] = [(0, -100.5, -1), (0, 0, -1), (1.2, 0, -1.3), (0, 0, -1), (-1.1, 0.1, -0.8)]
    sp["radius"] = [100, 0.5, 0.5, 0.5, 0.4]
    mt["type"] = [rt.RT_DIFFUSE, rt.RT_METAL, rt.RT_GLASS, rt.RT_DIFFUSE, rt.RT_METAL]
    mt["color"] = [(0.8, 0.8, 0.0), (0.1, 0.2, 0.5), (1, 1, 1), (0.9, 0.1, 0.1), (0.8, 0.6, 0.2)]
    mt["param"] = [0, 0.1, 1.5, 0, 0.3]
    mt["texId"] = -1
    cam = rt.make_camera((0.3, 0.6, 2.5), (0, 0, -1), (0, 1, 0), 40.0, nx / ny, 0.1, 3.0)
    return sp, mt, cam


def _tie_mirror_scene(rt, nx, ny):
    """A ground sphere and 12 pairs of equal spheres mirrored in the plane x = 0, the sphere at +x listed BEFORE its mirror image; the camera looks along
    -z from x = 0 and nx is odd, so the centre column's rays have direction x = 0 exactly and meet both spheres of the overlapping pair 0 (indices 1, 2)
    at the same t bit for bit.  The renderer sorts its sphere slots along the axis of largest extent (x, ascending: more than 16 small spheres), so it
    scans index 2 before index 1: only the explicit (t, caller index) rule gives those pixels to index 1, as the reference's scan in caller order does."""
    n = 25
    sp = np.zeros(n, rt.sphere_dtype)
    mt = np.zeros(n, rt.material_dtype)
    sp["center"][0] = (0, -100, 0); sp["radius"][0] = 100
    for k in range(12):
        x, z = 0.2 + 0.5 * k, -0.9 * (k % 4)
        sp["center"][1 + 2 * k] = (x, 0.5, z)
        sp["center"][2 + 2 * k] = (-x, 0.5, z)
    sp["radius"][1:] = 0.5
    rng = np.random.default_rng(5)
    mt["type"] = rng.integers(0, 3, n)
    mt["color"] = rng.uniform(0.1, 1, (n, 3))
    mt["param"] = np.where(mt["type"] == rt.RT_GLASS, 1.5, 0.1)
    mt["texId"] = -1
    cam = rt.make_camera((0, 1, 5), (0, 1, 0), (0, 1, 0), 40.0, nx / ny, 0.1, 5.0)
    return sp, mt, cam


def tie_mirror_pixels(rt, O):
    """Pixels of the tie_mirror frame whose centre ray meets spheres 1 and 2 at the same finite t (each tested on its own), and nothing nearer."""
    lib = O.load_oracle()
    sp, mt, cam, nx, ny = sphere_frame(rt, "tie_mirror")
    sp = np.ascontiguousarray(sp, dtype=rt.sphere_dtype)
    cam0 = _camera_without_lens(rt, cam)
    g = reference(rt, O, "tie_mirror")
    out = []
    for j in range(ny):
        for i in range(nx):
            org, d = _centre_ray(lib, rt, cam0, i, j, nx, ny)
            t = [lib.orc_sphere_hit(C.cast(sp.ctypes.data + 16 * k, C.POINTER(rt.sphere)), org, d, C.c_float(0.001), C.c_float(FLT_MAX)) for k in (1, 2)]
            if t[0] == t[1] and t[0] < FLT_MAX and float(g["depth"][j, i]) == t[0]:
                out.append((i, j))
    return out


def sphere_frame(rt, name):
    """(spheres, materials, camera, nx, ny) of a named sphere frame."""
    if name in ("random_96x64", "random_50x37", "random_48x32"):
        nx, ny = {"random_96x64": (96, 64), "random_50x37": (50, 37), "random_48x32": (48, 32)}[name]
        return rt.scene_random_spheres(nx, ny) + (nx, ny)
    if name == "three_spheres":
        return rt.scene_three_spheres(64, 40) + (64, 40)
    if name == "cloud_hybrid":                                  # past the full LDS copy: test data in the LDS, hit data in global memory
        return _cloud(rt, 2100, 32, 24) + (32, 24)
    if name == "cloud_global":                                  # past the LDS: the scene is read from global memory
        return _cloud(rt, 6000, 32, 24) + (32, 24)
    if name == "tie":
        return _tie_scene(rt, 40, 24) + (40, 24)
    if name == "tie_mirror":
        return _tie_mirror_scene(rt, 41, 24) + (41, 24)
    raise KeyError(name)


SPHERE_FRAMES = ("random_96x64", "random_50x37", "three_spheres", "cloud_hybrid", "cloud_global", "tie", "tie_mirror")


@functools.lru_cache(maxsize=None)
def _staircase(rt):
    tris, mats = rt.scene_staircase_procedural(1)
    return rt.HostMesh.build(tris, 5), mats


STAIR_NX, STAIR_NY = 40, 50
# what the two staircase frames put on the mesh ids the camera sees, most pixels first: "tex0" / "tex1" = a plain type with a texture
STAIR_KINDS = {"staircase_a": ["tex0", "RT_DIFFUSE", "RT_FLOOR_CHECKER", "tex1", "RT_METAL", "RT_FLOOR_COAT", "RT_FLOOR_DIFFUSE", "RT_MODEL_COAT", "RT_GLASS"],
               "staircase_b": ["RT_FLOOR_CHECKER", "RT_MODEL_DIFFUSE", "tex1", "RT_MODEL_GLOSSY", "RT_MODEL_GLASS", "RT_MODEL_TINTEDGLASS", "RT_MODEL_SSS", "RT_DIFFUSE",
                               "tex0"]}


def stair_textures():
    """Seeded random float images of unequal width and height."""
    rng = np.random.default_rng(11)
    return [rng.uniform(0, 1, (16, 24, 3)).astype(np.float32), rng.uniform(0, 1, (31, 9, 3)).astype(np.float32)]


@functools.lru_cache(maxsize=None)
def _stair_visible_ids(rt, O):
    """The mesh ids the staircase camera sees at STAIR_NX x STAIR_NY, most pixels first (from the reference's own primitive plane)."""
    hm, mats = _staircase(rt)
    g = mesh_guides(rt, O, hm, mats, [], rt.staircase_camera(STAIR_NX, STAIR_NY), STAIR_NX, STAIR_NY)
    ids = hm.tris["meshID"][g["prim"][g["prim"] >= 0]]
    vals, counts = np.unique(ids, return_counts=True)
    return tuple(int(v) for v in vals[np.argsort(-counts, kind="stable")])


def mesh_frame(rt, O, name):
    """dict(hm, mats, tex, cam, nx, ny, floor, kinds) of a named mesh frame; kinds: mesh id -> what the frame put on it (staircase frames)."""
    if name in STAIR_KINDS:
        hm, mats = _staircase(rt)
        mats = mats.copy()
        ids = _stair_visible_ids(rt, O)
        kinds = {}
        for mid, kind in zip(ids, STAIR_KINDS[name]):
            kinds[mid] = kind
            if kind.startswith("tex"):
                mats["type"][mid] = rt.RT_DIFFUSE
                mats["texId"][mid] = int(kind[3])
            else:
                mats["type"][mid] = getattr(rt, kind)
                mats["texId"][mid] = -1
                if kind == "RT_GLASS":
                    mats["param"][mid] = 1.5
        return dict(hm=hm, mats=mats, tex=stair_textures(), cam=rt.staircase_camera(STAIR_NX, STAIR_NY), nx=STAIR_NX, ny=STAIR_NY, floor=None, kinds=kinds)
    if name in ("tris300", "tris300_floor"):
        rng = np.random.default_rng(7)
        tris = np.zeros(300, rt.triangle_dtype)
        centre = rng.uniform(-10, 10, (300, 1, 3))
        tris["v"] = (centre + rng.uniform(-1.5, 1.5, (300, 3, 3))).astype(np.float32)
        tris["texCoords"] = rng.uniform(-2, 2, (300, 6)).astype(np.float32)
        tris["meshID"] = rng.integers(0, 4, 300)
        mats = np.zeros(4, rt.material_dtype)
        mats["type"] = [rt.RT_DIFFUSE, rt.RT_METAL, rt.RT_GLASS, rt.RT_DIFFUSE]
        mats["color"] = rng.uniform(0.1, 1, (4, 3))
        mats["param"] = [0, 0.2, 1.5, 0]
        mats["texId"] = [-1, -1, -1, 0]
        nx, ny = 48, 40
        cam = rt.make_camera((30, 18, 42), (0, 0, 0), (0, 1, 0), 40.0, nx / ny, 0.1, 50.0)
        floor = (0, 1, 0, 0, -12, 0) if name == "tris300_floor" else None
        return dict(hm=rt.HostMesh.build(tris, 5), mats=mats, tex=stair_textures()[:1], cam=cam, nx=nx, ny=ny, floor=floor, kinds={})
    raise KeyError(name)


MESH_FRAMES = ("staircase_a", "staircase_b", "tris300", "tris300_floor")


@functools.lru_cache(maxsize=None)
def reference(rt, O, name):
    """The reference planes of a named frame with the default options of its scene kind (and the floor of the *_floor frame)."""
    if name in MESH_FRAMES:
        f = mesh_frame(rt, O, name)
        return mesh_guides(rt, O, f["hm"], f["mats"], f["tex"], f["cam"], f["nx"], f["ny"], floor=f["floor"])
    sp, mt, cam, nx, ny = sphere_frame(rt, name)
    return sphere_guides(rt, O, sp, mt, cam, nx, ny)


def coverage(rt, O, name):
    """The coverage figures the issue's conditions are stated in, from the reference alone."""
    g = reference(rt, O, name)
    prim = g["prim"]
    res = {"hit": float((prim != PRIM_NONE).mean()), "miss": float((prim == PRIM_NONE).mean())}
    if name in MESH_FRAMES:
        f = mesh_frame(rt, O, name)
        res["bounds_miss"] = float(((prim == PRIM_NONE) & (g["nodes"] == 0)).mean())
        res["inside_miss"] = float(((prim == PRIM_NONE) & (g["nodes"] > 0)).mean())
        res["floor"] = float((prim == PRIM_FLOOR).mean())
        res["tri"] = float((prim >= 0).mean())
        ids = f["hm"].tris["meshID"][prim[prim >= 0]]
        res["kinds_seen"] = sorted({f["kinds"][int(m)] for m in np.unique(ids) if int(m) in f["kinds"]})
        res["nodes"] = (int(g["nodes"].min()), int(g["nodes"].max()), float(g["nodes"].mean()))
    else:
        mt = sphere_frame(rt, name)[1]
        res["types"] = sorted({int(t) for t in mt["type"][prim[prim >= 0]]})
        res["distinct"] = int(len(np.unique(prim[prim >= 0])))
    return res
