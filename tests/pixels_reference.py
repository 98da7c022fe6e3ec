"""The reference of renderPixels (include/rt_api.h), from the CPU oracle alone.  No test: a plain module, imported by tests/test_pixels_api.py and
tests/test_gpu_pixels.py.  A pixel (i, j) at a sample count is O.render(..., region=(i, j, i + 1, j + 1), counters=True): its colour and its `rays`.

Scenes (tag: scene, size, max depth, options):
  S1        scene_three_spheres, 40x24, 50, sphere defaults
  S2        scene_random_spheres, 64x48, 50, sphere defaults
  M1        scene_staircase_procedural(1), HostMesh.build(nppl=5), staircase_camera, 48x32, 8, mesh defaults (NEE + RR on)
  M1_floor  M1 with rt_render_options.floor = 1 and a floor plane below the room
  M1_tex    M1 with one textured material (the stairs' and the floor's, as tests/test_gpu_parity_mesh.py textures them)
  M2_floor  the tris300_floor frame of tests/guides_reference.py, 48x40, 8, floor = 1: the staircase is a closed room - no ray of M1_floor ever reaches
            its plane -, here the plane changes 98 % of the pixels (tests/test_pixels_api.py), and the sky and a wrapped texture are hit too
The standard list of a scene, from a fixed seed: every pixel once in a shuffled order, plus 37 duplicates drawn from it - its length is no multiple of 64
and it holds both corners."""
import functools

import numpy as np

SCENES = {"S1": (40, 24, 50), "S2": (64, 48, 50), "M1": (48, 32, 8), "M1_floor": (48, 32, 8), "M1_tex": (48, 32, 8), "M2_floor": (48, 40, 8)}
DUPLICATES = 37
LIST_SEED = {"S1": 101, "S2": 102, "M1": 103, "M1_floor": 104, "M1_tex": 105, "M2_floor": 106}


def is_mesh(tag):
    return tag.startswith("M")


@functools.lru_cache(maxsize=None)
def scene(rt, tag):
    """What init and the oracle need: a dict with nx, ny, depth, cam and (spheres: sp, mt | mesh: hm, mats, tex, floor)."""
    nx, ny, depth = SCENES[tag]
    if tag == "S1":
        sp, mt, cam = rt.scene_three_spheres(nx, ny)
        return dict(nx=nx, ny=ny, depth=depth, cam=cam, sp=sp, mt=mt)
    if tag == "S2":
        sp, mt, cam = rt.scene_random_spheres(nx, ny)
        return dict(nx=nx, ny=ny, depth=depth, cam=cam, sp=sp, mt=mt)
    if tag == "M2_floor":
        import guides_reference as G
        f = G.mesh_frame(rt, None, "tris300_floor")
        assert (f["nx"], f["ny"]) == (nx, ny)
        return dict(nx=nx, ny=ny, depth=depth, cam=f["cam"], hm=f["hm"], mats=f["mats"], tex=f["tex"], floor=f["floor"])
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    tex, floor = [], None
    if tag == "M1_tex":
        mats = mats.copy()
        tex = [np.random.default_rng(5).uniform(0, 1, (16, 24, 3)).astype(np.float32)]
        mats["texId"][17] = 0       # floor
        mats["texId"][19] = 0       # stairs
    if tag == "M1_floor":
        lo = np.array(hm.view.bounds.min.e[:])
        floor = (0.0, 1.0, 0.0, 0.0, float(lo[1]) - 10.0, 0.0)
    return dict(nx=nx, ny=ny, depth=depth, cam=rt.staircase_camera(nx, ny), hm=hm, mats=mats, tex=tex, floor=floor)


def options(tag):
    """The setRenderOptions fields the tag's frame differs in from the scene kind's defaults."""
    return {"floor": 1} if tag.endswith("_floor") else {}


def init(rt, tag, **opts):
    """init* of the tag's scene with its options (and `opts` over them); returns the framebuffer view."""
    s = scene(rt, tag)
    if is_mesh(tag):
        ks, keep = rt.make_kernel_scene(s["hm"], s["mats"], s["tex"], floor=s["floor"])
        fb = rt.initRenderer(ks, s["cam"], s["nx"], s["ny"], s["depth"], keepalive=keep)
    else:
        fb = rt.initRendererSpheres(s["sp"], s["mt"], s["cam"], s["nx"], s["ny"], s["depth"])
    o = rt.getDefaultRenderOptions(not is_mesh(tag))
    rt.setRenderOptions(o, **dict(options(tag), **opts))
    return fb


def _oracle_args(rt, O, tag):
    s = scene(rt, tag)
    opt = O.default_options(not is_mesh(tag))
    for k, v in options(tag).items():
        setattr(opt, k, v)
    sc = O.mesh_scene(s["hm"], s["mats"], s["tex"], s["floor"]) if is_mesh(tag) else O.sphere_scene(s["sp"], s["mt"])
    return sc, s["cam"], opt, s["nx"], s["ny"], s["depth"]


@functools.lru_cache(maxsize=None)
def oracle_frame(rt, O, tag, ns):
    """The oracle's whole frame at ns samples per pixel and its counters."""
    sc, cam, opt, nx, ny, depth = _oracle_args(rt, O, tag)
    fb, cnt = O.render(sc, cam, opt, nx, ny, ns, depth, counters=True)
    fb.setflags(write=False)
    return fb, cnt


@functools.lru_cache(maxsize=None)
def oracle_planes(rt, O, tag, ns):
    """Every pixel of the image on its own, one region render each: (colour (ny, nx, 3) float32, rays (ny, nx) uint32).  Computed once, read-only."""
    sc, cam, opt, nx, ny, depth = _oracle_args(rt, O, tag)
    col, rays = np.zeros((ny, nx, 3), np.float32), np.zeros((ny, nx), np.uint32)
    fb = np.zeros((ny, nx, 3), np.float32)
    for j in range(ny):
        for i in range(nx):
            _, cnt = O.render(sc, cam, opt, nx, ny, ns, depth, region=(i, j, i + 1, j + 1), counters=True, fb=fb)
            col[j, i] = fb[j, i]
            rays[j, i] = cnt.rays
    col.setflags(write=False)
    rays.setflags(write=False)
    return col, rays


def oracle_pixels(rt, O, tag, ij, ns):
    """(out (n, 3), rays (n,)) of the list ij at ns samples per pixel: an int, or one count per entry."""
    ij = np.asarray(ij)
    counts = np.full(len(ij), ns, np.int64) if np.isscalar(ns) else np.asarray(ns)
    out, rays = np.zeros((len(ij), 3), np.float32), np.zeros(len(ij), np.uint32)
    for c in np.unique(counts):
        col_c, rays_c = oracle_planes(rt, O, tag, int(c))
        m = counts == c
        out[m] = col_c[ij[m, 1], ij[m, 0]]
        rays[m] = rays_c[ij[m, 1], ij[m, 0]]
    return out, rays


@functools.lru_cache(maxsize=None)
def standard_list(tag):
    """(ij (n, 2) int32, first (n,) bool): the standard list and which entries are a pixel's first occurrence (the non-duplicates)."""
    nx, ny, _ = SCENES[tag]
    rng = np.random.default_rng(LIST_SEED[tag])
    every = np.array([(i, j) for j in range(ny) for i in range(nx)], np.int32)[rng.permutation(nx * ny)]
    dup_at = rng.integers(0, nx * ny, DUPLICATES)
    ij = np.concatenate([every, every[dup_at]])
    # the duplicates are spread through the list, not appended: a duplicate must not only ever meet a queue that is nearly empty
    where = rng.permutation(len(ij))
    ij = np.ascontiguousarray(ij[where])
    first = np.zeros(len(ij), bool)
    first[np.unique(ij[:, 1] * nx + ij[:, 0], return_index=True)[1]] = True
    ij.setflags(write=False)
    first.setflags(write=False)
    return ij, first
