"""Path-traced mesh frames that hold every material kind of include/rt_types.h, and the CPU oracle's renders of them.  No test: a plain module, read by
tests/test_mesh_materials_api.py (CPU: the frames test what they claim, the loose bound is one the reference keeps) and tests/test_gpu_mesh_materials.py
(GPU: every mesh kernel against the oracle).

Frames (name: scene, size, max depth):
  stair_exact  scene_staircase_procedural(1), 40x50, 16: STAIR_EXACT_KINDS on the nine mesh ids the camera sees, most pixels first
  stair_loose  the staircase_b frame of tests/guides_reference.py, 40x50, 16: adds the checker, tinted-glass and subsurface presets
  soup_exact   400 random triangles, 72x56, 12, a floor plane: 256 materials of the types EXACT_TYPES[k % 9], mesh ids uniform in 0..255, every triangle's
               three padding bytes random and non-zero, texture coordinates in (-2, 2), textures on every 16th material of two residues
  soup_all     the same with type k % 12
The exact frames hold only kinds whose device arithmetic is IEEE fp32 on both sides (types 0,1,2,3,4,6,7,8,9): the device must give the oracle's bits.
The loose frames add the three presets that call sinf / logf / expf, where the device's libm and the host's may differ by an ulp.  A pixel of a loose frame
is UNTOUCHED if the oracle's frame and the oracle's frame of the table with the loose kinds swapped for exact ones (swapped()) are bit-equal there in all
three channels: no sample's colour depended on a libm-based preset, so the device must give the oracle's bits there too."""
import functools

import numpy as np

import guides_reference as G

EXACT_FRAMES = ("stair_exact", "soup_exact")
LOOSE_FRAMES = ("stair_loose", "soup_all")
FRAMES = EXACT_FRAMES + LOOSE_FRAMES
STAIR_EXACT_KINDS = ["tex0", "RT_MODEL_DIFFUSE", "RT_FLOOR_COAT", "tex1:RT_METAL", "RT_MODEL_GLOSSY", "RT_MODEL_COAT", "RT_FLOOR_DIFFUSE", "RT_MODEL_GLASS",
                     "RT_GLASS"]
EXACT_TYPES = [0, 1, 2, 3, 4, 6, 7, 8, 9]
SOUP_FLOOR = (0.0, 1.0, 0.0, 0.0, -3.0, 0.0)
SOUP_SEED = 9
LIST_SEED = {"stair_exact": 201, "stair_loose": 202, "soup_exact": 203, "soup_all": 204}
DUPLICATES = 37


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def is_soup(name):
    return name.startswith("soup")


def loose_types(rt):
    """The three libm-based presets and the exact kind each is swapped for: the same opacity class, no libm call."""
    return {rt.RT_FLOOR_CHECKER: rt.RT_MODEL_DIFFUSE, rt.RT_MODEL_TINTEDGLASS: rt.RT_MODEL_GLASS, rt.RT_MODEL_SSS: rt.RT_MODEL_COAT}


def swapped(rt, mats):
    """The table with the loose kinds swapped for exact ones."""
    m = mats.copy()
    for a, b in loose_types(rt).items():
        m["type"][mats["type"] == a] = b
    return m


def replaced(rt, mats, mtype):
    """The table with every entry of type `mtype` replaced by a different opaque material (what "this kind matters" is measured against)."""
    m = mats.copy()
    sel = mats["type"] == mtype
    m["type"][sel] = rt.RT_METAL if mtype == rt.RT_DIFFUSE else rt.RT_DIFFUSE
    m["texId"][sel] = -1
    m["color"][sel] = (0.9, 0.1, 0.5)
    m["param"][sel] = 0.3
    return m


def _soup(rt, types):
    rng = np.random.default_rng(SOUP_SEED)
    n = 400
    tris = np.zeros(n, rt.triangle_dtype)
    c = rng.uniform(-2, 2, (n, 1, 3)).astype(np.float32)
    tris["v"] = c + rng.uniform(-0.7, 0.7, (n, 3, 3)).astype(np.float32)
    tris["texCoords"] = rng.uniform(-2, 2, (n, 6))
    tris["meshID"] = rng.integers(0, 256, n)
    tris["_pad"] = rng.integers(1, 256, (n, 3))
    k = np.arange(256)
    mats = np.zeros(256, rt.material_dtype)
    mats["type"] = np.array(types)[k % len(types)]
    mats["color"] = rng.uniform(0.2, 1, (256, 3))
    mats["param"] = np.where(mats["type"] == rt.RT_GLASS, 1.5, np.where(mats["type"] == rt.RT_METAL, 0.1, 0.0))
    mats["texId"] = np.where(k % 16 == 5, 0, np.where(k % 16 == 13, 1, -1))
    return tris, mats


@functools.lru_cache(maxsize=None)
def frame(rt, O, name):
    """dict(hm, mats, tex, cam, nx, ny, depth, floor) of a named frame; floor: the plane of the soups (rendered with rt_render_options.floor = 1 unless a
    test turns it off), None for the staircase.  Shared: copy `mats` before changing it."""
    if name == "stair_loose":
        f = G.mesh_frame(rt, O, "staircase_b")
        return dict(hm=f["hm"], mats=f["mats"], tex=f["tex"], cam=f["cam"], nx=f["nx"], ny=f["ny"], depth=16, floor=None)
    if name == "stair_exact":
        hm, mats = G._staircase(rt)
        mats = mats.copy()
        for mid, kind in zip(G._stair_visible_ids(rt, O), STAIR_EXACT_KINDS):
            if kind.startswith("tex"):
                mats["texId"][mid] = int(kind[3])
                mats["type"][mid] = rt.RT_DIFFUSE
                if ":" in kind:
                    mats["type"][mid] = getattr(rt, kind[5:])
                    mats["param"][mid] = 0.05
            else:
                mats["type"][mid] = getattr(rt, kind)
                mats["texId"][mid] = -1
                if kind == "RT_GLASS":
                    mats["param"][mid] = 1.5
        nx, ny = G.STAIR_NX, G.STAIR_NY
        return dict(hm=hm, mats=mats, tex=G.stair_textures(), cam=rt.staircase_camera(nx, ny), nx=nx, ny=ny, depth=16, floor=None)
    if is_soup(name):
        tris, mats = _soup(rt, EXACT_TYPES if name == "soup_exact" else list(range(12)))
        nx, ny = 72, 56
        cam = rt.make_camera((4.5, 2.5, 6.0), (0, 0, 0), (0, 1, 0), 40.0, nx / ny, 0.02, 8.0)
        return dict(hm=rt.HostMesh.build(tris, 5), mats=mats, tex=G.stair_textures(), cam=cam, nx=nx, ny=ny, depth=12, floor=SOUP_FLOOR)
    raise KeyError(name)


def plain_stair_table(rt):
    """The staircase's own table (plain types, no texture): the lean kernels' scene."""
    return G._staircase(rt)[1]


def real_triangles(hm):
    """The leaf-ordered triangle records that are no sentinel."""
    return hm.tris[~np.isinf(hm.tris["v"][:, 0, 0])]


def light_structs(rt, light):
    """(rt.sphere, rt.vec3) of a light ((centre xyz), radius, (colour rgb)): the values of rt_render_options.light and .lightColor."""
    (cx, cy, cz), radius, (r, g, b) = light
    sp, col = rt.sphere(), rt.vec3()
    sp.center.e[:] = (cx, cy, cz)
    sp.radius = radius
    col.e[:] = (r, g, b)
    return sp, col


def frame_options(rt, O, name, nee=1, floor=None, light=None):
    """The oracle's options of a frame: mesh defaults with `nee`, and the floor plane on for the soups unless floor = 0.  light: None for the default light,
    else ((centre xyz), radius, (colour rgb))."""
    o = O.default_options(False)
    o.nee = nee
    o.floor = (1 if is_soup(name) else 0) if floor is None else floor
    if light is not None:
        o.light, o.lightColor = light_structs(rt, light)
    return o


def device_options(name, nee=1, floor=None, **more):
    """The same as setRenderOptions keywords."""
    return dict(more, nee=nee, floor=(1 if is_soup(name) else 0) if floor is None else floor)


def oracle_render(rt, O, name, ns, mats, nee=1, floor=None, lib=None, light=None):
    """(frame, counters) of the oracle (lib: O.load_nudge() for the nudged twin) for the frame's scene with the table `mats`."""
    f = frame(rt, O, name)
    fb, cnt = O.render(O.mesh_scene(f["hm"], mats, f["tex"], floor=f["floor"]), f["cam"], frame_options(rt, O, name, nee, floor, light), f["nx"], f["ny"], ns,
                       f["depth"], counters=True, lib=lib)
    fb.setflags(write=False)
    return fb, cnt


@functools.lru_cache(maxsize=None)
def oracle_frame(rt, O, name, ns, nee=1, floor=None, table="own", nudged=False, light=None):
    """The oracle's frame and counters, computed once and read-only.  table: "own", "swapped" (swapped()), "plain" (stair frames: plain_stair_table());
    light: as frame_options."""
    mats = frame(rt, O, name)["mats"]
    mats = {"own": mats, "swapped": swapped(rt, mats), "plain": plain_stair_table(rt) if not is_soup(name) else None}[table]
    return oracle_render(rt, O, name, ns, mats, nee, floor, O.load_nudge() if nudged else None, light)


@functools.lru_cache(maxsize=None)
def untouched(rt, O, name, ns, floor=None):
    """(ny, nx) bool: the pixels of a loose frame (NEE on) no libm-based preset had a part in."""
    a = oracle_frame(rt, O, name, ns, 1, floor)[0]
    b = oracle_frame(rt, O, name, ns, 1, floor, "swapped")[0]
    m = (bits(a) == bits(b)).all(axis=2)
    m.setflags(write=False)
    return m


def within_loose_bound(got, ref):
    """Per channel: |got - ref| <= 1e-5 * max(|ref|, 1e-3), the bound tests/test_gpu_parity_spheres.py and tests/test_gpu_renorm.py state for these presets."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) <= 1e-5 * np.maximum(np.abs(ref), 1e-3)


@functools.lru_cache(maxsize=None)
def pixel_list(rt, O, name):
    """(ij (n, 2) int32, first (n,) bool): every pixel once in a shuffled order and DUPLICATES duplicates spread through it, built as
    pixels_reference.standard_list builds its lists; first marks a pixel's first occurrence."""
    f = frame(rt, O, name)
    nx, ny = f["nx"], f["ny"]
    rng = np.random.default_rng(LIST_SEED[name])
    every = np.array([(i, j) for j in range(ny) for i in range(nx)], np.int32)[rng.permutation(nx * ny)]
    ij = np.concatenate([every, every[rng.integers(0, nx * ny, DUPLICATES)]])
    ij = np.ascontiguousarray(ij[rng.permutation(len(ij))])
    first = np.zeros(len(ij), bool)
    first[np.unique(ij[:, 1] * nx + ij[:, 0], return_index=True)[1]] = True
    ij.setflags(write=False)
    first.setflags(write=False)
    return ij, first


def init(rt, O, name, mats=None, **opts):
    """initRenderer of the frame's scene (with the table `mats` in place of its own) and setRenderOptions(defaults + opts); returns the framebuffer view."""
    f = frame(rt, O, name)
    ks, keep = rt.make_kernel_scene(f["hm"], f["mats"] if mats is None else mats, f["tex"], floor=f["floor"])
    fb = rt.initRenderer(ks, f["cam"], f["nx"], f["ny"], f["depth"], keepalive=keep)
    rt.setRenderOptions(rt.getDefaultRenderOptions(False), **opts)
    return fb
