"""The production forms of the render kernels: for every template instantiation the launchers can choose without diagnostics, a scene, a frame, the
options and environment that select it, and the launch records (rtLastLaunches, include/rt_api.h) that the frame must report.  No test: the table,
the scene builder and the render helpers, read by tests/test_gpu_kernel_forms.py (which renders every form and holds it to the CPU oracle) and by the CPU tripwire in
tests/test_kernel_forms_table.py (which holds this table to the launch sites in the kernel sources).

How the sphere launcher (plan_spheres, rt_kernels_spheres.hip) picks LEAN for a scene in the LDS:
  bit 0   every material is RT_DIFFUSE / RT_METAL / RT_GLASS
  bit 1   culling on, cell tables on, 1..128 small groups (16 spheres each): one group list per ray batch
  bit 4   ... of two words (33..64 small groups)        bit 5   ... of four words (65..128 small groups)
  bit 3   the group boxes share no extent on y (box_shared_axis != 2): the 3-axis prefilter
  bit 2   one-word lists on a frame of at least RT_LEAN6_PIXELS pixels: six waves per SIMD (12-wave workgroups, two per CU)
The hybrid copy (scenes past the full LDS copy) keeps 1 and the four-word kinds, the sample chunks (counter RNG) keep 1, 3 and 7; a scene past the
hybrid copy is read from global memory (SCENE 1, no lean kinds).  The plan clips a kind that is not built (the lists KindsFull, KindsChunked,
KindsHybrid) to its basic-materials bit or, failing that, to LEAN 0 (the general kernel); a launch of a kind that is not built is an error."""

# record words compared by the tests (the device and fp words are fixed: device 0, RT_FP_PARITY)
FAMILY_SPHERE_QUEUE, FAMILY_SPHERE_TILES, FAMILY_MESH_QUEUE, FAMILY_MESH_TILES = 1, 2, 3, 4
RECORD_FIELDS = ("family", "phase", "cls", "chunked", "dbg", "scene", "lean", "threads", "blocks")

NX, NY = 96, 64                 # the frame of every form: 12 x 8 tiles of 8 x 8 pixels
MESH_THREADS = 256              # the mesh kernel's workgroup (RT_MESH_WG_WAVES = 4 waves)
TWO_NS, ONE_NS = 8, 3           # two dispatches from 8 spp (reference stream), the single dispatch below


def _blocks(nx, ny, threads):
    """Workgroups of a persistent kernel on a small frame: one per `threads` pixels of whole 8x8 tiles (fewer than the machine holds)."""
    px = ((nx + 7) // 8) * ((ny + 7) // 8) * 64
    return (px + threads - 1) // threads


def sphere_rec(phase, cls, chunked, scene, lean, waves, nx=NX, ny=NY):
    return (FAMILY_SPHERE_QUEUE, phase, cls, int(chunked), 0, scene, lean, 64 * waves, _blocks(nx, ny, 64 * waves))


def sphere_two(scene, lean, waves=16):
    """The cost-ordered frame in two dispatches: samples [0, 2) of every pixel, then the rest longest first."""
    return [sphere_rec(1, 0, False, scene, lean, waves), sphere_rec(2, 2, False, scene, lean, waves)]


def sphere_one(scene, lean, waves=16, cls=1, chunked=False):
    """One dispatch: ordered by the centre-ray pre-pass (CLS 1) for the full copy, scattered (CLS 0) for the hybrid copy and the global scene."""
    return [sphere_rec(0, cls, chunked, scene, lean, waves)]


def mesh_two(lean):
    return [(FAMILY_MESH_QUEUE, phase, 0, 0, 0, 0, int(lean), MESH_THREADS, _blocks(NX, NY, MESH_THREADS)) for phase in (1, 2)]


def mesh_one(lean):
    return [(FAMILY_MESH_QUEUE, 0, 0, 0, 0, 0, int(lean), MESH_THREADS, _blocks(NX, NY, MESH_THREADS))]


# Scene recipes (built by build_scene below):
#   ("random",)                   rt.scene_random_spheres: 488 spheres resting on y = 0.2, 31 small groups (the benchmark's scene)
#   ("cloud", n, shape, presets)  n - 1 small spheres + one ground sphere; shape "plane_y" / "plane_x" / "plane_z": centres and radii equal on that
#                                 axis (the group boxes share that extent), "volume": centres and radii spread on all three axes; presets: every
#                                 seventh small sphere takes a preset material without libm calls (not basic: LEAN 0, still bit-exact)
#   ("staircase", textured)       the procedural staircase mesh (detail 1, 5 triangles per leaf); textured: albedo textures on the floor and the stairs
# opts: rt_render_options fields; env: environment of the render (the renderer reads its switches once per frame); tol: the counter stream's sample
# chunks are added in chunk order - the tolerance of test_counter_rng_sample_chunks instead of bits.
_COUNTER = {"rng": 1, "samples_per_item": 2}        # RT_RNG_COUNTER, two samples per work item: ONE_NS = 3 samples in two chunks
_LEAN6 = {"RT_LEAN6_PIXELS": "1"}

FORMS = [
    # ---- SCENE 0: the full copy in the LDS, two dispatches and the single dispatch
    dict(name="full_general_two", scene=("cloud", 488, "plane_y", True), ns=TWO_NS, records=sphere_two(0, 0)),
    dict(name="full_general_one", scene=("cloud", 488, "plane_y", True), ns=ONE_NS, records=sphere_one(0, 0)),
    dict(name="full_lean1_two", scene=("random",), ns=TWO_NS, env={"RT_BOX_CELLS": "0"}, records=sphere_two(0, 1)),
    dict(name="full_lean1_one", scene=("random",), ns=ONE_NS, env={"RT_BOX_CELLS": "0"}, records=sphere_one(0, 1)),
    dict(name="full_lean3_two", scene=("random",), ns=TWO_NS, records=sphere_two(0, 3)),
    dict(name="full_lean3_one", scene=("random",), ns=ONE_NS, records=sphere_one(0, 3)),
    dict(name="full_lean7_two", scene=("random",), ns=TWO_NS, env=_LEAN6, records=sphere_two(0, 7, waves=12)),
    dict(name="full_lean7_one", scene=("random",), ns=ONE_NS, env=_LEAN6, records=sphere_one(0, 7, waves=12)),
    dict(name="full_lean11_two", scene=("cloud", 488, "volume", False), ns=TWO_NS, records=sphere_two(0, 11)),
    dict(name="full_lean11_one", scene=("cloud", 488, "volume", False), ns=ONE_NS, records=sphere_one(0, 11)),
    dict(name="full_lean11_plane_x", scene=("cloud", 200, "plane_x", False), ns=TWO_NS, records=sphere_two(0, 11)),
    dict(name="full_lean11_plane_z", scene=("cloud", 200, "plane_z", False), ns=ONE_NS, records=sphere_one(0, 11)),
    dict(name="full_lean15_two", scene=("cloud", 488, "volume", False), ns=TWO_NS, env=_LEAN6, records=sphere_two(0, 15, waves=12)),
    dict(name="full_lean15_one", scene=("cloud", 488, "volume", False), ns=ONE_NS, env=_LEAN6, records=sphere_one(0, 15, waves=12)),
    dict(name="full_lean19_two", scene=("cloud", 700, "plane_y", False), ns=TWO_NS, records=sphere_two(0, 19)),
    dict(name="full_lean19_one", scene=("cloud", 700, "plane_y", False), ns=ONE_NS, records=sphere_one(0, 19)),
    dict(name="full_lean27_two", scene=("cloud", 700, "volume", False), ns=TWO_NS, records=sphere_two(0, 27)),
    dict(name="full_lean27_one", scene=("cloud", 700, "volume", False), ns=ONE_NS, records=sphere_one(0, 27)),
    dict(name="full_lean35_two", scene=("cloud", 1100, "plane_y", False), ns=TWO_NS, records=sphere_two(0, 35)),
    dict(name="full_lean35_one", scene=("cloud", 1100, "plane_y", False), ns=ONE_NS, records=sphere_one(0, 35)),
    dict(name="full_lean43_two", scene=("cloud", 1100, "volume", False), ns=TWO_NS, records=sphere_two(0, 43)),
    dict(name="full_lean43_one", scene=("cloud", 1100, "volume", False), ns=ONE_NS, records=sphere_one(0, 43)),
    # ---- SCENE 0, sample chunks of the counter stream (single dispatch, ordered)
    dict(name="chunked_general", scene=("cloud", 488, "plane_y", True), ns=ONE_NS, opts=_COUNTER, tol=True, records=sphere_one(0, 0, chunked=True)),
    dict(name="chunked_lean1", scene=("cloud", 488, "volume", False), ns=ONE_NS, opts=_COUNTER, tol=True, records=sphere_one(0, 1, chunked=True)),
    dict(name="chunked_lean3", scene=("random",), ns=ONE_NS, opts=_COUNTER, tol=True, records=sphere_one(0, 3, chunked=True)),
    dict(name="chunked_lean7", scene=("random",), ns=ONE_NS, opts=_COUNTER, tol=True, env=_LEAN6,
         records=sphere_one(0, 7, waves=12, chunked=True)),
    # ---- SCENE 2: the hybrid copy (test data in the LDS, hit data in global memory), single scattered dispatch
    dict(name="hybrid16_general", scene=("cloud", 2100, "volume", True), ns=ONE_NS, records=sphere_one(2, 0, cls=0)),
    dict(name="hybrid16_lean1", scene=("cloud", 2100, "volume", False), ns=ONE_NS, records=sphere_one(2, 1, cls=0)),
    dict(name="hybrid16_lean1_two_spp", scene=("cloud", 2100, "volume", False), ns=TWO_NS, records=sphere_one(2, 1, cls=0)),
    dict(name="hybrid16_lean35", scene=("cloud", 1800, "plane_y", False), ns=ONE_NS, records=sphere_one(2, 35, cls=0)),
    dict(name="hybrid16_lean43", scene=("cloud", 1800, "volume", False), ns=ONE_NS, records=sphere_one(2, 43, cls=0)),
    dict(name="hybrid8_general", scene=("cloud", 4000, "volume", True), ns=ONE_NS, records=sphere_one(2, 0, waves=8, cls=0)),
    dict(name="hybrid8_lean1", scene=("cloud", 4000, "volume", False), ns=ONE_NS, records=sphere_one(2, 1, waves=8, cls=0)),
    dict(name="hybrid16_chunked", scene=("cloud", 2100, "volume", False), ns=ONE_NS, opts=_COUNTER, tol=True,
         records=sphere_one(2, 0, cls=0, chunked=True)),                          # (basic materials, but no chunked hybrid kind is built: the plan takes the general kernel)
    # ---- SCENE 1: the whole scene in global memory, single scattered dispatch
    dict(name="global", scene=("cloud", 6000, "volume", False), ns=ONE_NS, records=sphere_one(1, 0, cls=0)),
    dict(name="global_chunked", scene=("cloud", 6000, "volume", False), ns=ONE_NS, opts=_COUNTER, tol=True, records=sphere_one(1, 0, cls=0, chunked=True)),
    # ---- mesh: the staircase (basic materials: the lean kernel; textured: the general one), NEE + RR, 16 spp = two dispatches
    dict(name="mesh_lean_two", scene=("staircase", False), ns=16, records=mesh_two(True)),
    dict(name="mesh_lean_one", scene=("staircase", False), ns=ONE_NS, records=mesh_one(True)),
    dict(name="mesh_general_two", scene=("staircase", True), ns=16, records=mesh_two(False)),
    dict(name="mesh_general_one", scene=("staircase", True), ns=ONE_NS, records=mesh_one(False)),
]

# Instantiations that only A/B switches reach (no production frame launches them; the tests of their switches hold them to the oracle):
#   key = (family, phase, cls, chunked, scene, lean) as in a launch record without the dbg / threads / blocks words
AB_ONLY = [
    dict(name="hybrid_two_dispatch", why="RT_HYBRID_TWO=1: the cost-ordered two dispatches for the hybrid copy",
         keys=[(FAMILY_SPHERE_QUEUE, 1, 0, 0, 2, lean) for lean in (0, 1, 35, 43)] + [(FAMILY_SPHERE_QUEUE, 2, 2, 0, 2, lean) for lean in (0, 1, 35, 43)]),
    dict(name="sphere_tiles", why="variant 1 / the legacy scans: one tile per wave", keys=[(FAMILY_SPHERE_TILES, 0, 0, 0, 0, 0), (FAMILY_SPHERE_TILES, 0, 1, 0, 0, 0)]),
    dict(name="mesh_tiles", why="mesh variant 1: one tile per wave", keys=[(FAMILY_MESH_TILES, 0, 0, 0, 0, 0)]),
    dict(name="mesh_classic", why="mesh variant 1 << 24: the classic while-while traversal", keys=[(FAMILY_MESH_QUEUE, 0, 1, 0, 0, 0)]),
]


def form_key(rec):
    """(family, phase, cls, chunked, scene, lean) of a record."""
    return (rec[0], rec[1], rec[2], rec[3], rec[5], rec[6])


def build_scene(rt, recipe, nx=NX, ny=NY):
    """The scene of a recipe: ("spheres", spheres, materials, camera) or ("mesh", HostMesh, materials, textures, camera)."""
    import numpy as np
    if recipe[0] == "random":
        sp, mt, cam = rt.scene_random_spheres(nx, ny)
        return ("spheres", sp, mt, cam)
    if recipe[0] == "staircase":
        tris, mats = rt.scene_staircase_procedural(1)
        hm = rt.HostMesh.build(tris, 5)
        tex = []
        if recipe[1]:
            mats = mats.copy()
            tex = [np.random.default_rng(3).uniform(0, 1, (16, 24, 3)).astype(np.float32)]
            mats["texId"][17] = 0; mats["texId"][19] = 0
        return ("mesh", hm, mats, tex, rt.staircase_camera(nx, ny))
    _, n, shape, presets = recipe
    rng = np.random.default_rng(1000 + n + 7 * len(shape))
    half = 6.0 * (n / 488.0) ** 0.5                     # (the density of the benchmark's scene at every size)
    sp = np.zeros(n, rt.sphere_dtype)
    mt = np.zeros(n, rt.material_dtype)
    c = rng.uniform(-half, half, (n, 3))
    if shape == "volume":
        c[:, 1] = rng.uniform(0.3, 0.4 * half, n)
        sp["radius"] = rng.uniform(0.1, 0.3, n)
    else:
        c[:, "xyz".index(shape[-1])] = 0.2
        sp["radius"] = 0.2
    sp["center"] = c
    sp["center"][0] = (0, -1000, 0); sp["radius"][0] = 1000
    mt["type"] = rng.integers(0, 3, n)
    mt["color"] = rng.uniform(0.1, 1, (n, 3))
    mt["param"] = np.where(mt["type"] == rt.RT_GLASS, 1.5, rng.uniform(0, 0.3, n))
    mt["texId"] = -1
    mt["type"][0] = rt.RT_DIFFUSE; mt["param"][0] = 0.0
    if presets:
        kinds = np.array([rt.RT_FLOOR_COAT, rt.RT_FLOOR_DIFFUSE, rt.RT_MODEL_COAT, rt.RT_MODEL_DIFFUSE, rt.RT_MODEL_GLOSSY, rt.RT_MODEL_GLASS])
        idx = np.arange(1, n, 7)
        mt["type"][idx] = kinds[idx % len(kinds)]
    cam = rt.make_camera((1.6 * half, 0.5 * half + 1.0, 1.1 * half), (0, 0.5, 0), (0, 1, 0), 40.0, nx / ny, 0.05, 2.0 * half)
    return ("spheres", sp, mt, cam)


def render_form(rt, form, counters=0, nx=NX, ny=NY):
    """Render a form through the C-ABI (PARITY build, the form's options; the caller sets its env): (framebuffer copy, launch records)."""
    import numpy as np
    sc = build_scene(rt, form["scene"], nx, ny)
    if sc[0] == "spheres":
        fb = rt.initRendererSpheres(sc[1], sc[2], sc[3], nx, ny, 20)
        o = rt.getDefaultRenderOptions(True)
    else:
        ks, keep = rt.make_kernel_scene(sc[1], sc[2], sc[3])
        fb = rt.initRenderer(ks, sc[4], nx, ny, 24, keepalive=keep)
        o = rt.getDefaultRenderOptions(False)
    rt.setRenderOptions(o, counters=counters, **form.get("opts", {}))
    rt.runRenderer(form["ns"], 8, 8)
    got = np.array(fb, copy=True)
    recs = [tuple(r[f] for f in RECORD_FIELDS + ("device", "fp")) for r in rt.last_launches()]
    rt.cleanupRenderer()
    return got, recs


def render_oracle(rt, O, form, nx=NX, ny=NY):
    sc = build_scene(rt, form["scene"], nx, ny)
    if sc[0] == "spheres":
        o = O.default_options(True)
        o.rng = form.get("opts", {}).get("rng", o.rng)
        return O.render(O.sphere_scene(sc[1], sc[2]), sc[3], o, nx, ny, form["ns"], 20)[0]
    return O.render(O.mesh_scene(sc[1], sc[2], sc[3]), sc[4], O.default_options(False), nx, ny, form["ns"], 24)[0]
