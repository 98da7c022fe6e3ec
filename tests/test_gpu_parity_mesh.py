"""GPU parity, triangle-mesh/BVH path (kernels.cu:154-224,296-533 restated in HIP) against the CPU oracle.
Every operation is integer or IEEE fp32 on both sides: BIT-EXACT, with next-event estimation too - the light sample's cosf / sinf
(kernels.cu:378-379) are glibc's own algorithm restated on the device (csrc/rt_glibc_sincosf.h; round 2 held NEE frames to a tolerance)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def stair(rt):
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    return hm, mats


def _render_gpu(rt, hm, mats, cam, nx, ny, ns, depth, **opts):
    ks, keep = rt.make_kernel_scene(hm, mats)
    fb = rt.initRenderer(ks, cam, nx, ny, depth, keepalive=keep)
    o = rt.getDefaultRenderOptions(False)
    rt.setRenderOptions(o, **opts)
    rt.runRenderer(ns, 8, 8)
    out = np.array(fb, copy=True)
    st = rt.getRenderStats()
    rt.cleanupRenderer()
    return out, st


@pytest.mark.parametrize("variant", [0, 1, (1 << 8), (8 << 8), (1 << 24), (1 << 24) + (20 << 16)])   # 0 = persistent state machine (unified step), 1 = tile per wave; bits 8.. = WGs per CU; 1<<24 = while-while
def test_mesh_no_nee_bit_exact(rt, O, stair, variant):
    hm, mats = stair
    nx, ny, ns = 96, 120, 2
    cam = rt.staircase_camera(nx, ny)
    o = O.default_options(False)
    o.nee = 0
    ref, cnt = O.render(O.mesh_scene(hm, mats), cam, o, nx, ny, ns, 16, counters=True)
    got, st = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 16, nee=0, counters=1, variant=variant)
    assert np.array_equal(_bits(got), _bits(ref)), f"{np.count_nonzero(_bits(got) != _bits(ref))} differing words"
    assert st.rays == cnt.rays and st.node_visits == cnt.node_visits and st.prim_tests == cnt.prim_tests


@pytest.mark.parametrize("variant", [0, 1])
def test_mesh_nee_rr_bit_exact(rt, O, stair, variant):
    """The HEAD configuration (NEE + Russian roulette): image and every counter equal to the oracle's."""
    hm, mats = stair
    nx, ny, ns = 96, 120, 2
    cam = rt.staircase_camera(nx, ny)
    ref, cnt = O.render(O.mesh_scene(hm, mats), cam, O.default_options(False), nx, ny, ns, 64, counters=True)
    got, st = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 64, counters=1, variant=variant)
    assert np.array_equal(_bits(got), _bits(ref)), f"{np.count_nonzero(_bits(got) != _bits(ref))} differing words"
    assert (st.rays, st.shadow_rays, st.node_visits, st.prim_tests) == (cnt.rays, cnt.shadow_rays, cnt.node_visits, cnt.prim_tests)


def test_drop_in_link_against_reference_headers(rt, O, stair, tmp_path):
    """oracle/_ref/dropin_main was compiled against the REFERENCE'S kernels.h / helper_structs.h (its C++ classes,
    by-value kernel_scene + camera arguments) and linked to our librt_mi355x.so: the three extern "C" symbols of
    kernels.h:6-8 must bind and produce the same framebuffer as the Python ctypes path and the oracle."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "dropin_main")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/dropin_main was not built (needs /root/reference at build time)")
    nx, ny, ns, depth = 64, 80, 2, 12
    out = str(tmp_path / "fb.raw")
    r = subprocess.run([exe, str(nx), str(ny), str(ns), str(depth), out], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    got = np.fromfile(out, np.float32).reshape(ny, nx, 3)
    hm, mats = stair
    cam = rt.staircase_camera(nx, ny)
    via_python, _ = _render_gpu(rt, hm, mats, cam, nx, ny, ns, depth)          # mesh defaults: NEE on, RR on
    assert np.array_equal(_bits(got), _bits(via_python))
    ref, _ = O.render(O.mesh_scene(hm, mats), cam, O.default_options(False), nx, ny, ns, depth)
    assert np.array_equal(_bits(got), _bits(ref))


def test_mesh_variants_agree_bit_for_bit_with_nee(rt, stair):
    """Both kernels run the same device functions in the same per-lane order: with NEE + RR on (cos/sin included)
    they must agree with each other exactly, and textures (nearest texel, kernels.cu:456-476) too."""
    hm, mats = stair
    nx, ny, ns = 80, 96, 3
    cam = rt.staircase_camera(nx, ny)
    a, sa = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 64, counters=1, variant=0)
    for variant in (1, 1 << 24):                # tile per wave; persistent kernel with while-while traversal
        b, sb = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 64, counters=1, variant=variant)
        assert np.array_equal(_bits(a), _bits(b)), variant
        assert (sa.rays, sa.node_visits, sa.prim_tests) == (sb.rays, sb.node_visits, sb.prim_tests), variant


@pytest.fixture(scope="module")
def textured(rt, O, stair):
    """The staircase with three textured materials, 72x90 at 2 spp and depth 12 with NEE off, and the oracle's frame of it (computed once)."""
    hm, mats = stair
    mats = mats.copy()
    rng = np.random.default_rng(3)
    tex = [rng.uniform(0, 1, (16, 24, 3)).astype(np.float32), rng.uniform(0, 1, (7, 5, 3)).astype(np.float32)]
    mats["texId"][17] = 0       # floor
    mats["texId"][13] = 1       # back wall
    mats["texId"][19] = 0       # stairs
    nx, ny, ns = 72, 90, 2
    cam = rt.staircase_camera(nx, ny)
    o = O.default_options(False)
    o.nee = 0
    ref, _ = O.render(O.mesh_scene(hm, mats, tex), cam, o, nx, ny, ns, 12)
    return hm, mats, tex, cam, nx, ny, ns, ref


@pytest.mark.parametrize("variant", [0, 1])     # 0 = persistent state machine, 1 = tile per wave: each has its own call of the texture lookup
def test_mesh_textures_bit_exact(rt, textured, variant):
    """Albedo textures: nearest texel with wrap (kernels.cu:456-476), NEE off so the comparison is exact."""
    hm, mats, tex, cam, nx, ny, ns, ref = textured
    ks, keep = rt.make_kernel_scene(hm, mats, tex)
    fb = rt.initRenderer(ks, cam, nx, ny, 12, keepalive=keep)
    oo = rt.getDefaultRenderOptions(False)
    rt.setRenderOptions(oo, nee=0, variant=variant)
    rt.runRenderer(ns, 8, 8)
    got = np.array(fb, copy=True)
    rt.cleanupRenderer()
    assert np.array_equal(_bits(got), _bits(ref))


def test_mesh_stripe_partition_is_invisible(rt, stair):
    """The multi-GPU stripe partition on the mesh path: three partition members rendered in turn on the one GPU,
    interleaved, equal the whole frame bit for bit (NEE + RR on)."""
    hm, mats = stair
    nx, ny, ns = 64, 84, 2
    cam = rt.staircase_camera(nx, ny)
    whole, _ = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 32)
    merged = np.zeros_like(whole)
    for r in range(3):
        part, _ = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 32, part_rank=r, part_world=3, stripe_rows=8)
        for k in range(r, (ny + 7) // 8, 3):
            merged[k * 8:(k + 1) * 8] = part[k * 8:(k + 1) * 8]
    assert np.array_equal(_bits(merged), _bits(whole))


def test_mesh_fast_mode_within_tolerance(rt, O, stair):
    """FAST fp build of the mesh kernel (FMA contraction, 2.5-ulp divide/sqrt): same RNG stream, chaotic fp divergence
    (see the sphere-path test).  Stated tolerance at 96x120x4spp: >= 90 % of channels within 1e-3 absolute of the
    oracle, image RMSE (main.cpp:117-125) <= 0.05 — the frame's own Monte-Carlo noise at 4 spp is several times that."""
    hm, mats = stair
    nx, ny, ns = 96, 120, 4
    cam = rt.staircase_camera(nx, ny)
    ref, _ = O.render(O.mesh_scene(hm, mats), cam, O.default_options(False), nx, ny, ns, 64)
    got, _ = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 64, fp=rt.RT_FP_FAST)
    close = np.abs(got - ref) <= 1e-3
    print("mesh fast: close", close.mean(), "rmse", rt.rmse(got, ref))
    assert close.mean() >= 0.90
    assert rt.rmse(got, ref) <= 0.05


def _triangle_soup(rt, rng, n, n_mats=4):
    tris = np.zeros(n, rt.triangle_dtype)
    c = rng.uniform(-2, 2, (n, 1, 3)).astype(np.float32)
    tris["v"] = c + rng.uniform(-0.7, 0.7, (n, 3, 3)).astype(np.float32)
    tris["texCoords"] = rng.uniform(0, 1, (n, 6))
    tris["meshID"] = rng.integers(0, n_mats, n)
    mats = np.zeros(n_mats, rt.material_dtype)
    mats["type"] = [rt.RT_DIFFUSE, rt.RT_METAL, rt.RT_GLASS, rt.RT_DIFFUSE][:n_mats]
    mats["color"] = rng.uniform(0.2, 1, (n_mats, 3))
    mats["param"] = [0.0, 0.1, 1.5, 0.0][:n_mats]
    mats["texId"] = -1
    return tris, mats


@pytest.mark.parametrize("n,nppl", [(1, 1), (1, 5), (2, 1), (3, 2), (7, 5), (64, 8), (65, 3), (1000, 5), (1000, 16), (300, 20)])
def test_triangle_soups_and_leaf_sizes_bit_exact(rt, O, n, nppl):
    """Mesh shapes the staircase does not have: one triangle (the root's children are leaves), leaves of 1..20 slots (the
    pair rounds of the leaf phase handle <= 16, above that the sequential loop runs), sentinel-padded last leaves, overlapping
    random triangles with glass and metal.  NEE off: bit-exact image and equal ray / node-visit / triangle-test counts,
    in the default traversal, the classic while-while and the tile kernel."""
    rng = np.random.default_rng(4200 + 31 * n + nppl)
    tris, mats = _triangle_soup(rt, rng, n)
    hm = rt.HostMesh.build(tris, nppl)
    nx, ny, ns = 72, 56, 3
    cam = rt.make_camera((4.5, 2.5, 6.0), (0, 0, 0), (0, 1, 0), 40.0, nx / ny, 0.02, 8.0)
    o = O.default_options(False)
    o.nee = 0
    ref, cnt = O.render(O.mesh_scene(hm, mats), cam, o, nx, ny, ns, 12, counters=True)
    for variant in (0, 1 << 24, 1):
        got, st = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 12, nee=0, counters=1, variant=variant)
        assert np.array_equal(_bits(got), _bits(ref)), (variant, np.count_nonzero(_bits(got) != _bits(ref)))
        assert (st.rays, st.node_visits, st.prim_tests) == (cnt.rays, cnt.node_visits, cnt.prim_tests), variant


@pytest.mark.parametrize("depth", [0, 1, 2, 300])
def test_mesh_depth_limits(rt, O, stair, depth):
    """maxDepth 0 (the loop of kernels.cu:402 never runs: black frame), 1, 2, and above 255 (`uint8_t bounce`,
    helper_structs.h:58: clamped to 255 on both sides)."""
    hm, mats = stair
    nx, ny, ns = 48, 60, 2
    cam = rt.staircase_camera(nx, ny)
    o = O.default_options(False)
    o.nee = 0
    ref, _ = O.render(O.mesh_scene(hm, mats), cam, o, nx, ny, ns, min(depth, 255))
    got, _ = _render_gpu(rt, hm, mats, cam, nx, ny, ns, depth, nee=0)
    assert np.array_equal(_bits(got), _bits(ref))
    if depth == 0:
        assert not got.any()


def test_sentinel_in_the_middle_of_a_leaf(rt, O):
    """kernels.cu:202 stops a leaf at its FIRST sentinel triangle.  Builders pad leaves at the end, and the pair rounds of
    the mesh kernel rely on that; initRenderer checks it and a mesh with a real triangle BEHIND a sentinel takes the
    sequential leaf loop instead.  Same bits and counts as the oracle (which follows the reference literally)."""
    rng = np.random.default_rng(515)
    tris, mats = _triangle_soup(rt, rng, 200)
    hm = rt.HostMesh.build(tris, 5)
    t = hm.tris
    poked = 0
    for leaf in range(0, len(t) // 5, 3):
        if not np.isinf(t["v"][leaf * 5 + 2, 0, 0]):        # slots 0..2 real: hide slot 1, slot 2 becomes unreachable
            t["v"][leaf * 5 + 1, 0, 0] = np.inf
            poked += 1
    assert poked > 3
    nx, ny, ns = 72, 56, 3
    cam = rt.make_camera((4.5, 2.5, 6.0), (0, 0, 0), (0, 1, 0), 40.0, nx / ny, 0.02, 8.0)
    o = O.default_options(False)
    o.nee = 0
    ref, cnt = O.render(O.mesh_scene(hm, mats), cam, o, nx, ny, ns, 12, counters=True)
    for variant in (0, 1 << 24):
        got, st = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 12, nee=0, counters=1, variant=variant)
        assert np.array_equal(_bits(got), _bits(ref)), variant
        assert (st.rays, st.node_visits, st.prim_tests) == (cnt.rays, cnt.node_visits, cnt.prim_tests), variant


def test_larger_staircase_frame_bit_exact(rt, O):
    """A denser staircase (detail 2) at 320x180x4 spp, depth 64, Russian roulette on, NEE off (exact): the persistent kernel with
    all lanes busy for many iterations, queue refills, thresholded traversal and pair rounds, against the oracle's full frame."""
    tris, mats = rt.scene_staircase_procedural(2)
    hm = rt.HostMesh.build(tris, 5)
    nx, ny, ns = 320, 180, 4
    cam = rt.staircase_camera(nx, ny)
    o = O.default_options(False)
    o.nee = 0
    ref, cnt = O.render(O.mesh_scene(hm, mats), cam, o, nx, ny, ns, 64, counters=True)
    got, st = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 64, nee=0, counters=1)
    assert np.array_equal(_bits(got), _bits(ref)), f"{np.count_nonzero(_bits(got) != _bits(ref))} differing words"
    assert (st.rays, st.node_visits, st.prim_tests) == (cnt.rays, cnt.node_visits, cnt.prim_tests)


def _soup_with_floor(rt, rng, n=400):
    tris, mats = _triangle_soup(rt, rng, n)
    return tris, mats, (0.0, 1.0, 0.0, 0.0, -3.0, 0.0)      # plane {norm, point} (helper_structs.h:165-171)


@pytest.mark.parametrize("variant", [0, 1 << 24])
def test_floor_plane_and_reference_stats_bit_exact(rt, O, variant):
    """rt_render_options.floor = 1 re-enables the reference's commented-out floor call site (planeHit + floor_diffuse_scatter,
    kernels.cu:341-345,481-482) and counters = 1 fills the reference's 18 STATS counters (kernels.cu:47-67): with NEE off every
    operation is exact, so the frame AND every counter must equal the oracle's (which equals the reference-arithmetic twin,
    tests/test_oracle_vs_ref.py)."""
    rng = np.random.default_rng(4242)
    tris, mats, floor = _soup_with_floor(rt, rng)
    hm = rt.HostMesh.build(tris, 5)
    nx, ny, ns = 72, 56, 3
    cam = rt.make_camera((4.5, 2.5, 6.0), (0, 0, 0), (0, 1, 0), 40.0, nx / ny, 0.02, 8.0)
    for use_floor in (1, 0):
        o = O.default_options(False)
        o.nee = 0; o.floor = use_floor
        ref, cnt = O.render(O.mesh_scene(hm, mats, floor=floor), cam, o, nx, ny, ns, 12, counters=True)
        ks, keep = rt.make_kernel_scene(hm, mats, floor=floor)
        fb = rt.initRenderer(ks, cam, nx, ny, 12, keepalive=keep)
        oo = rt.getDefaultRenderOptions(False)
        rt.setRenderOptions(oo, nee=0, floor=use_floor, counters=1, variant=variant)
        rt.runRenderer(ns, 8, 8)
        got = np.array(fb, copy=True)
        st = rt.getRenderStats()
        rt.cleanupRenderer()
        assert np.array_equal(_bits(got), _bits(ref)), (use_floor, np.count_nonzero(_bits(got) != _bits(ref)))
        assert (st.rays, st.node_visits, st.prim_tests) == (cnt.rays, cnt.node_visits, cnt.prim_tests)
        assert list(st.ref_stats) == list(cnt.ref_stats), (use_floor, list(zip(rt.RT_STAT_NAMES, st.ref_stats, cnt.ref_stats)))
        if use_floor:
            assert st.ref_stats[rt.RT_STAT_SECONDARY_NOHIT] > 0 and st.ref_stats[rt.RT_STAT_PRIMARY_NOHITS] > 0
        assert st.ref_stats[rt.RT_STAT_PRIMARY] == nx * ny * ns and st.ref_stats[rt.RT_STAT_NODES_BOTH] + st.ref_stats[rt.RT_STAT_NODES_SINGLE] > 0


def test_floor_and_stats_with_nee_bit_exact(rt, O, stair):
    """The HEAD configuration (NEE + RR) with the floor on: image and all 18 STATS counters equal to the oracle's."""
    hm, mats = stair
    nx, ny, ns = 96, 120, 2
    cam = rt.staircase_camera(nx, ny)
    lo = np.array(hm.view.bounds.min.e[:])
    floor = (0.0, 1.0, 0.0, 0.0, float(lo[1]) + 30.0, 0.0)
    o = O.default_options(False)
    o.floor = 1
    ref, cnt = O.render(O.mesh_scene(hm, mats, floor=floor), cam, o, nx, ny, ns, 64, counters=True)
    ks, keep = rt.make_kernel_scene(hm, mats, floor=floor)
    fb = rt.initRenderer(ks, cam, nx, ny, 64, keepalive=keep)
    oo = rt.getDefaultRenderOptions(False)
    rt.setRenderOptions(oo, floor=1, counters=1)
    rt.runRenderer(ns, 8, 8)
    got = np.array(fb, copy=True)
    st = rt.getRenderStats()
    rt.cleanupRenderer()
    assert np.array_equal(_bits(got), _bits(ref)), np.count_nonzero(_bits(got) != _bits(ref))
    for k in range(18):
        assert int(st.ref_stats[k]) == int(cnt.ref_stats[k]), rt.RT_STAT_NAMES[k]
    assert st.ref_stats[rt.RT_STAT_SHADOWS] == st.shadow_rays > 0


@pytest.mark.parametrize("textured", [False, True])
def test_two_dispatch_cost_ordered_mesh_frame_bit_exact(rt, O, stair, textured):
    """From 16 spp the mesh frame is rendered in two dispatches (rt_kernels_mesh.hip, PHASE): 4 samples of every pixel measure its cost and park it (colour sum,
    stream position), the ordering pass of the sphere kernel sorts the pixels longest first, the second dispatch resumes every stream where it stopped.  No sample
    is traced twice or differently: the frame equals the oracle's bit for bit - the lean instantiation (untextured basic materials) and the general one (a
    textured scene), NEE + RR on - and equals the single dispatch (8 spp prefix of the same streams is covered by the other tests); three stripe members too."""
    hm, mats = stair
    tex = []
    if textured:
        mats = mats.copy()
        rng = np.random.default_rng(3)
        tex = [rng.uniform(0, 1, (16, 24, 3)).astype(np.float32)]
        mats["texId"][17] = 0; mats["texId"][19] = 0
    nx, ny, ns = 56, 72, 20
    cam = rt.staircase_camera(nx, ny)
    ref, _ = O.render(O.mesh_scene(hm, mats, tex), cam, O.default_options(False), nx, ny, ns, 24)
    ks, keep = rt.make_kernel_scene(hm, mats, tex)
    fb = rt.initRenderer(ks, cam, nx, ny, 24, keepalive=keep)
    rt.runRenderer(ns, 8, 8)
    got = np.array(fb, copy=True)
    assert np.array_equal(_bits(got), _bits(ref)), np.count_nonzero(_bits(got) != _bits(ref))
    rt.runRenderer(ns, 8, 8)                                         # a second frame into the same buffers (queue, lists, parked state are per frame)
    assert np.array_equal(_bits(np.array(fb)), _bits(ref))
    o = rt.getDefaultRenderOptions(False)
    merged = np.zeros_like(got)
    for r in range(3):
        rt.setRenderOptions(o, part_rank=r, part_world=3, stripe_rows=8)
        rt.runRenderer(ns, 8, 8)
        part = np.array(fb, copy=True)
        for k in range(r, (ny + 7) // 8, 3):
            merged[k * 8:(k + 1) * 8] = part[k * 8:(k + 1) * 8]
    assert np.array_equal(_bits(merged), _bits(ref))
    # chain waves (second dispatch: the most expensive pixels, a few per wave, in waves that take nothing else until they are done, then join the queue): with the
    # list-0 threshold at its floor and the "few pixels only" guard off EVERY pixel goes through them - 1, 6 and (auto-raised) more pixels per wave - and with 0 none
    import os
    saved = {k: os.environ.get(k) for k in ("RT_MESH_CHAIN_THR", "RT_MESH_CHAIN_LANES", "RT_MESH_CHAIN_FRAC")}
    try:
        rt.setRenderOptions(o, part_rank=0, part_world=1, stripe_rows=8)
        for thr, lanes, frac in ((17, 1, 0), (17, 6, 0), (17, 64, 0), (100, 3, 0), (448, 0, 8)):
            os.environ.update(RT_MESH_CHAIN_THR=str(thr), RT_MESH_CHAIN_LANES=str(lanes), RT_MESH_CHAIN_FRAC=str(frac))
            rt.runRenderer(ns, 8, 8)
            assert np.array_equal(_bits(np.array(fb)), _bits(ref)), (thr, lanes, frac)
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    rt.cleanupRenderer()


def test_traffic_forms_of_the_two_dispatch_mesh_frame_bit_exact(rt, O, stair, monkeypatch):
    """The traffic forms of the two-dispatch frame in the mesh kernel (32-byte parked records, one set of cost lists and queue counters per XCD with the
    other XCDs' waves taking what a queue has left - chain pixels too -, a first dispatch that scatters 8-pixel row segments): the legacy form, each alone, all together
    (the default) - the oracle's bits, also with every pixel forced through the chain lists (1 and 6 per wave) on a frame of a few workgroups (most XCDs have no wave:
    their queues are emptied by the others alone), and for three stripe members."""
    hm, mats = stair
    nx, ny, ns = 88, 72, 16
    cam = rt.staircase_camera(nx, ny)
    ref, _ = O.render(O.mesh_scene(hm, mats), cam, O.default_options(False), nx, ny, ns, 24)
    off = {"RT_ORD_PACKED": "0", "RT_XCD_QUEUES": "0", "RT_P1_TILE": "0"}
    combos = [{}, {"RT_ORD_PACKED": "1"}, {"RT_XCD_QUEUES": "1"}, {"RT_P1_TILE": "2"}, {"RT_ORD_PACKED": "1", "RT_XCD_QUEUES": "1", "RT_P1_TILE": "2"}]
    ks, keep = rt.make_kernel_scene(hm, mats)
    fb = rt.initRenderer(ks, cam, nx, ny, 24, keepalive=keep)
    o = rt.getDefaultRenderOptions(False)
    for combo in combos:
        for n in off:
            monkeypatch.setenv(n, combo.get(n, off[n]))
        for thr, lanes, frac in ((448, 3, 8), (17, 1, 0), (17, 6, 0)):
            monkeypatch.setenv("RT_MESH_CHAIN_THR", str(thr)); monkeypatch.setenv("RT_MESH_CHAIN_LANES", str(lanes)); monkeypatch.setenv("RT_MESH_CHAIN_FRAC", str(frac))
            rt.setRenderOptions(o, part_rank=0, part_world=1, stripe_rows=8)
            for frame in range(2):
                fb[:] = 0
                rt.runRenderer(ns, 8, 8)
                got = np.array(fb, copy=True)
                assert not np.isnan(got).any(), (combo, thr, lanes, frame)
                assert np.array_equal(_bits(got), _bits(ref)), (combo, thr, lanes, frame, np.count_nonzero(_bits(got) != _bits(ref)))
        fb[:] = 0
        for r in range(3):
            rt.setRenderOptions(o, part_rank=r, part_world=3, stripe_rows=8)
            rt.runRenderer(ns, 8, 8)
        assert np.array_equal(_bits(np.array(fb)), _bits(ref)), (combo, "stripes")
    rt.cleanupRenderer()


def test_full_size_c4_frame_two_dispatches_with_chain_waves_equals_single_dispatch(rt):
    """BASELINE config C4's scene and frame (detail-4 staircase, 1920x1080, depth 64, NEE + RR) at 16 spp: the production frame - two dispatches, cost
    order, expensive lists spread, the ~0.1 % most expensive pixels in chain waves with their real list-0 threshold - against the single scattered dispatch
    of the counting instantiation (which the tests above hold to the oracle), bit for bit; its chain-less form too."""
    import os
    tris, mats = rt.scene_staircase_procedural(4)
    hm = rt.HostMesh.build(tris, 5)
    nx, ny, ns = 1920, 1080, 16
    cam = rt.staircase_camera(nx, ny)
    single, _ = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 64, counters=1)
    two, _ = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 64)
    assert np.array_equal(_bits(two), _bits(single)), np.count_nonzero(_bits(two) != _bits(single))
    saved = os.environ.get("RT_MESH_CHAIN_LANES")
    try:
        os.environ["RT_MESH_CHAIN_LANES"] = "0"
        plain, _ = _render_gpu(rt, hm, mats, cam, nx, ny, ns, 64)
    finally:
        if saved is None: os.environ.pop("RT_MESH_CHAIN_LANES", None)
        else: os.environ["RT_MESH_CHAIN_LANES"] = saved
    assert np.array_equal(_bits(plain), _bits(single))
