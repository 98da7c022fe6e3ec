"""GPU checks of the three passes whose indexing changes once an image holds more than 1024 workgroups of 256 items (tests/capped_grids_support.py has the
two shapes: E = 512 x 512, exactly 1024 workgroups, and L = 523 x 503, 1028 of them): the histogram of displayFrame strides over the image, the count and
scatter of refineFrame go round twice, and a lane of the scan of rasterTexels / bakeTexels holds two counts.  Every comparison is the one the pass's own
GPU tests make at small sizes - against tests/display_reference.py, tests/refine_reference.py, tests/texels_reference.py and gatherRadiance - bit for bit;
tests/test_capped_grids_api.py shows on the references alone that the inputs reach what they are aimed at.  RT_REFINE_ORDER=0, the ascending scatter of
refineFrame, is run here too, at L and at 13 x 5."""
import numpy as np
import pytest

import capped_grids_support as S
import display_reference as D
import gather_reference as GR
import refine_reference as RR
import texels_reference as TR
from preview_support import bits, same
from texels_support import check_bake, check_raster, full_list, init, max_dist_of, private_mesh

pytestmark = pytest.mark.gpu
A = D.AUTO_EXPOSURE
ALL = D.TOP_DOWN | D.DITHER | D.AUTO_EXPOSURE
L = S.L


def _spheres(rt, nx, ny, depth=20):
    sp, mt, cam = rt.scene_three_spheres(nx, ny)
    return rt.initRendererSpheres(sp, mt, cam, nx, ny, depth)


# ---- 1. displayFrame past the histogram cap ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tonemap,plain", [(D.NONE, 0), (D.REINHARD, D.TOP_DOWN), (D.ACES, D.DITHER)])
@pytest.mark.parametrize("shape", sorted(S.SHAPES))
def test_display_synthetic_frames(rt, shape, tonemap, plain):
    """Every case of D.CASES with RT_DISPLAY_AUTO_EXPOSURE and one without per tone map, two calls each: the bytes, rtLastExposure and the histogram."""
    nx, ny = S.SHAPES[shape]
    frame = D.synthetic(100 + nx, nx, ny)
    src = np.ascontiguousarray(frame)
    flag_sets = [f for t, f in D.CASES if t == tonemap and f & A] + [plain]
    assert flag_sets == [A, ALL, plain] and (tonemap, plain) in D.CASES
    _spheres(rt, nx, ny)
    try:
        ref = D.Display()
        for flags in flag_sets:
            D.check(rt, ref, frame, src, flags, tonemap, what=f"{nx}x{ny}")
            D.check(rt, ref, frame, src, flags, tonemap, exposure=0.37, adapt=0.5, what=f"{nx}x{ny}")
    finally:
        rt.cleanupRenderer()


def test_display_counts_past_16_bits_and_hangs_on_round_two(rt):
    """At L: the synthetic frame scaled by 2^8, whose last bin holds more than 65 535 pixels, and the frame whose median bin is decided by the 925 pixels of
    the histogram kernel's second round - their two bins hold nothing else, and dropping or doubling them moves the exposure
    (tests/test_capped_grids_api.py)."""
    nx, ny = L
    scaled = D.synthetic(100 + nx, nx, ny, 256.0)
    hung, (r1, r2) = D.round_two_frame(7, nx, ny, S.CAP_ITEMS)
    _spheres(rt, nx, ny)
    try:
        ref = D.Display()
        D.check(rt, ref, scaled, np.ascontiguousarray(scaled), A, D.NONE, what="scaled by 256")
        assert rt.display_histogram()[-1] > 65535
        ref.reset()
        rt.reset_display()
        D.check(rt, ref, hung, np.ascontiguousarray(hung), A, D.REINHARD, what="round two decides")
        hist = rt.display_histogram()
        assert int(hist[r1]) + int(hist[r2]) == nx * ny - S.CAP_ITEMS == 925
    finally:
        rt.cleanupRenderer()


# ---- 2. refineFrame past the grid cap, and the ascending form ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frames_at_L(rt, O):
    """This renderer's own frames of the three spheres at L at 2, 4, 6 and 8 samples per pixel (tests/test_gpu_parity_spheres.py and tests/test_gpu_pixels.py
    hold such frames to the oracle bit for bit), anchored once more to the oracle on S.CROPS, and renderPixels' rays of every pixel over its first 2, 4 and 6
    samples.  Read-only, shared by the tests below."""
    nx, ny = L
    batch, _, max_samples, _ = RR.CASES[S.REFINE_TAG]
    fb = RR.init(rt, S.REFINE_TAG)
    try:
        frames, rays = {}, {}
        for n in range(batch, max_samples + 1, batch):
            rt.runRenderer(n, 8, 8)
            frames[n] = np.array(fb, copy=True)
            frames[n].setflags(write=False)
        for n in range(batch, max_samples, batch):
            rays[n] = rt.render_pixels(S.every_pixel(nx, ny), n, rays=True)[2].reshape(ny, nx)
            rays[n].setflags(write=False)
    finally:
        rt.cleanupRenderer()
    sp, mt, cam = rt.scene_three_spheres(nx, ny)
    for n, frame in frames.items():
        for x0, y0, x1, y1 in S.CROPS:
            ref = O.render(O.sphere_scene(sp, mt), cam, O.default_options(True), nx, ny, n, 50, region=(x0, y0, x1, y1))[0]
            same(frame[y0:y1, x0:x1], ref[y0:y1, x0:x1], f"runRenderer({n}) at L against the oracle on {(x0, y0, x1, y1)}")
    assert len({bits(f[180:196, 240:272]).tobytes() for f in frames.values()}) == len(frames)         # (the block is not sky: its pixels move with n)
    return frames, rays


def _check_call(got, ref, what):
    sampled, out, samples, error = got
    assert sampled == ref[0], (what, sampled, ref[0])
    assert np.array_equal(samples, ref[2]), (what, int((samples != ref[2]).sum()))
    same(error, ref[3], f"{what}: error")
    same(out, ref[1], f"{what}: out")


def _run(rt, tag, flags, ref):
    """The frame of `tag` to completion: every call's planes, the sample total after it and its list."""
    batch, min_batches, max_samples, threshold = RR.CASES[tag]
    RR.init(rt, tag)
    try:
        assert rt.refine_samples() == 0 and len(rt.refine_last_list()) == 0
        got, totals, lists = [], [], []
        for _ in ref:
            got.append(rt.refine_frame(batch, min_batches, max_samples, threshold, flags))
            totals.append(rt.refine_samples())
            lists.append(rt.refine_last_list())
            assert rt.last_refine_ms() > 0.0
    finally:
        rt.cleanupRenderer()
    return got, totals, lists


def _check_run(run, ref, batch, what):
    got, totals, lists = run
    print(what, "sampled per call", [g[0] for g in got])
    traced = 0
    for k, (g, r) in enumerate(zip(got, ref)):
        _check_call(g, r, f"{what} call {k + 1}")
        traced += r[0] * batch
        assert totals[k] == traced and len(lists[k]) == r[0]
    assert got[-1][0] == 0


@pytest.mark.parametrize("flags", [0, RR.DILATE])
def test_refine_to_completion_every_call(rt, O, frames_at_L, flags):
    """As tests/test_gpu_refine.py::test_to_completion_every_call, at L: sampled, out, samples, error and rtRefineSamples after every call, and the list of
    every pass - exactly the reference's active set, no pixel missing and none twice, the classes non-increasing along it."""
    frames, rays = frames_at_L
    nx, ny = L
    batch = RR.CASES[S.REFINE_TAG][0]
    ref = RR.run(rt, O, S.REFINE_TAG, flags, frames=frames.__getitem__)
    run = _run(rt, S.REFINE_TAG, flags, ref)
    _check_run(run, ref, batch, f"L dilate {flags}")
    cls = S.check_lists(ref, run[2], rays.__getitem__, nx, batch)
    print("classes per pass", [np.unique(c).tolist() for c in cls])
    assert len(ref) >= 5 and 0 < ref[2][0] < nx * ny and len(np.unique(cls[2])) >= 3
    in_round_two = ref[2][4].ravel()[S.CAP_ITEMS:]
    assert in_round_two.any() and not in_round_two.all()


@pytest.mark.parametrize("tag,flags", [(S.REFINE_TAG, RR.DILATE), ("S1_13x5", 0), ("S1_13x5", RR.DILATE)])
def test_refine_ascending_order(rt, O, frames_at_L, monkeypatch, tag, flags):
    """RT_REFINE_ORDER=0 (refineFrame reads its switches once per call): k_refine_scatter_ascending, one workgroup of 1024 lanes walking the image with a
    running base - 257 steps at L, the last one partial, and one step of one wave + 1 at 13 x 5.  Every plane and return value of every call equals the
    reference's and the default order's; the list of every pass ascends strictly in j * nx + i and is the active set."""
    nx, ny = RR.size(tag)
    batch = RR.CASES[tag][0]
    if tag == S.REFINE_TAG:
        frames, rays = frames_at_L
        ref = RR.run(rt, O, tag, flags, frames=frames.__getitem__)
        rays_of = rays.__getitem__
    else:
        ref = RR.run(rt, O, tag, flags)
        rays_of = lambda n: RR.oracle_rays(rt, O, tag, n)
    default = _run(rt, tag, flags, ref)
    monkeypatch.setenv("RT_REFINE_ORDER", "0")
    try:
        ascending = _run(rt, tag, flags, ref)
    finally:
        monkeypatch.delenv("RT_REFINE_ORDER")
    _check_run(ascending, ref, batch, f"{tag} dilate {flags}, ascending")
    _check_run(default, ref, batch, f"{tag} dilate {flags}, default order")
    for k, (a, d) in enumerate(zip(ascending[0], default[0])):
        assert a[0] == d[0]
        for x, y in zip(a[1:], d[1:]):
            assert np.array_equal(bits(x), bits(y)), (tag, k)
    S.check_lists(ref, ascending[2], rays_of, nx, batch, ascending=True)
    cls = S.check_lists(ref, default[2], rays_of, nx, batch)
    differ = [k for k, (a, d) in enumerate(zip(ascending[2], default[2])) if not np.array_equal(a, d)]
    print(tag, "passes whose list differs between the orders", differ, "classes of pass 3", np.unique(cls[2]).tolist())
    assert differ                                                                                    # the switch took effect


# ---- 3. rasterTexels / bakeTexels past one count per scan lane --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def meshes(rt, tmp_path_factory):
    """M1 and M2_floor with rtAtlasGrid UVs, read-only."""
    m = {tag: private_mesh(rt, tag, tmp_path_factory.mktemp("capped")) for tag in ("M1", "M2_floor")}
    for tag, hm in m.items():
        assert hm.tris.tobytes() == S.base_tris(rt, tag).tobytes()                                  # what tests/test_capped_grids_api.py looked at
    return m


def _upload(rt, meshes, name, W, H):
    """init of the atlas's mesh and the atlas uploaded through updateTriangles (the grid atlas is the mesh's own): (tris, slots, dilate)."""
    mesh, dilate = S.ATLASES[name]
    tris, slots = S.atlas(name, meshes[mesh].tris.copy(), W, H)
    init(rt, meshes, mesh)
    if name != "grid":
        rt.update_triangles(0, tris)
    return tris, slots, dilate


@pytest.mark.parametrize("name", sorted(S.ATLASES))
@pytest.mark.parametrize("shape", sorted(S.SHAPES))
def test_raster(rt, meshes, shape, name):
    """Every plane and the return value against the numpy raster and the host twin: M2_floor's own grid atlas (dilate 2), random overlapping UVs on M1
    (dilate 1, counts near 256 per workgroup) and one UV triangle across half of the atlas (dilate 0: a coverage walk of 156 000 texels by one wave)."""
    W, H = S.SHAPES[shape]
    try:
        tris, slots, dilate = _upload(rt, meshes, name, W, H)
        ref = check_raster(rt, tris, W, H, dilate, f"{name} at {shape}", slots=slots)
    finally:
        rt.cleanupRenderer()
    counts = S.group_counts(ref["prim"])
    assert len(counts) == S.groups_of(W * H) and (shape == "E" or counts[S.CAP:].any())


def _bake_at_L(rt, meshes, name, mode, dirs, ns):
    W, H = L
    mesh = S.ATLASES[name][0]
    kw = dict(ns=ns, base_id=5, bias=1e-3, max_dist=max_dist_of(mesh), rays=True)
    try:
        _upload(rt, meshes, name, W, H)
        owned, pl, pos, nrm = full_list(rt, W, H, 1)
        got = rt.bake_texels(W, H, mode, dirs, dilate=1, **kw)
        print(name, "mode", mode, "owned", got[0], "texels ms", rt.last_texels_ms(), "bake ms", rt.last_bake_ms())
        ref = rt.gather_radiance(pos, nrm, mode, dirs, **kw)
    finally:
        rt.cleanupRenderer()
    check_bake(got, pl, ref, f"{name} at L, mode {mode}")
    past = (pl["prim"] != TR.PRIM_NONE).ravel()[S.CAP_ITEMS:]                                       # the owned texels of the workgroups from the 1024th on
    values = np.unique(got[1]["out"].reshape(W * H, -1)[S.CAP_ITEMS:][past], axis=0)
    print("owned texels from 262 144 on:", int(past.sum()), "distinct values of out there:", len(values))
    assert past.any() and len(values) > 2
    return got, pl


@pytest.mark.parametrize("name", ["grid", "overlapping"])
def test_bake_visibility(rt, meshes, name):
    """RT_GATHER_VISIBILITY at L, dirs = 4, dilate = 1, against gatherRadiance over the full W*H list: what reads rank and list of the workgroups past the
    1024th."""
    _bake_at_L(rt, meshes, name, GR.VISIBILITY, 4, 1)


def test_bake_irradiance(rt, meshes):
    """RT_GATHER_IRRADIANCE in PARITY, dirs = 2, ns = 1: the acc and rays scatter at width 3 past the boundary."""
    got, pl = _bake_at_L(rt, meshes, "overlapping", GR.IRRADIANCE, 2, 1)
    mask = pl["prim"] != TR.PRIM_NONE
    assert (got[1]["rays"][mask] >= 2).all() and (got[1]["acc"][~mask] == 0).all()
