"""CPU: the host side of rebuildBvh (include/rt_api.h "editing the scene", include/rt_host.h).  rtRebuildBvh is the builder over the tree's own leaf count
followed by the refit: on the visible triangles of a mesh it yields the triangle bytes of rtBuildBvhLevels; an independent, level-synchronous numpy
restatement of the definition (tests/rebuild_support.py) agrees with it on quantised meshes, tiny, full and nearly full trees, hidden triangles, a
mostly empty tree and meshes at the float extremes (areas and costs that overflow to +inf or are NaN, nodes without a winner, costs that underflow to 0,
infinite and denormal centroids: each asserted from the restatement's own counts); old_slot is a bijection that moves whole triangles; refusals write nothing; and the rebuilt tree of a scrambled staircase is visited
less.  Every comparison is np.array_equal on raw words or bytes."""
import os
import re

import numpy as np
import pytest

import guides_reference as G
import rebuild_support as R
import scene_update_support as S
from preview_support import bits, exits_99

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rebuildBvh", "rtLastRebuildMs"]


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _twin_equals_builder(rt, hm, nppl, extra, what):
    first_leaf = hm.view.numBvhNodes // 2
    before = hm.tris.copy()
    v = before[R.visible_slots(before, first_leaf, nppl)]
    want = rt.HostMesh.build(v, nppl, extra_levels=extra)
    assert want.view.numBvhNodes == hm.view.numBvhNodes, what
    old_slot = hm.rebuild()
    assert hm.tris.tobytes() == want.tris.tobytes(), what + ": triangles against the builder's"
    want.refit()
    assert np.array_equal(_words(hm.bvh[1:]), _words(want.bvh[1:])), what + ": nodes against the refitted builder's"
    assert np.array_equal(bits(S.view_bounds(hm)), bits(S.view_bounds(want))), what
    R.check_old_slot(before, hm.tris, old_slot, first_leaf, nppl)


@pytest.mark.parametrize("nppl", [1, 3, 5])
@pytest.mark.parametrize("extra", [0, 1, 2])
def test_twin_equals_the_builder_staircase(rt, nppl, extra):
    tris, _ = rt.scene_staircase_procedural(1)
    hm = R.scrambled(rt.HostMesh.build(tris, nppl, extra_levels=extra))
    _twin_equals_builder(rt, hm, nppl, extra, f"staircase detail 1, nppl {nppl}, extra levels {extra}")


def test_twin_equals_the_builder_tris300(rt, O, tmp_path):
    hm = R.scrambled(S.fresh_copy(rt, G.mesh_frame(rt, O, "tris300")["hm"], tmp_path))
    _twin_equals_builder(rt, hm, 5, 1, "tris300, nppl 5")


def _numpy_cases(rt, O):
    yield "quantised, nppl 3", rt.HostMesh.build(R.quantised_tris(rt, 200), 3)
    yield "quantised, nppl 1, no spare level", rt.HostMesh.build(R.quantised_tris(rt, 97, seed=18), 1, extra_levels=0)
    for n in (1, 2, 3, 7):
        yield f"n = {n}", rt.HostMesh.build(S.blob_tris(rt, n, 20 + n), 2)
    yield "full tree", rt.HostMesh.build(S.blob_tris(rt, 8 * 3, 31), 3, extra_levels=0)
    yield "full tree less one", rt.HostMesh.build(S.blob_tris(rt, 8 * 3 - 1, 32), 3, extra_levels=0)
    yield "sentinel before real", S.sentinel_first_mesh(rt)
    src = G.mesh_frame(rt, O, "tris300")["hm"].tris
    yield "tris300 nppl 1, 2^17 leaves", rt.HostMesh.build(src[S.is_real(src)], 1, extra_levels=8)
    for case in R.EXTREMES:                                     # the float extremes: already scrambled
        yield case, R.extreme_mesh(rt, case)


CASES = ["quantised, nppl 3", "quantised, nppl 1, no spare level", "n = 1", "n = 2", "n = 3", "n = 7", "full tree", "full tree less one", "sentinel before real",
         "tris300 nppl 1, 2^17 leaves"] + list(R.EXTREMES)


def _claims(case, c):
    """What numpy_rebuild's counts must show for a case of R.EXTREMES to be what it claims."""
    nodes = c["winner"] + c["no_winner"]
    assert nodes >= 50, c
    if case == "scale 3e18":
        assert c["winner"] >= 10 and c["no_winner"] >= 10 and c["inf_costs"] >= 100 and c["nan_costs"] == 0
    if case in ("scale 1e25", "scale 1e37", "scale 2e37"):
        assert c["winner"] == 0 and c["no_winner"] == nodes and c["nan_costs"] == 0 and c["inf_costs"] == c["nonzero_costs"] > 0
        assert (c["inf_centroids"] > 0) == (case == "scale 2e37")
    if case.endswith("every 7th"):
        assert c["winner"] >= 10 and c["no_winner"] >= 10
        assert (c["mixed_nodes"] >= 1) == case.startswith("scale 1e18")
    if case == "flat in x, scale 2e37":
        assert c["nan_costs"] >= 100 and c["inf_costs"] >= 100 and c["winner"] == 0
    if case in ("scale 1e-25", "scale 1e-38", "scale 1e-44"):
        assert c["nonzero_costs"] == 0 and c["no_winner"] == 0 and c["inf_costs"] == 0
        small = c["denormal_centroids_pos"] >= 10 and c["denormal_centroids_neg"] >= 10
        assert small == (case != "scale 1e-25")


@pytest.mark.parametrize("case", CASES)
def test_twin_against_numpy(rt, O, case):
    hm = dict(_numpy_cases(rt, O))[case]
    nppl, first_leaf = hm.nppl, hm.view.numBvhNodes // 2
    if case.startswith("full tree"):
        n = int(S.is_real(hm.tris).sum())
        assert first_leaf == 8 and n == (24 if case == "full tree" else 23)
    if not case.startswith("sentinel") and case not in R.EXTREMES:
        R.scrambled(hm, 72)
    before = hm.tris.copy()
    hidden = int(S.is_real(before).sum()) - len(R.visible_slots(before, first_leaf, nppl))
    assert (hidden >= 4) == case.startswith("sentinel")
    counts = {}
    want_tris, want_old, want_nodes, want_bounds = R.numpy_rebuild(rt, before, hm.view.numBvhNodes, nppl, counts)
    if case in R.EXTREMES:
        print(case, counts)
        assert sorted(counts) == sorted(R.COUNTS) and int(S.is_real(before).sum()) == 200 and np.isfinite(before["v"][S.is_real(before)]).all()
        _claims(case, counts)
    old_slot = hm.rebuild()
    assert hm.tris.tobytes() == want_tris.tobytes(), case + ": triangles"
    assert np.array_equal(old_slot, want_old), case + ": old_slot"
    assert np.array_equal(_words(hm.bvh[1:]), _words(want_nodes[1:])), case + ": nodes"
    assert np.array_equal(bits(S.view_bounds(hm)), bits(want_bounds)), case + ": bounds"
    R.check_old_slot(before, hm.tris, old_slot, first_leaf, nppl)
    assert int(S.is_real(hm.tris).sum()) == int(S.is_real(before).sum()) - hidden          # the hidden triangles are dropped
    # a second rebuild is the twin of the rebuilt mesh: nothing more is claimed for it
    again = hm.tris.copy()
    want2 = R.numpy_rebuild(rt, again, hm.view.numBvhNodes, nppl)
    old2 = hm.rebuild()
    assert hm.tris.tobytes() == want2[0].tobytes() and np.array_equal(old2, want2[1]), case + ": second rebuild"


def test_arrays_entry_and_refusals(rt):
    hm = S.blob_mesh(rt, 8, 3)
    R.scrambled(hm, 73)
    tris, bvh = hm.tris.copy(), hm.bvh.copy()
    got = rt.rebuild_bvh_arrays(tris, bvh, 3)
    assert got is not None
    old = hm.rebuild()
    assert tris.tobytes() == hm.tris.tobytes() and np.array_equal(_words(bvh[1:]), _words(hm.bvh[1:])) and np.array_equal(got[1], old)
    assert np.array_equal(bits(got[0]), bits(S.view_bounds(hm)))
    # slots past first_leaf * nppl are kept and named by their own index
    longer = np.concatenate([hm.tris, S.blob_tris(rt, 5, 9)])
    keep = longer.copy()
    b2, o2 = rt.rebuild_bvh_arrays(longer, bvh.copy(), 3)
    assert longer[24:].tobytes() == keep[24:].tobytes() and np.array_equal(o2[24:], np.arange(24, 29))
    # a tree of 6 leaves: the refit takes it, the rebuild does not
    six = (np.concatenate([hm.tris, hm.tris])[:18].copy(), np.zeros(12, rt.bvh_node_dtype), 3)
    assert rt.refit_bvh_arrays(six[0], six[1].copy(), 3) is not None
    for what, args in (("odd numBvhNodes", (tris.copy(), bvh[:15].copy(), 3)), ("numBvhNodes below 4", (tris.copy(), bvh[:2].copy(), 3)),
                       ("first_leaf * nppl > numTris", (tris[:23].copy(), bvh.copy(), 3)), ("nppl 0", (tris.copy(), bvh.copy(), 0)),
                       ("6 leaves", six)):
        before = (args[0].copy(), args[1].copy())
        assert rt.rebuild_bvh_arrays(*args) is None, what
        assert args[0].tobytes() == before[0].tobytes() and args[1].tobytes() == before[1].tobytes(), what + ": something was written"
    h = rt.load_host()
    guard = np.full(24, 77, np.int32)
    assert h.rtRebuildBvhArrays(None, 24, bvh.ctypes.data, 16, 3, None, guard.ctypes.data) == -1
    assert h.rtRebuildBvhArrays(tris.ctypes.data, 24, None, 16, 3, None, guard.ctypes.data) == -1
    assert h.rtRebuildBvhArrays(tris.ctypes.data, 24, bvh.ctypes.data, 12, 3, None, guard.ctypes.data) == -1 and (guard == 77).all()
    assert h.rtRebuildBvh(None, None) == -1
    assert h.rtRebuildBvhArrays(tris.ctypes.data, 24, bvh.ctypes.data, 16, 3, None, None) == 0          # bounds and old_slot may be NULL


def test_wrappers_refuse_wrong_arrays_before_calling(rt, monkeypatch):
    monkeypatch.setattr(rt, "load_host", lambda: pytest.fail("the library was called"))
    tris, bvh = np.zeros(4, rt.triangle_dtype), np.zeros(4, rt.bvh_node_dtype)
    ro = tris.copy()
    ro.flags.writeable = False
    for bad in (tris.view(np.uint8), tris.reshape(2, 2), list(tris), None, bvh, ro, np.zeros(8, rt.triangle_dtype)[::2]):
        with pytest.raises(ValueError):
            rt.rebuild_bvh_arrays(bad, bvh, 1)
    for bad in (bvh.view(np.float32), bvh.reshape(2, 2), None, tris):
        with pytest.raises(ValueError):
            rt.rebuild_bvh_arrays(tris, bad, 1)
    for bad in (1.0, "1", None, True):
        with pytest.raises(ValueError):
            rt.rebuild_bvh_arrays(tris, bvh, bad)


def test_symbols_are_declared_and_bound(rt):
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    host = open(os.path.join(ROOT, "include", "rt_host.h")).read()
    lib = rt.load_renderer()
    for name in NEW:
        assert name in rt.RENDERER_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\(" % name, hdr), name
    for name in ("rtRebuildBvhArrays", "rtRebuildBvh"):
        assert name in rt.HOST_SYMBOLS and hasattr(rt.load_host(), name) and re.search(r"\b%s\(" % name, host), name
    assert re.search(r"#define RT_API_VERSION 1002\b", hdr)                 # additive: no struct changed
    tile = int(re.search(r"^#define RT_REBUILD_TILE (\d+)\s*$", hdr, re.M).group(1))
    assert rt.RT_REBUILD_TILE == tile and rt.RT_REBUILD_MAX_TRIS >= 1 << 20
    assert "rebuildBvh" in re.search(r"the tree is always refitted as a whole\.(.*?)\n \*\n", hdr, re.S).group(1)     # the refit's text points at the rebuild


@pytest.mark.parametrize("call", ["rt.rebuild_bvh()", "rt.last_rebuild_ms()", "rt.load_renderer().rebuildBvh(None)"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99(call + "\n")


def test_translation_unit():
    """The build kernels are one object of their own with display.o's flags, linked through BUILD_OBJS; only the renderer and the kernels know the header; the
    refit's rule and object list are what they were."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    rules = re.findall(r"^\$\(OBJ\)/(\S+)\.o:\s*\$\(CSRC\)/rt_kernels_build\.hip([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert len(rules) == 1 and rules[0][0] == "build", rules
    assert "$(CSRC)/rt_build.h" in rules[0][1].split()
    display = re.search(r"^\$\(OBJ\)/display\.o:[^\n]*\n\t([^\n]+)", mk, re.M).group(1)
    assert rules[0][2].split() == display.split() and "-ffp-contract=off" in rules[0][2].split()
    link = re.search(r"^\$\(PKG\)/librt_mi355x\.so:([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert "$(BUILD_OBJS)" in link.group(1).split() and "$(BUILD_OBJS)" in link.group(2).split()
    assert re.search(r"^BUILD_OBJS\s*:=\s*\$\(OBJ\)/build\.o\s*$", mk, re.M) and re.search(r"^UPDATE_OBJS\s*:=\s*\$\(OBJ\)/update\.o\s*$", mk, re.M)
    csrc = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")
    users = sorted(name for name in os.listdir(csrc) if name != "rt_build.h" and "rt_build.h" in open(os.path.join(csrc, name)).read())
    assert users == ["rt_kernels_build.hip", "rt_renderer.hip"], users
    kernel = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "rt_kernels_build.hip")).read())
    assert "rocprim" not in kernel.lower() and "hipcub" not in kernel.lower()
    assert set(re.findall(r"\batomic\w+", kernel)) <= {"atomicAdd", "atomicMin"}      # integer counters in LDS, an integer minimum: no order-dependent outcome


def test_rebuilt_tree_is_visited_less(rt, O):
    """The point of the call.  Node visits of the centre rays of a 40 x 50 frame (the oracle's RT_GUIDE_NODES plane) on the staircase: scrambled and refitted,
    rebuilt, and built from the triangles in their original order.  The last two differ in tie-breaks only: the factor 1.25 is a cap against a broken
    twin, not a measurement."""
    tris, mats = rt.scene_staircase_procedural(1)
    nx, ny = G.STAIR_NX, G.STAIR_NY
    cam = rt.staircase_camera(nx, ny)

    def visits(hm):
        return int(G.mesh_guides(rt, O, hm, mats, [], cam, nx, ny)["nodes"].astype(np.int64).sum())

    built = visits(rt.HostMesh.build(tris, 5))
    hm = R.scrambled(rt.HostMesh.build(tris, 5))
    bad = visits(hm)
    hm.rebuild()
    good = visits(hm)
    print(f"node visits: built {built}, scrambled {bad}, rebuilt {good}, rebuilt / built {good / built:.4f}")
    assert good < bad
    assert good <= 1.25 * built
