"""CPU: the scene edits' host side (include/rt_api.h "editing the scene", include/rt_host.h).  rtRefitBvh on the builder's own output reproduces every node and
the bounds bit for bit; an independent numpy restatement of the definition agrees with it on jittered triangles, on leaves with a sentinel in front of a real
triangle and on a mesh of signed zeros; rtRefitBvhArrays refuses what initRenderer refuses; the Python wrappers refuse a wrong dtype or shape before the
library is called; the calls exit 99 before init; the refit kernels are one object built without FMA contraction.  Every comparison is np.array_equal on the
raw 32-bit words."""
import os
import re

import numpy as np
import pytest

import guides_reference as G
import scene_update_support as S
from preview_support import bits, exits_99

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["updateTriangles", "updateMaterials", "updateSpheres", "getMeshBvh", "rtLastUpdateMs"]


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _refit_reproduces(rt, hm, what):
    nodes, bounds = hm.bvh.copy(), S.view_bounds(hm)
    hm.bvh[1:] = np.zeros(1, rt.bvh_node_dtype)                 # what the refit must rebuild
    hm.refit()
    diff = int((_words(hm.bvh[1:]) != _words(nodes[1:])).sum())
    print(f"{what}: {len(nodes)} nodes, {diff} words differ")
    assert np.array_equal(_words(hm.bvh[1:]), _words(nodes[1:])), what
    assert np.array_equal(_words(hm.bvh[:1]), _words(nodes[:1])), what + ": node 0 was written"
    assert np.array_equal(bits(S.view_bounds(hm)), bits(bounds)), what


@pytest.mark.parametrize("nppl", [1, 3, 5])
@pytest.mark.parametrize("extra", [0, 1, 2])
def test_refit_reproduces_the_builder_staircase(rt, nppl, extra):
    tris, _ = rt.scene_staircase_procedural(1)
    _refit_reproduces(rt, rt.HostMesh.build(tris, nppl, extra_levels=extra), f"staircase detail 1, nppl {nppl}, extra levels {extra}")


def test_refit_reproduces_the_builder_tris300(rt, O, tmp_path):
    _refit_reproduces(rt, S.fresh_copy(rt, G.mesh_frame(rt, O, "tris300")["hm"], tmp_path), "tris300, nppl 5")


def _against_numpy(rt, hm, what):
    want_nodes, want_bounds = S.numpy_refit(hm.tris, hm.bvh, hm.nppl)
    hm.refit()
    assert np.array_equal(_words(hm.bvh), _words(want_nodes)), what
    assert np.array_equal(bits(S.view_bounds(hm)), bits(want_bounds)), what
    return want_nodes


def test_numpy_refit_agrees_jittered(rt, O, tmp_path):
    hm = S.fresh_copy(rt, G.mesh_frame(rt, O, "tris300")["hm"], tmp_path)
    before = hm.bvh.copy()
    hm.tris[:] = S.jitter(hm.tris, 21)
    after = _against_numpy(rt, hm, "tris300 jittered")
    assert (_words(after[1:]) != _words(before[1:])).mean() > 0.5           # the jitter moved most boxes


def test_numpy_refit_agrees_sentinel_before_real(rt):
    hm = S.sentinel_first_mesh(rt)
    t = hm.tris
    real = S.is_real(t).reshape(-1, hm.nppl)
    hidden = np.flatnonzero(~real[:, 0] & real[:, 1])
    assert len(hidden) >= 4
    nodes = _against_numpy(rt, hm, "sentinel before a real triangle")
    first_leaf = len(nodes) // 2
    assert np.all(np.isinf(nodes["a"][first_leaf + hidden])) and np.all(nodes["a"][first_leaf + hidden] > 0)      # those leaves are empty: (+inf, -inf)
    assert np.all(nodes["b"][first_leaf + hidden] < 0)


def test_numpy_refit_agrees_signed_zeros(rt):
    hm = rt.HostMesh.build(S.zero_tris(rt), 5)
    nodes = _against_numpy(rt, hm, "signed zeros")
    first_leaf = len(nodes) // 2
    lo, hi = _words(nodes["a"][first_leaf:]), _words(nodes["b"][first_leaf:])
    for w, name in ((lo, "lo"), (hi, "hi")):
        assert (w == 0x00000000).any() and (w == 0x80000000).any(), f"no leaf box keeps both signs of zero in {name}"
    flipped = hm.tris.copy()
    flipped["v"] = flipped["v"][:, ::-1, :]                                 # the other vertex order: other zeros are met first
    hm.tris[:] = flipped
    nodes2 = _against_numpy(rt, hm, "signed zeros, vertices reversed")
    assert not np.array_equal(_words(nodes2), _words(nodes))
    assert np.array_equal(nodes2["a"][1:], nodes["a"][1:]) and np.array_equal(nodes2["b"][1:], nodes["b"][1:])     # equal as numbers, not as bits


def test_numpy_refit_agrees_extremes(rt):
    """The (128, 5) blob with twenty triangles that carry a NaN coordinate, twenty scaled by 1e37 and twenty by 1e-44 (scene_update_support.extremes): the
    twin and the restatement agree bit for bit, no box holds a NaN, the large triangles reach the root's box and denormal bounds appear in the leaves."""
    hm = S.blob_mesh(rt, 128, 5)
    before = hm.bvh.copy()
    new, (nan, big, small) = S.extremes(hm.tris)
    hm.tris[:] = new
    nodes = _against_numpy(rt, hm, "extremes")
    assert not np.isnan(nodes["a"][1:]).any() and not np.isnan(nodes["b"][1:]).any()
    assert np.abs(nodes["a"][1]).max() > 1e37 and np.abs(nodes["b"][1]).max() > 1e37
    first_leaf = len(nodes) // 2
    tiny = np.finfo(np.float32).tiny
    leaf = np.concatenate([nodes["a"][first_leaf:], nodes["b"][first_leaf:]]).reshape(-1)
    assert ((leaf != 0) & (np.abs(leaf) < tiny)).sum() >= 10
    # a leaf that holds a NaN triangle: its box is the box of all its other coordinates, as numbers
    for leaf in np.unique(nan // hm.nppl):
        t = hm.tris[leaf * hm.nppl:(leaf + 1) * hm.nppl]
        v = t["v"][S.is_real(t)].reshape(-1, 3)
        assert np.isnan(v).any()
        assert np.array_equal(nodes["a"][first_leaf + leaf], np.nanmin(v, axis=0)) and np.array_equal(nodes["b"][first_leaf + leaf], np.nanmax(v, axis=0)), leaf
    assert (_words(nodes[1:]) != _words(before[1:])).any()


def test_refit_arrays_refuses_bad_arrays(rt):
    hm = S.blob_mesh(rt, 8, 3)
    tris, bvh = hm.tris.copy(), hm.bvh.copy()
    keep = bvh.copy()
    assert rt.refit_bvh_arrays(tris, bvh, 3) is not None
    assert np.array_equal(_words(bvh), _words(keep))
    for what, args in (("odd numBvhNodes", (tris, bvh[:15].copy(), 3)), ("numBvhNodes below 4", (tris, bvh[:2].copy(), 3)),
                       ("first_leaf * nppl > numTris", (tris[:23].copy(), bvh.copy(), 3)), ("nppl 0", (tris, bvh.copy(), 0))):
        before = args[1].copy()
        assert rt.refit_bvh_arrays(*args) is None, what
        assert np.array_equal(_words(args[1]), _words(before)), what + ": nodes were written"
    h = rt.load_host()
    assert h.rtRefitBvhArrays(None, 24, bvh.ctypes.data, 16, 3, None) == -1 and h.rtRefitBvhArrays(tris.ctypes.data, 24, None, 16, 3, None) == -1
    assert h.rtRefitBvh(None) == -1
    assert h.rtRefitBvhArrays(tris.ctypes.data, 24, bvh.ctypes.data, 16, 3, None) == 0          # bounds may be NULL


def test_symbols_are_declared_and_bound(rt):
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    lib = rt.load_renderer()
    for name in NEW:
        assert name in rt.RENDERER_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\(" % name, hdr), name
    assert "Geometry that moves between calls is not followed" not in hdr
    assert re.search(r"#define RT_API_VERSION 1002\b", hdr)                 # additive: no struct changed
    for name in ("rtRefitBvhArrays", "rtRefitBvh"):
        assert name in rt.HOST_SYMBOLS and hasattr(rt.load_host(), name)


def test_wrappers_refuse_wrong_arrays_before_calling(rt, monkeypatch):
    """No renderer is initialised here: a call that reached the library would end the process with exit status 99."""
    monkeypatch.setattr(rt, "load_renderer", lambda: pytest.fail("the library was called"))
    tris = np.zeros(4, rt.triangle_dtype)
    mats = np.zeros(4, rt.material_dtype)
    sph = np.zeros(4, rt.sphere_dtype)
    for bad in (tris.view(np.uint8), np.zeros((4, 16), np.float32), tris.reshape(2, 2), list(tris), None, mats):
        with pytest.raises(ValueError):
            rt.update_triangles(0, bad)
    for first in (0.0, "0", None, True):
        with pytest.raises(ValueError):
            rt.update_triangles(first, tris)
    for bad in (mats.view(np.uint8), mats.reshape(2, 2), np.zeros((4, 6), np.float32), tris, None):
        with pytest.raises(ValueError):
            rt.update_materials(bad)
        with pytest.raises(ValueError):
            rt.update_spheres(sph, bad)
    for bad in (sph.view(np.float32), sph.reshape(4, 1), mats, None):
        with pytest.raises(ValueError):
            rt.update_spheres(bad, mats)
    with pytest.raises(ValueError):
        rt.update_spheres(sph, mats[:3])
    with pytest.raises(ValueError):
        rt.refit_bvh_arrays(tris, np.zeros(8, np.float32), 1)


@pytest.mark.parametrize("call", ["rt.update_triangles(0, np.zeros(1, rt.triangle_dtype))", "rt.update_triangles(0, np.zeros(0, rt.triangle_dtype))",
                                  "rt.update_materials(np.zeros(1, rt.material_dtype))",
                                  "rt.update_spheres(np.zeros(1, rt.sphere_dtype), np.zeros(1, rt.material_dtype))", "rt.mesh_bvh()", "rt.last_update_ms()"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99(call + "\n")


def test_translation_unit():
    """The refit kernels are one object of their own, built like the other bit-defined passes (no FMA contraction) and linked into the library; the render
    kernels' sources and headers do not know its header."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    rules = re.findall(r"^\$\(OBJ\)/(\S+)\.o:\s*\$\(CSRC\)/rt_kernels_update\.hip([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert len(rules) == 1 and rules[0][0] == "update", rules
    assert "$(CSRC)/rt_update.h" in rules[0][1].split()
    display = re.search(r"^\$\(OBJ\)/display\.o:[^\n]*\n\t([^\n]+)", mk, re.M).group(1)
    assert rules[0][2].split() == display.split() and "-ffp-contract=off" in rules[0][2].split()
    link = re.search(r"^\$\(PKG\)/librt_mi355x\.so:([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert "$(UPDATE_OBJS)" in link.group(1).split() and "$(UPDATE_OBJS)" in link.group(2).split()
    assert re.search(r"^UPDATE_OBJS\s*:=\s*\$\(OBJ\)/update\.o\s*$", mk, re.M)
    csrc = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")
    for name in os.listdir(csrc):
        if name not in ("rt_renderer.hip", "rt_kernels_update.hip", "rt_update.h"):
            assert "rt_update.h" not in open(os.path.join(csrc, name)).read(), name
    kernel = open(os.path.join(csrc, "rt_kernels_update.hip")).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", kernel)                  # nothing is shared between workgroups of a launch
