"""What the tests of the scene edits (updateTriangles / updateMaterials / updateSpheres, include/rt_api.h) share.  No test: a plain module, imported by
tests/test_scene_update_api.py (CPU) and tests/test_gpu_scene_update.py (GPU).

The named frames of guides_reference are cached and shared by other tests, so nothing here edits one: fresh_copy() makes an independent HostMesh with the
same triangles and nodes (through a BVH file), and the small meshes below are built anew by every call."""
import os

import numpy as np

import guides_reference as G

INF = np.float32(np.inf)


def fresh_copy(rt, hm, tmp_path):
    """An independent HostMesh equal to `hm`, slot for slot and node for node (rtSaveBvhFile + rtLoadBvhFile)."""
    path = os.path.join(str(tmp_path), "copy_%d.bvh" % len(os.listdir(str(tmp_path))))
    assert hm.save(path) == 0
    return rt.HostMesh.load(path)


def is_real(tris):
    return ~np.isinf(tris["v"][:, 0, 0])


def jitter(tris, seed, amount=3.0):
    """A copy of `tris` with every vertex of every real triangle moved by a seeded uniform offset in [-amount, amount) per coordinate."""
    rng = np.random.default_rng(seed)
    out = tris.copy()
    real = is_real(tris)
    out["v"][real] = out["v"][real] + rng.uniform(-amount, amount, (int(real.sum()), 3, 3)).astype(np.float32)
    return out


def extremes(tris, seed=61):
    """A copy of `tris` in which 60 real triangles, chosen by seed, sit at the edges of what updateTriangles takes: twenty with one coordinate a NaN (the boxes
    ignore it; a NaN is no infinity, so no slot's sentinel state changes), twenty scaled by 1e37 (finite, near FLT_MAX) and twenty by 1e-44 (denormals of a few
    units in the last place, zeros among them).  Returns (copy, the three index arrays)."""
    rng = np.random.default_rng(seed)
    out = tris.copy()
    pick = rng.permutation(np.flatnonzero(is_real(tris)))[:60]
    nan, big, small = pick[:20], pick[20:40], pick[40:]
    out["v"].reshape(len(out), 9)[nan, rng.integers(0, 9, 20)] = np.nan
    out["v"][big] = (out["v"][big].astype(np.float64) * 1e37).astype(np.float32)
    out["v"][small] = (out["v"][small].astype(np.float64) * 1e-44).astype(np.float32)
    assert np.array_equal(is_real(out), is_real(tris)) and np.isfinite(out["v"][big]).all() and int(np.isnan(out["v"]).sum()) == 20
    return out, (nan, big, small)


def blob_tris(rt, n, seed, mats=4):
    """n small seeded triangles scattered in a cube of side 20."""
    rng = np.random.default_rng(seed)
    tris = np.zeros(n, rt.triangle_dtype)
    tris["v"] = (rng.uniform(-10, 10, (n, 1, 3)) + rng.uniform(-1.5, 1.5, (n, 3, 3))).astype(np.float32)
    tris["texCoords"] = rng.uniform(-2, 2, (n, 6)).astype(np.float32)
    tris["meshID"] = rng.integers(0, mats, n)
    return tris


def blob_mesh(rt, first_leaf, nppl, seed=3):
    """A fresh mesh with exactly `first_leaf` leaves (a power of two, at least 2) of nppl slots, two thirds of them real."""
    assert first_leaf >= 2 and first_leaf & (first_leaf - 1) == 0
    n = max(2, -(-first_leaf * nppl * 2 // 3))                  # more than half the slots: the smallest complete tree that holds them has first_leaf leaves
    hm = rt.HostMesh.build(blob_tris(rt, n, seed), nppl, extra_levels=0)
    assert hm.view.numBvhNodes // 2 == first_leaf, (hm.view.numBvhNodes, first_leaf)
    return hm


def zero_tris(rt, n=96, seed=13):
    """Triangles whose coordinates are +0.0, -0.0 and one other value: on every axis the smallest (first half) or the largest (second half) coordinate of a
    leaf is a zero, and which sign a box keeps depends on the order its slots and vertices are visited in."""
    rng = np.random.default_rng(seed)
    tris = np.zeros(n, rt.triangle_dtype)
    pos = np.array([0.0, -0.0, 1.0], np.float32)
    neg = np.array([0.0, -0.0, -1.0], np.float32)
    v = np.where((np.arange(n) < n // 2)[:, None, None], pos[rng.integers(0, 3, (n, 3, 3))], neg[rng.integers(0, 3, (n, 3, 3))])
    tris["v"] = v
    tris["meshID"] = rng.integers(0, 4, n)
    return tris


def sentinel_first_mesh(rt, seed=5):
    """A fresh mesh (nppl 3) in which every fourth leaf with two real triangles has had its slot 0 turned into a sentinel: a sentinel followed by a real
    triangle, which the leaf loop - and the refit - never reach.  The renderer builds no compact leaf records for such a mesh."""
    hm = rt.HostMesh.build(blob_tris(rt, 200, seed), 3)
    t = hm.tris
    real = is_real(t).reshape(-1, 3)
    leaves = np.flatnonzero(real[:, 0] & real[:, 1])[::4]
    assert len(leaves) >= 4
    t["v"][leaves * 3] = INF
    hm.refit()
    return hm


def numpy_refit(tris, nodes, nppl):
    """The refit of include/rt_api.h restated with numpy selects (np.where keeps the bits of the operand it takes): returns (nodes, bounds) for the leaf-ordered
    `tris`; node 0 is copied from `nodes`."""
    count = len(nodes)
    first_leaf = count // 2
    v = tris["v"][:first_leaf * nppl].reshape(first_leaf, nppl, 3, 3)
    lo = np.full((count, 3), np.inf, np.float32)
    hi = np.full((count, 3), -np.inf, np.float32)
    alive = np.ones(first_leaf, bool)
    llo, lhi = lo[first_leaf:], hi[first_leaf:]
    for k in range(nppl):
        alive &= ~np.isinf(v[:, k, 0, 0])
        for vert in range(3):
            p = v[:, k, vert, :]
            llo[...] = np.where(alive[:, None] & (p < llo), p, llo)
            lhi[...] = np.where(alive[:, None] & (p > lhi), p, lhi)
    w = first_leaf // 2
    while w >= 1:
        i = np.arange(w, 2 * w)
        lo[i] = np.where(lo[2 * i + 1] < lo[2 * i], lo[2 * i + 1], lo[2 * i])
        hi[i] = np.where(hi[2 * i + 1] > hi[2 * i], hi[2 * i + 1], hi[2 * i])
        w //= 2
    out = nodes.copy()
    out["a"][1:] = lo[1:]
    out["b"][1:] = hi[1:]
    return out, np.stack([lo[1], hi[1]])


def view_bounds(hm):
    b = hm.view.bounds
    return np.array([list(b.min.e), list(b.max.e)], np.float32)

