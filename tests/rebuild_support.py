"""What the tests of rebuildBvh (include/rt_api.h, "editing the scene") share.  No test: a plain module, imported by tests/test_rebuild_api.py (CPU) and
tests/test_gpu_rebuild.py (GPU).

numpy_rebuild restates the definition independently of host/rt_bvh.cpp and level by level, as the device builds: three lists sorted once by
(cent[axis], i), per level the costs of every (axis, cut) of every node computed on their own, the first minimum in (axis, cut) order, a stable partition of
all three lists.  Every float operation is a float32 numpy operation, one rounding each."""
import numpy as np

import scene_update_support as S

F = np.float32


def visible_slots(tris, first_leaf, nppl):
    """The slots the traversal can see, in slot order: within a leaf everything before its first sentinel."""
    real = S.is_real(tris[:first_leaf * nppl]).reshape(first_leaf, nppl)
    return np.flatnonzero(np.logical_and.accumulate(real, axis=1).reshape(-1))


def sentinels(rt, n):
    t = np.zeros(n, rt.triangle_dtype)
    t["v"] = np.inf
    return t


def _area(lo, hi):
    """area(box) of the definition for arrays of boxes (k, 3)."""
    d = hi - lo
    a = F(2.0) * ((d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2]) + d[:, 2] * d[:, 0])
    return np.where(hi[:, 0] < lo[:, 0], F(0.0), a).astype(F)


COUNTS = ("winner", "no_winner", "mixed_nodes", "inf_costs", "nan_costs", "nonzero_costs", "inf_centroids", "denormal_centroids_pos", "denormal_centroids_neg")


def numpy_rebuild(rt, tris, num_nodes, nppl, counts=None):
    """(new tris, old_slot, nodes, bounds) of the rebuild of the leaf-ordered `tris` in a tree of num_nodes nodes.  counts: a dict that receives, for this
    rebuild, the nodes with m > 1 that have a winner and those that have none, the nodes that hold finite and +inf costs together, the +inf, NaN and non-zero
    costs seen, the infinite centroid coordinates and the denormal ones of either sign (COUNTS)."""
    first_leaf = num_nodes // 2
    slots = first_leaf * nppl
    src = visible_slots(tris, first_leaf, nppl)
    n = len(src)
    v = tris["v"][src].astype(F)
    lo, hi = v.min(axis=1), v.max(axis=1)
    with np.errstate(over="ignore"):
        cent = (F(0.5) * (lo + hi)).astype(F)
    ids = np.arange(n)
    if counts is not None:
        counts.update(dict.fromkeys(COUNTS, 0))
        tiny = np.finfo(F).tiny
        counts["inf_centroids"] = int(np.isinf(cent).sum())
        counts["denormal_centroids_pos"] = int(((cent > 0) & (cent < tiny)).sum())
        counts["denormal_centroids_neg"] = int(((cent < 0) & (cent > -tiny)).sum())
    order = [np.lexsort((ids, cent[:, a])) for a in range(3)]          # by (cent[axis], i): -0.0 == 0.0 in the comparison
    beg, end = {1: 0}, {1: n}
    waxis = {}
    leaves = first_leaf
    level = [1]
    with np.errstate(over="ignore", invalid="ignore"):
        while leaves > 1:
            cap_half = (leaves // 2) * nppl
            nxt = []
            for idx in level:
                b, e = beg[idx], end[idx]
                m = e - b
                nl, axis = 0, 0
                if m > 0:
                    lo_cut = max(m - cap_half, 1 if m > 1 else 0)
                    hi_cut = min(cap_half, m - 1 if m > 1 else m)
                    cuts = np.arange(max(lo_cut, 1), hi_cut + 1)
                    costs = []
                    for a in range(3):
                        seg = order[a][b:e]
                        left = _area(np.minimum.accumulate(lo[seg]), np.maximum.accumulate(hi[seg]))                    # [c - 1]: the first c
                        right = _area(np.minimum.accumulate(lo[seg][::-1])[::-1], np.maximum.accumulate(hi[seg][::-1])[::-1])   # [c]: from c on
                        right = np.append(right, F(0.0))
                        costs.append((left[cuts - 1] * cuts.astype(F) + right[cuts] * (m - cuts).astype(F)).astype(F))
                    flat = np.concatenate(costs)
                    if counts is not None and m > 1:
                        finite = flat < F(np.inf)
                        counts["winner" if finite.any() else "no_winner"] += 1
                        counts["mixed_nodes"] += int(finite.any() and bool(np.isposinf(flat).any()))
                        counts["inf_costs"] += int(np.isposinf(flat).sum())
                        counts["nan_costs"] += int(np.isnan(flat).sum())
                        counts["nonzero_costs"] += int((flat != 0).sum())
                    flat = np.where(flat < F(np.inf), flat, F(np.inf))          # a NaN never wins
                    cut = (m + 1) // 2
                    if len(flat) and flat.min() < F(np.inf):
                        k = int(np.argmin(flat))                                # the first of equal minima, axis-major
                        axis, cut = k // len(cuts), int(cuts[k % len(cuts)])
                    nl = min(max(cut, lo_cut), hi_cut)
                    to_left = np.zeros(n, bool)
                    to_left[order[axis][b:b + nl]] = True
                    for a in range(3):
                        seg = order[a][b:e]
                        order[a][b:e] = np.concatenate([seg[to_left[seg]], seg[~to_left[seg]]])
                waxis[idx] = axis
                beg[2 * idx], end[2 * idx], beg[2 * idx + 1], end[2 * idx + 1] = b, b + nl, b + nl, e
                nxt += [2 * idx, 2 * idx + 1]
            level = [i for i in nxt if end[i] > beg[i]]                         # (an empty node has empty children: nothing to decide below it)
            leaves //= 2
    out = tris.copy()
    out[:slots] = sentinels(rt, slots)
    old_slot = np.arange(len(tris), dtype=np.int32)
    old_slot[:slots] = -1
    for leaf in level:
        got = order[waxis[leaf // 2]][beg[leaf]:end[leaf]]
        assert len(got) <= nppl
        at = (leaf - first_leaf) * nppl + np.arange(len(got))
        out[at] = tris[src[got]]
        old_slot[at] = src[got]
    nodes, bounds = S.numpy_refit(out, np.zeros(num_nodes, rt.bvh_node_dtype), nppl)
    return out, old_slot, nodes, bounds


def quantised_tris(rt, n, seed=17):
    """Coordinates in multiples of 0.5 from -1.5 to 1.5 with zeros of both signs: many equal centroids, equal costs and degenerate boxes."""
    rng = np.random.default_rng(seed)
    tris = np.zeros(n, rt.triangle_dtype)
    v = (rng.integers(-3, 4, (n, 3, 3)) * 0.5).astype(F)
    v = np.where((v == 0) & (rng.integers(0, 2, (n, 3, 3)) == 1), F(-0.0), v)
    tris["v"] = v
    tris["texCoords"] = rng.uniform(-2, 2, (n, 6)).astype(F)
    tris["meshID"] = rng.integers(0, 4, n)
    assert (v.view(np.uint32) == 0x80000000).any() and (v.view(np.uint32) == 0).any()
    return tris


def scaled_blob(rt, n, scale, every=None, seed=5):
    """S.blob_tris(rt, n, seed) with the vertices scaled in float64 and then rounded to float32; every = k: only each k-th triangle is scaled.  Scales near the
    ends of the float32 range: areas and costs that overflow to +inf, costs that underflow to 0, denormal coordinates and centroids."""
    tris = S.blob_tris(rt, n, seed)
    v = tris["v"].astype(np.float64)
    sel = slice(None) if every is None else slice(0, None, every)
    v[sel] *= scale
    tris["v"] = v.astype(F)
    assert np.isfinite(tris["v"]).all()
    return tris


# case -> (scale, every, flat).  What each is there for is asserted from numpy_rebuild's counts by tests/test_rebuild_api.py::test_twin_against_numpy (_claims).
# A single triangle scaled by 1e25 already has an infinite area, so a node that holds one has no finite cost at all: finite and +inf costs in one node need
# 1e18, where one scaled triangle's box is finite and two of them overflow.  At 1e37 every centroid is still finite (|lo + hi| < 2.4e38): 2e37 has infinite
# ones.  A NaN cost needs 0 * inf: boxes of zero width (every x equal) and infinite height.
EXTREMES = {"scale 3e18": (3e18, None, False), "scale 1e25": (1e25, None, False), "scale 1e37": (1e37, None, False), "scale 2e37": (2e37, None, False),
            "scale 1e25, every 7th": (1e25, 7, False), "scale 1e18, every 7th": (1e18, 7, False), "scale 1e-25": (1e-25, None, False),
            "scale 1e-38": (1e-38, None, False), "scale 1e-44": (1e-44, None, False), "flat in x, scale 2e37": (2e37, None, True)}


def extreme_mesh(rt, case):
    """The mesh of a case of EXTREMES: 200 scaled triangles (flat: every x coordinate 1.0), 3 slots per leaf, scrambled."""
    scale, every, flat = EXTREMES[case]
    tris = scaled_blob(rt, 200, scale, every)
    if flat:
        tris["v"][:, :, 0] = 1.0
    return scrambled(rt.HostMesh.build(tris, 3))


def scrambled(hm, seed=71):
    """The real triangles of `hm` permuted among the real slots (in place) and the tree refitted: a correct tree whose boxes overlap everywhere."""
    t = hm.tris
    real = np.flatnonzero(S.is_real(t))
    t[real] = t[real][np.random.default_rng(seed).permutation(len(real))]
    hm.refit()
    return hm


def check_old_slot(before, after, old_slot, first_leaf, nppl):
    """old_slot maps the new real slots one to one onto the old visible ones, moves whole triangles and names every other slot as the definition says."""
    slots = first_leaf * nppl
    vis = visible_slots(before, first_leaf, nppl)
    real = np.flatnonzero(old_slot[:slots] >= 0)
    assert np.array_equal(np.sort(old_slot[real]), vis)
    assert np.array_equal(real, visible_slots(after, first_leaf, nppl)) and np.array_equal(real, np.flatnonzero(S.is_real(after[:slots])))
    assert after[real].tobytes() == before[old_slot[real]].tobytes()
    assert np.array_equal(old_slot[slots:], np.arange(slots, len(before)))
    assert after[slots:].tobytes() == before[slots:].tobytes()
