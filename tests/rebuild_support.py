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


def numpy_rebuild(rt, tris, num_nodes, nppl):
    """(new tris, old_slot, nodes, bounds) of the rebuild of the leaf-ordered `tris` in a tree of num_nodes nodes."""
    first_leaf = num_nodes // 2
    slots = first_leaf * nppl
    src = visible_slots(tris, first_leaf, nppl)
    n = len(src)
    v = tris["v"][src].astype(F)
    lo, hi = v.min(axis=1), v.max(axis=1)
    cent = (F(0.5) * (lo + hi)).astype(F)
    ids = np.arange(n)
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
