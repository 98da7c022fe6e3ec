"""The UV-atlas raster of rasterTexels / bakeTexels (include/rt_api.h, "baking texels") and the atlas of rtAtlasGrid (include/rt_host.h), restated in numpy
float32: one triangle at a time over the whole atlas, every operation one rounding, operands in the order the header writes them.  No test: a plain module,
imported by tests/test_texels_api.py and tests/test_gpu_texels.py, with the atlases both files use.  Nothing here calls the library."""
import functools

import numpy as np

F = np.float32
PRIM_NONE = -1
MAX_SIZE, MAX_DILATE = 8192, 16
TRIANGLE = np.dtype([("v", np.float32, (3, 3)), ("texCoords", np.float32, 6), ("meshID", np.uint8), ("_pad", np.uint8, 3)])


def samples(W, H):
    """(sx (H, W), sy (H, W)): the sample point of every texel."""
    sx = (np.arange(W).astype(F) + F(0.5)) / F(W)
    sy = (np.arange(H).astype(F) + F(0.5)) / F(H)
    return np.broadcast_to(sx[None, :], (H, W)), np.broadcast_to(sy[:, None], (H, W))


def _bound(a, b, c, smaller):
    m = a
    for v in (b, c):
        if (v < m) if smaller else (v > m):
            m = v
    return m


def cover(tc, sx, sy):
    """(covered (H, W) bool, hu, hv, w0) of one UV triangle over the whole atlas; hu, hv, w0 are meaningful where the box test passed and d != 0."""
    ax, ay, bx, by, cx, cy = (F(v) for v in tc)
    with np.errstate(all="ignore"):
        umin, umax = _bound(ax, bx, cx, True), _bound(ax, bx, cx, False)
        vmin, vmax = _bound(ay, by, cy, True), _bound(ay, by, cy, False)
        box = (umin <= sx) & (sx <= umax) & (vmin <= sy) & (sy <= vmax)
        d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        w1 = (sx - ax) * (cy - ay) - (sy - ay) * (cx - ax)
        w2 = (bx - ax) * (sy - ay) - (by - ay) * (sx - ax)
        hu, hv = w1 / d, w2 / d
        w0 = F(1) - hu - hv
        inside = (hu >= 0) & (hv >= 0) & (w0 >= 0)
        return box & inside & bool(d != 0), hu, hv, w0


def resolve(tri, hu, hv):
    """(pos (..., 3), nrm (3,)) of the triangle at the weights hu, hv."""
    v0, v1, v2 = (tri["v"][i].astype(F) for i in range(3))
    e1, e2 = v1 - v0, v2 - v0
    with np.errstate(all="ignore"):
        pos = np.stack([v0[k] + hu * e1[k] + hv * e2[k] for k in range(3)], axis=-1)
        c = np.array([e1[1] * e2[2] - e1[2] * e2[1], -(e1[0] * e2[2] - e1[2] * e2[0]), e1[0] * e2[1] - e1[1] * e2[0]], F)
        l = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
        return pos.astype(F), (c / l).astype(F)


def dilate_once(cur):
    H, W = cur.shape
    new = cur.copy()
    pad = np.full((H + 2, W + 2), -1, np.int32)
    pad[1:-1, 1:-1] = cur
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            q = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            take = (new == -1) & (q != -1)
            new[take] = q[take]
    return new


def raster(tris, W, H, dilate=0, slots=None):
    """The planes of the definition: dict(prim, src, bary, pos, nrm, owned) plus what the tests assert on the inputs - covers (H, W): covering slots per
    texel, on_edge (H, W): the owner's hu, hv or w0 is exactly 0.  `slots`: the ascending slots to evaluate, where the caller has parked every other one
    (keep_slots; checked here) - a parked slot covers nothing, and evaluating it over a large atlas only costs time."""
    sx, sy = samples(W, H)
    prim = np.full((H, W), PRIM_NONE, np.int32)
    bary, pos, nrm = np.zeros((H, W, 2), F), np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
    covers, on_edge = np.zeros((H, W), np.int32), np.zeros((H, W), bool)
    if slots is not None:
        slots = np.asarray(slots)
        rest = np.ones(len(tris), bool)
        rest[slots] = False
        assert (np.diff(slots) > 0).all() and (tris["texCoords"][rest] == np.asarray(PARKED, F)).all()
    for k in (range(len(tris)) if slots is None else slots.tolist()):
        if np.isinf(tris[k]["v"][0, 0]):
            continue
        cov, hu, hv, w0 = cover(tris[k]["texCoords"], sx, sy)
        if not cov.any():
            continue
        covers += cov
        new = cov & (prim == PRIM_NONE)
        prim[new] = k
        bary[new] = np.stack([hu, hv], axis=-1)[new]
        on_edge[new] = ((hu == 0) | (hv == 0) | (w0 == 0))[new]
        p, n = resolve(tris[k], hu, hv)
        pos[new] = p[new]
        nrm[new] = n
    t = np.arange(W * H, dtype=np.int32).reshape(H, W)
    src = np.where(prim != PRIM_NONE, t, np.int32(-1)).astype(np.int32)
    for _ in range(dilate):
        src = dilate_once(src)
    return dict(prim=prim, src=src, bary=bary, pos=pos, nrm=nrm, owned=int((prim != PRIM_NONE).sum()), covers=covers, on_edge=on_edge)


def fill_iterations(tris, W, H):
    """The first iteration count after which dilation changes nothing (every texel filled, or none owned), and the plane it leaves."""
    src = raster(tris, W, H)["src"]
    for i in range(W + H + 1):
        nxt = dilate_once(src)
        if np.array_equal(nxt, src):
            return i, src
        src = nxt
    raise AssertionError("dilation does not settle")


def atlas_grid(tris, margin):
    """rtAtlasGrid on a copy: (tris with the new texCoords, cells)."""
    out = tris.copy()
    n = len(tris)
    pairs = (n + 1) // 2
    cells = 1
    while cells * cells < pairs:
        cells += 1
    cs = F(1) / F(cells)
    m = F(margin) * cs
    m3 = F(3) * m
    for i in range(n):
        q = i // 2
        u0, v0 = F(q % cells) * cs, F(q // cells) * cs
        u1, v1 = u0 + cs, v0 + cs
        out["texCoords"][i] = ([u0 + m, v0 + m, u1 - m3, v0 + m, u0 + m, v1 - m3] if i % 2 == 0 else
                               [u1 - m, v1 - m, u0 + m3, v1 - m, u1 - m, v0 + m3])
    return out, cells


# ---- the atlases of the tests: UVs for the first slots of a triangle array, every other slot parked where it covers nothing ----------------------------

PARKED = (5.0, 5.0, 5.0, 5.0, 5.0, 5.0)         # d == 0, and outside the atlas


def random_triangles(n, seed=1):
    """n triangles with random vertices (the raster reads them for pos and nrm only) and parked UVs."""
    rng = np.random.default_rng(seed)
    tris = np.zeros(n, TRIANGLE)
    tris["v"] = rng.uniform(-4, 4, (n, 3, 3)).astype(F)
    tris["texCoords"] = PARKED
    return tris


def _place(tris, uvs, order=None):
    """A copy of tris with uvs[i] in the i-th slot that is no sentinel (so that the same atlas lands on a leaf-ordered array with padding) and every other
    slot parked."""
    out = tris.copy()
    out["texCoords"] = PARKED
    live = np.flatnonzero(~np.isinf(out["v"][:, 0, 0]))
    assert len(live) >= len(uvs), (len(live), len(uvs))
    out["texCoords"][live[:len(uvs)]] = np.asarray(uvs, F)
    return out


def live_slots(tris):
    """The slots that are no sentinel, ascending."""
    return np.flatnonzero(~np.isinf(tris["v"][:, 0, 0]))


def keep_slots(tris, slots):
    """A copy of tris with every slot but `slots` parked: the atlas of `slots` alone, which raster(..., slots=slots) evaluates in len(slots) steps."""
    out = tris.copy()
    out["texCoords"] = PARKED
    out["texCoords"][slots] = tris["texCoords"][slots]
    return out


def atlas_exact(tris):
    """(a): 16 x 16 with UV vertices on multiples of 1/32 - every texel centre (2x+1)/32 is exactly representable, and edges and vertices pass through
    centres: two right triangles that share the diagonal of [1/32, 17/32]^2 (the diagonal's centres are covered by both), one triangle on top of the first
    (whole overlap, the lower slot wins), one with a vertex exactly on a centre elsewhere; the upper right of the atlas stays empty."""
    u = lambda *k: [v / 32.0 for v in k]
    uvs = [u(1, 1, 17, 1, 1, 17), u(17, 17, 1, 17, 17, 1), u(3, 3, 9, 3, 3, 9), u(21, 5, 27, 5, 21, 11), u(5, 21, 5, 27, 11, 21)]
    return _place(tris, uvs), 16, 16


def atlas_odd(tris, seed=3):
    """(b): 37 x 23 with 60 random triangles with UVs in (-0.5, 1.5), and among them one with d == 0, one with a NaN UV, one smaller than a texel that
    covers no centre and (by the caller's array, or slot 7 here) one sentinel slot."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.5, 1.5, (60, 1, 2))
    uvs = np.clip(c + rng.uniform(-0.25, 0.25, (60, 3, 2)), -0.499, 1.499).reshape(60, 6).astype(F)
    uvs[11] = [0.2, 0.2, 0.4, 0.4, 0.6, 0.6]                    # collinear: d == 0
    uvs[23] = [0.3, np.nan, 0.7, 0.2, 0.5, 0.8]                 # a NaN UV
    x, y = (5 + 0.05) / 37, (4 + 0.05) / 23                     # inside texel (5, 4), left of and below its centre
    uvs[37] = [x, y, x + 0.3 / 37, y, x, y + 0.3 / 23]
    out = tris.copy()
    if not np.isinf(out["v"][:, 0, 0]).any():
        out["v"][7] = np.inf                                    # a sentinel slot
    return _place(out, uvs), 37, 23


def atlas_small(tris, W, H):
    """(c): one triangle over the lower left, one over the upper part: 1 x 1 and 1 x 5."""
    return _place(tris, [[-0.1, -0.1, 1.2, -0.1, -0.1, 1.2], [0.0, 0.65, 1.0, 0.65, 0.5, 1.1]]), W, H


def atlas_overlapping(tris, seed=9):
    """Random overlapping UVs on every live slot (uploaded through updateTriangles after init in the GPU tests)."""
    rng = np.random.default_rng(seed)
    live = np.flatnonzero(~np.isinf(tris["v"][:, 0, 0]))
    c = rng.uniform(0, 1, (len(live), 1, 2))
    return _place(tris, (c + rng.uniform(-0.2, 0.2, (len(live), 3, 2))).reshape(-1, 6).astype(F))
