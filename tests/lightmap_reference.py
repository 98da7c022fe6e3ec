"""The lookup of sampleTexels / renderLightmap (include/rt_api.h, "sampling texels") restated in numpy float32 on top of texels_reference: every operation
one ufunc - one rounding -, operands in the order the header writes them; and the frame renderLightmap owes, composed from renderGuides' albedo plane and
traceRays' planes over the centre rays.  No test: a plain module, imported by tests/test_lightmap_api.py and tests/test_gpu_lightmap.py, with the hit lists
and planes both files use.  Nothing here calls the library."""
import numpy as np

import texels_reference as TR

F = np.float32
IRRADIANCE, SH9, VISIBILITY = 0, 1, 2
WIDTH = {IRRADIANCE: 3, SH9: 27, VISIBILITY: 1}
MODE_OF = {3: IRRADIANCE, 27: SH9, 1: VISIBILITY}
BILINEAR, ALBEDO, FROM_BAKE, FROM_FILTER = 1, 2, 4, 8
PRIM_NONE, PRIM_FLOOR = -1, -2
SH_K = tuple(F(v) for v in (0.282095, 0.325735, 0.325735, 0.325735, 0.273137, 0.273137, 0.078848, 0.273137, 0.136568))


def valid_hits(tris, prim):
    prim = np.asarray(prim, np.int64)
    ok = (prim >= 0) & (prim < len(tris))
    x = tris["v"][np.where(ok, prim, 0), 0, 0]
    return ok & ~np.isinf(x)


def atlas_point(tc, hu, hv):
    """(tcu, tcv) of hits with texCoords tc (n, 6): mesh_texel's two lines."""
    w0 = F(1) - hu - hv
    tcu = hu * tc[:, 2] + hv * tc[:, 4] + w0 * tc[:, 0]
    tcv = hu * tc[:, 3] + hv * tc[:, 5] + w0 * tc[:, 1]
    return tcu, tcv


def nearest(c, n):
    f = c * F(n)
    f = np.where(f > 0, f, F(0))
    f = np.where(f < F(n - 1), f, F(n - 1))
    return f.astype(np.int32)


def linear(c, n):
    """(i0, i1, a, k): the two clamped columns, the weight of i1 and k = (int)floorf(fx) before the clamp (-1 .. n)."""
    f = c * F(n) - F(0.5)
    f = np.where(f > -1, f, F(-1))
    f = np.where(f < F(n), f, F(n))
    f0 = np.floor(f)
    a = f - f0
    k = f0.astype(np.int32)
    return np.clip(k, 0, n - 1), np.clip(k + 1, 0, n - 1), a, k


def sh9_value(c, nrm):
    """e (n, 3) of the coefficients c (n, 27) at the normals nrm (n, 3), before the clamp at 0."""
    X, Y, Z = nrm[:, 0:1], nrm[:, 1:2], nrm[:, 2:3]
    co = lambda i: c[:, 3 * i:3 * i + 3]
    k = SH_K
    e = (k[0] * co(0) + k[1] * (co(1) * Y) + k[2] * (co(2) * Z) + k[3] * (co(3) * X)
         + k[4] * (co(4) * (X * Y)) + k[5] * (co(5) * (Y * Z)) + k[6] * (co(6) * (F(3) * (Z * Z) - F(1)))
         + k[7] * (co(7) * (X * Z)) + k[8] * (co(8) * (X * X - Y * Y)))
    return e.astype(F)


def lookup(tris, prim, uv, normal, W, H, mode, planes, bilinear, details=None):
    """(out (n, 3) float32, valid (n,) uint8) of the definition.  `details`: a dict that receives what the tests assert on their inputs - per hit the atlas
    point, and for bilinear the unclamped tap columns / rows and the weights."""
    prim = np.asarray(prim, np.int32)
    uv = np.asarray(uv, F)
    C = WIDTH[mode]
    planes = np.asarray(planes, F).reshape(H * W, C)
    ok = valid_hits(tris, prim)
    tc = tris["texCoords"][np.where(ok, prim, 0)].astype(F)
    with np.errstate(all="ignore"):
        tcu, tcv = atlas_point(tc, uv[:, 0], uv[:, 1])
        if not bilinear:
            x, y = nearest(tcu, W), nearest(tcv, H)
            c = planes[y.astype(np.int64) * W + x]
            if details is not None:
                details.update(tcu=tcu, tcv=tcv, x=x, y=y)
        else:
            x0, x1, ax, kx = linear(tcu, W)
            y0, y1, ay, ky = linear(tcv, H)
            t = lambda yy, xx: planes[yy.astype(np.int64) * W + xx]
            w = lambda a: a[:, None]
            c = (w((F(1) - ax) * (F(1) - ay)) * t(y0, x0) + w(ax * (F(1) - ay)) * t(y0, x1) + w((F(1) - ax) * ay) * t(y1, x0) + w(ax * ay) * t(y1, x1))
            if details is not None:
                details.update(tcu=tcu, tcv=tcv, kx=kx, ky=ky, ax=ax, ay=ay)
        if mode == IRRADIANCE:
            e = c
        elif mode == VISIBILITY:
            e = np.repeat(c[:, :1], 3, axis=1)
        else:
            raw = sh9_value(c, np.asarray(normal, F))
            if details is not None:
                details.update(raw=raw)
            e = np.where(raw > 0, raw, F(0))
    out = np.where(ok[:, None], e, F(0)).astype(F)
    return out, ok.astype(np.uint8)


def compose(albedo, prim, uv, normal, tris, W, H, mode, planes, flags, floor_value=None):
    """The frame renderLightmap owes: albedo (ny, nx, 3) of renderGuides, prim (ny, nx), uv (ny, nx, 2) and normal (ny, nx, 3) of traceRays over the centre
    rays of every pixel, row 0 at the bottom."""
    ny, nx = prim.shape
    p = prim.reshape(-1)
    e, ok = lookup(tris, p, uv.reshape(-1, 2), normal.reshape(-1, 3), W, H, mode, planes, bool(flags & BILINEAR))
    assert ((p >= 0) == (ok == 1)).all()                                 # (a ray never reports a sentinel slot)
    fv = np.asarray((1, 1, 1) if floor_value is None else floor_value, F)
    L = np.where((p == PRIM_FLOOR)[:, None], fv[None, :], e).astype(F)
    A = albedo.reshape(-1, 3).astype(F)
    with np.errstate(all="ignore"):
        lit = (A * L).astype(F) if flags & ALBEDO else L
    return np.where((p == PRIM_NONE)[:, None], A, lit).astype(F).reshape(ny, nx, 3)


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------------------------------

def random_planes(W, H, C, seed):
    """Finite values of both signs (SH9 meets its clamp), seeded."""
    return np.random.default_rng(seed).uniform(-1, 1, (H, W, C)).astype(F)


def index_planes(W, H, C):
    """Every channel of texel t holds t."""
    return np.repeat(np.arange(W * H, dtype=F).reshape(H, W, 1), C, axis=2)


def with_dead_slot(tris):
    """(a copy of tris with at least one sentinel slot, the lowest such slot): where the array has none, the last slot becomes one."""
    out = tris.copy()
    dead = np.flatnonzero(np.isinf(out["v"][:, 0, 0]))
    if len(dead) == 0:
        out["v"][-1] = np.inf
        out["texCoords"][-1] = TR.PARKED
        dead = [len(out) - 1]
    return out, int(dead[0])


def edge_hits(tris, seed, random=200):
    """(prim, uv, normal) over `tris` (with a sentinel slot): seeded random hits inside and around the triangles whose UVs are not parked, then the synthetic
    edge list - barycentrics far outside [0, 1]^2 in the four directions, multiples of 1/8 (on the exact atlas: ax == 0), a NaN uv, prim NONE, FLOOR, past the
    array, and a sentinel slot."""
    rng = np.random.default_rng(seed)
    live = TR.live_slots(tris)
    placed = live[(tris["texCoords"][live] != np.asarray(TR.PARKED, F)).any(axis=1)]
    if len(placed) == 0:
        placed = live
    dead = int(np.flatnonzero(np.isinf(tris["v"][:, 0, 0]))[0])
    prim, uv = [], []
    p = placed[rng.integers(0, len(placed), random)]
    a, b = rng.uniform(0, 1, random), rng.uniform(0, 1, random)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    wide = rng.uniform(-1, 2, (random, 2))
    inside = rng.uniform(0, 1, random) < 0.7
    prim += p.tolist()
    uv += np.where(inside[:, None], np.stack([a, b], axis=1), wide).tolist()
    for s in placed[:4].tolist():
        for h in ((-40.0, 0.2), (40.0, 0.2), (0.2, -40.0), (0.2, 40.0), (-40.0, -40.0), (40.0, 40.0), (1e30, -1e30)):
            prim.append(s); uv.append(h)
        for i in range(9):
            for j in range(9 - i):
                prim.append(s); uv.append((i / 8.0, j / 8.0))
        for h in ((np.nan, 0.25), (0.25, np.nan), (np.nan, np.nan), (np.inf, 0.0), (0.0, -np.inf)):
            prim.append(s); uv.append(h)
    for s in (PRIM_NONE, PRIM_FLOOR, len(tris), len(tris) + 7, 2 ** 31 - 1, -(2 ** 31), dead):
        prim.append(s); uv.append((0.25, 0.25))
    prim, uv = np.asarray(prim, np.int32), np.asarray(uv, F)
    nrm = rng.normal(size=(len(prim), 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    return prim, uv, nrm
