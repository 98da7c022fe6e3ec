"""filterTexels (include/rt_api.h, "filtering texels") restated twice on top of texels_reference.raster: `iterate` in numpy float32 over the whole atlas, one ufunc
per operation, operands in the order the header writes them, and `iterate_scalar`, one texel and one tap at a time with float32 scalars.  No test: a plain
module, imported by tests/test_texel_filter_api.py and tests/test_gpu_texel_filter.py, with the inputs both files use.  Nothing here calls the library."""
import numpy as np

import texels_reference as TR

F = np.float32
K = (F(0.375), F(0.25), F(0.0625))
WIDTH = {0: 3, 1: 27, 2: 1}                     # RT_GATHER_IRRADIANCE, RT_GATHER_SH9, RT_GATHER_VISIBILITY
MODE_OF = {3: 0, 27: 1, 1: 2}
DEFAULTS = dict(iterations=3, normal_squarings=5, sigma_d=2.0, sigma_z=2.0, sigma_c=0.5)
MAX_ITERATIONS, MAX_SQUARINGS = 8, 7


def _max0(x):
    return np.where(x > 0, x, F(0)).astype(F)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def footprint(tris, ras, sigma_d, sigma_z):
    """(f2, r2, rz), each (H, W) float32: the footprint of every owned texel (zeros elsewhere)."""
    prim = ras["prim"]
    H, W = prim.shape
    owned = prim != TR.PRIM_NONE
    t = tris[np.where(owned, prim, 0)]
    tc, v = t["texCoords"].astype(F), t["v"].astype(F)
    ax, ay, bx, by, cx, cy = (tc[..., i] for i in range(6))
    with np.errstate(all="ignore"):
        d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        ux, vx, uy, vy = (cy - ay) / d, (ay - by) / d, (ax - cx) / d, (bx - ax) / d
        e1, e2 = v[..., 1, :] - v[..., 0, :], v[..., 2, :] - v[..., 0, :]
        Gx = (ux[..., None] * e1 + vx[..., None] * e2) / F(W)
        Gy = (uy[..., None] * e1 + vy[..., None] * e2) / F(H)
        f2 = F(0.5) * (_dot(Gx, Gx) + _dot(Gy, Gy))
        r2 = (F(sigma_d) * F(sigma_d)) * f2
        rz = F(1) / (F(sigma_z) * np.sqrt(f2))
    z = F(0)
    return np.where(owned, f2, z).astype(F), np.where(owned, r2, z).astype(F), np.where(owned, rz, z).astype(F)


def rc_of(sigma_c, it):
    sc = F(sigma_c) * (F(1) / F(1 << it))
    with np.errstate(all="ignore"):
        return F(1) / (sc * sc)


def new_stats():
    return dict(outside=0, unowned=0, reach=0, reach_other_cell=0, wn0=0, wz0=0, wc0=0, accepted=0)


def iterate(tris, ras, plane, iterations, normal_squarings, sigma_d, sigma_z, sigma_c, stats=None):
    """The filtered values after every iteration 1 .. iterations - a list of (H, W, C) float32 arrays, zeros at unowned texels - from the raster `ras` of
    `tris` (texels_reference.raster; its dilation is not read).  `stats` (new_stats()) counts, over all texels and iterations, why taps were dropped and
    which weights of accepted taps were 0."""
    prim, P, n = ras["prim"], ras["pos"], ras["nrm"]
    H, W = prim.shape
    owned = prim != TR.PRIM_NONE
    C = plane.shape[2]
    L = min(C, 3)
    _, r2, rz = footprint(tris, ras, sigma_d, sigma_z)
    c = np.where(owned[..., None], plane.astype(F), F(0)).astype(F)
    Y, X = np.mgrid[0:H, 0:W]
    steps = []
    with np.errstate(all="ignore"):
        for it in range(iterations):
            s = 1 << it
            rc = rc_of(sigma_c, it) if sigma_c > 0 else F(0)
            total, wsum = np.zeros((H, W, C), F), np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    h = K[abs(dx)] * K[abs(dy)]
                    if dx == 0 and dy == 0:
                        total = total + h * c
                        wsum = wsum + h
                        continue
                    qx, qy = X + dx * s, Y + dy * s
                    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    qx, qy = np.where(inside, qx, X), np.where(inside, qy, Y)
                    own_q, Pq, nq, cq = owned[qy, qx], P[qy, qx], n[qy, qx], c[qy, qx]
                    e = Pq - P
                    d2 = _dot(e, e)
                    reach = d2 <= r2 * F((dx * dx + dy * dy) * s * s)
                    wn = _max0(_dot(n, nq))
                    for _ in range(normal_squarings):
                        wn = wn * wn
                    pd = np.abs(_dot(n, e))
                    wz = _max0(F(1) - pd * rz)
                    wz = wz * wz
                    w = h * wn * wz
                    wc = None
                    if sigma_c > 0:
                        dc = c[..., :L] - cq[..., :L]
                        dd = dc[..., 0] * dc[..., 0]
                        if L == 3:
                            dd = dd + dc[..., 1] * dc[..., 1] + dc[..., 2] * dc[..., 2]
                        wc = _max0(F(1) - dd * rc)
                        wc = wc * wc
                        w = w * wc
                    ok = owned & inside & own_q & reach
                    total = np.where(ok[..., None], total + w[..., None] * cq, total)
                    wsum = np.where(ok, wsum + w, wsum)
                    if stats is not None:
                        stats["outside"] += int((owned & ~inside).sum())
                        stats["unowned"] += int((owned & inside & ~own_q).sum())
                        far = owned & inside & own_q & ~reach
                        stats["reach"] += int(far.sum())
                        stats["reach_other_cell"] += int((far & (prim // 2 != prim[qy, qx] // 2)).sum())
                        stats["accepted"] += int(ok.sum())
                        stats["wn0"] += int((ok & (wn == 0)).sum())
                        stats["wz0"] += int((ok & (wz == 0)).sum())
                        if wc is not None:
                            stats["wc0"] += int((ok & (wn > 0) & (wz > 0) & (wc == 0)).sum())
            c = np.where(owned[..., None], total / wsum[..., None], F(0)).astype(F)
            steps.append(c)
    return steps


def iterate_scalar(tris, ras, plane, iterations, normal_squarings, sigma_d, sigma_z, sigma_c):
    """`iterate` one texel and one tap at a time: float32 scalars, a dropped tap skipped (the C values of a texel are one float32 array: elementwise)."""
    prim, P, n = ras["prim"], ras["pos"], ras["nrm"]
    H, W = prim.shape
    C = plane.shape[2]
    L = min(C, 3)
    owned = [(y, x) for y in range(H) for x in range(W) if prim[y, x] != TR.PRIM_NONE]
    r2, rz = {}, {}
    sd, sz = F(sigma_d), F(sigma_z)
    with np.errstate(all="ignore"):
        for (y, x) in owned:
            t = tris[prim[y, x]]
            ax, ay, bx, by, cx, cy = (F(u) for u in t["texCoords"])
            d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            ux, vx, uy, vy = (cy - ay) / d, (ay - by) / d, (ax - cx) / d, (bx - ax) / d
            gx, gy = [], []
            for k in range(3):
                e1, e2 = F(t["v"][1, k]) - F(t["v"][0, k]), F(t["v"][2, k]) - F(t["v"][0, k])
                gx.append((ux * e1 + vx * e2) / F(W))
                gy.append((uy * e1 + vy * e2) / F(H))
            f2 = F(0.5) * ((gx[0] * gx[0] + gx[1] * gx[1] + gx[2] * gx[2]) + (gy[0] * gy[0] + gy[1] * gy[1] + gy[2] * gy[2]))
            r2[y, x] = (sd * sd) * f2
            rz[y, x] = F(1) / (sz * np.sqrt(f2))
        c = np.zeros((H, W, C), F)
        for (y, x) in owned:
            c[y, x] = plane[y, x]
        steps = []
        zero = F(0)
        for it in range(iterations):
            s = 1 << it
            rc = rc_of(sigma_c, it) if sigma_c > 0 else zero
            new = np.zeros((H, W, C), F)
            for (y, x) in owned:
                np_, Pp, cp = [F(v) for v in n[y, x]], [F(v) for v in P[y, x]], c[y, x]
                total, wsum = np.zeros(C, F), zero
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        h = K[abs(dx)] * K[abs(dy)]
                        qx, qy = x + dx * s, y + dy * s
                        if dx == 0 and dy == 0:
                            w = h
                        else:
                            if qx < 0 or qx >= W or qy < 0 or qy >= H or prim[qy, qx] == TR.PRIM_NONE:
                                continue
                            nq, Pq = [F(v) for v in n[qy, qx]], [F(v) for v in P[qy, qx]]
                            e = [Pq[0] - Pp[0], Pq[1] - Pp[1], Pq[2] - Pp[2]]
                            d2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
                            if not (d2 <= r2[y, x] * F((dx * dx + dy * dy) * s * s)):
                                continue
                            dn = np_[0] * nq[0] + np_[1] * nq[1] + np_[2] * nq[2]
                            wn = dn if dn > 0 else zero
                            for _ in range(normal_squarings):
                                wn = wn * wn
                            pd = abs(np_[0] * e[0] + np_[1] * e[1] + np_[2] * e[2])
                            t = F(1) - pd * rz[y, x]
                            wz = t if t > 0 else zero
                            wz = wz * wz
                            w = h * wn * wz
                            if sigma_c > 0:
                                cq = c[qy, qx]
                                dd = None
                                for j in range(L):
                                    dc = cp[j] - cq[j]
                                    dd = dc * dc if dd is None else dd + dc * dc
                                t = F(1) - dd * rc
                                wc = t if t > 0 else zero
                                wc = wc * wc
                                w = w * wc
                        total = total + w * c[qy, qx]
                        wsum = wsum + w
                new[y, x] = total / wsum
            c = new
            steps.append(c)
    return steps


def scatter(c, src):
    """out(t) = c(src(t)), zeros where src(t) == -1."""
    H, W, C = c.shape
    flat, s = c.reshape(-1, C), src.ravel()
    return np.where((s != -1)[:, None], flat[np.where(s != -1, s, 0)], F(0)).astype(F).reshape(H, W, C)


def filter_numpy(tris, W, H, dilate, plane, iterations, normal_squarings, sigma_d, sigma_z, sigma_c, ras=None):
    """(owned, out): the whole call in numpy."""
    ras = TR.raster(tris, W, H, dilate) if ras is None else ras
    steps = iterate(tris, ras, plane, iterations, normal_squarings, sigma_d, sigma_z, sigma_c)
    return ras["owned"], scatter(steps[-1], ras["src"])


# ---- the inputs of the tests -----------------------------------------------------------------------------------------------------------------------

def smooth(ras, C):
    """A smooth function of pos and nrm, (H, W, C) float32 in about [0, 1.5]: finite whatever the raster holds."""
    with np.errstate(all="ignore"):
        P = np.nan_to_num(ras["pos"].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
        n = np.nan_to_num(ras["nrm"].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
        j = np.arange(C)[None, None, :]
        v = 0.75 + 0.25 * np.sin(0.7 * P[..., 0:1] + 0.3 * P[..., 1:2] + 0.4 * j) + 0.25 * n[..., 2:3] + 0.25 * np.cos(0.5 * P[..., 2:3] - 0.2 * j)
    return v.astype(F)


def noisy_plane(ras, C, seed, amplitude=0.5):
    """smooth + seeded uniform noise of +-amplitude, everywhere (the filter reads it at owned texels only)."""
    rng = np.random.default_rng(seed)
    H, W = ras["prim"].shape
    return (smooth(ras, C) + rng.uniform(-amplitude, amplitude, (H, W, C)).astype(F)).astype(F)


def small_mesh(degenerate=True):
    """16 triangles for rtAtlasGrid, two per cell: a flat unit quad; a quad folded by 90 degrees along its diagonal; a triangle and its own copy with the winding
    reversed (opposite normals at the same place); two flat quads of other sizes; and - with `degenerate` - a triangle without extent (f2 = 0, the normal a
    NaN) and one of the size 1e30 (f2 = inf); else two more flat triangles.  Every cell lies 10 units from the next, so no tap reaches across cells."""
    tris = np.zeros(16, TR.TRIANGLE)
    quad = lambda o, a, b: ([o, o + a, o + b], [o + a + b, o + b, o + a])           # the lower-left and the upper-right half, as rtAtlasGrid maps them
    at = lambda i: np.array([10.0 * i, 0.0, 0.0])
    X, Y, Z = np.eye(3)
    v = []
    v += quad(at(0), X, Y)
    lo, _ = quad(at(1), X, Y)
    v += [lo, [at(1) + 0.5 * (X + Y) + 0.70710678 * Z, at(1) + Y, at(1) + X]]             # the far corner turned about the diagonal, out of the plane
    v += [[at(2), at(2) + X, at(2) + Y], [at(2) + X, at(2), at(2) + Y]]
    v += quad(at(3), 2 * X, 3 * Y)
    v += quad(at(4), 0.5 * Y, 0.5 * Z)
    v += quad(at(5), X + Z, Y)
    v += quad(at(6), X, Y + Z)
    if degenerate:
        v += [[at(7), at(7), at(7)], [at(7) + 1e30 * X, at(7) + 1e30 * Y, at(7) + 1e30 * Z]]
    else:
        v += quad(at(7), X, 2 * Y)
    tris["v"] = np.asarray(v, F)
    return TR.atlas_grid(tris, 0.05)[0]


def lambert(ras, light=(3.0, 4.0, 5.0)):
    """The clean signal of the quality check: (H, W, 3) Lambert shading of pos / nrm under a point light, zeros at unowned texels."""
    P, n = ras["pos"].astype(np.float64), ras["nrm"].astype(np.float64)
    to = np.asarray(light)[None, None, :] - P
    dist = np.linalg.norm(to, axis=-1, keepdims=True)
    cos = np.abs((n * to / dist).sum(-1, keepdims=True))
    v = 20.0 * cos / (dist * dist) * np.array([1.0, 0.8, 0.6])[None, None, :] + 0.05
    return np.where((ras["prim"] != TR.PRIM_NONE)[..., None], v, 0.0).astype(F)
