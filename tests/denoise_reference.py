"""The test reference of denoiseFrame (include/rt_api.h).  No test: read by tests/test_denoise_api.py (CPU: the vectorisation pinned against
a per-pixel scalar restatement, the coverage conditions, the quality figures) and tests/test_gpu_denoise.py (GPU: every frame, all pixels, bit for bit).

The filter is the edge-avoiding a-trous wavelet of the interface's definition in numpy float32, vectorised over the pixels of the image.  The 25 taps run in the
stated order (dy outer, dx inner); every product, sum, difference, quotient, max and abs is a ufunc call of its own on float32 arrays, so nothing is fused and
nothing is reordered.  max(x, 0) is written `x if x > 0 else 0` (a NaN gives 0, a zero of either sign gives +0).  Nothing of the code under test is used: the
guide planes come from guides_reference.reference(...), the centre ray's direction from the oracle's orc_get_ray."""
import functools

import numpy as np

import guides_reference as G
from preview_support import DEMODULATE, SAME_PRIM, default_flags, oracle_frame  # noqa: F401  (read as D.default_flags, D.oracle_frame by the tests)

F = np.float32
ALBEDO_FLOOR = F(0.01)
K = (F(0.375), F(0.25), F(0.0625))
DEFAULTS = dict(iterations=5, normal_squarings=5, sigma_z=0.01, sigma_c=1.0)
COUNTS = ("outside", "invalid", "accepted", "wn_lt1", "wz_lt1", "wc_lt1", "prim_mismatch")


def centre_dirs(rt, O, cam, nx, ny):
    """(origin[3], dn[ny, nx, 3]) float32: the centre ray of every pixel from orc_get_ray (as guides_reference._centre_ray), its direction normalised once more."""
    lib = O.load_oracle()
    cam0 = G._camera_without_lens(rt, cam)
    dn = np.zeros((ny, nx, 3), np.float32)
    origin = None
    for j in range(ny):
        for i in range(nx):
            org, d = G._centre_ray(lib, rt, cam0, i, j, nx, ny)
            dn[j, i] = G._unit(G._f3(d))
            origin = G._f3(org)
    return np.array(origin, np.float32), dn


def centre_dirs_numpy(cam, nx, ny):
    """The same in vectorised numpy float32 (camera.h:8-12 without the lens offset, then the ray's second normalisation): for frames too large for a ctypes
    call per pixel.  Pinned against centre_dirs by tests/test_denoise_api.py."""
    v3 = lambda f: [F(f.e[a]) for a in range(3)]
    org, llc, hor, ver = v3(cam.origin), v3(cam.lower_left_corner), v3(cam.horizontal), v3(cam.vertical)
    u = ((np.arange(nx, dtype=np.float32) + F(0.5)) / F(nx))[None, :]
    v = ((np.arange(ny, dtype=np.float32) + F(0.5)) / F(ny))[:, None]
    d = [((llc[a] + u * hor[a]) + v * ver[a]) - org[a] for a in range(3)]

    def unit(w):
        l = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
        return [w[0] / l, w[1] / l, w[2] / l]
    dn = unit(unit(d))
    return np.array(org, np.float32), np.stack(dn, axis=-1).astype(np.float32)


def _max0(x):
    return np.where(x > F(0.0), x, F(0.0)).astype(np.float32)


def denoise(inp, guides, origin, dn, iterations=5, flags=DEMODULATE | SAME_PRIM, normal_squarings=5, sigma_z=0.01, sigma_c=1.0, counts=None):
    """The filter on a whole image.  inp (ny, nx, 3) float32; guides: the planes of guides_reference (albedo, normal, depth, prim); origin, dn: centre_dirs.
    counts: a dict that receives, summed over the iterations and the valid pixels, the non-centre taps by what became of them (COUNTS), `taps` (all of them)
    and, per iteration, the same under `per_iteration`."""
    inp = np.ascontiguousarray(inp, np.float32)
    ny, nx = inp.shape[:2]
    n = [np.ascontiguousarray(guides["normal"][..., a], np.float32) for a in range(3)]
    alb = [np.ascontiguousarray(guides["albedo"][..., a], np.float32) for a in range(3)]
    t = np.ascontiguousarray(guides["depth"], np.float32)
    prim = np.ascontiguousarray(guides["prim"], np.int32)
    valid = prim != G.PRIM_NONE
    sigma_z, sigma_c = F(sigma_z), F(sigma_c)
    demod, same_prim = bool(flags & DEMODULATE), bool(flags & SAME_PRIM)
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    with np.errstate(all="ignore"):
        P = [F(origin[a]) + t * dn[..., a] for a in range(3)]
        rz = F(1.0) / (sigma_z * t)
        m = [np.where(alb[a] > ALBEDO_FLOOR, alb[a], ALBEDO_FLOOR).astype(np.float32) for a in range(3)]
        c = [inp[..., a] / m[a] if demod else inp[..., a].copy() for a in range(3)]
        if counts is not None:
            counts.update({k: 0 for k in COUNTS}, taps=0, per_iteration=[])
        for it in range(iterations):
            s = 1 << it
            if sigma_c > F(0.0):
                sc = sigma_c * F(2.0 ** -it)
                rc = F(1.0) / (sc * sc)
            here = {k: 0 for k in COUNTS}
            acc = [np.zeros((ny, nx), np.float32) for _ in range(3)]
            wsum = np.zeros((ny, nx), np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qi, qj = ii + dx * s, jj + dy * s
                    inside = (qi >= 0) & (qi < nx) & (qj >= 0) & (qj < ny)
                    qi, qj = np.clip(qi, 0, nx - 1), np.clip(qj, 0, ny - 1)
                    ok = valid & inside & valid[qj, qi]
                    h = K[abs(dx)] * K[abs(dy)]
                    cq = [c[a][qj, qi] for a in range(3)]
                    if dx == 0 and dy == 0:
                        w = np.full((ny, nx), h, np.float32)
                    else:
                        nq = [n[a][qj, qi] for a in range(3)]
                        d = n[0] * nq[0] + n[1] * nq[1] + n[2] * nq[2]
                        wn = _max0(d)
                        for _ in range(normal_squarings):
                            wn = wn * wn
                        e = [P[a][qj, qi] - P[a] for a in range(3)]
                        pd = np.abs(n[0] * e[0] + n[1] * e[1] + n[2] * e[2])
                        wz = _max0(F(1.0) - pd * rz)
                        wz = wz * wz
                        w = h * wn * wz
                        if sigma_c > F(0.0):
                            dc = [c[a] - cq[a] for a in range(3)]
                            d2 = dc[0] * dc[0] + dc[1] * dc[1] + dc[2] * dc[2]
                            wc = _max0(F(1.0) - d2 * rc)
                            wc = wc * wc
                            w = w * wc
                        mismatch = prim != prim[qj, qi]
                        if same_prim:
                            w = np.where(mismatch, F(0.0), w).astype(np.float32)
                        if counts is not None:
                            here["outside"] += int((valid & ~inside).sum())
                            here["invalid"] += int((valid & inside & ~valid[qj, qi]).sum())
                            here["accepted"] += int(ok.sum())
                            here["wn_lt1"] += int((ok & (wn < F(1.0))).sum())
                            here["wz_lt1"] += int((ok & (wz < F(1.0))).sum())
                            if sigma_c > F(0.0):
                                here["wc_lt1"] += int((ok & (wc < F(1.0))).sum())
                            if same_prim:
                                here["prim_mismatch"] += int((ok & mismatch).sum())
                    for a in range(3):
                        acc[a] = np.where(ok, acc[a] + w * cq[a], acc[a])
                    wsum = np.where(ok, wsum + w, wsum)
            c = [np.where(valid, acc[a] / wsum, c[a]).astype(np.float32) for a in range(3)]
            if counts is not None:
                here["taps"] = 24 * int(valid.sum())
                counts["per_iteration"].append(here)
                for k in COUNTS + ("taps",):
                    counts[k] += here[k]
        out = np.empty_like(inp)
        for a in range(3):
            out[..., a] = np.where(valid, c[a] * m[a] if demod else c[a], inp[..., a])
    return out


def denoise_scalar(inp, guides, origin, dn, iterations=5, flags=DEMODULATE | SAME_PRIM, normal_squarings=5, sigma_z=0.01, sigma_c=1.0):
    """The same filter one pixel and one tap at a time on numpy float32 scalars, written from the definition: pins the vectorisation of denoise()."""
    inp = np.ascontiguousarray(inp, np.float32)
    ny, nx = inp.shape[:2]
    nrm, alb, dep, prim = guides["normal"], guides["albedo"], guides["depth"], guides["prim"]
    sigma_z, sigma_c = F(sigma_z), F(sigma_c)
    demod, same_prim = bool(flags & DEMODULATE), bool(flags & SAME_PRIM)
    zero, one = F(0.0), F(1.0)
    max0 = lambda x: x if x > zero else zero
    valid = [[int(prim[j, i]) != G.PRIM_NONE for i in range(nx)] for j in range(ny)]
    P = [[None] * nx for _ in range(ny)]
    rz = [[None] * nx for _ in range(ny)]
    m = [[None] * nx for _ in range(ny)]
    c = [[None] * nx for _ in range(ny)]
    with np.errstate(all="ignore"):
        for j in range(ny):
            for i in range(nx):
                t = F(dep[j, i])
                P[j][i] = [F(origin[a]) + t * F(dn[j, i, a]) for a in range(3)]
                rz[j][i] = one / (sigma_z * t)
                m[j][i] = [F(alb[j, i, a]) if F(alb[j, i, a]) > ALBEDO_FLOOR else ALBEDO_FLOOR for a in range(3)]
                c[j][i] = [F(inp[j, i, a]) / m[j][i][a] if demod else F(inp[j, i, a]) for a in range(3)]
        for it in range(iterations):
            s = 1 << it
            if sigma_c > zero:
                sc = sigma_c * F(2.0 ** -it)
                rc = one / (sc * sc)
            nxt = [[c[j][i] for i in range(nx)] for j in range(ny)]
            for j in range(ny):
                for i in range(nx):
                    if not valid[j][i]:
                        continue
                    np_ = [F(nrm[j, i, a]) for a in range(3)]
                    acc, wsum = [zero, zero, zero], zero
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            qi, qj = i + dx * s, j + dy * s
                            if qi < 0 or qi >= nx or qj < 0 or qj >= ny or not valid[qj][qi]:
                                continue
                            h = K[abs(dx)] * K[abs(dy)]
                            cq = c[qj][qi]
                            if dx == 0 and dy == 0:
                                w = h
                            else:
                                nq = [F(nrm[qj, qi, a]) for a in range(3)]
                                wn = max0(np_[0] * nq[0] + np_[1] * nq[1] + np_[2] * nq[2])
                                for _ in range(normal_squarings):
                                    wn = wn * wn
                                e = [P[qj][qi][a] - P[j][i][a] for a in range(3)]
                                pd = abs(np_[0] * e[0] + np_[1] * e[1] + np_[2] * e[2])
                                wz = max0(one - pd * rz[j][i])
                                wz = wz * wz
                                w = h * wn * wz
                                if sigma_c > zero:
                                    dc = [c[j][i][a] - cq[a] for a in range(3)]
                                    d2 = dc[0] * dc[0] + dc[1] * dc[1] + dc[2] * dc[2]
                                    wc = max0(one - d2 * rc)
                                    wc = wc * wc
                                    w = w * wc
                                if same_prim and int(prim[j, i]) != int(prim[qj, qi]):
                                    w = zero
                            acc = [acc[a] + w * cq[a] for a in range(3)]
                            wsum = wsum + w
                    nxt[j][i] = [acc[a] / wsum for a in range(3)]
            c = nxt
        out = np.array(inp, copy=True)
        for j in range(ny):
            for i in range(nx):
                if valid[j][i]:
                    out[j, i] = [c[j][i][a] * m[j][i][a] if demod else c[j][i][a] for a in range(3)]
    return out


@functools.lru_cache(maxsize=None)
def frame_inputs(rt, O, name):
    """(guides, origin, dn, mesh) of a named frame of guides_reference with the default options of its scene kind."""
    mesh = name in G.MESH_FRAMES
    if mesh:
        f = G.mesh_frame(rt, O, name)
        cam, nx, ny = f["cam"], f["nx"], f["ny"]
    else:
        _, _, cam, nx, ny = G.sphere_frame(rt, name)
    origin, dn = centre_dirs(rt, O, cam, nx, ny)
    return G.reference(rt, O, name), origin, dn, mesh


def rmse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def ulp_distance(a, b):
    """Distance in units of the last place between two finite float32 arrays (the integer order of the sign-magnitude encoding)."""
    def key(x):
        u = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7FFFFFFF), u)
    return np.abs(key(a) - key(b))
