"""The test reference of previewFrame (include/rt_api.h).  No test: read by tests/test_preview_api.py (CPU: the vectorisation pinned against a
per-pixel scalar restatement, the coverage conditions, the quality figures) and tests/test_gpu_preview.py (GPU: every call, all pixels, bit for bit).

The definition of the interface in numpy float32, vectorised over the pixels of the image: every product, sum, difference, quotient, abs, floor and sqrt is a
ufunc call of its own on float32 operands, so nothing is fused and nothing is reordered; min(a, b) is `a if a < b else b`, max(x, 0) is `x if x > 0 else 0`; a
comparison with a NaN is false.  A Previewer keeps the history across calls - the previous call's camera and its planes P, n, prim, c, N, M1, M2 - as the
library does on the device, and uses nothing of the code under test: the guide planes come from guides_reference, the centre ray's direction from
denoise_reference.centre_dirs.  The helpers the two existing references have (camera fields, dot, the previous camera's constants, the a-trous kernel's
weights) are imported from them; the stages are restated here from the definition."""
import numpy as np

import accumulate_reference as A
import denoise_reference as D
import guides_reference as G

F = np.float32
DEMODULATE, SAME_PRIM = D.DEMODULATE, D.SAME_PRIM
ALBEDO_FLOOR = D.ALBEDO_FLOOR
K = D.K
MIN_HISTORY = F(4.0)
LUM_EPS = F(1e-4)
LR, LG, LB = F(0.2126), F(0.7152), F(0.0722)
DEFAULTS = dict(max_history=32, iterations=5, normal_squarings=5, sigma_z=0.01, normal_min=0.9, sigma_l=4.0)
# pixels by the branch of stage V they take; the non-centre taps of the spatial estimate (of the pixels that take it) that reach a valid pixel, by the weight
# that is zero for them (a tap may be counted under several); the non-centre a-trous taps that reach a valid pixel, and those of them with wl < 1
COUNTS = ("valid", "blended", "temporal_variance", "spatial_variance", "spatial_taps", "spatial_wn_zero", "spatial_wz_zero", "spatial_prim_mismatch",
          "atrous_taps", "atrous_wl_lt1")

_dot = A._dot


def lum(x):
    return LR * x[0] + LG * x[1] + LB * x[2]


def _max0(x):
    return np.where(x > F(0.0), x, F(0.0)).astype(np.float32)


class Previewer:
    """The history of one renderer.  step() is one previewFrame call; scalar=True runs the per-pixel restatement instead of the vectorised form."""

    def __init__(self, scalar=False):
        self.scalar = scalar
        self.reset()

    def reset(self):
        self.prev = None
        self.frames = 0

    def step(self, inp, guides, cam, origin, dn, flags=DEMODULATE | SAME_PRIM, max_history=32, iterations=5, normal_squarings=5, sigma_z=0.01, normal_min=0.9,
             sigma_l=4.0, counts=None):
        """inp (ny, nx, 3) float32; guides: the planes of guides_reference for `cam`; origin, dn: centre_dirs for `cam`.  Returns (out, N, variance).  counts: a
        dict whose COUNTS entries are increased by this call's figures."""
        fn = _step_scalar if self.scalar else _step
        out, N, var, store = fn(self.prev, np.ascontiguousarray(inp, np.float32), guides, origin, dn, flags, F(max_history), int(iterations),
                                int(normal_squarings), F(sigma_z), F(normal_min), F(sigma_l), counts)
        store["cam"] = A._cam(cam)
        self.prev = store
        self.frames += 1
        return out, N, var


def _add(counts, key, n):
    if counts is not None:
        counts[key] = counts.get(key, 0) + int(n)


def _step(prev, inp, guides, origin, dn, flags, max_history, iterations, normal_squarings, sigma_z, normal_min, sigma_l, counts):
    ny, nx = inp.shape[:2]
    n = [np.ascontiguousarray(guides["normal"][..., a], np.float32) for a in range(3)]
    alb = [np.ascontiguousarray(guides["albedo"][..., a], np.float32) for a in range(3)]
    t = np.ascontiguousarray(guides["depth"], np.float32)
    prim = np.ascontiguousarray(guides["prim"], np.int32)
    valid = prim != G.PRIM_NONE
    demod, same_prim = bool(flags & DEMODULATE), bool(flags & SAME_PRIM)
    one, zero = F(1.0), F(0.0)
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    with np.errstate(all="ignore"):
        P = [F(origin[a]) + t * dn[..., a] for a in range(3)]
        rz = one / (sigma_z * t)
        m = [np.where(alb[a] > ALBEDO_FLOOR, alb[a], ALBEDO_FLOOR).astype(np.float32) for a in range(3)]
        c0 = [inp[..., a] / m[a] if demod else inp[..., a].copy() for a in range(3)]
        l0 = lum(c0)
        q0 = l0 * l0
        # ---- stage T: accumulateFrame's definition, with the moments of the luminance ----
        if prev is None:
            c, M1, M2 = c0, l0, q0
            N = np.where(valid, one, zero).astype(np.float32)
            use = np.zeros((ny, nx), bool)
        else:
            pc = prev["cam"]
            Lu, Lv, Lw, Hl, Vl = A._constants(pc)
            e = [P[a] - pc["o"][a] for a in range(3)]
            ea, eb, ec = _dot(e, pc["u"]), _dot(e, pc["v"]), _dot(e, pc["w"])
            r = Lw / ec
            s = (ea * r - Lu) / Hl
            tt = (eb * r - Lv) / Vl
            x = s * F(nx) - F(0.5)
            y = tt * F(ny) - F(0.5)
            candidate = valid & (r > zero) & (x >= F(-1.0)) & (x < F(nx)) & (y >= F(-1.0)) & (y < F(ny))
            x0, y0 = np.floor(x), np.floor(y)
            fx, fy = x - x0, y - y0
            i0 = np.where(candidate, x0, zero).astype(np.int64)
            j0 = np.where(candidate, y0, zero).astype(np.int64)
            acc = [np.zeros((ny, nx), np.float32) for _ in range(3)]
            nsum, wsum, m1sum, m2sum = (np.zeros((ny, nx), np.float32) for _ in range(4))
            for dy in (0, 1):
                for dx in (0, 1):
                    qi, qj = i0 + dx, j0 + dy
                    inside = (qi >= 0) & (qi < nx) & (qj >= 0) & (qj < ny)
                    qi, qj = np.clip(qi, 0, nx - 1), np.clip(qj, 0, ny - 1)
                    bw = (fx if dx else one - fx) * (fy if dy else one - fy)
                    Nq = prev["N"][qj, qi]
                    d = [prev["P"][a][qj, qi] - P[a] for a in range(3)]
                    ok = inside & (Nq > zero) & (np.abs(_dot(n, d)) * rz < one) & (_dot(n, [prev["n"][a][qj, qi] for a in range(3)]) >= normal_min)
                    if same_prim:
                        ok = ok & (prim == prev["prim"][qj, qi])
                    for a in range(3):
                        acc[a] = np.where(ok, acc[a] + bw * prev["c"][a][qj, qi], acc[a]).astype(np.float32)
                    nsum = np.where(ok, nsum + bw * Nq, nsum).astype(np.float32)
                    wsum = np.where(ok, wsum + bw, wsum).astype(np.float32)
                    m1sum = np.where(ok, m1sum + bw * prev["M1"][qj, qi], m1sum).astype(np.float32)
                    m2sum = np.where(ok, m2sum + bw * prev["M2"][qj, qi], m2sum).astype(np.float32)
            use = candidate & (wsum > zero)
            length = nsum / wsum + one
            Nb = np.where(length < max_history, length, max_history).astype(np.float32)
            al = one / Nb
            c = []
            for a in range(3):
                h = acc[a] / wsum
                c.append(np.where(use, h + al * (c0[a] - h), c0[a]).astype(np.float32))
            h1, h2 = m1sum / wsum, m2sum / wsum
            M1 = np.where(use, h1 + al * (l0 - h1), l0).astype(np.float32)
            M2 = np.where(use, h2 + al * (q0 - h2), q0).astype(np.float32)
            N = np.where(valid, np.where(use, Nb, one), zero).astype(np.float32)
        store = dict(P=P, n=n, prim=prim, c=c, N=N, M1=M1, M2=M2)
        # ---- stage V: the variance of the luminance ----
        temporal = valid & (N >= MIN_HISTORY)
        spatial = valid & ~(N >= MIN_HISTORY)
        s1, s2, ws = (np.zeros((ny, nx), np.float32) for _ in range(3))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                qi, qj = ii + dx, jj + dy
                inside = (qi >= 0) & (qi < nx) & (qj >= 0) & (qj < ny)
                qi, qj = np.clip(qi, 0, nx - 1), np.clip(qj, 0, ny - 1)
                ok = inside & valid[qj, qi]
                if dx == 0 and dy == 0:
                    w = np.full((ny, nx), one, np.float32)
                else:
                    wn = _max0(_dot(n, [n[a][qj, qi] for a in range(3)]))
                    for _ in range(normal_squarings):
                        wn = wn * wn
                    e = [P[a][qj, qi] - P[a] for a in range(3)]
                    wz = _max0(one - np.abs(_dot(n, e)) * rz)
                    wz = wz * wz
                    w = wn * wz
                    mismatch = prim != prim[qj, qi]
                    if same_prim:
                        w = np.where(mismatch, zero, w).astype(np.float32)
                    if counts is not None:
                        tap = spatial & ok
                        _add(counts, "spatial_taps", tap.sum())
                        _add(counts, "spatial_wn_zero", (tap & (wn == zero)).sum())
                        _add(counts, "spatial_wz_zero", (tap & (wz == zero)).sum())
                        if same_prim:
                            _add(counts, "spatial_prim_mismatch", (tap & mismatch).sum())
                s1 = np.where(ok, s1 + w * M1[qj, qi], s1).astype(np.float32)
                s2 = np.where(ok, s2 + w * M2[qj, qi], s2).astype(np.float32)
                ws = np.where(ok, ws + w, ws).astype(np.float32)
        a1, a2 = s1 / ws, s2 / ws
        var_s = _max0(a2 - a1 * a1) * (F(4.0) / N)
        var_t = _max0(M2 - M1 * M1)
        var = np.where(temporal, var_t, np.where(spatial, var_s, zero)).astype(np.float32)
        variance = var.copy()
        for key, val in (("valid", valid), ("blended", use), ("temporal_variance", temporal), ("spatial_variance", spatial)):
            _add(counts, key, val.sum())
        # ---- stage A: the a-trous filter on (c, var) ----
        for it in range(iterations):
            s = 1 << it
            rl = one / (sigma_l * np.sqrt(var) + LUM_EPS)
            lc = lum(c)
            acc = [np.zeros((ny, nx), np.float32) for _ in range(3)]
            vsum, wsum = np.zeros((ny, nx), np.float32), np.zeros((ny, nx), np.float32)
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
                        wn = _max0(_dot(n, [n[a][qj, qi] for a in range(3)]))
                        for _ in range(normal_squarings):
                            wn = wn * wn
                        e = [P[a][qj, qi] - P[a] for a in range(3)]
                        wz = _max0(one - np.abs(_dot(n, e)) * rz)
                        wz = wz * wz
                        w = h * wn * wz
                        wl = _max0(one - np.abs(lc - lc[qj, qi]) * rl)
                        wl = wl * wl
                        w = w * wl
                        if same_prim:
                            w = np.where(prim != prim[qj, qi], zero, w).astype(np.float32)
                        if counts is not None:
                            _add(counts, "atrous_taps", ok.sum())
                            _add(counts, "atrous_wl_lt1", (ok & (wl < one)).sum())
                    for a in range(3):
                        acc[a] = np.where(ok, acc[a] + w * cq[a], acc[a]).astype(np.float32)
                    vsum = np.where(ok, vsum + (w * w) * var[qj, qi], vsum).astype(np.float32)
                    wsum = np.where(ok, wsum + w, wsum).astype(np.float32)
            c = [np.where(valid, acc[a] / wsum, c[a]).astype(np.float32) for a in range(3)]
            var = np.where(valid, vsum / (wsum * wsum), var).astype(np.float32)
        out = np.empty_like(inp)
        for a in range(3):
            out[..., a] = np.where(valid, c[a] * m[a] if demod else c[a], inp[..., a])
    return out, N, variance, store


def _step_scalar(prev, inp, guides, origin, dn, flags, max_history, iterations, normal_squarings, sigma_z, normal_min, sigma_l, counts):
    """The same call one pixel and one tap at a time on numpy float32 scalars, written from the definition: pins the vectorisation of _step()."""
    ny, nx = inp.shape[:2]
    nrm, alb, dep, prim = guides["normal"], guides["albedo"], guides["depth"], guides["prim"]
    demod, same_prim = bool(flags & DEMODULATE), bool(flags & SAME_PRIM)
    one, zero = F(1.0), F(0.0)
    max0 = lambda v: v if v > zero else zero
    lum1 = lambda v: LR * v[0] + LG * v[1] + LB * v[2]
    valid = [[int(prim[j, i]) != G.PRIM_NONE for i in range(nx)] for j in range(ny)]
    grid = lambda: [[None] * nx for _ in range(ny)]
    P, rz, m, c, nv = grid(), grid(), grid(), grid(), grid()
    N = np.zeros((ny, nx), np.float32)
    M1 = np.zeros((ny, nx), np.float32)
    M2 = np.zeros((ny, nx), np.float32)
    variance = np.zeros((ny, nx), np.float32)
    if prev is not None:
        pc = prev["cam"]
        Lu, Lv, Lw, Hl, Vl = A._constants(pc)
    with np.errstate(all="ignore"):
        # ---- stage T ----
        for j in range(ny):
            for i in range(nx):
                t = F(dep[j, i])
                Pp = [F(origin[a]) + t * F(dn[j, i, a]) for a in range(3)]
                P[j][i] = Pp
                rz[j][i] = one / (sigma_z * t)
                nv[j][i] = [F(nrm[j, i, a]) for a in range(3)]
                m[j][i] = [F(alb[j, i, a]) if F(alb[j, i, a]) > ALBEDO_FLOOR else ALBEDO_FLOOR for a in range(3)]
                cp = [F(inp[j, i, a]) / m[j][i][a] if demod else F(inp[j, i, a]) for a in range(3)]
                l0 = lum1(cp)
                q0 = l0 * l0
                m1, m2 = l0, q0
                c[j][i] = cp
                M1[j, i], M2[j, i] = m1, m2
                if not valid[j][i]:
                    continue                                    # out = in, N = 0
                Np = one
                if prev is not None:
                    npx = nv[j][i]
                    e = [Pp[a] - pc["o"][a] for a in range(3)]
                    ea, eb, ec = _dot(e, pc["u"]), _dot(e, pc["v"]), _dot(e, pc["w"])
                    r = Lw / ec
                    s = (ea * r - Lu) / Hl
                    tt = (eb * r - Lv) / Vl
                    x = s * F(nx) - F(0.5)
                    y = tt * F(ny) - F(0.5)
                    if r > zero and x >= F(-1.0) and x < F(nx) and y >= F(-1.0) and y < F(ny):
                        x0, y0 = np.floor(x), np.floor(y)
                        fx, fy = x - x0, y - y0
                        i0, j0 = int(x0), int(y0)
                        acc, nsum, wsum, m1sum, m2sum = [zero, zero, zero], zero, zero, zero, zero
                        for dy in (0, 1):
                            for dx in (0, 1):
                                qi, qj = i0 + dx, j0 + dy
                                bw = (fx if dx else one - fx) * (fy if dy else one - fy)
                                if qi < 0 or qi >= nx or qj < 0 or qj >= ny:
                                    continue
                                if not prev["N"][qj, qi] > zero:
                                    continue
                                d = [prev["P"][a][qj, qi] - Pp[a] for a in range(3)]
                                if not abs(_dot(npx, d)) * rz[j][i] < one:
                                    continue
                                if not _dot(npx, [prev["n"][a][qj, qi] for a in range(3)]) >= normal_min:
                                    continue
                                if same_prim and int(prim[j, i]) != int(prev["prim"][qj, qi]):
                                    continue
                                acc = [acc[a] + bw * prev["c"][a][qj, qi] for a in range(3)]
                                nsum = nsum + bw * prev["N"][qj, qi]
                                wsum = wsum + bw
                                m1sum = m1sum + bw * prev["M1"][qj, qi]
                                m2sum = m2sum + bw * prev["M2"][qj, qi]
                        if wsum > zero:
                            length = nsum / wsum + one
                            Np = length if length < max_history else max_history
                            al = one / Np
                            h = [acc[a] / wsum for a in range(3)]
                            cp = [h[a] + al * (cp[a] - h[a]) for a in range(3)]
                            h1, h2 = m1sum / wsum, m2sum / wsum
                            m1 = h1 + al * (l0 - h1)
                            m2 = h2 + al * (q0 - h2)
                N[j, i] = Np
                c[j][i] = cp
                M1[j, i], M2[j, i] = m1, m2
        store = dict(P=[np.array([[P[j][i][a] for i in range(nx)] for j in range(ny)], np.float32) for a in range(3)],
                     n=[np.array(nrm[..., a], np.float32) for a in range(3)], prim=np.array(prim, np.int32),
                     c=[np.array([[c[j][i][a] for i in range(nx)] for j in range(ny)], np.float32) for a in range(3)], N=N, M1=M1, M2=M2)

        def geometry_weight(i, j, qi, qj):
            """wn * wz of the denoiser's definition, left to right, for the pair p = (i, j), q = (qi, qj); h is multiplied in front by the caller."""
            wn = max0(_dot(nv[j][i], nv[qj][qi]))
            for _ in range(normal_squarings):
                wn = wn * wn
            e = [P[qj][qi][a] - P[j][i][a] for a in range(3)]
            wz = max0(one - abs(_dot(nv[j][i], e)) * rz[j][i])
            wz = wz * wz
            return wn, wz

        # ---- stage V ----
        var = grid()
        for j in range(ny):
            for i in range(nx):
                if not valid[j][i]:
                    var[j][i] = zero
                    continue
                if N[j, i] >= MIN_HISTORY:
                    v = max0(M2[j, i] - M1[j, i] * M1[j, i])
                else:
                    s1, s2, ws = zero, zero, zero
                    for dy in range(-3, 4):
                        for dx in range(-3, 4):
                            qi, qj = i + dx, j + dy
                            if qi < 0 or qi >= nx or qj < 0 or qj >= ny or not valid[qj][qi]:
                                continue
                            if dx == 0 and dy == 0:
                                w = one
                            else:
                                wn, wz = geometry_weight(i, j, qi, qj)
                                w = wn * wz
                                if same_prim and int(prim[j, i]) != int(prim[qj, qi]):
                                    w = zero
                            s1 = s1 + w * M1[qj, qi]
                            s2 = s2 + w * M2[qj, qi]
                            ws = ws + w
                    a1, a2 = s1 / ws, s2 / ws
                    v = max0(a2 - a1 * a1) * (F(4.0) / N[j, i])
                var[j][i] = v
                variance[j, i] = v
        # ---- stage A ----
        for it in range(iterations):
            s = 1 << it
            nxt_c = [[c[j][i] for i in range(nx)] for j in range(ny)]
            nxt_v = [[var[j][i] for i in range(nx)] for j in range(ny)]
            for j in range(ny):
                for i in range(nx):
                    if not valid[j][i]:
                        continue
                    rl = one / (sigma_l * np.sqrt(var[j][i]) + LUM_EPS)
                    lp = lum1(c[j][i])
                    acc, vsum, wsum = [zero, zero, zero], zero, zero
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
                                wn, wz = geometry_weight(i, j, qi, qj)
                                w = h * wn * wz
                                wl = max0(one - abs(lp - lum1(cq)) * rl)
                                wl = wl * wl
                                w = w * wl
                                if same_prim and int(prim[j, i]) != int(prim[qj, qi]):
                                    w = zero
                            acc = [acc[a] + w * cq[a] for a in range(3)]
                            vsum = vsum + (w * w) * var[qj][qi]
                            wsum = wsum + w
                    nxt_c[j][i] = [acc[a] / wsum for a in range(3)]
                    nxt_v[j][i] = vsum / (wsum * wsum)
            c, var = nxt_c, nxt_v
        out = np.array(inp, copy=True)
        for j in range(ny):
            for i in range(nx):
                if valid[j][i]:
                    out[j, i] = [c[j][i][a] * m[j][i][a] if demod else c[j][i][a] for a in range(3)]
    return out, N, variance, store
