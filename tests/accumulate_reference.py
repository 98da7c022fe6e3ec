"""The test reference of accumulateFrame (include/rt_api.h).  No test: read by tests/test_accumulate_api.py (CPU: the vectorisation pinned
against a per-pixel scalar restatement, the coverage conditions, the quality figures) and tests/test_gpu_accumulate.py (GPU: every call, all pixels, bit for
bit).

The definition of the interface in numpy float32, vectorised over the pixels of the image: every product, sum, difference, quotient, abs and floor is a ufunc
call of its own on float32 operands, so nothing is fused and nothing is reordered; min(a, b) is `a if a < b else b`; a comparison with a NaN is false.  An
Accumulator keeps the history across calls - the previous call's camera and its planes P, n, prim, c, N - as the library does on the device, and uses nothing
of the code under test: the guide planes come from guides_reference, the centre ray's direction from denoise_reference.centre_dirs (the oracle's orc_get_ray)."""
import functools
import math

import numpy as np

import denoise_reference as D
import guides_reference as G

F = np.float32
DEMODULATE, SAME_PRIM = D.DEMODULATE, D.SAME_PRIM
ALBEDO_FLOOR = D.ALBEDO_FLOOR
DEFAULTS = dict(max_history=32, sigma_z=0.01, normal_min=0.9)
# what became of the four taps of the candidate pixels (each tap in exactly one class, tested in this order), and of the pixels themselves
TAP_COUNTS = ("outside", "no_hit", "plane", "normal", "prim_alone", "accepted")
COUNTS = TAP_COUNTS + ("valid", "no_candidate", "candidate", "candidate_without_tap", "blended")


def _cam(cam):
    """The fields of an rt.camera the definition reads, as lists of float32 scalars."""
    v3 = lambda f: [F(f.e[a]) for a in range(3)]
    return dict(o=v3(cam.origin), llc=v3(cam.lower_left_corner), hor=v3(cam.horizontal), ver=v3(cam.vertical), u=v3(cam.u), v=v3(cam.v), w=v3(cam.w))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _constants(pc):
    L = [pc["llc"][a] - pc["o"][a] for a in range(3)]
    return _dot(L, pc["u"]), _dot(L, pc["v"]), _dot(L, pc["w"]), _dot(pc["hor"], pc["u"]), _dot(pc["ver"], pc["v"])


class Accumulator:
    """The history of one renderer.  step() is one accumulateFrame call; scalar=True runs the per-pixel restatement instead of the vectorised form."""

    def __init__(self, scalar=False):
        self.scalar = scalar
        self.reset()

    def reset(self):
        self.prev = None
        self.frames = 0

    def step(self, inp, guides, cam, origin, dn, flags=DEMODULATE | SAME_PRIM, max_history=32, sigma_z=0.01, normal_min=0.9, counts=None):
        """inp (ny, nx, 3) float32; guides: the planes of guides_reference for `cam`; origin, dn: centre_dirs for `cam`.  Returns (out, N).  counts: a dict
        whose COUNTS entries are increased by this call's figures."""
        fn = _step_scalar if self.scalar else _step
        out, N, store = fn(self.prev, np.ascontiguousarray(inp, np.float32), guides, origin, dn, flags, F(max_history), F(sigma_z), F(normal_min), counts)
        store["cam"] = _cam(cam)
        self.prev = store
        self.frames += 1
        return out, N


def _step(prev, inp, guides, origin, dn, flags, max_history, sigma_z, normal_min, counts):
    ny, nx = inp.shape[:2]
    n = [np.ascontiguousarray(guides["normal"][..., a], np.float32) for a in range(3)]
    alb = [np.ascontiguousarray(guides["albedo"][..., a], np.float32) for a in range(3)]
    t = np.ascontiguousarray(guides["depth"], np.float32)
    prim = np.ascontiguousarray(guides["prim"], np.int32)
    valid = prim != G.PRIM_NONE
    demod, same_prim = bool(flags & DEMODULATE), bool(flags & SAME_PRIM)
    one, zero = F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        P = [F(origin[a]) + t * dn[..., a] for a in range(3)]
        rz = one / (sigma_z * t)
        m = [np.where(alb[a] > ALBEDO_FLOOR, alb[a], ALBEDO_FLOOR).astype(np.float32) for a in range(3)]
        c0 = [inp[..., a] / m[a] if demod else inp[..., a].copy() for a in range(3)]
        if prev is None:
            c = c0
            N = np.where(valid, one, zero).astype(np.float32)
        else:
            pc = prev["cam"]
            Lu, Lv, Lw, Hl, Vl = _constants(pc)
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
            nsum = np.zeros((ny, nx), np.float32)
            wsum = np.zeros((ny, nx), np.float32)
            for dy in (0, 1):
                for dx in (0, 1):
                    qi, qj = i0 + dx, j0 + dy
                    inside = (qi >= 0) & (qi < nx) & (qj >= 0) & (qj < ny)
                    qi, qj = np.clip(qi, 0, nx - 1), np.clip(qj, 0, ny - 1)
                    bw = (fx if dx else one - fx) * (fy if dy else one - fy)
                    Nq = prev["N"][qj, qi]
                    d = [prev["P"][a][qj, qi] - P[a] for a in range(3)]
                    plane_ok = np.abs(_dot(n, d)) * rz < one
                    normal_ok = _dot(n, [prev["n"][a][qj, qi] for a in range(3)]) >= normal_min
                    prim_ok = (prim == prev["prim"][qj, qi]) if same_prim else np.ones((ny, nx), bool)
                    hit = Nq > zero
                    ok = inside & hit & plane_ok & normal_ok & prim_ok
                    for a in range(3):
                        acc[a] = np.where(ok, acc[a] + bw * prev["c"][a][qj, qi], acc[a]).astype(np.float32)
                    nsum = np.where(ok, nsum + bw * Nq, nsum).astype(np.float32)
                    wsum = np.where(ok, wsum + bw, wsum).astype(np.float32)
                    if counts is not None:
                        left = candidate.copy()
                        for key, passed in (("outside", inside), ("no_hit", hit), ("plane", plane_ok), ("normal", normal_ok), ("prim_alone", prim_ok)):
                            counts[key] = counts.get(key, 0) + int((left & ~passed).sum())
                            left &= passed
                        counts["accepted"] = counts.get("accepted", 0) + int(left.sum())
                        assert np.array_equal(left, candidate & ok)
            use = candidate & (wsum > zero)
            length = nsum / wsum + one
            Nb = np.where(length < max_history, length, max_history).astype(np.float32)
            al = one / Nb
            c = []
            for a in range(3):
                h = acc[a] / wsum
                c.append(np.where(use, h + al * (c0[a] - h), c0[a]).astype(np.float32))
            N = np.where(valid, np.where(use, Nb, one), zero).astype(np.float32)
            if counts is not None:
                for key, val in (("valid", valid), ("no_candidate", valid & ~candidate), ("candidate", candidate), ("candidate_without_tap", candidate & ~use),
                                 ("blended", use)):
                    counts[key] = counts.get(key, 0) + int(val.sum())
        out = np.empty_like(inp)
        for a in range(3):
            out[..., a] = np.where(valid, c[a] * m[a] if demod else c[a], inp[..., a])
    return out, N, dict(P=P, n=n, prim=prim, c=c, N=N)


def _step_scalar(prev, inp, guides, origin, dn, flags, max_history, sigma_z, normal_min, counts):
    """The same call one pixel and one tap at a time on numpy float32 scalars, written from the definition: pins the vectorisation of _step()."""
    ny, nx = inp.shape[:2]
    nrm, alb, dep, prim = guides["normal"], guides["albedo"], guides["depth"], guides["prim"]
    demod, same_prim = bool(flags & DEMODULATE), bool(flags & SAME_PRIM)
    one, zero = F(1.0), F(0.0)
    out = np.array(inp, copy=True)
    N = np.zeros((ny, nx), np.float32)
    sP = [np.zeros((ny, nx), np.float32) for _ in range(3)]
    sn = [np.array(nrm[..., a], np.float32) for a in range(3)]
    sc = [np.zeros((ny, nx), np.float32) for _ in range(3)]
    if prev is not None:
        pc = prev["cam"]
        Lu, Lv, Lw, Hl, Vl = _constants(pc)
    with np.errstate(all="ignore"):
        for j in range(ny):
            for i in range(nx):
                t = F(dep[j, i])
                P = [F(origin[a]) + t * F(dn[j, i, a]) for a in range(3)]
                m = [F(alb[j, i, a]) if F(alb[j, i, a]) > ALBEDO_FLOOR else ALBEDO_FLOOR for a in range(3)]
                c = [F(inp[j, i, a]) / m[a] if demod else F(inp[j, i, a]) for a in range(3)]
                for a in range(3):
                    sP[a][j, i] = P[a]
                if int(prim[j, i]) == G.PRIM_NONE:
                    for a in range(3):
                        sc[a][j, i] = c[a]
                    continue                                    # out = in, N = 0
                Np = one
                if prev is not None:
                    rz = one / (sigma_z * t)
                    npx = [F(nrm[j, i, a]) for a in range(3)]
                    e = [P[a] - pc["o"][a] for a in range(3)]
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
                        acc, nsum, wsum = [zero, zero, zero], zero, zero
                        for dy in (0, 1):
                            for dx in (0, 1):
                                qi, qj = i0 + dx, j0 + dy
                                bw = (fx if dx else one - fx) * (fy if dy else one - fy)
                                if qi < 0 or qi >= nx or qj < 0 or qj >= ny:
                                    continue
                                if not prev["N"][qj, qi] > zero:
                                    continue
                                d = [prev["P"][a][qj, qi] - P[a] for a in range(3)]
                                if not abs(_dot(npx, d)) * rz < one:
                                    continue
                                if not _dot(npx, [prev["n"][a][qj, qi] for a in range(3)]) >= normal_min:
                                    continue
                                if same_prim and int(prim[j, i]) != int(prev["prim"][qj, qi]):
                                    continue
                                acc = [acc[a] + bw * prev["c"][a][qj, qi] for a in range(3)]
                                nsum = nsum + bw * prev["N"][qj, qi]
                                wsum = wsum + bw
                        if wsum > zero:
                            length = nsum / wsum + one
                            Np = length if length < max_history else max_history
                            al = one / Np
                            h = [acc[a] / wsum for a in range(3)]
                            c = [h[a] + al * (c[a] - h[a]) for a in range(3)]
                N[j, i] = Np
                for a in range(3):
                    sc[a][j, i] = c[a]
                    out[j, i, a] = c[a] * m[a] if demod else c[a]
    return out, N, dict(P=sP, n=sn, prim=np.array(prim, np.int32), c=sc, N=N)


# ---------------------------------------------------------------------------------------------
# the camera sequences
# ---------------------------------------------------------------------------------------------

def orbit(lookfrom, lookat, degrees):
    """lookfrom turned about the vertical axis through lookat (counter-clockwise seen from above)."""
    a = math.radians(degrees)
    vx, vy, vz = (lookfrom[k] - lookat[k] for k in range(3))
    return (lookat[0] + math.cos(a) * vx + math.sin(a) * vz, lookat[1] + vy, lookat[2] - math.sin(a) * vx + math.cos(a) * vz)


# name -> (scene frame of guides_reference, camera of frame k); frame 0 is the named frame's own camera
SEQUENCES = ("three_spheres", "random_50x37", "tris300_floor")
MESH_SEQUENCES = ("tris300_floor", "staircase_a")


def sequence_camera(rt, name, k, still=False):
    k = 0 if still else k
    if name == "three_spheres":
        return rt.make_camera(orbit((0, 0, 1), (0, 0, -1), 3.0 * k), (0, 0, -1), (0, 1, 0), 60.0, 64 / 40, 0.0, 2.0)
    if name == "random_50x37":
        return rt.make_camera(orbit((13, 2, 3), (0, 0, 0), 2.0 * k), (0, 0, 0), (0, 1, 0), 30.0, 50 / 37, 0.1, 10.0)
    if name == "tris300_floor":
        return rt.make_camera((30 + 2 * k, 18, 42 - 2 * k), (0, 0, 0), (0, 1, 0), 40.0, 48 / 40, 0.1, 50.0)
    if name == "tie":                                           # the scalar restatement's frame: the camera of guides_reference._tie_scene, 4 degrees per frame
        return rt.make_camera(orbit((0.3, 0.6, 2.5), (0, 0, -1), 4.0 * k), (0, 0, -1), (0, 1, 0), 40.0, 40 / 24, 0.1, 3.0)
    if name == "staircase_a":                                   # two cameras: the frame's own, and the same view with every vector of the lens moved sideways
        cam = rt.staircase_camera(G.STAIR_NX, G.STAIR_NY)
        if k:
            for a in range(3):
                shift = F(0.05 * k) * F(cam.u.e[a])
                cam.origin.e[a] = float(F(cam.origin.e[a]) + shift)
                cam.lower_left_corner.e[a] = float(F(cam.lower_left_corner.e[a]) + shift)
        return cam
    raise KeyError(name)


def _size(rt, O, name):
    if name in G.MESH_FRAMES:
        f = G.mesh_frame(rt, O, name)
        return f["nx"], f["ny"]
    return G.sphere_frame(rt, name)[3:]


@functools.lru_cache(maxsize=None)
def sequence_inputs(rt, O, name, k, still=False):
    """(camera, guides, origin, dn) of frame k of a sequence, with the default options of the scene kind (and the floor of the *_floor frame)."""
    cam = sequence_camera(rt, name, k, still)
    nx, ny = _size(rt, O, name)
    if name in G.MESH_FRAMES:
        f = G.mesh_frame(rt, O, name)
        g = G.mesh_guides(rt, O, f["hm"], f["mats"], f["tex"], cam, nx, ny, floor=f["floor"])
    else:
        sp, mt = G.sphere_frame(rt, name)[:2]
        g = G.sphere_guides(rt, O, sp, mt, cam, nx, ny)
    origin, dn = D.centre_dirs(rt, O, cam, nx, ny)
    return cam, g, origin, dn
