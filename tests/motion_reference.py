"""The test reference of rtMarkPose / renderMotion (include/rt_api.h).  No test: read by tests/test_motion_api.py (CPU: the restatements pinned
against the two existing references, the coverage conditions, what the definition buys) and tests/test_gpu_motion.py (GPU: every plane and every call, all
pixels, bit for bit).

The definition of the interface in numpy float32, vectorised over the pixels of the image: every product, sum, difference, quotient and sqrt is a ufunc call
of its own on float32 operands, so nothing is fused and nothing is reordered; a comparison with a NaN is false.  Nothing of the code under test is used: the
guide planes come from guides_reference, the centre ray's direction from denoise_reference.centre_dirs, the host triangles from HostMesh.refit() / .rebuild().
MotionAccumulator and MotionPreviewer restate the _step of accumulate_reference and of preview_reference with Pm(p), nm(p) in the place of P(p), n(p) in
exactly three places - the reprojection, the tap's plane test, the tap's normal test; with Pm = P and nm = n they are those references bit for bit
(tests/test_motion_api.py)."""
import functools
import math

import numpy as np

import accumulate_reference as A
import denoise_reference as D
import guides_reference as G
import preview_reference as PR

F = np.float32
POS, NORMAL, SCREEN = 1, 2, 4
DEMODULATE, SAME_PRIM = D.DEMODULATE, D.SAME_PRIM
ALBEDO_FLOOR = D.ALBEDO_FLOOR
MOVED_IDS = (12, 19)                    # the mesh ids of staircase_a the edit moves
_dot = A._dot


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]]


def _unit(v):
    l = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return [v[0] / l, v[1] / l, v[2] / l]


def hit_points(guides, origin, dn):
    """P(p) of the accumulate kernel as a list of three (ny, nx) planes."""
    t = np.ascontiguousarray(guides["depth"], np.float32)
    with np.errstate(all="ignore"):
        return [F(origin[a]) + t * dn[..., a] for a in range(3)]


# ---------------------------------------------------------------------------------------------
# the edits
# ---------------------------------------------------------------------------------------------

def is_real(tris):
    return ~np.isinf(tris["v"][:, 0, 0])


def turn_and_shift(tris, sel, extent, degrees=4.0, shift=(0.02, 0.0, 0.01)):
    """A copy of `tris` with the triangles `sel` (a boolean mask over the slots) turned by `degrees` about the vertical axis through the float32 mean of their
    vertices, then shifted by `shift` times `extent` (the scene bounds' extents), all in float32."""
    out = tris.copy()
    v = out["v"][sel].astype(np.float32)                         # (m, 3 vertices, 3 axes)
    centre = v.reshape(-1, 3).mean(axis=0, dtype=np.float32)
    c, s = F(math.cos(math.radians(degrees))), F(math.sin(math.radians(degrees)))
    dx, dz = v[..., 0] - centre[0], v[..., 2] - centre[2]
    moved = v.copy()
    moved[..., 0] = (centre[0] + c * dx + s * dz) + F(shift[0]) * F(extent[0])
    moved[..., 1] = v[..., 1] + F(shift[1]) * F(extent[1])
    moved[..., 2] = (centre[2] - s * dx + c * dz) + F(shift[2]) * F(extent[2])
    out["v"][sel] = moved.astype(np.float32)
    return out


def extent_of(hm):
    return [F(hm.view.bounds.max.e[a]) - F(hm.view.bounds.min.e[a]) for a in range(3)]


@functools.lru_cache(maxsize=None)
def stair_pose(rt, O, k, rebuilt=False):
    """Frame k of the animated staircase_a: a HostMesh of its own with the edit applied k times (cumulatively) to the triangles of MOVED_IDS and refitted, and
    the slot arrays (live, previous): the triangles of frame k and of frame k - 1 in the slots of frame k.  rebuilt: the mesh of frame k is rebuilt after the
    edit (HostMesh.rebuild()), and `previous` is permuted by its old_slot - a sentinel where old_slot < 0.  Returns (hm, live, previous, old_slot or None)."""
    tris, _ = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    ext = extent_of(hm)
    sel = is_real(hm.tris) & np.isin(hm.tris["meshID"], MOVED_IDS)
    poses = [hm.tris.copy()]
    for _ in range(k):
        poses.append(turn_and_shift(poses[-1], sel, ext))
    hm.tris[:] = poses[-1]
    hm.refit()
    previous = poses[-2] if k else poses[-1]
    old_slot = None
    if rebuilt:
        old_slot = hm.rebuild()
        previous = permuted_mark(rt, previous, old_slot)
    return hm, hm.tris.copy(), previous, old_slot


def permuted_mark(rt, mark, old_slot):
    """The mark after a rebuild: slot s holds the old mark of old_slot[s], a sentinel where old_slot[s] < 0."""
    out = mark[np.clip(old_slot, 0, len(mark) - 1)].copy()
    gone = old_slot < 0
    sentinel = np.zeros(1, rt.triangle_dtype)
    sentinel["v"] = np.inf
    out[gone] = sentinel[0]
    return out


@functools.lru_cache(maxsize=None)
def stair_inputs(rt, O, k, rebuilt=False):
    """(camera k of the staircase_a sequence, guide planes of frame k's mesh, origin, dn, live, previous) - the inputs of frame k of the animated staircase."""
    f = G.mesh_frame(rt, O, "staircase_a")
    hm, live, previous, _ = stair_pose(rt, O, k, rebuilt)
    cam = A.sequence_camera(rt, "staircase_a", k)
    g = G.mesh_guides(rt, O, hm, f["mats"], f["tex"], cam, f["nx"], f["ny"])
    origin, dn = D.centre_dirs(rt, O, cam, f["nx"], f["ny"])
    return cam, g, origin, dn, live, previous


def tiny_camera(rt, nx, ny, k):
    """Camera k of the tiny tris300_floor frames: low and close, so that the frame holds triangles, the floor below them and the sky above."""
    return rt.make_camera((10 + 0.5 * k, -2, 12 - 0.5 * k), (0, -2, 0), (0, 1, 0), 40.0, nx / ny, 0.1, 20.0)


@functools.lru_cache(maxsize=None)
def tiny_frame(rt, O, nx, ny):
    """tris300_floor at nx x ny as a HostMesh of its own, under tiny_camera 0 and 1.  Of the triangles camera 1 sees, every other one by pixel count (the most
    seen first; 20 at the most, filled up to 20 with unseen ones) is turned and shifted for frame 1.  Returns dict(f: the frame of guides_reference, hm: the
    mesh of frame 1, first, live: the slot arrays of frame 0 and 1, cams, g, origin, dn: the guide planes and centre rays of frame 1, count: triangles moved)."""
    f = G.mesh_frame(rt, O, "tris300_floor")
    hm = rt.HostMesh.build(f["hm"].tris[is_real(f["hm"].tris)].copy(), 5)
    first = hm.tris.copy()
    cams = [tiny_camera(rt, nx, ny, k) for k in range(2)]
    g = G.mesh_guides(rt, O, hm, f["mats"], f["tex"], cams[1], nx, ny, floor=f["floor"])
    seen, counts = np.unique(g["prim"][g["prim"] >= 0], return_counts=True)
    order = [int(s) for s in seen[np.argsort(-counts, kind="stable")]][0::2][:20]
    order += [int(s) for s in np.flatnonzero(is_real(first)) if s not in set(int(q) for q in seen)][:20 - len(order)]
    sel = np.zeros(len(first), bool)
    sel[order] = True
    live = turn_and_shift(first, sel, extent_of(hm))
    hm.tris[:] = live
    hm.refit()
    g = G.mesh_guides(rt, O, hm, f["mats"], f["tex"], cams[1], nx, ny, floor=f["floor"])
    origin, dn = D.centre_dirs(rt, O, cams[1], nx, ny)
    return dict(f=f, hm=hm, first=first, live=live, cams=cams, g=g, origin=origin, dn=dn, count=int(sel.sum()))


def moved_spheres(spheres, idx, k, resized=2):
    """A copy of the spheres with those of `idx` shifted k times by (0.15, 0.05, -0.1), the first `resized` of them also grown by 10 % per step, in float32."""
    out = spheres.copy()
    idx = np.asarray(idx)
    for _ in range(k):
        out["center"][idx] = (out["center"][idx] + np.array([0.15, 0.05, -0.1], np.float32)).astype(np.float32)
        out["radius"][idx[:resized]] = (out["radius"][idx[:resized]] * F(1.1)).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def sphere_inputs(rt, O, k):
    """Frame k of the animated random_50x37: camera k of its sequence and the eight most seen spheres beside the ground moved k times, two of them resized.
    Returns (camera, guide planes, origin, dn, live spheres, previous spheres, materials, the moved indices)."""
    sp, mt, _, nx, ny = G.sphere_frame(rt, "random_50x37")
    prim = G.reference(rt, O, "random_50x37")["prim"]
    seen, counts = np.unique(prim[prim > 0], return_counts=True)       # (sphere 0 is the ground)
    idx = tuple(int(s) for s in seen[np.argsort(-counts, kind="stable")][:8])
    live, previous = moved_spheres(sp, idx, k), moved_spheres(sp, idx, max(k - 1, 0))
    cam = A.sequence_camera(rt, "random_50x37", k)
    g = G.sphere_guides(rt, O, live, mt, cam, nx, ny)
    origin, dn = D.centre_dirs(rt, O, cam, nx, ny)
    return cam, g, origin, dn, live, previous, mt, idx


# ---------------------------------------------------------------------------------------------
# the motion planes
# ---------------------------------------------------------------------------------------------

def motion_planes(guides, origin, dn, live=None, mark=None, prev_cam=None):
    """The planes of renderMotion for the guide planes of the current camera.  live, mark: the leaf-ordered triangle arrays (triangle_dtype) or the caller-order
    sphere arrays (sphere_dtype) now and as rtMarkPose saw them; mark None = no pose is marked.  prev_cam: C' of the screen plane (the caller passes the
    current camera for renderMotion's NULL).  Returns dict(Pm, nm: lists of three (ny, nx) planes; prev_pos, prev_normal (ny, nx, 3); screen (ny, nx, 2) with
    prev_cam; moved: the pixels that took the moved branch; turned: those of them whose marked normal was negated)."""
    prim = np.ascontiguousarray(guides["prim"], np.int32)
    ny, nx = prim.shape
    n = [np.ascontiguousarray(guides["normal"][..., a], np.float32) for a in range(3)]
    valid = prim != G.PRIM_NONE
    zero = F(0.0)
    P = hit_points(guides, origin, dn)
    Pm, nm = [p.copy() for p in P], [c.copy() for c in n]
    moved = np.zeros((ny, nx), bool)
    turned = np.zeros((ny, nx), bool)
    with np.errstate(all="ignore"):
        if mark is not None and "v" in mark.dtype.names:
            idx = np.clip(prim, 0, len(live) - 1)
            v, a = live["v"][idx].astype(np.float32), mark["v"][idx].astype(np.float32)        # (ny, nx, vertex, axis)
            differs = (_bits(v) != _bits(a)).reshape(ny, nx, 9).any(axis=-1)
            moved = (prim >= 0) & (prim < len(live)) & differs & ~np.isinf(a[..., 0, 0])
            v0, v1, v2 = ([v[..., k, c] for c in range(3)] for k in range(3))
            a0, a1, a2 = ([a[..., k, c] for c in range(3)] for k in range(3))
            e1 = [v1[c] - v0[c] for c in range(3)]
            e2 = [v2[c] - v0[c] for c in range(3)]
            w = [P[c] - v0[c] for c in range(3)]
            d11, d12, d22, d1w, d2w = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(e1, w), _dot(e2, w)
            den = d11 * d22 - d12 * d12
            bu = (d22 * d1w - d12 * d2w) / den
            bv = (d11 * d2w - d12 * d1w) / den
            f1 = [a1[c] - a0[c] for c in range(3)]
            f2 = [a2[c] - a0[c] for c in range(3)]
            gm = _unit(_cross(f1, f2))
            turned = moved & (_dot(_cross(e1, e2), n) < zero)
            for c in range(3):
                Pm[c] = np.where(moved, a0[c] + bu * f1[c] + bv * f2[c], P[c]).astype(np.float32)
                nm[c] = np.where(moved, np.where(turned, -gm[c], gm[c]), n[c]).astype(np.float32)
        elif mark is not None:
            idx = np.clip(prim, 0, len(live) - 1)
            lc, lr = live["center"][idx].astype(np.float32), live["radius"][idx].astype(np.float32)
            mc, mr = mark["center"][idx].astype(np.float32), mark["radius"][idx].astype(np.float32)
            differs = (_bits(lc) != _bits(mc)).any(axis=-1) | (_bits(lr) != _bits(mr))
            moved = (prim >= 0) & (prim < len(live)) & differs
            for c in range(3):
                Pm[c] = np.where(moved, mc[..., c] + ((P[c] - lc[..., c]) / lr) * mr, P[c]).astype(np.float32)
        for c in range(3):
            Pm[c] = np.where(valid, Pm[c], zero).astype(np.float32)
            nm[c] = np.where(valid, nm[c], zero).astype(np.float32)
        res = dict(Pm=Pm, nm=nm, prev_pos=np.stack(Pm, axis=-1), prev_normal=np.stack(nm, axis=-1), moved=moved, turned=turned, P=P)
        if prev_cam is not None:
            pc = A._cam(prev_cam)
            x, y, r = reproject(Pm, pc, nx, ny)
            jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
            seen = valid & (r > zero)
            res["screen"] = np.stack([np.where(seen, x - ii.astype(np.float32), zero), np.where(seen, y - jj.astype(np.float32), zero)], axis=-1).astype(np.float32)
    return res


def reproject(Pm, pc, nx, ny):
    """x, y, r of accumulateFrame's definition for the points Pm and the camera fields pc (accumulate_reference._cam)."""
    Lu, Lv, Lw, Hl, Vl = A._constants(pc)
    e = [Pm[a] - pc["o"][a] for a in range(3)]
    ea, eb, ec = _dot(e, pc["u"]), _dot(e, pc["v"]), _dot(e, pc["w"])
    r = Lw / ec
    s = (ea * r - Lu) / Hl
    tt = (eb * r - Lv) / Vl
    return s * F(nx) - F(0.5), tt * F(ny) - F(0.5), r


# ---------------------------------------------------------------------------------------------
# the passes with a pose marked
# ---------------------------------------------------------------------------------------------

def _temporal(prev, valid, prim, P, n, Pm, nm, rz, c0, extra0, flags, max_history, normal_min, nx, ny, info):
    """Stage T of both passes with (Pm, nm) in the three places: returns (c, N, use, blended extras).  extra0: the per-pixel quantities accumulated beside the
    colour (the moments of previewFrame; none for accumulateFrame) as a dict name -> (this frame's value, the key of the previous call's plane)."""
    same_prim = bool(flags & SAME_PRIM)
    one, zero = F(1.0), F(0.0)
    if prev is None:
        return c0, np.where(valid, one, zero).astype(np.float32), np.zeros((ny, nx), bool), {k: v0 for k, (v0, _) in extra0.items()}
    pc = prev["cam"]
    x, y, r = reproject(Pm, pc, nx, ny)                         # (1) the reprojection: e = Pm - o'
    candidate = valid & (r > zero) & (x >= F(-1.0)) & (x < F(nx)) & (y >= F(-1.0)) & (y < F(ny))
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    i0 = np.where(candidate, x0, zero).astype(np.int64)
    j0 = np.where(candidate, y0, zero).astype(np.int64)
    acc = [np.zeros((ny, nx), np.float32) for _ in range(3)]
    nsum = np.zeros((ny, nx), np.float32)
    wsum = np.zeros((ny, nx), np.float32)
    esum = {k: np.zeros((ny, nx), np.float32) for k in extra0}
    for dy in (0, 1):
        for dx in (0, 1):
            qi, qj = i0 + dx, j0 + dy
            inside = (qi >= 0) & (qi < nx) & (qj >= 0) & (qj < ny)
            qi, qj = np.clip(qi, 0, nx - 1), np.clip(qj, 0, ny - 1)
            bw = (fx if dx else one - fx) * (fy if dy else one - fy)
            Nq = prev["N"][qj, qi]
            d = [prev["P"][a][qj, qi] - Pm[a] for a in range(3)]
            plane_ok = np.abs(_dot(nm, d)) * rz < one            # (2) the plane test: abs(dot(nm, P'(q) - Pm)) * rz(p) < 1
            normal_ok = _dot(nm, [prev["n"][a][qj, qi] for a in range(3)]) >= normal_min      # (3) the normal test
            ok = inside & (Nq > zero) & plane_ok & normal_ok
            if same_prim:
                ok = ok & (prim == prev["prim"][qj, qi])
            for a in range(3):
                acc[a] = np.where(ok, acc[a] + bw * prev["c"][a][qj, qi], acc[a]).astype(np.float32)
            nsum = np.where(ok, nsum + bw * Nq, nsum).astype(np.float32)
            wsum = np.where(ok, wsum + bw, wsum).astype(np.float32)
            for k, (_, key) in extra0.items():
                esum[k] = np.where(ok, esum[k] + bw * prev[key][qj, qi], esum[k]).astype(np.float32)
    use = candidate & (wsum > zero)
    length = nsum / wsum + one
    Nb = np.where(length < max_history, length, max_history).astype(np.float32)
    al = one / Nb
    c, hs = [], []
    for a in range(3):
        h = acc[a] / wsum
        hs.append(h)
        c.append(np.where(use, h + al * (c0[a] - h), c0[a]).astype(np.float32))
    extras = {}
    for k, (v0, _) in extra0.items():
        h = esum[k] / wsum
        extras[k] = np.where(use, h + al * (v0 - h), v0).astype(np.float32)
    N = np.where(valid, np.where(use, Nb, one), zero).astype(np.float32)
    if info is not None:
        info.update(h=hs, use=use, candidate=candidate, x=x, y=y)
    return c, N, use, extras


def _prologue(inp, guides, origin, dn, flags, sigma_z):
    n = [np.ascontiguousarray(guides["normal"][..., a], np.float32) for a in range(3)]
    alb = [np.ascontiguousarray(guides["albedo"][..., a], np.float32) for a in range(3)]
    t = np.ascontiguousarray(guides["depth"], np.float32)
    prim = np.ascontiguousarray(guides["prim"], np.int32)
    valid = prim != G.PRIM_NONE
    demod = bool(flags & DEMODULATE)
    P = [F(origin[a]) + t * dn[..., a] for a in range(3)]
    rz = F(1.0) / (sigma_z * t)
    m = [np.where(alb[a] > ALBEDO_FLOOR, alb[a], ALBEDO_FLOOR).astype(np.float32) for a in range(3)]
    c0 = [inp[..., a] / m[a] if demod else inp[..., a].copy() for a in range(3)]
    return n, prim, valid, demod, P, rz, m, c0


class MotionAccumulator:
    """accumulate_reference.Accumulator with a marked pose: step() takes the motion planes of the call (Pm, nm: lists of three planes; None = P, n)."""

    def __init__(self):
        self.prev = None
        self.frames = 0

    def step(self, inp, guides, cam, origin, dn, Pm=None, nm=None, flags=DEMODULATE | SAME_PRIM, max_history=32, sigma_z=0.01, normal_min=0.9, info=None):
        inp = np.ascontiguousarray(inp, np.float32)
        ny, nx = inp.shape[:2]
        with np.errstate(all="ignore"):
            n, prim, valid, demod, P, rz, m, c0 = _prologue(inp, guides, origin, dn, flags, F(sigma_z))
            c, N, use, _ = _temporal(self.prev, valid, prim, P, n, P if Pm is None else Pm, n if nm is None else nm, rz, c0, {}, flags, F(max_history),
                                     F(normal_min), nx, ny, info)
            out = np.empty_like(inp)
            for a in range(3):
                out[..., a] = np.where(valid, c[a] * m[a] if demod else c[a], inp[..., a])
        self.prev = dict(P=P, n=n, prim=prim, c=c, N=N, cam=A._cam(cam))      # the records of the next call: the CURRENT P, n
        self.frames += 1
        return out, N


class MotionPreviewer:
    """preview_reference.Previewer with a marked pose: stage T takes the motion planes of the call, stages V and A are restated as they are."""

    def __init__(self):
        self.prev = None
        self.frames = 0

    def step(self, inp, guides, cam, origin, dn, Pm=None, nm=None, flags=DEMODULATE | SAME_PRIM, max_history=32, iterations=5, normal_squarings=5, sigma_z=0.01,
             normal_min=0.9, sigma_l=4.0, info=None):
        inp = np.ascontiguousarray(inp, np.float32)
        ny, nx = inp.shape[:2]
        sigma_z, sigma_l = F(sigma_z), F(sigma_l)
        one, zero = F(1.0), F(0.0)
        K, lum, max0 = PR.K, PR.lum, PR._max0
        jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        with np.errstate(all="ignore"):
            n, prim, valid, demod, P, rz, m, c0 = _prologue(inp, guides, origin, dn, flags, sigma_z)
            same_prim = bool(flags & SAME_PRIM)
            l0 = lum(c0)
            q0 = l0 * l0
            c, N, use, ex = _temporal(self.prev, valid, prim, P, n, P if Pm is None else Pm, n if nm is None else nm, rz, c0,
                                      {"M1": (l0, "M1"), "M2": (q0, "M2")}, flags, F(max_history), F(normal_min), nx, ny, info)
            M1, M2 = ex["M1"], ex["M2"]
            store = dict(P=P, n=n, prim=prim, c=c, N=N, M1=M1, M2=M2, cam=A._cam(cam))
            # ---- stage V ----
            temporal = valid & (N >= PR.MIN_HISTORY)
            spatial = valid & ~(N >= PR.MIN_HISTORY)
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
                        wn = max0(_dot(n, [n[a][qj, qi] for a in range(3)]))
                        for _ in range(normal_squarings):
                            wn = wn * wn
                        e = [P[a][qj, qi] - P[a] for a in range(3)]
                        wz = max0(one - np.abs(_dot(n, e)) * rz)
                        wz = wz * wz
                        w = wn * wz
                        if same_prim:
                            w = np.where(prim != prim[qj, qi], zero, w).astype(np.float32)
                    s1 = np.where(ok, s1 + w * M1[qj, qi], s1).astype(np.float32)
                    s2 = np.where(ok, s2 + w * M2[qj, qi], s2).astype(np.float32)
                    ws = np.where(ok, ws + w, ws).astype(np.float32)
            a1, a2 = s1 / ws, s2 / ws
            var_s = max0(a2 - a1 * a1) * (F(4.0) / N)
            var_t = max0(M2 - M1 * M1)
            var = np.where(temporal, var_t, np.where(spatial, var_s, zero)).astype(np.float32)
            variance = var.copy()
            # ---- stage A ----
            for it in range(int(iterations)):
                s = 1 << it
                rl = one / (sigma_l * np.sqrt(var) + PR.LUM_EPS)
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
                            wn = max0(_dot(n, [n[a][qj, qi] for a in range(3)]))
                            for _ in range(normal_squarings):
                                wn = wn * wn
                            e = [P[a][qj, qi] - P[a] for a in range(3)]
                            wz = max0(one - np.abs(_dot(n, e)) * rz)
                            wz = wz * wz
                            w = h * wn * wz
                            wl = max0(one - np.abs(lc - lc[qj, qi]) * rl)
                            wl = wl * wl
                            w = w * wl
                            if same_prim:
                                w = np.where(prim != prim[qj, qi], zero, w).astype(np.float32)
                        for a in range(3):
                            acc[a] = np.where(ok, acc[a] + w * cq[a], acc[a]).astype(np.float32)
                        vsum = np.where(ok, vsum + (w * w) * var[qj, qi], vsum).astype(np.float32)
                        wsum = np.where(ok, wsum + w, wsum).astype(np.float32)
                c = [np.where(valid, acc[a] / wsum, c[a]).astype(np.float32) for a in range(3)]
                var = np.where(valid, vsum / (wsum * wsum), var).astype(np.float32)
            out = np.empty_like(inp)
            for a in range(3):
                out[..., a] = np.where(valid, c[a] * m[a] if demod else c[a], inp[..., a])
        self.prev = store
        self.frames += 1
        return out, N, variance
