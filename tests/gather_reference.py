"""The reference of gatherRadiance (include/rt_api.h, "gathering at points"), restated in numpy.  No test: a plain module, imported by tests/test_gather_api.py
and tests/test_gpu_gather.py.  The xorshift and wang_hash are integer operations (in uint64, masked to 32 bits); everything else is float32 arrays under
+ - * / and sqrt, which numpy rounds one operation at a time - the definition's arithmetic.  The per-ray results come from a callable, so the one reduction
serves every source of L: this library's radianceRays / occludedRays, the CPU oracle, a constant."""
import functools

import numpy as np

IRRADIANCE, SH9, VISIBILITY = 0, 1, 2
WIDTH = {IRRADIANCE: 3, SH9: 27, VISIBILITY: 1}
F = np.float32
M32 = np.uint64(0xFFFFFFFF)


def wang_hash(seed):
    """rnd.h:31-39 on a uint64 array of 32-bit values."""
    s = np.asarray(seed, np.uint64) & M32
    s = (s ^ np.uint64(61)) ^ (s >> np.uint64(16))
    s = (s * np.uint64(9)) & M32
    s = s ^ (s >> np.uint64(4))
    s = (s * np.uint64(0x27d4eb2d)) & M32
    s = s ^ (s >> np.uint64(15))
    return s


def pixel_seed(ids):
    """kernels.cu:541-542."""
    return ((wang_hash(ids) * np.uint64(336343633)) & M32) | np.uint64(1)


def rnd(words):
    """rnd.h:5-18: (the next words, the float32 draws)."""
    x = np.asarray(words, np.uint64)
    x = x ^ ((x << np.uint64(13)) & M32)
    x = x ^ (x >> np.uint64(17))
    x = x ^ ((x << np.uint64(15)) & M32)
    return x, (x & np.uint64(0xFFFFFF)).astype(F) / F(16777216.0)


def ray_ids(n, first, dirs, dirs_total, base_id):
    """g of ray (k, m), shape (n, dirs), as uint64 values below 2^32."""
    k = np.arange(n, dtype=np.uint64)[:, None]
    m = np.arange(first, first + dirs, dtype=np.uint64)[None, :]
    return (np.uint64(base_id) + ((k * np.uint64(dirs_total) + m) & M32)) & M32


def unit_draws(g):
    """u of the direction stream pixel_seed(~g) for every id of the uint64 array g: (u float32 (..., 3), rounds of the rejection loop)."""
    shape = g.shape
    w = pixel_seed((~g.ravel()) & M32)
    n = len(w)
    xyz, l2, rounds = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, np.int64)
    todo = np.arange(n)
    while len(todo):
        ww = w[todo]
        c = []
        for _ in range(3):
            ww, r = rnd(ww)
            c.append(F(2.0) * r - F(1.0))
        w[todo] = ww
        x, y, z = c
        s = x * x + y * y + z * z
        xyz[todo], l2[todo] = np.stack(c, axis=1), s
        rounds[todo] += 1
        todo = todo[~(s < F(1.0)) | (s == F(0.0))]
    assert xyz.dtype == F and l2.dtype == F
    u = xyz / np.sqrt(l2)[:, None]
    assert u.dtype == F
    return u.reshape(shape + (3,)), rounds.reshape(shape)


def unit_normals(nrm):
    nrm = np.asarray(nrm, F)
    l = np.sqrt(nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2])
    assert l.dtype == F
    return nrm / l[:, None]


def directions(pos, nrm, mode, first, dirs, dirs_total, base_id=0, bias=0.0, details=False):
    """(org (n * dirs, 3), D (n * dirs, 3), ids (n * dirs,) uint32) of rtGatherDirections: entry k * dirs + (m - first).  details=True adds the rounds of the
    rejection loops (n * dirs,) and u (n * dirs, 3)."""
    pos = np.asarray(pos, F)
    n = len(pos)
    g = ray_ids(n, first, dirs, dirs_total, base_id)
    u, rounds = unit_draws(g)
    if mode == SH9:
        o = np.repeat(pos[:, None, :], dirs, axis=1)
        D = u
    else:
        nn = unit_normals(nrm)
        o = np.repeat((pos + F(bias) * nn)[:, None, :], dirs, axis=1)
        D = nn[:, None, :] + u
        zero = (D == 0).all(axis=2)
        D[zero] = np.broadcast_to(nn[:, None, :], D.shape)[zero]
    assert o.dtype == F and D.dtype == F
    res = (np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(D.reshape(-1, 3)), g.reshape(-1).astype(np.uint32))
    return res + (rounds.reshape(-1), u.reshape(-1, 3)) if details else res


def sh9(D):
    """y_0 .. y_8 of the raw directions D (n, 3): (n, 9) float32."""
    X, Y, Z = D[:, 0], D[:, 1], D[:, 2]
    y = np.stack([np.full(len(D), F(0.282095)), F(0.488603) * Y, F(0.488603) * Z, F(0.488603) * X, F(1.092548) * (X * Y), F(1.092548) * (Y * Z),
                  F(0.315392) * (F(3.0) * (Z * Z) - F(1.0)), F(1.092548) * (X * Z), F(0.546274) * (X * X - Y * Y)], axis=1)
    assert y.dtype == F
    return y


def reduce(mode, first, dirs, D, L, r, acc=None):
    """The reduction over the per-ray results in entry order k * dirs + j: D (n * dirs, 3), L (n * dirs, 3) - VISIBILITY: v (n * dirs,) -, r (n * dirs,).
    Returns (out (n, W), acc (n, W), rays (n,) uint32)."""
    W = WIDTH[mode]
    n = len(D) // dirs
    A = np.zeros((n, W), F) if first == 0 else np.array(acc, F).reshape(n, W)
    D, L = D.reshape(n, dirs, 3), np.asarray(L, F).reshape((n, dirs) + ((3,) if mode != VISIBILITY else ()))
    for j in range(dirs):
        if mode == IRRADIANCE:
            A = A + L[:, j]
        elif mode == VISIBILITY:
            A = A + L[:, j][:, None]
        else:
            y = sh9(D[:, j])
            A = A + (L[:, j][:, None, :] * y[:, :, None]).reshape(n, 27)      # A[3i + c] += L[c] * y_i
    assert A.dtype == F
    M = F(first + dirs)
    out = (A * F(12.566371)) / M if mode == SH9 else A / M
    rays = np.asarray(r, np.uint64).reshape(n, dirs).sum(axis=1).astype(np.uint32)
    return out.astype(F), A, rays


def gather(pos, nrm, mode, first, dirs, dirs_total, trace, base_id=0, bias=0.0, acc=None):
    """gatherRadiance with the per-ray results from trace(org, D, ids) -> (L (n * dirs, 3) or v (n * dirs,), r (n * dirs,))."""
    org, D, ids = directions(pos, nrm, mode, first, dirs, dirs_total, base_id, bias)
    L, r = trace(org, D, ids)
    return reduce(mode, first, dirs, D, L, r, acc)


# ---- the standard list of the generator's tests --------------------------------------------------------------------------------------

N_POINTS = 70


@functools.lru_cache(maxsize=None)
def standard_points():
    """(pos (70, 3), nrm (70, 3)) float32, read-only: random points; normals that are unnormalised (lengths 0.2 .. 5), axis-aligned (+-x, +-y, +-z, twice
    over), of length 1e-3 (four) and of length 1e3 (four)."""
    rng = np.random.default_rng(301)
    pos = rng.uniform(-5, 5, (N_POINTS, 3)).astype(F)
    v = rng.normal(size=(N_POINTS, 3))
    v = v / np.linalg.norm(v, axis=1)[:, None]
    nrm = v * rng.uniform(0.2, 5.0, N_POINTS)[:, None]
    for k in range(12):
        nrm[10 + k] = 0.0
        nrm[10 + k, k % 3] = (1.0 if (k // 3) % 2 == 0 else -1.0) * (1.0 if k < 6 else 2.5)
    nrm[30:34] = v[30:34] * 1e-3
    nrm[40:44] = v[40:44] * 1e3
    nrm = nrm.astype(F) + F(0.0)
    pos.setflags(write=False)
    nrm.setflags(write=False)
    return pos, nrm
