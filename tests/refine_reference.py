"""The reference of refineFrame (include/rt_api.h): the whole definition in numpy float32, driven only by the CPU oracle's frames at n = batch, 2 batch, ...
samples per pixel - a pixel of the oracle's frame at n is the pixel of the list at n (renderPixels' promise, tests/test_gpu_pixels.py).  No test: a plain
module, imported by tests/test_refine_api.py and tests/test_gpu_refine.py.

Scenes: the tags of tests/pixels_reference.py, and S1_13x5 = S1's three spheres re-initialised at 13 x 5 (65 pixels: one wave + 1, and the 3 x 3 window of
every pixel but the 33 inner ones is clipped by the border), and S1_523x503 = the same spheres at 523 x 503 (263 069 pixels = 1028 workgroups of 256: the
counting and scattering kernels, capped at 1024 workgroups, go round twice, and the second round holds 925 pixels; tests/test_capped_grids_api.py).  CASES holds the parameters the tests run with; the thresholds are chosen and pinned by
tests/test_refine_api.py.

Every operation below is one float32 operation of the header's definition, in its order: numpy rounds each on its own.  max0(x) = x < 0 ? 0 : x keeps a
NaN; a comparison with a NaN is false."""
import functools

import numpy as np

import pixels_reference as PR

F = np.float32
DILATE = 1
LUM_EPS = F(1e-3)
FLT_MAX = np.finfo(np.float32).max

#         tag: (batch, min_batches, max_samples, threshold)
CASES = {"S2": (2, 2, 12, 0.1), "M1": (2, 2, 8, 0.8), "S1_13x5": (2, 2, 10, 0.1), "S1_523x503": (2, 2, 8, 0.0003)}
SMALL = {"S1_13x5": ("S1", 13, 5), "S1_523x503": ("S1", 523, 503)}         # (a scene of pixels_reference at another size)


def size(tag):
    return SMALL[tag][1:] if tag in SMALL else PR.SCENES[tag][:2]


def init(rt, tag, **opts):
    """init* of the tag's scene (PR.init; S1_13x5: the three spheres at 13 x 5); returns the framebuffer view."""
    if tag not in SMALL:
        return PR.init(rt, tag, **opts)
    base, nx, ny = SMALL[tag]
    sp, mt, cam = rt.scene_three_spheres(nx, ny)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, PR.SCENES[base][2])
    rt.setRenderOptions(rt.getDefaultRenderOptions(True), **opts)
    return fb


@functools.lru_cache(maxsize=None)
def oracle_frame(rt, O, tag, n):
    """The oracle's frame of the tag at n samples per pixel, (ny, nx, 3) float32, read-only."""
    if tag not in SMALL:
        return PR.oracle_frame(rt, O, tag, n)[0]
    base, nx, ny = SMALL[tag]
    sp, mt, cam = rt.scene_three_spheres(nx, ny)
    fb, _ = O.render(O.sphere_scene(sp, mt), cam, O.default_options(True), nx, ny, n, PR.SCENES[base][2])
    fb.setflags(write=False)
    return fb


@functools.lru_cache(maxsize=None)
def oracle_rays(rt, O, tag, n):
    """The oracle's rays of every pixel over its first n samples, (ny, nx) uint32, read-only: one region render per pixel, as PR.oracle_planes counts them
    (which serves the tags that are not in SMALL)."""
    if tag not in SMALL:
        return PR.oracle_planes(rt, O, tag, n)[1]
    base, nx, ny = SMALL[tag]
    sp, mt, cam = rt.scene_three_spheres(nx, ny)
    sc, opt, fb = O.sphere_scene(sp, mt), O.default_options(True), np.zeros((ny, nx, 3), np.float32)
    rays = np.zeros((ny, nx), np.uint32)
    for j in range(ny):
        for i in range(nx):
            rays[j, i] = O.render(sc, cam, opt, nx, ny, n, PR.SCENES[base][2], region=(i, j, i + 1, j + 1), counters=True, fb=fb)[1].rays
    rays.setflags(write=False)
    return rays


def classes(rays):
    """The cost class of a last batch's rays: 31 - clz(max(rays, 1)); exact below 2^53."""
    return np.floor(np.log2(np.maximum(np.asarray(rays).astype(np.int64), 1))).astype(np.int64)


def lum(c):
    return F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1] + F(0.0722) * c[..., 2]


def max0(x):
    return np.where(x < 0, F(0), x).astype(F)


def dilate(mask):
    """Some pixel of the 3 x 3 window, clipped to the image, is set."""
    ny, nx = mask.shape
    padded = np.zeros((ny + 2, nx + 2), bool)
    padded[1:-1, 1:-1] = mask
    out = np.zeros_like(mask)
    for dy in range(3):
        for dx in range(3):
            out |= padded[dy:dy + ny, dx:dx + nx]
    return out


class Frame:
    """The adaptive frame of `tag` after a reset.  `frames`: n -> the (ny, nx, 3) float32 frame at n samples per pixel (default: the oracle's of the tag;
    synthetic frames come with their `shape` = (ny, nx) and no tag)."""

    def __init__(self, rt, O, tag, batch, frames=None, shape=None):
        nx, ny = size(tag) if shape is None else shape[::-1]
        self.frames = frames if frames is not None else (lambda n: oracle_frame(rt, O, tag, n))
        self.batch = batch
        self.n = np.zeros((ny, nx), np.int32)
        self.m1, self.m2, self.l = (np.zeros((ny, nx), F) for _ in range(3))
        self.mean = np.zeros((ny, nx, 3), F)
        self.total = 0

    def error(self):
        K = self.n // self.batch
        with np.errstate(all="ignore"):
            Kf = np.maximum(K, 1).astype(F)
            a1, a2 = self.m1 / Kf, self.m2 / Kf
            v = max0(a2 - a1 * a1) / np.maximum(K - 1, 1).astype(F)
            r = max0(self.l) + LUM_EPS
            err = v / (r * r)
        return np.where(K < 2, F(FLT_MAX), err).astype(F)

    def unconverged(self, min_batches, threshold):
        with np.errstate(all="ignore"):
            return (self.n // self.batch < min_batches) | ~(self.error() <= F(threshold) * F(threshold))

    def call(self, min_batches, max_samples, threshold, flags=0):
        """One refineFrame call: (sampled, out, samples, error, active mask)."""
        want = self.unconverged(min_batches, threshold)
        if flags & DILATE:
            want = dilate(want)
        active = want & (self.n + self.batch <= max_samples)
        before = self.n.copy()
        for n0 in np.unique(before[active]):
            m = active & (before == n0)
            n1 = int(n0) + self.batch
            mean = self.frames(n1)[m]
            with np.errstate(all="ignore"):
                l1 = lum(mean)
                y = l1 if n0 == 0 else (l1 * F(n1) - self.l[m] * F(n0)) / F(self.batch)
                self.m1[m] = self.m1[m] + y
                self.m2[m] = self.m2[m] + y * y
            self.mean[m], self.l[m], self.n[m] = mean, l1, n1
        sampled = int(active.sum())
        self.total += sampled * self.batch
        return sampled, self.mean.copy(), self.n.copy(), self.error(), active


def run(rt, O, tag, flags=0, params=None, limit=64, frames=None):
    """The calls of a frame to completion under CASES[tag] (or params): a list of call results, the last one with sampled == 0.  `frames`: as Frame's."""
    batch, min_batches, max_samples, threshold = params or CASES[tag]
    f, calls = Frame(rt, O, tag, batch, frames=frames), []
    while len(calls) < limit:
        calls.append(f.call(min_batches, max_samples, threshold, flags))
        if calls[-1][0] == 0:
            return calls
    raise AssertionError("the frame does not finish")
