"""The test reference of displayFrame (include/rt_api.h): the definition restated in numpy float32, one rounded operation per numpy operation, in the order
written.  powf goes through ctypes to libm.so.6's powf, element by element: numpy's own float32 power may be a SIMD routine with other bits.  No test: a plain
module, imported by tests/test_display_api.py (against rtDisplayFrameHost) and tests/test_gpu_display.py (against displayFrame); the frames and cases both use
are here too, so the CPU twin and the device are held against the same inputs, and so is the one comparison of a displayFrame call every GPU test makes
(check) and the frame of tests/test_gpu_capped_grids.py whose median depends on the pixels past the histogram kernel's first round (round_two_frame)."""
import ctypes as C
import functools
import itertools

import numpy as np

F = np.float32
TOP_DOWN, DITHER, AUTO_EXPOSURE, FROM_PREVIEW = 1, 2, 4, 8
NONE, REINHARD, ACES = 0, 1, 2
BINS, KEY = 256, F(0.18)
BIAS = (127 - 16) << 3
BAYER8 = np.array([[0, 32, 8, 40, 2, 34, 10, 42], [48, 16, 56, 24, 50, 18, 58, 26], [12, 44, 4, 36, 14, 46, 6, 38], [60, 28, 52, 20, 62, 30, 54, 22],
                   [3, 35, 11, 43, 1, 33, 9, 41], [51, 19, 59, 27, 49, 17, 57, 25], [15, 47, 7, 39, 13, 45, 5, 37], [63, 31, 55, 23, 61, 29, 53, 21]], np.uint8)
GAMMA = F(0.416666667)

_libm = C.CDLL("libm.so.6")
_libm.powf.argtypes = [C.c_float, C.c_float]
_libm.powf.restype = C.c_float


def powf(x, y=GAMMA):
    """libm's powf on every element of a float32 array."""
    x = np.ascontiguousarray(x, F)
    f, y = _libm.powf, float(y)
    return np.array([f(v, y) for v in x.ravel().tolist()], F).reshape(x.shape)


def lum(x):
    return F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1] + F(0.0722) * x[..., 2]


def max0(x):
    return np.where(x > 0, x, F(0))                             # 0 for a NaN


def bins_of(frame):
    """(b, counted) per pixel: the bin index before the clamp to BINS - 1, and whether the pixel is counted."""
    with np.errstate(all="ignore"):
        l = np.ascontiguousarray(lum(np.asarray(frame, F)))
    b = (l.view(np.uint32) >> 20).astype(np.int64) - BIAS
    return b, np.isfinite(l) & (l > 0) & (b >= 0)


def histogram(frame):
    b, counted = bins_of(frame)
    return np.bincount(np.minimum(b[counted], BINS - 1), minlength=BINS).astype(np.uint32)


def target_of(hist):
    total = int(hist.astype(np.int64).sum())
    if total == 0:
        return F(1)
    cum = np.cumsum(hist.astype(np.int64))
    m = int(np.argmax(2 * cum >= total))
    lmed = np.array(((m + BIAS) << 20) | (1 << 19), np.uint32).view(F)
    return F(KEY / lmed)


def transform(frame, E_used, flags=0, tonemap=NONE):
    """The per-pixel half: (ny, nx, 3) float32 -> (ny, nx, 4) uint8."""
    frame, E_used = np.asarray(frame, F), F(E_used)
    ny, nx = frame.shape[:2]
    with np.errstate(all="ignore"):
        y = frame * E_used
        if tonemap == REINHARD:
            y = y / (F(1) + max0(lum(y)))[..., None]
        elif tonemap == ACES:
            a = max0(y)
            y = (a * (F(2.51) * a + F(0.03))) / (a * (F(2.43) * a + F(0.59)) + F(0.14))
        s = max0(y)
        s = max0(F(1.055) * powf(s) - F(0.055))
        if flags & DITHER:
            j, i = np.mgrid[0:ny, 0:nx]
            d = (BAYER8[j & 7, i & 7].astype(F) + F(0.5)) / F(64)
            t = s * F(255) + d[..., None]
        else:
            t = s * F(255.9)
        u = np.where(t >= F(255), 255, np.where(t >= F(255), F(0), t).astype(np.uint32))
    out = np.full((ny, nx, 4), 255, np.uint8)
    out[..., :3] = u.astype(np.uint8)
    return out[::-1].copy() if flags & TOP_DOWN else out


class Display:
    """displayFrame's state and one call of it: step returns (rgba, E_used, histogram or None)."""

    def __init__(self):
        self.E = None                                           # E' of the auto exposure; None = adapt from nothing

    def reset(self):
        self.E = None

    def step(self, frame, flags=0, tonemap=NONE, exposure=1.0, adapt=1.0):
        exposure, adapt, hist = F(exposure), F(adapt), None
        E_used = exposure
        if flags & AUTO_EXPOSURE:
            hist = histogram(frame)
            target = target_of(hist)
            self.E = target if self.E is None else F(self.E + F(adapt * F(target - self.E)))
            E_used = F(self.E * exposure)
        return transform(frame, E_used, flags, tonemap), E_used, hist


# ---- the frames and cases of the tests ---------------------------------------------------------------------------------

SIZES = ((1, 1), (3, 2), (65, 1), (1, 65), (50, 37), (130, 67))           # (nx, ny): both sides of a wave, of a workgroup, of the 8 x 8 dither tile; an odd ny
FLAG_SETS = (0, TOP_DOWN, DITHER, AUTO_EXPOSURE, TOP_DOWN | DITHER | AUTO_EXPOSURE)
CASES = tuple(itertools.product((NONE, REINHARD, ACES), FLAG_SETS))
_K = (F(0.2126), F(0.7152), F(0.0722))


def pixel_with_luminance(L):
    """A pixel with one non-zero channel whose lum() is exactly the float32 L (the other two terms are +0)."""
    L = F(L)
    for c in (1, 0, 2):
        w = int(F(L / _K[c]).view(np.uint32))
        for d in range(-8, 9):
            g = np.uint32(w + d).view(F)
            if F(_K[c] * g) == L:
                px = np.zeros(3, F)
                px[c] = g
                return px
    raise ValueError(L)


def edge_pixels():
    """Pixels around the histogram's edges: luminance exactly 2^-16 (first bin's lower edge), one ulp below it (not counted), the first bin's upper edge
    (second bin), 2^16 and above (all in the last bin), exactly on inner edges, a negative and a mixed-sign pixel, zero."""
    below = np.uint32(int(F(2.0 ** -16).view(np.uint32)) - 1).view(F)
    lums = [2.0 ** -16, below, 2.0 ** -16 * 1.125, 2.0 ** -16 * 1.0625, 2.0 ** 16, 2.0 ** 16 * (1 - 2.0 ** -24), 2.0 ** 19, 1.0, 1.125, 0.5 * 1.875, 2.0 ** -3 * 1.25]
    px = [pixel_with_luminance(L) for L in lums]
    px += [np.array(v, F) for v in ((-0.5, -0.25, -1.0), (-2.0, 0.5, 0.25), (0.75, -0.01, 0.3), (0.0, 0.0, 0.0), (-0.0, 0.0, 3.0e-6))]
    return np.array(px, F)


@functools.lru_cache(maxsize=None)
def _synthetic(seed, nx, ny, scale):
    rng = np.random.default_rng(seed)
    a = (2.0 ** rng.uniform(-20, 20, (ny, nx, 1)) * rng.uniform(0.5, 1.5, (ny, nx, 3)) * scale).astype(F)
    flat = a.reshape(-1, 3)
    edge = edge_pixels()
    n = min(len(edge), len(flat) // 2)                          # (the smallest sizes keep at least half of their random pixels)
    if n:
        flat[rng.permutation(len(flat))[:n]] = edge[:n] if scale == 1.0 else edge[:n] * F(scale)
    neg = rng.random((ny, nx, 3)) < 0.05                        # negative channels among the random ones
    a[neg] = -a[neg]
    a.setflags(write=False)
    return a


def synthetic(seed, nx, ny, scale=1.0):
    """A seeded (ny, nx, 3) frame: values over 2^-20 .. 2^20 (times `scale`), the edge pixels above at random places, 5 % negative channels.  Read-only and
    shared: computed once."""
    return _synthetic(seed, nx, ny, float(scale))


@functools.lru_cache(maxsize=None)
def round_two_frame(seed, nx, ny, first, share=0.65):
    """synthetic(seed, nx, ny) rearranged so that the median bin hangs on the pixels with index >= `first` alone (the ones a grid capped at `first` lanes
    reaches in its second round): returns (frame, (r1, r2)).  r1, r2 are the two bins around the synthetic frame's median.  Pixels below `first` that fall
    in them move 16 bins up (times 4: exact), so that no pixel of the first round is counted there; the pixels from `first` on are given luminances in r1
    (`share` of them) and in r2 (the rest); then pixels of the first round move from above r2 to 32 bins lower (times 2^-4: exact) until
    D = (count above r2) - (count below r1) is 0.45 n.  With x pixels in r1 and n - x in r2 the median bin is
        r2 for the frame as it is     (2 x < D + n and D <= n),
        r1 with the n counted twice   (4 x >= D + 2 n),
        another bin without them      (r1 and r2 are empty then, and the median bin is never an empty one),
    which test_capped_grids_api.py asserts on the result.  Read-only and shared: computed once."""
    a = np.array(synthetic(seed, nx, ny), copy=True)
    flat = a.reshape(-1, 3)
    n = len(flat) - first
    assert 0 < n < first
    b, counted = bins_of(flat)
    cum = np.cumsum(np.bincount(np.minimum(b[counted], BINS - 1), minlength=BINS))
    r1 = int(np.argmax(2 * cum >= cum[-1]))
    r2 = r1 + 1
    head = np.arange(len(flat)) < first
    flat[head & counted & ((b == r1) | (b == r2))] *= F(4)
    x = int(share * n)
    lums = np.array([((r + BIAS) << 20) | (0x1000 + k * 1237 % 0xfe000) for k, r in enumerate([r1] * x + [r2] * (n - x))], np.uint32).view(F)
    flat[first:] = 0                                            # a green pixel whose luminance is within an ulp of one well inside the bin
    flat[first:, 1] = lums / _K[1]
    b, counted = bins_of(flat)
    D = int((counted & (b > r2)).sum()) - int((counted & (b < r1)).sum())
    want = 9 * n // 20                                          # x = 0.65 n lies in [(D + 2 n) / 4, (D + n) / 2) for D in (0.3 n, 0.6 n]: aim at the middle
    assert D >= want, (D, want)                                 # (the median bin itself was emptied upwards, so more lies above than below)
    above = np.flatnonzero(head & counted & (b > r2) & (b <= r2 + 8))[:(D - want) // 2]
    assert len(above) == (D - want) // 2
    flat[above] *= F(2.0 ** -4)
    a.setflags(write=False)
    return a, (r1, r2)


def check(rt, ref, frame, src, flags, tonemap, exposure=1.0, adapt=1.0, what=""):
    """One displayFrame call on both sides, bit for bit: the bytes, rtLastExposure and (with AUTO_EXPOSURE) the histogram.  `ref` is a Display, `frame` is
    what it sees, `src` what displayFrame is given (None: the framebuffer, which holds `frame`).  Returns the bytes."""
    got = rt.display_frame(src, flags=flags, tonemap=tonemap, exposure=exposure, adapt=adapt)
    want, E_used, hist = ref.step(frame, flags, tonemap, exposure, adapt)
    diff = got != want
    print(f"{what} flags {flags} tonemap {tonemap}: {int(diff.sum())} of {diff.size} bytes differ, E_used {rt.last_exposure()!r} / {float(E_used)!r}")
    assert got.shape == want.shape and got.dtype == np.uint8
    assert int(F(rt.last_exposure()).view(np.uint32)) == int(F(E_used).view(np.uint32)), (what, flags, tonemap, rt.last_exposure(), float(E_used))
    if flags & AUTO_EXPOSURE:
        assert np.array_equal(rt.display_histogram(), hist), (what, flags, tonemap)
    assert np.array_equal(got, want), (what, flags, tonemap, int(diff.sum()), np.argwhere(diff)[:5].tolist())
    assert rt.last_display_ms() > 0.0
    return got


SPECIAL_VALUES = (float("nan"), float("inf"), float("-inf"), 1e30, -1e30, 3.4028234e38, 2.0 ** 40, 1e-40, -1e-40, 0.0, -0.0, 1.0, 254.5 / 255.9)


@functools.lru_cache(maxsize=None)
def special_frame():
    """13 x 3: channel k of column v holds SPECIAL_VALUES[v] in row k and 0.25 elsewhere, so every special meets every channel position."""
    a = np.full((3, len(SPECIAL_VALUES), 3), 0.25, F)
    for v, x in enumerate(SPECIAL_VALUES):
        for k in range(3):
            a[k, v, k] = x
    a.setflags(write=False)
    return a
