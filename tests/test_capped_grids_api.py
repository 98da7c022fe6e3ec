"""CPU checks behind tests/test_gpu_capped_grids.py: the two shapes of tests/capped_grids_support.py still sit where the histogram of displayFrame, the
count and scatter of refineFrame and the scan of rasterTexels / bakeTexels change their indexing - the constants are read from the kernel sources, so that
whoever re-tunes a cap is told to move the shapes -, and the inputs of the GPU tests hold, on the references alone, what they are there for: conditions, no
tolerance, so that no GPU comparison can pass vacuously."""
import os
import re

import numpy as np
import pytest

import capped_grids_support as S
import display_reference as D
import refine_reference as RR
import texels_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")
L, E = S.L, S.E


def _constant(name, file):
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, file)).read())
    found = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert len(found) == 1, (name, file, found)
    return int(found[0])


# ---- 0. the shapes --------------------------------------------------------------------------------------------------------------------

def test_the_constants_the_shapes_were_derived_from():
    assert _constant("kHistogramMaxBlocks", "rt_kernels_display.hip") == S.CAP
    assert _constant("kRefineMaxBlocks", "rt_kernels_refine.hip") == S.CAP
    assert _constant("kScanThreads", "rt_kernels_texels.hip") == S.CAP
    assert _constant("kAscendingThreads", "rt_kernels_refine.hip") == 1024
    assert _constant("kDisplayThreads", "rt_kernels_display.hip") == S.GROUP
    assert _constant("kRefineThreads", "rt_kernels_refine.hip") == S.GROUP
    assert _constant("kTexelBlock", "rt_texels.h") == S.GROUP


def test_the_shapes_sit_on_and_just_past_the_cap():
    assert E[0] * E[1] == S.CAP_ITEMS and S.groups_of(E[0] * E[1]) == S.CAP                  # exactly on it: one round, one count per scan lane, none idle
    items = L[0] * L[1]
    assert items == 263069 and S.groups_of(items) == 1028 > S.CAP
    per = (S.groups_of(items) + S.CAP - 1) // S.CAP
    assert per == 2 and (S.groups_of(E[0] * E[1]) + S.CAP - 1) // S.CAP == 1
    second = items - S.CAP_ITEMS                                                              # the second round of a capped grid
    assert second == 925 == 3 * S.GROUP + 157                                                 # workgroups 0 .. 2 full, 3 partial, 1020 without a second round
    assert S.CAP_ITEMS // L[0] == 501 and 0 < S.CAP_ITEMS % L[0] < L[0]                       # the first item of round two lies inside row 501
    for v in L:
        assert all(v % d for d in range(2, int(v ** 0.5) + 1))                                # prime: no row, tile, wave or dither period lines up with a round
    assert S.groups_of(items) // per == 514                                                   # scan lanes 0 .. 513 hold two counts, the lanes from 514 on none
    nx, ny = RR.size("S1_13x5")
    assert nx * ny == 65 < 1024 < items                                                       # the ascending walk: one step, and 257 steps with a partial last one
    assert items % 1024 != 0 and RR.size(S.REFINE_TAG) == L


# ---- 1. displayFrame ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sorted(S.SHAPES))
def test_display_frames_cover_the_edges_and_overflow_16_bits(shape):
    """The synthetic frames of the GPU test: the first and the last bin are populated, pixels lie below the first bin's lower edge (not counted) and above the
    last bin's upper edge (clamped into it).  At scale 1 no bin of 263 069 pixels spread over 40 octaves holds more than some 27 000, so the GPU test adds one
    call on the frame scaled by 2^8, whose last bin holds more than 65 535: no count fits in 16 bits."""
    nx, ny = S.SHAPES[shape]
    frame = D.synthetic(100 + nx, nx, ny)
    b, counted = D.bins_of(frame)
    hist = D.histogram(frame)
    print(shape, "first bin", hist[0], "last bin", hist[-1], "largest", hist.max(), "below", int((b < 0).sum()), "above", int((counted & (b >= D.BINS)).sum()))
    assert hist[0] > 0 and hist[-1] > 0 and (counted & (b >= D.BINS)).any() and (b < 0).any() and (~counted).any()
    assert (hist > 0).all()
    scaled = D.histogram(D.synthetic(100 + nx, nx, ny, 256.0))
    assert scaled[-1] > 65535 and scaled.sum() < nx * ny


def test_the_round_two_frame_hangs_its_median_on_round_two():
    """round_two_frame at L: no pixel of round one is counted in the two bins the 925 pixels of round two fill, and the exposure target differs between the
    frame, the frame without round two (a stride that skips it) and the frame with round two counted twice (a stride one workgroup short)."""
    nx, ny = L
    frame, (r1, r2) = D.round_two_frame(7, nx, ny, S.CAP_ITEMS)
    flat = frame.reshape(-1, 3)
    b, counted = D.bins_of(flat)
    head, tail = flat[:S.CAP_ITEMS], flat[S.CAP_ITEMS:]
    assert len(tail) == 925 and counted[S.CAP_ITEMS:].all() and set(b[S.CAP_ITEMS:].tolist()) == {r1, r2}
    assert not (counted[:S.CAP_ITEMS] & ((b[:S.CAP_ITEMS] == r1) | (b[:S.CAP_ITEMS] == r2))).any()
    whole, without = D.histogram(flat), D.histogram(head)
    twice = (whole.astype(np.int64) + D.histogram(tail)).astype(np.uint32)
    assert whole[r1] + whole[r2] == 925 and without[r1] == without[r2] == 0 and twice[r1] + twice[r2] == 1850
    targets = [float(D.target_of(h)) for h in (whole, without, twice)]
    print("bins", r1, r2, "targets: whole, without round two, round two twice", targets)
    assert len(set(targets)) == 3
    assert (D.histogram(D.synthetic(7, nx, ny)) > 0).all()                                     # the frame it was made from had pixels of round one in every bin


# ---- 2. refineFrame -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, RR.DILATE])
def test_the_refine_case_exercises_round_two_and_the_classes(rt, O, flags):
    """The three spheres at L under RR.CASES (batch 2, min_batches 2, max_samples 8, threshold 3e-4: the rows of round two show the sky, whose error is 0
    or 1e-7, so the threshold is the largest of 0.1, 0.03, 0.01, 0.003, 0.001, 0.0003 under which some pixel of round two stays active), on the oracle's
    whole frames at 2, 4, 6 and 8 samples per pixel and its per-pixel ray counts (6 s in all).  Some pass after the min_batches passes has (a) an active
    set that is neither empty nor the image, (b) active and inactive pixels in round two, (c) at least 3 cost classes, (d) a wave-aligned run of 64 pixels
    with active pixels of at least 2 classes - so a wave of k_refine_scatter issues more than one atomic in a round -, and, for the ascending walk, active
    pixels in its last, partial step."""
    batch, min_batches, max_samples, threshold = RR.CASES[S.REFINE_TAG]
    assert 8 <= max_samples <= 12
    nx, ny = L
    calls = RR.run(rt, O, S.REFINE_TAG, flags)
    assert [c[0] for c in calls[:min_batches]] == [nx * ny] * min_batches and calls[-1][0] == 0
    rays = lambda n: RR.oracle_rays(rt, O, S.REFINE_TAG, n)
    good = []
    before = calls[min_batches - 1][2]
    for k in range(min_batches, len(calls) - 1):
        active = calls[k][4].ravel()
        n0 = before.ravel()
        last = np.zeros(nx * ny, np.int64)
        for n in np.unique(n0[active]).tolist():
            m = active & (n0 == n)
            last[m] = rays(n).ravel()[m].astype(np.int64) - rays(n - batch).ravel()[m]
        cls = np.where(active, RR.classes(last), -1)
        a = 0 < active.sum() < nx * ny
        b = active[S.CAP_ITEMS:].any() and not active[S.CAP_ITEMS:].all()
        c = len(np.unique(cls[active])) >= 3
        waves = np.full(-(-nx * ny // 64) * 64, -1, np.int64)
        waves[:nx * ny] = cls
        waves = waves.reshape(-1, 64)
        per_wave = np.array([len(np.unique(w[w >= 0])) for w in waves])
        d = (per_wave >= 2).any()
        tail = active[nx * ny // 1024 * 1024:].any()
        print("dilate", flags, "pass", k + 1, "active", int(active.sum()), "in round two", int(active[S.CAP_ITEMS:].sum()), "classes", np.unique(cls[active]).tolist(),
              "waves with 2+ classes", int((per_wave >= 2).sum()), "of them in round two", int((per_wave[S.CAP_ITEMS // 64:] >= 2).sum()), (a, b, c, d, tail))
        good.append(a and b and c and d and tail)
        before = calls[k][2]
    assert any(good)


# ---- 3. rasterTexels / bakeTexels -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(S.ATLASES))
def test_the_atlases_fill_the_scan_past_one_count_per_lane(rt, name):
    """TR.raster alone at L on each atlas of the GPU tests: more than 1024 workgroup counts, owned texels among the workgroups 1024 .. 1027, two workgroups
    2 i, 2 i + 1 that both hold owned texels (the second iteration of a scan lane adds something), a lane past the end next to one that is not (the clamp);
    the grid atlas has an empty workgroup between owned ones, the overlapping one owns more than 90 % of the texels, and the first slot of the small one
    covers some 130 000 texels, which one wave walks."""
    W, H = L
    mesh, dilate = S.ATLASES[name]
    tris, slots = S.atlas(name, S.base_tris(rt, mesh), W, H)
    ref = TR.raster(tris, W, H, dilate, slots=slots)
    counts = S.group_counts(ref["prim"])
    nz = np.flatnonzero(counts)
    both = int(((counts[0:1028:2] > 0) & (counts[1:1028:2] > 0)).sum())
    print(name, "owned", ref["owned"], "of", W * H, "workgroups", len(counts), "non-zero", len(nz), "1024 ..", counts[S.CAP:].tolist(), "pairs with both", both)
    assert len(counts) == 1028 > S.CAP and counts.sum() == ref["owned"]
    assert counts[S.CAP:].any() and both > 0
    assert (ref["prim"].ravel()[S.CAP_ITEMS:] != TR.PRIM_NONE).any()
    if name == "grid":
        assert (counts[nz[0]:nz[-1]] == 0).any() and ref["covers"].max() == 1 and slots is None
    if name == "overlapping":
        assert ref["owned"] > 0.9 * W * H and (ref["covers"] >= 4).any() and len(slots) == S.OVERLAPPING_SLOTS
    if name == "small":
        assert (ref["prim"] == slots[0]).sum() > 130000 and (ref["prim"] == slots[1]).any() and (ref["prim"] == TR.PRIM_NONE).any()


def test_restricting_the_slots_changes_nothing(rt):
    """TR.raster(..., slots=) against the loop over every slot and against the CPU twin, where that is cheap: the atlases of L at 37 x 23."""
    from preview_support import same
    for name in sorted(S.ATLASES):
        mesh, dilate = S.ATLASES[name]
        tris, slots = S.atlas(name, S.base_tris(rt, mesh), 37, 23)
        a, b = TR.raster(tris, 37, 23, dilate, slots=slots), TR.raster(tris, 37, 23, dilate)
        owned, twin = rt.raster_texels_host(tris, 37, 23, dilate)
        assert a["owned"] == b["owned"] == owned > 0
        for k in ("prim", "src", "bary", "pos", "nrm"):
            same(a[k], b[k], f"{name}: {k}, restricted against every slot")
            same(a[k], twin[k], f"{name}: {k}, restricted against the host twin")
