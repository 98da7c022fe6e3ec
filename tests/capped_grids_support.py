"""What tests/test_capped_grids_api.py (CPU: the conditions) and tests/test_gpu_capped_grids.py (GPU: the comparisons) share: the two shapes at which the
histogram of displayFrame, the count and scatter of refineFrame and the scan of rasterTexels / bakeTexels change their indexing, and the inputs built for
them.  No test: a plain module.

The three passes work in workgroups of 256 items.  k_display_histogram, k_refine_count and k_refine_scatter launch at most 1024 workgroups and stride over
the rest; k_texel_scan scans one count per workgroup with 1024 lanes, ceil(workgroups / 1024) counts per lane.  So the regime changes at 1024 * 256 =
262 144 items:
  L = 523 x 503 = 263 069 items = 1028 workgroups.  The second round holds 925 items: workgroups 0 .. 2 full, workgroup 3 partial, 1020 workgroups with an
      empty second round; a scan lane holds 2 counts, lanes 0 .. 513 both, lanes 514 .. 1023 none.  523 and 503 are prime: no row, tile, wave or dither period
      lines up with a round, and item 262 144 lies inside row 501.
  E = 512 x 512 = 262 144 items = exactly 1024 workgroups: the last size of one round and of one count per lane."""
import functools

import numpy as np

import pixels_reference as PR
import texels_reference as TR

L, E = (523, 503), (512, 512)                   # (nx, ny) = (W, H)
SHAPES = {"E": E, "L": L}
GROUP, CAP = 256, 1024                          # items per workgroup; the grid cap of the three passes = the lanes of the texel scan
CAP_ITEMS = GROUP * CAP
REFINE_TAG = "S1_523x503"                       # refine_reference's tag of the three spheres at L
CROPS = ((0, 500, 523, 503), (240, 180, 272, 196))         # where the frames at L are anchored to the oracle: rows 500 .. 502 whole, and a 32 x 16 block

# rasterTexels / bakeTexels: the atlases.  The grid atlas is M2_floor's own (all 300 live slots), not M1's: the last cells of M1's 51 x 51 grid hold even
# slots only, whose triangles end in a point below the centre of texel row 501, so no texel from 262 144 on is owned at L and the workgroups 1024 .. 1027
# would hold nothing.  The numpy raster costs 8 ms per evaluated slot at these sizes, so the overlapping atlas keeps its UVs on the first 288 live slots of
# M1 and parks the rest (still above 90 % owned), and TR.raster evaluates those alone.
ATLASES = {"grid": ("M2_floor", 2), "overlapping": ("M1", 1), "small": ("M1", 0)}          # name: (mesh, dilate)
OVERLAPPING_SLOTS = 288


def groups_of(items):
    return (items + GROUP - 1) // GROUP


def base_tris(rt, tag):
    """The tag's triangles with rtAtlasGrid UVs: what texels_support.private_mesh holds."""
    tris = PR.scene(rt, tag)["hm"].tris.copy()
    rt.atlas_grid(tris, 0.05)
    return tris


def atlas(name, base, W, H):
    """(tris, slots) of the named atlas over `base` (the triangles of ATLASES[name]'s mesh with their grid UVs): what the device is given, and TR.raster's
    `slots` (None: every slot)."""
    if name == "grid":
        return base.copy(), None
    live = TR.live_slots(base)
    if name == "overlapping":
        slots = live[:OVERLAPPING_SLOTS]
        return TR.keep_slots(TR.atlas_overlapping(base), slots), slots
    return TR.atlas_small(base, W, H)[0], live[:2]


def group_counts(prim):
    """Owned texels per workgroup of 256 texels: what k_texel_resolve writes and k_texel_scan scans."""
    owned = (prim != TR.PRIM_NONE).ravel()
    padded = np.zeros(groups_of(owned.size) * GROUP, bool)
    padded[:owned.size] = owned
    return padded.reshape(-1, GROUP).sum(axis=1)


@functools.lru_cache(maxsize=None)
def every_pixel(nx, ny):
    """The (nx * ny, 2) int32 list of every pixel, (i, j), in index order."""
    j, i = np.divmod(np.arange(nx * ny, dtype=np.int32), np.int32(nx))
    ij = np.ascontiguousarray(np.stack([i, j], axis=1).astype(np.int32))
    ij.setflags(write=False)
    return ij


def check_lists(ref, lists, rays, nx, batch, ascending=False):
    """The list of every pass against the reference's calls `ref`: exactly the active set - no pixel missing, none twice - and in the default order the
    classes of the pixels' last batches non-increasing, in the ascending one j * nx + i strictly increasing.  rays: n -> the (ny, nx) plane of a pixel's rays
    over its first n samples.  Returns the classes of every pass's list."""
    import refine_reference as RR
    out = []
    before = np.zeros_like(ref[0][2])
    for k, (call, ij) in enumerate(zip(ref, lists)):
        ids = ij[:, 1].astype(np.int64) * nx + ij[:, 0]
        active = np.flatnonzero(call[4].ravel())
        assert len(ids) == len(active) == call[0], (k, len(ids), len(active), call[0])
        assert np.array_equal(np.sort(ids), active), f"pass {k + 1}: the list is not the reference's active set"
        n0 = before[ij[:, 1], ij[:, 0]]
        last = np.zeros(len(ij), np.int64)
        for n in np.unique(n0).tolist():
            if n > 0:
                m = n0 == n
                last[m] = rays(n)[ij[m, 1], ij[m, 0]].astype(np.int64) - (rays(n - batch)[ij[m, 1], ij[m, 0]].astype(np.int64) if n > batch else 0)
        cls = RR.classes(last)
        if ascending:
            assert (np.diff(ids) > 0).all(), f"pass {k + 1}: the list does not ascend"
        else:
            assert (np.diff(cls) <= 0).all(), f"pass {k + 1}: the classes increase somewhere"
        out.append(cls)
        before = call[2]
    return out
