"""What the GPU tests of rasterTexels / bakeTexels share (tests/test_gpu_texels.py, tests/test_gpu_capped_grids.py): a private mesh with rtAtlasGrid UVs and its
init, the comparison of a device raster with the CPU twin and the numpy restatement, gatherRadiance's full W*H point list from the raster's planes and the
comparison of a bake with it.  No test: a plain module."""
import numpy as np

import pixels_reference as PR
import radiance_reference as RR
import texels_reference as TR
from preview_support import same

MARGIN = 0.05


def private_mesh(rt, tag, folder):
    """A private copy of the tag's mesh (the shared one of pixels_reference stays as it is), its triangles given rtAtlasGrid UVs before any init."""
    path = str(folder / (tag + ".bvh"))
    assert PR.scene(rt, tag)["hm"].save(path) == 0
    hm = rt.HostMesh.load(path)
    assert hm.nppl == PR.scene(rt, tag)["hm"].nppl
    rt.atlas_grid(hm.tris, MARGIN)
    return hm


def init(rt, meshes, tag, **opts):
    s = PR.scene(rt, tag)
    ks, keep = rt.make_kernel_scene(meshes[tag], s["mats"], s["tex"], floor=s["floor"])
    fb = rt.initRenderer(ks, s["cam"], s["nx"], s["ny"], s["depth"], keepalive=keep)
    rt.setRenderOptions(rt.getDefaultRenderOptions(False), **dict(PR.options(tag), **opts))
    return fb


def max_dist_of(tag):
    lo, hi = RR.scene_box(tag)
    return float(np.float32(0.15 * np.linalg.norm(hi - lo)))       # a bound: M1 is a closed room, without one nothing is open


def check_raster(rt, tris, W, H, dilate, what, slots=None):
    """rasterTexels now against the twin and numpy over `tris`, the triangles the device holds: every plane and the return value.  `slots`: as TR.raster's."""
    got = rt.raster_texels(W, H, dilate)
    ms = rt.last_texels_ms()
    ref = TR.raster(tris, W, H, dilate, slots=slots)
    twin = rt.raster_texels_host(tris, W, H, dilate)
    print(what, f"{W} x {H} dilate {dilate}: owned", got[0], "kernel ms", ms)
    assert got[0] == ref["owned"] == twin[0], (what, got[0], ref["owned"], twin[0])
    for k in ("prim", "src", "bary", "pos", "nrm"):
        same(got[1][k], ref[k], f"{what}: {k} against numpy")
        same(got[1][k], twin[1][k], f"{what}: {k} against the host twin")
    assert ms > 0.0
    return ref


def full_list(rt, W, H, dilate):
    """rasterTexels' planes as gatherRadiance's point list: (owned count, planes, pos (W*H, 3), nrm (W*H, 3)) with the filler at unowned texels."""
    owned, pl = rt.raster_texels(W, H, dilate)
    mask = (pl["prim"] != TR.PRIM_NONE).ravel()
    pos = pl["pos"].reshape(-1, 3).copy()
    nrm = pl["nrm"].reshape(-1, 3).copy()
    pos[~mask] = 0
    nrm[~mask] = (0, 0, 1)
    assert owned == mask.sum() and np.isfinite(pos).all() and np.isfinite(nrm).all()
    return owned, pl, pos, nrm


def expected(pl, ref):
    """The planes bakeTexels owes, from gatherRadiance's per-point (out, acc, rays) over the full list."""
    out, acc, rays = ref
    H, W = pl["prim"].shape
    mask = (pl["prim"] != TR.PRIM_NONE).ravel()
    src = pl["src"].ravel()
    e_out = np.where((src != -1)[:, None], out[np.where(src != -1, src, 0)], np.float32(0)).astype(np.float32)
    e_acc = np.where(mask[:, None], acc, np.float32(0)).astype(np.float32)
    e_rays = np.where(mask, rays, 0).astype(np.uint32)
    return e_out.reshape(H, W, -1), e_acc.reshape(H, W, -1), e_rays.reshape(H, W)


def check_bake(got, pl, ref, what):
    owned, planes = got
    e_out, e_acc, e_rays = expected(pl, ref)
    assert owned == (pl["prim"] != TR.PRIM_NONE).sum(), what
    assert np.array_equal(planes["prim"], pl["prim"]) and np.array_equal(planes["src"], pl["src"]), what
    same(planes["out"], e_out, what + ": out")
    same(planes["acc"], e_acc, what + ": acc")
    assert np.array_equal(planes["rays"], e_rays), (what, int((planes["rays"] != e_rays).sum()))
