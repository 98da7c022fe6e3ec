"""CPU: the device images of both scene kinds (layout_spheres / layout_mesh / permute_triangles, csrc/rt_scene_layout.h) against the rules restated here,
array by array and scalar by scalar.  The kernels' bit-exactness on sphere scenes rests on this host arithmetic - the slot order, the group boxes pushed out by
one float, the cell tables with their slack, the culling constants - and a box one float too tight or a missing cell bit changes a frame only for the rare
ray that grazes a group; the refit kernels have to reproduce the mesh records' bits.  tests/scene_layout_dump.cpp includes the header, is compiled as plain
C++ (no kernel, no HIP call) and builds the layouts of the scenes written here; a second build of it under AddressSanitizer and UBSan, a stand-alone process,
runs over the same scenes.

Two shapes hand the standard library a comparison that is no ordering, and there the test takes the library's choice from the output instead of restating it:
with NaN radii std::nth_element's "median" is whichever element it leaves at n / 2, so the big spheres must be those of the rule for SOME element of the radii;
with a NaN centre coordinate std::stable_sort's order is its own, so the slot order must be a permutation with the rule's group counts.  Everything else of
those scenes - the arrays, the boxes, the tables, the constants - is restated from that order like every other scene's."""
import os
import subprocess

import numpy as np
import pytest

from kernel_forms import FORMS, build_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

G, CELLS, CELL_WORDS_MAX, CELL_SLACK = 16, 64, 8, 1.0e-3        # kSphereGroup, kCellCount, kCellWordsMax (rt_params.h), kCellSlack (layout_spheres)
INT_MAX = 2 ** 31 - 1
F32 = np.float32
SPHERE_INTS = "n n_padded n_groups n_big_groups n_big basic_materials global_scene box_shared_axis cell_on cell_axes".split()
SPHERE_FLOATS = ("cull_cx cull_cy cull_cz cull_radius cull_k1 cull_k2 cull_k3 cull_coord_max box_shared_lo box_shared_hi pair_k0 "
                 "cell_scale0 cell_scale1 cell_scale2 cell_off0 cell_off1 cell_off2 ubox0 ubox1 ubox2 ubox3 ubox4 ubox5").split()
SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 488, 700, 1100, 2100, 4097, 6000]      # 4097: the first size without cell tables; 2100 / 6000: hybrid and global forms
SHAPES = ["volume", "plane_x", "plane_y", "plane_z", "negative", "nonfinite", "coincident", "nan_centre", "huge_centre", "no_big", "all_big", "no_cells"]


def _rt():
    import cuda_raytracing_optimized_amd as rt
    return rt


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.flatnonzero((got.reshape(-1).view(np.uint32 if got.itemsize == 4 else np.uint8) != want.reshape(-1).view(np.uint32 if want.itemsize == 4 else np.uint8)))
        pytest.fail(f"{what}: {len(bad)} entries differ, first at {bad[0]}: got {got.reshape(-1)[bad[0]]!r}, expected {want.reshape(-1)[bad[0]]!r}")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# sphere scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def sphere_case(shape, n):
    """(spheres, materials, box_cells) of a synthetic scene: the benchmark's density at every size, the ground sphere first where the shape has a big one."""
    rt = _rt()
    rng = np.random.default_rng(100 * SHAPES.index(shape) + n)
    half = 6.0 * (n / 488.0) ** 0.5
    sp, mt = np.zeros(n, rt.sphere_dtype), np.zeros(n, rt.material_dtype)
    c = rng.uniform(-half, half, (n, 3))
    c[:, 1] = rng.uniform(0.0, half, n)
    sp["radius"] = rng.uniform(0.1, 0.3, n)
    k = np.arange(n)
    if shape.startswith("plane_"):                                  # all centres and radii equal on one axis (plane_y: the benchmark's resting plane)
        c[:, "xyz".index(shape[-1])] = 0.2
        sp["radius"] = 0.2
    sp["center"] = c
    if shape == "negative":
        sp["radius"][k % 5 == 0] *= -1
    if shape == "nonfinite":
        sp["radius"][k % 7 == 0] = np.inf
        sp["radius"][k % 14 == 0] = np.nan
    if shape == "coincident":
        sp["center"] = (1.0, 1.0, 1.0)
    if shape in ("nan_centre", "huge_centre"):
        sel = np.flatnonzero(k % 9 == 0)
        # huge_centre: FLT_MAX pushes a box to inf (no valid cell geometry); nan_centre: an unordered key among the centres
        sp["center"][sel, sel % 3] = np.where(sel % 18 == 0, np.finfo(F32).max if shape == "huge_centre" else 3e38, 3e38 if shape == "huge_centre" else np.nan)
    if shape == "all_big":                                          # every radius non-finite: no small sphere, no group box
        sp["radius"] = np.where(k % 2 == 0, np.inf, np.nan)
    elif shape not in ("no_big", "coincident"):
        sp["center"][0] = (0, -1000, 0); sp["radius"][0] = 1000
    mt["type"] = rng.integers(0, 3, n)
    mt["color"] = rng.uniform(0.1, 1, (n, 3))
    mt["param"] = rng.uniform(0, 1.5, n)
    mt["texId"] = -1
    if shape == "negative" and n > 2:
        mt["type"][n // 2] = rt.RT_MODEL_GLOSSY                     # (a look preset: basic_materials 0)
    return sp, mt, shape != "no_cells"


def recipe_case(recipe):
    sc = build_scene(_rt(), recipe)
    return sc[1], sc[2], True


SPHERE_CASES = [(f"{shape}-{n}", (sphere_case, shape, n)) for shape in SHAPES for n in SIZES]
SPHERE_CASES += [("random_spheres", (recipe_case, ("random",)))]
CLOUDS = sorted({f["scene"] for f in FORMS if f["scene"][0] == "cloud"})      # every cloud the forms table renders: a form added there is a case here
SPHERE_CASES += [(f"cloud-{n}-{shape}-{int(presets)}", (recipe_case, recipe)) for recipe in CLOUDS for _, n, shape, presets in [recipe]]


def f32_of(x):
    """(float)x of a double: round to nearest, beyond the range to inf."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(F32)


def min_ignoring_nan(v, start):
    """std::min(start, x) folded over v: a NaN never replaces what is there."""
    v = v[~np.isnan(v)]
    return min(start, v.min()) if len(v) else start


def max_ignoring_nan(v, start):
    v = v[~np.isnan(v)]
    return max(start, v.max()) if len(v) else start


def split_order(centres, idx):
    """The recursive median split: `idx` (caller indices, in order) -> the order of the slots, -1 = pad.  Stable by the centre coordinate of the axis of largest
    centre extent (the first such axis), the left part (groups / 2) * G."""
    out = []

    def split(v):
        if len(v) <= G:
            out.extend(v)
            while len(out) % G:
                out.append(-1)
            return
        c = centres[v].astype(np.float64)
        ext = [max_ignoring_nan(c[:, a], -1e300) - min_ignoring_nan(c[:, a], 1e300) for a in range(3)]
        axis = 0
        for a in (1, 2):
            if ext[a] > ext[axis]:
                axis = a
        v = [v[i] for i in np.argsort(centres[v, axis], kind="stable")]
        left = min(len(v) - 1, ((len(v) + G - 1) // G // 2) * G)
        split(v[:left])
        split(v[left:])
    if idx:
        split(list(idx))
    return out


def expected_spheres(sp, mt, box_cells, got):
    """The layout of a sphere scene, restated: (ints, floats, arrays) as the dump writes them.  `got` is consulted only where the module docstring says so."""
    n = len(sp)
    centres, radius = sp["center"], sp["radius"]
    radii = np.abs(radius)
    finite = np.isfinite(radii)
    if not np.isnan(radii).any():
        big_above = F32(4.0) * np.sort(radii)[n // 2]
        is_big = (radii > big_above) | ~finite
    else:                                                           # the big spheres of the rule for some element of the radii as the median
        n_big = got[0]["n_big"]
        got_big = np.zeros(n, bool)
        got_big[got[2]["orig"][:n_big]] = True
        with np.errstate(invalid="ignore"):
            assert any(np.array_equal(got_big, (radii > F32(4.0) * m) | ~finite) for m in np.unique(radii)), "the big spheres are not those of 4 x any element of the radii"
        is_big = got_big
    big, small = [int(k) for k in np.flatnonzero(is_big)], [int(k) for k in np.flatnonzero(~is_big)]
    slots = list(big)
    while len(slots) % G:
        slots.append(-1)
    n_big_groups = len(slots) // G
    if np.isnan(centres[small]).any():                              # the order of std::stable_sort with an unordered key: a permutation with the rule's counts
        n_small_slots = (len(small) + G - 1) // G * G
        ordered = [int(k) if k != INT_MAX else -1 for k in got[2]["orig"][len(slots):len(slots) + n_small_slots]]
        assert sorted(k for k in ordered if k >= 0) == small and all(k >= 0 for k in ordered[:len(small)]), "the small slots are not a permutation of the small spheres"
    else:
        ordered = split_order(centres, small)
    slots += ordered
    while len(slots) % 64:
        slots.append(-1)
    slots = np.array(slots, np.int64)
    n_padded, n_groups = len(slots), len(slots) // G
    real_slot = np.flatnonzero(slots >= 0)
    who = slots[real_slot]

    ints = dict(n=n, n_padded=n_padded, n_groups=n_groups, n_big_groups=n_big_groups, n_big=len(big), global_scene=0,
                basic_materials=int(np.isin(mt["type"], (0, 1, 2)).all()))
    arr = {}
    arr["spheres"] = np.tile(np.array([0.0, 3.0e18, 0.0, 0.0], F32), (n_padded + n_groups, 1))       # pad entries: radius 0, far away
    with np.errstate(over="ignore", invalid="ignore"):
        arr["spheres"][real_slot + real_slot // G] = np.column_stack([centres[who], radius[who] * radius[who]])     # w: one fp32 multiply
    arr["rad"] = np.zeros(n_padded, F32); arr["rad"][real_slot] = radius[who]
    arr["mat_color"] = np.zeros((n_padded, 4), F32); arr["mat_color"][real_slot] = np.column_stack([mt["color"][who], mt["param"][who]])
    arr["mat_type"] = np.zeros(n_padded, np.int32); arr["mat_type"][real_slot] = mt["type"][who]
    arr["orig"] = np.full(n_padded, INT_MAX, np.int32); arr["orig"][real_slot] = who
    arr["slot_of"] = np.zeros(n, np.int32); arr["slot_of"][who] = real_slot

    # group boxes: nextafter(float(lo), -inf), nextafter(float(hi), +inf) of the double extent c -+ |r|; an empty group has lo > hi
    boxes = np.tile(np.array([3.0e38, -3.0e38, 3.0e38, 0.0], F32), (n_groups * 3, 1))
    c64, r64 = centres.astype(np.float64), radii.astype(np.float64)
    box_groups, lo_f, hi_f = [], {}, {}
    for g in range(n_big_groups, n_groups):
        members = slots[g * G:(g + 1) * G]
        members = members[members >= 0]
        if len(members) == 0:
            continue
        lo = np.array([min_ignoring_nan(c64[members, a] - r64[members], 1e300) for a in range(3)])
        hi = np.array([max_ignoring_nan(c64[members, a] + r64[members], -1e300) for a in range(3)])
        with np.errstate(over="ignore"):
            lo_f[g], hi_f[g] = np.nextafter(f32_of(lo), F32(-np.inf)), np.nextafter(f32_of(hi), F32(np.inf))
        for a in range(3):
            boxes[3 * g + a] = (lo_f[g][a], hi_f[g][a], lo_f[g][a], 0.0)
            inside = ~np.isnan(c64[members, a])                     # hence: every member's extent lies strictly inside the box
            assert (lo_f[g][a] < (c64[members, a] - r64[members])[inside]).all() and ((c64[members, a] + r64[members])[inside] < hi_f[g][a]).all()
        box_groups.append(g)
    coord_max = F32(max([0.0] + [float(max(np.abs(lo_f[g]).max(), np.abs(hi_f[g]).max())) for g in box_groups]))
    shared_ok = [all(lo_f[g][a] == lo_f[box_groups[0]][a] and hi_f[g][a] == hi_f[box_groups[0]][a] for g in box_groups) for a in range(3)]
    flo = dict(box_shared_lo=F32(0), box_shared_hi=F32(0))
    ints["box_shared_axis"] = 0
    for a in (2, 1, 0):                                             # the lowest axis on which every box has the same extent
        if box_groups and shared_ok[a]:
            ints["box_shared_axis"] = a + 1
            flo.update(box_shared_lo=lo_f[box_groups[0]][a], box_shared_hi=hi_f[box_groups[0]][a])

    # cell tables: 3 axes x (begins, ends) x CELLS cells x W words behind the boxes; bit k of a cell = small group k
    W = (n_groups + 31) // 32
    W = W if W <= CELL_WORDS_MAX else 0
    tab = np.zeros((3, 2, CELLS, W), np.uint32)
    ints.update(cell_on=0, cell_axes=0)
    ubox, scale, off = np.zeros(6, F32), np.zeros(3, F32), np.zeros(3, F32)
    if box_groups and W > 0:
        real = [g for g in box_groups if lo_f[g][0] <= hi_f[g][0]]
        cell = np.arange(CELLS)
        ok = True
        for a in range(3):
            amin = min([1e300] + [float(lo_f[g][a]) for g in real])
            amax = max([-1e300] + [float(hi_f[g][a]) for g in real])
            ubox[a], ubox[3 + a] = f32_of(amin), f32_of(amax)
            with np.errstate(all="ignore"):
                w = np.float64(amax - amin) / CELLS
                ok = bool(w > 1e-30 and np.isfinite(w) and np.isfinite(1.0 / w) and np.isfinite(amin / w))
            if not ok:
                break
            scale[a], off[a] = f32_of(1.0 / w), f32_of(-amin / w)
            if not shared_ok[a]:
                ints["cell_axes"] |= 1 << a
            begins_below = amin + (cell + 1 + CELL_SLACK) * w       # the double expressions of the header
            ends_above = amin + (cell - CELL_SLACK) * w
            for g in real:
                k = g - n_big_groups
                begins = (cell == CELLS - 1) | (np.float64(lo_f[g][a]) <= begins_below)
                ends = (cell == 0) | (np.float64(hi_f[g][a]) >= ends_above)
                tab[a, 0, :, k >> 5] |= begins.astype(np.uint32) << np.uint32(k & 31)
                tab[a, 1, :, k >> 5] |= ends.astype(np.uint32) << np.uint32(k & 31)
                # soundness, whatever the slack: a cell whose interval meets the group's extent has the group in both sets
                meets = (np.float64(lo_f[g][a]) <= amin + (cell + 1) * w) & (np.float64(hi_f[g][a]) >= amin + cell * w)
                have = ((tab[a, 0, :, k >> 5] >> np.uint32(k & 31)) & (tab[a, 1, :, k >> 5] >> np.uint32(k & 31)) & 1).astype(bool)
                assert (have | ~meets).all(), f"group {g}, axis {a}: a cell that meets the group's extent lacks its bit"
                assert tab[a, 0, CELLS - 1, k >> 5] >> np.uint32(k & 31) & 1 and tab[a, 1, 0, k >> 5] >> np.uint32(k & 31) & 1
        ints["cell_on"] = int(ok and box_cells)
    arr["groups"] = np.concatenate([boxes, tab.reshape(-1).view(F32).reshape(-1, 4)])

    # the per-ray margin constants
    cc, rad, r_min, r_max = np.zeros(3), 0.0, 1.0, 0.0
    if small:
        cs = c64[small]
        cc = np.array([0.5 * (min_ignoring_nan(cs[:, a], 1e300) + max_ignoring_nan(cs[:, a], -1e300)) for a in range(3)])
        d = cs - cc
        with np.errstate(over="ignore", invalid="ignore"):
            reach = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) + r64[small]
        rad = max_ignoring_nan(reach, 0.0)
        r_min, r_max = r64[small].min(), r64[small].max()
    k_eps = 96.0 * 5.9604645e-8
    flo.update(cull_cx=f32_of(cc[0]), cull_cy=f32_of(cc[1]), cull_cz=f32_of(cc[2]), cull_radius=f32_of(rad * 1.000001 + 1e-30),
               cull_k1=f32_of(k_eps / (2.0 * max(r_min, 1e-30))), cull_k2=f32_of(np.sqrt(k_eps)), cull_k3=F32(16.0) * F32(5.9604645e-8), cull_coord_max=coord_max,
               pair_k0=f32_of(2.0 * 3.814697265625e-6 * r_max * r_max * 1.0001))
    for a in range(3):
        flo[f"cell_scale{a}"], flo[f"cell_off{a}"], flo[f"ubox{a}"], flo[f"ubox{3 + a}"] = scale[a], off[a], ubox[a], ubox[3 + a]
    return ints, flo, arr


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# mesh scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def hand_mesh(leaves, nppl, seed, extra=0, empty_leaf=None, hole=None, presets=False, textured=False):
    """A hand-built tree: 2 * leaves nodes of arbitrary boxes, leaves * nppl + extra triangle slots, the last slots of some leaves sentinels; empty_leaf: a leaf
    of sentinels only; hole = (leaf, k): a sentinel in FRONT of that leaf's real triangles (k < nppl - 1)."""
    rt = _rt()
    rng = np.random.default_rng(seed)
    tris = np.zeros(leaves * nppl + extra, rt.triangle_dtype)
    tris["v"] = rng.uniform(-5, 5, tris["v"].shape)
    tris["texCoords"] = rng.uniform(0, 1, tris["texCoords"].shape)
    tris["meshID"] = rng.integers(0, 4, len(tris))
    for leaf in range(leaves):                                      # trailing sentinels: up to half a leaf
        pad = int(rng.integers(0, nppl // 2 + 1)) if nppl > 1 else 0
        if leaf == empty_leaf:
            pad = nppl
        if pad:
            tris["v"][(leaf + 1) * nppl - pad:(leaf + 1) * nppl] = np.inf
    if hole is not None:
        tris["v"][hole[0] * nppl + hole[1]] = np.inf
        tris["v"][hole[0] * nppl + hole[1] + 1] = rng.uniform(-5, 5, (3, 3))
    nodes = np.zeros(2 * leaves, rt.bvh_node_dtype)
    nodes["a"] = rng.uniform(-9, 0, (2 * leaves, 3)); nodes["b"] = rng.uniform(0, 9, (2 * leaves, 3))
    mats = np.zeros(4, rt.material_dtype)
    mats["type"] = [0, 1, 2, 0]; mats["color"] = rng.uniform(0, 1, (4, 3)); mats["param"] = rng.uniform(0, 1.5, 4); mats["texId"] = -1
    tex = []
    if presets:
        mats["type"][2] = rt.RT_MODEL_COAT
    if textured:
        tex = [rng.uniform(0, 1, (3, 5, 3)).astype(F32), rng.uniform(0, 1, (2, 2, 3)).astype(F32)]
        mats["texId"][1] = 1
    from_ = rng.permutation(len(tris)).astype(np.int32)
    from_[rng.integers(0, len(tris), max(1, len(tris) // 5))] = -1
    return dict(tris=tris, nodes=nodes, nppl=nppl, mats=mats, tex=tex, boxes=rng.uniform(-9, 9, 12).astype(F32), from_=from_)


def staircase_mesh():
    rt = _rt()
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    b = hm.view.bounds
    boxes = np.array([b.min.e[0], b.min.e[1], b.min.e[2], b.max.e[0], b.max.e[1], b.max.e[2], 0, 1, 0, 0, -3, 0], F32)
    rng = np.random.default_rng(5)
    from_ = rng.permutation(len(hm.tris)).astype(np.int32)
    from_[::11] = -1
    return dict(tris=hm.tris.copy(), nodes=hm.bvh.copy(), nppl=hm.nppl, mats=mats, tex=[], boxes=boxes, from_=from_)


MESH_CASES = [("staircase", (staircase_mesh,))]
MESH_CASES += [(f"hand-{leaves}x{nppl}", (hand_mesh, leaves, nppl, 10 * leaves + nppl)) for leaves in (2, 4) for nppl in (1, 3, 255, 256)]
MESH_CASES += [("extra_slots", (hand_mesh, 4, 3, 71, 5)), ("empty_leaf", (hand_mesh, 4, 3, 72, 0, 2)), ("sentinel_inside", (hand_mesh, 4, 5, 73, 0, None, (1, 1))),
               ("presets", (hand_mesh, 2, 3, 74, 0, None, None, True)), ("textured", (hand_mesh, 2, 3, 75, 0, None, None, False, True))]


def expected_mesh(m):
    tris, nodes, nppl = m["tris"], m["nodes"], m["nppl"]
    first_leaf = len(nodes) // 2
    sent = np.isinf(tris["v"][:first_leaf * nppl, 0, 0]).reshape(first_leaf, nppl)
    trailing = int(not (sent[:, :-1] & ~sent[:, 1:]).any())
    e = dict(first_leaf=first_leaf, nppl=nppl, leaf_sentinels_trailing=trailing, boxes=m["boxes"],
             lean_ok=int((np.isin(m["mats"]["type"], (0, 1, 2)) & (m["mats"]["texId"] == -1)).all()))
    e["tris"] = tris
    node_floats = np.column_stack([nodes["a"], nodes["b"]])         # 6 floats per node
    e["bvh"] = np.zeros(((node_floats.size + 3) // 4 + 1) * 4, F32)
    e["bvh"][:node_floats.size] = node_floats.reshape(-1)
    L, R = node_floats[0::2], node_floats[1::2]                     # the child pair of record i: nodes 2i, 2i + 1
    e["bvh_axis"] = np.stack([np.column_stack([L[:, a], R[:, a], L[:, 3 + a], R[:, 3 + a], L[:, 3 + a], R[:, 3 + a], L[:, a], R[:, a]]) for a in range(3)], axis=1).reshape(-1)
    if trailing and nppl <= 255:
        v = tris["v"][:first_leaf * nppl]
        with np.errstate(invalid="ignore"):
            rec = np.column_stack([v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0],                  # v0, one fp32 subtraction per edge component
                                   tris["meshID"][:first_leaf * nppl].astype(np.uint32).view(F32), np.zeros((len(v), 2), F32)])
        rec[sent.reshape(-1)] = 0.0
        e["leaf_tri"] = rec.reshape(-1)
        counts = np.zeros((first_leaf + 3) // 4 * 4, np.uint8)
        counts[:first_leaf] = (~sent).sum(axis=1)
        e["leaf_ofs"] = counts.view("<u4")
    else:
        e["leaf_tri"], e["leaf_ofs"] = np.zeros(0, F32), np.zeros(0, np.uint32)
    e["moved"] = np.zeros(len(tris), tris.dtype)
    e["moved"]["v"] = np.inf                                        # the sentinel triangle: every coordinate inf, the rest zero
    e["moved"][m["from_"] >= 0] = tris[m["from_"][m["from_"] >= 0]]
    return e


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the dump program
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _make(entry):
    return entry[0](*entry[1:])


def write_cases(path, spheres, meshes):
    i32 = lambda *v: np.array(v, "<i4").tobytes()
    with open(path, "wb") as f:
        f.write(i32(len(spheres) + len(meshes)))
        for sp, mt, box_cells in spheres:
            f.write(i32(0, len(sp), int(box_cells)) + sp.tobytes() + mt.tobytes())
        for m in meshes:
            f.write(i32(1, len(m["tris"]), len(m["nodes"]), m["nppl"], len(m["mats"]), len(m["tex"]), len(m["from_"])) + m["boxes"].tobytes())
            f.write(np.ascontiguousarray(m["tris"]).tobytes() + np.ascontiguousarray(m["nodes"]).tobytes() + np.ascontiguousarray(m["mats"]).tobytes())
            for t in m["tex"]:
                f.write(i32(t.shape[1], t.shape[0]) + t.tobytes())
            f.write(m["from_"].tobytes())


class Reader:
    def __init__(self, path):
        self.buf, self.pos = open(path, "rb").read(), 0

    def take(self, dtype, count):
        a = np.frombuffer(self.buf, dtype, count, self.pos)
        self.pos += a.nbytes
        return a

    def array(self, dtype, per=1):
        return self.take(dtype, per * int(self.take("<i8", 1)[0]))


def read_results(path, n_spheres, meshes):
    rt = _rt()
    r = Reader(path)
    out_s, out_m = [], []
    for _ in range(n_spheres):
        ints = dict(zip(SPHERE_INTS, (int(v) for v in r.take("<i4", len(SPHERE_INTS)))))
        floats = dict(zip(SPHERE_FLOATS, r.take(F32, len(SPHERE_FLOATS))))
        null = int(r.take("<i4", 1)[0])
        arr = dict(spheres=r.array(F32, 4).reshape(-1, 4), rad=r.array(F32), mat_color=r.array(F32, 4).reshape(-1, 4), mat_type=r.array(np.int32),
                   groups=r.array(F32, 4).reshape(-1, 4), orig=r.array(np.int32), slot_of=r.array(np.int32))
        out_s.append((ints, floats, arr, null))
    for m in meshes:
        g = dict(first_leaf=int(r.take("<u4", 1)[0]), nppl=int(r.take("<u4", 1)[0]))
        g["leaf_sentinels_trailing"], g["lean_ok"], g["null"] = (int(v) for v in r.take("<i4", 3))
        g["boxes"] = r.take(F32, 12)
        g.update(tris=r.array(rt.triangle_dtype), bvh=r.array(F32, 4), bvh_axis=r.array(F32), leaf_tri=r.array(F32, 4), leaf_ofs=r.array(np.uint32),
                 materials=r.array(rt.material_dtype), tex_w=r.array(np.int32), tex_h=r.array(np.int32))
        g["tex"] = [r.array(F32) for _ in m["tex"]]
        g["moved"] = r.array(rt.triangle_dtype)
        out_m.append(g)
    assert r.pos == len(r.buf), "the dump wrote more than the cases' records"
    return out_s, out_m


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """Every case through tests/scene_layout_dump.cpp, compiled as plain C++ against the header - and a second time under ASan + UBSan, run as a stand-alone
    process over the same cases.  Returns (inputs, results, the sanitized run) per kind."""
    tmp = tmp_path_factory.mktemp("scene_layout")
    spheres = [_make(entry) for _, entry in SPHERE_CASES]
    meshes = [_make(entry) for _, entry in MESH_CASES]
    write_cases(str(tmp / "cases.bin"), spheres, meshes)
    builds = {name: subprocess.Popen([os.environ.get("HIPCC", "hipcc"), "-std=c++17", "-O1", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "scene_layout_dump.cpp"),
                                      "-o", str(tmp / f"scene_layout_dump_{name}")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
              for name, flags in (("plain", []), ("sanitized", SANITIZE))}         # (the two compilations side by side)
    runs = {}
    for name, build in builds.items():
        _, err = build.communicate()
        assert build.returncode == 0, err[-3000:]
        runs[name] = subprocess.run([str(tmp / f"scene_layout_dump_{name}"), str(tmp / "cases.bin"), str(tmp / f"{name}.bin")], capture_output=True, text=True)
    assert runs["plain"].returncode == 0, runs["plain"].stderr[-2000:]
    got_s, got_m = read_results(str(tmp / "plain.bin"), len(spheres), meshes)
    same_output = runs["sanitized"].returncode == 0 and open(tmp / "plain.bin", "rb").read() == open(tmp / "sanitized.bin", "rb").read()
    return dict(spheres=dict(zip((k for k, _ in SPHERE_CASES), zip(spheres, got_s))), meshes=dict(zip((k for k, _ in MESH_CASES), zip(meshes, got_m))),
                sanitized=runs["sanitized"], same_output=same_output)


def test_sanitized_build_runs_clean(layouts):
    r = layouts["sanitized"]
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    assert layouts["same_output"], "the sanitized build wrote other layouts than the plain one"


@pytest.mark.parametrize("name", [k for k, _ in SPHERE_CASES])
def test_sphere_layout(layouts, name):
    (sp, mt, box_cells), got = layouts["spheres"][name]
    g_ints, g_floats, g_arr, null = got
    ints, floats, arr = expected_spheres(sp, mt, box_cells, got)
    assert null == 1, "a scene pointer of the template is not null"
    assert g_ints == ints, {k: (g_ints[k], ints[k]) for k in ints if g_ints[k] != ints[k]}
    for k in SPHERE_FLOATS:
        same(np.array([g_floats[k]]), np.array([floats[k]], F32), k)
    for k in ("spheres", "rad", "mat_color", "mat_type", "orig", "slot_of", "groups"):
        same(g_arr[k], arr[k], k)
    # what the restatement implies, said on its own: whole blocks of 64 slots in groups of G, big spheres in front, orig and slot_of inverse over the real slots
    n, n_big = len(sp), ints["n_big"]
    assert ints["n_padded"] % 64 == 0 and ints["n_groups"] * G == ints["n_padded"] and ints["n_big_groups"] == (n_big + G - 1) // G
    radii = np.abs(sp["radius"])
    if not np.isnan(radii).any():
        big = (radii > F32(4.0) * np.sort(radii)[n // 2]) | ~np.isfinite(radii)
        assert sorted(g_arr["orig"][:n_big]) == list(np.flatnonzero(big)) and (g_arr["orig"][n_big:ints["n_big_groups"] * G] == INT_MAX).all()
    real = g_arr["orig"] != INT_MAX
    assert real.sum() == n and (g_arr["slot_of"][g_arr["orig"][real]] == np.flatnonzero(real)).all() and (g_arr["orig"][g_arr["slot_of"]] == np.arange(n)).all()
    boxes = g_arr["groups"][:3 * ints["n_groups"]].reshape(-1, 3, 4)
    empty = ~real.reshape(-1, G).any(axis=1)
    assert (boxes[empty][:, :, 0] > boxes[empty][:, :, 1]).all() and (boxes[:ints["n_big_groups"], :, 0] > boxes[:ints["n_big_groups"], :, 1]).all()
    assert ints["cell_on"] in (0, 1) and (box_cells or ints["cell_on"] == 0)


def test_sphere_cases_reach_every_branch(layouts):
    got = {k: v[1] for k, v in layouts["spheres"].items()}
    i = lambda k: got[k][0]
    assert i("volume-488")["cell_on"] == 1 and i("no_cells-488")["cell_on"] == 0 and i("volume-4097")["cell_on"] == 0 and len(got["volume-4097"][2]["groups"]) == 3 * i("volume-4097")["n_groups"]
    assert i("volume-2100")["cell_on"] == 1 and i("volume-488")["cell_axes"] == 7
    assert (i("plane_x-488")["box_shared_axis"], i("plane_y-488")["box_shared_axis"], i("plane_z-488")["box_shared_axis"], i("volume-488")["box_shared_axis"]) == (1, 2, 3, 0)
    assert (i("plane_y-488")["cell_axes"], i("plane_y-488")["cell_on"]) == (5, 1)
    assert i("huge_centre-488")["cell_on"] == 0 and i("huge_centre-488")["cell_axes"] == 0 and np.isinf(got["huge_centre-488"][1]["cull_coord_max"])      # (a box at inf: no tables)
    assert i("no_big-488")["n_big"] == 0 and i("all_big-488")["n_big"] == 488 and i("all_big-488")["n_groups"] == i("all_big-488")["n_big_groups"] + 1
    assert i("negative-488")["basic_materials"] == 0 and i("volume-488")["basic_materials"] == 1 and i("cloud-2100-volume-1")["basic_materials"] == 0
    assert i("nonfinite-488")["n_big"] >= 70 and i("volume-1")["n_padded"] == 64 and i("volume-65")["n_padded"] == 128
    assert i("random_spheres")["n_big"] == 4 and i("random_spheres")["box_shared_axis"] == 2 and i("random_spheres")["cell_on"] == 1


@pytest.mark.parametrize("name", [k for k, _ in MESH_CASES])
def test_mesh_layout(layouts, name):
    m, g = layouts["meshes"][name]
    e = expected_mesh(m)
    assert g["null"] == 1, "a scene pointer of the template is not null"
    for k in ("first_leaf", "nppl", "leaf_sentinels_trailing", "lean_ok"):
        assert g[k] == e[k], (k, g[k], e[k])
    same(g["boxes"], e["boxes"], "bounds and floor")
    for k in ("tris", "bvh", "bvh_axis", "leaf_tri", "leaf_ofs", "moved"):
        same(g[k].view(np.uint8) if k in ("tris", "moved") else g[k], np.ascontiguousarray(e[k]).view(np.uint8) if k in ("tris", "moved") else e[k], k)
    same(g["materials"].view(np.uint8), np.ascontiguousarray(m["mats"]).view(np.uint8), "materials")
    assert list(g["tex_w"]) == [t.shape[1] for t in m["tex"]] and list(g["tex_h"]) == [t.shape[0] for t in m["tex"]]
    for got, t in zip(g["tex"], m["tex"]):
        same(got, t.reshape(-1), "texture")


def test_mesh_cases_reach_every_branch(layouts):
    g = {k: v[1] for k, v in layouts["meshes"].items()}
    assert len(g["hand-2x255"]["leaf_tri"]) == 2 * 255 * 12 and len(g["hand-2x256"]["leaf_tri"]) == 0 and len(g["hand-4x256"]["leaf_ofs"]) == 0
    assert g["sentinel_inside"]["leaf_sentinels_trailing"] == 0 and len(g["sentinel_inside"]["leaf_tri"]) == 0 and g["empty_leaf"]["leaf_sentinels_trailing"] == 1
    assert g["empty_leaf"]["leaf_ofs"].view(np.uint8)[2] == 0 and g["empty_leaf"]["leaf_ofs"].view(np.uint8)[:4].sum() > 0
    assert (g["presets"]["lean_ok"], g["textured"]["lean_ok"], g["hand-2x3"]["lean_ok"], g["staircase"]["lean_ok"]) == (0, 0, 1, 1)
    assert g["staircase"]["first_leaf"] == 1024 and g["staircase"]["nppl"] == 5 and g["staircase"]["leaf_sentinels_trailing"] == 1
    assert len(g["extra_slots"]["tris"]) == 4 * 3 + 5
