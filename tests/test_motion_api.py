"""CPU checks of rtMarkPose / renderMotion (include/rt_api.h): the six calls are declared, exported and bound, the ABI version and the struct sizes are the
parent's, a call before init is the library's misuse exit, the new translation unit is built once with the accumulation's flags; and, from the test reference
alone (tests/motion_reference.py): its restatements of the two temporal passes equal the existing references bit for bit when the motion planes are P and n
themselves, the frames of the GPU tests cover every class of pixel, and the definition buys what it is there for - history taken from where the surface was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import accumulate_reference as A
import denoise_reference as D
import guides_reference as G
import motion_reference as M
import preview_reference as V
from preview_support import bits as _bits, exits_99, same as _same, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "include", "rt_api.h")).read()
NEW = ("rtMarkPose", "rtClearPose", "rtPoseMarked", "renderMotion", "rtLastMotionMs")


def test_declared_exported_and_bound(rt):
    assert re.search(r"void\s+rtMarkPose\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"void\s+rtClearPose\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"int\s+rtPoseMarked\s*\(\s*void\s*\)\s*;", API)
    assert re.search(r"enum\s*\{\s*RT_MOTION_POS\s*=\s*1\s*,\s*RT_MOTION_NORMAL\s*=\s*2\s*,\s*RT_MOTION_SCREEN\s*=\s*4\s*\}\s*;", API)
    assert re.search(r"void\s+renderMotion\s*\(\s*int\s+mask\s*,\s*const\s+rt_camera\s*\*\s*prev_cam\s*,\s*float\s*\*\s*prev_pos\s*,\s*float\s*\*\s*prev_normal\s*,"
                     r"\s*float\s*\*\s*screen\s*\)\s*;", API)
    assert re.search(r"double\s+rtLastMotionMs\s*\(\s*void\s*\)\s*;", API)
    lib = C.CDLL(os.path.join(ROOT, "cuda-raytracing-optimized_amd", "librt_mi355x.so"))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in rt.RENDERER_SYMBOLS
    r = rt.load_renderer()
    fp = C.POINTER(C.c_float)
    assert r.renderMotion.argtypes == [C.c_int, C.POINTER(rt.camera), fp, fp, fp] and r.renderMotion.restype is None
    assert r.rtMarkPose.argtypes == [] and r.rtMarkPose.restype is None and r.rtClearPose.argtypes == [] and r.rtClearPose.restype is None
    assert r.rtPoseMarked.restype is C.c_int and r.rtLastMotionMs.restype is C.c_double
    assert (rt.RT_MOTION_POS, rt.RT_MOTION_NORMAL, rt.RT_MOTION_SCREEN) == (M.POS, M.NORMAL, M.SCREEN) == (1, 2, 4)
    for fn in (rt.mark_pose, rt.clear_pose, rt.pose_marked, rt.last_motion_ms, rt.renderMotion):
        assert callable(fn)


def test_abi_unchanged(rt):
    assert rt.load_renderer().rtApiVersion() == 1002 == rt.RT_API_VERSION
    assert re.search(r"#define RT_API_VERSION 1002\b", API)
    sizes = (C.c_int32 * 32)()
    n = rt.load_renderer().rtStructSizes(sizes, 32)
    assert n == 13 and [sizes[k] for k in range(n)] == [C.sizeof(s) for s in rt.ABI_STRUCTS]


@pytest.mark.parametrize("call", ["rt.mark_pose()", "rt.clear_pose()", "rt.pose_marked()", "rt.last_motion_ms()", "rt.renderMotion()",
                                  "a = np.zeros((4, 4, 3), np.float32); p = a.ctypes.data_as(C.POINTER(C.c_float)); rt.load_renderer().renderMotion(1, None, p, None, None)"])
def test_before_init_exits_99(call):
    """The library's misuse convention in a child process: 'rt error' on stderr and exit status 99.  No GPU: the check precedes any HIP call."""
    exits_99("rt._state.update(nx=4, ny=4)\n%s\n" % call)


def test_translation_unit_is_built_once_with_the_accumulation_s_flags():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    rules = re.findall(r"^\$\(OBJ\)/(\S+)\.o:\s*\$\(CSRC\)/rt_kernels_motion\.hip([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert len(rules) == 1 and rules[0][0] == "motion", rules
    assert "$(CSRC)/rt_motion.h" in rules[0][1].split()
    accumulate = re.search(r"^\$\(OBJ\)/accumulate\.o:[^\n]*\n\t([^\n]+)", mk, re.M).group(1)
    assert rules[0][2].split() == accumulate.split()            # the same command
    assert "$(CSRC)/rt_motion.h" in re.search(r"^\$\(OBJ\)/renderer\.o:([^\n]*)", mk, re.M).group(1).split()
    link = re.search(r"^\$\(PKG\)/librt_mi355x\.so:([^\n]*)\n\t([^\n]+)", mk, re.M)
    assert "$(MOTION_OBJS)" in link.group(1).split() and "$(MOTION_OBJS)" in link.group(2).split()
    csrc = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")
    seen = [f for f in sorted(os.listdir(csrc)) if '#include "rt_motion.h"' in open(os.path.join(csrc, f)).read()]
    assert seen == ["rt_kernels_motion.hip", "rt_renderer.hip"], seen


# ---- the restatements are pinned ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,calls", [("three_spheres", 3), ("random_50x37", 2), ("staircase_a", 2)])
def test_restatements_equal_the_existing_references(rt, O, name, calls):
    """With Pm = P and nm = n (no motion planes passed) MotionAccumulator is accumulate_reference.Accumulator and MotionPreviewer is preview_reference.Previewer,
    bit for bit, over the existing sequences with seeded inputs."""
    flags = D.default_flags(name in G.MESH_FRAMES)
    acc, macc, pre, mpre = A.Accumulator(), M.MotionAccumulator(), V.Previewer(), M.MotionPreviewer()
    for k in range(calls):
        cam, g, origin, dn = A.sequence_inputs(rt, O, name, k)
        src = synthetic(40 + k, *g["prim"].shape)
        ref, got = acc.step(src, g, cam, origin, dn, flags=flags), macc.step(src, g, cam, origin, dn, flags=flags)
        for a, b, what in zip(ref, got, ("out", "history")):
            _same(b, a, f"{name} call {k} accumulate {what}")
        ref, got = pre.step(src, g, cam, origin, dn, flags=flags), mpre.step(src, g, cam, origin, dn, flags=flags)
        for a, b, what in zip(ref, got, ("out", "history", "variance")):
            _same(b, a, f"{name} call {k} preview {what}")
    assert float(ref[1].max()) > 1.0                            # the last call did blend


# ---- coverage ----------------------------------------------------------------------------------------------------------------

def test_staircase_edit_covers_moved_unmoved_and_turned_pixels(rt, O):
    cam, g, origin, dn, live, previous = M.stair_inputs(rt, O, 1)
    mp = M.motion_planes(g, origin, dn, live, previous)
    npix = mp["moved"].size
    ids = live["meshID"][np.clip(g["prim"], 0, len(live) - 1)]
    on_moved = (g["prim"] >= 0) & np.isin(ids, M.MOVED_IDS)
    print(f"staircase_a frame 1: {int(mp['moved'].sum())} moved, {int((~mp['moved']).sum())} unmoved of {npix}; {int(mp['turned'].sum())} moved and turned")
    assert np.array_equal(on_moved, mp["moved"])                # every triangle of the two objects moved, and nothing else
    assert mp["moved"].sum() >= 0.25 * npix and (~mp["moved"]).sum() >= 0.25 * npix
    assert mp["turned"].sum() >= 50
    still = ~mp["moved"] & (g["prim"] != G.PRIM_NONE)
    for a in range(3):                                          # what did not move: P and n themselves
        assert np.array_equal(_bits(mp["Pm"][a])[still], _bits(mp["P"][a])[still])
        assert np.array_equal(_bits(mp["nm"][a])[still], _bits(g["normal"][..., a])[still])


def test_tiny_mesh_covers_floor_miss_moved_and_unmoved(rt, O):
    t = M.tiny_frame(rt, O, 33, 9)
    g, count = t["g"], t["count"]
    mp = M.motion_planes(g, t["origin"], t["dn"], t["live"], t["first"])
    classes = dict(floor=int((g["prim"] == G.PRIM_FLOOR).sum()), miss=int((g["prim"] == G.PRIM_NONE).sum()), moved=int(mp["moved"].sum()),
                   unmoved=int(((g["prim"] >= 0) & ~mp["moved"]).sum()))
    print("tris300_floor 33 x 9:", classes, "triangles moved:", count)
    assert count == 20 and all(v > 0 for v in classes.values()), classes


# ---- the definition means what it says -----------------------------------------------------------------------------------------

def test_history_comes_from_where_the_surface_was(rt, O):
    """Frame 0 (unedited, camera 0) gets its own world positions as the input, flags 0: the colour history IS the position history.  In frame 1 (the edit,
    camera 1) h = sum / wsum of a blended pixel is then the point of frame 0 its history was taken from - to be compared with Pm, where its surface point was.
    Conditions on the inputs, from the reference alone."""
    cam0, g0, o0, dn0, live0, _ = M.stair_inputs(rt, O, 0)
    cam1, g1, o1, dn1, live, previous = M.stair_inputs(rt, O, 1)
    P0 = np.stack(M.hit_points(g0, o0, dn0), axis=-1)
    mp = M.motion_planes(g1, o1, dn1, live, previous, prev_cam=cam0)
    plain = M.motion_planes(g1, o1, dn1, prev_cam=cam0)
    res = {}
    for what, planes in (("marked", mp), ("unmarked", plain)):
        acc, info = M.MotionAccumulator(), {}
        acc.step(P0, g0, cam0, o0, dn0, flags=0)
        acc.step(np.zeros_like(P0), g1, cam1, o1, dn1, planes["Pm"], planes["nm"], flags=0, info=info)
        use = info["use"] & mp["moved"]
        h = np.stack(info["h"], axis=-1).astype(np.float64)
        err = np.linalg.norm(h - mp["prev_pos"].astype(np.float64), axis=-1) / g1["depth"].astype(np.float64)
        res[what] = dict(blended=int(use.sum()), median=float(np.median(err[use])), x=info["x"], y=info["y"])
    moved = int(mp["moved"].sum())
    print(f"moved pixels {moved}; blended with the mark {res['marked']['blended']}, without {res['unmarked']['blended']}; "
          f"median |h - Pm| / t with the mark {res['marked']['median']:.3e}, without {res['unmarked']['median']:.3e}")
    assert res["marked"]["median"] <= 1e-3
    assert res["marked"]["median"] * 10 <= res["unmarked"]["median"]
    assert res["marked"]["blended"] >= 0.9 * moved
    assert res["marked"]["blended"] >= 1.5 * res["unmarked"]["blended"]
    still = ~mp["moved"] & (g1["prim"] != G.PRIM_NONE)
    for k in ("x", "y"):
        assert np.array_equal(_bits(res["marked"][k])[still], _bits(res["unmarked"][k])[still])
    assert np.array_equal(_bits(mp["screen"])[still], _bits(plain["screen"])[still])
