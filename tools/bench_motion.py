"""The marked pose and the motion planes (rtMarkPose / renderMotion) beside the guide kernel, and the temporal passes with and without a mark, on one GPU.

    python tools/bench_motion.py [--cases spheres,mesh] [--repeats 20] [--out profiles/motion.json] [--root build/ab/<tree>]

Both cases at 1200 x 800: the random spheres and the procedural staircase.  The camera alternates between two positions (spheres: one degree of an orbit
apart, mesh: 0.05 sideways), so every timed call reprojects into a different previous frame.  Per case one JSON line with medians (and the spread as
max - min) of --repeats, every figure a HIP-event time of the kernels alone:
  * accumulate_ms / preview_ms: rtLastAccumulateMs / rtLastPreviewMs of synthetic input WITHOUT a marked pose - the figures to hold against another build;
and, where the library has the calls:
  * accumulate_marked_ms / preview_marked_ms: the same with a pose marked and a share of the scene moved in front of every call;
  * motion_ms beside guides_ms: rtLastMotionMs of renderMotion (all three planes) and rtLastGuidesMs of renderGuides for the same frame - the traversal
    the projection avoids;
  * mark_pose_ms: the wall time of rtMarkPose (a device-to-device copy of the slots, or the upload of the spheres).
--root: a directory that holds another build of the package (its cuda-raytracing-optimized_amd/ with the libraries, cuda_raytracing_optimized_amd.py and
include/), e.g. the parent commit's, for an A/B in the same job; the figures it cannot measure are left out."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"spheres": dict(kind="spheres", nx=1200, ny=800, depth=50), "mesh": dict(kind="mesh", nx=1200, ny=800, depth=16, detail=1)}


def cameras(rt, w):
    if w["kind"] == "spheres":
        def orbit(deg):
            a = math.radians(deg)
            return rt.make_camera((math.cos(a) * 13 + math.sin(a) * 3, 2, -math.sin(a) * 13 + math.cos(a) * 3), (0, 0, 0), (0, 1, 0), 30.0, w["nx"] / w["ny"], 0.1, 10.0)
        return [orbit(0.0), orbit(1.0)]
    cams = []
    for amount in (0.0, 0.05):
        cam = rt.staircase_camera(w["nx"], w["ny"])
        for a in range(3):
            cam.origin.e[a] += amount * cam.u.e[a]
            cam.lower_left_corner.e[a] += amount * cam.u.e[a]
        cams.append(cam)
    return cams


def run_case(rt, name, w, repeats):
    nx, ny = w["nx"], w["ny"]
    if w["kind"] == "spheres":
        sp, mt, cam = rt.scene_random_spheres(nx, ny)
        rt.initRendererSpheres(sp, mt, cam, nx, ny, w["depth"])
        poses = [sp, sp.copy()]
        poses[1]["center"][1::5] += np.float32(0.05)
        edit = lambda k: rt.update_spheres(poses[k & 1], mt)
        keep = None
    else:
        tris, mats = rt.scene_staircase_procedural(w["detail"])
        hm = rt.HostMesh.build(tris, 5)
        ks, keep = rt.make_kernel_scene(hm, mats)
        rt.initRenderer(ks, rt.staircase_camera(nx, ny), nx, ny, w["depth"], keepalive=keep)
        poses = [hm.tris.copy(), hm.tris.copy()]
        sel = ~np.isinf(poses[1]["v"][:, 0, 0]) & np.isin(poses[1]["meshID"], (12, 19))
        poses[1]["v"][sel] += np.float32(0.01)
        edit = lambda k: rt.update_triangles(0, poses[k & 1])
    cams = cameras(rt, w)
    src = np.random.default_rng(3).uniform(0, 4, (ny, nx, 3)).astype(np.float32)
    out = np.empty_like(src)
    med, spread = statistics.median, lambda x: max(x) - min(x)
    res = dict(case=name, kind=w["kind"], nx=nx, ny=ny, repeats=repeats)

    def passes(marked):
        acc, pre = [], []
        rt.reset_history(); rt.reset_preview()
        for k in range(repeats + 4):                            # four warm-up calls: code objects, first touch of the buffers
            if marked:
                rt.mark_pose()
                edit(k + 1)
            rt.setCamera(cams[k & 1])
            rt.accumulateFrame(src, out=out)
            rt.previewFrame(src, out=out)
            if k >= 4:
                acc.append(rt.last_accumulate_ms()); pre.append(rt.last_preview_ms())
        return acc, pre

    acc, pre = passes(False)
    res.update(accumulate_ms=round(med(acc), 4), accumulate_spread_ms=round(spread(acc), 4), preview_ms=round(med(pre), 4), preview_spread_ms=round(spread(pre), 4))
    if hasattr(rt, "mark_pose"):
        acc, pre = passes(True)
        res.update(accumulate_marked_ms=round(med(acc), 4), preview_marked_ms=round(med(pre), 4))
        motion, guides, mark = [], [], []
        for k in range(repeats + 2):
            t0 = time.perf_counter()
            rt.mark_pose()
            t1 = time.perf_counter()
            edit(k + 1)
            rt.setCamera(cams[k & 1])
            rt.renderMotion(cams[~k & 1])
            rt.renderGuides()
            if k >= 2:
                motion.append(rt.last_motion_ms()); guides.append(rt.last_guides_ms()); mark.append((t1 - t0) * 1e3)
        res.update(motion_ms=round(med(motion), 4), motion_spread_ms=round(spread(motion), 4), guides_ms=round(med(guides), 4),
                   mark_pose_ms=round(med(mark), 4), motion_to_guides=round(med(motion) / med(guides), 4))
    rt.cleanupRenderer()
    del keep
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="spheres,mesh")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root) if args.root else ROOT
    sys.path.insert(0, root)
    import cuda_raytracing_optimized_amd as rt
    if rt.device_count() < 1:
        raise SystemExit("bench_motion: no HIP device visible")
    lines = []
    for name in args.cases.split(","):
        line = run_case(rt, name, CASES[name], args.repeats)
        line["root"] = os.path.relpath(root, ROOT)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
