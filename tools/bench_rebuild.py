"""rebuildBvh on one GPU: what a rebuild costs against the path it replaces, and what the rebuilt tree is worth.

    python tools/bench_rebuild.py [--detail 4] [--repeats 15] [--frames 5] [--stages rebuild,reinit,frames] [--out profiles/rebuild.json]

The procedural staircase at --detail, 5 triangles per leaf, 1920x1080, scrambled: the real triangles permuted among the real slots with a fixed seed and
refitted - a correct tree whose boxes overlap everywhere.  One JSON line per run; --out is read first and updated, so the stages may run one by one:
  rebuild   (a) rebuildBvh of the scrambled tree: wall time around the Python call and rtLastRebuildMs (HIP events around the build and refit kernels), medians
            of --repeats calls after three warm-up calls; the triangles are scrambled again (updateTriangles, not timed) before every call, so every call does
            the same kind of work.  launches: kernel launches per rebuild, build + refit.  equals_twin: the device's nodes and old_slot after the last call
            against rtRebuildBvh's, bit for bit.
  reinit    (b) the path a rebuild took before: rtBuildBvhLevels of the same triangles on the host + cleanupRenderer + initRenderer, the same medians.
  frames    (c) on the scrambled tree, the rebuilt tree and the tree rtBuildBvh built from the triangles in their original order: node visits per sample
            (a counters = 1 frame of 480x270 at 4 spp - the counting kernel pays a device atomic per event, and the scrambled tree has some 25 times
            the events) and the kernel time of --frames frames of 1920x1080 at 16 spp (median, min, max: the run-to-run spread; the scrambled tree: one
            frame without a warm-up, it is slow).  The built and the rebuilt tree alternate, frame by frame, in two renderer lifetimes each."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPP = 16


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--detail", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--stages", default="rebuild,reinit,frames")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stages = set(args.stages.split(","))
    import cuda_raytracing_optimized_amd as rt
    if rt.device_count() < 1:
        raise SystemExit("bench_rebuild: no HIP device visible")
    nx, ny, depth = 1920, 1080, 64
    tris, mats = rt.scene_staircase_procedural(args.detail)
    built = rt.HostMesh.build(tris, 5)
    hm = rt.HostMesh.build(tris, 5)
    cam = rt.staircase_camera(nx, ny)
    r4 = lambda x: round(float(x), 4)
    real = np.flatnonzero(~np.isinf(hm.tris["v"][:, 0, 0]))
    scrambled = hm.tris.copy()
    scrambled[real] = scrambled[real][np.random.default_rng(71).permutation(len(real))]
    hm.tris[:] = scrambled
    hm.refit()
    first_leaf = hm.view.numBvhNodes // 2
    levels = int(math.log2(first_leaf))
    line = {}
    if args.out and os.path.exists(args.out):
        line = json.load(open(args.out))[0]
    line.update(scene="staircase_procedural", detail=args.detail, nppl=5, nx=nx, ny=ny, spp=SPP, repeats=args.repeats, triangles=int(len(real)),
                slots=int(len(scrambled)), bvh_nodes=int(hm.view.numBvhNodes), levels=levels)

    def init(mesh, w=nx, h=ny):
        ks, keep = rt.make_kernel_scene(mesh, mats)
        rt.initRenderer(ks, rt.staircase_camera(w, h), w, h, depth, keepalive=keep)
        return rt.getDefaultRenderOptions(False)

    if "rebuild" in stages:
        # (a) every call from a freshly scrambled tree
        init(hm)
        wall, kernel = [], []
        sentinel = np.zeros(1, rt.triangle_dtype)
        sentinel["v"] = np.inf
        cur = scrambled.copy()
        rng = np.random.default_rng(72)
        for k in range(3 + args.repeats):
            t0 = time.perf_counter()
            old = rt.rebuild_bvh()
            w = (time.perf_counter() - t0) * 1e3
            if k >= 3:
                wall.append(w)
                kernel.append(rt.last_rebuild_ms())
            say(f"rebuild {k}: wall {w:.3f} ms, kernels {rt.last_rebuild_ms():.3f} ms")
            before = cur
            cur = np.where(old >= 0, before[np.maximum(old, 0)], sentinel[0])      # the slots as the device holds them now
            if k + 1 < 3 + args.repeats:                        # scrambled again (not timed): a slot's sentinel state must stay, so within the new real slots
                now = np.flatnonzero(~np.isinf(cur["v"][:, 0, 0]))
                cur[now] = cur[now][rng.permutation(len(now))]
                rt.update_triangles(0, cur)
        twin = rt.HostMesh.build(tris, 5)
        twin.tris[:] = before
        want = twin.rebuild()
        nodes, _ = rt.mesh_bvh()
        equal = bool(np.array_equal(old, want) and np.array_equal(nodes.view(np.uint32), twin.bvh.view(np.uint32)))
        rt.cleanupRenderer()
        launches = 29 + 10 * levels + int(math.ceil(levels / 8))   # gather 6, sort 4 x 5, per level 10, emit 3; the refit: one launch per 8 levels
        line.update(launches_per_rebuild=launches, rebuild_wall_ms=r4(statistics.median(wall)), rebuild_wall_min_ms=r4(min(wall)), rebuild_wall_max_ms=r4(max(wall)),
                    rebuild_kernel_ms=r4(statistics.median(kernel)), rebuild_kernel_min_ms=r4(min(kernel)), rebuild_kernel_max_ms=r4(max(kernel)),
                    equals_twin=equal)

    if "reinit" in stages:
        # (b) the path it replaces: the builder on the host and a new init
        visible = scrambled[real]
        re_wall, host = [], []
        init(built)
        for k in range(3 + args.repeats):
            t0 = time.perf_counter()
            fresh = rt.HostMesh.build(visible, 5)
            t1 = time.perf_counter()
            rt.cleanupRenderer()
            init(fresh)
            t2 = time.perf_counter()
            say(f"reinit {k}: host build {(t1 - t0) * 1e3:.1f} ms, cleanup + init {(t2 - t1) * 1e3:.1f} ms")
            if k >= 3:
                re_wall.append((t2 - t0) * 1e3)
                host.append((t1 - t0) * 1e3)
        rt.cleanupRenderer()
        line.update(reinit_wall_ms=r4(statistics.median(re_wall)), reinit_wall_min_ms=r4(min(re_wall)), reinit_wall_max_ms=r4(max(re_wall)),
                    host_build_ms=r4(statistics.median(host)))
    if "rebuild_wall_ms" in line and "reinit_wall_ms" in line:
        line["reinit_over_rebuild"] = r4(line["reinit_wall_ms"] / line["rebuild_wall_ms"])

    if "frames" in stages:
        rebuilt = rt.HostMesh.build(tris, 5)
        rebuilt.tris[:] = scrambled
        rebuilt.rebuild()
        trees = (("built", built), ("rebuilt", rebuilt), ("scrambled", hm))
        visits = {}
        for name, mesh in trees:                                # node visits per sample: a small counted frame
            o = init(mesh, 480, 270)
            rt.setRenderOptions(o, counters=1)
            rt.runRenderer(4)
            visits[name] = r4(rt.getRenderStats().node_visits / float(480 * 270 * 4))
            rt.cleanupRenderer()
            say(f"node visits per sample, {name}: {visits[name]}")
        ms = {"built": [], "rebuilt": []}
        for life in range(2):                                   # the two good trees alternate: two renderer lifetimes each, frames interleaved in time
            for name, mesh in trees[:2]:
                init(mesh)
                rt.runRenderer(SPP)                             # warm-up
                for _ in range(args.frames):
                    rt.runRenderer(SPP)
                    ms[name].append(rt.getRenderStats().kernel_ms)
                rt.cleanupRenderer()
                say(f"frames, {name}, lifetime {life}: {[round(x, 3) for x in ms[name][-args.frames:]]}")
        init(hm)
        rt.runRenderer(SPP)
        ms_bad = [rt.getRenderStats().kernel_ms]
        rt.cleanupRenderer()
        say(f"frame, scrambled: {ms_bad}")

        def spread(v):
            return dict(median_ms=r4(statistics.median(v)), min_ms=r4(min(v)), max_ms=r4(max(v)), frames=len(v))

        line.update(node_visits_per_sample=visits, frame_scrambled=spread(ms_bad), frame_rebuilt=spread(ms["rebuilt"]), frame_built=spread(ms["built"]))

    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump([line], f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
