"""Scene edits on one GPU: what updateTriangles costs against the path it replaces.

    python tools/bench_update.py [--detail 4] [--repeats 15] [--out profiles/update.json]

The procedural staircase at --detail, 5 triangles per leaf, 1920x1080 (the image only sizes the framebuffer: no frame is rendered).  One JSON line, every figure
the median of --repeats calls after three warm-up calls; kernel times from rtLastUpdateMs (HIP events around the refit kernels), wall times around the call:
  all      updateTriangles of every slot: the whole mesh moves (64 bytes per slot over the bus, one refit)
  object   updateTriangles of the slots of one object, the steel ball (mesh id 12): first .. last of its slots in leaf order
  reinit   the path an edit took before: cleanupRenderer + initRenderer of the same edited scene - once with the host's rtRefitBvh in front (the caller has
           to refit either way to get valid boxes), once without
The edited triangles alternate between two seeded versions, so every call changes every box.  all_equals_twin: the device's nodes after the last edit against
rtRefitBvh's, bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BALL = 12


def timed(call, repeats, kernel_ms=None):
    """(median wall ms, median kernel ms or None) of call(k), k the call's number, after three warm-up calls."""
    for k in range(3):
        call(k)
    wall, kernel = [], []
    for k in range(repeats):
        t0 = time.perf_counter()
        call(3 + k)
        wall.append((time.perf_counter() - t0) * 1e3)
        if kernel_ms:
            kernel.append(kernel_ms())
    return statistics.median(wall), (statistics.median(kernel) if kernel else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--detail", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    if rt.device_count() < 1:
        raise SystemExit("bench_update: no HIP device visible")
    nx, ny, depth = 1920, 1080, 64
    tris, mats = rt.scene_staircase_procedural(args.detail)
    hm = rt.HostMesh.build(tris, 5)
    cam = rt.staircase_camera(nx, ny)
    ks, keep = rt.make_kernel_scene(hm, mats)
    rt.initRenderer(ks, cam, nx, ny, depth, keepalive=keep)
    r4 = lambda x: round(float(x), 4)

    base = hm.tris.copy()
    real = ~np.isinf(base["v"][:, 0, 0])
    rng = np.random.default_rng(2025)
    versions = []
    for _ in range(2):
        v = base.copy()
        v["v"][real] = v["v"][real] + rng.uniform(-0.5, 0.5, (int(real.sum()), 3, 3)).astype(np.float32)
        versions.append(v)
    sel = np.flatnonzero(real & (base["meshID"] == BALL))
    first, last = int(sel.min()), int(sel.max())
    pieces = [np.ascontiguousarray(v[first:last + 1]) for v in versions]

    all_wall, all_kernel = timed(lambda k: rt.update_triangles(0, versions[k & 1]), args.repeats, rt.last_update_ms)
    hm.tris[:] = versions[(3 + args.repeats - 1) & 1]
    hm.refit()
    nodes, _ = rt.mesh_bvh()
    equal = bool(np.array_equal(nodes.view(np.uint32), hm.bvh.view(np.uint32)))
    obj_wall, obj_kernel = timed(lambda k: rt.update_triangles(first, pieces[k & 1]), args.repeats, rt.last_update_ms)

    def reinit(k, refit):
        hm.tris[:] = versions[k & 1]
        t0 = time.perf_counter()
        if refit:
            hm.refit()
        host = (time.perf_counter() - t0) * 1e3
        rt.cleanupRenderer()
        rt.initRenderer(ks, cam, nx, ny, depth, keepalive=keep)
        return host

    host_ms = []
    re_wall, _ = timed(lambda k: host_ms.append(reinit(k, True)), args.repeats)
    bare_wall, _ = timed(lambda k: reinit(k, False), args.repeats)
    rt.cleanupRenderer()

    line = dict(scene="staircase_procedural", detail=args.detail, nppl=5, nx=nx, ny=ny, repeats=args.repeats, triangles=int(real.sum()), slots=int(len(base)),
                bvh_nodes=int(hm.view.numBvhNodes), refit_launches=int(np.ceil(np.log2(hm.view.numBvhNodes // 2) / 8)),
                all_wall_ms=r4(all_wall), all_kernel_ms=r4(all_kernel), all_equals_twin=equal,
                object_slots=last - first + 1, object_triangles=int(len(sel)), object_wall_ms=r4(obj_wall), object_kernel_ms=r4(obj_kernel),
                reinit_with_host_refit_wall_ms=r4(re_wall), host_refit_ms=r4(statistics.median(host_ms[3:])), reinit_wall_ms=r4(bare_wall),
                reinit_over_all=r4(bare_wall / all_wall), reinit_over_object=r4(bare_wall / obj_wall))
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump([line], f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
