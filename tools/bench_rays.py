"""The batched ray queries (traceRays / occludedRays) on one GPU: the guide pass's own rays, incoherent rays, and what a small batch costs end to end.

    python tools/bench_rays.py [--cases C2,C4] [--repeats 15] [--out profiles/rays.json]

C2: random spheres 1200x800 (the bench frame).  C4: the staircase mesh 1920x1080.  Per case one JSON line, every figure the median of --repeats calls after
three warm-up calls, kernel times from rtLastRaysMs / rtLastGuidesMs (HIP events), wall times around the Python call:
  centre      the centre rays of every pixel (rt.centre_rays) through trace_rays with the planes t, prim, normal (+ nodes), against renderGuides with normal,
              depth, prim (+ nodes) of the same frame: same rays, same arithmetic; centre_ratio = ray kernel / guide kernel
  incoherent  1 M seeded rays, origins uniform in the scene's extent, directions uniform on the sphere: Mrays/s of the closest-hit and the any-hit kernel;
              incoherent_to_centre = that closest-hit rate / the centre rays' rate (the price of one lane per ray without sorting)
  small       wall and kernel ms of trace_rays at 1, 1 k and 1 M rays (t and prim only): what a pick costs end to end"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "C2": dict(kind="spheres", nx=1200, ny=800, depth=50),
    "C4": dict(kind="mesh", nx=1920, ny=1080, depth=64, detail=4),
}


def open_case(rt, w):
    """Initialises the case; returns (camera, extent lo, extent hi, keepalive)."""
    if w["kind"] == "spheres":
        sp, mt, cam = rt.scene_random_spheres(w["nx"], w["ny"])
        rt.initRendererSpheres(sp, mt, cam, w["nx"], w["ny"], w["depth"])
        return cam, np.array([-12.0, 0.0, -12.0]), np.array([12.0, 3.0, 12.0]), None
    tris, mats = rt.scene_staircase_procedural(w["detail"])
    hm = rt.HostMesh.build(tris, 5)
    ks, keep = rt.make_kernel_scene(hm, mats)
    cam = rt.staircase_camera(w["nx"], w["ny"])
    rt.initRenderer(ks, cam, w["nx"], w["ny"], w["depth"], keepalive=keep)
    b = hm.view.bounds
    return cam, np.array([b.min.e[a] for a in range(3)]), np.array([b.max.e[a] for a in range(3)]), (hm, keep)


def timed(rt, call, repeats):
    """(median kernel ms, median wall ms) of `call` after three warm-up calls."""
    for _ in range(3):
        call()
    kernel, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(rt.last_rays_ms())
    return statistics.median(kernel), statistics.median(wall)


def run_case(rt, name, w, repeats):
    cam, lo, hi, keep = open_case(rt, w)
    mesh = w["kind"] == "mesh"
    nx, ny = w["nx"], w["ny"]
    r4 = lambda x: round(float(x), 4)
    line = dict(case=name, kind=w["kind"], nx=nx, ny=ny, repeats=repeats)

    # the guide pass's own rays
    ij = np.stack(np.meshgrid(np.arange(nx), np.arange(ny)), axis=-1).reshape(-1, 2).astype(np.int32)     # row-major: (i, j) of pixel j * nx + i
    org, d = rt.centre_rays(cam, nx, ny, ij)
    n = len(org)
    g_mask = rt.RT_GUIDE_NORMAL | rt.RT_GUIDE_DEPTH | rt.RT_GUIDE_PRIM | (rt.RT_GUIDE_NODES if mesh else 0)
    r_mask = rt.RT_RAY_T | rt.RT_RAY_PRIM | rt.RT_RAY_NORMAL | (rt.RT_RAY_NODES if mesh else 0)
    g_out = rt.renderGuides(g_mask)
    for _ in range(3):
        rt.renderGuides(g_mask, out=g_out)
    g_kernel = []
    for _ in range(repeats):
        rt.renderGuides(g_mask, out=g_out)
        g_kernel.append(rt.last_guides_ms())
    r_out = rt.trace_rays(org, d, mask=r_mask)
    same = all(np.array_equal(r_out[a].view(np.uint32).reshape(-1), g_out[b].view(np.uint32).reshape(-1))
               for a, b in (("t", "depth"), ("prim", "prim"), ("normal", "normal")))
    c_kernel, c_wall = timed(rt, lambda: rt.trace_rays(org, d, mask=r_mask, out=r_out), repeats)
    occ = rt.occluded_rays(org, d)
    a_kernel, a_wall = timed(rt, lambda: rt.occluded_rays(org, d, out=occ), repeats)
    g_med = statistics.median(g_kernel)
    line.update(centre_rays=n, centre_equals_guides=bool(same), guides_kernel_ms=r4(g_med), centre_kernel_ms=r4(c_kernel), centre_wall_ms=r4(c_wall),
                centre_ratio=r4(c_kernel / g_med), centre_mrays_s=r4(n / c_kernel / 1e3), centre_any_kernel_ms=r4(a_kernel),
                centre_any_mrays_s=r4(n / a_kernel / 1e3), centre_hit_share=r4((r_out["prim"] != rt.RT_GUIDE_PRIM_NONE).mean()))

    # incoherent rays
    rng = np.random.default_rng(2024)
    m = 1 << 20
    ro = rng.uniform(lo, hi, (m, 3)).astype(np.float32)
    rd = rng.normal(size=(m, 3))
    rd = (rd / np.sqrt((rd * rd).sum(axis=1, keepdims=True))).astype(np.float32)
    i_out = rt.trace_rays(ro, rd, mask=r_mask)
    i_kernel, i_wall = timed(rt, lambda: rt.trace_rays(ro, rd, mask=r_mask, out=i_out), repeats)
    i_occ = rt.occluded_rays(ro, rd)
    ia_kernel, ia_wall = timed(rt, lambda: rt.occluded_rays(ro, rd, out=i_occ), repeats)
    line.update(incoherent_rays=m, incoherent_kernel_ms=r4(i_kernel), incoherent_wall_ms=r4(i_wall), incoherent_mrays_s=r4(m / i_kernel / 1e3),
                incoherent_any_kernel_ms=r4(ia_kernel), incoherent_any_wall_ms=r4(ia_wall), incoherent_any_mrays_s=r4(m / ia_kernel / 1e3),
                incoherent_to_centre=r4((m / i_kernel) / (n / c_kernel)), incoherent_hit_share=r4((i_out["prim"] != rt.RT_GUIDE_PRIM_NONE).mean()),
                incoherent_occluded_share=r4(i_occ.mean()))
    if mesh:
        line.update(centre_nodes_mean=r4(r_out["nodes"].mean()), incoherent_nodes_mean=r4(i_out["nodes"].mean()))

    # a pick end to end
    small = {}
    for k in (1, 1000, m):
        s_out = rt.trace_rays(ro[:k], rd[:k], mask=rt.RT_RAY_T | rt.RT_RAY_PRIM)
        s_kernel, s_wall = timed(rt, lambda: rt.trace_rays(ro[:k], rd[:k], mask=rt.RT_RAY_T | rt.RT_RAY_PRIM, out=s_out), repeats)
        small[str(k)] = dict(kernel_ms=r4(s_kernel), wall_ms=r4(s_wall))
    line["small"] = small
    rt.cleanupRenderer()
    del keep
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="C2,C4")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    if rt.device_count() < 1:
        raise SystemExit("bench_rays: no HIP device visible")
    lines = []
    for name in args.cases.split(","):
        line = run_case(rt, name, CASES[name], args.repeats)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
