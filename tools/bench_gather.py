"""gatherRadiance on one GPU against the route a caller had before it - recorded, nothing here is gated.

    python tools/bench_gather.py [--nx 1200] [--ny 800] [--dirs 16] [--ns 1] [--runs 10] [--out profiles/gather.json]

The bench scene (random spheres, 488 spheres, max depth 50), PARITY.  The points are the first hits of renderGuides: position = origin + depth * d of the
centre ray, the normal plane, bias 1e-3; pixels that see the sky are left out.  RT_GATHER_IRRADIANCE at `dirs` directions per point, `ns` samples each.  In
one process, after one warm-up round, `runs` times - median, min, max:
  gather   gatherRadiance: rtLastGatherMs (HIP events around generator + trace + reduce, not the copies) and the wall time of the call
  host     the route without it: rtGatherDirectionsHost (wall), radianceRays on those rays (rtLastRadianceMs and wall), the per-point mean in numpy (wall)
The two must agree bit for bit - out and rays - and the tool asserts it.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def brief(a):
    return dict(median=round(statistics.median(a), 4), min=round(min(a), 4), max=round(max(a), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=800)
    ap.add_argument("--dirs", type=int, default=16)
    ap.add_argument("--ns", type=int, default=1)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt

    nx, ny, dirs, ns, bias = a.nx, a.ny, a.dirs, a.ns, 1e-3
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    jj, ii = np.mgrid[0:ny, 0:nx]
    o, d = rt.centre_rays(cam, nx, ny, np.stack([ii.ravel(), jj.ravel()], axis=1))
    rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    try:
        g = rt.renderGuides(rt.RT_GUIDE_NORMAL | rt.RT_GUIDE_DEPTH | rt.RT_GUIDE_PRIM)
        hit = g["prim"].ravel() != rt.RT_GUIDE_PRIM_NONE
        pos = np.ascontiguousarray((o + g["depth"].reshape(-1, 1) * d)[hit], dtype=np.float32)
        nrm = np.ascontiguousarray(g["normal"].reshape(-1, 3)[hit])
        n = len(pos)

        def gather():
            t0 = time.perf_counter()
            out, _, rays = rt.gather_radiance(pos, nrm, rt.RT_GATHER_IRRADIANCE, dirs, ns=ns, bias=bias, rays=True)
            return dict(wall=(time.perf_counter() - t0) * 1e3, kernel=rt.last_gather_ms()), out, rays

        def host():
            t0 = time.perf_counter()
            org, D, ids = rt.gather_directions_host(pos, nrm, rt.RT_GATHER_IRRADIANCE, dirs, bias=bias)
            t1 = time.perf_counter()
            L, _, r = rt.radiance_rays(org, D, ns, ids=ids, rays=True)
            t2 = time.perf_counter()
            kernel = rt.last_radiance_ms()
            L, A = L.reshape(n, dirs, 3), np.zeros((n, 3), np.float32)
            for m in range(dirs):                           # the definition's order: m ascending, one fp32 addition each
                A = A + L[:, m]
            out, rays = A / np.float32(dirs), r.reshape(n, dirs).sum(axis=1, dtype=np.uint64).astype(np.uint32)
            t3 = time.perf_counter()
            return dict(directions_wall=(t1 - t0) * 1e3, trace_wall=(t2 - t1) * 1e3, kernel=kernel, mean_wall=(t3 - t2) * 1e3, wall=(t3 - t0) * 1e3), out, rays

        rows = {"gather": [], "host": []}
        for run in range(a.runs + 1):                       # interleaved: both routes see the same machine
            tg, g_out, g_rays = gather()
            th, h_out, h_rays = host()
            assert np.array_equal(g_out.view(np.uint32), h_out.view(np.uint32)) and np.array_equal(g_rays, h_rays), "gatherRadiance differs from the host route"
            if run > 0:                                     # (round 0 warms up: buffers allocated, code loaded)
                rows["gather"].append(tg)
                rows["host"].append(th)
        res = dict(scene="random-spheres (488 spheres)", nx=nx, ny=ny, points=n, dirs=dirs, ns=ns, runs=a.runs, fp="parity", mode="irradiance", bit_equal=True,
                   rays_per_sample=round(float(g_rays.sum(dtype=np.uint64)) / (n * dirs * ns), 4),
                   bus_bytes=dict(gather=n * (24 + 12 + 12 + 4), host=n * dirs * (24 + 4 + 16 + 12 + 4)),
                   gather={k + "_ms": brief([r[k] for r in rows["gather"]]) for k in rows["gather"][0]},
                   host={k + "_ms": brief([r[k] for r in rows["host"]]) for k in rows["host"][0]})
        res["wall_ratio_host_over_gather"] = round(res["host"]["wall_ms"]["median"] / res["gather"]["wall_ms"]["median"], 2)
    finally:
        rt.cleanupRenderer()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
