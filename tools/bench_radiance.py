"""radianceRays on one GPU against renderPixels of the same frame - recorded, nothing here is gated.

    python tools/bench_radiance.py [--nx 1200] [--ny 800] [--spp 16] [--runs 10] [--out profiles/radiance.json]

The bench scene (random spheres, 488 spheres, max depth 50).  In one process, after one warm-up call each:
  radiance   radianceRays of the nx x ny pixel-centre target rays of the scene camera from its origin (no lens, no jitter), ids = the index, spp samples:
             rtLastRadianceMs (HIP events around the kernels, not the copies) and the wall time of the call, `runs` times - median, min, max
  pixels     renderPixels of the full pixel list at spp samples: rtLastPixelsMs and the wall time, likewise
The two trace different rays - the pixels go through the lens and the jitter - so the ratio is informational.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, last_ms, runs):
    call()                                                  # warm-up: buffers allocated, code loaded
    kernel, wall = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(last_ms())
    brief = lambda a: dict(median=round(statistics.median(a), 4), min=round(min(a), 4), max=round(max(a), 4))
    return dict(kernel_ms=brief(kernel), wall_ms=brief(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=800)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt

    nx, ny = a.nx, a.ny
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    v = lambda x: np.array(list(x.e), np.float32)
    jj, ii = np.mgrid[0:ny, 0:nx]
    u = ((ii.ravel().astype(np.float32) + np.float32(0.5)) / np.float32(nx))[:, None]
    w = ((jj.ravel().astype(np.float32) + np.float32(0.5)) / np.float32(ny))[:, None]
    target = (v(cam.lower_left_corner) + u * v(cam.horizontal) + w * v(cam.vertical)).astype(np.float32)
    org = np.repeat(v(cam.origin)[None], nx * ny, axis=0)
    d = np.ascontiguousarray(target - org)
    ij = np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.int32)

    rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    try:
        res = dict(scene="random-spheres (488 spheres)", nx=nx, ny=ny, spp=a.spp, runs=a.runs, fp="parity",
                   radiance=timed(lambda: rt.radiance_rays(org, d, a.spp), rt.last_radiance_ms, a.runs),
                   pixels=timed(lambda: rt.render_pixels(ij, a.spp), rt.last_pixels_ms, a.runs))
        _, _, r_rays = rt.radiance_rays(org, d, a.spp, rays=True)
        _, _, p_rays = rt.render_pixels(ij, a.spp, rays=True)
        res["radiance"]["rays_per_sample"] = round(float(r_rays.sum(dtype=np.uint64)) / (nx * ny * a.spp), 4)
        res["pixels"]["rays_per_sample"] = round(float(p_rays.sum(dtype=np.uint64)) / (nx * ny * a.spp), 4)
    finally:
        rt.cleanupRenderer()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
