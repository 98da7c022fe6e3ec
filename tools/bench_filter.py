"""filterTexels on one GPU: what it costs against denoiseFrame's iteration, what the device-resident plane saves, and what it does to a real bake's error -
recorded, nothing here is gated but the bits.

    python tools/bench_filter.py [--size 1024] [--dirs 16] [--ref-dirs 4096] [--dilate 2] [--runs 7] [--commit HASH] [--out profiles/filter.json]

The procedural staircase with the atlas of rtAtlasGrid (margin 0.05), a size x size atlas, PARITY: the workload of tools/bench_bake.py.  In one process, after a
warm-up, `runs` times each - median, min, max:
  time      rtLastFilterMs of a call of k = 1 .. 4 iterations at C = 1, 3 and 27, with the colour weight (sigma_c 0.5) and without; iteration_ms = the mean
            difference per iteration between k = 4 and k = 1 (strides 2, 4, 8), and that per owned texel.  The yardstick, in the same process: denoiseFrame's
            kernels for k = 1 .. 4 iterations on a size x size frame of the same scene, per valid pixel.  Both read the same three-record tap.
  wall      bake_texels + filter_texels(None) - the plane stays on the device - against bake_texels + filter_texels(the downloaded out), and the CPU twin once
            (which must agree with the device bit for bit).
  quality   VISIBILITY and IRRADIANCE bakes at `dirs` directions against a bake of the same texels at `ref-dirs` directions: RMSE(filtered) / RMSE(noisy) over
            the owned texels for the header's defaults, for sigma_c = 2 / sqrt(dirs), for one parameter changed at a time, and for iterations x sigma_d x
            sigma_c jointly.
One JSON line."""
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
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dirs", type=int, default=16)
    ap.add_argument("--ref-dirs", type=int, default=4096)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    if rt.device_count() < 1:
        raise SystemExit("bench_filter: no HIP device visible")

    S, dirs, dilate, bias = a.size, a.dirs, a.dilate, 1e-3
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    cells = rt.atlas_grid(hm.tris, 0.05)
    slots = hm.tris.copy()
    lo, hi = np.array(hm.view.bounds.min.e[:]), np.array(hm.view.bounds.max.e[:])
    max_dist = float(np.float32(0.15 * np.linalg.norm(hi - lo)))
    ks, keep = rt.make_kernel_scene(hm, mats)
    fb = rt.initRenderer(ks, rt.staircase_camera(S, S), S, S, 16, keepalive=keep)
    defaults = dict(iterations=rt.RT_FILTER_ITERATIONS, normal_squarings=rt.RT_FILTER_SQUARINGS, sigma_d=rt.RT_FILTER_SIGMA_D, sigma_z=rt.RT_FILTER_SIGMA_Z,
                    sigma_c=rt.RT_FILTER_SIGMA_C)
    res = dict(commit=a.commit, scene="procedural staircase, rtAtlasGrid", slots=len(slots), cells=cells, atlas=[S, S], dilate=dilate, dirs=dirs,
               ref_dirs=a.ref_dirs, runs=a.runs, fp="parity", defaults=defaults)
    med = statistics.median
    try:
        owned, ras = rt.raster_texels(S, S, dilate, want=("prim",))
        mask = ras["prim"] != rt.RT_GUIDE_PRIM_NONE
        res["owned"] = owned
        rng = np.random.default_rng(1)

        # ---- time: the filter's kernels by iteration count, per width and colour regime ----
        timing = {}
        for C, mode in ((1, rt.RT_GATHER_VISIBILITY), (3, rt.RT_GATHER_IRRADIANCE), (27, rt.RT_GATHER_SH9)):
            plane = rng.uniform(0.0, 1.0, (S, S, C)).astype(np.float32)
            out = np.empty_like(plane)
            for label, sc in (("colour", 0.5), ("no_colour", 0.0)):
                rt.filter_texels(S, S, mode, plane, dilate=dilate, iterations=4, sigma_c=sc, out=out)      # warm-up: buffers, code objects
                by_k = []
                for k in range(1, 5):
                    t = []
                    for _ in range(a.runs):
                        rt.filter_texels(S, S, mode, plane, dilate=dilate, iterations=k, sigma_c=sc, out=out)
                        t.append(rt.last_filter_ms())
                    by_k.append(brief(t))
                step = (by_k[3]["median"] - by_k[0]["median"]) / 3.0
                timing[f"C{C}_{label}"] = dict(kernel_ms_by_iterations=by_k, iteration_ms=round(step, 4), ns_per_owned_texel=round(step * 1e6 / owned, 4))
        res["filter"] = timing

        # ---- the yardstick: denoiseFrame's iteration on a frame of the same size, in the same process ----
        valid = int((rt.renderGuides(rt.RT_GUIDE_PRIM)["prim"] != rt.RT_GUIDE_PRIM_NONE).sum())
        rt.runRenderer(1)
        frame = np.empty((S, S, 3), np.float32)
        rt.denoiseFrame(out=frame)
        by_k = []
        for k in range(1, 5):
            t = []
            for _ in range(a.runs):
                rt.denoiseFrame(iterations=k, out=frame)
                t.append(rt.last_denoise_ms())
            by_k.append(brief(t))
        step = (by_k[3]["median"] - by_k[0]["median"]) / 3.0
        res["denoise"] = dict(valid=valid, kernel_ms_by_iterations=by_k, iteration_ms=round(step, 4), ns_per_valid_pixel=round(step * 1e6 / valid, 4))
        for k, v in timing.items():
            v["ratio_to_denoise_per_item"] = round(v["ns_per_owned_texel"] / res["denoise"]["ns_per_valid_pixel"], 3)

        # ---- wall: the plane stays on the device, or comes down and goes up again ----
        wall = {}
        for name, mode, md in (("visibility", rt.RT_GATHER_VISIBILITY, max_dist), ("irradiance", rt.RT_GATHER_IRRADIANCE, 0.0)):
            kw = dict(ns=1, bias=bias, max_dist=md, dilate=dilate, want=())
            rows = {"bake": [], "resident": [], "host_plane": []}
            for run in range(a.runs + 1):
                t0 = time.perf_counter()
                _, pl = rt.bake_texels(S, S, mode, dirs, **kw)
                t1 = time.perf_counter()
                _, here = rt.filter_texels(S, S, mode, None, dilate=dilate)
                t2 = time.perf_counter()
                _, pl2 = rt.bake_texels(S, S, mode, dirs, **kw)
                _, there = rt.filter_texels(S, S, mode, pl2["out"], dilate=dilate)
                t3 = time.perf_counter()
                assert np.array_equal(here.view(np.uint32), there.view(np.uint32)), f"{name}: in = NULL differs from the downloaded plane"
                if run > 0:
                    rows["bake"].append((t1 - t0) * 1e3)
                    rows["resident"].append((t2 - t0) * 1e3)
                    rows["host_plane"].append((t3 - t2) * 1e3)
            t0 = time.perf_counter()
            _, twin = rt.filter_texels_host(slots, S, S, mode, pl["out"], dilate=dilate)
            twin_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(twin.view(np.uint32), here.view(np.uint32)), f"{name}: the device differs from the CPU twin"
            wall[name] = dict({k + "_wall_ms": brief(v) for k, v in rows.items()}, cpu_twin_filter_wall_ms=round(twin_ms, 1), bit_equal_to_twin=True,
                              filter_resident_wall_ms=round(med(rows["resident"]) - med(rows["bake"]), 4),
                              filter_host_plane_wall_ms=round(med(rows["host_plane"]) - med(rows["bake"]), 4))
        res["wall"] = wall

        # ---- quality: a bake at `dirs` directions against one at `ref-dirs` ----
        quality = {}
        rmse = lambda x, ref: float(np.sqrt(np.mean((x[mask].astype(np.float64) - ref[mask].astype(np.float64)) ** 2)))
        grid = [("defaults", {}), ("sigma_c_2_over_sqrt_dirs", dict(sigma_c=2.0 / dirs ** 0.5))]
        grid += [(f"sigma_c_{v}", dict(sigma_c=v)) for v in (0.0, 0.05, 0.1, 0.25)]
        grid += [(f"iterations_{v}", dict(iterations=v)) for v in (2, 3, 5, 6)]
        grid += [(f"sigma_d_{v}", dict(sigma_d=v)) for v in (1.0, 1.5, 3.0, 4.0)]
        grid += [(f"sigma_z_{v}", dict(sigma_z=v)) for v in (1.0, 4.0)]
        grid += [(f"squarings_{v}", dict(normal_squarings=v)) for v in (2, 7)]
        for name, mode, md in (("visibility", rt.RT_GATHER_VISIBILITY, max_dist), ("irradiance", rt.RT_GATHER_IRRADIANCE, 0.0)):
            ref = rt.bake_texels(S, S, mode, a.ref_dirs, ns=1, bias=bias, max_dist=md, dilate=dilate, base_id=0x9e3779b9, want=())[1]["out"]
            noisy = rt.bake_texels(S, S, mode, dirs, ns=1, bias=bias, max_dist=md, dilate=dilate, want=())[1]["out"]
            base = rmse(noisy, ref)
            q = dict(rmse_noisy=round(base, 6), mean_ref=round(float(ref[mask].mean()), 6), ratio={})
            for label, kw in grid:
                got = rt.filter_texels(S, S, mode, None, dilate=dilate, **kw)[1]
                q["ratio"][label] = round(rmse(got, ref) / base, 4)
            # the colour scale follows the signal: sigma_c relative to the reference's mean
            for rel in (0.5, 1.0, 2.0, 4.0):
                got = rt.filter_texels(S, S, mode, None, dilate=dilate, sigma_c=rel * float(ref[mask].mean()))[1]
                q["ratio"][f"sigma_c_{rel}_x_mean"] = round(rmse(got, ref) / base, 4)
            # the three parameters that move the ratio, jointly
            q["joint"] = {}
            for it in (2, 3, 4):
                for sd in (1.0, 1.5, 2.0):
                    for sc in (0.25, 0.5, 1.0):
                        got = rt.filter_texels(S, S, mode, None, dilate=dilate, iterations=it, sigma_d=sd, sigma_c=sc)[1]
                        q["joint"][f"iterations_{it}_sigma_d_{sd}_sigma_c_{sc}"] = round(rmse(got, ref) / base, 4)
            quality[name] = q
        res["quality"] = quality
    finally:
        rt.cleanupRenderer()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
