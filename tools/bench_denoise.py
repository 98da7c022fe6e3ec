"""The preview denoiser (denoiseFrame, default parameters) against a one-sample frame (runRenderer(1)) on one GPU.

    python tools/bench_denoise.py [--cases C2,C4] [--repeats 20] [--out profiles/denoise.json] [--lib build/ab/<name>.so] [--no-quality]

C2: random spheres 1200x800 (the bench frame).  C4: the staircase mesh 1920x1080.  After a warm-up the denoise call alternates with runRenderer(1) in one
process; per case one JSON line with medians (and the best) of --repeats:
  * denoise_kernel_ms: the HIP-event time of the denoiser's kernels (rtLastDenoiseMs: prologue + 5 iterations, the epilogue fused into the last);
  * kernel_ms_by_iterations[k-1]: the same for a call of k = 1 .. 5 iterations, and iteration_ms[it] = their differences: the cost of the iteration of stride
    1 << it (iteration_ms[0] includes the prologue), with taps_per_ns = 24 taps x valid pixels / that time;
  * denoise_call_ms: the wall time of the whole call (upload of the frame, guide kernel, kernels, download);
  * frame_1spp_kernel_ms / total_ms: the yardstick, what one preview pass costs (getRenderStats);
  * rmse_ratio[spp] = RMSE(denoised, target) / RMSE(noisy, target) for runRenderer(spp), spp = 1, 4, 16, the target a 4096 spp render, with sigma_c = 1 and
    with sigma_c = 2 / sqrt(spp) (the noise scale followed by the caller).
--lib: another build of the library (tools/build_variant.sh) for an A/B of the same measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_guides import CASES, open_case  # noqa: E402


def rmse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def run_case(rt, name, w, repeats, quality):
    keep = open_case(rt, w)
    nx, ny = w["nx"], w["ny"]
    valid = int((rt.renderGuides(rt.RT_GUIDE_PRIM)["prim"] != rt.RT_GUIDE_PRIM_NONE).sum())
    fb = rt._state["fb"]
    out = np.empty((ny, nx, 3), np.float32)
    res = dict(case=name, kind=w["kind"], nx=nx, ny=ny, repeats=repeats, flags=rt.default_denoise_flags(), valid_share=round(valid / (nx * ny), 4))
    if quality:
        rt.runRenderer(4096)
        target = np.array(fb, copy=True)
        ratios = {}
        for spp in (1, 4, 16):
            rt.runRenderer(spp)
            noisy = np.array(fb, copy=True)
            base = rmse(noisy, target)
            ratios[str(spp)] = dict(rmse_noisy=round(base, 5),
                                    sigma_c_1=round(rmse(rt.denoiseFrame(noisy, out=out), target) / base, 4),
                                    sigma_c_2_over_sqrt_spp=round(rmse(rt.denoiseFrame(noisy, sigma_c=2.0 / spp ** 0.5, out=out), target) / base, 4))
        res["rmse_ratio"] = ratios
    for _ in range(3):                               # warm-up: code objects, first touch of the buffers
        rt.runRenderer(1)
        rt.denoiseFrame(out=out)
    d_kernel, d_wall, f_kernel, f_wall = [], [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        rt.denoiseFrame(out=out)
        d_wall.append((time.perf_counter() - t0) * 1e3)
        d_kernel.append(rt.last_denoise_ms())
        rt.runRenderer(1)
        st = rt.getRenderStats()
        f_kernel.append(st.kernel_ms)
        f_wall.append(st.total_ms)
    by_iterations = []
    for k in range(1, 6):
        t = []
        for _ in range(repeats):
            rt.denoiseFrame(iterations=k, out=out)
            t.append(rt.last_denoise_ms())
            rt.runRenderer(1)
        by_iterations.append(statistics.median(t))
    rt.cleanupRenderer()
    del keep
    med, r4 = statistics.median, lambda x: round(x, 4)
    steps = [by_iterations[0]] + [by_iterations[k] - by_iterations[k - 1] for k in range(1, 5)]
    res.update(denoise_kernel_ms=r4(med(d_kernel)), denoise_kernel_ms_best=r4(min(d_kernel)), denoise_call_ms=r4(med(d_wall)), denoise_call_ms_best=r4(min(d_wall)),
               frame_1spp_kernel_ms=r4(med(f_kernel)), frame_1spp_kernel_ms_best=r4(min(f_kernel)), frame_1spp_total_ms=r4(med(f_wall)),
               kernel_ratio=r4(med(d_kernel) / med(f_kernel)), kernel_ms_by_iterations=[r4(x) for x in by_iterations], iteration_ms=[r4(x) for x in steps],
               taps_per_ns=[r4(24.0 * valid / (x * 1e6)) if x > 0 else None for x in steps],
               compulsory_bytes_per_iteration=64 * nx * ny)     # each pixel's three 16-byte records read once, its colour record written once
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="C2,C4")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--no-quality", action="store_true")
    args = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    if args.lib:
        rt.RENDERER_LIB = os.path.abspath(args.lib)
    if rt.device_count() < 1:
        raise SystemExit("bench_denoise: no HIP device visible")
    lines = []
    for name in args.cases.split(","):
        line = run_case(rt, name, CASES[name], args.repeats, not args.no_quality)
        line["lib"] = os.path.relpath(rt.RENDERER_LIB, ROOT)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
