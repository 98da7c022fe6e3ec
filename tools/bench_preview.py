"""previewFrame (default parameters) beside the two calls it fuses, accumulateFrame and denoiseFrame, on one GPU, in one job and one process.

    python tools/bench_preview.py [--cases C2,C4] [--repeats 20] [--out profiles/preview.json] [--lib build/ab/<name>.so] [--no-quality]

C2: random spheres 1200x800 (the bench frame), cameras one degree of an orbit apart.  C4: the staircase mesh 1920x1080, cameras 0.05 sideways apart.  The camera
alternates between the two positions, so every timed call reprojects into a different previous frame.  After a warm-up, per repeat: setCamera, runRenderer(1),
previewFrame, accumulateFrame, denoiseFrame of its result; per case one JSON line with medians (and the best) of --repeats:
  * preview_call_ms / accumulate_call_ms / denoise_call_ms: the wall time of the whole call (upload of the frame, guide kernel, kernels, download);
    chain_call_ms = accumulate + denoise per repeat, call_ratio = preview / chain (the condition: below 1 on both scenes);
  * preview_kernel_ms / accumulate_kernel_ms / denoise_kernel_ms: the HIP-event times (rtLast*Ms), kernel_ratio = preview / (accumulate + denoise);
  * preview_first_kernel_ms / preview_first_call_ms: the call after rtResetPreview, where every pixel takes the 49-tap spatial variance;
  * temporal_share: the share of the valid pixels with N >= RT_PREVIEW_MIN_HISTORY in the last timed call;
  * C2 only, orbit: the 8 frames at 1 spp of tools/bench_accumulate.py, two degrees per frame, against runRenderer(1024):
    RMSE(result, target) / RMSE(last noisy frame, target) for previewFrame beside accumulate then denoise at its defaults and at sigma_c 0.5.
--lib: another build of the library for an A/B of the same measurement."""
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

from bench_accumulate import orbit_camera, rmse, shifted_camera  # noqa: E402
from bench_guides import CASES, open_case  # noqa: E402


def run_case(rt, name, w, repeats, quality):
    keep = open_case(rt, w)
    nx, ny = w["nx"], w["ny"]
    cams = [orbit_camera(rt, w, 0.0), orbit_camera(rt, w, 1.0)] if w["kind"] == "spheres" else [shifted_camera(rt, w, 0.0), shifted_camera(rt, w, 0.05)]
    valid = int((rt.renderGuides(rt.RT_GUIDE_PRIM)["prim"] != rt.RT_GUIDE_PRIM_NONE).sum())
    fb = rt._state["fb"]
    pre, acc, den = (np.empty((ny, nx, 3), np.float32) for _ in range(3))
    hist = np.empty((ny, nx), np.float32)
    res = dict(case=name, kind=w["kind"], nx=nx, ny=ny, repeats=repeats, flags=rt.default_denoise_flags(), valid_share=round(valid / (nx * ny), 4))
    if quality and w["kind"] == "spheres":
        frames, step = 8, 2.0
        rt.setCamera(orbit_camera(rt, w, 0.0))
        rt.runRenderer(1024)
        target = np.array(fb, copy=True)
        rt.reset_history()
        rt.reset_preview()
        for k in range(frames):
            rt.setCamera(orbit_camera(rt, w, -step * (frames - 1 - k)))
            rt.runRenderer(1)
            rt.accumulateFrame(out=acc)
            rt.previewFrame(out=pre, history=hist)
        noisy = np.array(fb, copy=True)
        base = rmse(noisy, target)
        res["orbit"] = dict(frames=frames, degrees_per_frame=step, target_spp=1024, rmse_noisy=round(base, 5),
                            preview=round(rmse(pre, target) / base, 4),
                            accumulate_then_denoise=round(rmse(rt.denoiseFrame(acc, out=den), target) / base, 4),
                            accumulate_then_denoise_sigma_c_0_5=round(rmse(rt.denoiseFrame(acc, sigma_c=0.5, out=den), target) / base, 4),
                            mean_history=round(float(hist[hist > 0].mean()), 3))
    rt.reset_history()
    rt.reset_preview()
    for k in range(4):                               # warm-up: code objects, first touch of the buffers
        rt.setCamera(cams[k & 1])
        rt.runRenderer(1)
        rt.previewFrame(out=pre)
        rt.accumulateFrame(out=acc)
        rt.denoiseFrame(acc, out=den)
    t = {k: [] for k in ("p_wall", "a_wall", "d_wall", "chain_wall", "p_kernel", "a_kernel", "d_kernel")}
    for k in range(repeats):
        rt.setCamera(cams[k & 1])
        rt.runRenderer(1)
        t0 = time.perf_counter()
        rt.previewFrame(out=pre, history=hist)
        t1 = time.perf_counter()
        rt.accumulateFrame(out=acc)
        t2 = time.perf_counter()
        rt.denoiseFrame(acc, out=den)
        t3 = time.perf_counter()
        t["p_wall"].append((t1 - t0) * 1e3); t["a_wall"].append((t2 - t1) * 1e3); t["d_wall"].append((t3 - t2) * 1e3); t["chain_wall"].append((t3 - t1) * 1e3)
        t["p_kernel"].append(rt.last_preview_ms()); t["a_kernel"].append(rt.last_accumulate_ms()); t["d_kernel"].append(rt.last_denoise_ms())
    temporal = int((hist >= rt.RT_PREVIEW_MIN_HISTORY).sum())
    first_kernel, first_wall = [], []
    for k in range(repeats):
        rt.reset_preview()
        t0 = time.perf_counter()
        rt.previewFrame(out=pre)
        first_wall.append((time.perf_counter() - t0) * 1e3)
        first_kernel.append(rt.last_preview_ms())
    rt.cleanupRenderer()
    del keep
    med, r4 = statistics.median, lambda x: round(x, 4)
    res.update(preview_call_ms=r4(med(t["p_wall"])), preview_call_ms_best=r4(min(t["p_wall"])),
               accumulate_call_ms=r4(med(t["a_wall"])), denoise_call_ms=r4(med(t["d_wall"])),
               chain_call_ms=r4(med(t["chain_wall"])), chain_call_ms_best=r4(min(t["chain_wall"])), call_ratio=r4(med(t["p_wall"]) / med(t["chain_wall"])),
               preview_kernel_ms=r4(med(t["p_kernel"])), preview_kernel_ms_best=r4(min(t["p_kernel"])),
               accumulate_kernel_ms=r4(med(t["a_kernel"])), denoise_kernel_ms=r4(med(t["d_kernel"])),
               kernel_ratio=r4(med(t["p_kernel"]) / (med(t["a_kernel"]) + med(t["d_kernel"]))),
               preview_first_kernel_ms=r4(med(first_kernel)), preview_first_call_ms=r4(med(first_wall)),
               temporal_share=r4(temporal / max(1, valid)),
               # per valid pixel: the temporal kernel's four taps of three 16-byte records and the 8-byte moments, the variance kernel's 49 taps of two records and
               # the moments where the history is short, an a-trous iteration's 24 taps of three records
               temporal_tap_bytes=4 * 56 * valid, variance_tap_bytes_first_call=49 * 40 * valid, atrous_tap_bytes_per_iteration=24 * 48 * valid)
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
        raise SystemExit("bench_preview: no HIP device visible")
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
