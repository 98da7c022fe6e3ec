"""The temporal accumulation (accumulateFrame, default parameters) beside one denoiser iteration and a one-sample frame (runRenderer(1)) on one GPU.

    python tools/bench_accumulate.py [--cases C2,C4] [--repeats 20] [--out profiles/accumulate.json] [--lib build/ab/<name>.so] [--no-quality]

C2: random spheres 1200x800 (the bench frame).  C4: the staircase mesh 1920x1080.  The camera alternates between two positions (C2: one degree of an orbit
about the look-at point apart, C4: 0.05 sideways), so every timed call reprojects into a different previous frame.  After a warm-up, per repeat: setCamera,
runRenderer(1), accumulateFrame, denoiseFrame(iterations=1), denoiseFrame() in one process; per case one JSON line with medians (and the best) of --repeats:
  * accumulate_kernel_ms: the HIP-event time of the kernel (rtLastAccumulateMs); accumulate_first_kernel_ms: the same for a call without history;
  * accumulate_call_ms: the wall time of the whole call (upload of the frame, guide kernel, kernel, download of out);
  * denoise_1_kernel_ms / denoise_5_kernel_ms: rtLastDenoiseMs of denoiseFrame(iterations=1) and of the default five iterations, same job;
  * frame_1spp_kernel_ms / total_ms: what one preview pass costs (getRenderStats);
  * blended_share, mean_history: the share of the valid pixels that found a history in the last call and their mean N;
  * C2 only, orbit: 8 frames at 1 spp, two degrees per frame, ending at the scene's own camera, against runRenderer(1024) there:
    RMSE(result, target) / RMSE(last noisy frame, target) for accumulate, for denoise alone, and for accumulate then denoise (sigma_c 0.5 and the default).
--lib: another build of the library for an A/B of the same measurement."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_guides import CASES, open_case  # noqa: E402


def rmse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def orbit_camera(rt, w, degrees):
    """The camera of scene_random_spheres turned about the vertical axis through its look-at point."""
    a = math.radians(degrees)
    x, y, z = 13.0, 2.0, 3.0
    return rt.make_camera((math.cos(a) * x + math.sin(a) * z, y, -math.sin(a) * x + math.cos(a) * z), (0, 0, 0), (0, 1, 0), 30.0, w["nx"] / w["ny"], 0.1, 10.0)


def shifted_camera(rt, w, amount):
    """The staircase camera moved sideways (along its u) with its whole lens."""
    cam = rt.staircase_camera(w["nx"], w["ny"])
    for a in range(3):
        cam.origin.e[a] += amount * cam.u.e[a]
        cam.lower_left_corner.e[a] += amount * cam.u.e[a]
    return cam


def run_case(rt, name, w, repeats, quality):
    keep = open_case(rt, w)
    nx, ny = w["nx"], w["ny"]
    cams = [orbit_camera(rt, w, 0.0), orbit_camera(rt, w, 1.0)] if w["kind"] == "spheres" else [shifted_camera(rt, w, 0.0), shifted_camera(rt, w, 0.05)]
    valid = int((rt.renderGuides(rt.RT_GUIDE_PRIM)["prim"] != rt.RT_GUIDE_PRIM_NONE).sum())
    fb = rt._state["fb"]
    out, den, hist = np.empty((ny, nx, 3), np.float32), np.empty((ny, nx, 3), np.float32), np.empty((ny, nx), np.float32)
    res = dict(case=name, kind=w["kind"], nx=nx, ny=ny, repeats=repeats, flags=rt.default_denoise_flags(), valid_share=round(valid / (nx * ny), 4))
    if quality and w["kind"] == "spheres":
        frames, step = 8, 2.0
        rt.setCamera(orbit_camera(rt, w, 0.0))
        rt.runRenderer(1024)
        target = np.array(fb, copy=True)
        rt.reset_history()
        for k in range(frames):
            rt.setCamera(orbit_camera(rt, w, -step * (frames - 1 - k)))
            rt.runRenderer(1)
            rt.accumulateFrame(out=out, history=hist)
        noisy = np.array(fb, copy=True)
        base = rmse(noisy, target)
        res["orbit"] = dict(frames=frames, degrees_per_frame=step, target_spp=1024, rmse_noisy=round(base, 5),
                            accumulate=round(rmse(out, target) / base, 4),
                            denoise=round(rmse(rt.denoiseFrame(noisy, out=den), target) / base, 4),
                            denoise_sigma_c_2=round(rmse(rt.denoiseFrame(noisy, sigma_c=2.0, out=den), target) / base, 4),
                            accumulate_then_denoise_sigma_c_0_5=round(rmse(rt.denoiseFrame(out, sigma_c=0.5, out=den), target) / base, 4),
                            accumulate_then_denoise=round(rmse(rt.denoiseFrame(out, out=den), target) / base, 4),
                            mean_history=round(float(hist[hist > 0].mean()), 3))
    rt.reset_history()
    for k in range(4):                               # warm-up: code objects, first touch of the buffers
        rt.setCamera(cams[k & 1])
        rt.runRenderer(1)
        rt.accumulateFrame(out=out)
        rt.denoiseFrame(out=den)
    a_kernel, a_wall, d1_kernel, d5_kernel, f_kernel, f_wall = [], [], [], [], [], []
    for k in range(repeats):
        rt.setCamera(cams[k & 1])
        rt.runRenderer(1)
        st = rt.getRenderStats()
        f_kernel.append(st.kernel_ms)
        f_wall.append(st.total_ms)
        t0 = time.perf_counter()
        rt.accumulateFrame(out=out, history=hist)
        a_wall.append((time.perf_counter() - t0) * 1e3)
        a_kernel.append(rt.last_accumulate_ms())
        rt.denoiseFrame(out, iterations=1, out=den)
        d1_kernel.append(rt.last_denoise_ms())
        rt.denoiseFrame(out, out=den)
        d5_kernel.append(rt.last_denoise_ms())
    blended = int((hist > 1).sum())
    mean_history = float(hist[hist > 0].mean())
    first = []
    for k in range(repeats):
        rt.reset_history()
        rt.accumulateFrame(out=out)
        first.append(rt.last_accumulate_ms())
    rt.cleanupRenderer()
    del keep
    med, r4 = statistics.median, lambda x: round(x, 4)
    res.update(accumulate_kernel_ms=r4(med(a_kernel)), accumulate_kernel_ms_best=r4(min(a_kernel)), accumulate_first_kernel_ms=r4(med(first)),
               accumulate_call_ms=r4(med(a_wall)), accumulate_call_ms_best=r4(min(a_wall)),
               denoise_1_kernel_ms=r4(med(d1_kernel)), denoise_5_kernel_ms=r4(med(d5_kernel)),
               frame_1spp_kernel_ms=r4(med(f_kernel)), frame_1spp_total_ms=r4(med(f_wall)),
               ratio_to_denoise_1=r4(med(a_kernel) / med(d1_kernel)), ratio_to_frame=r4(med(a_kernel) / med(f_kernel)),
               blended_share=r4(blended / max(1, valid)), mean_history=r4(mean_history),
               # per pixel: guides 32 + in 12 read, three records + out + N written (64), and per valid pixel four taps of three 16-byte records
               compulsory_bytes=(32 + 12 + 48 + 12 + 4) * nx * ny + 48 * valid, tap_bytes_requested=4 * 48 * valid)
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
        raise SystemExit("bench_accumulate: no HIP device visible")
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
