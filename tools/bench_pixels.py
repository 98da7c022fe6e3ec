"""renderPixels on one GPU against the frame it is defined by: what a list of pixels costs, recorded - nothing here is gated.

    python tools/bench_pixels.py [--cases C2,C4] [--spp 16] [--repeats 7] [--out profiles/pixels.json]

C2: random spheres 1200x800 (the bench frame).  C4: the staircase mesh 1920x1080.  Per case one JSON line, every figure the median of --repeats calls after
two warm-up calls, kernel times from rtLastPixelsMs / getRenderStats().kernel_ms (HIP events), wall times around the Python call:
  full      the list of every pixel (row-major) at --spp against runRenderer(--spp) of the same frame: full_ratio = frame kernel / list kernel (the lean
            queue kernels of the frame are not reused: well below 1); full_equals_frame: the two agree bit for bit (PARITY)
  sparse    a seeded 3 % random subset of the pixels at --spp: Msamples/s, and sparse_to_full = that rate / the full list's
  latency   wall and kernel ms of 1 pixel (the image centre) and of 1 k random pixels at --spp
  fast      under RT_FP_FAST: the share of channels of the full list that are bit-equal to the FAST frame, and its kernel times"""
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
    """Initialises the case; returns (framebuffer view, keepalive)."""
    if w["kind"] == "spheres":
        sp, mt, cam = rt.scene_random_spheres(w["nx"], w["ny"])
        return rt.initRendererSpheres(sp, mt, cam, w["nx"], w["ny"], w["depth"]), None
    tris, mats = rt.scene_staircase_procedural(w["detail"])
    hm = rt.HostMesh.build(tris, 5)
    ks, keep = rt.make_kernel_scene(hm, mats)
    return rt.initRenderer(ks, rt.staircase_camera(w["nx"], w["ny"]), w["nx"], w["ny"], w["depth"], keepalive=keep), (hm, keep)


def timed(call, kernel_ms, repeats, warm=2):
    """(median kernel ms, median wall ms) of `call` after `warm` warm-up calls; kernel_ms() reads the last call's HIP-event time."""
    for _ in range(warm):
        call()
    kernel, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(kernel_ms())
    return statistics.median(kernel), statistics.median(wall)


def run_case(rt, name, w, spp, repeats):
    fb, keep = open_case(rt, w)
    nx, ny = w["nx"], w["ny"]
    r4 = lambda x: round(float(x), 4)
    line = dict(case=name, kind=w["kind"], nx=nx, ny=ny, spp=spp, repeats=repeats)
    every = np.stack(np.meshgrid(np.arange(nx), np.arange(ny)), axis=-1).reshape(-1, 2).astype(np.int32)     # row-major: (i, j) of pixel j * nx + i
    rng = np.random.default_rng(1)
    pix = lambda: rt.last_pixels_ms()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

    fk, fw = timed(lambda: rt.runRenderer(spp, 8, 8), lambda: rt.getRenderStats().kernel_ms, repeats)
    frame = np.array(fb, copy=True)
    res = {}
    lk, lw = timed(lambda: res.update(out=rt.render_pixels(every, spp)[0]), pix, repeats)
    line.update(frame_kernel_ms=r4(fk), frame_wall_ms=r4(fw), full_kernel_ms=r4(lk), full_wall_ms=r4(lw), full_ratio=r4(fk / lk),
                full_msamples_s=r4(len(every) * spp / lk * 1e-3), frame_msamples_s=r4(len(every) * spp / fk * 1e-3),
                full_equals_frame=bool(np.array_equal(bits(res["out"]).reshape(-1), bits(frame).reshape(-1))))

    sub = every[rng.permutation(len(every))[: (len(every) * 3) // 100]]
    sk, sw = timed(lambda: rt.render_pixels(sub, spp), pix, repeats)
    line.update(sparse_pixels=len(sub), sparse_kernel_ms=r4(sk), sparse_wall_ms=r4(sw), sparse_msamples_s=r4(len(sub) * spp / sk * 1e-3),
                sparse_to_full=r4((len(sub) / sk) / (len(every) / lk)))

    line["latency"] = {}
    for n, ij in ((1, np.array([[nx // 2, ny // 2]], np.int32)), (1000, every[rng.permutation(len(every))[:1000]])):
        k, wl = timed(lambda: rt.render_pixels(ij, spp), pix, repeats)
        line["latency"][str(n)] = dict(kernel_ms=r4(k), wall_ms=r4(wl))

    rt.setRenderOptions(rt.getDefaultRenderOptions(w["kind"] == "spheres"), fp=rt.RT_FP_FAST)
    ffk, _ = timed(lambda: rt.runRenderer(spp, 8, 8), lambda: rt.getRenderStats().kernel_ms, repeats)
    fast_frame = np.array(fb, copy=True)
    flk, _ = timed(lambda: res.update(fast=rt.render_pixels(every, spp)[0]), pix, repeats)
    line.update(fast_frame_kernel_ms=r4(ffk), fast_full_kernel_ms=r4(flk), fast_full_ratio=r4(ffk / flk),
                fast_bit_equal_share=r4((bits(res["fast"]).reshape(-1) == bits(fast_frame).reshape(-1)).mean()))
    rt.cleanupRenderer()
    del keep
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="C2,C4")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixels.json"))
    args = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    lines = []
    for name in args.cases.split(","):
        line = run_case(rt, name, CASES[name], args.spp, args.repeats)
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
