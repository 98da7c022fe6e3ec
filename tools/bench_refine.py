"""refineFrame on one GPU: an adaptive frame to completion against the uniform frame and against the host loop it replaces - recorded, nothing here is gated.

    python tools/bench_refine.py [--cases C2,C4] [--batch 4] [--min-batches 2] [--max-samples 64] [--threshold 0.1] [--flags 1] [--out profiles/refine.json]

C2: random spheres 1200x800 (the bench frame).  C4: the staircase mesh 1920x1080.  Per case one JSON line; kernel times are HIP events (rtLastRefineMs:
select + pixel kernel + update; getRenderStats().kernel_ms; rtLastPixelsMs), wall times are taken around the Python call, one run each after one warm-up
frame of the same kind:
  passes        per pass of the adaptive frame: pixels sampled, kernel ms, wall ms (no plane downloaded)
  refine        their sums, the samples traced (rtRefineSamples), the wall time of one delivering call at the end and that call's kernel ms: it samples
                nothing, so it times the select alone (select_only_ms; a pass's pixel kernel + update is its kernel ms less this)
  progressive   runRendererProgressive(max_samples) of the same frame: every pixel gets the cap
  host_loop     the same lists (rtRefineLastList of every pass) through renderPixels from the host, state gathered and scattered with numpy as the loop of
                INTEGRATION.md 2 does: wall ms per pass and in all, the pixel kernels' share of it, and whether its means equal refineFrame's
  ascending     the adaptive frame again under RT_REFINE_ORDER=0 - the list in ascending pixel order instead of dearest first: kernel ms per pass and in
                all, its select alone (one workgroup walks the image: slower than the cost-ordered select), and whether its planes equal the cost-ordered
                frame's"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pixels import CASES, open_case


def adaptive_frame(rt, params, flags, keep_lists):
    """The frame to completion after a reset: (passes, lists, final planes, wall ms of the delivering call, kernel ms of that call: it returns 0, so
    what it times is the select alone)."""
    rt.reset_refine()
    passes, lists = [], []
    while True:
        t0 = time.perf_counter()
        sampled = rt.refine_frame(*params, flags, want=())[0]
        wall = (time.perf_counter() - t0) * 1e3
        if sampled == 0:
            break
        passes.append(dict(sampled=sampled, kernel_ms=round(rt.last_refine_ms(), 4), wall_ms=round(wall, 4)))
        if keep_lists:
            lists.append(rt.refine_last_list())
    t0 = time.perf_counter()
    final = rt.refine_frame(*params, flags)
    return passes, lists, final, (time.perf_counter() - t0) * 1e3, rt.last_refine_ms()


def host_loop(rt, lists, nx, ny, batch):
    """The lists through renderPixels: per-pixel state on the host, gathered before and scattered after every call."""
    state = np.zeros((ny * nx, 4), np.uint32)
    count = np.zeros(ny * nx, np.int32)
    walls, kernel = [], 0.0
    for ij in lists:
        t0 = time.perf_counter()
        ids = ij[:, 1].astype(np.int64) * nx + ij[:, 0]
        first = count[ids]
        fresh = not first.any()
        _, st, _ = rt.render_pixels(ij, batch, first=None if fresh else first, state=None if fresh else state[ids])
        state[ids] = st
        count[ids] = first + batch
        walls.append((time.perf_counter() - t0) * 1e3)
        kernel += rt.last_pixels_ms()
    mean = (state[:, :3].view(np.float32) / count[:, None].astype(np.float32)).reshape(ny, nx, 3)
    return walls, kernel, mean


def run_case(rt, name, w, params, flags):
    fb, keep = open_case(rt, w)
    nx, ny = w["nx"], w["ny"]
    r4 = lambda x: round(float(x), 4)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    batch, min_batches, max_samples, threshold = params
    line = dict(case=name, kind=w["kind"], nx=nx, ny=ny, batch=batch, min_batches=min_batches, max_samples=max_samples, threshold=threshold, flags=flags)

    adaptive_frame(rt, params, flags, False)                                        # warm-up: allocations, code objects
    passes, lists, final, deliver_wall, select_ms = adaptive_frame(rt, params, flags, True)
    samples = int(rt.refine_samples())
    line["passes"] = passes
    line["refine"] = dict(passes=len(passes), samples=samples, mean_samples_per_pixel=r4(samples / (nx * ny)), kernel_ms=r4(sum(p["kernel_ms"] for p in passes)),
                          wall_ms=r4(sum(p["wall_ms"] for p in passes)), deliver_wall_ms=r4(deliver_wall), select_only_ms=r4(select_ms),
                          samples_histogram={str(int(k)): int(v) for k, v in zip(*np.unique(final[2], return_counts=True))})

    for _ in range(2):                                                              # (the second frame is the warm one)
        rt.resetProgressive()
        t0 = time.perf_counter()
        rt.runRendererProgressive(max_samples, 8, 8)
        prog_wall = (time.perf_counter() - t0) * 1e3
    line["progressive"] = dict(samples=nx * ny * max_samples, kernel_ms=r4(rt.getRenderStats().kernel_ms), wall_ms=r4(prog_wall))

    host_loop(rt, lists[:2], nx, ny, batch)                                         # warm-up: renderPixels' buffers
    walls, kernel, mean = host_loop(rt, lists, nx, ny, batch)
    line["host_loop"] = dict(wall_ms_per_pass=[r4(x) for x in walls], wall_ms=r4(sum(walls)), pixel_kernel_ms=r4(kernel),
                             equals_refine=bool(np.array_equal(bits(mean), bits(final[1]))))
    del lists

    os.environ["RT_REFINE_ORDER"] = "0"                                             # (the switches are read once per call)
    try:
        asc_passes, _, asc_final, _, asc_select_ms = adaptive_frame(rt, params, flags, False)
    finally:
        del os.environ["RT_REFINE_ORDER"]
    line["ascending"] = dict(kernel_ms_per_pass=[p["kernel_ms"] for p in asc_passes], kernel_ms=r4(sum(p["kernel_ms"] for p in asc_passes)), select_only_ms=r4(asc_select_ms),
                             equals_cost_order=bool(all(np.array_equal(bits(a), bits(b)) for a, b in zip(asc_final[1:], final[1:]))))
    rt.cleanupRenderer()
    del keep
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="C2,C4")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--min-batches", type=int, default=2)
    ap.add_argument("--max-samples", type=int, default=64)
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--flags", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine.json"))
    args = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    lines = []
    for name in args.cases.split(","):
        line = run_case(rt, name, CASES[name], (args.batch, args.min_batches, args.max_samples, args.threshold), args.flags)
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
