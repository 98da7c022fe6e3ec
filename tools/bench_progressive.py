"""Progressive rendering on one GPU: the frame of a bench.py workload rendered as passes of a fixed size (runRendererProgressive) against the same
samples in one runRenderer call.

    python tools/bench_progressive.py [--cases C2,C4] [--repeats 3] [--out-dir profiles]

C2: random spheres 1200x800, 100 spp in passes of 1, 4, 10, 25.  C4: the staircase mesh 1920x1080, 256 spp in passes of 16, 64.  One JSON line per
(case, pass size): the passes' getRenderStats total_ms / kernel_ms, their sums against the monolithic frame (best of --repeats each), and whether
the final framebuffer equals the monolithic one bit for bit.  With --out-dir the lines of a case are also written to <dir>/progressive_<case>.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "C2": dict(kind="spheres", nx=1200, ny=800, spp=100, depth=50, passes=(1, 4, 10, 25)),
    "C4": dict(kind="mesh", nx=1920, ny=1080, spp=256, depth=64, detail=4, passes=(16, 64)),
}


def open_case(rt, w):
    if w["kind"] == "spheres":
        sp, mt, cam = rt.scene_random_spheres(w["nx"], w["ny"])
        return rt.initRendererSpheres(sp, mt, cam, w["nx"], w["ny"], w["depth"]), None
    tris, mats = rt.scene_staircase_procedural(w["detail"])
    hm = rt.HostMesh.build(tris, 5)
    ks, keep = rt.make_kernel_scene(hm, mats)
    return rt.initRenderer(ks, rt.staircase_camera(w["nx"], w["ny"]), w["nx"], w["ny"], w["depth"], keepalive=keep), (hm, keep)


def run_case(rt, name, w, repeats):
    fb, keep = open_case(rt, w)
    rt.runRenderer(min(w["spp"], 8))                 # warm-up: code objects, first-touch of the buffers
    rt.runRendererProgressive(2)
    rt.resetProgressive()
    mono_ms, mono_kernel = [], []
    for _ in range(repeats):
        rt.runRenderer(w["spp"])
        st = rt.getRenderStats()
        mono_ms.append(st.total_ms)
        mono_kernel.append(st.kernel_ms)
    mono = np.array(fb, copy=True)
    lines = []
    for size in w["passes"]:
        best = None
        for _ in range(repeats):
            rt.resetProgressive()
            total, kern = [], []
            for _ in range(w["spp"] // size):
                rt.runRendererProgressive(size)
                st = rt.getRenderStats()
                total.append(st.total_ms)
                kern.append(st.kernel_ms)
            if best is None or sum(total) < sum(best[0]):
                best = (total, kern)
        equal = bool(np.array_equal(np.array(fb, copy=False).view(np.uint32), mono.view(np.uint32)))
        total, kern = best
        line = dict(case=name, nx=w["nx"], ny=w["ny"], spp=w["spp"], pass_spp=size, passes=len(total),
                    pass_total_ms=[round(x, 3) for x in total], pass_kernel_ms=[round(x, 3) for x in kern],
                    sum_total_ms=round(sum(total), 3), sum_kernel_ms=round(sum(kern), 3),
                    mono_total_ms=round(min(mono_ms), 3), mono_kernel_ms=round(min(mono_kernel), 3),
                    ratio_total=round(sum(total) / min(mono_ms), 3), ratio_kernel=round(sum(kern) / min(mono_kernel), 3),
                    bit_equal_to_monolithic=equal, repeats=repeats)
        print(json.dumps(line), flush=True)
        lines.append(line)
    rt.cleanupRenderer()
    del keep
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="C2,C4")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    if rt.device_count() < 1:
        raise SystemExit("bench_progressive: no HIP device visible")
    for name in args.cases.split(","):
        lines = run_case(rt, name, CASES[name], args.repeats)
        if args.out_dir:
            os.makedirs(args.out_dir, exist_ok=True)
            with open(os.path.join(args.out_dir, "progressive_%s.json" % name), "w") as f:
                json.dump(lines, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
