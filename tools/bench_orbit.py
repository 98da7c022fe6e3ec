#!/usr/bin/env python3
"""tools/bench_orbit.py [--spp 16] [--repeat 3] — the moving-camera use of the cost map: one init of the benchmark scene at 1200x800, then
setCamera + runRenderer(spp) over a 24-step orbit in 2-degree steps, one 180-degree cut and 8 more steps, with RT_COST_REUSE=0 (no map: every frame measures),
1 (the default: setCamera drops the map, so every frame of the orbit measures - and records) and 2 (the map survives setCamera: a frame is ordered by the
frame before it), each in a fresh child process, `repeat` times alternating.  Prints per frame kernel_ms and wall
ms (rt_render_stats.total_ms: upload, kernels, delivery) of the last repeat, then for every child the mean over the orbit steps (the first frame of a
child, which always measures, and the cut frame left out) and the cut frame."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY, DEPTH = 1200, 800, 50
STEP_DEG, ORBIT, CUT_DEG, AFTER = 2.0, 24, 180.0, 8
MODES = ("0", "1", "2")


def angles():
    a, out = 0.0, [0.0]
    for _ in range(ORBIT):
        a += STEP_DEG
        out.append(a)
    a += CUT_DEG
    out.append(a)
    for _ in range(AFTER):
        a += STEP_DEG
        out.append(a)
    return out


def child(spp):
    sys.path.insert(0, ROOT)
    import cuda_raytracing_optimized_amd as rt
    sp, mt, cam = rt.scene_random_spheres(NX, NY)
    rt.initRendererSpheres(sp, mt, cam, NX, NY, DEPTH)
    rt.runRenderer(1)                                       # (first use of the device: kernel load, buffers)
    frames = []
    for deg in angles():
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        rt.setCamera(rt.make_camera((13 * c + 3 * s, 2, -13 * s + 3 * c), (0, 0, 0), (0, 1, 0), 30.0, NX / NY, 0.1, 10.0))
        rt.runRenderer(spp)
        st = rt.getRenderStats()
        frames.append(dict(deg=deg, kernel_ms=st.kernel_ms, wall_ms=st.total_ms, phases=[r["phase"] for r in rt.last_launches()]))
    rt.cleanupRenderer()
    print(json.dumps(frames))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.spp)
    runs = {"0": [], "1": [], "2": []}
    for _ in range(a.repeat):
        for reuse in MODES:
            env = dict(os.environ, RT_COST_REUSE=reuse)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--spp", str(a.spp)], env=env, capture_output=True, text=True, timeout=300, check=True)
            runs[reuse].append(json.loads(r.stdout.strip().splitlines()[-1]))
    cut = ORBIT + 1
    print(f"# 1200x800, {a.spp} spp, depth 50; frame 0 = the scene's camera, frames 1..{ORBIT} orbit by {STEP_DEG:g} deg, frame {cut} cuts by {CUT_DEG:g} deg, then {AFTER} more steps")
    print("# frame   deg | " + " | ".join(f"RT_COST_REUSE={m}: kernel_ms wall_ms phases" for m in MODES))
    for k in range(len(runs["0"][-1])):
        f = [runs[m][-1][k] for m in MODES]
        print(f"{k:7d} {f[0]['deg']:5.0f} | " + " | ".join(f"{x['kernel_ms']:8.3f} {x['wall_ms']:8.3f} {x['phases']}" for x in f))
    steps = [k for k in range(1, len(runs["0"][0])) if k != cut]
    med = lambda v: sorted(v)[len(v) // 2]
    means = {}
    for m in MODES:
        means[m] = [(sum(f[k]["kernel_ms"] for k in steps) / len(steps), sum(f[k]["wall_ms"] for k in steps) / len(steps), f[cut]["kernel_ms"]) for f in runs[m]]
        for n, (km, wm, c) in enumerate(means[m]):
            print(f"RT_COST_REUSE={m} run {n}: orbit steps mean kernel_ms {km:.4f} wall_ms {wm:.4f}; cut frame kernel_ms {c:.3f}")
    base = med([x[0] for x in means["0"]])
    for m in MODES:
        k, c = [x[0] for x in means[m]], [x[2] for x in means[m]]
        print(f"RT_COST_REUSE={m}: orbit steps kernel_ms median {med(k):.4f} (spread {max(k) - min(k):.4f}), {100.0 * (base / med(k) - 1.0):+.1f} % frames per second against 0; "
              f"cut frame median {med(c):.3f}")


if __name__ == "__main__":
    main()
