"""The guide pass (renderGuides, all planes) against a one-sample frame (runRenderer(1)) on one GPU.

    python tools/bench_guides.py [--cases C2,C4] [--repeats 20] [--out profiles/guides.json] [--lib build/ab/<name>.so]

C2: random spheres 1200x800 (the bench frame).  C4: the staircase mesh 1920x1080.  After a warm-up the two calls alternate in one process; per case one
JSON line with the median and the best of --repeats: the guide kernel's HIP-event time (rtLastGuidesMs) and the call's wall time, the frame's kernel_ms
and total_ms (getRenderStats).  The yardstick is the one-sample frame: the guide pass traces one ray per pixel where that frame traces at least one plus
its bounces and shading.  --lib: another build of the library (tools/build_variant.sh) for an A/B of the same measurement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "C2": dict(kind="spheres", nx=1200, ny=800, depth=50),
    "C4": dict(kind="mesh", nx=1920, ny=1080, depth=64, detail=4),
}


def open_case(rt, w):
    if w["kind"] == "spheres":
        sp, mt, cam = rt.scene_random_spheres(w["nx"], w["ny"])
        rt.initRendererSpheres(sp, mt, cam, w["nx"], w["ny"], w["depth"])
        return None
    tris, mats = rt.scene_staircase_procedural(w["detail"])
    hm = rt.HostMesh.build(tris, 5)
    ks, keep = rt.make_kernel_scene(hm, mats)
    rt.initRenderer(ks, rt.staircase_camera(w["nx"], w["ny"]), w["nx"], w["ny"], w["depth"], keepalive=keep)
    return hm, keep


def run_case(rt, name, w, repeats):
    keep = open_case(rt, w)
    mask = rt.RT_GUIDE_ALBEDO | rt.RT_GUIDE_NORMAL | rt.RT_GUIDE_DEPTH | rt.RT_GUIDE_PRIM | (rt.RT_GUIDE_NODES if w["kind"] == "mesh" else 0)
    out = rt.renderGuides(mask)                      # the caller's arrays: reused by every call
    for _ in range(3):                               # warm-up: code objects, first touch of the buffers
        rt.runRenderer(1)
        rt.renderGuides(mask, out=out)
    g_kernel, g_wall, f_kernel, f_wall = [], [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        rt.renderGuides(mask, out=out)
        g_wall.append((time.perf_counter() - t0) * 1e3)
        g_kernel.append(rt.last_guides_ms())
        rt.runRenderer(1)
        st = rt.getRenderStats()
        f_kernel.append(st.kernel_ms)
        f_wall.append(st.total_ms)
    rt.cleanupRenderer()
    del keep
    med, r3 = statistics.median, lambda x: round(x, 4)
    return dict(case=name, kind=w["kind"], nx=w["nx"], ny=w["ny"], planes=mask, repeats=repeats,
                guides_kernel_ms=r3(med(g_kernel)), guides_kernel_ms_best=r3(min(g_kernel)), guides_wall_ms=r3(med(g_wall)), guides_wall_ms_best=r3(min(g_wall)),
                frame_1spp_kernel_ms=r3(med(f_kernel)), frame_1spp_kernel_ms_best=r3(min(f_kernel)), frame_1spp_total_ms=r3(med(f_wall)),
                frame_1spp_total_ms_best=r3(min(f_wall)), kernel_ratio=r3(med(g_kernel) / med(f_kernel)),
                hit_share=r3(float((out["prim"] != rt.RT_GUIDE_PRIM_NONE).mean())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="C2,C4")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    if args.lib:
        rt.RENDERER_LIB = os.path.abspath(args.lib)
    if rt.device_count() < 1:
        raise SystemExit("bench_guides: no HIP device visible")
    lines = []
    for name in args.cases.split(","):
        line = run_case(rt, name, CASES[name], args.repeats)
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
