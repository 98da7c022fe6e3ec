"""renderLightmap on one GPU against the route a caller had before it - recorded, nothing here is gated but the bits.

    timeout -k 10 600 python tools/bench_lightmap.py [--nx 1920 --ny 1080] [--detail 4] [--size 1024] [--runs 7] [--commit HASH] [--out profiles/lightmap.json]

The benchmark's procedural staircase (detail 4) with the atlas of rtAtlasGrid (margin 0.05), an nx x ny image, a size x size atlas of seeded values, PARITY.
In one process, after a warm-up, `runs` times each - median, min, max:
  frame     render_lightmap with RT_LIGHTMAP_ALBEDO for the three modes and both filters, planes uploaded per call: rtLastLightmapMs (generator + trace +
            shade) and the call's wall time; and once per mode with the planes read where a bake left them (RT_TEXELS_FROM_BAKE, a 1-direction bake).
  hand      the route by hand, in the same process: renderGuides(ALBEDO) + rtCentreRays + traceRays(PRIM, UV, NORMAL) + sampleTexels with the planes uploaded
            + the composition in numpy - wall time, and the kernel times of its three device calls.  It must agree with the frame bit for bit; the tool
            asserts it in every round.
  shade     not timed alone (the three kernels of a frame share one event pair), so bracketed: generator_plus_shade_ms = the frame's kernel time minus
            rtLastRaysMs of the same rays traced by traceRays; rtLastSampleMs is the lookup alone over the same hits; rtLastGuidesMs, beside them, is the
            guide kernel of the same frame (one traversal and the albedo).
  scale     runRenderer at 1 spp: the kernel time of one path-traced sample per pixel.
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
    ap.add_argument("--nx", type=int, default=1920)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--detail", type=int, default=4)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    if rt.device_count() < 1:
        raise SystemExit("bench_lightmap: no HIP device visible")

    nx, ny, S = a.nx, a.ny, a.size
    tris, mats = rt.scene_staircase_procedural(a.detail)
    hm = rt.HostMesh.build(tris, 5)
    cells = rt.atlas_grid(hm.tris, 0.05)
    cam = rt.staircase_camera(nx, ny)
    ks, keep = rt.make_kernel_scene(hm, mats)
    rt.initRenderer(ks, cam, nx, ny, 64, keepalive=keep)
    res = dict(commit=a.commit, scene=f"procedural staircase detail {a.detail}, rtAtlasGrid", slots=len(hm.tris), cells=cells, image=[nx, ny], atlas=[S, S],
               runs=a.runs, fp="parity", frame={}, hand={}, resident={})
    ij = np.stack(np.meshgrid(np.arange(nx), np.arange(ny)), axis=-1).reshape(-1, 2).astype(np.int32)
    rng = np.random.default_rng(1)
    A = rt.RT_LIGHTMAP_ALBEDO
    try:
        for name, mode in (("visibility", rt.RT_GATHER_VISIBILITY), ("irradiance", rt.RT_GATHER_IRRADIANCE), ("sh9", rt.RT_GATHER_SH9)):
            planes = rng.uniform(0.0, 1.0, (S, S, rt.gather_width(mode))).astype(np.float32)
            out = np.empty((ny, nx, 3), np.float32)
            for label, flt in (("nearest", 0), ("bilinear", rt.RT_SAMPLE_BILINEAR)):
                rt.render_lightmap(S, S, mode, planes, A | flt, out=out)                            # warm-up: buffers, code objects
                kernel, wall, hand_wall, hand_k = [], [], [], dict(guides=[], rays=[], sample=[])
                for _ in range(a.runs):
                    t0 = time.perf_counter()
                    rt.render_lightmap(S, S, mode, planes, A | flt, out=out)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    kernel.append(rt.last_lightmap_ms())
                    t0 = time.perf_counter()
                    albedo = rt.renderGuides(rt.RT_GUIDE_ALBEDO)["albedo"].reshape(-1, 3)
                    org, d = rt.centre_rays(cam, nx, ny, ij)
                    h = rt.trace_rays(org, d, mask=rt.RT_RAY_PRIM | rt.RT_RAY_UV | rt.RT_RAY_NORMAL)
                    _, e, _ = rt.sample_texels(h["prim"], h["uv"], h["normal"], S, S, mode, planes, flt)
                    p = h["prim"][:, None]
                    lit = np.where(p == rt.RT_GUIDE_PRIM_FLOOR, np.float32(1), e)
                    by_hand = np.where(p == rt.RT_GUIDE_PRIM_NONE, albedo, albedo * lit).astype(np.float32).reshape(ny, nx, 3)
                    hand_wall.append((time.perf_counter() - t0) * 1e3)
                    hand_k["guides"].append(rt.last_guides_ms()); hand_k["rays"].append(rt.last_rays_ms()); hand_k["sample"].append(rt.last_sample_ms())
                    assert np.array_equal(by_hand.view(np.uint32), out.view(np.uint32)), f"{name} {label}: the frame differs from the route by hand"
                res["frame"][f"{name}_{label}"] = dict(kernel_ms=brief(kernel), wall_ms=brief(wall))
                res["frame"][f"{name}_{label}"]["generator_plus_shade_ms"] = round(statistics.median(kernel) - statistics.median(hand_k["rays"]), 4)
                res["hand"][f"{name}_{label}"] = dict(wall_ms=brief(hand_wall), bit_equal_to_frame=True,
                                                      **{k + "_kernel_ms": brief(v) for k, v in hand_k.items()})
            # the planes read where a bake left them: no upload
            rt.bake_texels(S, S, mode, 1, ns=1, bias=1e-3, max_dist=1.0, want=())
            rt.render_lightmap(S, S, mode, None, A | rt.RT_SAMPLE_BILINEAR | rt.RT_TEXELS_FROM_BAKE, out=out)
            kernel, wall = [], []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                rt.render_lightmap(S, S, mode, None, A | rt.RT_SAMPLE_BILINEAR | rt.RT_TEXELS_FROM_BAKE, out=out)
                wall.append((time.perf_counter() - t0) * 1e3)
                kernel.append(rt.last_lightmap_ms())
            res["resident"][f"{name}_bilinear"] = dict(kernel_ms=brief(kernel), wall_ms=brief(wall))
        hits = int((h["prim"] >= 0).sum())
        res["pixels"] = dict(all=nx * ny, triangle_hits=hits)
        t = []
        for _ in range(a.runs + 1):
            rt.runRenderer(1)
            t.append(rt.getRenderStats().kernel_ms)
        res["run_renderer_1spp_kernel_ms"] = brief(t[1:])
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
