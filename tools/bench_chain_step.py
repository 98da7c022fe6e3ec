#!/usr/bin/env python3
"""tools/bench_chain_step.py [--lib PATH] [--frames 6] [--spp 400] — a yardstick for the chain step itself: small frames of the benchmark
scene whose time is nothing but the single-ray step of the folded sphere kinds.

The view is chosen here, on the CPU with the oracle, before the GPU part: the camera looks along the ground at the line where a small sphere rests on it,
so close that the whole frame is the wedge between the two, and a candidate view is taken when every pixel of the 16x8 frame traces at least 24 rays per
sample (the threshold of chain list 0) over the samples the frame renders.  The oracle's ray counts of that frame, per pixel, are the divisor.

Two frames are timed, each `frames` times after a first frame that records the cost map (the later ones are ordered by it and must report the folded
form, one launch of phase 2):
  frame   16x8 pixels, `spp` samples, depth 50.  Reported as kernel ms / rays of the longest pixel.  The frame is one workgroup (a frame never has more
          lanes than pixels) with three chain waves, so its pixels are traced a few at a time and this figure is an upper bound of the step, not the step.
  pixel   the same view as ONE pixel.  Its wave has one live lane from the first ray to the last and the GPU is otherwise idle: kernel ms / rays of the
          pixel is the isolated step.
Beside them: the step implied by the benchmark frame, --c2-ms / --c2-rays (the longest pixel of C2 and the fastest cost-ordered dispatch recorded in
DESIGN.md 3.26), and the difference - what the neighbours on the CU cost."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NX, NY, DEPTH, LIST0 = 16, 8, 50, 24
FOLDED = 1


def candidate_views(sp, mt, rt):
    """Cameras low above the ground, outside every sphere, that look at the point of the ground below a small diffuse sphere from 0.6 units away, under
    ever narrower angles."""
    small = [k for k in range(1, len(sp)) if sp["radius"][k] < 0.5 and mt["type"][k] == rt.RT_DIFFUSE]
    centres, radii = sp["center"].astype(np.float64), sp["radius"].astype(np.float64)
    g0, r0 = centres[0], radii[0]                                              # the ground sphere
    small.sort(key=lambda k: np.hypot(centres[k][0] - g0[0], centres[k][2] - g0[2]))      # nearest the top of the ground first: every sphere's centre is at
                                                                               # y = its radius, so only there does a sphere rest ON the ground
    for vfov in (0.5, 0.25, 0.125):
        for k in small[:12]:
            u = (centres[k] - g0) / np.linalg.norm(centres[k] - g0)
            foot = g0 + r0 * u                                                 # the ground under the sphere's centre
            for ang in (0.0, 2.1, 4.2):
                d = np.array([np.cos(ang), 0.0, np.sin(ang)])
                eye = foot + 0.6 * d
                eye[1] = g0[1] + np.sqrt(r0 * r0 - (eye[0] - g0[0]) ** 2 - (eye[2] - g0[2]) ** 2) + 0.02       # 0.02 above the ground where it stands
                if (np.linalg.norm(centres - eye, axis=1) <= radii + 1e-3).any():
                    continue
                yield dict(sphere=int(k), vfov=vfov, lookfrom=tuple(float(x) for x in eye), lookat=tuple(float(x) for x in foot))


def camera_of(rt, view, nx, ny):
    return rt.make_camera(view["lookfrom"], view["lookat"], (0, 1, 0), view["vfov"], nx / ny, 0.0, 0.6)


def oracle_rays(O, sp, mt, cam, nx, ny, ns):
    sc, opt = O.sphere_scene(sp, mt), O.default_options(True)
    return np.array([O.render(sc, cam, opt, nx, ny, ns, DEPTH, region=(x, y, x + 1, y + 1), counters=True)[1].rays for y in range(ny) for x in range(nx)], dtype=np.int64)


def choose_view(rt, O, sp, mt, spp):
    for view in candidate_views(sp, mt, rt):
        cam = camera_of(rt, view, NX, NY)
        if oracle_rays(O, sp, mt, cam, NX, NY, 4).mean() < 1.25 * LIST0 * 4:   # a cheap look first (four samples of one pixel say little: the frame's mean)
            continue
        rays = oracle_rays(O, sp, mt, cam, NX, NY, spp)
        if rays.min() >= LIST0 * spp and rays.max() < DEPTH * spp:              # (all of them at the depth limit: a camera shut in, not a wedge)
            return view, rays
    raise SystemExit("bench_chain_step: no candidate view puts every pixel at or above 24 rays per sample")


def timed(rt, sp, mt, cam, nx, ny, spp, frames):
    rt.initRendererSpheres(sp, mt, cam, nx, ny, DEPTH)
    rt.runRenderer(spp)                                                         # measures, and records the cost map
    ms, launch = [], None
    for _ in range(frames):
        rt.runRenderer(spp)
        recs = rt.last_launches()
        assert rt.last_sphere_form() == FOLDED and [r["phase"] for r in recs] == [2], (rt.last_sphere_form(), recs)
        ms.append(rt.getRenderStats().kernel_ms)
        launch = recs[-1]
    rt.cleanupRenderer()
    return ms, launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="a build of librt_mi355x.so to time instead of the tree's")
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--spp", type=int, default=400)
    ap.add_argument("--c2-ms", type=float, default=9.18)
    ap.add_argument("--c2-rays", type=int, default=3728)
    ap.add_argument("--cpu-only", action="store_true", help="choose the view and count the rays, then stop")
    ap.add_argument("--cpu-json", default=None, help="the output of an earlier --cpu-only run: its view and ray counts are taken instead of computed again")
    a = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    from oracle import oracle as O
    if a.lib:
        rt.RENDERER_LIB = os.path.abspath(a.lib)
    sp, mt, _ = rt.scene_random_spheres(NX, NY)
    if a.cpu_json:
        out = json.load(open(a.cpu_json))
        assert out["spp"] == a.spp, (out["spp"], a.spp)
        out["lib"] = a.lib or "tree"
    else:
        view, rays = choose_view(rt, O, sp, mt, a.spp)
        one = int(oracle_rays(O, sp, mt, camera_of(rt, view, 1, 1), 1, 1, a.spp)[0])
        out = dict(view=view, spp=a.spp, frame_rays_per_sample=dict(min=float(rays.min()) / a.spp, max=float(rays.max()) / a.spp), frame_longest_rays=int(rays.max()),
                   pixel_rays=one, lib=a.lib or "tree")
    view, longest, one = out["view"], out["frame_longest_rays"], out["pixel_rays"]
    if not a.cpu_only:
        f_ms, f_launch = timed(rt, sp, mt, camera_of(rt, view, NX, NY), NX, NY, a.spp, a.frames)
        p_ms, p_launch = timed(rt, sp, mt, camera_of(rt, view, 1, 1), 1, 1, a.spp, a.frames)
        implied = a.c2_ms * 1e3 / a.c2_rays
        out.update(frame_kernel_ms=f_ms, frame_us_per_ray_of_longest=min(f_ms) * 1e3 / longest, frame_launch=f_launch,
                   pixel_kernel_ms=p_ms, isolated_us_per_ray=min(p_ms) * 1e3 / one, pixel_launch=p_launch,
                   c2_implied_us_per_ray=implied, neighbours_us_per_ray=implied - min(p_ms) * 1e3 / one)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
