"""bakeTexels on one GPU against the route a caller had before it - recorded, nothing here is gated but the bits.

    python tools/bench_bake.py [--size 1024] [--dirs 16] [--dilate 2] [--runs 5] [--out profiles/bake.json]

The procedural staircase with the atlas of rtAtlasGrid (margin 0.05), a size x size atlas, PARITY.  Two cases: RT_GATHER_VISIBILITY at `dirs` directions
(bounded at 0.15 of the scene's diagonal: the room is closed), RT_GATHER_IRRADIANCE at `dirs` directions and one sample.  In one process, after one warm-up
round, `runs` times - median, min, max:
  bake       bakeTexels: rtLastTexelsMs (raster, resolve, dilation, compaction), rtLastBakeMs (generator + trace + reduce + scatter) and the call's wall time
  hand       the route without it: rtRasterTexelsHost (wall), gatherRadiance over the owned points alone (rtLastGatherMs and wall), the scatter through src
             in numpy (wall).  Its point index is the position in the owned list, not the texel: the same estimate from other ids, so it is timed, not compared.
  hand_full  the same with gatherRadiance over all size * size points (a filler at unowned texels), which is what gives the texel index as the point index:
             this one must agree with the bake bit for bit - out, acc and rays - and the tool asserts it in every round.
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
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dirs", type=int, default=16)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt

    S, dirs, dilate, bias = a.size, a.dirs, a.dilate, 1e-3
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    cells = rt.atlas_grid(hm.tris, 0.05)
    slots = hm.tris.copy()
    lo, hi = np.array(hm.view.bounds.min.e[:]), np.array(hm.view.bounds.max.e[:])
    max_dist = float(np.float32(0.15 * np.linalg.norm(hi - lo)))
    ks, keep = rt.make_kernel_scene(hm, mats)
    rt.initRenderer(ks, rt.staircase_camera(64, 64), 64, 64, 16, keepalive=keep)
    res = dict(scene="procedural staircase, rtAtlasGrid", slots=len(slots), cells=cells, atlas=[S, S], dilate=dilate, dirs=dirs, runs=a.runs, fp="parity", cases={})
    try:
        for name, mode, ns, md in (("visibility", rt.RT_GATHER_VISIBILITY, 1, max_dist), ("irradiance", rt.RT_GATHER_IRRADIANCE, 1, 0.0)):
            kw = dict(ns=ns, bias=bias, max_dist=md, rays=True)
            Wd = rt.gather_width(mode)

            def bake():
                t0 = time.perf_counter()
                owned, pl = rt.bake_texels(S, S, mode, dirs, dilate=dilate, **kw)
                return dict(wall=(time.perf_counter() - t0) * 1e3, texels=rt.last_texels_ms(), kernel=rt.last_bake_ms()), owned, pl

            def hand(full):
                t0 = time.perf_counter()
                owned, pl = rt.raster_texels_host(slots, S, S, dilate, want=("prim", "src", "pos", "nrm"))
                t1 = time.perf_counter()
                mask = (pl["prim"] != rt.RT_GUIDE_PRIM_NONE).ravel()
                pos, nrm = pl["pos"].reshape(-1, 3), pl["nrm"].reshape(-1, 3)
                if full:
                    nrm = nrm.copy()
                    nrm[~mask] = (0, 0, 1)
                else:
                    pos, nrm = pos[mask], nrm[mask]
                out, acc, rays = rt.gather_radiance(pos, nrm, mode, dirs, **kw)
                kernel = rt.last_gather_ms()
                t2 = time.perf_counter()
                o_pl, a_pl, r_pl = np.zeros((S * S, Wd), np.float32), np.zeros((S * S, Wd), np.float32), np.zeros(S * S, np.uint32)
                if full:
                    o_pl, a_pl[mask], r_pl[mask] = out, acc[mask], rays[mask]
                else:
                    o_pl[mask], a_pl[mask], r_pl[mask] = out, acc, rays
                src = pl["src"].ravel()
                o_pl = np.where((src != -1)[:, None], o_pl[np.where(src != -1, src, 0)], np.float32(0))
                t3 = time.perf_counter()
                return (dict(raster_wall=(t1 - t0) * 1e3, gather_wall=(t2 - t1) * 1e3, kernel=kernel, scatter_wall=(t3 - t2) * 1e3, wall=(t3 - t0) * 1e3),
                        owned, dict(out=o_pl.reshape(S, S, Wd), acc=a_pl.reshape(S, S, Wd), rays=r_pl.reshape(S, S), prim=pl["prim"], src=pl["src"]))

            rows = {"bake": [], "hand": [], "hand_full": []}
            for run in range(a.runs + 1):                       # interleaved: the routes see the same machine
                tb, owned, b = bake()
                th, h_owned, _ = hand(False)
                tf, f_owned, f = hand(True)
                assert owned == h_owned == f_owned
                for k in ("out", "acc", "rays", "prim", "src"):
                    assert np.array_equal(b[k].view(np.uint32), f[k].view(np.uint32)), f"{name}: bakeTexels differs from the route by hand in {k}"
                if run > 0:                                     # (round 0 warms up: buffers allocated, code loaded)
                    rows["bake"].append(tb)
                    rows["hand"].append(th)
                    rows["hand_full"].append(tf)
            case = dict(owned=owned, rays=owned * dirs, bit_equal=True, mean_out=round(float(b["out"].mean()), 6),
                        **{r: {k + "_ms": brief([x[k] for x in rows[r]]) for k in rows[r][0]} for r in rows})
            case["raster_share_of_kernel_time"] = round(case["bake"]["texels_ms"]["median"] / (case["bake"]["texels_ms"]["median"] + case["bake"]["kernel_ms"]["median"]), 4)
            case["wall_ratio_hand_over_bake"] = round(case["hand"]["wall_ms"]["median"] / case["bake"]["wall_ms"]["median"], 2)
            res["cases"][name] = case
    finally:
        rt.cleanupRenderer()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
