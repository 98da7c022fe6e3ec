"""displayFrame beside the host conversion it replaces (rtDisplayFrameHost: one libm powf per channel, single-threaded) on one GPU, in one process.

    python tools/bench_display.py [--cases C2] [--repeats 20] [--out profiles/display.json]

C2: random spheres 1200x800 (the bench frame).  After runRenderer(1), a previewFrame and a warm-up, medians (and the best) of --repeats:
  * display_kernel_ms / display_auto_kernel_ms: rtLastDisplayMs without and with RT_DISPLAY_AUTO_EXPOSURE (transform alone; clear + histogram + resolve + transform);
  * display_call_ms / display_auto_call_ms: the wall time of the whole call with in = NULL (upload 12 B per pixel, kernels, download 4 B per pixel);
  * display_from_preview_call_ms: the whole call with RT_DISPLAY_FROM_PREVIEW (no upload);
  * preview_kernel_ms / preview_call_ms: rtLastPreviewMs and the wall time of the previewFrame of the same session;
  * host_call_ms: rtDisplayFrameHost on the same frame on this machine's CPU (--host-repeats, default 5);
  * same_bytes: the device's bytes equal the host's on that frame.
The claim DESIGN.md 3.14 checks: display_call_ms < host_call_ms."""
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

from bench_guides import CASES, open_case  # noqa: E402


def run_case(rt, name, w, repeats, host_repeats):
    keep = open_case(rt, w)
    nx, ny = w["nx"], w["ny"]
    fb = rt._state["fb"]
    rt.runRenderer(1)
    frame = np.array(fb, copy=True)
    out, pre = np.empty((ny, nx, 4), np.uint8), np.empty((ny, nx, 3), np.float32)
    A, P = rt.RT_DISPLAY_AUTO_EXPOSURE, rt.RT_DISPLAY_FROM_PREVIEW
    for k in range(4):                               # warm-up: code objects, first touch of the buffers
        rt.previewFrame(out=pre)
        rt.display_frame(out=out)
        rt.display_frame(out=out, flags=A)
        rt.display_frame(out=out, flags=P)
    t = {k: [] for k in ("k", "ka", "w", "wa", "wp", "pk", "pw")}
    for k in range(repeats):
        t0 = time.perf_counter()
        rt.previewFrame(out=pre)
        t1 = time.perf_counter()
        rt.display_frame(out=out)
        t2 = time.perf_counter()
        t["k"].append(rt.last_display_ms())
        t3 = time.perf_counter()
        rt.display_frame(out=out, flags=A)
        t4 = time.perf_counter()
        t["ka"].append(rt.last_display_ms())
        t5 = time.perf_counter()
        rt.display_frame(out=out, flags=P)
        t6 = time.perf_counter()
        t["pw"].append((t1 - t0) * 1e3); t["w"].append((t2 - t1) * 1e3); t["wa"].append((t4 - t3) * 1e3); t["wp"].append((t6 - t5) * 1e3)
        t["pk"].append(rt.last_preview_ms())
    host = []
    for k in range(host_repeats):
        t0 = time.perf_counter()
        want = rt.display_frame_host(frame)
        host.append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(rt.display_frame(frame), want))
    rt.cleanupRenderer()
    del keep
    med, r4 = statistics.median, lambda x: round(x, 4)
    return dict(case=name, kind=w["kind"], nx=nx, ny=ny, repeats=repeats, host_repeats=host_repeats,
                display_kernel_ms=r4(med(t["k"])), display_kernel_ms_best=r4(min(t["k"])),
                display_auto_kernel_ms=r4(med(t["ka"])), display_auto_kernel_ms_best=r4(min(t["ka"])),
                display_call_ms=r4(med(t["w"])), display_call_ms_best=r4(min(t["w"])),
                display_auto_call_ms=r4(med(t["wa"])),
                display_from_preview_call_ms=r4(med(t["wp"])), display_from_preview_call_ms_best=r4(min(t["wp"])),
                preview_kernel_ms=r4(med(t["pk"])), preview_call_ms=r4(med(t["pw"])),
                host_call_ms=r4(med(host)), host_call_ms_best=r4(min(host)), same_bytes=same,
                call_over_host=r4(med(t["w"]) / med(host)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="C2")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import cuda_raytracing_optimized_amd as rt
    if rt.device_count() < 1:
        raise SystemExit("bench_display: no HIP device visible")
    lines = []
    for name in args.cases.split(","):
        line = run_case(rt, name, CASES[name], args.repeats, args.host_repeats)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
