"""What the tests of the preview calls (renderGuides, denoiseFrame, accumulateFrame) share.  No test: a plain module, imported as guides_reference is, by
tests/test_gpu_{guides,denoise,accumulate}.py, tests/test_{guides,denoise,accumulate}_api.py and the two references of the whole-image passes
(tests/denoise_reference.py and tests/accumulate_reference.py take default_flags and oracle_frame from here)."""
import os
import subprocess
import sys

import numpy as np

import guides_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMODULATE, SAME_PRIM = 1, 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, ref, what):
    """Bit for bit: np.array_equal on the raw 32-bit words."""
    diff = bits(got) != bits(ref)
    print(f"{what}: {int(diff.sum())} of {diff.size} words differ")
    assert np.array_equal(bits(got), bits(ref)), (what, int(diff.sum()), np.argwhere(diff)[:5].tolist())


def stats_tuple(st):
    return (st.kernel_ms, st.total_ms, st.samples, st.num_launches, st.rays, st.prim_tests, st.node_visits, st.exec_tests, st.shadow_rays, st.box_tests,
            tuple(st.ref_stats))


def init_frame(rt, O, name, **opts):
    """Initialises the named frame of guides_reference (a sequence: its frame-0 camera); returns (framebuffer view, options, is-mesh)."""
    mesh = name in G.MESH_FRAMES
    if mesh:
        f = G.mesh_frame(rt, O, name)
        ks, keep = rt.make_kernel_scene(f["hm"], f["mats"], f["tex"], floor=f["floor"])
        fb = rt.initRenderer(ks, f["cam"], f["nx"], f["ny"], 16, keepalive=keep)
        if f["floor"] is not None:
            opts = dict(opts, floor=1)
    else:
        sp, mt, cam, nx, ny = G.sphere_frame(rt, name)
        fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 20)
    o = rt.getDefaultRenderOptions(not mesh)
    if opts:
        rt.setRenderOptions(o, **opts)
    return fb, o, mesh


def exits_99(body):
    """The library's misuse convention: `body` (after the imports: C, np, rt) in a child process of its own ends with 'rt error' on stderr and exit status 99
    (a clean exit of a host-side check)."""
    code = ("import sys; sys.path.insert(0, %r); import ctypes as C; import numpy as np; import cuda_raytracing_optimized_amd as rt\n" % ROOT) + body
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 99, (r.returncode, r.stderr[-1000:])
    assert "rt error" in r.stderr


def default_flags(mesh):
    return DEMODULATE if mesh else DEMODULATE | SAME_PRIM


def oracle_frame(rt, O, name, spp, cam=None):
    """The CPU oracle's render of a named frame with the default options (and the floor of the *_floor frame), from `cam` or the frame's own camera."""
    if name in G.MESH_FRAMES:
        f = G.mesh_frame(rt, O, name)
        opt = O.default_options(False)
        if f["floor"] is not None:
            opt.floor = 1
        fb, _ = O.render(O.mesh_scene(f["hm"], f["mats"], f["tex"], f["floor"]), f["cam"] if cam is None else cam, opt, f["nx"], f["ny"], spp, 16)
        return fb
    sp, mt, own, nx, ny = G.sphere_frame(rt, name)
    fb, _ = O.render(O.sphere_scene(sp, mt), own if cam is None else cam, O.default_options(True), nx, ny, spp, 20)
    return fb
