"""The exact re-normalisation of unit directions (csrc/rt_renorm.h) on the device: the probe against the host program built from the same header, and
whole frames against the CPU oracle, bit for bit ("bits" = float32 words), at the smallest sizes that still reach each form of the sphere kernel - the
folded cost-ordered form, a six-wave kind, the general form - a frame of preset materials whose subsurface event leaves the path's direction un-normalised
(the plain path inside a frame), and the mesh kernel's make_ray under NEE + RR."""
import os
import subprocess

import numpy as np
import pytest

from test_renorm import build_dump

pytestmark = pytest.mark.gpu

VIEW = dict(lookfrom=(2.5, 0.4, 1.5), lookat=(0.5, 0.1, 0.5), vfov=20.0, focus=3.0)        # the close-up of tests/test_gpu_sphere_form.py: chain pixels included
NS = 16
GENERAL, DEFAULT = 0, 1
CLASSES = 5
_REFS = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, ref, what=""):
    assert not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    assert np.array_equal(_bits(got), _bits(ref)), (what, int(np.count_nonzero(_bits(got) != _bits(ref))))


def _scene(rt, nx, ny):
    sp, mt, _ = rt.scene_random_spheres(nx, ny)
    return sp, mt, rt.make_camera(VIEW["lookfrom"], VIEW["lookat"], (0, 1, 0), VIEW["vfov"], nx / ny, 0.0, VIEW["focus"])


def _ref(rt, O, nx, ny):
    """The oracle's frame, computed once per size and shared (read-only)."""
    if (nx, ny) not in _REFS:
        sp, mt, cam = _scene(rt, nx, ny)
        fb, _ = O.render(O.sphere_scene(sp, mt), cam, O.default_options(True), nx, ny, NS, 50)
        fb.setflags(write=False)
        _REFS[(nx, ny)] = fb
    return _REFS[(nx, ny)]


def _two_frames(rt, nx, ny):
    """Two frames in a row (measured, then ordered by the first frame's cost map): [(frame, phases, form, last launch record)]."""
    sp, mt, cam = _scene(rt, nx, ny)
    fb = rt.initRendererSpheres(sp, mt, cam, nx, ny, 50)
    out = []
    for _ in range(2):
        rt.runRenderer(NS)
        recs = rt.last_launches()
        out.append((np.array(fb, copy=True), [r["phase"] for r in recs], rt.last_sphere_form(), recs[-1]))
    rt.cleanupRenderer()
    return out


# ---- the probe ---------------------------------------------------------------------------------------------------------------------------------------

def test_probe_against_the_host_program(rt, tmp_path):
    """About 50 k bounce directions from the host program's seeded generator - at least 100 of every class, found there by rejection - and its edge inputs
    (not unit, zero, infinite, NaN, -0 components, tiny components, components on every threshold under every class): the device's bits are the host's."""
    exe = build_dump(tmp_path)
    text = subprocess.run([exe, "--sample", "20261019", "100", "50000"], capture_output=True, text=True, check=True).stdout
    host = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    v = np.array([[int(w, 16) for w in line.split()] for line in text.splitlines()], dtype=np.uint32)
    h = np.array([[int(w, 16) for w in line.split()[:6]] + [int(w) for w in line.split()[6:]] for line in host.splitlines()], dtype=np.uint32)
    assert len(v) == len(h) > 50000
    hist = np.bincount(h[:, 7][h[:, 6] == 1], minlength=CLASSES)
    assert len(hist) == CLASSES and hist.min() >= 100, hist                        # every class through the exact path
    assert np.count_nonzero(h[:, 6] == 0) >= 100                                    # and the plain path
    nan = lambda a: (a & 0x7FFFFFFF) > 0x7F800000
    same = lambda a, b: (a == b) | (nan(a) & nan(b))
    assert same(h[:, 0:3], h[:, 3:6]).all()                                         # the host program's own check: the exact path is plain unit()
    got = _bits(rt.Probe("parity").renorm(v.view(np.float32)))
    bad = ~same(got, h[:, 0:3]).all(axis=1)
    assert not bad.any(), (int(bad.sum()), v[bad][:3], got[bad][:3], h[bad][:3])


# ---- frames ------------------------------------------------------------------------------------------------------------------------------------------

def test_folded_form_two_frames_in_a_row(rt, O):
    nx, ny = 128, 64
    ref = _ref(rt, O, nx, ny)
    (first, ph1, form1, last1), (second, ph2, form2, last2) = _two_frames(rt, nx, ny)
    assert ph1 == [1, 2] and ph2 == [2] and form1 == form2 == DEFAULT, (ph1, form1, ph2, form2)
    assert (last2["cls"], last2["lean"]) == (2, 3), last2
    _same(first, ref, "measured")
    _same(second, ref, "ordered by the map")


def test_six_wave_kind(rt, O, monkeypatch):
    monkeypatch.setenv("RT_LEAN6_PIXELS", "1")
    nx, ny = 128, 64
    ref = _ref(rt, O, nx, ny)
    for (got, phases, form, last), frame in zip(_two_frames(rt, nx, ny), ("measured", "ordered by the map")):
        assert phases[-1] == 2 and (last["cls"], last["lean"], last["threads"]) == (2, 7, 768), (frame, phases, last)
        _same(got, ref, frame)


def test_general_form(rt, O, monkeypatch):
    monkeypatch.setenv("RT_POOL", "8")
    nx, ny = 96, 64
    ref = _ref(rt, O, nx, ny)
    for (got, phases, form, last), frame in zip(_two_frames(rt, nx, ny), ("measured", "ordered by the map")):
        assert phases[-1] == 2 and last["cls"] == 2 and form == GENERAL, (frame, phases, form, last)
        _same(got, ref, frame)


def test_preset_materials_in_a_frame(rt, O):
    """The two scenes of dormant presets of tests/test_gpu_parity_spheres.py (test_preset_materials_in_a_frame), which the kernel without BASIC renders.
    The presets without libm calls: the oracle's frame bit for bit.  The scene with the subsurface preset, whose scattering event stores a direction that
    is not unit (material.h:128) - the next ray's re-normalisation must take it down the plain path: that fixture's own bound, at least 99.5 % of the
    channels within 1e-5 relative.  Bits are out of reach there whatever normalises the direction: the preset's logf / expf are OCML's on the device and
    glibc's in the oracle (at 64x40x4 with the preset on sphere 485 alone, 58 words of the frame differ from the oracle's, the same 58 with unit() in
    place of the exact path: the two libraries' frames are equal bit for bit)."""
    nx, ny, ns = 64, 40, 4
    sp, mt, cam = rt.scene_random_spheres(nx, ny)
    small = np.arange(1, 485)
    kinds = np.array([rt.RT_FLOOR_COAT, rt.RT_FLOOR_DIFFUSE, rt.RT_MODEL_COAT, rt.RT_MODEL_DIFFUSE, rt.RT_MODEL_GLOSSY, rt.RT_MODEL_GLASS])

    def frames(m):
        ref, _ = O.render(O.sphere_scene(sp, m), cam, O.default_options(True), nx, ny, ns, 50)
        fb = rt.initRendererSpheres(sp, m, cam, nx, ny, 50)
        rt.runRenderer(ns, 8, 8)
        got = np.array(fb, copy=True)
        rt.cleanupRenderer()
        return got, ref

    m1 = mt.copy()
    m1["type"][small] = kinds[small % len(kinds)]
    m1["type"][485] = rt.RT_MODEL_GLASS
    _same(*frames(m1), "presets without libm calls")
    m2 = mt.copy()
    m2["type"][0] = rt.RT_FLOOR_CHECKER
    m2["type"][485] = rt.RT_MODEL_SSS
    m2["type"][small[::3]] = rt.RT_MODEL_TINTEDGLASS
    got, ref = frames(m2)
    assert not np.isnan(got).any()
    rel = np.abs(got - ref) <= 1e-5 * np.maximum(np.abs(ref), 1e-3)
    print("subsurface scene: channels within 1e-5 relative", rel.mean(), "differing words", int(np.count_nonzero(_bits(got) != _bits(ref))))
    assert rel.mean() >= 0.995, rel.mean()


def test_staircase_mesh_with_nee_and_rr(rt, O):
    tris, mats = rt.scene_staircase_procedural(1)
    hm = rt.HostMesh.build(tris, 5)
    nx, ny, ns = 48, 60, 8
    cam = rt.staircase_camera(nx, ny)
    ks, keep = rt.make_kernel_scene(hm, mats)
    fb = rt.initRenderer(ks, cam, nx, ny, 16, keepalive=keep)
    rt.runRenderer(ns, 8, 8)
    got = np.array(fb, copy=True)
    rt.cleanupRenderer()
    ref, _ = O.render(O.mesh_scene(hm, mats), cam, O.default_options(False), nx, ny, ns, 16)
    _same(got, ref, "staircase")
