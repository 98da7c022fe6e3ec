"""CPU only: the frames of tests/mesh_materials_support.py test what they claim, and the bound tests/test_gpu_mesh_materials.py holds the libm-based
presets to is one the reference itself keeps when its libm moves by an ulp (oracle/liboracle_nudge.so against oracle/liboracle.so).  Everything here is
the oracle's own output: nothing of the code under test runs.  Frames are rendered at the 4 samples per pixel the GPU tests use."""
import numpy as np
import pytest

import mesh_materials_support as M

SPP = 4


@pytest.mark.parametrize("name,nee", [(n, 1) for n in M.FRAMES] + [("stair_exact", 0)])
def test_every_kind_matters(rt, O, name, nee):
    """Each material type of the frame's table, replaced by a different opaque material, changes at least 3 % of the pixels: a kernel that shaded the kind
    wrongly could not hide."""
    f = M.frame(rt, O, name)
    own = M.oracle_frame(rt, O, name, SPP, nee)[0]
    types = sorted(set(f["mats"]["type"].tolist()))
    assert set(types) >= ({0, 1, 5, 7, 8, 9, 10, 11} if name == "stair_loose" else set(M.EXACT_TYPES) if name in M.EXACT_FRAMES else set(range(12)))
    for ty in types:
        other, _ = M.oracle_render(rt, O, name, SPP, M.replaced(rt, f["mats"], ty), nee)
        share = float((M.bits(own) != M.bits(other)).any(axis=2).mean())
        print(f"{name} nee {nee}: type {ty} changes {share:.3f} of the pixels")
        assert share >= 0.03, (name, nee, ty, share)


def test_stair_exact_table(rt, O):
    """The kinds the issue names sit on the nine mesh ids the camera sees, most pixels first, and the textured metal is a metal."""
    import guides_reference as G
    f = M.frame(rt, O, "stair_exact")
    ids = G._stair_visible_ids(rt, O)
    assert len(ids) >= 9
    mats = f["mats"]
    expect = [(rt.RT_DIFFUSE, 0), (rt.RT_MODEL_DIFFUSE, -1), (rt.RT_FLOOR_COAT, -1), (rt.RT_METAL, 1), (rt.RT_MODEL_GLOSSY, -1), (rt.RT_MODEL_COAT, -1),
              (rt.RT_FLOOR_DIFFUSE, -1), (rt.RT_MODEL_GLASS, -1), (rt.RT_GLASS, -1)]
    assert [(int(mats["type"][m]), int(mats["texId"][m])) for m in ids[:9]] == expect
    assert mats["param"][ids[3]] == np.float32(0.05) and mats["param"][ids[8]] == np.float32(1.5)
    assert not set(mats["type"].tolist()) & set(M.loose_types(rt))


@pytest.mark.parametrize("name", ["soup_exact", "soup_all"])
def test_high_ids_and_padding(rt, O, name):
    """The soups have real triangles whose mesh id needs the byte's top bit, a different material there than at id & 0x7F, and non-zero padding beside
    every id: a device that read the id through a wider or narrower mask would shade another material."""
    f = M.frame(rt, O, name)
    tr = M.real_triangles(f["hm"])
    assert len(tr) == 400 and len(f["mats"]) == 256
    high = tr["meshID"] >= 128
    assert int(high.sum()) == 202
    assert (tr["_pad"] != 0).all()
    ty = f["mats"]["type"]
    assert (ty[tr["meshID"][high]] != ty[tr["meshID"][high] & 0x7F]).mean() > 0.5
    k = np.arange(256)
    assert np.array_equal(ty, np.array(M.EXACT_TYPES if name == "soup_exact" else list(range(12)))[k % (9 if name == "soup_exact" else 12)])
    assert np.array_equal(f["mats"]["texId"], np.where(k % 16 == 5, 0, np.where(k % 16 == 13, 1, -1)))
    tc = tr["texCoords"]
    assert tc.min() < -1 and tc.max() > 1                       # the texture wrap is taken


@pytest.mark.parametrize("name", M.FRAMES)
def test_counters(rt, O, name):
    """Shadow rays with NEE on, sky and floor reached on the soups, no NaN."""
    fb, cnt = M.oracle_frame(rt, O, name, SPP)
    assert not np.isnan(fb).any() and cnt.ref_stats[rt.RT_STAT_NAN] == 0
    assert cnt.shadow_rays > 0 and cnt.ref_stats[rt.RT_STAT_SHADOWS] == cnt.shadow_rays
    assert cnt.ref_stats[rt.RT_STAT_SHADOWS_NOHITS] > 0
    if M.is_soup(name):
        assert cnt.ref_stats[rt.RT_STAT_SECONDARY_NOHIT] > 0 and cnt.ref_stats[rt.RT_STAT_PRIMARY_NOHITS] > 0
        _, off = M.oracle_frame(rt, O, name, SPP, 1, 0)
        assert off.ref_stats[rt.RT_STAT_SECONDARY_NOHIT] == 0   # that counter is the floor's
    if name == "stair_exact":
        assert M.oracle_frame(rt, O, name, SPP, 0)[1].shadow_rays == 0


@pytest.mark.parametrize("name", M.LOOSE_FRAMES)
def test_untouched_share(rt, O, name):
    """Between 15 % and 85 % of a loose frame's pixels are untouched: the exact half and the bounded half of the GPU comparison both have pixels."""
    share = float(M.untouched(rt, O, name, SPP).mean())
    print(f"{name}: untouched share {share:.3f}")
    assert 0.15 <= share <= 0.85
    if M.is_soup(name):
        assert 0.15 <= float(M.untouched(rt, O, name, SPP, 0).mean()) <= 0.85      # the floor-less frame of the tile kernel


@pytest.mark.parametrize("name", M.EXACT_FRAMES)
def test_exact_frames_have_nothing_to_nudge(rt, O, name):
    """No libm-based preset in an exact frame: the nudged twin renders the oracle's bits (and wraps nothing else)."""
    a, ca = M.oracle_frame(rt, O, name, SPP)
    b, cb = M.oracle_frame(rt, O, name, SPP, nudged=True)
    assert np.array_equal(M.bits(a), M.bits(b))
    assert list(ca.ref_stats) == list(cb.ref_stats)


@pytest.mark.parametrize("name", M.LOOSE_FRAMES)
def test_the_loose_bound_is_one_the_reference_keeps(rt, O, name):
    """The oracle with sinf / logf / expf of the three presets an ulp off: every channel within 1e-5 * max(|ref|, 1e-3) of the oracle, the same rays and
    shadow rays, the untouched pixels bit-equal - and the twin is a different renderer (some channels do differ in bits)."""
    ref, cr = M.oracle_frame(rt, O, name, SPP)
    got, cg = M.oracle_frame(rt, O, name, SPP, nudged=True)
    ok = M.within_loose_bound(got, ref)
    differ = M.bits(got) != M.bits(ref)
    print(f"{name}: within the bound {ok.mean():.4f}, largest difference {np.abs(got - ref).max():.3g}, channels that differ in bits {differ.mean():.4f}, "
          f"rays {cg.rays} / {cr.rays}, shadow rays {cg.shadow_rays} / {cr.shadow_rays}")
    assert ok.all(), int((~ok).sum())
    assert (cg.rays, cg.shadow_rays) == (cr.rays, cr.shadow_rays)
    assert differ.mean() > 0.005
    u = M.untouched(rt, O, name, SPP)
    assert np.array_equal(M.bits(got)[u], M.bits(ref)[u])
    assert differ.any(axis=2)[~u].any() and not differ.any(axis=2)[u].any()
