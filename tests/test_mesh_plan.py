"""CPU: what the mesh launcher decides (plan_mesh, csrc/rt_mesh_plan.h) against the rules restated here, field by field.  In PARITY mode a frame's bits do not
depend on the work order, so a wrong stride, threshold, grid or chain constant fails no render test - it only costs speed; this test holds those values.
tests/mesh_plan_dump.cpp includes the header, is compiled as plain C++ (no kernel, no HIP call) and runs the plan on the cases fed to it: hand-written rows on
both sides of every boundary of the rules, and a seeded sweep over the same fields."""
import math
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")

INPUTS = ("nx rows ns queue dbg counters lean_ok floor_on sentinels leaf_ofs leaf_tri nppl first_leaf rng_mode px_state px_rays ord_rec order ord_state ord_rays "
          "acc_first p1_segments xcd_queues variant cus mesh_lean mesh_tile_order mesh_two mesh_split mesh_heavy mesh_rounds mesh_rev mesh_chain_thr mesh_chain_lanes "
          "mesh_chain_frac").split()
OUTPUTS = "error frame trav dbg stats lean grid_x grid_y threads lds stride stride1 min_traversing min_traversing1 leaf_thr leaf_thr1 split chain_top_thr xcd_queues".split()

# the constants launcher and kernel share (rt_mesh_plan.h), restated
WAVES_PER_WG, THREADS, LEAN_WAVES, MIN_TRAVERSING_CLASSIC, LEAF_CNT_LDS = 4, 256, 4, 40, 32768
TILES, TWO, SINGLE = 0, 1, 2            # MeshFrame
NO_QUEUE = 1                            # MeshPlanError

# The staircase of the benchmark at 1920 x 1080 x 256 spp, reference stream, packed parked records, the switches' defaults (RtSwitches, rt_params.h)
BASE = dict(nx=1920, rows=1080, ns=256, queue=1, dbg=0, counters=0, lean_ok=1, floor_on=0, sentinels=1, leaf_ofs=1, leaf_tri=1, nppl=5, first_leaf=16384, rng_mode=0,
            px_state=1, px_rays=1, ord_rec=1, order=1, ord_state=0, ord_rays=0, acc_first=0, p1_segments=1, xcd_queues=8, variant=0, cus=256,
            mesh_lean=1, mesh_tile_order=0, mesh_two=1, mesh_split=2, mesh_heavy=5, mesh_rounds=2, mesh_rev=0, mesh_chain_thr=448, mesh_chain_lanes=6, mesh_chain_frac=8)
assert list(BASE) == INPUTS


def coprime_stride(n):
    """rt_coprime_stride (rt_params.h): ~0.618 n, odd, coprime with n."""
    cand = int(float(n) * 0.6180339887) | 1
    while math.gcd(cand, n) != 1:
        cand += 2
    return (cand % n) & 0xFFFFFFFF


def expected(c):
    """The rules of the mesh launcher, restated: the plan of case `c` as a dict over OUTPUTS."""
    pl = dict(error=0, frame=SINGLE, trav=0, dbg=0, stats=0, lean=0, grid_x=1, grid_y=1, threads=THREADS, lds=0, stride=1, stride1=1,
              min_traversing=0, min_traversing1=0, leaf_thr=0, leaf_thr1=0, split=0, chain_top_thr=0, xcd_queues=0)
    v = c["variant"]
    tiles_x, tiles_y = (c["nx"] + 7) // 8, (c["rows"] + 7) // 8
    if v & 0xFF == 1:           # the tile kernel: a grid, nothing else
        pl.update(frame=TILES, grid_x=(c["nx"] + 8 * WAVES_PER_WG - 1) // (8 * WAVES_PER_WG), grid_y=tiles_y)
        return pl
    if not c["queue"]:
        pl["error"] = NO_QUEUE
        return pl
    classic = (v >> 24) & 3 == 1
    nppl_ok = 1 <= c["nppl"] <= 16
    lean = bool(c["mesh_lean"] and not classic and not c["dbg"] and not c["counters"] and c["lean_ok"] and not c["floor_on"] and c["sentinels"] and
                c["leaf_ofs"] and c["leaf_tri"] and nppl_ok and c["first_leaf"] <= LEAF_CNT_LDS)
    # the instantiation: classic takes dbg, else counters, else plain; the default traversal lean, else dbg, else counters, else plain
    pl.update(trav=int(classic), lean=int(lean), dbg=int(bool(c["dbg"])), stats=int(bool(c["counters"]) and not c["dbg"]))
    wg_per_cu = (v >> 8) & 0xFF
    if wg_per_cu == 0:
        wg_per_cu = LEAN_WAVES if lean else (5 if classic else 4)
    total_px = tiles_x * tiles_y * 64
    pl["grid_x"] = max(1, min(c["cus"] * wg_per_cu * 4 // WAVES_PER_WG, (total_px + THREADS - 1) // THREADS))
    stride = coprime_stride(total_px) if total_px > 64 and not c["mesh_tile_order"] else 1
    mt = (v >> 16) & 0xFF
    if mt == 0:
        mt = MIN_TRAVERSING_CLASSIC if classic else 24
    thr = (v >> 26) & 0x3F
    if thr == 0:
        thr = 64 // c["nppl"] if nppl_ok else 16
    pl.update(stride=stride, min_traversing=mt, leaf_thr=thr)
    if not classic and c["leaf_ofs"] and c["first_leaf"] <= LEAF_CNT_LDS:
        pl["lds"] = (c["first_leaf"] + 15) & ~15
    parked = c["px_state"] and c["px_rays"] and (c["ord_rec"] or (c["order"] and c["ord_state"] and c["ord_rays"]))
    two = (c["mesh_two"] and not classic and not c["dbg"] and not c["counters"] and c["rng_mode"] == 0 and parked and c["acc_first"] == 0 and
           c["ns"] >= 4 * c["mesh_split"] and c["nx"] <= 65535 and c["rows"] <= 65535)
    if not two:
        return pl
    pl.update(frame=TWO, split=c["mesh_split"], chain_top_thr=c["mesh_chain_thr"], stride1=stride, min_traversing1=mt, leaf_thr1=thr, xcd_queues=c["xcd_queues"])
    if c["p1_segments"] and total_px > 512 and not c["mesh_tile_order"]:
        pl.update(stride1=coprime_stride(total_px >> 3), min_traversing1=mt | 1 << 8)
    if c["mesh_rev"]:           # cheapest first: from the back of the lists, and one queue for the machine (the per-XCD queues are handed on from the front)
        pl.update(stride=0xFFFFFFFF, xcd_queues=0)
    pl["leaf_thr"] = thr | (c["mesh_heavy"] & 0xF) << 8 | (c["mesh_rounds"] & 0xF) << 12 | c["mesh_chain_lanes"] << 16 | c["mesh_chain_frac"] << 24
    return pl


def case(**kw):
    assert set(kw) <= set(BASE), kw
    return dict(BASE, **kw)


def variant(kernel=0, wgs=0, min_trav=0, trav=0, leaf_thr=0):
    return kernel | wgs << 8 | min_trav << 16 | trav << 24 | leaf_thr << 26


def boundary_cases():
    """Each boundary of the rules from both sides, every variant field zero and non-zero, every switch at its default (BASE) and at one other value."""
    three_arrays = dict(ord_rec=0, order=1, ord_state=1, ord_rays=1)
    cs = [case()]
    cs += [case(ns=8), case(ns=7), case(mesh_split=4, ns=16), case(mesh_split=4, ns=15), case(mesh_split=5, ns=16)]         # ns = 4 split and one below
    cs += [case(nx=65535, rows=8), case(nx=65536, rows=8), case(nx=8, rows=65535), case(nx=8, rows=65536)]
    cs += [case(first_leaf=LEAF_CNT_LDS), case(first_leaf=LEAF_CNT_LDS + 1), case(first_leaf=LEAF_CNT_LDS + 1, leaf_ofs=0), case(first_leaf=1), case(first_leaf=17)]
    cs += [case(nppl=16), case(nppl=17), case(nppl=1), case(nppl=0), case(nppl=3)]
    cs += [case(nx=8, rows=8), case(nx=16, rows=8), case(nx=9, rows=8), case(nx=1, rows=1)]                                 # total_px 64 / 128: stride 1 against coprime
    cs += [case(nx=64, rows=8), case(nx=72, rows=8), case(nx=64, rows=8, p1_segments=0), case(nx=72, rows=8, p1_segments=0)]       # total_px 512 / 576: segments
    cs += [case(nx=72, rows=8, mesh_tile_order=1), case(nx=16, rows=8, mesh_tile_order=1)]
    cs += [case(nx=96, rows=64), case(nx=48, rows=60), case(nx=96, rows=64, variant=variant(wgs=8)), case(nx=97, rows=57)]   # blocks clipped by the pixels
    cs += [case(cus=256), case(cus=1), case(cus=1, nx=8, rows=8), case(cus=304), case(cus=256, variant=variant(wgs=255))]    # ... by cus x wg_per_cu
    cs += [case(), case(**three_arrays), case(ord_rec=0, order=0), case(ord_rec=0, order=1, ord_state=1, ord_rays=0), case(ord_rec=0, order=1, ord_state=0, ord_rays=1),
           case(ord_rec=0, order=0, ord_state=1, ord_rays=1), case(px_state=0), case(px_rays=0), case(px_state=0, **three_arrays)]
    cs += [case(acc_first=0), case(acc_first=8), case(xcd_queues=0), case(xcd_queues=0, mesh_rev=1)]
    cs += [case(variant=variant(kernel=1)), case(variant=variant(kernel=1), queue=0), case(variant=variant(kernel=1), nx=97, rows=57), case(variant=variant(kernel=2)),
           case(queue=0), case(variant=variant(wgs=6)), case(variant=variant(min_trav=32)), case(variant=variant(trav=1)), case(variant=variant(trav=2)),
           case(variant=variant(trav=3)), case(variant=variant(leaf_thr=12)), case(variant=variant(leaf_thr=63)), case(variant=variant(trav=1, min_trav=48, wgs=3, leaf_thr=9)),
           case(variant=variant(trav=1), dbg=1), case(variant=variant(trav=1), counters=1), case(variant=variant(trav=1), dbg=1, counters=1)]
    cs += [case(dbg=1), case(counters=1), case(dbg=1, counters=1), case(rng_mode=1), case(lean_ok=0), case(floor_on=1), case(sentinels=0), case(leaf_ofs=0),
           case(leaf_tri=0), case(leaf_ofs=0, leaf_tri=0), case(lean_ok=0, ns=4)]
    cs += [case(mesh_lean=0), case(mesh_lean=0, ns=4), case(mesh_tile_order=1), case(mesh_two=0), case(mesh_split=1), case(mesh_split=8), case(mesh_heavy=0),
           case(mesh_heavy=7), case(mesh_heavy=21), case(mesh_rounds=0), case(mesh_rounds=3), case(mesh_rounds=18), case(mesh_rev=1), case(mesh_rev=1, mesh_two=0),
           case(mesh_chain_thr=17), case(mesh_chain_lanes=0), case(mesh_chain_lanes=64), case(mesh_chain_frac=0), case(mesh_chain_frac=15)]
    return cs


def sweep_cases(n=4000, seed=20240607):
    """A seeded sweep over the same fields: sizes around the boundaries and ordinary ones, every flag both ways, every variant field zero in half the cases."""
    rng = random.Random(seed)
    flag = lambda p=0.5: int(rng.random() < p)
    pick = rng.choice
    cs = []
    for _ in range(n):
        nx, rows = pick([(pick([1, 8, 9, 16, 64, 72, 96, 200, 640, 1920, 3840, 65535, 65536]), pick([1, 8, 57, 64, 135, 1080, 2160])), (rng.randint(1, 4000), rng.randint(1, 2400)),
                         (pick([8, 16, 96]), pick([65535, 65536]))])
        split = pick([1, 2, 2, 2, 4, 5, 8])
        v = variant(kernel=pick([0, 0, 0, 0, 0, 0, 0, 1, 2]), wgs=pick([0, 0, rng.randint(1, 255)]), min_trav=pick([0, 0, rng.randint(1, 255)]), trav=pick([0, 0, 0, 0, 0, 1, 1, 2, 3]),
                    leaf_thr=pick([0, 0, rng.randint(1, 63)]))
        cs.append(case(nx=nx, rows=rows, ns=pick([1, 4 * split - 1, 4 * split, 4 * split, 64, 256, rng.randint(1, 1000)]), queue=flag(0.97), dbg=flag(0.06), counters=flag(0.08),
                       lean_ok=flag(0.8), floor_on=flag(0.15), sentinels=flag(0.85), leaf_ofs=flag(0.85), leaf_tri=flag(0.85), nppl=pick([0, 1, 2, 3, 4, 5, 5, 5, 8, 15, 16, 17, 32, 64]),
                       first_leaf=pick([1, 2, 17, 4096, 16384, LEAF_CNT_LDS - 1, LEAF_CNT_LDS, LEAF_CNT_LDS + 1, 1 << 20, rng.randint(1, 70000)]), rng_mode=flag(0.08),
                       px_state=flag(0.95), px_rays=flag(0.95), ord_rec=flag(), order=flag(0.9), ord_state=flag(0.9), ord_rays=flag(0.9), acc_first=pick([0, 0, 0, 0, 0, 8, rng.randint(1, 64)]),
                       p1_segments=flag(0.7), xcd_queues=pick([8, 8, 0]), variant=v, cus=pick([1, 2, 64, 256, 256, 304, rng.randint(1, 512)]), mesh_lean=flag(0.8), mesh_tile_order=flag(0.2), mesh_two=flag(0.9),
                       mesh_split=split, mesh_heavy=pick([5, 0, rng.randint(0, 40)]), mesh_rounds=pick([2, 0, rng.randint(0, 40)]), mesh_rev=flag(0.2),
                       mesh_chain_thr=pick([448, 17, rng.randint(17, 4000)]), mesh_chain_lanes=pick([6, 0, 64, rng.randint(0, 64)]), mesh_chain_frac=pick([8, 0, rng.randint(0, 15)])))
    return cs


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/mesh_plan_dump.cpp, compiled as plain C++ against the header; returns run(cases) -> list of plans (dicts over OUTPUTS)."""
    exe = str(tmp_path_factory.mktemp("mesh_plan") / "mesh_plan_dump")
    r = subprocess.run([os.environ.get("HIPCC", "hipcc"), "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "mesh_plan_dump.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    fields = subprocess.run([exe, "--fields"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert [f.split() for f in fields] == [INPUTS, OUTPUTS]

    def run(cases):
        text = "".join(" ".join(str(c[k]) for k in INPUTS) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-1000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        return [dict(zip(OUTPUTS, [int(t) for t in line.split()], strict=True)) for line in lines]
    return run


def _compare(dump, cases):
    got = dump(cases)
    bad = [(c, e, g) for c, e, g in zip(cases, map(expected, cases), got) if e != g]
    if bad:
        c, e, g = bad[0]
        diff = {k: (e[k], g[k]) for k in OUTPUTS if e[k] != g[k]}
        pytest.fail(f"{len(bad)} of {len(cases)} plans differ; first: {({k: c[k] for k in INPUTS if c[k] != BASE[k]})} (expected, got) {diff}")
    return got


def test_boundary_rows(dump):
    cases = boundary_cases()
    got = _compare(dump, cases)
    # the rows are what they are meant to be: both sides of each boundary are reached
    by = lambda **kw: got[cases.index(case(**kw))]
    assert by()["frame"] == TWO and by()["lean"] == 1 and by()["grid_x"] == 1024 and by()["leaf_thr"] == 12 | 5 << 8 | 2 << 12 | 6 << 16 | 8 << 24
    assert by()["min_traversing1"] == 24 | 256 and by()["min_traversing"] == 24 and by()["lds"] == 16384
    assert (by(ns=8)["frame"], by(ns=7)["frame"], by(mesh_split=4, ns=16)["frame"], by(mesh_split=4, ns=15)["frame"]) == (TWO, SINGLE, TWO, SINGLE)
    assert (by(nx=65535, rows=8)["frame"], by(nx=65536, rows=8)["frame"], by(nx=8, rows=65535)["frame"], by(nx=8, rows=65536)["frame"]) == (TWO, SINGLE, TWO, SINGLE)
    assert (by(first_leaf=LEAF_CNT_LDS)["lds"], by(first_leaf=LEAF_CNT_LDS + 1)["lds"]) == (LEAF_CNT_LDS, 0)
    assert (by(first_leaf=LEAF_CNT_LDS)["lean"], by(first_leaf=LEAF_CNT_LDS + 1)["lean"]) == (1, 0)
    assert (by(nppl=16)["leaf_thr1"], by(nppl=17)["leaf_thr1"], by(nppl=16)["lean"], by(nppl=17)["lean"]) == (4, 16, 1, 0)
    assert (by(nx=8, rows=8)["stride"], by(nx=16, rows=8)["stride"]) == (1, coprime_stride(128))
    assert by(nx=64, rows=8)["min_traversing1"] == 24 and by(nx=72, rows=8)["min_traversing1"] == 24 | 256 and by(nx=72, rows=8)["stride1"] == coprime_stride(72)
    assert (by(nx=96, rows=64)["grid_x"], by(nx=48, rows=60)["grid_x"], by(nx=96, rows=64, variant=variant(wgs=8))["grid_x"]) == (24, 12, 24)
    assert (by(cus=256)["grid_x"], by(cus=1)["grid_x"], by(cus=304)["grid_x"]) == (1024, 4, 1216)
    assert by(leaf_ofs=0)["lds"] == 0 and by(leaf_tri=0)["lds"] == 16384 and by(leaf_tri=0)["lean"] == 0          # (the LDS size tests leaf_ofs alone)
    assert by(queue=0)["error"] == NO_QUEUE and by(variant=variant(kernel=1), queue=0)["error"] == 0
    assert by(variant=variant(kernel=1))["frame"] == TILES and (by(variant=variant(kernel=1))["grid_x"], by(variant=variant(kernel=1))["grid_y"]) == (60, 135)
    assert (by()["xcd_queues"], by(mesh_rev=1)["xcd_queues"], by(mesh_two=0)["xcd_queues"]) == (8, 0, 0)
    assert by(mesh_rev=1)["stride"] == 0xFFFFFFFF and by(mesh_rev=1, mesh_two=0)["stride"] == coprime_stride(240 * 135 * 64)
    assert by(acc_first=8)["frame"] == SINGLE and by(ord_rec=0, order=1, ord_state=1, ord_rays=1)["frame"] == TWO and by(ord_rec=0, order=0)["frame"] == SINGLE


def test_seeded_sweep(dump):
    cases = sweep_cases()
    got = _compare(dump, cases)
    # the sweep reaches every kind of frame, the error, and every instantiation the launcher can name
    assert {g["frame"] for g in got} == {TILES, TWO, SINGLE} and {g["error"] for g in got} == {0, NO_QUEUE}
    forms = {(g["frame"], g["trav"], g["dbg"], g["stats"], g["lean"]) for g in got if g["frame"] != TILES and not g["error"]}
    assert forms == {(TWO, 0, 0, 0, 1), (TWO, 0, 0, 0, 0), (SINGLE, 0, 0, 0, 1), (SINGLE, 0, 0, 0, 0), (SINGLE, 0, 1, 0, 0), (SINGLE, 0, 0, 1, 0),
                     (SINGLE, 1, 0, 0, 0), (SINGLE, 1, 1, 0, 0), (SINGLE, 1, 0, 1, 0)}
    assert sum(g["frame"] == TWO for g in got) > 400 and sum(g["min_traversing1"] >> 8 for g in got) > 100 and sum(g["stride"] == 0xFFFFFFFF for g in got) > 40
