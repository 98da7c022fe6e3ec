"""The mesh launcher's switches that no other GPU test sets, each a branch of its plan (plan_mesh, csrc/rt_mesh_plan.h): the staircase at detail 1, 96 x 64,
16 spp, NEE + RR, depth 24, counters off, rendered through the C-ABI.  Each case must report exactly the launch records named (rtLastLaunches) and give the
oracle's bits - the work order, the instantiation and the grid change, the frame does not.  (What the plan makes of the switches' values: tests/test_mesh_plan.py.)"""
import numpy as np
import pytest

import kernel_forms as K

pytestmark = pytest.mark.gpu

FORM = dict(name="mesh_switches", scene=("staircase", False), ns=16)

# (id, environment, variant, expected records)
CASES = [
    ("two_off", {"RT_MESH_TWO": "0"}, 0, K.mesh_one(True)),
    ("lean_off", {"RT_MESH_LEAN": "0"}, 0, K.mesh_two(False)),
    ("tile_order", {"RT_MESH_ORDER": "t"}, 0, K.mesh_two(True)),
    ("cheapest_first", {"RT_MESH_REV": "1"}, 0, K.mesh_two(True)),
    ("no_heavy_classes", {"RT_MESH_HEAVY": "0"}, 0, K.mesh_two(True)),
    ("no_spread_rounds", {"RT_MESH_ROUNDS": "0"}, 0, K.mesh_two(True)),
    ("split_4", {"RT_MESH_SPLIT": "4"}, 0, K.mesh_two(True)),                   # 16 = 4 x 4: still two dispatches
    ("split_5", {"RT_MESH_SPLIT": "5"}, 0, K.mesh_one(True)),
    ("eight_wgs_per_cu", {}, 8 << 8, K.mesh_two(True)),                         # the pixels clip the grid: 24 workgroups
]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def oracle_frame(rt, O):
    ref = K.render_oracle(rt, O, FORM)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("env,variant,records", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_switch_takes_its_branch_and_keeps_the_bits(rt, oracle_frame, env, variant, records, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, recs = K.render_form(rt, dict(FORM, opts={"variant": variant}))
    assert [r[:len(K.RECORD_FIELDS)] for r in recs] == records, recs
    assert all(r[len(K.RECORD_FIELDS):] == (0, 0) for r in recs), recs          # device 0, RT_FP_PARITY
    assert all(r[-1] == 24 for r in records)                                    # 96 x 64 pixels in workgroups of 256
    assert not np.isnan(got).any()
    assert np.array_equal(_bits(got), _bits(oracle_frame)), np.count_nonzero(_bits(got) != _bits(oracle_frame))
