"""Every production instantiation of the render kernels, pinned: each form of tests/kernel_forms.py is rendered through the C-ABI WITHOUT counters (the
counting instantiation is the general diagnostic kernel, so a counters-on test never reaches a lean kind), the launch report (rtLastLaunches) must
name exactly the instantiations the table expects, and the frame must be the oracle's bit for bit (the sample chunks of the counter stream: the
tolerance of test_counter_rng_sample_chunks).  The same scene with counters on must give the same bits: the production kernel and the diagnostic one
are held to each other as well as to the oracle."""
import numpy as np
import pytest

import kernel_forms as K

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_frame(form, got, ref):
    assert not np.isnan(got).any(), form["name"]
    if form.get("tol"):                  # chunk sums added in chunk order: 2e-6 relative + 1e-7 absolute per channel
        assert np.all(np.abs(got - ref) <= 2e-6 * np.abs(ref) + 1e-7), form["name"]
    else:
        assert np.array_equal(_bits(got), _bits(ref)), (form["name"], np.count_nonzero(_bits(got) != _bits(ref)))


def _check_records(form, recs):
    assert [r[:len(K.RECORD_FIELDS)] for r in recs] == form["records"], (form["name"], recs)
    assert all(r[len(K.RECORD_FIELDS):] == (0, 0) for r in recs), recs        # device 0, RT_FP_PARITY


@pytest.mark.parametrize("form", K.FORMS, ids=lambda f: f["name"])
def test_production_form_is_launched_and_matches_the_oracle(rt, O, form, monkeypatch):
    for k, v in form.get("env", {}).items():
        monkeypatch.setenv(k, v)
    ref = K.render_oracle(rt, O, form)
    got, recs = K.render_form(rt, form)
    _check_records(form, recs)
    _check_frame(form, got, ref)
    counted, crecs = K.render_form(rt, form, counters=1)
    assert crecs and all(r[4] != 0 for r in crecs), crecs                     # (the counting instantiation ran)
    assert np.array_equal(_bits(counted), _bits(got)), (form["name"], np.count_nonzero(_bits(counted) != _bits(got)))


@pytest.mark.parametrize("lanes", [1, 6])
def test_mesh_chain_set_up_on_a_frame_of_few_workgroups(rt, O, lanes, monkeypatch):
    """A 48x60 mesh frame launches 12 workgroups of 4 waves.  With one set of lists per XCD each queue is served first by max(12 / 8, 1) = 1 workgroup,
    i.e. by no eighth of a wave: max_waves = 0.  With the list-0 threshold at its floor (RT_MESH_CHAIN_THR=17: every pixel that spent more than about
    one ray per sample in its first two samples - every pixel that hit the staircase) and the "few pixels only" guard off (RT_MESH_CHAIN_FRAC=0),
    list 0 of every queue that holds such a pixel is not empty, so the chain set-up of the second dispatch runs with max_waves = 0.  It divided by
    max_waves there; now it takes no chain waves (as the cap after the division made of it).  Two dispatches, lean kernel, NEE + RR: the oracle's bits."""
    for k, v in (("RT_XCD_QUEUES", "1"), ("RT_MESH_CHAIN_THR", "17"), ("RT_MESH_CHAIN_FRAC", "0"), ("RT_MESH_CHAIN_LANES", str(lanes))):
        monkeypatch.setenv(k, v)
    nx, ny = 48, 60
    form = dict(name="mesh_small", scene=("staircase", False), ns=8)
    ref = K.render_oracle(rt, O, form, nx, ny)
    got, recs = K.render_form(rt, form, nx=nx, ny=ny)
    assert [r[:len(K.RECORD_FIELDS)] for r in recs] == [(K.FAMILY_MESH_QUEUE, phase, 0, 0, 0, 0, 1, K.MESH_THREADS, 12) for phase in (1, 2)], recs
    assert not np.isnan(got).any()
    assert np.array_equal(_bits(got), _bits(ref)), np.count_nonzero(_bits(got) != _bits(ref))
