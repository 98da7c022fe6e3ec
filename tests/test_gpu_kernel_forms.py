"""Every production instantiation of the render kernels, pinned: each form of tests/kernel_forms.py is rendered through the C-ABI WITHOUT counters (the
counting instantiation is the general diagnostic kernel, so a counters-on test never reaches a lean kind), the launch report (rtLastLaunches) must
name exactly the instantiations the table expects, and the frame must be the oracle's bit for bit (the sample chunks of the counter stream: the
tolerance of test_counter_rng_sample_chunks).  The same scene with counters on must give the same bits: the production kernel and the diagnostic one
are held to each other as well as to the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_forms as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.mark.parametrize("form", [f for f in K.FORMS if not f.get("child")], ids=lambda f: f["name"])
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


def test_six_wave_forms_in_a_fresh_process(rt, O, tmp_path):
    """The six-wave kinds (7, 15 and the chunked 7) are chosen from RT_LEAN6_PIXELS pixels on, a threshold the launcher reads once per process (a
    function static): one child process renders them all with the threshold at 1 pixel and writes frames and launch records; the oracle runs here."""
    forms = [f for f in K.FORMS if f.get("child")]
    env = dict(os.environ)
    for f in forms:
        env.update(f["env"])
    code = ("import sys, json, numpy as np; sys.path[:0] = [%r, %r]; import cuda_raytracing_optimized_amd as rt, kernel_forms as K; out = {}\n"
            "for f in [f for f in K.FORMS if f.get('child')]:\n"
            "    for c in (0, 1):\n"
            "        got, recs = K.render_form(rt, f, counters=c); np.save(%r + '/' + f['name'] + '_%%d.npy' %% c, got); out[f['name'] + '_%%d' %% c] = recs\n"
            "json.dump(out, open(%r, 'w'))\n") % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path), str(tmp_path / "records.json"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    records = json.load(open(tmp_path / "records.json"))
    for f in forms:
        ref = K.render_oracle(rt, O, f)
        got = np.load(tmp_path / (f["name"] + "_0.npy"))
        _check_records(f, [tuple(x) for x in records[f["name"] + "_0"]])
        _check_frame(f, got, ref)
        counted = np.load(tmp_path / (f["name"] + "_1.npy"))
        assert all(x[4] != 0 for x in records[f["name"] + "_1"])
        assert np.array_equal(_bits(counted), _bits(got)), f["name"]


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
