"""CPU: the rule by which the sphere launcher takes the folded form of its cost-ordered dispatch (sphere_frame_form, csrc/rt_sphere_form.h) against the rule
restated here, over EVERY combination of its inputs.  The folded kernel has no code for a frame outside the rule - one queue for the machine, parked state in
three arrays, a middle tier, rows of the host framebuffer - so a hole in the rule would render a wrong frame or write out of bounds; and a rule that is too
narrow only costs speed, which no render test sees.  tests/sphere_form_dump.cpp includes the header, is compiled as plain C++ (no kernel, no HIP call) and
runs the rule on the cases fed to it."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")

INPUTS = "frame kind_folded default_constants xcd_queues ord_rec mid_waves tune fb_global_rows poison_fb counters wave_dbg".split()
GENERAL, DEFAULT = 0, 1
TILES, GLOBAL_SINGLE, TWO, TWO_RESUME, ORDERED_SINGLE, CLASSIFIED_SINGLE, PLAIN_SINGLE = range(7)      # SphereFrame
XCD_QUEUES = 8                                                                                         # kXcdQueues (rt_params.h)
VALUES = dict(frame=range(7), kind_folded=(0, 1), default_constants=(0, 1), xcd_queues=(XCD_QUEUES, 0, 1), ord_rec=(1, 0), mid_waves=(0, 1, 2, 12), tune=(0, 1), fb_global_rows=(0, 1),
              poison_fb=(0, 1), counters=(0, 1), wave_dbg=(0, 1))
assert list(VALUES) == INPUTS


def expected(c):
    """The rule of the issue, restated: a frame with a cost-ordered dispatch, an instantiation that is built folded, the scheduling words it is compiled with,
    and every switch at its default."""
    ok = (c["frame"] in (TWO, TWO_RESUME, ORDERED_SINGLE) and c["kind_folded"] and c["default_constants"] and c["xcd_queues"] == XCD_QUEUES and c["ord_rec"] and c["mid_waves"] == 0 and
          not c["tune"] and not c["fb_global_rows"] and not c["poison_fb"] and not c["counters"] and not c["wave_dbg"])
    return DEFAULT if ok else GENERAL


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/sphere_form_dump.cpp, compiled as plain C++ against the header; returns run(cases) -> list of forms."""
    exe = str(tmp_path_factory.mktemp("sphere_form") / "sphere_form_dump")
    r = subprocess.run([os.environ.get("HIPCC", "hipcc"), "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "sphere_form_dump.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    fields = subprocess.run([exe, "--fields"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert [f.split() for f in fields] == [INPUTS, [str(GENERAL), str(DEFAULT)], [str(k) for k in range(7)]]

    def run(cases):
        text = "".join(" ".join(str(c[k]) for k in INPUTS) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-1000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        return [int(line) for line in lines]
    return run


def test_every_combination_of_the_inputs(dump):
    cases = [dict(zip(INPUTS, combo)) for combo in itertools.product(*(VALUES[k] for k in INPUTS))]
    got = dump(cases)
    bad = [(c, expected(c), g) for c, g in zip(cases, got) if expected(c) != g]
    assert bad == [], (len(bad), bad[:3])
    # the table is what it is meant to be: the folded form is reached, by exactly the three frames that have the dispatch and one value of everything else
    assert sorted(c["frame"] for c, g in zip(cases, got) if g == DEFAULT) == [TWO, TWO_RESUME, ORDERED_SINGLE]
    assert len(cases) == 7 * 2 * 2 * 3 * 2 * 4 * 2 ** 5


def test_the_header_is_free_of_hip_and_the_launcher_uses_it():
    code = lambda name: re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
    hdr = code("rt_sphere_form.h")
    assert re.findall(r"hip[A-Z]\w*\(", hdr) == [] and "__global__" not in hdr
    assert re.findall(r"#include\s*[<\"]([^>\"]*)[>\"]", hdr) == ["rt_params.h"]           # the parameter blocks, nothing of the kernels
    src = code("rt_kernels_spheres.hip")
    assert len(re.findall(r"\bsphere_frame_form\(", src)) == 1                              # one decision per plan
    plan = src[src.index("static SpherePlan plan_spheres("):]
    assert "sphere_frame_form(" in plan[:plan.index("\n}")]
