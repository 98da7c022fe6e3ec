"""CPU: the hit normal's division by a stored reciprocal (csrc/rt_exactdiv.h: rt_exdiv_stored, rt_exdiv3_y, rt_exdiv3_window_y) against the plain float
division, bit for bit.  tests/exactdiv_stored_dump.cpp includes the header, is compiled as plain C++ with -ffp-contract=off and enumerates the cases of
`exactdiv_dump --shared` (tests/test_exactdiv.py) again - the benchmark's radii over every mantissa of a binade, 160 divisors spread through the window,
the seed RN(1 / l) held and its neighbours counted - with the reciprocal computed once per divisor and handed on as a word.  ZERO mismatches inside the
guard: a condition, not a tolerance.  The device, whose seed is v_rcp_f32's, is held by the probe (tests/test_gpu_ray_step_loads.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")


def build_dump(directory, *extra):
    exe = os.path.join(str(directory), "exactdiv_stored_dump")
    r = subprocess.run([os.environ.get("HIPCC", "hipcc"), "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I", CSRC,
                        os.path.join(ROOT, "tests", "exactdiv_stored_dump.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = build_dump(tmp_path_factory.mktemp("exactdiv_stored"))
    return lambda *args: subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.splitlines()


def _fields(line):
    f = line.split()
    return dict(zip(f[0::2], f[1::2]))


def test_stored_reciprocal_on_the_cases_of_the_shared_check(dump):
    lines = dump("--shared", 160, 61)
    assert len(lines) == 5
    for line in lines[:4]:                                                    # the benchmark's radii (0.2, 1, 1000) and 0.5: every mantissa
        r = _fields(line)
        assert int(r["checked"]) == 2 * 2 ** 23 and int(r["bad"]) == 0 and int(r["guard_bad"]) == 0, line
    r = _fields(lines[4])
    assert int(r["divisors"]) == 164 and int(r["checked"]) > 160 * 2 * (2 ** 23 // 61) and int(r["bad"]) == 0 and int(r["guard_bad"]) == 0, lines[4]
    print("for the record - mismatches with the neighbouring seeds: within 1 ulp of 1 / l", r["near_bad"], "up to 1.5 ulp", r["far_bad"])


def test_the_marker_is_stored_exactly_outside_the_window(dump):
    rows = [_fields(line) for line in dump("--marker")]
    # 2^-40, one ulp below, one above, 2^40, one below, one above, +-0, -0.5, +-inf, NaN, a denormal, 2^45, 2^-45, 0.2
    assert [int(r["in"]) for r in rows] == [1, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    for r in rows:
        assert int(r["marker"]) == 1 - int(r["in"]) and int(r["guard_bad"]) == 0 and int(r["bad"]) == 0, r


def test_the_dump_runs_clean_under_the_host_sanitizers(tmp_path):
    exe = build_dump(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    r = subprocess.run([exe, "--marker"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
