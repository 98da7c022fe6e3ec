"""CPU: the exact re-normalisation of unit directions (csrc/rt_renorm.h) against the plain float operators it replaces, bit for bit.  hit() normalises a
direction that is unit already; the header returns the bits of that second unit_vector from a class of s2 and one fused multiply-add per component, and sends
every other input down the plain path.  tests/renorm_dump.cpp includes the header, is compiled as plain C++ with -ffp-contract=off (no kernel, no HIP call)
and holds it against `x / l2` and `a / sqrtf(s2)`: per divisor over every mantissa, the map from s2 to the divisor, and whole vectors."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")

ONE = 0x3F800000
# the divisor of each class: 1 - 3 eps, 1 - 2 eps, 1 - eps, 1, 1 + 2 eps (eps = 2^-24), its t and the multiplier r of the header's argument
L2 = [ONE - 3, ONE - 2, ONE - 1, ONE, ONE + 1]
T = [-3, -2, -1, 0, 2]
R = [0x34400003, 0x34000001, 0x33800001, 0, 0xB3FFFFFE]
# k = bits(s2) - bits(1.0f) -> class
CLASS_OF_K = {-6: 0, -5: 0, -4: 1, -3: 1, -2: 2, -1: 2, 0: 3, 1: 3, 2: 4, 3: 4}
# bits(x / l2) - bits(x) over the mantissas of one binade, as runs (first mantissa, d): what the quotient does to the bits (the header quotes it)
RUNS = [[(0, 2), (0x555553, 3), (0x7FFFFF, 2)], [(0, 1), (0x3FFFFF, 2)], [(0, 1)], [(0, 0)], [(0, -2), (1, -1), (0x400002, -2)]]


def build_dump(directory):
    exe = os.path.join(str(directory), "renorm_dump")
    r = subprocess.run([os.environ.get("HIPCC", "hipcc"), "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "renorm_dump.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = build_dump(tmp_path_factory.mktemp("renorm"))
    return lambda *args: subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_every_handled_s2_has_its_class_divisor_and_the_neighbours_have_none(dump):
    rows = {int(f[0]): f[1:] for f in (line.split() for line in dump("--classes"))}
    assert sorted(rows) == list(range(-9, 7))
    for k, row in rows.items():
        s2, root, cls = int(row[0], 16), int(row[1], 16), int(row[2])
        assert s2 == ONE + k
        if k in CLASS_OF_K:
            t, l2, r = int(row[3]), int(row[4], 16), int(row[5], 16)
            assert cls == CLASS_OF_K[k] and t == T[cls] and l2 == L2[cls] == root and r == R[cls], (k, row)      # sqrtf(s2) is the class's divisor
        else:
            assert cls == len(L2) and len(row) == 3, (k, row)                                                     # not silently mapped
    # the nearest unhandled s2 on either side really has another square root
    assert int(rows[-7][1], 16) == ONE - 4 and int(rows[4][1], 16) == ONE + 2


def test_the_bit_patterns_the_header_quotes_are_the_enumerated_ones(dump):
    got = []
    for line in dump("--runs"):
        f = line.split()
        got.append([(int(m, 16), int(d)) for m, d in zip(f[1::2], f[2::2])])
    assert got == RUNS
    text = open(os.path.join(CSRC, "rt_renorm.h")).read()
    for m in (0x555553, 0x3FFFFF, 0x400001, 0x7FFFFF, *R[:3], R[4]):
        assert f"{m:#x}" in text, hex(m)


def test_every_mantissa_per_divisor_against_the_plain_division(dump):
    lines = dump("--components")
    assert len(lines) == len(L2)
    for cls, line in enumerate(lines):
        f = line.split()
        assert int(f[0]) == cls and int(f[1], 16) == L2[cls]
        r = dict(zip(f[2::2], f[3::2]))
        assert int(r["r"], 16) == R[cls]
        # five whole binades (three around 1, the two lowest) and the denormals in both signs, and 601 patterns at each of five thresholds in every binade
        assert int(r["checked"]) >= 2 * (6 * 2 ** 23 - 1) and int(r["bad"]) == 0, line
        # the quotient keeps the sign of a zero; the multiply-add does too unless r < 0: why a vector with a zero component takes the plain path
        assert int(r["zero_quotient"]) == 1 and int(r["zero_fma"]) == (0 if cls == 4 else 1), line


def test_whole_vectors_against_plain_unit(dump):
    (line,) = dump("--vectors", 2_000_000, 20261019)
    f = line.split()
    r = dict(zip(f[0:8:2], f[1:8:2]))
    assert int(r["unit"]) == 2_000_000 and int(r["edges"]) > 1000
    assert int(r["bad"]) == 0, line
    assert int(r["plain_unit"]) * 5000 < int(r["unit"]), line                    # the plain path is rare on the path's own directions
    hist = [int(h) for h in f[f.index("hist") + 1:]]
    assert len(hist) == len(L2) + 1 and all(h > 0 for h in hist[:len(L2)]), hist     # every class occurs among them


def test_the_header_is_free_of_hip_and_only_the_parity_objects_use_it():
    code = lambda name: re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
    hdr = code("rt_renorm.h")
    assert re.findall(r"hip[A-Z]\w*\(", hdr) == [] and "__global__" not in hdr and "__device__" not in hdr
    assert re.findall(r"#include\s*[<\"]([^>\"]*)[>\"]", hdr) == ["stdint.h"]
    assert "sqrt" not in hdr[:hdr.index("rt_renorm_plain")]                                 # no square root on the exact path
    dev = code("rt_device.h")
    guard = dev[:dev.index('#include "rt_renorm.h"')]
    assert guard.rstrip().splitlines()[-2].strip() == "#ifdef RT_MODE_PARITY"
    assert "renorm_unit(L.dir, has_ray)" in code("rt_kernels_spheres.hip")
    assert "r.d = renorm_unit(dir);" in dev[dev.index("Ray make_ray("):]
