"""CPU: the bounce's divisions by a special divisor (csrc/rt_exactdiv.h) against the plain float division they replace, bit for bit.  Form B divides the roots
of sphereHit by a = dot(dn, dn), one of seven floats next to 1, in one fused multiply-add; form C divides the three components of a vector by one divisor
with the reciprocal refined once - the compiler's own division sequence where it neither scales nor fixes up.  tests/exactdiv_dump.cpp includes the header,
is compiled as plain C++ with -ffp-contract=off (no kernel, no HIP call) and holds both against `x / d`.  Every operand the header handles without the plain
path must have ZERO mismatches inside its guard: a condition, not a tolerance.  The exhaustive modes are run by hand and recorded in DESIGN 3.21 and
profiles/exactdiv_host_exhaustive.txt (all 2^32 numerators per a; every mantissa in both signs over 1505 divisors - the tool takes the count as an argument);
what runs here is the reduced set."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")

ONE = 0x3F800000
# k = bits(a) - bits(1.0f) -> the multiplier r with fmaf(x, r, x) == x / a for every x (the enumerated words)
R_OF_K = {-4: 0x34800002, -3: 0x34400003, -2: 0x34000001, -1: 0x33800001, 0: 0, 1: 0xB3FFFFFE, 2: 0xB47FFFFC}


def build_dump(directory, *extra):
    exe = os.path.join(str(directory), "exactdiv_dump")
    r = subprocess.run([os.environ.get("HIPCC", "hipcc"), "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", *extra, "-I", CSRC,
                        os.path.join(ROOT, "tests", "exactdiv_dump.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = build_dump(tmp_path_factory.mktemp("exactdiv"))
    return lambda *args: subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_the_computed_r_is_the_enumerated_word_and_the_neighbours_are_not_handled(dump):
    rows = {int(f[0]): f[1:] for f in (line.split() for line in dump("--words"))}
    assert sorted(rows) == list(range(-6, 5))
    for k, (a, handled, r) in rows.items():
        assert int(a, 16) == ONE + k
        assert int(handled) == (1 if k in R_OF_K else 0), k                  # k = -5 and k = 3 have no single r: not silently mapped
        if k in R_OF_K:
            assert int(r, 16) == R_OF_K[k], (k, r)
    text = open(os.path.join(CSRC, "rt_exactdiv.h")).read()
    for w in R_OF_K.values():
        assert w == 0 or f"{w:#010x}" in text, hex(w)


def test_form_b_every_mantissa_of_the_binades_that_matter_per_a(dump):
    lines = dump("--quot-a")
    assert len(lines) == len(R_OF_K)
    for line in lines:
        f = line.split()
        k, r = int(f[0]), dict(zip(f[1::2], f[2::2]))
        assert int(r["a"], 16) == ONE + k and int(r["r"], 16) == R_OF_K[k]
        # every mantissa of the denormals and of the two binades around 1, the ends of the lowest and the highest binade, both signs, the special values
        assert int(r["checked"]) == 3 * 2 * 2 ** 23 + 2 * 2 * 2 * 4096 + 7
        assert int(r["bad"]) == 0, line
        # the two exceptions the header names: -0 becomes +0 for r < 0, an infinite x gives NaN for r <= 0 (inf - inf, inf * 0)
        assert int(r["zero_sign"]) == (1 if k > 0 else 0) and int(r["inf_nan"]) == (2 if k >= 0 else 0), line


def test_the_handled_a_are_the_ones_bounce_directions_have(dump):
    lines = dump("--ahist", 400_000, 20261019)
    hist = {int(f[0]): int(f[1]) for f in (line.split() for line in lines[:-1])}
    assert lines[-1].split() == ["other", "0"]
    assert set(hist) <= set(R_OF_K), hist                                     # nothing outside the seven
    assert hist[0] + hist[1] > 0.9 * 400_000                                  # and almost all of it at k = 0 and 1


def test_form_c_shared_reciprocal_seeded_with_the_rounded_one(dump):
    lines = dump("--shared", 160, 61)
    assert len(lines) == 6
    for line in lines[:5]:                                                    # the benchmark's radii (0.2, 1, 1000) and 0.5 in both signs: every mantissa
        f = line.split()
        assert int(f[3]) == 2 * 2 ** 23 and int(f[5]) == 0, line              # a binade of x in both signs, the seed RN(1 / l)
    f = lines[5].split()
    assert int(f[1]) == 165 and int(f[5]) > 160 * 2 * (2 ** 23 // 61) and int(f[7]) == 0, lines[5]
    print("for the record - mismatches with the neighbouring seeds: within 1 ulp of 1 / l", f[9], "up to 1.5 ulp", f[11])


def test_the_guards_from_both_sides_of_each_edge(dump):
    lines = dump("--window")
    div3 = [line.split() for line in lines if line.startswith("div3")]
    unit = [line.split() for line in lines if line.startswith("unit")]
    # (x, y, z, l): inside at the window's own ends (2^-40 and 2^40, quotients of 2^-80 and 2^78); outside one ulp beyond either end in any operand, for a
    # zero of either sign, a NaN or an infinity in any operand, and for a negative divisor
    assert [int(f[6]) for f in div3] == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert all(int(f[8]) == 0 for f in div3), div3
    # unit(v): s2 in [2^-60, 2^60] and the least square >= 2^-80, each from both sides; zero, NaN and inf components outside
    assert [int(f[5]) for f in unit] == [1, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    assert all(int(f[9]) == 0 for f in unit), unit
    assert all(int(f[7]) == 1 for f in unit if int(f[5])), unit               # the unit guard implies the general one


def test_whole_vectors_against_plain_unit(dump):
    (line,) = dump("--vectors", 1_000_000, 20261019)
    f = line.split()
    assert int(f[1]) == 1_000_000 and int(f[5]) == 0, line
    assert int(f[3]) == 0, line                                              # the plain path is not taken on the path's own directions


def test_the_dump_runs_clean_under_the_host_sanitizers(tmp_path):
    exe = build_dump(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for args in (["--words"], ["--window"], ["--vectors", "20000", "7"], ["--ahist", "20000", "7"]):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stderr[-2000:])


def test_the_header_is_free_of_hip_and_only_the_parity_objects_use_it():
    code = lambda name: re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
    hdr = code("rt_exactdiv.h")
    assert re.findall(r"hip[A-Z]\w*\(", hdr) == [] and "__global__" not in hdr and "__device__" not in hdr
    assert re.findall(r"#include\s*[<\"]([^>\"]*)[>\"]", hdr) == ["stdint.h"]
    assert "sqrt" not in hdr and " / " not in hdr                            # no square root and no division in it
    dev = code("rt_device.h")
    guard = dev[:dev.index('#include "rt_exactdiv.h"')]
    assert guard.rstrip().splitlines()[-2].strip() == "#ifdef RT_MODE_PARITY"
    assert "rt_exactdiv.h" in open(os.path.join(ROOT, "Makefile")).read()
