"""CPU tripwire: the library's environment switches are read in one place (rt_read_switches, rt_renderer.hip) by one rule (once per frame or
progressive pass).  Every getenv of the sources lies in that reader or in a parsing helper that only it calls, no static variable
caches the environment (a cached switch makes an in-process test of it silently test the default), and the switches read are the ones INTEGRATION.md
§5 documents."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")
READER = "rt_read_switches"
# a function definition at column 0: return type, name, parameters, the opening brace
FUNC = re.compile(r"^[A-Za-z_][\w:<>,*& ]*?\b(\w+)\s*\([^;{}]*\)\s*(?:const\s*)?\{", re.M)


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert paths
    return {os.path.basename(p): re.sub(r"//[^\n]*", "", open(p).read()) for p in paths}


def _functions(src):
    """(name, start, end) of every function defined at column 0 (the body ends at the next '}' at column 0)."""
    out = []
    for m in FUNC.finditer(src):
        end = src.find("\n}", m.end())
        out.append((m.group(1), m.start(), len(src) if end < 0 else end))
    return out


def _enclosing(funcs, pos):
    inside = [f for f in funcs if f[1] <= pos < f[2]]
    return inside[-1][0] if inside else None


def _reader_body(srcs):
    bodies = [src[s:e] for src in srcs.values() for name, s, e in _functions(src) if name == READER]
    assert len(bodies) == 1, f"{READER} is defined {len(bodies)} times"
    return bodies[0]


def _env_helpers(srcs):
    """The functions other than the reader that call getenv (each must be a parsing helper of the reader)."""
    helpers = set()
    for fname, src in srcs.items():
        funcs = _functions(src)
        for m in re.finditer(r"\bgetenv\s*\(", src):
            where = _enclosing(funcs, m.start())
            assert where is not None, f"{fname}: getenv outside a function, offset {m.start()}"
            if where != READER:
                helpers.add(where)
    return helpers


def test_getenv_only_in_the_reader_and_its_helpers():
    srcs = _sources()
    helpers = _env_helpers(srcs)
    reader = _reader_body(srcs)
    assert re.search(r"\b(%s)\s*\(" % "|".join(helpers | {"getenv"}), reader), f"{READER} reads nothing"
    for h in helpers:
        # a function outside the reader that reads the environment is one of its parsing helpers: called there ...
        assert re.search(r"\b%s\s*\(" % h, reader), f"{h} reads the environment, but {READER} does not call it"
        # ... and nowhere else
        for fname, src in srcs.items():
            funcs = _functions(src)
            for m in re.finditer(r"\b%s\s*\(" % h, src):
                if any(name == h and s == src.rfind("\n", 0, m.start()) + 1 for name, s, _ in funcs):
                    continue                                        # (its own definition)
                assert _enclosing(funcs, m.start()) == READER, f"{fname}: {h}, which reads the environment, is called outside {READER}"


def test_no_static_caches_the_environment():
    srcs = _sources()
    readers = {"getenv", READER} | _env_helpers(srcs)
    for fname, src in srcs.items():
        for m in re.finditer(r"\bstatic\b[^;{}()]*=[^;]*;", src):
            stmt = m.group(0)
            assert not re.search(r"\b(%s)\s*\(" % "|".join(readers), stmt), f"{fname}: {stmt}"
            assert not re.search(r"\bsw\s*\.", stmt), f"{fname}: a static copy of a switch: {stmt}"
        assert not re.search(r"\bstatic\s+(const\s+)?RtSwitches\b", src), f"{fname}: a static RtSwitches"


def _documented_switches():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    i = doc.index("\n## 5.")
    j = doc.find("\n## ", i + 1)
    names = set()
    for line in doc[i:j if j > 0 else len(doc)].splitlines():
        if line.startswith("| `"):
            names |= set(re.findall(r"\bRT_[A-Z0-9_]+", line.split("|")[1]))
    return {n for n in names if not n.startswith("RT_BENCH_")}


def test_switches_read_are_the_documented_ones():
    read = re.findall(r'"(RT_[A-Z0-9_]+)"', _reader_body(_sources()))
    assert len(read) == len(set(read)), sorted(n for n in set(read) if read.count(n) > 1)
    documented = _documented_switches()
    assert set(read) - documented == set(), f"read by {READER}, not in INTEGRATION.md §5: {sorted(set(read) - documented)}"
    assert documented - set(read) == set(), f"in INTEGRATION.md §5, not read by {READER}: {sorted(documented - set(read))}"
