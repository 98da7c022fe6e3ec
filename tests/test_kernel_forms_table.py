"""CPU tripwire: the table of production forms (tests/kernel_forms.py, rendered by test_gpu_kernel_forms.py) against the launch sites in the kernel
sources.  Every instantiation a launcher can launch without diagnostics must have a row, and every row must name an instantiation that is still
launched: a new kind in the lists of rt_kernels_spheres.hip (KindsFull, KindsChunked, KindsHybrid) without a test, or a deleted one with a stale row,
fails here without a GPU.  The sphere launcher's shape is held too: a plan without HIP calls, one place that sets the LDS attribute, one statement of the kinds;
and the mesh launcher's: a plan without HIP calls in a header of its own, one function that names the kernel, the packed arguments read by their fields' names."""
import os
import re

import kernel_forms as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc")
SQ, ST, MQ, MT = K.FAMILY_SPHERE_QUEUE, K.FAMILY_SPHERE_TILES, K.FAMILY_MESH_QUEUE, K.FAMILY_MESH_TILES


def _code(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def _bool(tok):
    return {"true": 1, "false": 0}[tok]


def _function(src, signature):
    """The body of the function whose definition starts with `signature` (up to the next definition at column 0)."""
    i = src.index(signature)
    j = src.find("\n}", i)
    return src[i:j]


KIND_LISTS = {"KindsFull": (0, 0), "KindsChunked": (0, 1), "KindsHybrid": (2, 0)}     # list -> (scene, chunked) of its instantiations


def sphere_kind_lists(src):
    """The LEAN kinds the source declares: {list name: [kinds]} of every `using Kinds... = std::integer_sequence<int, ...>`."""
    return {name: [int(v) for v in kinds.split(",")] for name, kinds in re.findall(r"using\s+(Kinds\w+)\s*=\s*std::integer_sequence<int,([^>]*)>;", src)}


def sphere_source_forms():
    """(scene, chunked, lean) of every non-diagnostic k_render_spheres_queue launch, (phase, cls, chunked) of the launcher's calls, tile kernels."""
    src = _code("rt_kernels_spheres.hip")
    lists = sphere_kind_lists(src)
    assert set(lists) == set(KIND_LISTS) | {"KindsStamped"}, sorted(lists)           # (KindsStamped: diagnostic instantiations)
    form_fn = _function(src, "static hipError_t launch_queue_form(")
    forms = set()
    for name, (scene, chunked) in KIND_LISTS.items():
        # the list is expanded into non-diagnostic instantiations of its own scene form and chunking, and of nothing else
        sites = re.findall(r"launch_kind_of<PHASE,\s*CLS,\s*(true|false),\s*(true|false),\s*(\d+)>\(%s\{\}" % name, form_fn)
        assert sites == [({0: "false", 1: "true"}[chunked], "false", str(scene))], (name, sites)
        assert all(v != 0 for v in lists[name]) and len(set(lists[name])) == len(lists[name]), (name, lists[name])
        forms |= {(scene, chunked, v) for v in lists[name]}
    assert len(re.findall(r"launch_kind_of<", form_fn)) == len(KIND_LISTS) + 1
    assert re.findall(r"launch_kind_of<PHASE,\s*CLS,\s*false,\s*true,\s*0>\((\w+)\{\}", form_fn) == ["KindsStamped"]
    # the general kernel of the two LDS scene forms, for every chunking the launcher passes in
    scenes = {int(s) for s in re.findall(r"SphereQueueForm<PHASE,\s*CLS,\s*CHUNKED,\s*false,\s*(\d+)>\{\}", form_fn)}
    calls = {(int(p), int(c), _bool(ch)) for p, c, ch in re.findall(r"launch_queue_form<(\d+),\s*(\d+),\s*(true|false)>\(", src)}
    assert scenes and calls
    forms |= {(s, ch, 0) for s in scenes for ch in {ch for _, _, ch in calls}}
    # the global scene: the launch sites of (PHASE 0, CLS 0) alone
    assert re.search(r"if constexpr \(PHASE == 0 && CLS == 0\)[^\n]*SphereQueueForm<0,\s*0,\s*CHUNKED,\s*false,\s*1>\{\}", form_fn)
    forms |= {(1, ch, 0) for p, c, ch in calls if (p, c) == (0, 0)}
    # every instantiation is named in launch_queue_form (through SphereQueueForm) and launched by launch_sphere_queue alone
    assert len(re.findall(r"k_render_spheres_queue<", src)) == 1 and "k_render_spheres_queue<PHASE, CLS, CHUNKED, DBG, SCENE, LEAN>" in _function(src, "static hipError_t launch_sphere_queue(")
    elsewhere = set(re.findall(r"SphereQueueForm<([^>]*)>", src.replace(form_fn, "")))
    assert elsewhere == {"PHASE, CLS, CHUNKED, DBG, SCENE, LEAN", "PHASE, CLS, CHUNKED, DBG, SCENE, LEANS"}, elsewhere       # launch_sphere_queue, launch_kind_of
    tiles = {_bool(t) for t in re.findall(r"k_render_spheres_tiles<(true|false)>", _function(src, "hipError_t RT_LAUNCH_NAME("))}
    return forms, calls, tiles


def mesh_source_forms():
    """(phase, trav, lean) of every non-diagnostic k_render_mesh_queue instantiation and the tile kernel's variants.  The instantiations are the MeshQueueForm<...>
    that launch_mesh_form names: one whose last argument is PHASE exists for every phase the launcher calls launch_mesh_form<phase> with, one inside an
    `if constexpr (PHASE == 0)` block for phase 0 alone (it must say 0)."""
    src = _code("rt_kernels_mesh.hip")
    form_fn = _function(src, "static hipError_t launch_mesh_form(")
    phases = {int(p) for p in re.findall(r"launch_mesh_form<(\d+)>\(", src)}
    assert phases == {0, 1, 2}, phases
    only0 = "".join(re.findall(r"if constexpr \(PHASE == 0\) \{(.*?)\n    \}", form_fn, re.S))
    forms = set()
    for args in re.findall(r"MeshQueueForm<([^>]*)>\{\}", form_fn):
        a = [x.strip() for x in args.split(",")]
        assert len(a) == 5, args
        trav, dbg, stats, lean = int(a[0]), _bool(a[1]), _bool(a[2]), _bool(a[3])
        assert (a[4] == "0") == (("MeshQueueForm<%s>{}" % args) in only0), args
        for phase in (phases if a[4] == "PHASE" else {int(a[4])}):
            if not dbg and not stats:
                forms.add((phase, trav, lean))
    # every instantiation is named in launch_mesh_form (through MeshQueueForm) and launched by launch_mesh_queue alone
    assert set(re.findall(r"MeshQueueForm<([^>]*)>", src.replace(form_fn, ""))) == {"TRAV, DBG, STATS, LEAN, PHASE"}
    tiles = {int(v) for v in re.findall(r"hipLaunchKernelGGL\(k_render_mesh<(\d+)>", src)}
    assert forms and tiles
    return forms, tiles


def table_keys():
    keys = {K.form_key(r) for f in K.FORMS for r in f["records"]}
    for ab in K.AB_ONLY:
        keys |= set(ab["keys"])
    return keys


def test_every_sphere_instantiation_has_a_row_and_every_row_an_instantiation():
    forms, calls, tiles = sphere_source_forms()
    keys = table_keys()
    table = {(k[4], k[3], k[5]) for k in keys if k[0] == SQ}
    assert forms - table == set(), f"launched in the source, not in tests/kernel_forms.py: {sorted(forms - table)}"
    assert table - forms == set(), f"rows of tests/kernel_forms.py that the source no longer launches: {sorted(table - forms)}"
    table_calls = {(k[1], k[2], k[3]) for k in keys if k[0] == SQ and k[4] != 1}
    assert calls == table_calls, (sorted(calls), sorted(table_calls))
    assert tiles == {k[2] for k in keys if k[0] == ST}


def test_every_mesh_instantiation_has_a_row_and_every_row_an_instantiation():
    forms, tiles = mesh_source_forms()
    keys = table_keys()
    table = {(k[1], k[2], k[5]) for k in keys if k[0] == MQ}
    assert forms == table, (sorted(forms), sorted(table))
    assert tiles == {k[2] for k in keys if k[0] == MT}


def test_table_rows_are_complete():
    """Unique names; every lean kind of the full copy on the two-dispatch path and the single dispatch; the six-wave kinds with their pixel threshold at
    one pixel and 12-wave workgroups; the expected records of a frame use the frame's workgroup shape throughout."""
    names = [f["name"] for f in K.FORMS]
    assert len(names) == len(set(names))
    full = {}
    for f in K.FORMS:
        for r in f["records"]:
            assert len(r) == len(K.RECORD_FIELDS) and r[4] == 0, f["name"]            # production kernels only
            if r[0] == SQ and r[5] == 0 and not r[3]:
                full.setdefault(r[6], set()).add(r[1])
            if r[0] == SQ and r[6] & 4:
                assert f["env"]["RT_LEAN6_PIXELS"] == "1" and r[7] == 768, f["name"]
        assert len({r[7:] for r in f["records"]}) == 1, f["name"]
    assert set(full) == {0, 1, 3, 7, 11, 15, 19, 27, 35, 43}
    assert all(phases == {0, 1, 2} for phases in full.values()), full


# ---- the sphere launcher: a pure plan, one attribute site, one statement of the kinds ----------------------------------

def _host_region(src):
    """The launcher: everything behind the kernels."""
    return src[src.index("constexpr size_t kStaticLds"):]


def test_plan_spheres_makes_no_hip_call():
    body = _function(_code("rt_kernels_spheres.hip"), "static SpherePlan plan_spheres(")
    assert len(body) > 2000 and "return pl;" in body
    assert re.findall(r"hip[A-Z]\w*\(", body) == []


def test_lds_attribute_is_set_in_one_function():
    src = _code("rt_kernels_spheres.hip")
    assert len(re.findall(r"hipFuncSetAttribute", src)) == 1
    assert "hipFuncSetAttribute" in _function(src, "static hipError_t launch_with_lds(")


def test_lean_literals_of_the_built_kinds_occur_only_in_the_kind_lists():
    """Outside the kind lists the launcher names no built kind by its number: no `case`, no comparison or assignment of a lean value with such a literal,
    no template argument list that ends in one.  (The LEAN bits are named constants written as shifts.)"""
    src = _code("rt_kernels_spheres.hip")
    built = {v for kinds in sphere_kind_lists(src).values() for v in kinds}
    assert {1, 3, 7, 35, 43} <= built
    host = re.sub(r"using\s+Kinds\w+\s*=\s*std::integer_sequence<int,[^>]*>;", "", _host_region(src))
    found = [(m.group(0), int(m.group(1), 0)) for m in re.finditer(r"\bcase\s+(\d+|0x[0-9a-fA-F]+)\s*:", host)]
    found += [(m.group(0), int(m.group(1), 0)) for m in re.finditer(r"\blean\w*\s*(?:==|!=|\|=|&=|=|&|\|)\s*(\d+|0x[0-9a-fA-F]+)\b", host)]
    found += [(m.group(0), int(m.group(1), 0)) for m in re.finditer(r"(?:SphereQueueForm|k_render_spheres_queue)<(?:[^<>,]*,){5}\s*(\d+)\s*>", host)]
    assert [f for f in found if f[1] in built] == [], found


# ---- the mesh launcher: a pure plan in its own header, one function that names the kernel, the packed arguments by name ----------------------------------

def test_plan_mesh_makes_no_hip_call():
    hdr = _code("rt_mesh_plan.h")
    body = _function(hdr, "inline MeshPlan plan_mesh(")
    assert len(body) > 2000 and "return pl;" in body
    assert re.findall(r"hip[A-Z]\w*\(", hdr) == []
    assert re.findall(r"#include\s*[<\"]([^>\"]*)[>\"]", hdr) == ["rt_params.h"]           # the parameter blocks, nothing of the kernels
    launcher = _function(_code("rt_kernels_mesh.hip"), "hipError_t RT_LAUNCH_NAME(const RtMeshParams& p")
    assert len(re.findall(r"\bplan_mesh\(", launcher)) == 1 and len(re.findall(r"\bvariant\b", launcher)) == 2          # (the parameter, and the plan's argument)


def test_mesh_queue_kernel_is_named_in_one_function():
    src = _code("rt_kernels_mesh.hip")
    assert len(re.findall(r"k_render_mesh_queue<", src)) == 1
    assert "k_render_mesh_queue<TRAV, DBG, STATS, LEAN, PHASE>" in _function(src, "static hipError_t launch_mesh_queue(")


def test_mesh_packed_arguments_are_read_by_field_name():
    """Outside rt_mesh_plan.h neither the kernel nor the launcher applies a literal shift or mask to leaf_thr or min_traversing (or to a copy named after them)."""
    src = _code("rt_kernels_mesh.hip")
    words = r"\b(?:leaf_thr|min_traversing|lt|mt)\w*"
    lit = r"(?:0[xX][0-9a-fA-F]+|\d+)[uU]?\b"
    found = re.findall(r"%s\s*(?:>>|<<|&|\||\^|>>=|<<=|&=|\|=)\s*%s" % (words, lit), src)
    found += re.findall(r"%s\s*(?:>>|<<|&|\||\^)\s*%s" % (lit, words), src)
    found += re.findall(r"\(\s*%s\s*\)\s*(?:>>|<<|&|\|)" % words, src)
    assert found == [], found
    for field in ("kLeafThr", "kLeafHeavyClasses", "kLeafSpreadRounds", "kLeafChainLanes", "kLeafChainFrac"):
        assert re.search(r"%s\.get\(leaf_thr\)" % field, src), field
    for field in ("kMinTravLanes", "kMinTravSegments"):
        assert re.search(r"%s\.get\(min_traversing\)" % field, src), field
    assert len(re.findall(r"\bstruct BitField\b", _code("rt_params.h") + _code("rt_kernels_spheres.hip") + _code("rt_mesh_plan.h") + src)) == 1
