"""CPU tripwire: the table of production forms (tests/kernel_forms.py, rendered by test_gpu_kernel_forms.py) against the launch sites in the kernel
sources.  Every instantiation a launcher can launch without diagnostics must have a row, and every row must name an instantiation that is still
launched: a new `case` in launch_queue_kernel_scene without a test, or a deleted one with a stale row, fails here without a GPU."""
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


def sphere_source_forms():
    """(scene, chunked, lean) of every non-diagnostic k_render_spheres_queue launch, (phase, cls, chunked) of the launcher's calls, tile kernels."""
    src = _code("rt_kernels_spheres.hip")
    scene_fn = _function(src, "static hipError_t launch_queue_kernel_scene(")
    forms = set()
    for case, args in re.findall(r"case\s+(\d+)\s*:\s*return\s+go\(\s*SphereQueueForm<([^>]*)>\{\}\)", scene_fn):
        phase, cls, chunked, dbg, scene, lean = [a.strip() for a in args.split(",")]
        assert (phase, cls) == ("PHASE", "CLS") and dbg == "false" and int(lean) == int(case), args
        forms.add((int(scene), _bool(chunked), int(lean)))
    # the fallback: the general kernel of every scene form and chunking the launcher passes in
    assert re.search(r"return\s+go\(\s*SphereQueueForm<PHASE,\s*CLS,\s*CHUNKED,\s*false,\s*SCENE>\{\}\);", scene_fn)
    scenes = {int(s) for s in re.findall(r"launch_queue_kernel_scene<PHASE,\s*CLS,\s*CHUNKED,\s*(\d+)>\(", src)}
    calls = {(int(p), int(c), _bool(ch)) for p, c, ch in re.findall(r"launch_queue_kernel<(\d+),\s*(\d+),\s*(true|false)>\(", src)}
    assert scenes and calls
    forms |= {(s, ch, 0) for s in scenes for ch in {ch for _, _, ch in calls}}
    # the global scene
    global_fn = _function(src, "static hipError_t launch_queue_kernel_global(")
    assert re.search(r"SphereQueueForm<0,\s*0,\s*CHUNKED,\s*false,\s*1>\{\}", global_fn)
    forms |= {(1, _bool(ch), 0) for ch in re.findall(r"launch_queue_kernel_global<(true|false)>\(", src)}
    tiles = {_bool(t) for t in re.findall(r"hipLaunchKernelGGL\(k_render_spheres_tiles<(true|false)>", src)}
    return forms, calls, tiles


def mesh_source_forms():
    """(phase, trav, lean) of every non-diagnostic k_render_mesh_queue launch and the tile kernel's variants."""
    src = _code("rt_kernels_mesh.hip")
    forms = set()
    for args in re.findall(r"launch_mesh_queue<([^>]*)>\(grid", src):
        a = [x.strip() for x in args.split(",")]
        trav, dbg, stats = int(a[0]), _bool(a[1]), _bool(a[2])
        lean = _bool(a[3]) if len(a) > 3 else 0
        phase = int(a[4]) if len(a) > 4 else 0
        if not dbg and not stats:
            forms.add((phase, trav, lean))
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
