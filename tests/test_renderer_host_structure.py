"""CPU tripwire: the host runtime (rt_renderer.hip) says each thing once.  Device memory is allocated by one function that records the pointer with its
owner and freed only by the functions that walk that record, so a new buffer cannot be forgotten in a hand-kept list of frees; every scene pointer of a
kernel parameter block is assigned in exactly one place (sphere_params / mesh_params), so a frame, the guide planes and the denoiser cannot disagree about
the scene; RenderContext holds the scene as the two layout structs of rt_scene_layout.h, which keep the scene's constants in parameter-block form (their
`scene` templates), not as a second set of members that is copied across field by field; and the whole-image preview passes (denoiseFrame,
accumulateFrame) share one state struct (PassState), one release (free_pass) and one path around their kernels (begin_pass / end_pass), so a third pass
is not a third copy of them; and the query calls (traceRays / occludedRays, renderPixels, refineFrame) share one state base, one chunked path, one launch
of the pixel kernels and one statement of what a path is (sphere_path_params / mesh_path_params), which a frame takes too."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDERER = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc", "rt_renderer.hip")
LAYOUT = os.path.join(ROOT, "cuda-raytracing-optimized_amd", "csrc", "rt_scene_layout.h")
# a function definition at column 0: return type, name, parameters, the opening brace
FUNC = re.compile(r"^[A-Za-z_][\w:<>,*& ]*?\b(\w+)\s*\([^;{}]*\)\s*(?:const\s*)?\{", re.M)

ALLOCATORS = {"dev_alloc"}
RELEASERS = {"dev_release", "dev_release_all"}
SCENE_POINTERS = ["spheres", "rad", "mat_color", "mat_type", "groups", "orig", "slot_of", "tris", "bvh4", "materials", "tex_data"]
# scalars of RtSphereParams / RtMeshParams (and the names a member-by-member mirror of them would carry): they live in the scene templates only
MIRRORED = ["n_spheres", "n_padded", "n_groups", "n_big_groups", "n_big", "global_scene", "basic_materials", "cull_c", "cull_radius", "cull_k1", "cull_k2",
            "cull_k3", "cull_coord_max", "pair_k0", "box_shared_axis", "box_shared_lo", "box_shared_hi", "cell_on", "cell_axes", "cell_scale", "cell_off",
            "ubox", "num_bvh_nodes", "nppl", "leaf_sentinels_trailing", "bounds", "floor"]
# what every whole-image pass holds on the device
PASS_MEMBERS = ["device", "npix", "owned", "d_guide", "d_in", "d_out"]
PASSES = {"denoiseFrame", "accumulateFrame"}
# the query calls and their chunk functions: whichever of them the file defines
QUERIES = {"traceRays", "occludedRays", "renderPixels", "refineFrame", "rtRefineLastList", "run_rays", "run_pixels"}
QUERY_MEMBERS = ["device", "owned", "ev_start", "ev_stop"]
QUERY_STATES = ["g_rays", "g_pixels", "g_refine"]


def _source(path=RENDERER):
    return re.sub(r"//[^\n]*", "", open(path).read())


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


def _callers(src, call):
    funcs = _functions(src)
    return [_enclosing(funcs, m.start()) for m in re.finditer(r"\b%s\s*\(" % call, src)]


def test_device_memory_is_allocated_and_freed_in_one_place():
    src = _source()
    mallocs, frees = _callers(src, "hipMalloc"), _callers(src, "hipFree")
    assert mallocs and frees
    assert set(mallocs) <= ALLOCATORS, f"hipMalloc outside the allocation function: {sorted(set(map(str, mallocs)) - ALLOCATORS)}"
    assert set(frees) <= RELEASERS, f"hipFree outside the release functions: {sorted(set(map(str, frees)) - RELEASERS)}"


def test_every_scene_pointer_is_assigned_once():
    src = _source()
    for name in SCENE_POINTERS:
        n = len(re.findall(r"\.%s\s*=(?!=)" % name, src))
        assert n == 1, f".{name} is assigned {n} times"


def test_render_context_does_not_mirror_the_parameter_blocks():
    m = re.search(r"^struct RenderContext \{(.*?)^\};", _source(), re.M | re.S)
    assert m, "struct RenderContext not found"
    body = m.group(1)
    assert re.search(r"\bSphereLayout\s+\w+", body) and re.search(r"\bMeshLayout\s+\w+", body), "no scene layout in RenderContext"
    mirrored = [name for name in MIRRORED if re.search(r"\b%s\b" % name, body)]
    assert mirrored == [], f"RenderContext mirrors parameter-block fields: {mirrored}"
    # the layout structs it holds: one template each, and no field of it a second time beside the template
    for struct, template in (("SphereLayout", "RtSphereParams"), ("MeshLayout", "RtMeshParams")):
        m = re.search(r"^struct %s \{(.*?)^\};" % struct, _source(LAYOUT), re.M | re.S)
        assert m, f"struct {struct} not found"
        members = re.findall(r"\b%s\s+\w+[^;]*;" % template, m.group(1))
        assert len(members) == 1, f"{struct} holds {len(members)} {template} templates"
        rest = m.group(1).replace(members[0], "")
        mirrored = [name for name in MIRRORED if re.search(r"\b%s\b" % name, rest)]
        assert mirrored == [], f"{struct} mirrors parameter-block fields: {mirrored}"


def test_one_function_builds_the_whole_image_partition():
    src = _source()
    funcs = _functions(src)
    builders = [_enclosing(funcs, m.start()) for m in re.finditer(r"\.world\s*=\s*1\b", src)]
    assert builders == ["whole_image_partition"], builders
    assert "RtPartition" not in "".join(src[a:b] for n, a, b in funcs if n in PASSES)


def test_the_passes_leave_events_and_the_current_device_to_the_shared_path():
    src = _source()
    creators = set(_callers(src, "hipEventCreate"))
    assert creators == {"setup_devices", "begin_pass"}, sorted(map(str, creators))
    for call in ("hipEventCreate", "hipGetDevice", "hipSetDevice"):
        assert not PASSES & set(_callers(src, call)), call
    assert not re.search(r"\bfree_(denoise|accumulate)\b", src)


def test_pass_members_are_declared_in_one_struct():
    structs = re.findall(r"^struct (\w+)[^{\n]*\{(.*?)^\};", _source(), re.M | re.S)
    holders = {name: [s for s, body in structs if re.search(r"\b%s\b\s*(?:\[\d+\]\s*)?[=;]" % name, body)] for name in PASS_MEMBERS}
    whole = [s for s, body in structs if all(s in holders[name] for name in PASS_MEMBERS)]
    assert len(whole) == 1, holders
    for name in ("npix", "d_in", "d_out"):                      # (a DeviceState has a device, a record of its allocations and guide planes of its own rows)
        assert holders[name] == whole, (name, holders[name])


# ---- the query calls (traceRays / occludedRays, renderPixels, refineFrame): one state base, one chunked path, one pixel launch, one statement of a path ----

def _body(src, name):
    bodies = [src[a:b] for n, a, b in _functions(src) if n == name]
    assert len(bodies) == 1, (name, len(bodies))
    return bodies[0]


def _assigners(src, field):
    """The functions that assign `.field` of a struct as a whole - `o->light.center.e[0] = ...` writes an element, not the field - in the file's order.
    RenderContext's own max_depth (`c.max_depth = ...`, common_init) is what the parameter blocks copy, not one of them."""
    funcs = _functions(src)
    return [_enclosing(funcs, m.start()) for m in re.finditer(r"(?<!\bc)\.%s\b\s*=(?!=)" % field, src)]


def test_the_query_calls_leave_memory_events_and_the_current_device_to_the_shared_path():
    src = _source()
    defined = {n for n, _, _ in _functions(src)}
    assert {"traceRays", "occludedRays", "renderPixels", "refineFrame", "rtRefineLastList"} <= defined
    for call in ("hipMalloc", "hipFree", "hipEventCreate", "hipGetDevice", "hipSetDevice", "hipEventElapsedTime"):
        callers = set(_callers(src, call))
        assert callers, call
        assert not QUERIES & callers, (call, sorted(QUERIES & callers))
    assert set(_callers(src, "hipEventCreate")) == {"setup_devices", "begin_pass"}


def test_the_ray_and_pixel_kernels_are_launched_from_one_place_each():
    src = _source()
    for name in ("rt_launch_pixels_spheres_parity", "rt_launch_pixels_spheres_fast", "rt_launch_pixels_mesh_parity", "rt_launch_pixels_mesh_fast",
                 "rt_launch_rays_spheres", "rt_launch_rays_mesh"):
        n = len(re.findall(r"\b%s\b" % name, src))
        assert n == 1, f"{name} occurs {n} times"
    launchers = {c for name in ("parity", "fast") for kind in ("spheres", "mesh") for c in _callers(src, f"rt_launch_pixels_{kind}_{name}")}
    assert launchers == {"launch_pixels"}, launchers
    assert {"run_pixels", "refineFrame"} <= set(_callers(src, "launch_pixels"))


def test_what_a_path_is_is_assigned_once_per_scene_kind():
    src = _source()
    for field in ("max_depth", "rr", "rng_mode"):
        assert _assigners(src, field) == ["sphere_path_params", "mesh_path_params"], (field, _assigners(src, field))
    for field in ("nee", "light", "lightColor"):
        assert _assigners(src, field) == ["mesh_path_params"], (field, _assigners(src, field))
    for fn in ("render_frame", "launch_pixels"):
        assert "sphere_path_params" in _body(src, fn) and "mesh_path_params" in _body(src, fn), fn


def test_the_query_states_share_one_base():
    src = _source()
    structs = {name: (base, body) for name, base, body in re.findall(r"^struct (\w+)(?:\s*:\s*(\w+))?\s*\{(.*?)^\};", src, re.M | re.S)}
    declares = lambda struct, member: re.search(r"\b%s\b\s*(?:\[\d+\]\s*)?[=;,]" % member, structs[struct][1]) is not None
    types = []
    for var in QUERY_STATES:
        m = re.search(r"^(\w+)\s+(?:\w+\s*,\s*)*%s\b[^;()]*;" % var, src, re.M)
        assert m and m.group(1) in structs, var
        types.append(m.group(1))
    bases = {structs[t][0] for t in types}
    assert len(bases) == 1 and bases != {""}, dict(zip(QUERY_STATES, [(t, structs[t][0]) for t in types]))
    base = bases.pop()
    assert base != "PassState" and structs[base][0] == ""
    for member in QUERY_MEMBERS:
        assert declares(base, member), (base, member)
        assert not [t for t in types if declares(t, member)], (member, types)


def test_every_query_state_is_released_where_the_passes_are():
    src = _source()
    for fn in ("setup_devices", "cleanup_impl"):
        for var in QUERY_STATES:
            assert re.search(r"\bfree_pass\(%s\)" % var, _body(src, fn)), (fn, var)
