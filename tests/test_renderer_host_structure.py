"""CPU tripwire: the host runtime (rt_renderer.hip) says each thing once.  Device memory is allocated by one function that records the pointer with its
owner and freed only by the functions that walk that record, so a new buffer cannot be forgotten in a hand-kept list of frees; every scene pointer of a
kernel parameter block is assigned in exactly one place (sphere_params / mesh_params), so a frame, the guide planes and the denoiser cannot disagree about
the scene; RenderContext holds the scene as the two layout structs of rt_scene_layout.h, which keep the scene's constants in parameter-block form (their
`scene` templates), not as a second set of members that is copied across field by field; and the whole-image preview passes (denoiseFrame,
accumulateFrame) share one state struct (PassState), one release (free_pass) and one path around their kernels (begin_pass / end_pass), so a third pass
is not a third copy of them."""
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
