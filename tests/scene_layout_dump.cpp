// scene_layout_dump.cpp — runs layout_spheres / layout_mesh / permute_triangles (rt_scene_layout.h) on the scenes of tests/test_scene_layout.py: plain C++,
// no kernel, no HIP call, no GPU.  usage: scene_layout_dump IN OUT [REPEAT].  Both files are flat little-endian records (the layouts the test writes and reads
// with numpy):
//   IN   int32 cases, then per case int32 kind and
//        kind 0 (spheres): int32 n, box_cells; n rt_sphere; n rt_material
//        kind 1 (mesh):    int32 numTris, numBvhNodes, nppl, numMaterials, numTextures, nfrom; float bounds[6], floor[6]; the triangles; the nodes; the
//                          materials; per texture int32 width, height and width * height * 3 floats; nfrom int32 `from` (0 = no permutation asked for)
//   OUT  per case
//        kind 0: the template's ints and floats in the order of kSphereInts / kSphereFloats below, int32 "every scene pointer is null", then the seven arrays
//        kind 1: uint32 first_leaf, nppl, int32 leaf_sentinels_trailing, lean_ok, "every scene pointer is null", float bounds[6], floor[6], then tris, bvh,
//                bvh_axis, leaf_tri, leaf_ofs, materials, tex_w, tex_h, every texture; with nfrom > 0 the triangles after permute_triangles
//        an array = int64 element count, then its bytes.
// REPEAT > 1 builds every layout that many times and prints the median time of one build per case, in microseconds (nothing else changes).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_scene_layout.h"

static FILE* g_in;
static FILE* g_out;

template <typename T>
static std::vector<T> get(size_t count) {
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, g_in) != count) { fprintf(stderr, "scene_layout_dump: input too short\n"); exit(1); }
    return v;
}
static int32_t get_int() { return get<int32_t>(1)[0]; }

template <typename T>
static void put(const T* p, size_t count) {
    if (count && fwrite(p, sizeof(T), count, g_out) != count) { fprintf(stderr, "scene_layout_dump: write failed\n"); exit(1); }
}
template <typename T>
static void put_array(const std::vector<T>& v) {
    const int64_t count = (int64_t)v.size();
    put(&count, 1);
    put(v.data(), v.size());
}

template <typename F>
static auto timed(int repeat, F build) {
    std::vector<double> us;
    auto r = build();
    for (int k = 1; k < repeat; k++) {
        const auto t0 = std::chrono::steady_clock::now();
        r = build();                                            // (move-assigned, as the renderer does)
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    if (!us.empty()) {
        std::sort(us.begin(), us.end());
        printf("%.1f\n", us[us.size() / 2]);
    }
    return r;
}

static void sphere_case(int repeat) {
    const int n = get_int(), box_cells = get_int();
    const std::vector<rt_sphere> spheres = get<rt_sphere>(n);
    const std::vector<rt_material> materials = get<rt_material>(n);
    const SphereLayout L = timed(repeat, [&] { return layout_spheres(spheres.data(), materials.data(), n, box_cells != 0); });
    const RtSphereParams& s = L.scene;
    const int32_t ints[] = { s.n, s.n_padded, s.n_groups, s.n_big_groups, s.n_big, s.basic_materials, s.global_scene, s.box_shared_axis, s.cell_on, s.cell_axes };     // kSphereInts
    const float floats[] = { s.cull_cx, s.cull_cy, s.cull_cz, s.cull_radius, s.cull_k1, s.cull_k2, s.cull_k3, s.cull_coord_max, s.box_shared_lo, s.box_shared_hi,
                             s.pair_k0, s.cell_scale[0], s.cell_scale[1], s.cell_scale[2], s.cell_off[0], s.cell_off[1], s.cell_off[2],
                             s.ubox[0], s.ubox[1], s.ubox[2], s.ubox[3], s.ubox[4], s.ubox[5] };                                                                        // kSphereFloats
    const int32_t null = !s.spheres && !s.rad && !s.groups && !s.mat_color && !s.mat_type && !s.orig && !s.slot_of && !s.self && !s.fb;
    put(ints, sizeof ints / sizeof ints[0]);
    put(floats, sizeof floats / sizeof floats[0]);
    put(&null, 1);
    put_array(L.spheres); put_array(L.rad); put_array(L.mat_color); put_array(L.mat_type); put_array(L.groups); put_array(L.orig); put_array(L.slot_of);
}

static void mesh_case(int repeat) {
    const int num_tris = get_int(), num_nodes = get_int(), nppl = get_int(), num_materials = get_int(), num_textures = get_int(), nfrom = get_int();
    const std::vector<float> boxes = get<float>(12);
    std::vector<rt_triangle> tris = get<rt_triangle>(num_tris);
    std::vector<rt_bvh_node> nodes = get<rt_bvh_node>(num_nodes);
    std::vector<rt_material> materials = get<rt_material>(num_materials);
    std::vector<std::vector<float>> tex_data(num_textures);
    std::vector<rt_stexture> textures(num_textures);
    for (int t = 0; t < num_textures; t++) {
        textures[t].width = get_int(); textures[t].height = get_int();
        tex_data[t] = get<float>((size_t)textures[t].width * textures[t].height * 3);
        textures[t].data = tex_data[t].data();
    }
    const std::vector<int32_t> from = get<int32_t>(nfrom);
    rt_mesh m;
    m.tris = tris.data(); m.numTris = (uint32_t)num_tris; m.bvh = nodes.data(); m.numBvhNodes = num_nodes;
    rt_kernel_scene sc;
    sc.m = &m; sc.materials = materials.data(); sc.numMaterials = num_materials; sc.textures = textures.data(); sc.numTextures = num_textures;
    sc.numPrimitivesPerLeaf = nppl;
    for (int a = 0; a < 3; a++) {
        m.bounds.min.e[a] = boxes[a]; m.bounds.max.e[a] = boxes[3 + a];
        sc.floor.norm.e[a] = boxes[6 + a]; sc.floor.point.e[a] = boxes[9 + a];
    }
    MeshLayout L = timed(repeat, [&] { return layout_mesh(sc); });
    const RtMeshParams& p = L.scene;
    const uint32_t words[] = { p.first_leaf, p.nppl };
    const int32_t null = !p.tris && !p.bvh4 && !p.bvh_axis && !p.leaf_tri && !p.leaf_ofs && !p.materials && !p.tex_data && !p.tex_width && !p.tex_height;
    const int32_t ints[] = { p.leaf_sentinels_trailing, p.lean_ok, null };
    put(words, 2);
    put(ints, 3);
    put(p.bounds.min.e, 3); put(p.bounds.max.e, 3); put(p.floor.norm.e, 3); put(p.floor.point.e, 3);
    put_array(L.tris); put_array(L.bvh); put_array(L.bvh_axis); put_array(L.leaf_tri); put_array(L.leaf_ofs); put_array(L.materials);
    put_array(L.tex_w); put_array(L.tex_h);
    for (const std::vector<float>& t : L.tex) put_array(t);
    if (nfrom > 0) {
        permute_triangles(L, from);
        put_array(L.tris);
    }
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: scene_layout_dump IN OUT [REPEAT]\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { fprintf(stderr, "scene_layout_dump: cannot open the files\n"); return 2; }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    const int cases = get_int();
    for (int k = 0; k < cases; k++) {
        const int kind = get_int();
        if (kind == 0) sphere_case(repeat);
        else if (kind == 1) mesh_case(repeat);
        else { fprintf(stderr, "scene_layout_dump: unknown kind %d\n", kind); return 1; }
    }
    fclose(g_in);
    return fclose(g_out) == 0 ? 0 : 1;
}
