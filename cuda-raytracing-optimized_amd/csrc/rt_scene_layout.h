// rt_scene_layout.h — the device images of the two scene kinds, built on the host: every array the renderer uploads for a scene and every scene constant of
// its parameter blocks (layout_spheres, layout_mesh), and the host side of a rebuild's triangle permutation (permute_triangles).  The kernels' bit-exactness
// rests on this arithmetic - a group box one float too tight, a missing cell bit, an edge rounded twice - and the refit kernels reproduce its bits.
// Host only: no kernel, no HIP call, no global and no environment read in here (a switch the layout depends on is an argument), so a plain C++ program that
// includes this header builds the images on a machine without a GPU and under a sanitizer (tests/scene_layout_dump.cpp, tests/test_scene_layout.py).
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "rt_params.h"

// A sphere scene as the kernels read it.  `scene`: the scene's constants in parameter-block form, every pointer null - the slot and group counts,
// basic_materials, the culling constants and the cell tables' geometry; the start of every sphere parameter block (global_scene is the launcher's decision:
// the renderer's build_sphere_scene sets it).
struct SphereLayout {
    RtSphereParams scene = {};
    std::vector<float4> spheres;        // the kernel's sphere image (rt_params.h): (n_padded + n_groups) x (cx, cy, cz, r*r)
    std::vector<float> rad;             // n_padded radii
    std::vector<float4> mat_color;
    std::vector<int32_t> mat_type;
    std::vector<float4> groups;         // three float4 per group of kSphereGroup slots: per axis (lo, hi, lo, -) of the tight AABB; then the cell tables
    std::vector<int32_t> orig;          // slot -> caller's sphere index (INT_MAX = pad)
    std::vector<int32_t> slot_of;       // caller's sphere index -> slot
};

// A mesh scene as the kernels read it.  `scene`: first_leaf, nppl, leaf_sentinels_trailing, lean_ok, bounds and floor (kernel_scene.floor,
// helper_structs.h:219) in parameter-block form, every pointer null; the start of every mesh parameter block.
struct MeshLayout {
    RtMeshParams scene = {};
    std::vector<rt_triangle> tris;
    std::vector<float4> bvh;            // numBvhNodes * 24 B viewed as float4 (padded)
    std::vector<float> bvh_axis;        // RtMeshParams::bvh_axis
    std::vector<float4> leaf_tri;       // RtMeshParams::leaf_tri (empty = not built: sentinels inside leaves, or more than 255 triangles per leaf)
    std::vector<uint32_t> leaf_ofs;     // RtMeshParams::leaf_ofs
    std::vector<rt_material> materials;
    std::vector<std::vector<float>> tex;
    std::vector<int32_t> tex_w, tex_h;
};

// Device layout of a sphere scene.  The spheres are re-ordered into SLOTS, kSphereGroup (G) slots per group:
//   * "big" spheres (radius > 4 x the median radius: the ground and the three unit spheres of the benchmark scene)
//     come first; their groups are always scanned, by every lane, and give each ray a first `closest`;
//   * "small" spheres are split recursively at medians so that the G slots of a group are neighbours in space; each
//     group of G gets its tight axis-aligned bounding box, three entries (lo, hi, lo, -), one per axis, with the cell
//     tables behind them; the kernel uses it to skip the group for rays that cannot reach it before their current hit,
//     and the culling is exact through the margin every ray adds for itself (make_box_ray), not through an inflation;
//   * pad slots fill the last group of each class and the tail up to a multiple of 64 slots; they carry
//     orig = INT_MAX and are never accepted.
// Scanning in slot order instead of the caller's order cannot change the result: the kernel resolves equal-t ties
// by the caller's index (orig), which is exactly the reference's first-index-wins rule.
// box_cells: the switch RtSwitches::box_cells, read by the caller (cell_on = the tables are valid and the switch is on).
inline SphereLayout layout_spheres(const rt_sphere* spheres, const rt_material* materials, int n, bool box_cells) {
    SphereLayout c;
    std::vector<float> radii(n);
    for (int k = 0; k < n; k++) radii[k] = fabsf(spheres[k].radius);
    std::vector<float> sorted = radii;
    std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
    const float big_above = 4.0f * sorted[n / 2];
    std::vector<int> small, big;
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
    for (int k = 0; k < n; k++) {
        if (radii[k] > big_above || !std::isfinite(radii[k])) { big.push_back(k); continue; }
        small.push_back(k);
        for (int a = 0; a < 3; a++) {
            lo[a] = std::min(lo[a], (double)spheres[k].center.e[a]);
            hi[a] = std::max(hi[a], (double)spheres[k].center.e[a]);
        }
    }
    // Groups of G = kSphereGroup: recursive median split of the small spheres along the axis of largest centre extent, the left part
    // rounded to a multiple of G, until a part fits one group.  Compact parts = small boxes = few (ray, group) pairs; a
    // 3D Morton sort (the first version) makes strips and L-shapes when the spheres lie on a plane.  ceil(n / G) groups.
    constexpr size_t G = (size_t)kSphereGroup;
    std::vector<int> ordered;
    std::function<void(std::vector<int>&, size_t, size_t)> split = [&](std::vector<int>& v, size_t b0, size_t e0) {
        const size_t cnt = e0 - b0;
        if (cnt <= (size_t)G) {
            for (size_t q = b0; q < e0; q++) ordered.push_back(v[q]);
            while (ordered.size() % G) ordered.push_back(-1);      // pad this group
            return;
        }
        double l3[3] = { 1e300, 1e300, 1e300 }, h3[3] = { -1e300, -1e300, -1e300 };
        for (size_t q = b0; q < e0; q++)
            for (int a = 0; a < 3; a++) {
                l3[a] = std::min(l3[a], (double)spheres[v[q]].center.e[a]);
                h3[a] = std::max(h3[a], (double)spheres[v[q]].center.e[a]);
            }
        int axis = 0;
        for (int a = 1; a < 3; a++) if (h3[a] - l3[a] > h3[axis] - l3[axis]) axis = a;
        std::stable_sort(v.begin() + b0, v.begin() + e0, [&](int x, int y) { return spheres[x].center.e[axis] < spheres[y].center.e[axis]; });
        const size_t groups = (cnt + G - 1) / G;
        const size_t left = std::min(cnt - 1, (groups / 2) * G);     // a multiple of G: only the last group of the scene is padded
        split(v, b0, b0 + left);
        split(v, b0 + left, e0);
    };
    std::vector<int> slots;                                     // slot -> caller index, -1 = pad
    for (int k : big) slots.push_back(k);                       // big spheres first: groups [0, n_big_groups)
    while (slots.size() % G) slots.push_back(-1);
    const int n_big_groups = (int)slots.size() / G;
    if (!small.empty()) split(small, 0, small.size());
    for (int k : ordered) slots.push_back(k);
    while (slots.size() % 64) slots.push_back(-1);

    RtSphereParams& sp = c.scene;                                // the scene's constants go straight into the parameter-block template
    sp.n = n;
    sp.n_padded = (int)slots.size();
    sp.n_groups = sp.n_padded / G;
    sp.n_big_groups = n_big_groups;
    sp.n_big = (int)big.size();
    const auto sidx = [](int slot) { return slot + slot / kSphereGroup; };
    c.spheres.assign(sp.n_padded + sp.n_groups, make_float4(0.0f, 3.0e18f, 0.0f, 0.0f));      // pad: radius 0, far away
    c.rad.assign(sp.n_padded, 0.0f);
    c.mat_color.assign(sp.n_padded, make_float4(0, 0, 0, 0));
    c.mat_type.assign(sp.n_padded, RT_DIFFUSE);
    c.orig.assign(sp.n_padded, INT_MAX);
    c.slot_of.assign(n, 0);
    // bounds: 3 float4 per group, one per AXIS: (lo, hi, lo, -) - a ray reads two consecutive floats, at 0 or at 1 by the sign of its direction,
    // and has (near plane, far plane).  Empty group: lo > hi on every axis (never reachable).
    c.groups.assign((size_t)sp.n_groups * 3, make_float4(3.0e38f, -3.0e38f, 3.0e38f, 0.0f));
    sp.basic_materials = 1;
    for (int k = 0; k < n; k++) if (materials[k].type != RT_DIFFUSE && materials[k].type != RT_METAL && materials[k].type != RT_GLASS) sp.basic_materials = 0;
    for (int s = 0; s < sp.n_padded; s++) {
        const int k = slots[s];
        if (k < 0) continue;
        const float r = spheres[k].radius;
        const float r2 = r * r;                                    // intersections.h:89 radius*radius: one IEEE multiply, the same bits as on the device
        c.spheres[sidx(s)] = make_float4(spheres[k].center.e[0], spheres[k].center.e[1], spheres[k].center.e[2], r2);
        c.rad[s] = r;
        c.mat_color[s] = make_float4(materials[k].color.e[0], materials[k].color.e[1], materials[k].color.e[2], materials[k].param);
        c.mat_type[s] = materials[k].type;
        c.orig[s] = k;
        c.slot_of[k] = s;
    }
    // Group boxes: the tight AABB of the group's spheres, pushed out by one float on conversion.  What makes the culling EXACT is
    // not a static inflation but the per-ray margin the kernel adds (make_box_ray): it covers (a) the rounding of the
    // reference's own fp32 discriminant b*b - a*c, whose error grows like |org - centre|^2 - for a far camera the reference
    // accepts "hits" of rays that geometrically miss a sphere by more than any fixed inflation - and (b) the rounding of the slab test.
    float coord_max = 0.0f;
    double r_min = 1e300;
    float shared_lo[3] = { 0, 0, 0 }, shared_hi[3] = { 0, 0, 0 };
    bool shared_ok[3] = { true, true, true };
    int n_boxes = 0;
    for (int g = n_big_groups; g < sp.n_groups; g++) {
        double blo[3] = { 1e300, 1e300, 1e300 }, bhi[3] = { -1e300, -1e300, -1e300 };
        int cnt = 0;
        for (int s = g * G; s < g * G + G; s++) {
            if (slots[s] < 0) continue;
            cnt++;
            r_min = std::min(r_min, (double)radii[slots[s]]);
            for (int a = 0; a < 3; a++) {
                blo[a] = std::min(blo[a], (double)spheres[slots[s]].center.e[a] - radii[slots[s]]);
                bhi[a] = std::max(bhi[a], (double)spheres[slots[s]].center.e[a] + radii[slots[s]]);
            }
        }
        if (cnt == 0) continue;
        float flo[3], fhi[3];
        for (int a = 0; a < 3; a++) {
            flo[a] = std::nextafter((float)blo[a], -INFINITY);
            fhi[a] = std::nextafter((float)bhi[a], INFINITY);
            coord_max = std::max(coord_max, std::max(fabsf(flo[a]), fabsf(fhi[a])));
        }
        for (int a = 0; a < 3; a++) c.groups[3 * g + a] = make_float4(flo[a], fhi[a], flo[a], 0.0f);
        for (int a = 0; a < 3; a++) {                                // an axis on which every group box has the same extent?
            if (n_boxes == 0) { shared_lo[a] = flo[a]; shared_hi[a] = fhi[a]; }
            else if (shared_lo[a] != flo[a] || shared_hi[a] != fhi[a]) shared_ok[a] = false;
        }
        n_boxes++;
    }
    sp.box_shared_axis = 0;
    for (int a = 2; a >= 0; a--) if (n_boxes > 0 && shared_ok[a]) { sp.box_shared_axis = a + 1; sp.box_shared_lo = shared_lo[a]; sp.box_shared_hi = shared_hi[a]; }
    // Cell tables (rt_params.h, group_needs_cells): for scenes of up to 32 x kCellWordsMax groups, on all three axes.  Bit g of a word = small group g.
    // begins[c] = boxes with lo <= upper edge of cell c, ends[c] = boxes with hi >= lower edge of cell c, both with a slack of kCellSlack cells for
    // the rounding of the device's cell index (x * scale + off in fp32 with |index| <= kCellCount: off by < 2e-5 cells); the last begins-word and the
    // first ends-word hold every box, so that a coordinate beyond the tables' extent - clamped to the first / last cell on the device - rejects
    // nothing it should not.  An axis on which every box has the same extent (spheres resting on a plane: the vertical one) gets no bit in cell_axes:
    // its table could not reject anything.  ubox = the union of the boxes, to which the kernel clips the ray before it looks anything up.
    constexpr double kCellSlack = 1.0e-3;
    sp.cell_on = 0;
    sp.cell_axes = 0;
    const int cell_words = rt_cell_words(sp.n_groups);
    c.groups.resize((size_t)sp.n_groups * 3 + (size_t)rt_cell_f4(sp.n_groups), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (int a = 0; a < 3; a++) { sp.ubox[a] = 0.0f; sp.ubox[3 + a] = 0.0f; sp.cell_scale[a] = 0.0f; sp.cell_off[a] = 0.0f; }
    if (n_boxes > 0 && cell_words > 0) {
        const int W = cell_words;
        uint32_t* tab = reinterpret_cast<uint32_t*>(c.groups.data() + (size_t)sp.n_groups * 3);
        std::vector<char> real(sp.n_groups, 0);
        for (int g = n_big_groups; g < sp.n_groups; g++) real[g] = c.groups[3 * g].x <= c.groups[3 * g].y;
        bool ok = true;
        for (int a = 0; a < 3 && ok; a++) {
            double amin = 1e300, amax = -1e300;
            for (int g = n_big_groups; g < sp.n_groups; g++) {
                if (!real[g]) continue;
                amin = std::min(amin, (double)c.groups[3 * g + a].x);
                amax = std::max(amax, (double)c.groups[3 * g + a].y);
            }
            sp.ubox[a] = (float)amin; sp.ubox[3 + a] = (float)amax;      // (box coordinates are floats: exact)
            const double w = (amax - amin) / kCellCount;
            if (!(w > 1e-30) || !std::isfinite(w) || !std::isfinite(1.0 / w) || !std::isfinite(amin / w)) { ok = false; break; }
            sp.cell_scale[a] = (float)(1.0 / w);
            sp.cell_off[a] = (float)(-amin / w);
            if (!shared_ok[a]) sp.cell_axes |= 1 << a;
            for (int cell = 0; cell < kCellCount; cell++) {
                uint32_t* begins = tab + ((size_t)(2 * a) * kCellCount + cell) * W;
                uint32_t* ends = tab + ((size_t)(2 * a + 1) * kCellCount + cell) * W;
                for (int g = n_big_groups; g < sp.n_groups; g++) {
                    if (!real[g]) continue;
                    const int k = g - n_big_groups;
                    if (cell == kCellCount - 1 || (double)c.groups[3 * g + a].x <= amin + (cell + 1 + kCellSlack) * w) begins[k >> 5] |= 1u << (k & 31);
                    if (cell == 0 || (double)c.groups[3 * g + a].y >= amin + (cell - kCellSlack) * w) ends[k >> 5] |= 1u << (k & 31);
                }
            }
        }
        sp.cell_on = (ok && box_cells) ? 1 : 0;
    }
    // per-ray margin constants
    double cc[3] = { 0, 0, 0 }, rad = 0.0;
    if (!small.empty()) {
        for (int a = 0; a < 3; a++) cc[a] = 0.5 * (lo[a] + hi[a]);
        for (int k : small) {
            double d2 = 0.0;
            for (int a = 0; a < 3; a++) d2 += (spheres[k].center.e[a] - cc[a]) * (spheres[k].center.e[a] - cc[a]);
            rad = std::max(rad, std::sqrt(d2) + radii[k]);
        }
    } else r_min = 1.0;
    const double K_eps = 96.0 * 5.9604645e-8;            // K x 2^-24, see make_box_ray
    sp.cull_cx = (float)cc[0]; sp.cull_cy = (float)cc[1]; sp.cull_cz = (float)cc[2];
    sp.cull_radius = (float)(rad * 1.000001 + 1e-30);
    sp.cull_k1 = (float)(K_eps / (2.0 * std::max(r_min, 1e-30)));
    sp.cull_k2 = (float)std::sqrt(K_eps);
    sp.cull_k3 = 16.0f * 5.9604645e-8f;
    sp.cull_coord_max = coord_max;
    double r_max_small = 0.0;
    for (int k : small) r_max_small = std::max(r_max_small, (double)radii[k]);
    sp.pair_k0 = (float)(2.0 * 3.814697265625e-6 * r_max_small * r_max_small * 1.0001);     // 2 x kPairSlack (2^-18) x r_max^2, rounded up
    return c;
}

// RtMeshParams::lean_ok of a mesh scene's materials (layout_mesh, updateMaterials): every one RT_DIFFUSE / RT_METAL / RT_GLASS and untextured.
inline int mesh_lean_ok(const std::vector<rt_material>& materials) {
    for (const rt_material& m : materials)
        if ((m.type != RT_DIFFUSE && m.type != RT_METAL && m.type != RT_GLASS) || m.texId != -1) return 0;
    return 1;
}

// Device layout of a mesh scene (initRenderer has validated `sc`): the caller's triangles and BVH, the axis-grouped node records, the compact leaf records,
// materials and textures as host arrays, the scene's constants in the parameter-block template.
inline MeshLayout layout_mesh(const rt_kernel_scene& sc) {
    MeshLayout c;
    RtMeshParams& mp = c.scene;
    const int nppl = sc.numPrimitivesPerLeaf;
    const uint32_t first_leaf = (uint32_t)sc.m->numBvhNodes / 2;                               // kernels.cu:614
    mp.first_leaf = first_leaf;
    mp.nppl = (uint32_t)nppl;                                                                  // kernels.cu:648
    mp.bounds = sc.m->bounds;
    mp.floor = sc.floor;
    c.tris.assign(sc.m->tris, sc.m->tris + sc.m->numTris);                                    // kernels.cu:582-583
    const size_t nfloats = (size_t)sc.m->numBvhNodes * 6;                                      // kernels.cu:587-605
    c.bvh.assign((nfloats + 3) / 4 + 1, make_float4(0, 0, 0, 0));
    memcpy(c.bvh.data(), sc.m->bvh, nfloats * sizeof(float));
    {   // axis-grouped child-pair records (rt_params.h, bvh_axis): 24 floats per internal node
        const size_t nrec = (size_t)sc.m->numBvhNodes / 2;
        c.bvh_axis.assign(nrec * 24, 0.0f);
        const float* nodes = reinterpret_cast<const float*>(sc.m->bvh);
        for (size_t i = 0; i < nrec; i++) {
            const float* L = nodes + (2 * i) * 6;
            const float* R = nodes + (2 * i + 1) * 6;
            for (int a = 0; a < 3; a++) {
                float* o = c.bvh_axis.data() + i * 24 + a * 8;
                o[0] = L[a]; o[1] = R[a]; o[2] = L[3 + a]; o[3] = R[3 + a];
                o[4] = L[3 + a]; o[5] = R[3 + a]; o[6] = L[a]; o[7] = R[a];
            }
        }
    }
    // The leaf loop of kernels.cu:196-214 stops at the first sentinel (inf) triangle of a leaf.  The pair rounds of the mesh
    // kernel test a leaf's triangles in parallel and rely on sentinels being TRAILING (true for every builder that pads
    // leaves at the end); a leaf with a real triangle behind a sentinel sends the kernel to its sequential leaf loop.
    mp.leaf_sentinels_trailing = 1;
    for (uint32_t leaf = 0; leaf < first_leaf && mp.leaf_sentinels_trailing; leaf++) {
        bool seen = false;
        for (int k = 0; k < nppl; k++) {
            const bool sent = std::isinf(c.tris[(size_t)leaf * nppl + k].v[0].e[0]);
            if (seen && !sent) mp.leaf_sentinels_trailing = 0;
            seen = seen || sent;
        }
    }
    // Compact leaf records for the pair rounds (rt_params.h, leaf_tri / leaf_ofs): what triangleHit reads of a triangle and nothing else - v0 and the
    // two edges, e1 = v1 - v0 and e2 = v2 - v0 computed here with the same single fp32 subtraction per component as intersections.h:56-57 (same bits) -
    // for the REAL triangles only.  The caller's 64-byte array stays the ABI of this boundary (helper_structs.h:81-96) and is what a closest hit re-reads.
    if (mp.leaf_sentinels_trailing && nppl <= 255) {
        c.leaf_tri.assign((size_t)first_leaf * nppl * 3, make_float4(0, 0, 0, 0));
        c.leaf_ofs.assign(((size_t)first_leaf + 3) / 4, 0u);
        for (uint32_t leaf = 0; leaf < first_leaf; leaf++) {
            uint32_t cnt = 0;
            for (int k = 0; k < nppl; k++) {
                const rt_triangle& t = c.tris[(size_t)leaf * nppl + k];
                if (std::isinf(t.v[0].e[0])) break;
                volatile float e1[3], e2[3];                         // (volatile: one rounded fp32 subtraction each, never a contracted or widened form)
                for (int a = 0; a < 3; a++) { e1[a] = t.v[1].e[a] - t.v[0].e[a]; e2[a] = t.v[2].e[a] - t.v[0].e[a]; }
                float4* rec = c.leaf_tri.data() + ((size_t)leaf * nppl + k) * 3;
                rec[0] = make_float4(t.v[0].e[0], t.v[0].e[1], t.v[0].e[2], e1[0]);
                rec[1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
                uint32_t mesh_bits = (uint32_t)t.meshID;
                float mesh_f;
                memcpy(&mesh_f, &mesh_bits, 4);
                rec[2] = make_float4(e2[2], mesh_f, 0.0f, 0.0f);       // (.y: meshID as an integer bit pattern - a closest hit reads its record again for the normal and the material)
                cnt++;
            }
            c.leaf_ofs[leaf >> 2] |= cnt << (8 * (leaf & 3));
        }
    }
    c.materials.assign(sc.materials, sc.materials + sc.numMaterials);                          // kernels.cu:617-618
    mp.lean_ok = mesh_lean_ok(c.materials);
    for (int t = 0; t < sc.numTextures; t++) {                                                 // kernels.cu:620-645
        const rt_stexture& tx = sc.textures[t];
        c.tex.emplace_back(tx.data, tx.data + (size_t)tx.width * tx.height * 3);
        c.tex_w.push_back(tx.width);
        c.tex_h.push_back(tx.height);
    }
    return c;
}

// The host mirror of the triangles after a rebuild (rebuildBvh): slot s holds what slot from[s] held, a sentinel triangle (every coordinate inf, the rest
// zero) where from[s] < 0.
inline void permute_triangles(MeshLayout& c, const std::vector<int32_t>& from) {
    rt_triangle sentinel;
    memset(&sentinel, 0, sizeof sentinel);
    for (int v = 0; v < 3; v++) for (int a = 0; a < 3; a++) sentinel.v[v].e[a] = INFINITY;
    std::vector<rt_triangle> moved(from.size());
    for (size_t s = 0; s < from.size(); s++) moved[s] = from[s] < 0 ? sentinel : c.tris[(size_t)from[s]];
    c.tris.swap(moved);
}
