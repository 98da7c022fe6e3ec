// rt_kernels_mesh.hip — the render() hot path for TRIANGLE-MESH scenes on gfx950 (wave64).
//
// Replaces /root/reference/kernels.cu:535-569 (render), :396-533 (color), :325-360 (hit),
// :296-323 (hitMesh), :154-224 (hitBvh, DUAL_NODES), :148-152 (pop_bitstack) and :363-393
// (generateShadowRay), plus the primitive tests of intersections.h:7-41,54-104.
// Compiled twice (see rt_kernels_spheres.hip): PARITY (-ffp-contract=off: bit-exact vs the oracle, light sampling included - cosf / sinf / powf are
// glibc's algorithms restated, rt_glibc_sincosf.h / rt_glibc_powf.h) and FAST (FMA contraction).
//
// MI355X design:
//   * one lane = one pixel + its RNG stream; persistent waves, a pixel queue, and a per-lane ray-JOB state machine (closest-hit or shadow ray, same code):
//     a wave alternates between TRAVERSE (node steps for the lanes at an internal node, or (ray, triangle) pair rounds for the lanes waiting at a leaf)
//     and PROCESS (scatter, next-event estimation, Russian roulette in the reference's order for the lanes whose traversal ended);
//   * BVH child pairs are read from axis-grouped 96-byte records (per axis the four planes in both orders: the `if (invD < 0) swap` of
//     intersections.h:30 is a choice of address), three global_load_dwordx4 per node visit (the reference used a 1D texture object: kernels.cu:166-173);
//   * leaves are read as compact 48-byte records (v0 and the two edges, rounded as intersections.h:56-57 rounds them; the count of real triangles per
//     leaf in the LDS): 1.5 MB of node records + 1.7 MB of leaf records touched per frame of the benchmark tree - one XCD's L2 holds them;
//   * 1/direction is computed once per ray instead of per box per axis (intersections.h:28) - the same quotient each time, so bit-identical; the slab
//     test runs all three axes branch-free (t_min only grows, t_max only shrinks: the final `t_max < t_min` equals the per-axis early-out);
//   * a lean instantiation (template LEAN) for untextured scenes of the three basic materials: fewer registers, no (u, v) through the traversal.
#include "rt_device.h"
#include "rt_params.h"
#include "rt_mesh_plan.h"

#include <float.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <cstdio>

using namespace rtd;

#if defined(RT_MODE_PARITY)
#define RT_LAUNCH_NAME rt_launch_mesh_parity
#define RT_PIXELS_LAUNCH_NAME rt_launch_pixels_mesh_parity
#define RT_RADIANCE_LAUNCH_NAME rt_launch_radiance_mesh_parity
#elif defined(RT_MODE_FAST)
#define RT_LAUNCH_NAME rt_launch_mesh_fast
#define RT_PIXELS_LAUNCH_NAME rt_launch_pixels_mesh_fast
#define RT_RADIANCE_LAUNCH_NAME rt_launch_radiance_mesh_fast
#else
#error "define RT_MODE_PARITY or RT_MODE_FAST"
#endif

namespace {

__device__ __forceinline__ int global_row(const RtPartition& pt, int lr) {
    const int stripe = lr / pt.stripe_rows;
    return (stripe * pt.world + pt.rank) * pt.stripe_rows + (lr - stripe * pt.stripe_rows);
}

struct Tri { f3 v0, v1, v2; float tc[6]; int meshID; };

__device__ __forceinline__ Tri load_tri(const rt_triangle* tris, uint32_t id) {
    const float4* p = reinterpret_cast<const float4*>(tris + id);
    const float4 a = p[0], b = p[1], c = p[2], d = p[3];
    Tri t;
    t.v0 = F3(a.x, a.y, a.z); t.v1 = F3(a.w, b.x, b.y); t.v2 = F3(b.z, b.w, c.x);
    t.tc[0] = c.y; t.tc[1] = c.z; t.tc[2] = c.w; t.tc[3] = d.x; t.tc[4] = d.y; t.tc[5] = d.z;
    t.meshID = (int)(__float_as_uint(d.w) & 0xFFu);
    return t;
}

struct TravStats { uint32_t nodes, tests; };
typedef float f4u __attribute__((ext_vector_type(4)));

// hitBvh (DUAL_NODES), kernels.cu:154-224
__device__ __forceinline__ float hit_bvh(const RtMeshParams& P, const Ray& r, float t_min, float t_max, bool is_shadow,
                                         uint32_t& triId, float& hu, float& hv, TravStats& st) {
    int idx = 1;
    float closest = t_max;
    uint32_t bitStack = 1;
    while (idx) {
        if ((uint32_t)idx < P.first_leaf) {
            const int idx2 = idx << 1;
            const float4* n = P.bvh4 + (size_t)idx * 3;
            const float4 na = n[0], nb = n[1], nc = n[2];
            st.nodes++;
            const float leftHit = hit_bbox_dist(F3(na.x, na.y, na.z), F3(na.w, nb.x, nb.y), r, closest);
            const bool traverseLeft = leftHit < closest;
            const float rightHit = hit_bbox_dist(F3(nb.z, nb.w, nc.x), F3(nc.y, nc.z, nc.w), r, closest);
            const bool traverseRight = rightHit < closest;
            const bool swap = rightHit < leftHit;
            if (traverseLeft && traverseRight) {
                idx = idx2 + (swap ? 1 : 0);
                bitStack = (bitStack << 1) + 1;
            } else if (traverseLeft || traverseRight) {
                idx = idx2 + (swap ? 1 : 0);
                bitStack = bitStack << 1;
            } else {
                const int m = __ffs((int)bitStack) - 1;              // pop_bitstack, kernels.cu:148-152
                bitStack = (bitStack >> m) ^ 1u;
                idx = (idx >> m) ^ 1;
            }
        } else {
            const uint32_t first = ((uint32_t)idx - P.first_leaf) * P.nppl;
            for (uint32_t i = 0; i < P.nppl; i++) {
                const float4* p = reinterpret_cast<const float4*>(P.tris + first + i);
                const float4 a = p[0], b = p[1];
                if (isinf(a.x)) break;                               // kernels.cu:202 sentinel
                const float cx = p[2].x;
                float u, v;
                st.tests++;
                const float hitT = triangle_hit(F3(a.x, a.y, a.z), F3(a.w, b.x, b.y), F3(b.z, b.w, cx), r, t_min, closest, u, v);
                if (hitT < closest) {
                    if (is_shadow) return 0.0f;
                    closest = hitT;
                    triId = first + i;
                    hu = u; hv = v;
                }
            }
            const int m = __ffs((int)bitStack) - 1;
            bitStack = (bitStack >> m) ^ 1u;
            idx = (idx >> m) ^ 1;
        }
    }
    return closest;
}

// hitMesh, kernels.cu:296-323
__device__ __forceinline__ float hit_mesh(const RtMeshParams& P, const Ray& r, float t_min, float t_max, bool is_shadow,
                                          uint32_t& triId, float& hu, float& hv, TravStats& st) {
    if (!hit_bbox(ld3(P.bounds.min), ld3(P.bounds.max), r, t_max)) return FLT_MAX;
    return hit_bvh(P, r, t_min, t_max, is_shadow, triId, hu, hv, st);
}

// ---- one shading step for the kernels that nest their traversals (tile, pixel list) and the first-hit kernels (guides, rays) ------------
// The default kernel's PROCESS phase below is this code regrouped around its ray jobs; what it shares is named there.

// Nearest-texel albedo, kernels.cu:452-480: the barycentric texture coordinates of (hu, hv) on a triangle whose six are `tc`, wrapped into [0, 1).
__device__ __forceinline__ f3 mesh_texel(const RtMeshParams& P, int texId, const float* tc, float hu, float hv) {
    const float w0 = 1 - hu - hv;
    const float tcu = (hu * tc[2] + hv * tc[4] + w0 * tc[0]);
    const float tcv = (hu * tc[3] + hv * tc[5] + w0 * tc[1]);
    const int width = P.tex_width[texId];
    const int height = P.tex_height[texId];
    float tu = tcu; tu = tu - floorf(tu);
    float tv = tcv; tv = tv - floorf(tv);
    const int tx = (int)((float)(width - 1) * tu);
    const int ty = (int)((float)(height - 1) * tv);
    const int tIdx = ty * width + tx;
    const float* d = P.tex_data[texId];
    return F3(d[tIdx * 3 + 0], d[tIdx * 3 + 1], d[tIdx * 3 + 2]);
}

// What a ray met, the tail of hit() (kernels.cu:331-360) after hitMesh returned t for (t_min, t_max) - a hit iff t < t_max: the triangle (re-loaded,
// kernels.cu:334) with its geometric normal; else the floor plane (FLOOR and rt_render_options.floor; kernels.cu:341-345) against the same t_max.  The
// normal faces the ray (kernels.cu:354-355).  prim: the triangle's index in mesh.tris, RT_GUIDE_PRIM_FLOOR or RT_GUIDE_PRIM_NONE (rt_api.h).
struct MeshGeom {
    int prim;
    float t;                    // FLT_MAX unless a triangle or the floor is hit
    f3 normal;                  // (0, 0, 0) likewise
    Tri tri;                    // the triangle hit (prim >= 0 only)
};
template <bool FLOOR>
__device__ __forceinline__ MeshGeom mesh_geometry(const RtMeshParams& P, const Ray& r, float t_min, float t_max, float t, uint32_t triId) {
    MeshGeom g;
    g.t = t;
    g.normal = F3(0, 0, 0);
    g.prim = RT_GUIDE_PRIM_NONE;
    if (g.t < t_max) {
        g.tri = load_tri(P.tris, triId);
        g.normal = unit(cross(g.tri.v1 - g.tri.v0, g.tri.v2 - g.tri.v0));
        g.prim = (int)triId;
    } else {
        g.t = FLT_MAX;
        if (FLOOR && P.floor_on) g.t = plane_hit(ld3(P.floor.norm), ld3(P.floor.point), r, t_min, t_max);
        if (g.t < FLT_MAX) {
            g.normal = ld3(P.floor.norm);
            g.prim = RT_GUIDE_PRIM_FLOOR;
        }
    }
    if (g.prim != RT_GUIDE_PRIM_NONE && dot(r.d, g.normal) > 0.0f) g.normal = -g.normal;
    return g;
}

// ... for a path: a specular one that met nothing may see the light sphere (kernels.cu:346); and what the surface is made of (kernels.cu:452-482): the
// triangle's material with its texture applied, floor_diffuse_scatter (scene_materials.h:30-33) for the plane.  FLOOR = false (the tile kernel: the host
// refuses the floor with variant 1) compiles no plane test.
constexpr int kMeshPrimLight = -3;      // beside RT_GUIDE_PRIM_NONE, RT_GUIDE_PRIM_FLOOR and a triangle's index (>= 0)
struct MeshSurface {
    int prim;                   // as MeshGeom's, or kMeshPrimLight
    float t_hit;
    f3 normal, albedo;
    int mtype;
    float mparam;
};
template <bool FLOOR>
__device__ __forceinline__ MeshSurface mesh_surface(const RtMeshParams& P, const Ray& r, float t, uint32_t triId, float hu, float hv, bool specular) {
    const MeshGeom g = mesh_geometry<FLOOR>(P, r, P.t_min, FLT_MAX, t, triId);
    MeshSurface sf;
    sf.prim = g.prim; sf.t_hit = g.t; sf.normal = g.normal;
    if (g.prim == RT_GUIDE_PRIM_NONE && specular && sphere_hit(ld3(P.light.center), P.light.radius, r, P.t_min, FLT_MAX) < FLT_MAX) sf.prim = kMeshPrimLight;     // kernels.cu:346
    sf.albedo = F3(0, 0, 0); sf.mtype = RT_FLOOR_DIFFUSE; sf.mparam = 0.0f;
    if (g.prim >= 0) {
        const rt_material mat = P.materials[g.tri.meshID];
        sf.mtype = mat.type; sf.mparam = mat.param;
        if (mat.texId != -1) sf.albedo = mesh_texel(P, mat.texId, g.tri.tc, hu, hv);
        else sf.albedo = ld3(mat.color);
    }
    return sf;
}

// Per-lane path state of the kernels that nest their traversals (path, helper_structs.h:48-71).
struct MeshLane {
    uint32_t rng;
    f3 col;                     // pixel accumulator (kernels.cu:547)
    f3 org, dir, atten, pcolor;
    int bounce;
    bool inside, specular;
    int s;                      // sample index within the pixel
    int i, j;                   // global pixel coordinates
};

// kernels.cu:549-555 + the head of color() :397-398: starts sample L.s of the lane's pixel.  COUNTER = false: the caller knows the stream is the
// reference's (renderPixels refuses RT_RNG_COUNTER).
template <bool COUNTER>
__device__ __forceinline__ void start_sample(const RtMeshParams& P, MeshLane& L) {
    if (COUNTER && P.rng_mode == RT_RNG_COUNTER) L.rng = sample_seed((uint32_t)(L.j * P.nx + L.i), (uint32_t)L.s);
    const float u = ((float)L.i + rnd(L.rng)) / (float)P.nx;
    const float v = ((float)L.j + rnd(L.rng)) / (float)P.ny;
    f3 d;
    get_ray(P.cam, u, v, L.rng, L.org, d);
    L.dir = unit(d);
    L.atten = F3(1.0f, 1.0f, 1.0f);
    L.pcolor = F3(0, 0, 0);
    L.bounce = 0;
    L.inside = false;
    L.specular = false;
}

// One iteration of the loop of color(), kernels.cu:402-531, for the lane's path: closest hit, what was met, sky or light, else scatter, next-event
// estimation with its shadow traversal nested, Russian roulette, the depth bound.  True = the sample's path has ended (L.pcolor is its colour).
template <bool FLOOR>
__device__ __forceinline__ bool mesh_bounce_step(const RtMeshParams& P, MeshLane& L, TravStats& st, uint32_t& nrays, uint32_t& nshadow) {
    const float eps = P.t_min;
    // ---- hit(context, p, FLT_MAX, false, inters), kernels.cu:325-360
    const Ray r = make_ray(L.org, L.dir);
    uint32_t triId = 0;
    float hu = 0.0f, hv = 0.0f;
    nrays++;
    const float t = hit_mesh(P, r, eps, FLT_MAX, false, triId, hu, hv, st);
    const MeshSurface sf = mesh_surface<FLOOR>(P, r, t, triId, hu, hv, L.specular);
    if (sf.prim == RT_GUIDE_PRIM_NONE) {
        L.pcolor = L.pcolor + L.atten * sky_color(P.sky, L.dir);     // kernels.cu:419-425
        return true;
    }
    if (sf.prim == kMeshPrimLight) {
        if (!P.nee) L.pcolor = L.pcolor + L.atten * ld3(P.lightColor);       // kernels.cu:440-446
        return true;
    }
    Scatter sc;
    material_scatter(sc, sf.t_hit, r.o + sf.t_hit * r.d, sf.normal, L.inside, L.dir, sf.mtype, sf.albedo, sf.mparam, L.rng);
    L.org = L.org + sc.t * L.dir;                                    // kernels.cu:485-489
    L.dir = sc.wi;
    L.atten = L.atten * sc.throughput;
    L.specular = sc.specular;
    L.inside = sc.refracted ? !L.inside : L.inside;

    if (P.nee && !L.specular) {                                      // generateShadowRay, kernels.cu:363-393 (rt_device.h)
        ShadowSample sh;
        if (generate_shadow_ray(ld3(P.light.center), P.light.radius, ld3(P.lightColor), L.org, L.atten, sf.normal, L.rng, sh)) {
            const Ray sr = make_ray(L.org, sh.dir);
            uint32_t tid2 = 0; float u2, v2;
            nshadow++;
            const float ts = hit_mesh(P, sr, eps, sh.dist, true, tid2, u2, v2, st);
            if (!(ts < sh.dist)) L.pcolor = L.pcolor + sh.contrib;   // kernels.cu:504-510
        }
    }
    if (P.rr && L.bounce > 3) {                                      // kernels.cu:512-527
        const float mx = max3(L.atten);
        if (rnd(L.rng) > mx) return true;
        const float kk = 1.0f / mx;
        L.atten = F3(L.atten.x * kk, L.atten.y * kk, L.atten.z * kk);
    }
    L.bounce++;
    return L.bounce >= P.max_depth;                                  // loop bound, kernels.cu:402,529-531
}

template <int VARIANT>
__global__ void __launch_bounds__(kThreads) k_render_mesh(const RtMeshParams P) {
    __shared__ float s_fb[kThreads * 3];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i0 = (blockIdx.x * kWavesPerWg + wave) * 8;
    const int lr0 = blockIdx.y * 8;
    const int lr = lr0 + (lane >> 3);

    MeshLane L;
    L.i = i0 + (lane & 7);
    L.j = global_row(P.part, lr);
    L.rng = pixel_seed((uint32_t)(L.j * P.nx + L.i));
    L.col = F3(0, 0, 0);
    L.s = 0;
    TravStats st = { 0, 0 };
    uint32_t nrays = 0, nshadow = 0;

    bool active = (L.i < P.nx) && (lr < P.part.local_rows) && (P.ns > 0);
    if (active) start_sample<true>(P, L);

    while (active) {
        if (mesh_bounce_step<false>(P, L, st, nrays, nshadow)) {
            L.col = L.col + L.pcolor;
            L.s++;
            if (L.s < P.ns) start_sample<true>(P, L);
            else active = false;
        }
    }

    const f3 out = L.col / (float)P.ns;                              // kernels.cu:568
    float* my = s_fb + threadIdx.x * 3;
    my[0] = out.x; my[1] = out.y; my[2] = out.z;
    __syncthreads();
    const float* wfb = s_fb + wave * 192;
    float* fbf = reinterpret_cast<float*>(P.fb);
#pragma unroll
    for (int q = lane; q < 192; q += 64) {
        const int row = q / 24, off = q - row * 24;
        const int px = i0 + off / 3;
        const int rr = lr0 + row;
        if (px < P.nx && rr < P.part.local_rows)
            fbf[((size_t)rr * P.nx + i0) * 3 + off] = wfb[q];
    }

    if (P.counters) {
        atomicAdd(&P.counters->rays, (unsigned long long)nrays);
        atomicAdd(&P.counters->shadow_rays, (unsigned long long)nshadow);
        atomicAdd(&P.counters->prim_tests, (unsigned long long)st.tests);
        atomicAdd(&P.counters->node_visits, (unsigned long long)st.nodes);
    }
}

// ---- a list of pixels (renderPixels, rt_api.h) -----------------------------------------------------------------------------
// One lane = one entry of the caller's list in 256-thread workgroups of persistent waves: a lane whose pixel is finished takes the next unassigned entry -
// per refill round a wave takes ONE atomicAdd of the number of its idle lanes on B.queue and the lanes take their positions by mbcnt (the entries' costs
// differ by more than an order of magnitude).  One iteration of the wave-uniform loop is one mesh_bounce_step - the step of k_render_mesh above - for every
// lane that holds an entry, with the floor plane of rt_render_options.floor where the default kernel tests it (a ray that misses the mesh;
// kernels.cu:341-345); what is this kernel's own is the refill, the resume from B.state and the three result stores.  Not the default kernel's ray-job state
// machine: the lanes of a wave wait for its slowest traversal.  An entry that continues a stream (first > 0) loads (colour sum, xorshift word) from
// B.state instead of the pixel's seed; a finished entry stores state / out / rays from the lane that owns it.  No spin: the loop ends when the queue is
// empty and the wave's lanes are done.
constexpr int kPixelThreads = 256;
__global__ void __launch_bounds__(kPixelThreads) k_pixels_mesh(const RtMeshParams P, const RtPixelBatch B) {
    const uint32_t n = (uint32_t)B.n;

    MeshLane L;
    L.rng = 0u; L.i = 0; L.j = 0; L.s = 0; L.bounce = 0;
    L.inside = false; L.specular = false;
    L.col = F3(0, 0, 0); L.org = F3(0, 0, 0); L.dir = F3(0, 0, 1); L.atten = F3(1, 1, 1); L.pcolor = F3(0, 0, 0);
    int s_end = 0;                      // the lane's entry ends with sample s_end - 1
    TravStats st = { 0, 0 };
    uint32_t entry = 0, pix_rays = 0, nshadow = 0;
    bool active = false;                // the lane owns an unfinished entry
    bool exhausted = false;             // wave-uniform: the queue is empty

    while (true) {
        const unsigned long long idle = __ballot(!active);
        if (!exhausted && idle != 0ull) {                            // one refill round
            const uint32_t cnt = (uint32_t)__popcll(idle);
            uint32_t base = 0;
            if ((threadIdx.x & 63) == 0) base = atomicAdd(B.queue, cnt);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base + cnt >= n) exhausted = true;
            const uint32_t k = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            if (!active && k < n) {
                entry = k;
                L.i = B.ij[2 * (size_t)k]; L.j = B.ij[2 * (size_t)k + 1];
                L.s = B.first ? B.first[k] : 0;
                s_end = L.s + (B.ns ? B.ns[k] : B.ns_all);
                if (L.s > 0) {                                       // the stream continues where an earlier call stopped
                    const uint4 st4 = reinterpret_cast<const uint4*>(B.state)[k];
                    L.col = F3(__uint_as_float(st4.x), __uint_as_float(st4.y), __uint_as_float(st4.z));
                    L.rng = st4.w;
                } else {
                    L.col = F3(0, 0, 0);
                    L.rng = pixel_seed((uint32_t)(L.j * P.nx + L.i));        // kernels.cu:541 (global id -> seed)
                }
                start_sample<false>(P, L);
                pix_rays = 0;
                active = true;
            }
        }
        if (__ballot(active) == 0ull) break;
        if (active) {
            // (max_depth <= 0: the loop of kernels.cu:402 never runs: no ray, a black sample)
            if (P.max_depth <= 0 || mesh_bounce_step<true>(P, L, st, pix_rays, nshadow)) {
                L.col = L.col + L.pcolor;                            // kernels.cu:558
                L.s++;
                if (L.s < s_end) {
                    start_sample<false>(P, L);
                } else {
                    const f3 col = L.col;
                    if (B.state) reinterpret_cast<uint4*>(B.state)[entry] = make_uint4(__float_as_uint(col.x), __float_as_uint(col.y), __float_as_uint(col.z), L.rng);
                    if (B.out) {
                        const f3 out = col / (float)s_end;           // kernels.cu:568
                        *reinterpret_cast<float3*>(reinterpret_cast<float*>(B.out) + (size_t)entry * 3) = make_float3(out.x, out.y, out.z);
                    }
                    if (B.rays) B.rays[entry] = pix_rays;
                    active = false;
                }
            }
        }
    }
}

// ---- a list of the caller's own rays (radianceRays, rt_api.h) ---------------------------------------------------------------
// k_pixels_mesh above with another entry and another sample start: one lane = one ray (o, d, seed id) of the caller's list, the same persistent waves, the
// same one-atomic refill round, one mesh_bounce_step per iteration of the wave-uniform loop, the same resume from B.state and the same three stores.  An
// entry loads its origin and normalises its raw direction once (ray.h:9, the rule of traceRays); a sample starts by drawing what a camera sample draws in
// front of its path - the two jitter words (kernels.cu:549-550) and the lens's rejection loop (camera.h) - and throwing it away, then takes (o, dn) as its
// ray.  With those draws a ray is the pixel `id` of a frame through a pinhole at o that looks at o + d (rtPinholeCamera, rt_host.h), bit for bit: that frame
// is this kernel's oracle.  Nothing of the camera, the image size or the partition is read.
// kernels.cu:549-555 + the head of color() :397-398 for a caller's ray
__device__ __forceinline__ void start_ray_sample(MeshLane& L, f3 org, f3 dn) {
    (void)rnd(L.rng);                                                // the jitter of u
    (void)rnd(L.rng);                                                // ... and of v
    (void)random_in_unit_disk(L.rng);                                // the lens
    L.org = org;
    L.dir = dn;
    L.atten = F3(1.0f, 1.0f, 1.0f);
    L.pcolor = F3(0, 0, 0);
    L.bounce = 0;
    L.inside = false;
    L.specular = false;
}

__global__ void __launch_bounds__(kPixelThreads) k_radiance_mesh(const RtMeshParams P, const RtRadianceBatch B) {
    const uint32_t n = (uint32_t)B.n;

    MeshLane L;
    L.rng = 0u; L.i = 0; L.j = 0; L.s = 0; L.bounce = 0;
    L.inside = false; L.specular = false;
    L.col = F3(0, 0, 0); L.org = F3(0, 0, 0); L.dir = F3(0, 0, 1); L.atten = F3(1, 1, 1); L.pcolor = F3(0, 0, 0);
    f3 ray_org = F3(0, 0, 0), ray_dn = F3(0, 0, 1);                  // the lane's entry: every sample starts here
    int s_end = 0;                      // the lane's entry ends with sample s_end - 1
    TravStats st = { 0, 0 };
    uint32_t entry = 0, ray_rays = 0, nshadow = 0;
    bool active = false;                // the lane owns an unfinished entry
    bool exhausted = false;             // wave-uniform: the queue is empty

    while (true) {
        const unsigned long long idle = __ballot(!active);
        if (!exhausted && idle != 0ull) {                            // one refill round
            const uint32_t cnt = (uint32_t)__popcll(idle);
            uint32_t base = 0;
            if ((threadIdx.x & 63) == 0) base = atomicAdd(B.queue, cnt);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base + cnt >= n) exhausted = true;
            const uint32_t k = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            if (!active && k < n) {
                entry = k;
                L.s = B.first ? B.first[k] : 0;
                s_end = L.s + (B.ns ? B.ns[k] : B.ns_all);
                ray_org = F3(B.org[3 * (size_t)k], B.org[3 * (size_t)k + 1], B.org[3 * (size_t)k + 2]);
                ray_dn = unit(F3(B.dir[3 * (size_t)k], B.dir[3 * (size_t)k + 1], B.dir[3 * (size_t)k + 2]));     // ray.h:9
                if (L.s > 0) {                                       // the stream continues where an earlier call stopped
                    const uint4 st4 = reinterpret_cast<const uint4*>(B.state)[k];
                    L.col = F3(__uint_as_float(st4.x), __uint_as_float(st4.y), __uint_as_float(st4.z));
                    L.rng = st4.w;
                } else {
                    L.col = F3(0, 0, 0);
                    L.rng = pixel_seed(B.ids ? B.ids[k] : B.id0 + k);        // kernels.cu:541 (the caller's id -> seed)
                }
                start_ray_sample(L, ray_org, ray_dn);
                ray_rays = 0;
                active = true;
            }
        }
        if (__ballot(active) == 0ull) break;
        if (active) {
            // (max_depth <= 0: the loop of kernels.cu:402 never runs: no ray, a black sample)
            if (P.max_depth <= 0 || mesh_bounce_step<true>(P, L, st, ray_rays, nshadow)) {
                L.col = L.col + L.pcolor;                            // kernels.cu:558
                L.s++;
                if (L.s < s_end) {
                    start_ray_sample(L, ray_org, ray_dn);
                } else {
                    const f3 col = L.col;
                    if (B.state) reinterpret_cast<uint4*>(B.state)[entry] = make_uint4(__float_as_uint(col.x), __float_as_uint(col.y), __float_as_uint(col.z), L.rng);
                    if (B.out) {
                        const f3 out = col / (float)s_end;           // kernels.cu:568
                        *reinterpret_cast<float3*>(reinterpret_cast<float*>(B.out) + (size_t)entry * 3) = make_float3(out.x, out.y, out.z);
                    }
                    if (B.rays) B.rays[entry] = ray_rays;
                    active = false;
                }
            }
        }
    }
}

// ---- first-hit guide planes (renderGuides, rt_api.h) ------------------------------------------------------------------
// One lane per pixel of an 8x8 tile per wave, the grid of k_render_mesh above: the centre ray (no lens offset, no jitter) through hitMesh / hitBvh in the
// reference's own visiting order with its TravStats, so the node count of the closest-hit query is the oracle's; then the floor (rt_render_options.floor);
// normal, texture coordinates and texture lookup as bounce 0 above does them.  No atomics, no queue: a lane writes the planes of its own pixel.
// PARITY objects only: one arithmetic for both fp modes.
#if defined(RT_MODE_PARITY)
// The per-ray part, shared with the ray kernel below (traceRays, rt_api.h): hitMesh over (t_min, t_max) - a hit iff the result is below t_max -, then the
// floor (rt_render_options.floor) against the same t_max, the geometric normal and its orientation.  A miss has t = FLT_MAX and prim = RT_GUIDE_PRIM_NONE;
// hu, hv stay 0 unless a triangle is hit; st.nodes is the closest-hit query's count either way (0 for a ray that misses the scene bounds).
struct FirstHitMesh {
    float t;
    int prim;
    f3 normal;
    float hu, hv;
    Tri tri;                    // the triangle hit (prim >= 0 only)
    TravStats st;
};
__device__ __forceinline__ FirstHitMesh first_hit_mesh(const RtMeshParams& P, const Ray& r, float t_min, float t_max) {
    FirstHitMesh h;
    h.st = { 0, 0 };
    h.hu = 0.0f; h.hv = 0.0f;
    uint32_t triId = 0;
    const float t = hit_mesh(P, r, t_min, t_max, false, triId, h.hu, h.hv, h.st);
    const MeshGeom g = mesh_geometry<true>(P, r, t_min, t_max, t, triId);
    h.t = g.t;
    h.prim = g.prim;
    h.normal = g.normal;
    h.tri = g.tri;
    return h;
}

__global__ void __launch_bounds__(kThreads) k_guides_mesh(const RtMeshParams P, const RtGuidePlanes G) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i = (blockIdx.x * kWavesPerWg + wave) * 8 + (lane & 7);
    const int lr = blockIdx.y * 8 + (lane >> 3);
    if (!(i < P.nx && lr < P.part.local_rows)) return;
    const int j = global_row(P.part, lr);
    const float u = ((float)i + 0.5f) / (float)P.nx, v = ((float)j + 0.5f) / (float)P.ny;
    const f3 org = ld3(P.cam.origin);
    const f3 dir = unit(ld3(P.cam.lower_left_corner) + u * ld3(P.cam.horizontal) + v * ld3(P.cam.vertical) - org);   // camera.h:8-12, no lens offset
    const Ray r = make_ray(org, dir);                                // hit(), kernels.cu:325-360: the ray normalises the direction once more
    const FirstHitMesh h = first_hit_mesh(P, r, P.t_min, FLT_MAX);
    f3 albedo;
    if (h.prim >= 0) {
        const rt_material mat = P.materials[h.tri.meshID];           // kernels.cu:452-480
        const bool basic = mat.type == RT_DIFFUSE || mat.type == RT_METAL || mat.type == RT_GLASS;
        f3 color = ld3(mat.color);
        if (basic && mat.texId != -1) color = mesh_texel(P, mat.texId, h.tri.tc, h.hu, h.hv);
        albedo = guide_albedo(mat.type, color, r.o + h.t * r.d);
    } else if (h.prim == RT_GUIDE_PRIM_FLOOR) {
        albedo = guide_albedo(RT_FLOOR_DIFFUSE, F3(0, 0, 0), F3(0, 0, 0));          // kernels.cu:481-482
    } else {
        albedo = sky_color(P.sky, dir);                              // kernels.cu:419-425: the path's direction, normalised once
    }
    const size_t px = (size_t)lr * P.nx + i;
    if (G.albedo) { float* o = G.albedo + px * 3; o[0] = albedo.x; o[1] = albedo.y; o[2] = albedo.z; }
    if (G.normal) { float* o = G.normal + px * 3; o[0] = h.normal.x; o[1] = h.normal.y; o[2] = h.normal.z; }
    if (G.depth) G.depth[px] = h.t;
    if (G.prim) G.prim[px] = h.prim;
    if (G.nodes) G.nodes[px] = (int32_t)h.st.nodes;
}

// ---- batched ray queries (traceRays / occludedRays, rt_api.h) -------------------------------------------------------------
// One lane per caller's ray in kThreads-thread workgroups, no LDS.  The direction is the caller's raw one: make_ray normalises it once (ray.h:9).  Closest
// hit: first_hit_mesh, the guide kernel's.  ANY (occludedRays): hitMesh with is_shadow = 1, occluded iff its result is below t_max; the floor is never
// tested, as the reference's shadow rays never test it.  Incoherent lanes diverge and a wave lasts as long as its longest ray.
// Consecutive lanes read consecutive 12-byte triples of org / dir and consecutive floats of t_min / t_max, and store the same way; nothing is written
// through a null pointer.
template <bool ANY>
__global__ void __launch_bounds__(kThreads) k_rays_mesh(const RtMeshParams P, const RtRayBatch B) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= (uint32_t)B.n) return;
    const float* o = B.org + (size_t)k * 3;
    const float* d = B.dir + (size_t)k * 3;
    const Ray r = make_ray(F3(o[0], o[1], o[2]), F3(d[0], d[1], d[2]));
    const float t_min = B.t_min ? B.t_min[k] : B.t_min_default;
    const float t_max = B.t_max ? fminf(B.t_max[k], FLT_MAX) : FLT_MAX;       // a t_max above FLT_MAX (+inf) is taken as FLT_MAX (rt_api.h)
    if (ANY) {
        uint32_t triId = 0;
        float hu = 0.0f, hv = 0.0f;
        TravStats st = { 0, 0 };
        B.occluded[k] = hit_mesh(P, r, t_min, t_max, ANY, triId, hu, hv, st) < t_max ? 1 : 0;
        return;
    }
    const FirstHitMesh h = first_hit_mesh(P, r, t_min, t_max);
    if (B.t) B.t[k] = h.t;
    if (B.prim) B.prim[k] = h.prim;
    if (B.normal) { float* q = B.normal + (size_t)k * 3; q[0] = h.normal.x; q[1] = h.normal.y; q[2] = h.normal.z; }
    if (B.uv) { float* q = B.uv + (size_t)k * 2; q[0] = h.hu; q[1] = h.hv; }
    if (B.nodes) B.nodes[k] = (int32_t)h.st.nodes;
}
#endif

// ---- variant 0 (default): persistent waves, pixel queue, ray-job state machine ---------------------------------------
// The first kernel (above) nests two traversals (closest hit, then the shadow ray) inside one loop iteration and lets a
// lane whose traversal ended wait for the slowest lane of the wave: rocprof showed 17 % of the lanes active per VALU
// instruction.  Here every lane owns a JOB = one ray to traverse (closest-hit or shadow, same code) and the wave
// alternates between two phases:
//   TRAVERSE  while at least `kMinTraversing` lanes still have nodes to visit: "while-while" steps — all lanes descend
//             internal nodes together until each sits on a leaf (or is done), then all lanes test their leaf's triangles.
//             The per-lane visiting order is exactly hitBvh's (kernels.cu:154-224), only the control flow is regrouped;
//   PROCESS   the lanes whose traversal has ended consume the result (scatter + next-event estimation + Russian roulette
//             exactly in the reference's order, kernels.cu:415-527) and set up their next job: the shadow ray, the next
//             bounce, the next sample, or the next pixel from the global queue (ballot + mbcnt allocation).
// Lanes that are still traversing simply keep their state across a PROCESS phase.
// (kMinTraversing, kLeafCntLds, the workgroup's shape and the bit fields of the arguments leaf_thr and min_traversing: rt_mesh_plan.h, shared with the launcher's plan)

struct Job {
    f3 d, inv;              // unit direction and its reciprocal (ray.h:9, intersections.h:28); the ORIGIN is the path's `org`: every job of a path starts there,
                            // and `org` only moves in PROCESS, when no job is running
    int idx;                // 0 = traversal finished
    uint32_t bitStack;
    float closest;          // running closest t (t_max at start)
    uint32_t triId;
    float hu, hv;           // (only a textured material reads them: the lean instantiation does not carry them)
    bool shadow;
    uint32_t ax, ay, az;    // byte offsets of the ray's (near_L, near_R, far_L, far_R) on each axis inside a bvh_axis record
};

__device__ __forceinline__ void job_start(const RtMeshParams& P, Job& J, f3 org, f3 dir, float t_max, bool shadow) {
    const Ray r = make_ray(org, dir);
    J.d = r.d; J.inv = r.inv;
    J.shadow = shadow;
    J.closest = t_max;
    J.bitStack = 1;
    J.triId = 0; J.hu = 0.0f; J.hv = 0.0f;
    J.ax = r.inv.x < 0.0f ? 16u : 0u;                    // `if (invD < 0.0f) swap(t0, t1)`, intersections.h:30, as a choice of address
    J.ay = r.inv.y < 0.0f ? 48u : 32u;
    J.az = r.inv.z < 0.0f ? 80u : 64u;
    // hitMesh, kernels.cu:296-323: scene bounds first; a miss reports FLT_MAX
    if (hit_bbox(ld3(P.bounds.min), ld3(P.bounds.max), r, t_max)) {
        J.idx = 1;
    } else {
        J.idx = 0;
        J.closest = FLT_MAX;
    }
}

// TRAV 0: thresholded while-while (default); TRAV 1: classic while-while (all lanes descend to a leaf, then all test their leaf)
// STATS: the reference's `#ifdef STATS` counters (kernels.cu:47-67,399-561) as device atomics - the counting instantiation only.
// (Round 2 built and measured a form with TWO concurrent jobs per lane - the shadow ray beside the next bounce ray, both known
// after a diffuse hit; Russian roulette and the light sample draw in the reference's order, the shadow result is added before
// anything else: bit-exact.  One PROCESS per bounce instead of two (-31 % process steps), 33 instead of 31 lanes per node step -
// but every node step had to select the lane's job (+28 % cycles per step): 573-590 against 609 Msamples/s.  Not kept.)
// LEAN (the launcher's promise: every material is RT_DIFFUSE / RT_METAL / RT_GLASS without a texture - what scene_materials.h:13-20 at HEAD can produce -, no
// floor plane, pair rounds available): PROCESS without the preset tables, textures and the plane, no (u, v) carried through the traversal - fewer registers,
// so more waves per SIMD (RT_MESH_LEAN_WAVES) to hide the dependent node loads behind.
// (the second dispatch's scheduling constants - expensive classes and their spread, the list-0 threshold, chain lanes - are RtSwitches fields, rt_params.h)
#ifndef RT_MESH_TAIL_DIAG
#define RT_MESH_TAIL_DIAG 0
#endif
#if RT_MESH_TAIL_DIAG
__device__ uint32_t* g_diag_items;      // per pixel: (start, end) of its second-dispatch item, microseconds
#endif
// PHASE (the cost-ordered frame, rt_params.h): 0 = whole pixels in one dispatch (scattered order); 1 = samples [0, s_split) of every pixel, then park the pixel;
// 2 = resume the parked pixels in the order of P.order (longest first; since round 4 from one set of lists and counters per XCD, with 32-byte records - the sphere
// kernel's traffic forms, DESIGN.md 3.8: here they halve the reads of the parked state, the writes still leave the L2 as partial lines).  A frame ends one pixel-time after its queue runs empty, and a pixel of C4 is 1/8 of a
// lane's frame: in scattered order the 1920x1080x256 frame ran at 782 Msamples/s where the same samples as a 3840x2160x64 frame ran at 1106
// (profiles/r04_mesh_tail_probe.txt) - the expensive pixels were still running when everything else was done.
template <int TRAV, bool DBG, bool STATS, bool LEAN = false, int PHASE = 0>
__global__ void __launch_bounds__(kThreads, LEAN ? RT_MESH_LEAN_WAVES : (TRAV == 0 ? 4 : 5)) k_render_mesh_queue(const RtMeshParams P, uint32_t stride, int min_traversing, int leaf_thr) {
    const int tiles_x = (P.nx + 7) >> 3;
    const int tiles_y = (P.part.local_rows + 7) >> 3;
    const uint32_t total = (uint32_t)tiles_x * (uint32_t)tiles_y * 64u;
    const float eps = P.t_min;
#if RT_MESH_TAIL_DIAG
    const unsigned long long t_start_diag = __builtin_amdgcn_s_memrealtime();
#endif
    // leaf phase of TRAV 0: per-wave LDS scratch and this lane's fixed role in a pair round (ray j / nppl, triangle j % nppl)
    __shared__ uint32_t s_owner[kThreads];
    __shared__ unsigned long long s_best[kThreads];
    __shared__ float2 s_uv[kThreads];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* w_owner = s_owner + (threadIdx.x & ~63u);
    unsigned long long* w_best = s_best + (threadIdx.x & ~63u);
    float2* w_uv = s_uv + (threadIdx.x & ~63u);
    // (pair rounds need the compact leaf records of the host - RtMeshParams::leaf_tri / leaf_ofs, built when no leaf has a real triangle behind a sentinel)
    const int pair_per = (TRAV == 0 && P.leaf_sentinels_trailing && P.leaf_ofs != nullptr && P.leaf_tri != nullptr && P.nppl >= 1u && P.nppl <= 16u &&
                          P.first_leaf <= kLeafCntLds) ? (int)(64u / P.nppl) : 0;     // rays per pair round
    const uint32_t pair_r = pair_per ? lane / P.nppl : 0u;
    const uint32_t pair_k = pair_per ? lane - pair_r * P.nppl : 0u;
    const bool pair_ok = pair_per && (int)pair_r < pair_per;
    // Compact leaf records (rt_params.h): a pair lane reads the 48 bytes triangleHit needs (v0 and the two edges) of a REAL triangle only - the number
    // of real triangles of every leaf sits in the LDS (one byte per leaf, staged once per workgroup), so the sentinel slots of a leaf (on the
    // benchmark tree 2.8 of its 5) are never requested: 1.7 MB of triangle data touched instead of 5.2 MB.
    extern __shared__ __align__(16) unsigned char s_leaf_cnt[];
    if (pair_per > 0) {
        const uint32_t words = (P.first_leaf + 3u) >> 2;
        for (uint32_t k = threadIdx.x; k < words; k += kThreads) reinterpret_cast<uint32_t*>(s_leaf_cnt)[k] = P.leaf_ofs[k];
        __syncthreads();
    }
    const f3 lightC = ld3(P.light.center);
    const float lightR = P.light.radius;
    float* fbf = reinterpret_cast<float*>(P.fb);
    // PHASE 2 work order.  P.order holds the pixels by descending cost class.  Taken as it lies, the first fill gives every wave 64 pixels of the top class - and a
    // pixel advances one node step per step of its wave, whose time grows with the lanes that are traversing (the loads, not their latency, bound a step): a wave
    // full of long traversals makes each of them ~1.5x longer, and the frame ends with them.  So the expensive lists (the first `heavy_cls` classes: nH pixels)
    // are SPREAD evenly over the first S queue positions, S = spread_rounds x (lanes in flight): position p takes an expensive pixel iff floor((p + 1) nH / S) >
    // floor(p nH / S), else the next of the rest (also by descending cost).  (kLeafHeavyClasses and kLeafSpreadRounds of leaf_thr, from the launcher's plan.)
    // One set of lists and counters for the machine, or (P.xcd_queues, as in the sphere kernel: rt_params.h) one per XCD: a wave serves the queue of the XCD it runs
    // on - the numbers below are then those of that XCD's lists and of an eighth of the grid - and when that is empty takes what the others have left (s_mx, `stolen`).
    __shared__ uint32_t s_m[4];         // [0] nH  [1] S  [2] E  [3] chain lanes (PHASE 2; of this wave's own queue)
    __shared__ uint32_t s_mx[8 * kXcdQueues];      // per queue: [0] nH [1] S [2] E [4] first position of its lists in P.order [5] items of its general part
    const uint32_t xq = (PHASE == 2 && P.xcd_queues == kXcdQueues) ? (uint32_t)kXcdQueues : 1u;
    const uint32_t myx = xq > 1u ? ((uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) & (uint32_t)(kXcdQueues - 1)) : 0u;       // XCC_ID
    if (PHASE == 2 && threadIdx.x < xq) {
        const uint32_t* const Q = P.queue + (size_t)threadIdx.x * kXcdQueueWords;
        const uint32_t grid_x = xq > 1u ? max(gridDim.x / xq, 1u) : gridDim.x;      // workgroups that serve this queue first
        uint32_t pixels = 0;
        for (int c = 0; c < 18; c++) pixels += Q[4 + c];
        const int heavy_cls = kLeafHeavyClasses.get(leaf_thr), rounds = kLeafSpreadRounds.get(leaf_thr);
        uint32_t nH = 0;
        for (int c = 0; c < heavy_cls; c++) nH += Q[4 + c];
        // the chains: list 0 (the launcher's threshold: pixels several times the mean) goes, `chain_lanes` pixels per wave, to the first waves that ask, and those
        // waves take nothing else while these run (below); at most one wave in eight
        uint32_t chain_lanes = (uint32_t)kLeafChainLanes.get(leaf_thr);
        uint32_t E = chain_lanes ? Q[4] : 0u;
        if (E > nH) E = nH;
        if (E > (pixels >> kLeafChainFrac.get(leaf_thr))) E = 0u;
        // The chains end the frame only when a pixel of 10-20 x the mean (at about half the time per node visit of a cheap one) outlasts the whole queue, i.e. when
        // the frame is less than ~16 fills of the machine (C4: 7.9; 3840x2160: 31.6 - chain waves measured -3 % there, +12 % on C4; profiles/r04_mesh_chain_scenes.txt)
        if (kLeafChainFrac.get(leaf_thr) != 0 &&(uint32_t)P.part.local_rows * (uint32_t)P.nx > 16u * gridDim.x * blockDim.x) E = 0u;      // list 0 is not "a few pixels" in this scene (its threshold is absolute): no chain waves
        const uint32_t max_waves = grid_x * (blockDim.x >> 6) >> 3;
        if (max_waves == 0u) E = 0u;          // fewer than 8 waves serve this queue (a frame of < 16 workgroups): no chain waves, as the cap below gave before
        if (E > max_waves * chain_lanes) chain_lanes = min(64u, (E + max_waves - 1u) / max_waves);      // (a long list: more of its pixels per wave, not fewer of them in chain waves)
        if (E > max_waves * chain_lanes) E = max_waves * chain_lanes;
        const uint32_t N = pixels - E;
        nH -= E;
        uint32_t S = (uint32_t)rounds * grid_x * blockDim.x;
        if (S > N) S = N;
        if (heavy_cls == 0 || rounds == 0 || nH == 0u || nH > S || S - nH > N - nH) { nH = 0u; S = 0u; }      // (off: the lists as they lie)
        uint32_t* const sm = s_mx + 8 * threadIdx.x;
        sm[0] = nH; sm[1] = S; sm[2] = E; sm[4] = xq > 1u ? Q[3] : 0u; sm[5] = N;
        if (threadIdx.x == myx) { s_m[0] = nH; s_m[1] = S; s_m[2] = E; s_m[3] = chain_lanes; }
    }
    if (PHASE == 2) __syncthreads();
    const int chain_lanes = PHASE == 2 ? (int)s_m[3] : 0;
    leaf_thr = kLeafThr.get(leaf_thr);

    // path state (path, helper_structs.h:48-71)
    uint32_t rng = 1;
    f3 col = F3(0, 0, 0), org = F3(0, 0, 0), dir = F3(0, 0, 1), atten = F3(1, 1, 1), pcolor = F3(0, 0, 0);
    f3 pend_contrib = F3(0, 0, 0);      // lightContribution of the pending shadow ray
    float pend_dist = 0.0f;
    int bounce = 0, s = 0, pi = 0, pj = 0, lr = 0;
    bool inside = false, specular = false;
    uint32_t pixelId = 0;
    Job J;
    J.idx = 0; J.shadow = false; J.closest = FLT_MAX; J.bitStack = 1; J.triId = 0; J.hu = J.hv = 0.0f;
    J.d = F3(0, 0, 1); J.inv = F3(0, 0, 1);
    bool have_pixel = false, exhausted = false;
    TravStats st = { 0, 0 };
    uint32_t nrays = 0, nshadow = 0;
    uint32_t pix_jobs = 0;              // PHASE 1: node visits of this pixel so far: its measured cost
    const int s_end = PHASE == 1 ? P.s_split : P.ns;
    const uint32_t n_chain = PHASE == 2 ? s_m[2] : 0u;
    const uint32_t n_items = PHASE == 2 ? s_mx[8 * myx + 5] : total;      // the lists hold the valid pixels only
    const uint32_t seg_own = PHASE == 2 ? s_mx[8 * myx + 4] : 0u;          // first position of this wave's own lists in P.order
    uint32_t* const Qown = P.queue + (size_t)myx * kXcdQueueWords;
    uint32_t stolen = 0;                // (a queue per XCD) stages beyond this wave's own general queue known to be empty: stage 2k + 1 = what is left of the chain
                                        // pixels of queue (myx + k) mod 8, stage 2k + 2 = the general part of queue (myx + k + 1) mod 8
    const bool p1seg = PHASE == 1 && kMinTravSegments.get(min_traversing) != 0;     // first dispatch: the permutation moves row segments of 8 pixels (a line of px_state per 8 lanes)
    min_traversing = kMinTravLanes.get(min_traversing);
    // diagnostics (P.dbg): cycles and active lanes per phase, per wave; summed over the waves at the end
    unsigned long long g_cyc[4] = { 0, 0, 0, 0 };   // process, refill, node loop, leaf
    unsigned long long g_act[4] = { 0, 0, 0, 0 }, g_it[4] = { 0, 0, 0, 0 };   // active lanes summed over steps; steps
    const bool dbg = DBG && P.dbg != nullptr;       // DBG = false: the diagnostics (and their SGPR pressure) compile away
    constexpr bool COUNT = STATS || DBG;            // ray / node / triangle counters: only the instantiations launched when counters are asked for
    auto stat = [&](int k) { if (STATS && P.counters) atomicAdd(&P.counters->ref_stats[k], 1ull); };
    bool from_mesh = false;                         // the path's previous hit was the triangle mesh (STATS, kernels.cu:399-432)

    // A lane needs a new ray job in four places (new sample, new pixel, next bounce, shadow ray); job_start (ray set-up with
    // three IEEE divides + the scene-bounds test) is called at ONE place for all of them, after PROCESS and the refill:
    // as separate call sites a wave ran it once per place.  1 = closest-hit ray along `dir`, 2 = shadow ray along `shadow_dir`.
    int want_job = 0;
    bool need_sample = false;
    f3 shadow_dir = F3(0, 0, 1);
    auto start_sample = [&]() {                                      // kernels.cu:549-555, 397-398
        if (P.rng_mode == RT_RNG_COUNTER) rng = sample_seed(pixelId, (uint32_t)s);
        const float u = ((float)pi + rnd(rng)) / (float)P.nx;
        const float v = ((float)pj + rnd(rng)) / (float)P.ny;
        f3 d;
        get_ray(P.cam, u, v, rng, org, d);
        dir = unit(d);
        atten = F3(1.0f, 1.0f, 1.0f);
        pcolor = F3(0, 0, 0);
        bounce = 0;
        inside = false;
        specular = false;
        from_mesh = false;
        nrays++;
        stat(RT_STAT_PRIMARY);
        want_job = 1;                                               // hit(context, p, FLT_MAX, false, ...)
    };

    auto resume_pixel = [&](uint32_t pos) {                          // PHASE 2: the pixel's stream continues where the first dispatch left it
        uint32_t packed;
        float4 st4;
        if (P.ord_rec) {                                             // one 32-byte record per queue position (RtSphereParams::ord_rec)
            st4 = P.ord_rec[2 * (size_t)pos];
            packed = __float_as_uint(P.ord_rec[2 * (size_t)pos + 1].x);
        } else {
            packed = P.order[pos];
            st4 = P.ord_state[pos];
        }
        pi = (int)(packed & 0xFFFFu); lr = (int)(packed >> 16);
        pj = global_row(P.part, lr);
        pixelId = (uint32_t)(pj * P.nx + pi);
        rng = __float_as_uint(st4.w);
        col = F3(st4.x, st4.y, st4.z);
        s = P.s_split;
        have_pixel = true;
        need_sample = true;
#if RT_MESH_TAIL_DIAG
        g_diag_items[((size_t)lr * P.nx + pi) * 2] = (uint32_t)(__builtin_amdgcn_s_memrealtime() / 100ull);
#endif
    };
    // Chain waves (PHASE 2).  The frame cannot end before its most expensive pixel has traced its 250 samples one after the other (the stream is
    // sequential), and in a wave of 64 busy lanes a pixel advances only in the steps of its own kind (node / leaf) and waits through the others: measured,
    // the ~60 most expensive pixels of C4 ended 100 ms after everything else (profiles/r04_mesh_tail_diag.txt).  So the first waves to ask take `chain_lanes`
    // pixels of list 0 each and nothing else until those are done: few lanes, every step is theirs (leaf phase as soon as one lane waits, PROCESS as soon as one
    // traversal ends); then the wave joins the others at the queue.
    const int leaf_thr0 = leaf_thr, min_traversing0 = min_traversing;
    bool chain_wave = false;                                         // (wave-uniform) holds pixels of list 0 only; when they are done it joins the others
    bool chain_ask = PHASE == 2 && n_chain != 0u;                    // (asked at the first refill: a pixel is taken where the others are, after PROCESS)

    while (true) {
        // ================= PROCESS: lanes without a running traversal =======================================
        // mesh_bounce_step (above) regrouped around the ray jobs; of its pieces mesh_texel is shared.
        // kept inline: what the ray met (here from the compact leaf record the leaf test read, without texture and plane when LEAN), extraction changes the code object
        // kept inline: Russian roulette, extraction changes the code object
        unsigned long long c0 = dbg ? __builtin_amdgcn_s_memtime() : 0ull;
        if (dbg) { const int n_ = (int)__popcll(__ballot(have_pixel && J.idx == 0)); g_act[0] += (unsigned long long)n_; g_it[0] += n_ ? 1ull : 0ull; }
        if (have_pixel && J.idx == 0) {
            bool path_done = false;
            bool next_ray = false;                                   // continue the path with a new closest-hit job
            if (!J.shadow) {
                // ---- the result of hit(context, p, FLT_MAX, false, inters), kernels.cu:325-360
                const bool primary = bounce == 0;
                const float t = J.closest;
                int obj = 0;                                         // 0 none, 1 triangle mesh, 2 floor, 3 light
                float t_hit = t;
                f3 normal = F3(0, 1, 0);
                f3 albedo = F3(0, 0, 0);
                int mtype = RT_FLOOR_DIFFUSE;                        // floor_diffuse_scatter, scene_materials.h:30-33 (kernels.cu:481-482)
                float mparam = 0.0f;
                if (t < FLT_MAX) {
                    obj = 1;
                    // kernels.cu:334 re-loads the triangle.  With compact leaf records the normal and the material come from the record the leaf test read
                    // (the two edges ARE v1 - v0 and v2 - v0 as kernels.cu:336 computes them; meshID rides in the record): the caller's 64-byte array is
                    // touched only for the texture coordinates of a TEXTURED material - the traversal's working set (1.5 MB of node records + 1.7 MB of
                    // records) then fits one XCD's L2.
                    f3 e1, e2;
                    int mesh_id;
                    if (pair_per > 0) {
                        const float4* rec = P.leaf_tri + (size_t)J.triId * 3;
                        const float4 ra = rec[0], rb = rec[1], rc = rec[2];
                        e1 = F3(ra.w, rb.x, rb.y); e2 = F3(rb.z, rb.w, rc.x);
                        mesh_id = (int)(__float_as_uint(rc.y) & 0xFFu);
                    } else {
                        const Tri tri = load_tri(P.tris, J.triId);
                        e1 = tri.v1 - tri.v0; e2 = tri.v2 - tri.v0;
                        mesh_id = tri.meshID;
                    }
                    normal = unit(cross(e1, e2));
                    const rt_material mat = P.materials[mesh_id];    // kernels.cu:452-480
                    mtype = mat.type; mparam = mat.param;
                    if (!LEAN && mat.texId != -1) {
                        albedo = mesh_texel(P, mat.texId, P.tris[J.triId].texCoords, J.hu, J.hv);
                    } else {
                        albedo = ld3(mat.color);
                    }
                } else {
                    float tp = FLT_MAX;
                    Ray jr; jr.o = org; jr.d = J.d; jr.inv = J.inv;
                    if (!LEAN && P.floor_on) tp = plane_hit(ld3(P.floor.norm), ld3(P.floor.point), jr, eps, FLT_MAX);   // kernels.cu:341-345, re-enabled by rt_render_options.floor
                    if (tp < FLT_MAX) {
                        obj = 2; t_hit = tp; normal = ld3(P.floor.norm);
                    } else if (specular && sphere_hit(lightC, lightR, jr, eps, FLT_MAX) < FLT_MAX) {             // kernels.cu:346
                        obj = 3;
                    }
                }
                if (obj == 0) {
                    if (primary) stat(RT_STAT_PRIMARY_NOHITS); else stat(from_mesh ? RT_STAT_SECONDARY_MESH_NOHIT : RT_STAT_SECONDARY_NOHIT);
                    pcolor = pcolor + atten * sky_color(P.sky, dir);                                            // kernels.cu:419-425
                    path_done = true;
                } else {
                    from_mesh = obj == 1;                                                                       // kernels.cu:428-432
                    if (primary) stat(from_mesh ? RT_STAT_PRIMARY_HIT_MESH : RT_STAT_PRIMARY_NOHITS);
                    if (obj == 3) {
                        if (!P.nee) pcolor = pcolor + atten * ld3(P.lightColor);                                // kernels.cu:440-446
                        path_done = true;
                    } else {
                        if (dot(J.d, normal) > 0.0f) normal = -normal;                                          // kernels.cu:354-355
                        Scatter sc;
                        material_scatter<LEAN>(sc, t_hit, org + t_hit * J.d, normal, inside, dir, mtype, albedo, mparam, rng);
                        org = org + sc.t * dir;                      // kernels.cu:485-489
                        dir = sc.wi;
                        atten = atten * sc.throughput;
                        specular = sc.specular;
                        inside = sc.refracted ? !inside : inside;

                        bool shadow_job = false;
                        if (P.nee && !specular) {                    // generateShadowRay, kernels.cu:363-393 (rt_device.h)
                            ShadowSample sh;
                            if (generate_shadow_ray(lightC, lightR, ld3(P.lightColor), org, atten, normal, rng, sh)) {
                                pend_contrib = sh.contrib;
                                pend_dist = sh.dist;
                                nshadow++;
                                stat(RT_STAT_SHADOWS);
                                shadow_dir = sh.dir;
                                want_job = 2;                        // hit(context, p, lightDist, true, ...)
                                shadow_job = true;
                            }
                        }
                        if (!shadow_job) next_ray = true;            // falls through to Russian roulette below
                    }
                }
            } else {
                // shadow traversal finished: hitMesh returned J.closest; "hit" means closest < lightDist (kernels.cu:331,504-510)
                if (!(J.closest < pend_dist)) { pcolor = pcolor + pend_contrib; stat(RT_STAT_SHADOWS_NOHITS); }
                J.shadow = false;
                next_ray = true;
            }
            if (next_ray) {
                if (P.rr && bounce > 3) {                            // kernels.cu:512-527
                    const float mx = max3(atten);
                    if (rnd(rng) > mx) {
                        stat(RT_STAT_RUSSIAN_KILL);
                        path_done = true;
                    } else {
                        const float kk = 1.0f / mx;
                        atten = F3(atten.x * kk, atten.y * kk, atten.z * kk);
                    }
                }
                if (!path_done) {
                    bounce++;
                    if (bounce >= P.max_depth) { stat(RT_STAT_EXCEED_MAX_BOUNCE); path_done = true; }          // loop bound, kernels.cu:402,529-531
                }
                if (!path_done) {
                    nrays++;
                    stat(RT_STAT_SECONDARY);                                                                    // kernels.cu:403-408
                    if (from_mesh) stat(RT_STAT_SECONDARY_MESH);
                    if (STATS && len(atten) < 0.01f) stat(RT_STAT_LOW_POWER);
                    want_job = 1;
                }
            }
            if (STATS && path_done && (isnan(pcolor.x) || isnan(pcolor.y) || isnan(pcolor.z))) stat(RT_STAT_NAN);   // kernels.cu:559-561
            if (path_done) {
                col = col + pcolor;                                  // kernels.cu:558
                s++;
                if (s < s_end) {
                    need_sample = true;
                } else if (PHASE == 1) {                             // first samples done: park the pixel (colour sum, stream position, cost)
                    const size_t px = (size_t)lr * P.nx + pi;
                    P.px_state[px] = make_float4(col.x, col.y, col.z, __uint_as_float(rng));
                    P.px_rays[px] = (pix_jobs + 12u) / 24u;         // in the ordering pass's unit: ~150 node visits per sample are ~6 "rays" per sample (class thresholds of cost_class)
                    have_pixel = false;
                } else {
                    const f3 out = col / (float)P.ns;                // kernels.cu:568
                    // one 12-byte store (global_store_dwordx3): a lane finishes its pixel on its own, three dword stores are three partial-sector writes
                    *reinterpret_cast<float3*>(fbf + ((size_t)lr * P.nx + pi) * 3) = make_float3(out.x, out.y, out.z);
                    float4* const acc = rt_cold_arg<float4*>(offsetof(RtMeshParams, acc_state));
                    if (acc) acc[(size_t)lr * P.nx + pi] = make_float4(col.x, col.y, col.z, __uint_as_float(rng));      // a progressive pass: state for the next
                    have_pixel = false;
#if RT_MESH_TAIL_DIAG
                    if (PHASE == 2) g_diag_items[((size_t)lr * P.nx + pi) * 2 + 1] = (uint32_t)(__builtin_amdgcn_s_memrealtime() / 100ull);
#endif
                }
            }
        }

        if (dbg) { const unsigned long long c1 = __builtin_amdgcn_s_memtime(); g_cyc[0] += c1 - c0; c0 = c1; }
        // ================= refill idle lanes from the global pixel queue ======================================
        if (PHASE == 2 && chain_ask) {
            chain_ask = false;
            uint32_t c = 0;
            if ((threadIdx.x & 63) == 0) c = atomicAdd(Qown + 1, (uint32_t)chain_lanes);
            c = __builtin_amdgcn_readfirstlane(c);
            if (c < n_chain) {
                chain_wave = true;
                leaf_thr = 1; min_traversing = 63;
                const uint32_t l = threadIdx.x & 63u;
                if (l < (uint32_t)chain_lanes && c + l < n_chain) resume_pixel(seg_own + c + l);
            }
        }
        if (PHASE == 2 && chain_wave) {
            if (__ballot(have_pixel) != 0ull) goto refilled;         // a chain wave takes nothing while a chain runs
            chain_wave = false; leaf_thr = leaf_thr0; min_traversing = min_traversing0;
        }
        while (!exhausted) {
            const unsigned long long need = __ballot(!have_pixel);
            if (need == 0ull) break;
            const uint32_t cnt = (uint32_t)__popcll(need);
            uint32_t base = 0;
            if ((threadIdx.x & 63) == 0) base = atomicAdd(Qown, cnt);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= n_items) { exhausted = true; break; }
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            if (base + cnt >= n_items) exhausted = true;
#if RT_MESH_TAIL_DIAG
            if (PHASE == 2 && exhausted && (threadIdx.x & 63) == 0) atomicMin(reinterpret_cast<unsigned long long*>(P.queue + 48), __builtin_amdgcn_s_memrealtime());      // the queue ran empty
#endif
            if (!have_pixel && base + rank < n_items) {
                if (PHASE == 2) {                                    // resume: the pixel's stream continues where the first dispatch left it
                    uint32_t pos = (stride == 0xFFFFFFFFu) ? n_items - 1u - (base + rank) : base + rank;      // (stride ~0: experiment, cheapest first)
                    const uint32_t nH = s_m[0], S = s_m[1];
                    if (nH != 0u && stride != 0xFFFFFFFFu) {
                        if (pos < S) {
                            const uint32_t before = (uint32_t)(((unsigned long long)pos * nH) / S);
                            const uint32_t after = (uint32_t)(((unsigned long long)(pos + 1u) * nH) / S);
                            pos = after > before ? before : nH + (pos - before);
                        }                                            // (pos >= S: every expensive pixel is out: the rest list at nH + (pos - nH) = pos)
                    }
                    resume_pixel(seg_own + n_chain + pos);
                } else {
                const uint32_t it = base + rank;
                const uint32_t p = p1seg ? (((uint32_t)(((unsigned long long)(it >> 3) * stride) % (total >> 3)) << 3) | (it & 7u))
                                         : (uint32_t)(((unsigned long long)it * stride) % total);
                const uint32_t tile = p >> 6, within = p & 63u;
                const int ty = (int)(tile / (uint32_t)tiles_x), tx = (int)(tile - (uint32_t)ty * (uint32_t)tiles_x);
                const int i = tx * 8 + (int)(within & 7u);
                lr = ty * 8 + (int)(within >> 3);
                if (i < P.nx && lr < P.part.local_rows) {
                    pi = i; pj = global_row(P.part, lr);
                    pixelId = (uint32_t)(pj * P.nx + pi);
                    const int acc_first = PHASE == 0 ? rt_cold_arg<int32_t>(offsetof(RtMeshParams, acc_first)) : 0;
                    if (acc_first > 0) {                             // a progressive pass: the pixel's stream continues where the last pass left it
                        const float4 st4 = rt_cold_arg<const float4*>(offsetof(RtMeshParams, acc_state))[(size_t)lr * P.nx + pi];
                        rng = __float_as_uint(st4.w);
                        col = F3(st4.x, st4.y, st4.z);
                        s = acc_first;
                    } else {
                        rng = pixel_seed(pixelId);
                        col = F3(0, 0, 0);
                        s = 0;
                    }
                    pix_jobs = 0;
                    have_pixel = true;
                    need_sample = true;
                }
                }
            }
        }
        // (a queue per XCD) this wave's own queue is empty and lanes are idle: what the other stages have left - chain pixels nobody took (an XCD without a
        // workgroup of this grid has nobody to take them), then the next XCD's general part, its chain pixels, ... - as ordinary pixels
        while (PHASE == 2 && xq > 1u && exhausted && stolen + 1u < 2u * xq) {
            const unsigned long long need = __ballot(!have_pixel);
            if (need == 0ull) break;
            const uint32_t cnt = (uint32_t)__popcll(need);
            const uint32_t stage = stolen + 1u;
            const uint32_t qx = (myx + (stage >> 1)) & (uint32_t)(kXcdQueues - 1);
            const bool leftovers = (stage & 1u) != 0u;
            const uint32_t* const sm = s_mx + 8 * qx;
            const uint32_t limit = leftovers ? sm[2] : sm[5];
            uint32_t base = 0;
            if ((threadIdx.x & 63) == 0) base = atomicAdd(P.queue + (size_t)qx * kXcdQueueWords + (leftovers ? 1 : 0), cnt);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= limit) { stolen = stage; continue; }
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            if (!have_pixel && base + rank < limit) {
                uint32_t pos = base + rank;
                if (!leftovers) {
                    const uint32_t nH = sm[0], S = sm[1];
                    if (nH != 0u && pos < S) {
                        const uint32_t before = (uint32_t)(((unsigned long long)pos * nH) / S);
                        const uint32_t after = (uint32_t)(((unsigned long long)(pos + 1u) * nH) / S);
                        pos = after > before ? before : nH + (pos - before);
                    }
                    pos += sm[2];
                }
                resume_pixel(sm[4] + pos);
            }
        }
    refilled:
        if (__ballot(have_pixel) == 0ull) break;
        if (need_sample) { start_sample(); need_sample = false; }    // one site for "path ended" and "new pixel"
        if (want_job) {
            const bool sh = want_job == 2;
            job_start(P, J, org, sh ? shadow_dir : dir, sh ? pend_dist : FLT_MAX, sh);
            if (STATS && J.idx == 0) stat(sh ? RT_STAT_SHADOWS_BBOX_NOHITS : (bounce == 0 ? RT_STAT_PRIMARY_BBOX_NOHITS : RT_STAT_SECONDARY_BBOX_NOHIT));   // kernels.cu:298-301
            want_job = 0;
        }
        if (dbg) { const unsigned long long c1 = __builtin_amdgcn_s_memtime(); g_cyc[1] += c1 - c0; c0 = c1; }

        // ================= TRAVERSE ================================================================================
        // at least once; keep going while enough lanes have nodes left (the others wait for the next PROCESS phase)
        if (TRAV == 0) {
            // Thresholded while-while.  One wave step is EITHER a node step (kernels.cu:162-195) for the lanes at an
            // internal node OR the leaf loop (kernels.cu:196-214) for the lanes at a leaf.  Classic while-while runs node
            // steps until EVERY lane sits on a leaf: measured 17.7 of 64 lanes busy per node step (tools/mesh_debug.py),
            // because descents between two leaves take 1..30 steps.  Here the leaf loop runs as soon as `leaf_thr` lanes
            // wait at a leaf (or no lane is at a node): lanes waiting for the slowest descent are capped at leaf_thr.
            // Every ray still sees the reference's own sequence of node visits and triangle tests.
            // A lane without a pixel has J.idx == 0 (a pixel ends in PROCESS, where J.idx is 0, and nothing starts a job for it), so the
            // lane masks of a step are two compares of J.idx; `have_pixel` does not change inside the loop.
            const int n_have = (int)__popcll(__builtin_amdgcn_ballot_w64(have_pixel));
            bool first = true;
            for (;;) {
                // ---- node steps (kernels.cu:162-195) for the lanes at an internal node, until the leaf phase is due or the loop is left
                unsigned long long act_m, node_m;
                bool leave = false;
                int n_leaf = 0;
                for (;;) {
                    act_m = __builtin_amdgcn_ballot_w64(J.idx != 0);
                    // back to PROCESS when enough lanes have a finished traversal to consume (or nothing is left to traverse); at least one
                    // step; lanes without a pixel (end of the frame) do not count, so the tail does not bounce between the phases
                    if (act_m == 0ull || (!first && n_have - (int)__popcll(act_m) >= 64 - min_traversing)) { leave = true; break; }
                    first = false;
                    node_m = act_m & __builtin_amdgcn_ballot_w64((uint32_t)J.idx < P.first_leaf);
                    const int n_node = (int)__popcll(node_m);
                    n_leaf = (int)__popcll(act_m & ~node_m);
                    if (n_node == 0 || n_leaf >= leaf_thr) break;
                    if (dbg) { g_act[2] += (unsigned long long)n_node; g_it[2]++; }
                    const bool at_node = J.idx != 0 && (uint32_t)J.idx < P.first_leaf;
                    if (at_node) {
                        if (PHASE == 1) pix_jobs++;                  // the pixel's measured cost: node visits (rays differ little between pixels, their traversals a lot)
                        const int idx2 = J.idx << 1;
                        // child pair of node idx from its axis-grouped record (rt_params.h): per axis (near_L, near_R, far_L, far_R)
                        const char* rec = reinterpret_cast<const char*>(P.bvh_axis);
                        const uint32_t rb = __umul24((uint32_t)J.idx, 96u);
                        const f4u px = *reinterpret_cast<const f4u*>(rec + (rb + J.ax));
                        const f4u py = *reinterpret_cast<const f4u*>(rec + (rb + J.ay));
                        const f4u pz = *reinterpret_cast<const f4u*>(rec + (rb + J.az));
                        if (COUNT) st.nodes++;
                        // leftHit / rightHit of kernels.cu:175-181 are (hit ? entry : FLT_MAX); only compared, so kept as (hit, entry):
                        // `x < closest` = hit && entry < closest (closest <= FLT_MAX), `rightHit < leftHit` = as below when one side is taken.
                        // hit_bbox_dist (intersections.h:25-41) per box: t_min from 0.001f, t_max from closest, v_max / v_min updates (rt_device.h slab)
                        float le = 0.001f, re = 0.001f, lx = J.closest, rx = J.closest;
                        le = fmaxf((px.x - org.x) * J.inv.x, le); lx = fminf((px.z - org.x) * J.inv.x, lx);
                        re = fmaxf((px.y - org.x) * J.inv.x, re); rx = fminf((px.w - org.x) * J.inv.x, rx);
                        le = fmaxf((py.x - org.y) * J.inv.y, le); lx = fminf((py.z - org.y) * J.inv.y, lx);
                        re = fmaxf((py.y - org.y) * J.inv.y, re); rx = fminf((py.w - org.y) * J.inv.y, rx);
                        le = fmaxf((pz.x - org.z) * J.inv.z, le); lx = fminf((pz.z - org.z) * J.inv.z, lx);
                        re = fmaxf((pz.y - org.z) * J.inv.z, re); rx = fminf((pz.w - org.z) * J.inv.z, rx);
                        const bool hl = !(lx < le), hr = !(rx < re);
                        const bool traverseLeft = hl && le < J.closest;
                        const bool traverseRight = hr && re < J.closest;
                        const bool swap = traverseRight && (!traverseLeft || re < le);
                        if (traverseLeft || traverseRight) {
                            if (STATS) stat((traverseLeft && traverseRight) ? RT_STAT_NODES_BOTH : RT_STAT_NODES_SINGLE);   // BVH_COUNT, kernels.cu:184-191
                            J.idx = idx2 + (swap ? 1 : 0);
                            J.bitStack = (J.bitStack << 1) + ((traverseLeft && traverseRight) ? 1u : 0u);
                        } else {
                            const int m = __ffs((int)J.bitStack) - 1;    // pop_bitstack, kernels.cu:148-152
                            J.bitStack = (J.bitStack >> m) ^ 1u;
                            J.idx = (J.idx >> m) ^ 1;
                        }
                    }
                    if (dbg) { const unsigned long long c1 = __builtin_amdgcn_s_memtime(); g_cyc[2] += c1 - c0; c0 = c1; }
                }
                if (leave) break;
                const bool act = J.idx != 0;
                const bool at_node = act && (uint32_t)J.idx < P.first_leaf;
                {
                    if (dbg) { g_act[3] += (unsigned long long)n_leaf; g_it[3]++; }
                    if (pair_per > 0) {
                        // (ray, triangle) pairs: the <= leaf_thr lanes at a leaf have nppl triangles each; tested one triangle
                        // per lane and nppl steps they would keep n_leaf of 64 lanes busy.  Instead lane j of a round takes
                        // triangle j % nppl of the (j / nppl)-th waiting ray: ray fetched with ds_bpermute, result folded into
                        // the owner's slot with one 64-bit LDS atomicMin.  The reference's loop (kernels.cu:196-214) returns the
                        // lexicographic minimum of (t, k) over the triangles before the first sentinel that hit below `closest`
                        // (its running t_max only rejects what the minimum rejects too); a shadow ray stops at the FIRST k that
                        // hits.  Both are what min(key) below is, key = t_bits << 32 | k (t > 0) resp. k for shadow rays.
                        const bool at_leaf = act && !at_node;
                        const unsigned long long leaf_m = act_m & ~node_m;
                        const uint32_t my_rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(leaf_m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)leaf_m, 0u));
                        if (at_leaf) { w_owner[my_rank] = lane; w_best[lane] = ~0ull; }
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        const uint32_t packed = (uint32_t)J.idx | (J.shadow ? 0x80000000u : 0u);
                        // only FULL rounds (pair_per rays x nppl triangles fill the wave); the remaining owners keep waiting at their leaf and
                        // are served by the next leaf phase - a second round with a handful of pairs costs as much as a full one
                        // (16 owners x 5 triangles = 64 + 16 pairs was the common case).  Fewer owners than one round: all of them.
                        const int n_serve = n_leaf >= pair_per ? (n_leaf / pair_per) * pair_per : n_leaf;
                        for (int base = 0; base < n_serve; base += pair_per) {
                            const int r = base + (int)pair_r;
                            const bool pv = pair_ok && r < n_serve;
                            const uint32_t owner = pv ? w_owner[r] : lane;
                            const int src = (int)(owner << 2);
                            const float ox = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(org.x)));
                            const float oy = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(org.y)));
                            const float oz = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(org.z)));
                            const float dx = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(J.d.x)));
                            const float dy = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(J.d.y)));
                            const float dz = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(J.d.z)));
                            const float o_closest = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(J.closest)));
                            const uint32_t o_packed = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)packed);
                            const bool o_shadow = (o_packed & 0x80000000u) != 0u;
                            bool reached = false, hit = false;
                            float u = 0.0f, v = 0.0f;
                            unsigned long long key = ~0ull;
                            {
                                const uint32_t o_leaf = (o_packed & 0x7FFFFFFFu) - P.first_leaf;
                                reached = pv && pair_k < (uint32_t)s_leaf_cnt[pv ? o_leaf : 0u];     // kernels.cu:202: the loop ends at the leaf's first sentinel = after its real triangles
                                if (reached) {
                                    const float4* pt = P.leaf_tri + (size_t)(o_leaf * P.nppl + pair_k) * 3;
                                    const float4 ta = pt[0], tb = pt[1];
                                    const float tcx = pt[2].x;
                                    Ray pr;
                                    pr.o = F3(ox, oy, oz); pr.d = F3(dx, dy, dz); pr.inv = F3(0, 0, 0);
                                    const float hitT = triangle_hit_edges(F3(ta.x, ta.y, ta.z), F3(ta.w, tb.x, tb.y), F3(tb.z, tb.w, tcx), pr, eps, o_closest, u, v);
                                    hit = hitT < o_closest;
                                    if (hit) {
                                        key = o_shadow ? (unsigned long long)pair_k
                                                       : (((unsigned long long)__float_as_uint(hitT) << 32) | (unsigned long long)pair_k);
                                        atomicMin(&w_best[owner], key);
                                    }
                                }
                            }
                            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            if (pv) {
                                const unsigned long long best = w_best[owner];
                                // tests the reference executes: every reached triangle; a shadow ray stops after its first hit
                                if (COUNT && reached && (!o_shadow || best == ~0ull || (unsigned long long)pair_k <= best)) st.tests++;
                                if (!LEAN && hit && key == best) w_uv[owner] = make_float2(u, v);
                            }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        unsigned long long my_best = ~0ull;              // owner side: result of my leaf
                        float my_u = 0.0f, my_v = 0.0f;
                        const bool served = at_leaf && (int)my_rank < n_serve;
                        if (served) {
                            my_best = w_best[lane];
                            if (!LEAN) { const float2 uv = w_uv[lane]; my_u = uv.x; my_v = uv.y; }
                        }
                        if (served) {
                            if (my_best != ~0ull && J.shadow) {          // any-hit: hitBvh returns 0.0f (kernels.cu:205)
                                J.closest = 0.0f;
                                J.idx = 0;
                            } else {
                                if (my_best != ~0ull) {
                                    J.closest = __uint_as_float((uint32_t)(my_best >> 32));
                                    J.triId = ((uint32_t)J.idx - P.first_leaf) * P.nppl + (uint32_t)(my_best & 0xFFFFFFFFull);
                                    if (!LEAN) { J.hu = my_u; J.hv = my_v; }
                                }
                                const int m = __ffs((int)J.bitStack) - 1;
                                J.bitStack = (J.bitStack >> m) ^ 1u;
                                J.idx = (J.idx >> m) ^ 1;
                            }
                        }
                    } else
                    if (act && !at_node) {
                        const uint32_t first = ((uint32_t)J.idx - P.first_leaf) * P.nppl;
                        bool occluded = false;
                        for (uint32_t k = 0; k < P.nppl; k++) {
                            const float4* pt = reinterpret_cast<const float4*>(P.tris + first + k);
                            const float4 a = pt[0], b = pt[1];
                            if (isinf(a.x)) break;                       // kernels.cu:202 sentinel
                            const float cx = pt[2].x;
                            float u, v;
                            if (COUNT) st.tests++;
                            const float hitT = triangle_hit(F3(a.x, a.y, a.z), F3(a.w, b.x, b.y), F3(b.z, b.w, cx), Ray{ org, J.d, J.inv }, eps, J.closest, u, v);
                            if (hitT < J.closest) {
                                if (J.shadow) { occluded = true; break; }    // any-hit: hitBvh returns 0.0f (kernels.cu:205)
                                J.closest = hitT;
                                J.triId = first + k;
                                J.hu = u; J.hv = v;
                            }
                        }
                        if (occluded) {
                            J.closest = 0.0f;
                            J.idx = 0;
                        } else {
                            const int m = __ffs((int)J.bitStack) - 1;
                            J.bitStack = (J.bitStack >> m) ^ 1u;
                            J.idx = (J.idx >> m) ^ 1;
                        }
                    }
                    if (dbg) { const unsigned long long c1 = __builtin_amdgcn_s_memtime(); g_cyc[3] += c1 - c0; c0 = c1; }
                }
            }
        } else {
            do {
                // descend: internal nodes (kernels.cu:162-195)
                for (;;) {
                    const bool at_node = have_pixel && J.idx != 0 && (uint32_t)J.idx < P.first_leaf;
                    const unsigned long long node_m = __ballot(at_node);
                    if (node_m == 0ull) break;
                    if (dbg) { g_act[2] += (unsigned long long)__popcll(node_m); g_it[2]++; }
                    if (!at_node) continue;
                    const int idx2 = J.idx << 1;
                    const float4* n = P.bvh4 + (size_t)J.idx * 3;
                    const float4 na = n[0], nb = n[1], nc = n[2];
                    st.nodes++;
                    const float leftHit = hit_bbox_dist(F3(na.x, na.y, na.z), F3(na.w, nb.x, nb.y), Ray{ org, J.d, J.inv }, J.closest);
                    const bool traverseLeft = leftHit < J.closest;
                    const float rightHit = hit_bbox_dist(F3(nb.z, nb.w, nc.x), F3(nc.y, nc.z, nc.w), Ray{ org, J.d, J.inv }, J.closest);
                    const bool traverseRight = rightHit < J.closest;
                    const bool swap = rightHit < leftHit;
                    if (traverseLeft && traverseRight) {
                        stat(RT_STAT_NODES_BOTH);
                        J.idx = idx2 + (swap ? 1 : 0);
                        J.bitStack = (J.bitStack << 1) + 1;
                    } else if (traverseLeft || traverseRight) {
                        stat(RT_STAT_NODES_SINGLE);
                        J.idx = idx2 + (swap ? 1 : 0);
                        J.bitStack = J.bitStack << 1;
                    } else {
                        const int m = __ffs((int)J.bitStack) - 1;        // pop_bitstack, kernels.cu:148-152
                        J.bitStack = (J.bitStack >> m) ^ 1u;
                        J.idx = (J.idx >> m) ^ 1;
                    }
                }
                if (dbg) { const unsigned long long c1 = __builtin_amdgcn_s_memtime(); g_cyc[2] += c1 - c0; c0 = c1; }
                if (dbg) { g_act[3] += (unsigned long long)__popcll(__ballot(have_pixel && J.idx != 0)); g_it[3]++; }
                // leaf (kernels.cu:196-214)
                if (have_pixel && J.idx != 0) {
                    const uint32_t first = ((uint32_t)J.idx - P.first_leaf) * P.nppl;
                    bool occluded = false;
                    for (uint32_t k = 0; k < P.nppl; k++) {
                        const float4* pt = reinterpret_cast<const float4*>(P.tris + first + k);
                        const float4 a = pt[0], b = pt[1];
                        if (isinf(a.x)) break;                           // kernels.cu:202 sentinel
                        const float cx = pt[2].x;
                        float u, v;
                        st.tests++;
                        const float hitT = triangle_hit(F3(a.x, a.y, a.z), F3(a.w, b.x, b.y), F3(b.z, b.w, cx), Ray{ org, J.d, J.inv }, eps, J.closest, u, v);
                        if (hitT < J.closest) {
                            if (J.shadow) { occluded = true; break; }    // any-hit: hitBvh returns 0.0f (kernels.cu:205)
                            J.closest = hitT;
                            J.triId = first + k;
                            J.hu = u; J.hv = v;
                        }
                    }
                    if (occluded) {
                        J.closest = 0.0f;
                        J.idx = 0;
                    } else {
                        const int m = __ffs((int)J.bitStack) - 1;
                        J.bitStack = (J.bitStack >> m) ^ 1u;
                        J.idx = (J.idx >> m) ^ 1;
                    }
                }
                if (dbg) { const unsigned long long c1 = __builtin_amdgcn_s_memtime(); g_cyc[3] += c1 - c0; c0 = c1; }
            } while (__popcll(__ballot(have_pixel && J.idx != 0)) >= min_traversing);
        }
    }
#if RT_MESH_TAIL_DIAG
    if (PHASE == 2 && (threadIdx.x & 63) == 0) {                    // (diagnostic build: when did the queue run empty, when did the last wave end: tools/build_variant.sh -DRT_MESH_TAIL_DIAG=1)
        atomicMin(reinterpret_cast<unsigned long long*>(P.queue + 50), t_start_diag);
        atomicMax(reinterpret_cast<unsigned long long*>(P.queue + 52), __builtin_amdgcn_s_memrealtime());
        atomicAdd(reinterpret_cast<unsigned long long*>(P.queue + 54), __builtin_amdgcn_s_memrealtime() - t_start_diag);      // wave-time
    }
#endif
    if (dbg && (threadIdx.x & 63) == 0) {
        for (int k = 0; k < 4; k++) { atomicAdd(P.dbg + k, g_cyc[k]); atomicAdd(P.dbg + 4 + k, g_act[k]); atomicAdd(P.dbg + 8 + k, g_it[k]); }
        atomicAdd(P.dbg + 12, 1ull);
    }

    if (P.counters) {
        atomicAdd(&P.counters->rays, (unsigned long long)nrays);
        atomicAdd(&P.counters->shadow_rays, (unsigned long long)nshadow);
        atomicAdd(&P.counters->prim_tests, (unsigned long long)st.tests);
        atomicAdd(&P.counters->node_visits, (unsigned long long)st.nodes);
    }
}


}  // namespace

// One instantiation of k_render_mesh_queue, named by its template arguments: launch_mesh_queue launches it with the plan's grid and LDS and notes those
// arguments for the launch report (rtLastLaunches).  Every launch of the persistent kernel goes through it.
template <int TRAV, bool DBG, bool STATS, bool LEAN, int PHASE> struct MeshQueueForm {};

template <int TRAV, bool DBG, bool STATS, bool LEAN, int PHASE>
static hipError_t launch_mesh_queue(MeshQueueForm<TRAV, DBG, STATS, LEAN, PHASE>, const MeshPlan& pl, const RtMeshParams& q, hipStream_t stream,
                                    uint32_t stride, int min_traversing, int leaf_thr) {
    hipLaunchKernelGGL((k_render_mesh_queue<TRAV, DBG, STATS, LEAN, PHASE>), dim3(pl.grid_x), dim3(pl.threads), pl.lds, stream, q, stride, min_traversing, leaf_thr);
    rt_note_launch(RT_KERNEL_MESH_QUEUE, PHASE, TRAV, 0, (DBG ? 1 : 0) | (STATS ? 2 : 0), 0, LEAN ? 1 : 0, pl.threads, pl.grid_x);
    return hipGetLastError();
}

// The planned instantiation (TRAV, DBG, STATS, LEAN) of one dispatch (PHASE).  The classic traversal and the diagnostic and counting instantiations exist as
// single dispatches only; the lean kernel is never one of them (plan_mesh).
template <int PHASE>
static hipError_t launch_mesh_form(const MeshPlan& pl, const RtMeshParams& q, hipStream_t stream, uint32_t stride, int min_traversing, int leaf_thr) {
    auto go = [&](auto form) -> hipError_t { return launch_mesh_queue(form, pl, q, stream, stride, min_traversing, leaf_thr); };
    if constexpr (PHASE == 0) {
        if (pl.trav == 1 && pl.dbg) return go(MeshQueueForm<1, true, false, false, 0>{});
        if (pl.trav == 1 && pl.stats) return go(MeshQueueForm<1, false, true, false, 0>{});
        if (pl.trav == 1) return go(MeshQueueForm<1, false, false, false, 0>{});
    }
    if (pl.lean) return go(MeshQueueForm<0, false, false, true, PHASE>{});      // (named here, between the two: the kernels lie in the code object in the order they are named)
    if constexpr (PHASE == 0) {
        if (pl.dbg) return go(MeshQueueForm<0, true, false, false, 0>{});
        if (pl.stats) return go(MeshQueueForm<0, false, true, false, 0>{});
    }
    return go(MeshQueueForm<0, false, false, false, PHASE>{});
}

#if defined(RT_MODE_PARITY)
hipError_t rt_launch_guides_mesh(const RtMeshParams& p, const RtGuidePlanes& g, hipStream_t stream) {
    const dim3 grid((p.nx + 8 * kWavesPerWg - 1) / (8 * kWavesPerWg), (p.part.local_rows + 7) / 8);
    hipLaunchKernelGGL(k_guides_mesh, grid, dim3(kThreads), 0, stream, p, g);
    return hipGetLastError();
}
hipError_t rt_launch_rays_mesh(const RtMeshParams& p, const RtRayBatch& b, bool any, hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    const dim3 grid(((unsigned)b.n + kThreads - 1) / kThreads);
    if (any) hipLaunchKernelGGL(k_rays_mesh<true>, grid, dim3(kThreads), 0, stream, p, b);
    else hipLaunchKernelGGL(k_rays_mesh<false>, grid, dim3(kThreads), 0, stream, p, b);
    return hipGetLastError();
}
#endif

// renderPixels (rt_api.h): k_pixels_mesh over one chunk of the list, in this object's arithmetic.  Waves: four per SIMD of every CU - what stays resident -
// and never more than ceil(n / 64), so a one-pixel call is one wave; max_waves > 0 caps them.
// radianceRays takes the same launch with k_radiance_mesh: the two kernels have one structure and one launch bound.
template <typename Batch>
static hipError_t launch_list_mesh(void (*kern)(const RtMeshParams, const Batch), const RtMeshParams& p, const Batch& b, int max_waves, hipStream_t stream) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    constexpr unsigned wg_waves = kPixelThreads / 64;
    unsigned waves = std::min((unsigned)cus * 16u, ((unsigned)b.n + 63u) / 64u);
    if (max_waves > 0) waves = std::min(waves, (unsigned)max_waves);
    const dim3 grid((waves + wg_waves - 1) / wg_waves), block(64u * std::min(waves, wg_waves));
    hipLaunchKernelGGL(kern, grid, block, 0, stream, p, b);
    return hipGetLastError();
}
hipError_t RT_PIXELS_LAUNCH_NAME(const RtMeshParams& p, const RtPixelBatch& b, int max_waves, hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    if (!b.queue || !b.ij) return hipErrorInvalidValue;
    return launch_list_mesh(k_pixels_mesh, p, b, max_waves, stream);
}
hipError_t RT_RADIANCE_LAUNCH_NAME(const RtMeshParams& p, const RtRadianceBatch& b, int max_waves, hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    if (!b.queue || !b.org || !b.dir) return hipErrorInvalidValue;
    return launch_list_mesh(k_radiance_mesh, p, b, max_waves, stream);
}

#if RT_MESH_TAIL_DIAG
// The diagnostic build (tools/build_variant.sh taildiag -DRT_MESH_TAIL_DIAG=1; tools/mesh_tail_diag.py): when did the second dispatch's queue run empty, when
// did its last wave end, and the per-pixel items.  Before the second dispatch: the items' buffer (once) and the time marks in p.queue[48..56).
static uint32_t* s_diag_items = nullptr;
static void tail_diag_begin(const RtMeshParams& p, hipStream_t stream) {
    if (!s_diag_items) {
        (void)hipMalloc(&s_diag_items, (size_t)p.part.local_rows * p.nx * 8);
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_diag_items), &s_diag_items, sizeof s_diag_items);
    }
    const unsigned long long init[4] = { ~0ull, ~0ull, 0ull, 0ull };
    (void)hipMemcpyAsync(p.queue + 48, init, sizeof init, hipMemcpyHostToDevice, stream);
    (void)hipStreamSynchronize(stream);
}
// After it: the report on stderr, and the items with the first dispatch's ray counts into RT_MESH_DIAG_FILE.
static void tail_diag_end(const RtMeshParams& p, const MeshPlan& pl, const RtSwitches& sw, hipStream_t stream) {
    const size_t n_px = (size_t)p.part.local_rows * p.nx;
    const unsigned waves = pl.grid_x * (pl.threads / 64);
    unsigned long long r[4];
    unsigned list0 = 0;
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(r, p.queue + 48, sizeof r, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&list0, p.queue + 4, 4, hipMemcpyDeviceToHost);
    fprintf(stderr, "list 0: %u pixels; ", list0);
    fprintf(stderr, "mesh tail diag: queue empty at %.1f ms, last wave ends at %.1f ms, mean wave life %.1f ms (%u waves)\n", (double)(r[0] - r[1]) * 1e-5,
            (double)(r[2] - r[1]) * 1e-5, (double)r[3] * 1e-5 / (double)waves, waves);
    if (!sw.mesh_diag_file) return;
    std::vector<uint32_t> h(n_px * 3);
    (void)hipMemcpy(h.data(), s_diag_items, n_px * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(h.data() + n_px * 2, p.px_rays, n_px * 4, hipMemcpyDeviceToHost);
    FILE* f = fopen(sw.mesh_diag_file->c_str(), "wb");
    if (!f) return;
    fwrite(h.data(), 4, h.size(), f);
    fclose(f);
}
#else
static void tail_diag_begin(const RtMeshParams&, hipStream_t) {}
static void tail_diag_end(const RtMeshParams&, const MeshPlan&, const RtSwitches&, hipStream_t) {}
#endif

// What the ordering pass between the two dispatches reads (rt_params.h: rt_order_pixels_by_cost).
static RtSphereParams mesh_order_params(const RtMeshParams& p, const MeshPlan& pl) {
    RtSphereParams o;
    memset(&o, 0, sizeof o);
    o.nx = p.nx;
    o.ny = p.ny;
    o.part = p.part;
    o.s_split = pl.split;
    o.chain_top_thr = pl.chain_top_thr;
    o.px_rays = p.px_rays;
    o.px_state = p.px_state;
    o.order = p.order;
    o.ord_state = p.ord_state;
    o.ord_rays = p.ord_rays;
    o.queue = p.queue;
    o.ord_rec = p.ord_rec;
    o.xcd_queues = pl.xcd_queues;
    return o;
}

// Plans the frame (plan_mesh, rt_mesh_plan.h: `variant`, the switches, every size and scheduling constant), then issues what the plan says.
hipError_t RT_LAUNCH_NAME(const RtMeshParams& p, int variant, const RtSwitches& sw, hipStream_t stream) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const MeshPlan pl = plan_mesh(p, variant, sw, cus);
    if (pl.error != MeshPlanError::None) return hipErrorInvalidValue;
    if (pl.frame == MeshFrame::Tiles) {
        hipLaunchKernelGGL(k_render_mesh<0>, dim3(pl.grid_x, pl.grid_y), dim3(pl.threads), 0, stream, p);
        rt_note_launch(RT_KERNEL_MESH_TILES, 0, 0, 0, 0, 0, 0, pl.threads, pl.grid_x * pl.grid_y);
        return hipGetLastError();
    }
    hipError_t e = hipMemsetAsync(p.queue, 0, 64, stream);
    if (e != hipSuccess) return e;
    if (pl.frame == MeshFrame::TwoDispatch) {
        RtMeshParams q = p;
        q.s_split = pl.split;
        q.xcd_queues = pl.xcd_queues;
        if ((e = launch_mesh_form<1>(pl, q, stream, pl.stride1, pl.min_traversing1, pl.leaf_thr1)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(p.queue, 0, sizeof(uint32_t) * kXcdQueues * kXcdQueueWords, stream)) != hipSuccess) return e;
        if ((e = rt_order_pixels_by_cost(mesh_order_params(p, pl), stream)) != hipSuccess) return e;
        tail_diag_begin(p, stream);
        e = launch_mesh_form<2>(pl, q, stream, pl.stride, pl.min_traversing, pl.leaf_thr);
        tail_diag_end(p, pl, sw, stream);
        return e;
    }
    return launch_mesh_form<0>(pl, p, stream, pl.stride, pl.min_traversing, pl.leaf_thr);
}
