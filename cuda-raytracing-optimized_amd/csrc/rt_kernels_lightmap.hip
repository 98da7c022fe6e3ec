// rt_kernels_lightmap.hip — the kernels of sampleTexels / renderLightmap (include/rt_api.h, "sampling texels"): the lookup of texel planes at hits, and
// around the closest-hit ray kernel (k_rays_mesh<false>: untouched) the generator of a chunk of centre rays and the shade kernel that turns the ray kernel's
// planes into a frame.  DESIGN.md 3.33 has the reasons and the measurements.
//
// The arithmetic is the contract (rt_texel_sample.h, which the CPU twin compiles too; tests/lightmap_reference.py restates it in numpy float32): fp32 only,
// every operation rounded on its own, operands in the order written.  So this translation unit is compiled once, like the other passes': -ffp-contract=off,
// no vectorisers, the default correctly rounded division and square root, fp32 denormals kept - and with RT_MODE_PARITY, so that rt_device.h gives the centre
// ray, the albedo and the sky the forms the guide kernel and the ray kernel compile (they exist in the PARITY objects only).
//
//   k_sample_texels    one lane per hit: rt_sample_lookup; out, valid, and one atomicAdd per wave of its valid hits (an integer sum: deterministic).
//   k_lightmap_rays    one lane per pixel: k_guides_mesh's centre ray - origin, and the direction normalised once - into the ray buffers.
//   k_lightmap_shade   one lane per pixel: reads the ray and (t, prim, normal, uv), and forms what the pixel shows: the lookup at a triangle hit,
//                      floor_value at a floor hit, the sky at a miss; with RT_LIGHTMAP_ALBEDO times the albedo k_guides_mesh computes for the pixel.
// 256-thread workgroups, no LDS.  Consecutive lanes read and write consecutive entries of every per-hit array; the texel reads are as scattered as the hits'
// atlas points.  Plane indices are computed in size_t (W * H reaches 2^26, times 27 floats); chunk-local indices are below RT_RAY_CHUNK, in 32 bits.
#include "rt_device.h"
#include "rt_lightmap.h"

#define RT_SAMPLE_FN __device__ __forceinline__
#include "rt_texel_sample.h"

using namespace rtd;

namespace {

__device__ __forceinline__ bool lookup(const rt_triangle* slots, uint32_t num_slots, const RtTexelSource& S, int32_t p, float hu, float hv, const float* nrm,
                                       float* e) {
    return rt_sample_lookup(slots, num_slots, p, hu, hv, nrm, S.W, S.H, S.mode, S.bilinear, S.planes, e);
}

__global__ void __launch_bounds__(kLightmapBlock) k_sample_texels(const RtSampleParams Q) {
    const uint32_t k = blockIdx.x * (uint32_t)kLightmapBlock + threadIdx.x;
    bool ok = false;
    if (k < (uint32_t)Q.n) {
        float nrm[3] = { 0.0f, 0.0f, 0.0f }, e[3];
        if (Q.src.mode == RT_GATHER_SH9) { const float* q = Q.normal + (size_t)k * 3; nrm[0] = q[0]; nrm[1] = q[1]; nrm[2] = q[2]; }
        const float* h = Q.uv + (size_t)k * 2;
        ok = lookup(Q.slots, Q.num_slots, Q.src, Q.prim[k], h[0], h[1], nrm, e);
        float* o = Q.out + (size_t)k * 3;
        o[0] = e[0]; o[1] = e[1]; o[2] = e[2];
        if (Q.valid) Q.valid[k] = ok ? 1 : 0;
    }
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && m != 0ull) atomicAdd(Q.count, (uint32_t)__popcll(m));
}

__global__ void __launch_bounds__(kLightmapBlock) k_lightmap_rays(const RtMeshParams P, const RtLightmapParams L) {
    const uint32_t k = blockIdx.x * (uint32_t)kLightmapBlock + threadIdx.x;
    if (k >= (uint32_t)L.n) return;
    const uint32_t id = L.first + k;
    const int j = (int)(id / (uint32_t)P.nx), i = (int)(id - (uint32_t)j * (uint32_t)P.nx);
    const float u = ((float)i + 0.5f) / (float)P.nx, v = ((float)j + 0.5f) / (float)P.ny;
    const f3 org = ld3(P.cam.origin);
    const f3 dir = unit(ld3(P.cam.lower_left_corner) + u * ld3(P.cam.horizontal) + v * ld3(P.cam.vertical) - org);   // k_guides_mesh's, rtCentreRays'
    float* o = L.org + (size_t)k * 3;
    float* d = L.dir + (size_t)k * 3;
    o[0] = org.x; o[1] = org.y; o[2] = org.z;
    d[0] = dir.x; d[1] = dir.y; d[2] = dir.z;
}

// Nearest-texel albedo: mesh_texel (rt_kernels_mesh.hip) restated on the atlas point of rt_texel_sample.h, which is its first two lines; wrapped into [0, 1).
__device__ __forceinline__ f3 albedo_texel(const RtMeshParams& P, int texId, const float* tc, float hu, float hv) {
    float tcu, tcv;
    rt_sample_atlas_point(tc, hu, hv, &tcu, &tcv);
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

__global__ void __launch_bounds__(kLightmapBlock) k_lightmap_shade(const RtMeshParams P, const RtLightmapParams L) {
    const uint32_t k = blockIdx.x * (uint32_t)kLightmapBlock + threadIdx.x;
    if (k >= (uint32_t)L.n) return;
    const float* d = L.dir + (size_t)k * 3;
    const f3 dir = F3(d[0], d[1], d[2]);
    const int32_t prim = L.prim[k];
    f3 res;
    if (prim == RT_GUIDE_PRIM_NONE) {
        res = sky_color(P.sky, dir);                                 // RT_GUIDE_ALBEDO's miss value: the direction normalised once
    } else {
        f3 lit = F3(L.floor_value[0], L.floor_value[1], L.floor_value[2]);
        f3 albedo = guide_albedo(RT_FLOOR_DIFFUSE, F3(0, 0, 0), F3(0, 0, 0));
        if (prim >= 0) {
            const float* h = L.uv + (size_t)k * 2;
            const float* n = L.normal + (size_t)k * 3;
            const float hu = h[0], hv = h[1];
            const float nrm[3] = { n[0], n[1], n[2] };
            float e[3];
            lookup(P.tris, L.num_slots, L.src, prim, hu, hv, nrm, e);
            lit = F3(e[0], e[1], e[2]);
            if (L.albedo) {                                          // k_guides_mesh's albedo of a triangle hit
                const rt_triangle* tri = P.tris + prim;
                float tc[6];
#pragma unroll
                for (int q = 0; q < 6; q++) tc[q] = tri->texCoords[q];
                const rt_material mat = P.materials[tri->meshID];
                const bool basic = mat.type == RT_DIFFUSE || mat.type == RT_METAL || mat.type == RT_GLASS;
                f3 color = ld3(mat.color);
                if (basic && mat.texId != -1) color = albedo_texel(P, mat.texId, tc, hu, hv);
                const float* o = L.org + (size_t)k * 3;
                const Ray r = make_ray(F3(o[0], o[1], o[2]), dir);
                albedo = guide_albedo(mat.type, color, r.o + L.t[k] * r.d);
            }
        }
        res = L.albedo ? albedo * lit : lit;
    }
    L.out[k].e[0] = res.x; L.out[k].e[1] = res.y; L.out[k].e[2] = res.z;
}

dim3 grid_of(int32_t n) { return dim3((unsigned)(((uint32_t)n + kLightmapBlock - 1) / kLightmapBlock)); }

}  // namespace

hipError_t rt_launch_sample_texels(const RtSampleParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(k_sample_texels, grid_of(p.n), dim3(kLightmapBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_lightmap_rays(const RtMeshParams& p, const RtLightmapParams& l, hipStream_t stream) {
    hipLaunchKernelGGL(k_lightmap_rays, grid_of(l.n), dim3(kLightmapBlock), 0, stream, p, l);
    return hipGetLastError();
}

hipError_t rt_launch_lightmap_shade(const RtMeshParams& p, const RtLightmapParams& l, hipStream_t stream) {
    hipLaunchKernelGGL(k_lightmap_shade, grid_of(l.n), dim3(kLightmapBlock), 0, stream, p, l);
    return hipGetLastError();
}
