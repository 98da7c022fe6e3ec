// rt_kernels_texel_filter.hip — the kernels of filterTexels (include/rt_api.h, "filtering texels"): an edge-avoiding a-trous filter over the texel planes of a
// bake, steered by what the UV-atlas raster knows of every texel - position, geometric normal and the world footprint of a texel step.  DESIGN.md 3.32 has the
// reasons and the measurements; the skeleton is the denoiser's (rt_kernels_denoise.hip).
//
// The arithmetic is the contract (rt_texel_filter.h and rt_texel_raster.h, which the CPU twins compile too; tests/texel_filter_reference.py restates the filter
// in numpy float32): fp32 only, every operation rounded on its own, operands in the order written, correctly rounded division and square root.  So this
// translation unit is compiled once, like the other passes': -ffp-contract=off, no vectorisers, the default correctly rounded division, fp32 denormals kept.
//
//   k_filter_prologue  one lane per texel: the owner's position, normal and footprint, recomputed with the lines that claimed the texel, into two 16-byte
//                      records; an unowned texel is marked in the first (kFilterUnowned).  The values into col[0] (zeros at unowned texels: `in` is not
//                      read there).
//   k_filter_atrous    one lane per texel, one launch per iteration; a wave is a 32 x 2 patch and a workgroup a 32 x 8 tile, so a tap row of a wave is 512
//                      contiguous bytes of each record plane.  The 25 taps are unrolled, every tap is bounds-checked before its address is formed, a tap
//                      outside the atlas reads the texel's own records and, like an unowned one or one out of reach, is removed by the selects at the end.
//                      normal_squarings and the layout of the values are template arguments: the tap loop is straight-line code.  C = 27 runs as nine
//                      launches of three channels, each recomputing the weight - which does not depend on the channel, so the bits are those of 27
//                      accumulators -: 27 accumulators do not fit the 64 registers of 8 waves per SIMD.  The leading group, and every group without the
//                      colour weight, is the C = 3 kernel on that group's plane; the other eight read the leading group's values for the colour weight
//                      beside their own (kLead).
//   k_filter_scatter   one lane per texel: out(t) = the filtered value of src(t), zeros where src(t) == -1.
// No atomics, no LDS, no communication between workgroups.  The grids cover the atlas: at most 256 x 1024 workgroups, (W*H + 255) / 256 <= 2^18 for the
// per-texel kernels.  Plane indices are computed in size_t (W * H reaches 2^26, times 27 floats).
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <stdint.h>

#define RT_TEXEL_FN __device__ __forceinline__
#define RT_FILTER_FN __host__ __device__ __forceinline__
#include "rt_texel_raster.h"
#include "rt_texel_filter.h"
#include "rt_texel_filter_launch.h"

namespace {

constexpr int kFilterBlock = 256;                       // texels per workgroup of the per-texel kernels
constexpr int kTileW = 32, kTileH = 8, kTileThreads = kTileW * kTileH;
// The layout of the values (rt_texel_filter_launch.h): one float, one float4, and one float4 whose colour weight is that of another plane.
enum { kOne = 0, kThree = 1, kLead = 2 };

__global__ void __launch_bounds__(kFilterBlock) k_filter_prologue(const RtTexelFilterParams F) {
    const size_t n = (size_t)F.W * F.H, t = (size_t)blockIdx.x * kFilterBlock + threadIdx.x;
    if (t >= n) return;
    const int32_t o = F.owner[t];
    const bool owned = o != INT32_MAX;
    float pos[3] = { 0.0f, 0.0f, 0.0f }, nrm[3] = { 0.0f, 0.0f, 0.0f }, r2 = __uint_as_float(kFilterUnowned), rz = 0.0f;
    if (owned) {
        const rt_triangle* tri = F.slots + o;
        float tc[6], box[4], s[2], h[2] = { 0.0f, 0.0f };
#pragma unroll
        for (int i = 0; i < 6; i++) tc[i] = tri->texCoords[i];
        rt_texel_box(tc, box);
        rt_texel_sample((int)(t % (size_t)F.W), (int)(t / (size_t)F.W), F.W, F.H, s);
        rt_texel_cover(tc, box, s, h);
        rt_texel_resolve(tri, h, pos, nrm);
        rt_filter_footprint(tri, F.W, F.H, F.sigma_d, F.sigma_z, &r2, &rz);
        if (r2 != r2) r2 = __uint_as_float(0x7fc00000u);    // (any NaN fails every reach test; this one is not the mark)
    }
    F.rec[t] = make_float4(nrm[0], nrm[1], nrm[2], r2);
    F.rec[n + t] = make_float4(pos[0], pos[1], pos[2], rz);
    if (F.C == 1) {
        reinterpret_cast<float*>(F.col[0])[t] = owned ? F.in[t] : 0.0f;
    } else {
        float4* col = reinterpret_cast<float4*>(F.col[0]);
        const int groups = F.C / 3;
        for (int g = 0; g < groups; g++) {
            const size_t at = t * (size_t)F.C + 3 * (size_t)g;
            col[(size_t)g * n + t] = owned ? make_float4(F.in[at], F.in[at + 1], F.in[at + 2], 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

template <int KIND>
__device__ __forceinline__ void load_values(const void* plane, size_t q, float* c) {
    if (KIND == kOne) {
        c[0] = reinterpret_cast<const float*>(plane)[q]; c[1] = 0.0f; c[2] = 0.0f;
    } else {
        const float4 v = reinterpret_cast<const float4*>(plane)[q];
        c[0] = v.x; c[1] = v.y; c[2] = v.z;
    }
}

// SQ = normal_squarings, KIND = the layout of the values.  `src` and `dst` are the planes of the group this launch filters, `lead` that of the leading
// group (kLead: the colour weight's, and sigma_c > 0; otherwise unused).  Nothing in the tap loop branches.
template <int SQ, int KIND>
__global__ void __launch_bounds__(kTileThreads) k_filter_atrous(const RtTexelFilterParams F, const void* __restrict__ src, const void* __restrict__ lead,
                                                                void* __restrict__ dst, const int s, const float rc) {
    const int x = (int)blockIdx.x * kTileW + (int)(threadIdx.x & (kTileW - 1));
    const int y = (int)blockIdx.y * kTileH + (int)(threadIdx.x / kTileW);
    if (x >= F.W || y >= F.H) return;
    const size_t n = (size_t)F.W * (size_t)F.H, px = (size_t)y * F.W + x;
    const float4 gp = F.rec[px];
    if (__float_as_uint(gp.w) == kFilterUnowned) return;    // (its values are never read: an unowned texel is no tap and no source)
    const float4 pp = F.rec[n + px];
    constexpr int CH = KIND == kOne ? 1 : 3;
    const float np[3] = { gp.x, gp.y, gp.z }, Pp[3] = { pp.x, pp.y, pp.z };
    const float r2 = gp.w, rz = pp.w;
    const bool colour = F.sigma_c > 0.0f;
    float cp[3], lp[3] = { 0.0f, 0.0f, 0.0f };
    load_values<KIND>(src, px, cp);
    if (KIND == kLead) load_values<KIND>(lead, px, lp);
    const int ss = s * s;
    float sum[3] = { 0.0f, 0.0f, 0.0f }, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = rt_filter_kernel(dx, dy);
            if (dx == 0 && dy == 0) {
#pragma unroll
                for (int j = 0; j < CH; j++) sum[j] = sum[j] + h * cp[j];
                wsum = wsum + h;
                continue;
            }
            const int qx = x + dx * s, qy = y + dy * s;
            const bool inside = qx >= 0 && qx < F.W && qy >= 0 && qy < F.H;
            const size_t q = inside ? (size_t)qy * F.W + qx : px;
            const float4 gq = F.rec[q];
            const float4 pq = F.rec[n + q];
            float cq[3], lq[3];
            load_values<KIND>(src, q, cq);
            if (KIND == kLead) load_values<KIND>(lead, q, lq);
            const float nq[3] = { gq.x, gq.y, gq.z }, Pq[3] = { pq.x, pq.y, pq.z };
            float w;
            const bool reach = rt_filter_tap(np, Pp, r2, rz, nq, Pq, h, (float)((dx * dx + dy * dy) * ss), SQ, &w);
            const bool ok = inside && __float_as_uint(gq.w) != kFilterUnowned && reach;
            const float wc = KIND == kLead ? rt_filter_colour(lp, lq, 3, rc) : rt_filter_colour(cp, cq, CH, rc);
            w = colour ? w * wc : w;
#pragma unroll
            for (int j = 0; j < CH; j++) sum[j] = ok ? sum[j] + w * cq[j] : sum[j];
            wsum = ok ? wsum + w : wsum;
        }
    }
    if (KIND == kOne) {
        reinterpret_cast<float*>(dst)[px] = sum[0] / wsum;                  // wsum >= 9/64: the centre tap
    } else {
        reinterpret_cast<float4*>(dst)[px] = make_float4(sum[0] / wsum, sum[1] / wsum, sum[2] / wsum, 0.0f);
    }
}

__global__ void __launch_bounds__(kFilterBlock) k_filter_scatter(const RtTexelFilterParams F, const void* __restrict__ fin) {
    const size_t n = (size_t)F.W * F.H, t = (size_t)blockIdx.x * kFilterBlock + threadIdx.x;
    if (t >= n) return;
    const int32_t s = F.src[t];
    if (F.C == 1) {
        F.out[t] = s < 0 ? 0.0f : reinterpret_cast<const float*>(fin)[s];
        return;
    }
    const float4* col = reinterpret_cast<const float4*>(fin);
    const int groups = F.C / 3;
    for (int g = 0; g < groups; g++) {
        const float4 v = s < 0 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : col[(size_t)g * n + (size_t)s];
        const size_t at = t * (size_t)F.C + 3 * (size_t)g;
        F.out[at] = v.x; F.out[at + 1] = v.y; F.out[at + 2] = v.z;
    }
}

inline unsigned texel_blocks(const RtTexelFilterParams& p) { return (unsigned)(((size_t)p.W * p.H + kFilterBlock - 1) / kFilterBlock); }

// Group g of iteration `it` (g = 0 where the values are one plane).
template <int KIND>
hipError_t launch_iteration(const RtTexelFilterParams& p, int it, int g, hipStream_t stream) {
    const size_t at = (size_t)g * ((size_t)p.W * p.H);
    const void* lead = p.col[it & 1];
    const void* src = KIND == kOne ? lead : (const void*)(reinterpret_cast<const float4*>(lead) + at);
    void* dst = KIND == kOne ? p.col[~it & 1] : (void*)(reinterpret_cast<float4*>(p.col[~it & 1]) + at);
    const float rc = rt_filter_rc(p.sigma_c, it);
    const dim3 grid((unsigned)((p.W + kTileW - 1) / kTileW), (unsigned)((p.H + kTileH - 1) / kTileH)), block(kTileThreads);
    const int s = 1 << it;
#define RT_FILTER_LAUNCH(SQ) \
    case SQ: hipLaunchKernelGGL((k_filter_atrous<SQ, KIND>), grid, block, 0, stream, p, src, lead, dst, s, rc); break;
    switch (p.normal_squarings) {
        RT_FILTER_LAUNCH(0) RT_FILTER_LAUNCH(1) RT_FILTER_LAUNCH(2) RT_FILTER_LAUNCH(3)
        RT_FILTER_LAUNCH(4) RT_FILTER_LAUNCH(5) RT_FILTER_LAUNCH(6) RT_FILTER_LAUNCH(7)
        default: return hipErrorInvalidValue;
    }
#undef RT_FILTER_LAUNCH
    return hipGetLastError();
}

}  // namespace

hipError_t rt_launch_texel_filter_prologue(const RtTexelFilterParams& p, hipStream_t stream) {
    if (p.C != 1 && p.C != 3 && p.C != 27) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_filter_prologue, dim3(texel_blocks(p)), dim3(kFilterBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_texel_filter_iteration(const RtTexelFilterParams& p, int it, hipStream_t stream) {
    if (it < 0 || it >= RT_DENOISE_MAX_ITERATIONS) return hipErrorInvalidValue;
    switch (p.C) {
        case 1: return launch_iteration<kOne>(p, it, 0, stream);
        case 3: return launch_iteration<kThree>(p, it, 0, stream);
        case 27:
            for (int g = 0; g < 9; g++) {
                const hipError_t e = g > 0 && p.sigma_c > 0.0f ? launch_iteration<kLead>(p, it, g, stream) : launch_iteration<kThree>(p, it, g, stream);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        default: return hipErrorInvalidValue;
    }
}

hipError_t rt_launch_texel_filter_scatter(const RtTexelFilterParams& p, int iterations, hipStream_t stream) {
    hipLaunchKernelGGL(k_filter_scatter, dim3(texel_blocks(p)), dim3(kFilterBlock), 0, stream, p, (const void*)p.col[iterations & 1]);
    return hipGetLastError();
}
