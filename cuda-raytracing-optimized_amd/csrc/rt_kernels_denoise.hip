// rt_kernels_denoise.hip — the preview denoiser of denoiseFrame (include/rt_api.h): an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010, the
// spatial half of SVGF) steered by the first-hit guide planes.  DESIGN.md 3.11 has the definition, the record layout and the measurements.
//
// The arithmetic is the contract (tests/denoise_reference.py restates it in numpy float32): fp32 only, + - * / max abs only, every product and sum rounded on
// its own, operands in the order written.  So this translation unit is compiled once, like the PARITY objects: -ffp-contract=off, no vectorisers, the default
// correctly rounded division and square root; fp32 denormals are kept (hipcc's default float mode for gfx9: the five squarings of the normal weight reach them).
// max(x, 0) is `x > 0 ? x : 0`: a NaN gives 0 and a zero of either sign +0, as the reference's np.where does.
//
// One lane per pixel, a wave is a 32 x 2 patch and a workgroup a 32 x 8 tile: a tap row of a wave is 512 contiguous bytes of each record plane.  No atomics, no
// LDS, no communication between workgroups; the 25 taps are unrolled and every tap is bounds-checked against the image before its address is formed.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "rt_denoise.h"

namespace {

constexpr int kTileW = 32, kTileH = 8, kDenoiseThreads = kTileW * kTileH;

__device__ __forceinline__ float max0(float x) { return x > 0.0f ? x : 0.0f; }
__device__ __forceinline__ size_t geo_at(size_t q, size_t npix) { (void)npix; return RT_DENOISE_INTERLEAVED ? 2 * q : q; }
__device__ __forceinline__ size_t pos_at(size_t q, size_t npix) { return RT_DENOISE_INTERLEAVED ? 2 * q + 1 : npix + q; }

__device__ __forceinline__ bool tile_pixel(int nx, int ny, int& i, int& j) {
    i = (int)blockIdx.x * kTileW + (int)(threadIdx.x & (kTileW - 1));
    j = (int)blockIdx.y * kTileH + (int)(threadIdx.x / kTileW);
    return i < nx && j < ny;
}

// vec3.h:194 as the guide kernels evaluate it (a / sqrt(squared_length), three divisions)
__device__ __forceinline__ void unit3(float& x, float& y, float& z) {
    const float l = __builtin_sqrtf(x * x + y * y + z * z);
    x = x / l; y = y / l; z = z / l;
}

__global__ void __launch_bounds__(kDenoiseThreads) k_denoise_prologue(const RtDenoiseParams D) {
    int i, j;
    if (!tile_pixel(D.nx, D.ny, i, j)) return;
    const size_t npix = (size_t)D.nx * (size_t)D.ny, px = (size_t)j * D.nx + i;
    // the centre ray of the guide kernels: camera.h:8-12 without the lens offset, and the ray's own normalisation on top (ray.h:9)
    const float u = ((float)i + 0.5f) / (float)D.nx, v = ((float)j + 0.5f) / (float)D.ny;
    const float* org = D.cam.origin.e;
    float d[3];
    for (int a = 0; a < 3; a++) d[a] = D.cam.lower_left_corner.e[a] + u * D.cam.horizontal.e[a] + v * D.cam.vertical.e[a] - org[a];
    unit3(d[0], d[1], d[2]);
    unit3(d[0], d[1], d[2]);
    const float t = D.depth[px];
    const int32_t prim = D.prim[px];
    const float4 geo = make_float4(D.normal[px * 3], D.normal[px * 3 + 1], D.normal[px * 3 + 2], __int_as_float(prim));
    const float4 pos = make_float4(org[0] + t * d[0], org[1] + t * d[1], org[2] + t * d[2], 1.0f / (D.sigma_z * t));
    const rt_vec3 in = D.in[px];
    float c[3] = { in.e[0], in.e[1], in.e[2] };
    if (D.flags & RT_DENOISE_DEMODULATE)
        for (int a = 0; a < 3; a++) {
            const float al = D.albedo[px * 3 + a];
            c[a] = c[a] / (al > RT_DENOISE_ALBEDO_FLOOR ? al : RT_DENOISE_ALBEDO_FLOOR);
        }
    D.rec[geo_at(px, npix)] = geo;
    D.rec[pos_at(px, npix)] = pos;
    D.col[0][px] = make_float4(c[0], c[1], c[2], 0.0f);
    if (prim == RT_GUIDE_PRIM_NONE) D.out[px] = in;         // never filtered, never a tap: the input bit for bit
}

// SQ = normal_squarings as a template argument: the tap is straight-line code.  Nothing in the tap loop branches: a tap outside the image reads the pixel's own
// records instead (a cached address) and, like a tap without a first hit, is dropped by the selects at the end, so the loads of several taps are in flight
// at once instead of one tap's geometry record deciding whether its other two records are fetched at all (the A/B: DESIGN.md 3.11).
template <bool LAST, int SQ>
__global__ void __launch_bounds__(kDenoiseThreads) k_denoise_atrous(const RtDenoiseParams D, const float4* __restrict__ src, float4* __restrict__ dst,
                                                                    const int s, const float rc) {
    int i, j;
    if (!tile_pixel(D.nx, D.ny, i, j)) return;
    const size_t npix = (size_t)D.nx * (size_t)D.ny, px = (size_t)j * D.nx + i;
    const float4 gp = D.rec[geo_at(px, npix)];
    const int32_t prim_p = __float_as_int(gp.w);
    if (prim_p == RT_GUIDE_PRIM_NONE) return;               // (its colour entry is never read: invalid pixels are no taps)
    const float4 pp = D.rec[pos_at(px, npix)];
    const float4 cp = src[px];
    const float rz = pp.w;
    const bool colour = D.sigma_c > 0.0f, same_prim = (D.flags & RT_DENOISE_SAME_PRIM) != 0;
    constexpr float K[3] = { 0.375f, 0.25f, 0.0625f };
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = K[dx < 0 ? -dx : dx] * K[dy < 0 ? -dy : dy];
            if (dx == 0 && dy == 0) {
                sx = sx + h * cp.x; sy = sy + h * cp.y; sz = sz + h * cp.z;
                wsum = wsum + h;
                continue;
            }
            const int qi = i + dx * s, qj = j + dy * s;
            const bool inside = qi >= 0 && qi < D.nx && qj >= 0 && qj < D.ny;
            const size_t q = inside ? (size_t)qj * D.nx + qi : px;
            const float4 gq = D.rec[geo_at(q, npix)];
            const float4 pq = D.rec[pos_at(q, npix)];
            const float4 cq = src[q];
            const int32_t prim_q = __float_as_int(gq.w);
            const bool ok = inside && prim_q != RT_GUIDE_PRIM_NONE;
            float wn = max0(gp.x * gq.x + gp.y * gq.y + gp.z * gq.z);
#pragma unroll
            for (int k = 0; k < SQ; k++) wn = wn * wn;
            const float ex = pq.x - pp.x, ey = pq.y - pp.y, ez = pq.z - pp.z;
            const float pd = fabsf(gp.x * ex + gp.y * ey + gp.z * ez);
            float wz = max0(1.0f - pd * rz);
            wz = wz * wz;
            float w = h * wn * wz;
            const float cx = cp.x - cq.x, cy = cp.y - cq.y, cz = cp.z - cq.z;
            const float d2 = cx * cx + cy * cy + cz * cz;
            float wc = max0(1.0f - d2 * rc);
            wc = wc * wc;
            w = colour ? w * wc : w;
            w = (same_prim && prim_p != prim_q) ? 0.0f : w;
            sx = ok ? sx + w * cq.x : sx;
            sy = ok ? sy + w * cq.y : sy;
            sz = ok ? sz + w * cq.z : sz;
            wsum = ok ? wsum + w : wsum;
        }
    }
    float r[3] = { sx / wsum, sy / wsum, sz / wsum };      // wsum >= 9/64: the centre tap
    if (!LAST) {
        dst[px] = make_float4(r[0], r[1], r[2], 0.0f);
        return;
    }
    if (D.flags & RT_DENOISE_DEMODULATE)
        for (int a = 0; a < 3; a++) {
            const float al = D.albedo[px * 3 + a];
            r[a] = r[a] * (al > RT_DENOISE_ALBEDO_FLOOR ? al : RT_DENOISE_ALBEDO_FLOOR);
        }
    rt_vec3 o;
    o.e[0] = r[0]; o.e[1] = r[1]; o.e[2] = r[2];
    D.out[px] = o;
}

dim3 tile_grid(const RtDenoiseParams& p) { return dim3((unsigned)((p.nx + kTileW - 1) / kTileW), (unsigned)((p.ny + kTileH - 1) / kTileH)); }

}  // namespace

hipError_t rt_launch_denoise_prologue(const RtDenoiseParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(k_denoise_prologue, tile_grid(p), dim3(kDenoiseThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_denoise_iteration(const RtDenoiseParams& p, int it, int last, hipStream_t stream) {
    const float4* src = p.col[it & 1];
    float4* dst = p.col[~it & 1];
    float rc = 0.0f;
    if (p.sigma_c > 0.0f) {
        const float sc = p.sigma_c * (1.0f / (float)(1 << it));     // sigma_c * 2^-it: an exact scaling (barring underflow)
        rc = 1.0f / (sc * sc);
    }
    const dim3 grid = tile_grid(p), block(kDenoiseThreads);
    const int sn = 1 << it;
#define RT_DENOISE_LAUNCH(SQ) \
    case SQ: \
        if (last) hipLaunchKernelGGL((k_denoise_atrous<true, SQ>), grid, block, 0, stream, p, src, dst, sn, rc); \
        else hipLaunchKernelGGL((k_denoise_atrous<false, SQ>), grid, block, 0, stream, p, src, dst, sn, rc); \
        break;
    switch (p.normal_squarings) {
        RT_DENOISE_LAUNCH(0) RT_DENOISE_LAUNCH(1) RT_DENOISE_LAUNCH(2) RT_DENOISE_LAUNCH(3)
        RT_DENOISE_LAUNCH(4) RT_DENOISE_LAUNCH(5) RT_DENOISE_LAUNCH(6) RT_DENOISE_LAUNCH(7)
        default: return hipErrorInvalidValue;
    }
#undef RT_DENOISE_LAUNCH
    return hipGetLastError();
}
