// rt_kernels_preview.hip — the kernels of previewFrame (include/rt_api.h): the temporal accumulation of accumulateFrame extended by the first two moments of
// the luminance, the per-pixel variance from them (from the 7 x 7 neighbourhood where the history is short) and the a-trous filter of denoiseFrame with that
// variance as its colour width, carried from iteration to iteration (SVGF, Schied et al. 2017, without the feedback of filtered colour and without the
// variance pre-blur).  DESIGN.md 3.13 has the definition, the record layout and the measurements.
//
// The arithmetic is the contract (tests/preview_reference.py restates it in numpy float32): fp32 only, + - * / abs floor min max sqrt only, every product and
// sum rounded on its own, operands in the order written, a comparison with a NaN false.  So this translation unit is compiled once, like the denoiser's:
// -ffp-contract=off, no vectorisers, the default correctly rounded division and square root, fp32 denormals kept.  The constants of the previous camera are
// computed by the launcher below, on the host, under the same flags.  max(x, 0) is `x > 0 ? x : 0`: a NaN gives 0 and a zero of either sign +0.
//
// One lane per pixel, a wave a 32 x 2 patch and a workgroup a 32 x 8 tile, as the two passes this one fuses.  No atomics, no LDS, no communication between
// workgroups.  The taps are straight-line code: their records are loaded first, then tested with selects; a tap's address is formed from an index that is
// inside the image, or it is the pixel's own.  The helpers the other two passes have as well are restated here, not shared (DESIGN.md 3.12 "Not shared").
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "rt_preview.h"

namespace {

constexpr int kTileW = 32, kTileH = 8, kPreviewThreads = kTileW * kTileH;

__host__ __device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ float max0(float x) { return x > 0.0f ? x : 0.0f; }
__device__ __forceinline__ float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

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

// Stage T.  k_accumulate's reprojection and taps with two more accumulated quantities, the moments of the luminance; a tap reads the 8-byte moment record
// beside its three 16-byte ones.  MOTION: a pose is marked (rtMarkPose) - the reprojection and the taps' plane and normal tests take Pm(p), nm(p) of the
// motion planes (rt_motion.h) in the place of P(p), n(p), as k_accumulate's; MOTION = false is the kernel as it was.
template <bool HIST, bool MOTION>
__global__ void __launch_bounds__(kPreviewThreads) k_preview_temporal(const RtPreviewParams D) {
    int i, j;
    if (!tile_pixel(D.nx, D.ny, i, j)) return;
    const size_t npix = (size_t)D.nx * (size_t)D.ny, px = (size_t)j * D.nx + i;
    const rt_vec3 in = D.in[px];
    const int32_t prim = D.prim[px];
    const float t = D.depth[px];
    const float n[3] = { D.normal[px * 3], D.normal[px * 3 + 1], D.normal[px * 3 + 2] };
    // the centre ray of the guide kernels: camera.h:8-12 without the lens offset, and the ray's own normalisation on top (ray.h:9)
    const float u = ((float)i + 0.5f) / (float)D.nx, v = ((float)j + 0.5f) / (float)D.ny;
    const float* org = D.cam.origin.e;
    float d[3];
    for (int a = 0; a < 3; a++) d[a] = D.cam.lower_left_corner.e[a] + u * D.cam.horizontal.e[a] + v * D.cam.vertical.e[a] - org[a];
    unit3(d[0], d[1], d[2]);
    unit3(d[0], d[1], d[2]);
    const float P[3] = { org[0] + t * d[0], org[1] + t * d[1], org[2] + t * d[2] };
    const bool valid = prim != RT_GUIDE_PRIM_NONE;
    float c[3] = { in.e[0], in.e[1], in.e[2] };
    if (D.flags & RT_DENOISE_DEMODULATE)
        for (int a = 0; a < 3; a++) {
            const float al = D.albedo[px * 3 + a];
            c[a] = c[a] / (al > RT_DENOISE_ALBEDO_FLOOR ? al : RT_DENOISE_ALBEDO_FLOOR);
        }
    const float l0 = lum(c[0], c[1], c[2]), q0 = l0 * l0;
    float N = valid ? 1.0f : 0.0f, M1 = l0, M2 = q0;
    if (HIST) {
        const float rz = 1.0f / (D.sigma_z * t);
        const bool same_prim = (D.flags & RT_DENOISE_SAME_PRIM) != 0;
        float Pm[3] = { P[0], P[1], P[2] }, nm[3] = { n[0], n[1], n[2] };
        if (MOTION) {
            const float4 mp = D.motion[px], mn = D.motion[npix + px];
            Pm[0] = mp.x; Pm[1] = mp.y; Pm[2] = mp.z;
            nm[0] = mn.x; nm[1] = mn.y; nm[2] = mn.z;
        }
        const float e[3] = { Pm[0] - D.prev_origin.e[0], Pm[1] - D.prev_origin.e[1], Pm[2] - D.prev_origin.e[2] };
        const float ea = dot3(e, D.prev_u.e), eb = dot3(e, D.prev_v.e), ec = dot3(e, D.prev_w.e);
        const float r = D.Lw / ec;
        const float s = (ea * r - D.Lu) / D.Hl, tt = (eb * r - D.Lv) / D.Vl;
        const float x = s * (float)D.nx - 0.5f, y = tt * (float)D.ny - 0.5f;
        const bool candidate = valid && r > 0.0f && x >= -1.0f && x < (float)D.nx && y >= -1.0f && y < (float)D.ny;
        // x and y can be anything (NaN, infinite, beyond int) unless `candidate`: only then they become indices
        const float x0 = candidate ? floorf(x) : 0.0f, y0 = candidate ? floorf(y) : 0.0f;
        const float fx = x - x0, fy = y - y0;
        const int i0 = (int)x0, j0 = (int)y0;                  // -1 .. nx - 1, -1 .. ny - 1
        bool inside[4];
        float4 pq[4], gq[4], cq[4];
        float2 mq[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int qi = i0 + (k & 1), qj = j0 + (k >> 1);
            inside[k] = (qi >= 0) & (qi < D.nx) & (qj >= 0) & (qj < D.ny);
            const size_t q = inside[k] ? (size_t)qj * D.nx + qi : px;
            pq[k] = D.prev[q];
            gq[k] = D.prev[npix + q];
            cq[k] = D.prev[2 * npix + q];
            mq[k] = D.prev_mom[q];
        }
        float sum[3] = { 0.0f, 0.0f, 0.0f }, nsum = 0.0f, wsum = 0.0f, m1sum = 0.0f, m2sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {                           // dy = k >> 1 (outer), dx = k & 1 (inner)
            const float bw = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
            const float ex = pq[k].x - Pm[0], ey = pq[k].y - Pm[1], ez = pq[k].z - Pm[2];
            const float pd = fabsf(nm[0] * ex + nm[1] * ey + nm[2] * ez) * rz;
            const float dn = nm[0] * gq[k].x + nm[1] * gq[k].y + nm[2] * gq[k].z;
            const bool other_prim = same_prim & (prim != __float_as_int(gq[k].w));
            const bool ok = inside[k] & (pq[k].w > 0.0f) & (pd < 1.0f) & (dn >= D.normal_min) & !other_prim;
            sum[0] = ok ? sum[0] + bw * cq[k].x : sum[0];
            sum[1] = ok ? sum[1] + bw * cq[k].y : sum[1];
            sum[2] = ok ? sum[2] + bw * cq[k].z : sum[2];
            nsum = ok ? nsum + bw * pq[k].w : nsum;
            wsum = ok ? wsum + bw : wsum;
            m1sum = ok ? m1sum + bw * mq[k].x : m1sum;
            m2sum = ok ? m2sum + bw * mq[k].y : m2sum;
        }
        if (candidate && wsum > 0.0f) {
            const float len = nsum / wsum + 1.0f;
            N = len < D.max_history ? len : D.max_history;
            const float al = 1.0f / N;
            for (int a = 0; a < 3; a++) {
                const float h = sum[a] / wsum;
                c[a] = h + al * (c[a] - h);
            }
            const float h1 = m1sum / wsum, h2 = m2sum / wsum;
            M1 = h1 + al * (l0 - h1);
            M2 = h2 + al * (q0 - h2);
        }
    }
    D.next[px] = make_float4(P[0], P[1], P[2], N);
    D.next[npix + px] = make_float4(n[0], n[1], n[2], __int_as_float(prim));
    D.next[2 * npix + px] = make_float4(c[0], c[1], c[2], 0.0f);
    D.next_mom[px] = make_float2(M1, M2);
    if (D.history) D.history[px] = N;
    if (!valid) D.out[px] = in;                                 // never filtered, never a tap: the input bit for bit
}

// Stage V.  Where the history is long enough the variance is M2 - M1^2 of the pixel's own moments; the 49 taps of the spatial estimate sit behind a
// wave-uniform branch that a wave takes only when one of its lanes has N < RT_PREVIEW_MIN_HISTORY (every wave on a first call, the disoccluded rims later).
// A row of seven taps is straight-line code, the seven rows a loop.
template <int SQ>
__global__ void __launch_bounds__(kPreviewThreads) k_preview_variance(const RtPreviewParams D) {
    int i, j;
    if (!tile_pixel(D.nx, D.ny, i, j)) return;
    const size_t npix = (size_t)D.nx * (size_t)D.ny, px = (size_t)j * D.nx + i;
    const float4 pp = D.next[px];
    const float4 gp = D.next[npix + px];
    const float4 cp = D.next[2 * npix + px];
    const float2 mp = D.next_mom[px];
    const int32_t prim_p = __float_as_int(gp.w);
    const bool valid = prim_p != RT_GUIDE_PRIM_NONE;
    const float N = pp.w;
    float var = max0(mp.y - mp.x * mp.x);
    const bool spatial = valid & !(N >= RT_PREVIEW_MIN_HISTORY);
    if (__builtin_amdgcn_ballot_w64(spatial) != 0) {
        const float rz = 1.0f / (D.sigma_z * D.depth[px]);
        const bool same_prim = (D.flags & RT_DENOISE_SAME_PRIM) != 0;
        float s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
#pragma unroll 1
        for (int dy = -3; dy <= 3; dy++) {
            const int qj = j + dy;
            const bool row = (qj >= 0) & (qj < D.ny);
            bool inside[7];
            float4 pq[7], gq[7];
            float2 mq[7];
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const int qi = i + k - 3;
                inside[k] = row & (qi >= 0) & (qi < D.nx);
                const size_t q = inside[k] ? (size_t)qj * D.nx + qi : px;
                pq[k] = D.next[q];
                gq[k] = D.next[npix + q];
                mq[k] = D.next_mom[q];
            }
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const int32_t prim_q = __float_as_int(gq[k].w);
                const bool ok = inside[k] & (prim_q != RT_GUIDE_PRIM_NONE);
                float wn = max0(gp.x * gq[k].x + gp.y * gq[k].y + gp.z * gq[k].z);
#pragma unroll
                for (int q = 0; q < SQ; q++) wn = wn * wn;
                const float ex = pq[k].x - pp.x, ey = pq[k].y - pp.y, ez = pq[k].z - pp.z;
                const float pd = fabsf(gp.x * ex + gp.y * ey + gp.z * ez);
                float wz = max0(1.0f - pd * rz);
                wz = wz * wz;
                float w = wn * wz;
                w = (same_prim & (prim_p != prim_q)) ? 0.0f : w;
                w = (k == 3 && dy == 0) ? 1.0f : w;             // the centre tap
                s1 = ok ? s1 + w * mq[k].x : s1;
                s2 = ok ? s2 + w * mq[k].y : s2;
                ws = ok ? ws + w : ws;
            }
        }
        const float a1 = s1 / ws, a2 = s2 / ws;
        const float sv = max0(a2 - a1 * a1) * (4.0f / N);
        var = spatial ? sv : var;
    }
    var = valid ? var : 0.0f;
    D.col[0][px] = make_float4(cp.x, cp.y, cp.z, var);
    if (D.variance) D.variance[px] = var;
}

// Stage A.  The denoiser's tap with the luminance weight in place of the colour weight, its width from the centre pixel's variance, and the variance filtered
// with the squared weights.  SQ = normal_squarings as a template argument: the tap is straight-line code, nothing in the tap loop branches.
template <bool LAST, int SQ>
__global__ void __launch_bounds__(kPreviewThreads) k_preview_atrous(const RtPreviewParams D, const float4* __restrict__ src, float4* __restrict__ dst, const int s) {
    int i, j;
    if (!tile_pixel(D.nx, D.ny, i, j)) return;
    const size_t npix = (size_t)D.nx * (size_t)D.ny, px = (size_t)j * D.nx + i;
    const float4 gp = D.next[npix + px];
    const int32_t prim_p = __float_as_int(gp.w);
    if (prim_p == RT_GUIDE_PRIM_NONE) return;                   // (its colour entry is dropped by every tap's select: invalid pixels are no taps)
    const float4 pp = D.next[px];
    const float4 cp = src[px];
    const float rz = 1.0f / (D.sigma_z * D.depth[px]);
    const float rl = 1.0f / (D.sigma_l * __builtin_sqrtf(cp.w) + RT_PREVIEW_LUM_EPS);
    const float lp = lum(cp.x, cp.y, cp.z);
    const bool same_prim = (D.flags & RT_DENOISE_SAME_PRIM) != 0;
    constexpr float K[3] = { 0.375f, 0.25f, 0.0625f };
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, vs = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = K[dx < 0 ? -dx : dx] * K[dy < 0 ? -dy : dy];
            if (dx == 0 && dy == 0) {
                sx = sx + h * cp.x; sy = sy + h * cp.y; sz = sz + h * cp.z;
                vs = vs + (h * h) * cp.w;
                wsum = wsum + h;
                continue;
            }
            const int qi = i + dx * s, qj = j + dy * s;
            const bool inside = (qi >= 0) & (qi < D.nx) & (qj >= 0) & (qj < D.ny);
            const size_t q = inside ? (size_t)qj * D.nx + qi : px;
            const float4 gq = D.next[npix + q];
            const float4 pq = D.next[q];
            const float4 cq = src[q];
            const int32_t prim_q = __float_as_int(gq.w);
            const bool ok = inside & (prim_q != RT_GUIDE_PRIM_NONE);
            float wn = max0(gp.x * gq.x + gp.y * gq.y + gp.z * gq.z);
#pragma unroll
            for (int k = 0; k < SQ; k++) wn = wn * wn;
            const float ex = pq.x - pp.x, ey = pq.y - pp.y, ez = pq.z - pp.z;
            const float pd = fabsf(gp.x * ex + gp.y * ey + gp.z * ez);
            float wz = max0(1.0f - pd * rz);
            wz = wz * wz;
            float w = h * wn * wz;
            float wl = max0(1.0f - fabsf(lp - lum(cq.x, cq.y, cq.z)) * rl);
            wl = wl * wl;
            w = w * wl;
            w = (same_prim & (prim_p != prim_q)) ? 0.0f : w;
            sx = ok ? sx + w * cq.x : sx;
            sy = ok ? sy + w * cq.y : sy;
            sz = ok ? sz + w * cq.z : sz;
            if (!LAST) vs = ok ? vs + (w * w) * cq.w : vs;
            wsum = ok ? wsum + w : wsum;
        }
    }
    float r[3] = { sx / wsum, sy / wsum, sz / wsum };          // wsum >= 9/64: the centre tap
    if (!LAST) {
        dst[px] = make_float4(r[0], r[1], r[2], vs / (wsum * wsum));
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

dim3 tile_grid(const RtPreviewParams& p) { return dim3((unsigned)((p.nx + kTileW - 1) / kTileW), (unsigned)((p.ny + kTileH - 1) / kTileH)); }

}  // namespace

hipError_t rt_launch_preview_temporal(RtPreviewParams p, const rt_camera& prev_cam, hipStream_t stream) {
    if (p.has_history) {
        float L[3];
        for (int a = 0; a < 3; a++) L[a] = prev_cam.lower_left_corner.e[a] - prev_cam.origin.e[a];
        p.prev_origin = prev_cam.origin; p.prev_u = prev_cam.u; p.prev_v = prev_cam.v; p.prev_w = prev_cam.w;
        p.Lu = dot3(L, prev_cam.u.e); p.Lv = dot3(L, prev_cam.v.e); p.Lw = dot3(L, prev_cam.w.e);
        p.Hl = dot3(prev_cam.horizontal.e, prev_cam.u.e);
        p.Vl = dot3(prev_cam.vertical.e, prev_cam.v.e);
    }
    const dim3 grid = tile_grid(p), block(kPreviewThreads);
    if (p.has_history && p.motion) hipLaunchKernelGGL((k_preview_temporal<true, true>), grid, block, 0, stream, p);
    else if (p.has_history) hipLaunchKernelGGL((k_preview_temporal<true, false>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((k_preview_temporal<false, false>), grid, block, 0, stream, p);
    return hipGetLastError();
}

#define RT_PREVIEW_SWITCH(LAUNCH) \
    switch (p.normal_squarings) { \
        LAUNCH(0) LAUNCH(1) LAUNCH(2) LAUNCH(3) LAUNCH(4) LAUNCH(5) LAUNCH(6) LAUNCH(7) \
        default: return hipErrorInvalidValue; \
    }

hipError_t rt_launch_preview_variance(const RtPreviewParams& p, hipStream_t stream) {
    const dim3 grid = tile_grid(p), block(kPreviewThreads);
#define RT_PREVIEW_VARIANCE(SQ) case SQ: hipLaunchKernelGGL((k_preview_variance<SQ>), grid, block, 0, stream, p); break;
    RT_PREVIEW_SWITCH(RT_PREVIEW_VARIANCE)
#undef RT_PREVIEW_VARIANCE
    return hipGetLastError();
}

hipError_t rt_launch_preview_iteration(const RtPreviewParams& p, int it, int last, hipStream_t stream) {
    const float4* src = p.col[it & 1];
    float4* dst = p.col[~it & 1];
    const dim3 grid = tile_grid(p), block(kPreviewThreads);
    const int sn = 1 << it;
#define RT_PREVIEW_ATROUS(SQ) \
    case SQ: \
        if (last) hipLaunchKernelGGL((k_preview_atrous<true, SQ>), grid, block, 0, stream, p, src, dst, sn); \
        else hipLaunchKernelGGL((k_preview_atrous<false, SQ>), grid, block, 0, stream, p, src, dst, sn); \
        break;
    RT_PREVIEW_SWITCH(RT_PREVIEW_ATROUS)
#undef RT_PREVIEW_ATROUS
    return hipGetLastError();
}
