// rt_kernels_accumulate.hip — the temporal accumulation of accumulateFrame (include/rt_api.h): every pixel with a first hit is reprojected into the previous
// call's frame through its world-space hit point, the four pixels around that position are checked against the previous frame's geometry and blended into
// the new sample with a per-pixel history length (the temporal half of SVGF).  DESIGN.md 3.12 has the definition, the record layout and the measurements.
//
// The arithmetic is the contract (tests/accumulate_reference.py restates it in numpy float32): fp32 only, + - * / abs floor min only, every product and sum
// rounded on its own, operands in the order written, a comparison with a NaN false.  So this translation unit is compiled once, like the denoiser's:
// -ffp-contract=off, no vectorisers, the default correctly rounded division and square root, fp32 denormals kept.  The constants of the previous camera are
// computed by the launcher below, on the host, under the same flags.
//
// One lane per pixel, a wave a 32 x 2 patch and a workgroup a 32 x 8 tile, as the denoiser's: a wave's four taps are four shifted 32 x 2 patches of each record
// plane.  No atomics, no LDS, no communication between workgroups.  The four taps are straight-line code: their twelve records are loaded first, then tested with
// selects; a tap's address is formed from an index that is inside the image, or it is the pixel's own.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "rt_accumulate.h"

namespace {

constexpr int kTileW = 32, kTileH = 8, kAccumulateThreads = kTileW * kTileH;

__host__ __device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// vec3.h:194 as the guide kernels evaluate it (a / sqrt(squared_length), three divisions)
__device__ __forceinline__ void unit3(float& x, float& y, float& z) {
    const float l = __builtin_sqrtf(x * x + y * y + z * z);
    x = x / l; y = y / l; z = z / l;
}

// MOTION: a pose is marked (rtMarkPose) - the reprojection and the taps' plane and normal tests take Pm(p), nm(p) of the motion planes (rt_motion.h) in the
// place of P(p), n(p); everything else, the stored records included, is the pixel's own.  MOTION = false is the kernel as it was.
template <bool HIST, bool MOTION>
__global__ void __launch_bounds__(kAccumulateThreads) k_accumulate(const RtAccumulateParams D) {
    const int i = (int)blockIdx.x * kTileW + (int)(threadIdx.x & (kTileW - 1));
    const int j = (int)blockIdx.y * kTileH + (int)(threadIdx.x / kTileW);
    if (i >= D.nx || j >= D.ny) return;
    const size_t npix = (size_t)D.nx * (size_t)D.ny, px = (size_t)j * D.nx + i;
    const rt_vec3 in = D.in[px];
    const int32_t prim = D.prim[px];
    const float t = D.depth[px];
    const float n[3] = { D.normal[px * 3], D.normal[px * 3 + 1], D.normal[px * 3 + 2] };
    // the centre ray of the guide kernels: camera.h:8-12 without the lens offset, and the ray's own normalisation on top (ray.h:9) - as the denoiser's prologue
    const float u = ((float)i + 0.5f) / (float)D.nx, v = ((float)j + 0.5f) / (float)D.ny;
    const float* org = D.cam.origin.e;
    float d[3];
    for (int a = 0; a < 3; a++) d[a] = D.cam.lower_left_corner.e[a] + u * D.cam.horizontal.e[a] + v * D.cam.vertical.e[a] - org[a];
    unit3(d[0], d[1], d[2]);
    unit3(d[0], d[1], d[2]);
    const float P[3] = { org[0] + t * d[0], org[1] + t * d[1], org[2] + t * d[2] };
    const bool valid = prim != RT_GUIDE_PRIM_NONE;
    const bool demodulate = (D.flags & RT_DENOISE_DEMODULATE) != 0;
    float m[3] = { 1.0f, 1.0f, 1.0f }, c[3] = { in.e[0], in.e[1], in.e[2] };
    if (demodulate)
        for (int a = 0; a < 3; a++) {
            const float al = D.albedo[px * 3 + a];
            m[a] = al > RT_DENOISE_ALBEDO_FLOOR ? al : RT_DENOISE_ALBEDO_FLOOR;
            c[a] = c[a] / m[a];
        }
    float N = valid ? 1.0f : 0.0f;
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
        // All twelve records of the four taps are requested before any of them is tested (a tap outside the image reads the pixel's own, a cached address),
        // and the tests are combined with `&`, not `&&`: a short circuit would put the geo load of a tap behind a branch on its pos record, and the next
        // tap's loads behind that (the A/B: DESIGN.md 3.12).
        bool inside[4];
        float4 pq[4], gq[4], cq[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int qi = i0 + (k & 1), qj = j0 + (k >> 1);
            inside[k] = (qi >= 0) & (qi < D.nx) & (qj >= 0) & (qj < D.ny);
            const size_t q = inside[k] ? (size_t)qj * D.nx + qi : px;
            pq[k] = D.prev[q];
            gq[k] = D.prev[npix + q];
            cq[k] = D.prev[2 * npix + q];
        }
        float sum[3] = { 0.0f, 0.0f, 0.0f }, nsum = 0.0f, wsum = 0.0f;
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
        }
        if (candidate && wsum > 0.0f) {
            const float len = nsum / wsum + 1.0f;
            N = len < D.max_history ? len : D.max_history;
            const float al = 1.0f / N;
            for (int a = 0; a < 3; a++) {
                const float h = sum[a] / wsum;
                c[a] = h + al * (c[a] - h);
            }
        }
    }
    D.next[px] = make_float4(P[0], P[1], P[2], N);
    D.next[npix + px] = make_float4(n[0], n[1], n[2], __int_as_float(prim));
    D.next[2 * npix + px] = make_float4(c[0], c[1], c[2], 0.0f);
    if (D.history) D.history[px] = N;
    rt_vec3 o = in;                                             // without a first hit: the input bit for bit
    if (valid)
        for (int a = 0; a < 3; a++) o.e[a] = demodulate ? c[a] * m[a] : c[a];
    D.out[px] = o;
}

}  // namespace

hipError_t rt_launch_accumulate(RtAccumulateParams p, const rt_camera& prev_cam, hipStream_t stream) {
    if (p.has_history) {
        float L[3];
        for (int a = 0; a < 3; a++) L[a] = prev_cam.lower_left_corner.e[a] - prev_cam.origin.e[a];
        p.prev_origin = prev_cam.origin; p.prev_u = prev_cam.u; p.prev_v = prev_cam.v; p.prev_w = prev_cam.w;
        p.Lu = dot3(L, prev_cam.u.e); p.Lv = dot3(L, prev_cam.v.e); p.Lw = dot3(L, prev_cam.w.e);
        p.Hl = dot3(prev_cam.horizontal.e, prev_cam.u.e);
        p.Vl = dot3(prev_cam.vertical.e, prev_cam.v.e);
    }
    const dim3 grid((unsigned)((p.nx + kTileW - 1) / kTileW), (unsigned)((p.ny + kTileH - 1) / kTileH)), block(kAccumulateThreads);
    if (p.has_history && p.motion) hipLaunchKernelGGL((k_accumulate<true, true>), grid, block, 0, stream, p);
    else if (p.has_history) hipLaunchKernelGGL((k_accumulate<true, false>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((k_accumulate<false, false>), grid, block, 0, stream, p);
    return hipGetLastError();
}
