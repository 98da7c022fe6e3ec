// rt_kernels_motion.hip — the motion planes of rtMarkPose / renderMotion (include/rt_api.h): for every pixel with a first hit, the point Pm its surface point
// had in the marked pose of the scene ("the previous frame's geometry"), the normal nm it had there, and optionally where the previous camera saw Pm.  The
// temporal passes (accumulateFrame, stage T of previewFrame) reproject through Pm and test their taps against (Pm, nm), so what an edit moved keeps its history.
// DESIGN.md 3.25 has the definition, the reasons and the measurements.
//
// No traversal: the guide planes of the pass already say which primitive a pixel sees and at which distance.  For a triangle the barycentrics of the hit
// point come by projecting P - v0 onto the live edges (the normal equations of the 2 x 3 system), and are applied to the marked vertices; for a sphere the
// point keeps its direction from the centre.  A primitive whose marked words equal the live ones bit for bit is not touched at all: Pm = P, nm = n.
//
// The arithmetic is the contract (tests/motion_reference.py restates it in numpy float32): fp32 only, every product and sum rounded on its own, operands in
// the order written, a comparison with a NaN false.  So this translation unit is compiled once, like the accumulation's: -ffp-contract=off, no vectorisers,
// the default correctly rounded division and square root, fp32 denormals kept.  The constants of the previous camera are computed by the launcher below, on
// the host, under the same flags, exactly as rt_launch_accumulate computes them.
//
// One lane per pixel, a wave a 32 x 2 patch and a workgroup a 32 x 8 tile, as the accumulation's.  No atomics, no LDS, no communication between workgroups.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "rt_motion.h"

namespace {

constexpr int kTileW = 32, kTileH = 8, kMotionThreads = kTileW * kTileH, kGatherThreads = 256;

__host__ __device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// vec3.h:194 as the guide kernels evaluate it (a / sqrt(squared_length), three divisions)
__device__ __forceinline__ void unit3(float& x, float& y, float& z) {
    const float l = __builtin_sqrtf(x * x + y * y + z * z);
    x = x / l; y = y / l; z = z / l;
}

// vec3.h cross(): the middle component is the negated difference
__device__ __forceinline__ void cross3(const float* a, const float* b, float* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = -(a[0] * b[2] - a[2] * b[0]);
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_int(a) == __float_as_int(b); }

__global__ void __launch_bounds__(kMotionThreads) k_motion(const RtMotionParams D) {
    const int i = (int)blockIdx.x * kTileW + (int)(threadIdx.x & (kTileW - 1));
    const int j = (int)blockIdx.y * kTileH + (int)(threadIdx.x / kTileW);
    if (i >= D.nx || j >= D.ny) return;
    const size_t npix = (size_t)D.nx * (size_t)D.ny, px = (size_t)j * D.nx + i;
    const int32_t prim = D.prim[px];
    const float t = D.depth[px];
    const float n[3] = { D.normal[px * 3], D.normal[px * 3 + 1], D.normal[px * 3 + 2] };
    // the centre ray of the guide kernels, as k_accumulate forms it
    const float u = ((float)i + 0.5f) / (float)D.nx, v = ((float)j + 0.5f) / (float)D.ny;
    const float* org = D.cam.origin.e;
    float d[3];
    for (int a = 0; a < 3; a++) d[a] = D.cam.lower_left_corner.e[a] + u * D.cam.horizontal.e[a] + v * D.cam.vertical.e[a] - org[a];
    unit3(d[0], d[1], d[2]);
    unit3(d[0], d[1], d[2]);
    const float P[3] = { org[0] + t * d[0], org[1] + t * d[1], org[2] + t * d[2] };
    const bool valid = prim != RT_GUIDE_PRIM_NONE;
    float Pm[3] = { P[0], P[1], P[2] }, nm[3] = { n[0], n[1], n[2] };
    if (!valid) {
        for (int a = 0; a < 3; a++) Pm[a] = nm[a] = 0.0f;
    } else if (prim >= 0 && (uint32_t)prim < D.count) {         // (the floor does not move)
        if (D.mark) {
            // a slot is 64 bytes at a 64-byte offset of the allocation: its nine coordinates are the first 36 bytes
            const float4* lv = reinterpret_cast<const float4*>(D.live + prim);
            const float4* mk = reinterpret_cast<const float4*>(D.mark + prim);
            const float4 l0 = lv[0], l1 = lv[1], l2 = lv[2], m0 = mk[0], m1 = mk[1], m2 = mk[2];
            const float v0[3] = { l0.x, l0.y, l0.z }, v1[3] = { l0.w, l1.x, l1.y }, v2[3] = { l1.z, l1.w, l2.x };
            const float a0[3] = { m0.x, m0.y, m0.z }, a1[3] = { m0.w, m1.x, m1.y }, a2[3] = { m1.z, m1.w, m2.x };
            bool moved = false;
            for (int a = 0; a < 3; a++) moved = moved || !same_bits(v0[a], a0[a]) || !same_bits(v1[a], a1[a]) || !same_bits(v2[a], a2[a]);
            const bool sentinel = fabsf(a0[0]) == INFINITY;
            if (moved && !sentinel) {
                float e1[3], e2[3], w[3], f1[3], f2[3];
                for (int a = 0; a < 3; a++) { e1[a] = v1[a] - v0[a]; e2[a] = v2[a] - v0[a]; w[a] = P[a] - v0[a]; }
                const float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), d1w = dot3(e1, w), d2w = dot3(e2, w);
                const float den = d11 * d22 - d12 * d12;
                const float bu = (d22 * d1w - d12 * d2w) / den, bv = (d11 * d2w - d12 * d1w) / den;
                for (int a = 0; a < 3; a++) { f1[a] = a1[a] - a0[a]; f2[a] = a2[a] - a0[a]; }
                for (int a = 0; a < 3; a++) Pm[a] = a0[a] + bu * f1[a] + bv * f2[a];
                float gm[3], gl[3];
                cross3(f1, f2, gm);
                unit3(gm[0], gm[1], gm[2]);
                cross3(e1, e2, gl);
                const bool turned = dot3(gl, n) < 0.0f;             // the turn hit() gave the live normal
                for (int a = 0; a < 3; a++) nm[a] = turned ? -gm[a] : gm[a];
            }
        } else if (D.mark_sph) {
            const float4 ls = D.live_sph[prim], ms = D.mark_sph[prim];
            const bool moved = !same_bits(ls.x, ms.x) || !same_bits(ls.y, ms.y) || !same_bits(ls.z, ms.z) || !same_bits(ls.w, ms.w);
            if (moved) {
                const float c[3] = { ls.x, ls.y, ls.z }, cm[3] = { ms.x, ms.y, ms.z };
                for (int a = 0; a < 3; a++) Pm[a] = cm[a] + ((P[a] - c[a]) / ls.w) * ms.w;
            }
        }
    }
    D.planes[px] = make_float4(Pm[0], Pm[1], Pm[2], 0.0f);
    D.planes[npix + px] = make_float4(nm[0], nm[1], nm[2], 0.0f);
    if (D.screen) {
        // k_accumulate's reprojection with Pm in the place of P
        const float e[3] = { Pm[0] - D.prev_origin.e[0], Pm[1] - D.prev_origin.e[1], Pm[2] - D.prev_origin.e[2] };
        const float ea = dot3(e, D.prev_u.e), eb = dot3(e, D.prev_v.e), ec = dot3(e, D.prev_w.e);
        const float r = D.Lw / ec;
        const float s = (ea * r - D.Lu) / D.Hl, tt = (eb * r - D.Lv) / D.Vl;
        const float x = s * (float)D.nx - 0.5f, y = tt * (float)D.ny - 0.5f;
        const bool seen = valid && r > 0.0f;
        D.screen[px] = seen ? make_float2(x - (float)i, y - (float)j) : make_float2(0.0f, 0.0f);
    }
}

__global__ void __launch_bounds__(kGatherThreads) k_motion_gather(const float4* __restrict__ in, float4* __restrict__ out, const int32_t* __restrict__ old_slot,
                                                                  const uint32_t count) {
    const uint32_t s = blockIdx.x * (uint32_t)kGatherThreads + threadIdx.x;
    if (s >= count) return;
    const int32_t from = old_slot[s];
    const bool real = from >= 0 && (uint32_t)from < count;
    const size_t src = real ? (size_t)from : (size_t)s;         // (an address inside the array either way)
    float4 r0 = in[src * 4], r1 = in[src * 4 + 1], r2 = in[src * 4 + 2], r3 = in[src * 4 + 3];
    if (!real) {
        r0 = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
        r1 = r0;
        r2 = make_float4(INFINITY, 0.0f, 0.0f, 0.0f);
        r3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    out[(size_t)s * 4] = r0; out[(size_t)s * 4 + 1] = r1; out[(size_t)s * 4 + 2] = r2; out[(size_t)s * 4 + 3] = r3;
}

}  // namespace

hipError_t rt_launch_motion(RtMotionParams p, const rt_camera& prev_cam, hipStream_t stream) {
    if (p.screen) {
        float L[3];
        for (int a = 0; a < 3; a++) L[a] = prev_cam.lower_left_corner.e[a] - prev_cam.origin.e[a];
        p.prev_origin = prev_cam.origin; p.prev_u = prev_cam.u; p.prev_v = prev_cam.v; p.prev_w = prev_cam.w;
        p.Lu = dot3(L, prev_cam.u.e); p.Lv = dot3(L, prev_cam.v.e); p.Lw = dot3(L, prev_cam.w.e);
        p.Hl = dot3(prev_cam.horizontal.e, prev_cam.u.e);
        p.Vl = dot3(prev_cam.vertical.e, prev_cam.v.e);
    }
    const dim3 grid((unsigned)((p.nx + kTileW - 1) / kTileW), (unsigned)((p.ny + kTileH - 1) / kTileH)), block(kMotionThreads);
    hipLaunchKernelGGL(k_motion, grid, block, 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_motion_gather(const rt_triangle* in, rt_triangle* out, const int32_t* old_slot, uint32_t count, hipStream_t stream) {
    static_assert(sizeof(rt_triangle) == 4 * sizeof(float4), "a slot is four 16-byte words");
    if (count == 0) return hipSuccess;
    const dim3 grid((count + kGatherThreads - 1) / kGatherThreads), block(kGatherThreads);
    hipLaunchKernelGGL(k_motion_gather, grid, block, 0, stream, reinterpret_cast<const float4*>(in), reinterpret_cast<float4*>(out), old_slot, count);
    return hipGetLastError();
}
