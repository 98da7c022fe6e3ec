// rt_kernels_gather.hip — the kernels of gatherRadiance / rtGatherDirections (include/rt_api.h) around the radiance and any-hit kernels: the directions of a
// chunk of points in front of them, the per-point reduction behind them.  The tracing itself is k_radiance_* / k_rays_*, untouched, over the batch arrays
// these kernels fill and read.  DESIGN.md 3.29 has the reasons and the measurements.
//
// The arithmetic is the contract (rt_gather_dirs.h, which the CPU twin compiles too; tests/gather_reference.py restates it in numpy float32): fp32 only, every
// operation rounded on its own, operands in the order written, correctly rounded division and square root.  So this translation unit is compiled once, like
// the other passes': -ffp-contract=off, no vectorisers, the default correctly rounded division, fp32 denormals kept.
//
//   k_gather_dirs     one lane per (point, direction) of the chunk: lane t is entry t of the per-ray arrays, so a wave stores consecutive entries (and
//                     reads at most a few points).  The rejection loop is its only loop; it diverges (a wave runs the longest of its lanes' loops; a
//                     lane's loop takes 1.9 rounds on average).
//   k_gather_reduce   one lane per point: the sequential loop over the point's directions in ascending m; a lane walks its own dirs consecutive
//                     entries.  Plain vector loads and stores, no atomics: a point belongs to one lane.
// Every index is below pts * dirs <= RT_RAY_CHUNK (the host's chunking), computed in 32 bits.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#define RT_GATHER_FN __device__ __forceinline__
#include "rt_gather_dirs.h"
#include "rt_gather.h"

namespace {

constexpr int kGatherThreads = 256;

__global__ void __launch_bounds__(kGatherThreads) k_gather_dirs(const RtGatherParams G) {
    const uint32_t t = blockIdx.x * (uint32_t)kGatherThreads + threadIdx.x;
    if (t >= G.pts * G.dirs) return;
    const uint32_t kp = t / G.dirs, j = t - kp * G.dirs, e = t;
    const uint32_t g = rt_gather_id(G.base_id, G.k0 + kp, G.dirs_total, G.first + j);
    const float P[3] = { G.pos[3 * kp], G.pos[3 * kp + 1], G.pos[3 * kp + 2] };
    float N[3] = { 0.0f, 0.0f, 0.0f };
    if (G.mode != RT_GATHER_SH9) { N[0] = G.nrm[3 * kp]; N[1] = G.nrm[3 * kp + 1]; N[2] = G.nrm[3 * kp + 2]; }
    float o[3], D[3];
    rt_gather_ray(G.mode, P, N, G.bias, g, o, D);
    if (G.org) { G.org[3 * e] = o[0]; G.org[3 * e + 1] = o[1]; G.org[3 * e + 2] = o[2]; }
    if (G.dir) { G.dir[3 * e] = D[0]; G.dir[3 * e + 1] = D[1]; G.dir[3 * e + 2] = D[2]; }
    if (G.ids) G.ids[e] = g;
    if (G.t_max) G.t_max[e] = G.t_max_value;
}

__global__ void __launch_bounds__(kGatherThreads) k_gather_reduce(const RtGatherParams G) {
    const uint32_t kp = blockIdx.x * (uint32_t)kGatherThreads + threadIdx.x;
    if (kp >= G.pts) return;
    const int W = G.mode == RT_GATHER_IRRADIANCE ? 3 : G.mode == RT_GATHER_SH9 ? 27 : 1;
    float A[27];
#pragma unroll
    for (int i = 0; i < 27; i++) A[i] = (G.first > 0u && i < W) ? G.acc[(size_t)kp * W + i] : 0.0f;
    uint32_t r = 0u;
    for (uint32_t j = 0; j < G.dirs; j++) {
        const uint32_t e = kp * G.dirs + j;
        if (G.mode == RT_GATHER_VISIBILITY) {
            A[0] += G.occluded[e] ? 0.0f : 1.0f;
            continue;
        }
        const rt_vec3 L = G.L[e];
        if (G.rays) r += G.rays[e];
        if (G.mode == RT_GATHER_IRRADIANCE) {
            A[0] += L.e[0]; A[1] += L.e[1]; A[2] += L.e[2];
        } else {
            const float D[3] = { G.dir[3 * e], G.dir[3 * e + 1], G.dir[3 * e + 2] };
            float y[9];
            rt_gather_sh9(D, y);
#pragma unroll
            for (int i = 0; i < 9; i++) {
                A[3 * i] += L.e[0] * y[i]; A[3 * i + 1] += L.e[1] * y[i]; A[3 * i + 2] += L.e[2] * y[i];
            }
        }
    }
    const float M = (float)(G.first + G.dirs);
#pragma unroll
    for (int i = 0; i < 27; i++) {
        if (i >= W) break;
        if (G.acc) G.acc[(size_t)kp * W + i] = A[i];
        if (G.out) G.out[(size_t)kp * W + i] = G.mode == RT_GATHER_SH9 ? (A[i] * 12.566371f) / M : A[i] / M;
    }
    if (G.nrays) G.nrays[kp] = r;
}

}  // namespace

hipError_t rt_launch_gather_dirs(const RtGatherParams& p, hipStream_t stream) {
    const uint32_t n = p.pts * p.dirs;
    hipLaunchKernelGGL(k_gather_dirs, dim3((n + kGatherThreads - 1) / kGatherThreads), dim3(kGatherThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_gather_reduce(const RtGatherParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(k_gather_reduce, dim3((p.pts + kGatherThreads - 1) / kGatherThreads), dim3(kGatherThreads), 0, stream, p);
    return hipGetLastError();
}
