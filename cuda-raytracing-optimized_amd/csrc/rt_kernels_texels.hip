// rt_kernels_texels.hip — the kernels of rasterTexels / bakeTexels (include/rt_api.h, "baking texels"): the UV-atlas raster over the live triangle slots, the
// dilation of the chart borders, the compaction of the owned texels, the generator of a chunk of the compact list's directions and the scatter of the
// per-point results back into texel planes.  The tracing is k_radiance_* / k_rays_*, the per-point fold k_gather_reduce: untouched.  DESIGN.md 3.30 has the
// reasons and the measurements.
//
// The arithmetic is the contract (rt_texel_raster.h and rt_gather_dirs.h, which the CPU twins compile too; tests/texels_reference.py restates the raster in
// numpy float32): fp32 only, every operation rounded on its own, operands in the order written, correctly rounded division and square root.  So this
// translation unit is compiled once, like the other passes': -ffp-contract=off, no vectorisers, the default correctly rounded division, fp32 denormals kept.
//
//   k_texel_clear      one lane per texel: owner = INT32_MAX.
//   k_texel_coverage   one wave per slot: the slot's UV box clipped to the atlas and padded by a texel per side is walked 64 texels at a time; a lane whose
//                      texel passes the box and inside tests does atomicMin(owner[t], slot).  The minimum does not depend on the order: deterministic.
//   k_texel_resolve    one lane per texel: prim, src_0, and - recomputed from the owner with the lines that claimed it - bary, pos, nrm; the workgroup's owned
//                      count (one word per workgroup).
//   k_texel_dilate     one lane per texel, one launch per iteration, plane i - 1 to plane i.
//   k_texel_scan       one workgroup: the exclusive scan of the workgroup counts, the total into *length.
//   k_texel_compact    one lane per texel: the position of an owned texel in the list is the scanned count of its workgroup plus its rank inside it (ballot,
//                      popcount, four wave totals through LDS) - the list is ascending -; list, rank and the packed pos / nrm beside the list.
//   k_texel_dirs       one lane per (list entry, direction) of a chunk: k_gather_dirs with the point's index read from the list.
//   k_texel_fetch      one lane per list entry: the entry's sums from the acc plane (first > 0).
//   k_texel_scatter    one lane per texel: out through src and rank, acc and rays at owned texels, 0 elsewhere.
// Plane indices are computed in size_t (W * H reaches 2^26, times 27 floats); chunk-local indices are below RT_RAY_CHUNK, in 32 bits.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <stdint.h>

#define RT_GATHER_FN __device__ __forceinline__
#define RT_TEXEL_FN __device__ __forceinline__
#include "rt_gather_dirs.h"
#include "rt_texel_raster.h"
#include "rt_texels.h"

namespace {

constexpr int kWavesPerBlock = kTexelBlock / 64;
constexpr int kScanThreads = 1024;

__global__ void __launch_bounds__(kTexelBlock) k_texel_clear(const RtTexelParams T) {
    const size_t t = (size_t)blockIdx.x * kTexelBlock + threadIdx.x;
    if (t < (size_t)T.W * T.H) T.owner[t] = INT32_MAX;
}

__global__ void __launch_bounds__(kTexelBlock) k_texel_coverage(const RtTexelParams T) {
    const uint32_t slot = blockIdx.x * (uint32_t)kWavesPerBlock + (threadIdx.x >> 6);
    if (slot >= T.num_slots) return;
    const int lane = threadIdx.x & 63;
    const rt_triangle* tri = T.slots + slot;
    if (!rt_texel_candidate(tri)) return;
    float tc[6], box[4];
#pragma unroll
    for (int i = 0; i < 6; i++) tc[i] = tri->texCoords[i];
    rt_texel_box(tc, box);
    int x0, x1, y0, y1;
    rt_texel_span(box[0], box[1], T.W, &x0, &x1);
    rt_texel_span(box[2], box[3], T.H, &y0, &y1);
    if (x0 > x1 || y0 > y1) return;
    const uint32_t bw = (uint32_t)(x1 - x0 + 1), n = bw * (uint32_t)(y1 - y0 + 1);     // at most 2^26
    for (uint32_t i = lane; i < n; i += 64u) {
        const int y = y0 + (int)(i / bw), x = x0 + (int)(i - (i / bw) * bw);
        float s[2], h[2];
        rt_texel_sample(x, y, T.W, T.H, s);
        if (rt_texel_cover(tc, box, s, h)) atomicMin(&T.owner[(size_t)y * T.W + x], (int32_t)slot);
    }
}

__global__ void __launch_bounds__(kTexelBlock) k_texel_resolve(const RtTexelParams T) {
    const size_t t = (size_t)blockIdx.x * kTexelBlock + threadIdx.x;
    const bool in = t < (size_t)T.W * T.H;
    const int32_t o = in ? T.owner[t] : INT32_MAX;
    const bool owned = o != INT32_MAX;
    if (in) {
        if (T.prim) T.prim[t] = owned ? o : (int32_t)RT_GUIDE_PRIM_NONE;
        T.src[0][t] = owned ? (int32_t)t : -1;
        if (T.bary || T.pos || T.nrm) {
            float h[2] = { 0.0f, 0.0f }, pos[3] = { 0.0f, 0.0f, 0.0f }, nrm[3] = { 0.0f, 0.0f, 0.0f };
            if (owned) {
                const rt_triangle* tri = T.slots + o;
                float tc[6], box[4], s[2];
#pragma unroll
                for (int i = 0; i < 6; i++) tc[i] = tri->texCoords[i];
                rt_texel_box(tc, box);
                rt_texel_sample((int)(t % (size_t)T.W), (int)(t / (size_t)T.W), T.W, T.H, s);
                rt_texel_cover(tc, box, s, h);
                rt_texel_resolve(tri, h, pos, nrm);
            }
            if (T.bary) { T.bary[2 * t] = h[0]; T.bary[2 * t + 1] = h[1]; }
            if (T.pos) { T.pos[3 * t] = pos[0]; T.pos[3 * t + 1] = pos[1]; T.pos[3 * t + 2] = pos[2]; }
            if (T.nrm) { T.nrm[3 * t] = nrm[0]; T.nrm[3 * t + 1] = nrm[1]; T.nrm[3 * t + 2] = nrm[2]; }
        }
    }
    const int count = __syncthreads_count(owned ? 1 : 0);
    if (threadIdx.x == 0) T.counts[blockIdx.x] = (uint32_t)count;
}

__global__ void __launch_bounds__(kTexelBlock) k_texel_dilate(const int32_t* prev, int32_t* next, int W, int H) {
    const size_t t = (size_t)blockIdx.x * kTexelBlock + threadIdx.x;
    if (t >= (size_t)W * H) return;
    next[t] = rt_texel_dilate(prev, (int)(t % (size_t)W), (int)(t / (size_t)W), W, H);
}

// counts[b] -> the sum of counts[0 .. b - 1]; *length = the sum of all.  Thread i owns entries [i * per, (i + 1) * per).
__global__ void __launch_bounds__(kScanThreads) k_texel_scan(const RtTexelParams T) {
    __shared__ uint32_t part[kScanThreads];
    const uint32_t per = (T.blocks + kScanThreads - 1) / kScanThreads;
    const uint32_t b0 = min(threadIdx.x * per, T.blocks), b1 = min(b0 + per, T.blocks);
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; b++) sum += T.counts[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t step = 1; step < kScanThreads; step <<= 1) {
        const uint32_t add = threadIdx.x >= step ? part[threadIdx.x - step] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;                    // exclusive
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t c = T.counts[b];
        T.counts[b] = run;
        run += c;
    }
    if (threadIdx.x == kScanThreads - 1) *T.length = part[kScanThreads - 1];
}

__global__ void __launch_bounds__(kTexelBlock) k_texel_compact(const RtTexelParams T) {
    __shared__ uint32_t wave_total[kWavesPerBlock];
    const size_t t = (size_t)blockIdx.x * kTexelBlock + threadIdx.x;
    const bool in = t < (size_t)T.W * T.H;
    const int32_t o = in ? T.owner[t] : INT32_MAX;
    const bool owned = o != INT32_MAX;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(owned);
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t at = T.counts[blockIdx.x];
    for (int w = 0; w < wave; w++) at += wave_total[w];
    at += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (!in) return;
    T.rank[t] = owned ? (int32_t)at : -1;
    if (!owned) return;
    T.list[at] = (uint32_t)t;
    if (T.list_pos) {
        const rt_triangle* tri = T.slots + o;
        float tc[6], box[4], s[2], h[2] = { 0.0f, 0.0f }, pos[3], nrm[3];
#pragma unroll
        for (int i = 0; i < 6; i++) tc[i] = tri->texCoords[i];
        rt_texel_box(tc, box);
        rt_texel_sample((int)(t % (size_t)T.W), (int)(t / (size_t)T.W), T.W, T.H, s);
        rt_texel_cover(tc, box, s, h);
        rt_texel_resolve(tri, h, pos, nrm);
        T.list_pos[3 * (size_t)at] = pos[0]; T.list_pos[3 * (size_t)at + 1] = pos[1]; T.list_pos[3 * (size_t)at + 2] = pos[2];
        T.list_nrm[3 * (size_t)at] = nrm[0]; T.list_nrm[3 * (size_t)at + 1] = nrm[1]; T.list_nrm[3 * (size_t)at + 2] = nrm[2];
    }
}

__global__ void __launch_bounds__(kTexelBlock) k_texel_dirs(const RtGatherParams G, const uint32_t* list) {
    const uint32_t e = blockIdx.x * (uint32_t)kTexelBlock + threadIdx.x;
    if (e >= G.pts * G.dirs) return;
    const uint32_t kp = e / G.dirs, j = e - kp * G.dirs;
    const uint32_t g = rt_gather_id(G.base_id, list[G.k0 + kp], G.dirs_total, G.first + j);
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

__global__ void __launch_bounds__(kTexelBlock) k_texel_fetch(const RtTexelBakeParams B) {
    const uint32_t r = blockIdx.x * (uint32_t)kTexelBlock + threadIdx.x;
    if (r >= B.length) return;
    const size_t t = B.list[r];
    for (int i = 0; i < B.Wd; i++) B.acc[(size_t)r * B.Wd + i] = B.acc_plane[t * B.Wd + i];
}

__global__ void __launch_bounds__(kTexelBlock) k_texel_scatter(const RtTexelBakeParams B) {
    const size_t t = (size_t)blockIdx.x * kTexelBlock + threadIdx.x;
    if (t >= (size_t)B.texels) return;
    const int32_t r = B.rank[t];
    if (B.out_plane) {
        const int32_t s = B.src[t];
        const int32_t rs = s == -1 ? -1 : B.rank[s];
        for (int i = 0; i < B.Wd; i++) B.out_plane[t * B.Wd + i] = rs < 0 ? 0.0f : B.out[(size_t)rs * B.Wd + i];
    }
    if (B.acc_plane)
        for (int i = 0; i < B.Wd; i++) B.acc_plane[t * B.Wd + i] = r < 0 ? 0.0f : B.acc[(size_t)r * B.Wd + i];
    if (B.rays_plane) B.rays_plane[t] = r < 0 ? 0u : B.nrays[r];
}

inline uint32_t texel_blocks(const RtTexelParams& p) { return (uint32_t)(((size_t)p.W * p.H + kTexelBlock - 1) / kTexelBlock); }

}  // namespace

hipError_t rt_launch_texel_coverage(const RtTexelParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(k_texel_clear, dim3(texel_blocks(p)), dim3(kTexelBlock), 0, stream, p);
    if (p.num_slots > 0)
        hipLaunchKernelGGL(k_texel_coverage, dim3((p.num_slots + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kTexelBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_texel_resolve(const RtTexelParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(k_texel_resolve, dim3(texel_blocks(p)), dim3(kTexelBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_texel_dilate(const RtTexelParams& p, int i, hipStream_t stream) {
    hipLaunchKernelGGL(k_texel_dilate, dim3(texel_blocks(p)), dim3(kTexelBlock), 0, stream, (const int32_t*)p.src[(i - 1) & 1], p.src[i & 1], p.W, p.H);
    return hipGetLastError();
}

hipError_t rt_launch_texel_scan(const RtTexelParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(k_texel_scan, dim3(1), dim3(kScanThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_texel_compact(const RtTexelParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(k_texel_compact, dim3(texel_blocks(p)), dim3(kTexelBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_texel_dirs(const RtGatherParams& g, const uint32_t* list, hipStream_t stream) {
    const uint32_t n = g.pts * g.dirs;
    hipLaunchKernelGGL(k_texel_dirs, dim3((n + kTexelBlock - 1) / kTexelBlock), dim3(kTexelBlock), 0, stream, g, list);
    return hipGetLastError();
}

hipError_t rt_launch_texel_fetch(const RtTexelBakeParams& b, hipStream_t stream) {
    if (b.length == 0) return hipSuccess;
    hipLaunchKernelGGL(k_texel_fetch, dim3((b.length + kTexelBlock - 1) / kTexelBlock), dim3(kTexelBlock), 0, stream, b);
    return hipGetLastError();
}

hipError_t rt_launch_texel_scatter(const RtTexelBakeParams& b, hipStream_t stream) {
    hipLaunchKernelGGL(k_texel_scatter, dim3((b.texels + kTexelBlock - 1) / kTexelBlock), dim3(kTexelBlock), 0, stream, b);
    return hipGetLastError();
}
