// rt_kernels_refine.hip — the kernels of refineFrame (include/rt_api.h) around the pixel kernels: which pixels get another batch, in which order, and what their
// statistics become.  The path tracing itself is k_pixels_spheres / k_pixels_mesh, untouched, over the batch arrays these kernels fill.  DESIGN.md 3.23 has
// the reasons and the measurements.
//
// The arithmetic is the contract (tests/refine_reference.py restates it in numpy float32): fp32 only, + - * / only, every operation rounded on its own,
// operands in the order written, a comparison with a NaN false, max(x, 0) = x < 0 ? 0 : x - a NaN stays a NaN, so a pixel whose mean is not finite never
// passes `err <= threshold^2`.  So this translation unit is compiled once, like the other passes': -ffp-contract=off, no vectorisers, the default correctly
// rounded division, fp32 denormals kept.  Everything that decides the list is integers: no result depends on the order in which waves run.
//
//   k_refine_mark     one pixel per lane: err from (n, M1, M2, lum), unconverged(p) as a byte.
//   k_refine_count    one pixel per lane: the 3 x 3 window of those bytes, the sample cap, the class of the last batch's rays; the byte active ? cls + 1 : 0;
//                     a workgroup counts its classes in the LDS and adds its non-zero bins to the global histogram with one atomic each.
//   k_refine_scatter  every workgroup scans the 32 bins (descending class) for the class offsets; a wave takes 64 consecutive pixels and, for each class
//                     among them, ONE atomicAdd of that class's lane count on the class cursor - the lanes take their positions by ballot + mbcnt.
//   k_refine_scatter_ascending  RT_REFINE_ORDER=0 (measurements): one workgroup walks the image in order, so the list is ascending.
//   k_refine_gather / k_refine_update / k_refine_deliver  one list entry, respectively one pixel, per lane.
// Every barrier is reached by all lanes of its workgroup, every ballot by all lanes of its wave: lanes beyond the image take part with "nothing".
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "rt_refine.h"

namespace {

constexpr int kRefineThreads = 256;
constexpr int kRefineMaxBlocks = 1024;          // the counting and scattering kernels stride over the image beyond that
constexpr int kAscendingThreads = 1024;

__device__ __forceinline__ float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
__device__ __forceinline__ float max0(float x) { return x < 0.0f ? 0.0f : x; }
__device__ __forceinline__ uint32_t lane_rank(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// err(p) of rt_api.h from the pixel's statistics; K = n / batch
__device__ __forceinline__ float refine_err(int K, float M1, float M2, float l) {
    if (K < 2) return FLT_MAX;
    const float a1 = M1 / (float)K, a2 = M2 / (float)K;
    const float v = max0(a2 - a1 * a1) / (float)(K - 1);
    const float r = max0(l) + RT_REFINE_LUM_EPS;
    return v / (r * r);
}

__global__ void __launch_bounds__(kRefineThreads) k_refine_mark(const RtRefineParams R) {
    const size_t npix = (size_t)R.nx * (size_t)R.ny, p = (size_t)blockIdx.x * kRefineThreads + threadIdx.x;
    if (p >= npix) return;
    const int K = R.n[p] / R.batch;
    const float2 m = R.mom[p];
    const float err = refine_err(K, m.x, m.y, R.lum[p]);
    const bool unconverged = K < R.min_batches || !(err <= R.threshold * R.threshold);
    R.flag[p] = unconverged ? 1 : 0;
}

__global__ void __launch_bounds__(kRefineThreads) k_refine_count(const RtRefineParams R) {
    __shared__ uint32_t s_hist[kRefineClasses];
    const int t = (int)threadIdx.x;
    if (t < kRefineClasses) s_hist[t] = 0u;
    __syncthreads();
    const size_t npix = (size_t)R.nx * (size_t)R.ny, stride = (size_t)gridDim.x * kRefineThreads;
    for (size_t p = (size_t)blockIdx.x * kRefineThreads + t; p < npix; p += stride) {
        const int j = (int)(p / (size_t)R.nx), i = (int)(p - (size_t)j * (size_t)R.nx);
        bool want = R.flag[p] != 0;
        if (R.flags & RT_REFINE_DILATE) {
            const int j0 = j > 0 ? j - 1 : 0, j1 = j < R.ny - 1 ? j + 1 : R.ny - 1;
            const int i0 = i > 0 ? i - 1 : 0, i1 = i < R.nx - 1 ? i + 1 : R.nx - 1;
            for (int y = j0; y <= j1; y++)
                for (int x = i0; x <= i1; x++) want = want || R.flag[(size_t)y * (size_t)R.nx + (size_t)x] != 0;
        }
        const bool active = want && R.n[p] <= R.max_samples - R.batch;
        uint32_t c = 0u;
        if (active && R.cost_order) {
            const uint32_t r = R.rays[p];
            c = 31u - (uint32_t)__clz((int)(r > 1u ? r : 1u));
        }
        R.cls[p] = active ? (uint8_t)(c + 1u) : (uint8_t)0;
        if (active) atomicAdd(&s_hist[c], 1u);
    }
    __syncthreads();
    if (t < kRefineClasses) {
        const uint32_t n = s_hist[t];
        if (n != 0u) atomicAdd(&R.words[kRefineHist + t], n);
    }
}

__global__ void __launch_bounds__(kRefineThreads) k_refine_scatter(const RtRefineParams R) {
    __shared__ uint32_t s_off[kRefineClasses];
    const int t = (int)threadIdx.x;
    if (t < kRefineClasses) {                                   // the list starts with the dearest class: the offset of class t is the count of every class above it
        uint32_t off = 0u;
        for (int c = kRefineClasses - 1; c > t; c--) off += R.words[kRefineHist + c];
        s_off[t] = off;
        if (t == 0 && blockIdx.x == 0) R.words[kRefineTotal] = off + R.words[kRefineHist];
    }
    __syncthreads();
    const size_t npix = (size_t)R.nx * (size_t)R.ny, stride = (size_t)gridDim.x * kRefineThreads;
    const size_t rounds = (npix + stride - 1) / stride;         // (the same for every lane: the ballots below are reached by whole waves)
    for (size_t k = 0; k < rounds; k++) {
        const size_t p = k * stride + (size_t)blockIdx.x * kRefineThreads + t;
        const uint32_t c1 = p < npix ? R.cls[p] : 0u;
        unsigned long long rest = __ballot(c1 != 0u);
        while (rest != 0ull) {
            const uint32_t c = (uint32_t)__shfl((int)c1, __ffsll((long long)rest) - 1);      // the class of the first lane still waiting: wave-uniform
            const unsigned long long mine = __ballot(c1 == c);
            uint32_t base = 0u;
            if ((t & 63) == 0) base = atomicAdd(&R.words[kRefineCursor + c - 1u], (uint32_t)__popcll(mine));
            base = (uint32_t)__shfl((int)base, 0);
            if (c1 == c) R.list[s_off[c - 1u] + base + lane_rank(mine)] = (uint32_t)p;
            rest &= ~mine;
        }
    }
}

__global__ void __launch_bounds__(kAscendingThreads) k_refine_scatter_ascending(const RtRefineParams R) {
    __shared__ uint32_t s_cnt[kAscendingThreads / 64];
    __shared__ uint32_t s_base;
    const int t = (int)threadIdx.x, wave = t >> 6;
    if (t == 0) s_base = 0u;
    __syncthreads();
    const size_t npix = (size_t)R.nx * (size_t)R.ny;
    for (size_t first = 0; first < npix; first += kAscendingThreads) {
        const size_t p = first + t;
        const bool active = p < npix && R.cls[p] != 0;
        const unsigned long long m = __ballot(active);
        if ((t & 63) == 0) s_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = s_base;
        for (int w = 0; w < wave; w++) before += s_cnt[w];
        if (active) R.list[before + lane_rank(m)] = (uint32_t)p;
        __syncthreads();
        if (t == 0) {
            uint32_t total = 0u;
            for (int w = 0; w < kAscendingThreads / 64; w++) total += s_cnt[w];
            s_base += total;
        }
        __syncthreads();
    }
    if (t == 0) R.words[kRefineTotal] = s_base;
}

__global__ void __launch_bounds__(kRefineThreads) k_refine_gather(const RtRefineParams R) {
    const uint32_t e = blockIdx.x * kRefineThreads + threadIdx.x;
    if (e >= R.chunk_n) return;
    const uint32_t p = R.list[R.chunk_first + e];
    const uint32_t j = p / (uint32_t)R.nx;
    R.b_ij[2 * (size_t)e] = (int32_t)(p - j * (uint32_t)R.nx);
    R.b_ij[2 * (size_t)e + 1] = (int32_t)j;
    R.b_first[e] = R.n[p];
    reinterpret_cast<uint4*>(R.b_state)[e] = R.state[p];       // (an entry with first = 0 starts from the pixel's seed: the kernel does not read this)
}

__global__ void __launch_bounds__(kRefineThreads) k_refine_update(const RtRefineParams R) {
    const uint32_t e = blockIdx.x * kRefineThreads + threadIdx.x;
    if (e >= R.chunk_n) return;
    const uint32_t p = R.list[R.chunk_first + e];
    const uint4 st = reinterpret_cast<const uint4*>(R.b_state)[e];
    const int n0 = R.n[p], n1 = n0 + R.batch;
    const float fn1 = (float)n1;
    const float l1 = lum(__uint_as_float(st.x) / fn1, __uint_as_float(st.y) / fn1, __uint_as_float(st.z) / fn1);
    float y = l1;
    if (n0 != 0) y = (l1 * fn1 - R.lum[p] * (float)n0) / (float)R.batch;
    float2 m = R.mom[p];
    m.x = m.x + y;
    m.y = m.y + y * y;
    R.state[p] = st;
    R.rays[p] = R.b_rays[e];
    R.n[p] = n1;
    R.mom[p] = m;
    R.lum[p] = l1;
}

__global__ void __launch_bounds__(kRefineThreads) k_refine_deliver(const RtRefineParams R) {
    const size_t npix = (size_t)R.nx * (size_t)R.ny, p = (size_t)blockIdx.x * kRefineThreads + threadIdx.x;
    if (p >= npix) return;
    const int n = R.n[p];
    if (R.out) {
        const uint4 st = R.state[p];
        const float fn = (float)n;
        rt_vec3 o;
        o.e[0] = __uint_as_float(st.x) / fn; o.e[1] = __uint_as_float(st.y) / fn; o.e[2] = __uint_as_float(st.z) / fn;
        R.out[p] = o;
    }
    if (R.err) {
        const float2 m = R.mom[p];
        R.err[p] = refine_err(n / R.batch, m.x, m.y, R.lum[p]);
    }
}

unsigned blocks_of(size_t items) { return (unsigned)((items + kRefineThreads - 1) / kRefineThreads); }
unsigned capped_blocks_of(size_t items) {
    const size_t b = (items + kRefineThreads - 1) / kRefineThreads;
    return (unsigned)(b < (size_t)kRefineMaxBlocks ? b : (size_t)kRefineMaxBlocks);
}

}  // namespace

hipError_t rt_launch_refine_select(const RtRefineParams& p, hipStream_t stream) {
    const size_t npix = (size_t)p.nx * (size_t)p.ny;
    if (npix == 0 || npix > (1ull << 30) || p.batch < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_refine_mark, dim3(blocks_of(npix)), dim3(kRefineThreads), 0, stream, p);
    hipLaunchKernelGGL(k_refine_count, dim3(capped_blocks_of(npix)), dim3(kRefineThreads), 0, stream, p);
    if (p.cost_order) hipLaunchKernelGGL(k_refine_scatter, dim3(capped_blocks_of(npix)), dim3(kRefineThreads), 0, stream, p);
    else hipLaunchKernelGGL(k_refine_scatter_ascending, dim3(1), dim3(kAscendingThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_refine_gather(const RtRefineParams& p, hipStream_t stream) {
    if (p.chunk_n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_refine_gather, dim3(blocks_of(p.chunk_n)), dim3(kRefineThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_refine_update(const RtRefineParams& p, hipStream_t stream) {
    if (p.chunk_n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_refine_update, dim3(blocks_of(p.chunk_n)), dim3(kRefineThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_refine_deliver(const RtRefineParams& p, hipStream_t stream) {
    const size_t npix = (size_t)p.nx * (size_t)p.ny;
    if (npix == 0 || npix > (1ull << 30)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_refine_deliver, dim3(blocks_of(npix)), dim3(kRefineThreads), 0, stream, p);
    return hipGetLastError();
}
