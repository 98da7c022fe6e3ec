// rt_kernels_display.hip — the kernels of displayFrame (include/rt_api.h): the luminance histogram of the input frame, the median bin and the adapted exposure
// from it, and the per-pixel transform exposure -> tone map -> sRGB -> dither -> four bytes.  DESIGN.md 3.14 has the definition's reasons and the measurements.
//
// The arithmetic is the contract (tests/display_reference.py restates it in numpy float32 with libm's powf; host/rt_display_host.cpp is the CPU twin): fp32
// only, every product and sum rounded on its own, operands in the order written, a comparison with a NaN false, max(a, b) = a > b ? a : b.  So this translation
// unit is compiled once, like the other passes': -ffp-contract=off, no vectorisers, the default correctly rounded division, fp32 denormals kept.  powf is
// glibc's algorithm restated (rt_glibc_powf_pos.h: fp64 inside with explicit fused operations, one rounding to fp32).
//
// Three kernels on one stream, nothing of the host between them:
//   (a) k_display_histogram  a workgroup counts its pixels into RT_DISPLAY_BINS words of the LDS with LDS atomics, then adds its non-zero bins to the global
//                            histogram with one global atomic each.  Integer counts: the order of the adds does not matter.
//   (b) k_display_resolve    one workgroup: inclusive prefix sum of the bins in the LDS, the median bin, target, E and E_used into device memory.
//   (c) k_display_transform  one pixel per lane: three floats in, one 32-bit word out, consecutive lanes consecutive words of an output row.  The 512 bytes of
//                            powf tables and the 64 dither offsets are copied into the LDS by the workgroup's first lanes, as the render kernels keep theirs.
// Every barrier is reached by all lanes of its workgroup: lanes beyond the image leave after the last one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_display.h"

#define RT_POWF_FN __device__ __forceinline__
#define RT_POWF_TABLE static __constant__ const
#include "rt_glibc_powf_pos.h"

namespace {

constexpr int kDisplayThreads = 256;
constexpr int kHistogramMaxBlocks = 1024;                       // (a) strides over the image beyond that: at most 1024 x 256 global atomics
constexpr int kBinBias = (127 - 16) << 3;                       // bits(2^-16) >> 20
static_assert(RT_DISPLAY_BINS == kDisplayThreads, "one lane per bin in (a) and (b)");

static __constant__ const uint8_t kBayer8[8][8] = RT_DISPLAY_BAYER8;

__device__ __forceinline__ float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
__device__ __forceinline__ float max0(float x) { return x > 0.0f ? x : 0.0f; }

__global__ void __launch_bounds__(kDisplayThreads) k_display_histogram(const RtDisplayParams D) {
    __shared__ uint32_t s_hist[RT_DISPLAY_BINS];
    const int t = (int)threadIdx.x;
    s_hist[t] = 0u;
    __syncthreads();
    const size_t npix = (size_t)D.nx * (size_t)D.ny, stride = (size_t)gridDim.x * kDisplayThreads;
    for (size_t q = (size_t)blockIdx.x * kDisplayThreads + t; q < npix; q += stride) {
        const rt_vec3 c = D.in[q];
        const float l = lum(c.e[0], c.e[1], c.e[2]);
        const uint32_t w = __float_as_uint(l);
        const int b = (int)(w >> 20) - kBinBias;
        if ((w & 0x7f800000u) != 0x7f800000u && l > 0.0f && b >= 0) atomicAdd(&s_hist[b < RT_DISPLAY_BINS - 1 ? b : RT_DISPLAY_BINS - 1], 1u);
    }
    __syncthreads();
    const uint32_t n = s_hist[t];
    if (n != 0u) atomicAdd(&D.hist[t], n);
}

__global__ void __launch_bounds__(kDisplayThreads) k_display_resolve(const RtDisplayParams D) {
    __shared__ uint32_t s_cum[2][RT_DISPLAY_BINS];
    const int t = (int)threadIdx.x;
    s_cum[0][t] = D.hist[t];
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < RT_DISPLAY_BINS; off <<= 1) {      // Hillis-Steele, ping-pong: one barrier per step
        uint32_t a = s_cum[cur][t];
        if (t >= off) a += s_cum[cur][t - off];
        s_cum[cur ^ 1][t] = a;
        __syncthreads();
        cur ^= 1;
    }
    const uint32_t total = s_cum[cur][RT_DISPLAY_BINS - 1];
    const uint64_t cum = s_cum[cur][t], below = t > 0 ? s_cum[cur][t - 1] : 0u;
    // exactly one lane: lane 0 of an empty histogram, else the smallest bin with 2 cum >= T (cum does not decrease and ends at T)
    const bool mine = total == 0u ? t == 0 : (2u * cum >= total && 2u * below < total);
    if (!mine) return;
    float target = 1.0f;
    if (total != 0u) {
        const float lmed = __uint_as_float(((uint32_t)(t + kBinBias) << 20) | (1u << 19));
        target = RT_DISPLAY_KEY / lmed;
    }
    float E = target;
    if (D.adapted) {
        const float prev = D.state[0];
        E = prev + D.adapt * (target - prev);
    }
    D.state[0] = E;
    D.state[1] = E * D.exposure;
}

// rtLinearToSRGB's lines on one channel, the conversion clamped first; `d` is the pixel's dither offset
template <bool DITHER>
__device__ __forceinline__ uint32_t encode(float y, float d, const double* log2_tab, const uint64_t* exp2_tab) {
    float s = max0(y);
    s = max0(1.055f * rt_glibc_powf_pos_tab(s, 0.416666667f, log2_tab, exp2_tab) - 0.055f);
    const float t = DITHER ? s * 255.0f + d : s * 255.9f;
    return t >= 255.0f ? 255u : (uint32_t)t;
}

template <int TONEMAP, bool DITHER>
__global__ void __launch_bounds__(kDisplayThreads) k_display_transform(const RtDisplayParams D) {
    __shared__ double s_log2[32];
    __shared__ uint64_t s_exp2[32];
    __shared__ float s_dither[64];
    const int t = (int)threadIdx.x;
    if (t < 32) s_log2[t] = rt_powf_log2_tab[t];
    else if (t < 64) s_exp2[t - 32] = rt_powf_exp2_tab[t - 32];
    else if (t < 128) s_dither[t - 64] = ((float)kBayer8[(t - 64) >> 3][(t - 64) & 7] + 0.5f) / 64.0f;
    __syncthreads();
    const size_t npix = (size_t)D.nx * (size_t)D.ny, q = (size_t)blockIdx.x * kDisplayThreads + t;
    if (q >= npix) return;
    const int j = (int)(q / (size_t)D.nx), i = (int)(q - (size_t)j * (size_t)D.nx);
    const float E = D.state ? D.state[1] : D.exposure;
    const rt_vec3 c = D.in[q];
    float y[3] = { c.e[0] * E, c.e[1] * E, c.e[2] * E };
    if (TONEMAP == RT_TONEMAP_REINHARD) {
        const float den = 1.0f + max0(lum(y[0], y[1], y[2]));
        for (int k = 0; k < 3; k++) y[k] = y[k] / den;
    } else if (TONEMAP == RT_TONEMAP_ACES) {
        for (int k = 0; k < 3; k++) {
            const float a = max0(y[k]);
            y[k] = (a * (2.51f * a + 0.03f)) / (a * (2.43f * a + 0.59f) + 0.14f);
        }
    }
    const float d = s_dither[(j & 7) * 8 + (i & 7)];
    uint32_t word = 255u << 24;
    for (int k = 0; k < 3; k++) word |= encode<DITHER>(y[k], d, s_log2, s_exp2) << (8 * k);
    const size_t row = (D.flags & RT_DISPLAY_TOP_DOWN) ? (size_t)(D.ny - 1 - j) : (size_t)j;
    D.out[row * (size_t)D.nx + (size_t)i] = word;
}

template <int TONEMAP>
hipError_t launch_transform(const RtDisplayParams& p, unsigned blocks, hipStream_t stream) {
    if (p.flags & RT_DISPLAY_DITHER) hipLaunchKernelGGL((k_display_transform<TONEMAP, true>), dim3(blocks), dim3(kDisplayThreads), 0, stream, p);
    else hipLaunchKernelGGL((k_display_transform<TONEMAP, false>), dim3(blocks), dim3(kDisplayThreads), 0, stream, p);
    return hipGetLastError();
}

size_t pixel_blocks(const RtDisplayParams& p) {
    const size_t npix = (size_t)p.nx * (size_t)p.ny;
    return (npix + kDisplayThreads - 1) / kDisplayThreads;
}

}  // namespace

hipError_t rt_launch_display_histogram(const RtDisplayParams& p, hipStream_t stream) {
    const size_t blocks = pixel_blocks(p);
    hipLaunchKernelGGL(k_display_histogram, dim3((unsigned)(blocks < (size_t)kHistogramMaxBlocks ? blocks : (size_t)kHistogramMaxBlocks)), dim3(kDisplayThreads), 0,
                       stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_display_resolve(const RtDisplayParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(k_display_resolve, dim3(1), dim3(kDisplayThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t rt_launch_display_transform(const RtDisplayParams& p, hipStream_t stream) {
    const size_t blocks = pixel_blocks(p);
    if (blocks == 0 || blocks > 0x7fffffffu) return hipErrorInvalidValue;
    if (p.tonemap == RT_TONEMAP_REINHARD) return launch_transform<RT_TONEMAP_REINHARD>(p, (unsigned)blocks, stream);
    if (p.tonemap == RT_TONEMAP_ACES) return launch_transform<RT_TONEMAP_ACES>(p, (unsigned)blocks, stream);
    return launch_transform<RT_TONEMAP_NONE>(p, (unsigned)blocks, stream);
}
