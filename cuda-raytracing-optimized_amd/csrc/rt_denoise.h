// rt_denoise.h — the parameter block and the launchers of the preview denoiser (denoiseFrame, include/rt_api.h).  Its own header: the kernel
// translation units of the renderer do not see it, so their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"

// Whole-image device buffers of one denoiseFrame call, npix = nx * ny entries each, row 0 = bottom.  What a tap reads is three 16-byte records:
//   geo[q] = (normal.xyz, prim as bits)      pos[q] = (P.xyz, rz)      col[q] = (c.xyz, unused)
// geo and pos never change after the prologue; col is the ping-pong pair of the iterations.  rec holds geo and pos: RT_DENOISE_INTERLEAVED = 0 as two
// planes (geo at rec[q], pos at rec[npix + q]), 1 as one 32-byte record per pixel (rec[2q], rec[2q + 1]) - the A/B of DESIGN.md 3.11.
#ifndef RT_DENOISE_INTERLEAVED
#define RT_DENOISE_INTERLEAVED 0
#endif

struct RtDenoiseParams {
    rt_camera cam;
    int32_t nx, ny;
    const float* albedo;        // guide planes of the whole image (rt_launch_guides_* with a rank-0-of-1 partition of ny rows)
    const float* normal;
    const float* depth;
    const int32_t* prim;
    const rt_vec3* in;          // the noisy frame
    rt_vec3* out;               // the result (a different buffer: the last iteration writes it while others still read col)
    float4* rec;                // 2 * npix
    float4* col[2];             // npix each
    int32_t flags, normal_squarings;
    float sigma_z, sigma_c;
};

// prologue: P, rz, demodulated colour -> rec, col[0]; pixels without a first hit: out = in.  Returns the hipError_t of the launch.
hipError_t rt_launch_denoise_prologue(const RtDenoiseParams& p, hipStream_t stream);
// iteration `it` (stride 1 << it) from col[it & 1] into col[~it & 1]; last = 1: re-modulates and writes p.out instead (the fused epilogue).
hipError_t rt_launch_denoise_iteration(const RtDenoiseParams& p, int it, int last, hipStream_t stream);
