// rt_preview.h — the parameter block and the launchers of previewFrame (include/rt_api.h): temporal accumulation with luminance moments, the
// per-pixel variance from them and the variance-guided a-trous filter, in one device pass.  Its own header, as rt_denoise.h and rt_accumulate.h are: the
// kernel translation units of the renderer, the denoiser and the accumulation do not see it, so their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"

// The history of one call is the three 16-byte record planes of rt_accumulate.h, npix entries each in one allocation of 3 * npix float4, and an 8-byte plane
// of luminance moments:
//   pos[q] = (P.xyz, N)   at rec[q]        geo[q] = (normal.xyz, prim as bits)   at rec[npix + q]        col[q] = (c.xyz, unused)   at rec[2 * npix + q]
//   mom[q] = (M1, M2)
// N = 0 marks a pixel without a first hit: never a tap.  The temporal kernel reads the previous call's set (`prev`, `prev_mom`) and writes its own (`next`,
// `next_mom`): two sets, swapped by the host after every call.  The variance and the a-trous kernels read geo and pos of `next` (they do not change after the
// temporal kernel; col of `next` stays the UNFILTERED accumulated colour, the history of the next call) and the ping-pong pair `col`, whose records are
// (c.xyz, var): the variance travels in the word the denoiser's colour record leaves unused, so a tap of the filter stays three 16-byte loads.
struct RtPreviewParams {
    rt_camera cam;              // the camera of this call: the centre ray, P(p)
    rt_vec3 prev_origin, prev_u, prev_v, prev_w;    // the camera of the previous call, C', and its constants (rt_launch_preview_temporal fills Lu .. Vl from prev_cam)
    float Lu, Lv, Lw, Hl, Vl;
    int32_t nx, ny;
    const float* albedo;        // guide planes of the whole image for this call's camera (rt_launch_guides_* with a rank-0-of-1 partition of ny rows)
    const float* normal;
    const float* depth;
    const int32_t* prim;
    const rt_vec3* in;          // the noisy frame
    rt_vec3* out;
    float* history;             // N(p) as a plane of its own for the caller, or null
    float* variance;            // var(p) of stage V as a plane for the caller, or null
    const float4* prev;         // 3 * npix: the previous call's records; not read without history
    float4* next;               // 3 * npix: this call's
    const float2* prev_mom;     // npix: the previous call's moments; not read without history
    float2* next_mom;           // npix: this call's
    float4* col[2];             // npix each: (c.xyz, var) of the a-trous iterations
    int32_t flags, has_history, normal_squarings;
    float max_history, sigma_z, normal_min, sigma_l;
    const float4* motion;       // 2 * npix: (Pm, -), (nm, -) of rt_motion.h for this call's camera, with a pose marked and a history; null = P, n themselves
};

// Stage T: reprojection, the four taps, the blend of colour and moments, the records of the next call; pixels without a first hit: out = in.  prev_cam is C'
// (ignored with has_history = 0).  Each launcher returns the hipError_t of its launch.
hipError_t rt_launch_preview_temporal(RtPreviewParams p, const rt_camera& prev_cam, hipStream_t stream);
// Stage V: var(p) from the moments, or from the 7 x 7 neighbourhood where N(p) < RT_PREVIEW_MIN_HISTORY; writes col[0] = (c, var) and p.variance.
hipError_t rt_launch_preview_variance(const RtPreviewParams& p, hipStream_t stream);
// Stage A, iteration `it` (stride 1 << it) from col[it & 1] into col[~it & 1]; last = 1: re-modulates and writes p.out instead (the fused epilogue).
hipError_t rt_launch_preview_iteration(const RtPreviewParams& p, int it, int last, hipStream_t stream);
