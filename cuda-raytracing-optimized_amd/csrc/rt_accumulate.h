// rt_accumulate.h — the parameter block and the launcher of the temporal accumulation (accumulateFrame, include/rt_api.h).  Its own header,
// as rt_denoise.h is: the kernel translation units of the renderer and of the denoiser do not see it, so their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"

// The history of one call is three planes of 16-byte records, npix entries each, row 0 = bottom, in one allocation of 3 * npix float4:
//   pos[q] = (P.xyz, N)   at rec[q]          geo[q] = (normal.xyz, prim as bits)   at rec[npix + q]          col[q] = (c.xyz, unused)   at rec[2 * npix + q]
// N = 0 marks a pixel without a first hit: never a tap.  A call reads the previous call's set (`prev`) at the four pixels around the reprojected hit point
// and writes its own (`next`) at its pixel: two sets, swapped by the host after every call.
struct RtAccumulateParams {
    rt_camera cam;              // the camera of this call: the centre ray, P(p)
    rt_vec3 prev_origin, prev_u, prev_v, prev_w;    // the camera of the previous call, C', and its constants (rt_launch_accumulate fills Lu .. Vl from prev_cam)
    float Lu, Lv, Lw, Hl, Vl;
    int32_t nx, ny;
    const float* albedo;        // guide planes of the whole image for this call's camera (rt_launch_guides_* with a rank-0-of-1 partition of ny rows)
    const float* normal;
    const float* depth;
    const int32_t* prim;
    const rt_vec3* in;          // the noisy frame
    rt_vec3* out;
    float* history;             // N(p) as a plane of its own for the caller, or null
    const float4* prev;         // 3 * npix: the previous call's records; not read without history
    float4* next;               // 3 * npix: this call's
    int32_t flags, has_history;
    float max_history, sigma_z, normal_min;
    const float4* motion;       // 2 * npix: (Pm, -), (nm, -) of rt_motion.h for this call's camera, with a pose marked and a history; null = P, n themselves
};

// One kernel: reprojection, the four taps, the blend, the records of the next call, out.  prev_cam is C' (ignored with has_history = 0).  Returns the
// hipError_t of the launch.
hipError_t rt_launch_accumulate(RtAccumulateParams p, const rt_camera& prev_cam, hipStream_t stream);
