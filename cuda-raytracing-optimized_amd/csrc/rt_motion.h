// rt_motion.h — the parameter block and the launchers of the motion planes (rtMarkPose / renderMotion, include/rt_api.h): where the surface
// point of every pixel's first hit was in the marked pose of the scene, the normal it had there, and where the previous camera saw it.  Its own header, as
// rt_accumulate.h and rt_preview.h are: no other kernel translation unit sees it, so their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"

// The planes of one call are two planes of 16-byte records, npix entries each, row 0 = bottom, in one allocation of 2 * npix float4:
//   pos[p] = (Pm.xyz, 0)   at planes[p]          nrm[p] = (nm.xyz, 0)   at planes[npix + p]
// the layout k_accumulate<.., MOTION = true> and k_preview_temporal<.., MOTION = true> read at their own pixel.  `screen`, when asked for, is a plane of npix
// float2 of its own.  The kernel has no traversal: it reads the whole-image guide planes of the call's camera, the live primitive and the marked one.
struct RtMotionParams {
    rt_camera cam;              // the camera of this call: the centre ray, P(p)
    rt_vec3 prev_origin, prev_u, prev_v, prev_w;    // C' of the screen plane and its constants (rt_launch_motion fills Lu .. Vl from prev_cam); not read without `screen`
    float Lu, Lv, Lw, Hl, Vl;
    int32_t nx, ny;
    const float* normal;        // guide planes of the whole image for this call's camera
    const float* depth;
    const int32_t* prim;
    const rt_triangle* live;    // mesh scenes: the leaf-ordered triangle slots as they are now and
    const rt_triangle* mark;    // as rtMarkPose saw them (the same layout; carried along by rebuildBvh); null = no pose is marked
    const float4* live_sph;     // sphere scenes: (center, radius) in the caller's order, now and
    const float4* mark_sph;     // as rtMarkPose saw them; null = no pose is marked
    uint32_t count;             // slots / spheres of the arrays above: a primitive id outside [0, count) is taken as "not moved"
    float4* planes;             // 2 * npix
    float2* screen;             // npix, or null
};

// One kernel, one lane per pixel.  prev_cam is the C' of the screen plane (ignored with screen = null).  Returns the hipError_t of the launch.
hipError_t rt_launch_motion(RtMotionParams p, const rt_camera& prev_cam, hipStream_t stream);

// rebuildBvh carries the mark along: out[s] = old_slot[s] >= 0 ? in[old_slot[s]] : a sentinel (all nine coordinates +inf, everything else zero), s < count.
// An old_slot outside [0, count) is taken as a sentinel's.
hipError_t rt_launch_motion_gather(const rt_triangle* in, rt_triangle* out, const int32_t* old_slot, uint32_t count, hipStream_t stream);
