// rt_gather.h — the parameter block and the launchers of gatherRadiance / rtGatherDirections (include/rt_api.h): the directions of one chunk of
// the caller's points, generated on the device into the batch arrays the radiance kernels (rt_params.h, RtRadianceBatch) and the any-hit kernels (RtRayBatch)
// run over, and the per-point reduction of what those kernels return.  Its own header, as the other passes' are: no other kernel translation unit sees it, so
// their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"

// One chunk: points [k0, k0 + pts) of the caller's list, directions [first, first + dirs) of each.  Ray (kp, j) - point k0 + kp, direction first + j - is
// entry kp * dirs + j of the per-ray arrays: point-major, the order rtGatherDirections returns - so the batch the tracing kernels see is entry for entry the
// list a caller of radianceRays / occludedRays would have passed for these points (DESIGN.md 3.29 has why that matters in RT_FP_FAST).
struct RtGatherParams {
    // per point of the chunk (pts entries)
    const float* pos;           // 3 floats
    const float* nrm;           // 3 floats; nullptr in RT_GATHER_SH9
    float* acc;                 // W floats: read where first > 0, written; nullptr = neither (first == 0 and the caller passed none: the sums are not kept)
    float* out;                 // W floats, or nullptr
    uint32_t* nrays;            // 1 word, or nullptr
    // per ray of the chunk (pts * dirs entries)
    float* org;                 // 3 floats: RtRadianceBatch::org / RtRayBatch::org
    float* dir;                 // 3 floats, raw D
    uint32_t* ids;              // g: RtRadianceBatch::ids
    float* t_max;               // RT_GATHER_VISIBILITY: RtRayBatch::t_max
    rt_vec3* L;                 // RtRadianceBatch::out: written by the tracing kernels, read by the reduction, as the next two
    uint32_t* rays;             // RtRadianceBatch::rays
    uint8_t* occluded;          // RtRayBatch::occluded
    uint32_t pts, dirs, first, dirs_total;
    uint32_t k0;                // the chunk's first point in the caller's list
    uint32_t base_id;
    int32_t mode;
    float bias;
    float t_max_value;          // max_dist > 0 ? max_dist : FLT_MAX
};

// k_gather_dirs: one lane per (point, direction) of the chunk; writes org, dir, ids and t_max where they are not nullptr.
hipError_t rt_launch_gather_dirs(const RtGatherParams& p, hipStream_t stream);
// k_gather_reduce: one lane per point; the sequential loop over the chunk's directions, then acc, out and nrays where they are not nullptr.
hipError_t rt_launch_gather_reduce(const RtGatherParams& p, hipStream_t stream);
