// rt_update.h — the parameter block and the launcher of the BVH refit behind updateTriangles (include/rt_api.h, "editing the scene").  Its own
// header, as the passes' are: no other kernel translation unit sees it, so their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"

// The mesh scene's device arrays as the refit reads and writes them (rt_params.h has the layouts: RtMeshParams::tris, bvh4, bvh_axis, leaf_tri).
struct RtRefitParams {
    const rt_triangle* slots;   // the leaf-ordered triangles: leaf L owns slots [(L - first_leaf) * nppl, + nppl)
    float* nodes;               // heap-indexed nodes, 6 floats each (min.xyz, max.xyz): nodes 1 .. 2 * first_leaf - 1 are rewritten
    float* axis;                // the 96-byte child-pair records: records 1 .. first_leaf - 1 are rewritten
    float4* leaf_rec;           // the compact leaf records, 3 float4 per slot: the real slots are rewritten; nullptr = the scene has none
    uint32_t first_leaf;        // a power of two, 2 .. 2^30
    uint32_t nppl;
};

// The whole refit on `stream`: the bottom kernel (leaf records, leaf boxes, the lowest 8 levels) and the upper kernel once per further 8 levels; the order
// between them is the stream's.  Returns the hipError_t of the first launch that failed.
hipError_t rt_launch_refit(const RtRefitParams& p, hipStream_t stream);
