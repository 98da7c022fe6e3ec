// rt_build.h — the parameter block and the launcher of the BVH rebuild behind rebuildBvh (include/rt_api.h, "editing the scene").  Its own
// header, as the passes' are: no other kernel translation unit sees it, so their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"

// Elements one workgroup of the scan kernels covers (one per lane): rt_api.h exports it, the tests take their sizes from it.
constexpr uint32_t kBuildTile = RT_REBUILD_TILE;

// Device words of workspace a rebuild of `n` visible triangles in a tree of `first_leaf` leaves needs (rt_build_carve lays them out).
size_t rt_build_workspace_words(uint32_t n, uint32_t first_leaf);

// The mesh scene's device arrays as the rebuild reads and writes them, and its workspace.  The host knows n (it mirrors the triangles).
struct RtBuildParams {
    const rt_triangle* slots_in;    // the leaf-ordered triangles as they are
    rt_triangle* slots_out;         // a second buffer of num_tris slots: receives the rebuilt order (the caller swaps the two)
    int32_t* old_slot;              // num_tris entries (rt_api.h)
    uint32_t* leaf_ofs;             // the per-leaf count bytes, (first_leaf + 3) / 4 words; nullptr = the scene has none (nppl > 255)
    uint32_t* work;                 // rt_build_workspace_words(n, first_leaf) words
    uint32_t num_tris;              // slots in either buffer
    uint32_t first_leaf;            // a power of two, 2 .. 2^30
    uint32_t nppl;
    uint32_t n;                     // visible triangles, <= RT_REBUILD_MAX_TRIS and <= first_leaf * nppl
};

// The whole rebuild on `stream` (gather, three sorts, one round of passes per tree level, emit); the order between the passes is the stream's.  The refit
// of the new slots is the caller's next step (rt_launch_refit).  29 + 10 * log2(first_leaf) launches (28 without leaf_ofs): gather 6, four radix passes of 5,
// 10 per level, emit 3.  Returns the hipError_t of the first launch that failed.
hipError_t rt_launch_rebuild(const RtBuildParams& p, hipStream_t stream);
