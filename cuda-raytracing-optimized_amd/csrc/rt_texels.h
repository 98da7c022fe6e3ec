// rt_texels.h — the parameter block and the launchers of rasterTexels / bakeTexels (include/rt_api.h, "baking texels"): the UV-atlas raster
// over the live leaf-ordered triangle slots, the dilation, the compaction of the owned texels into a list, the generator that draws a chunk of that list's
// directions into the batch arrays the radiance and any-hit kernels run over, and the scatter of the per-point results back into texel planes.  The per-point
// fold between them is gatherRadiance's own (rt_gather.h, rt_launch_gather_reduce).  Its own header, as the other passes' are: no other kernel translation
// unit sees it, so their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"
#include "rt_gather.h"

constexpr int kTexelBlock = 256;        // texels per workgroup of the per-texel kernels: one entry of `counts` each

// The raster's planes (W * H entries each, t = y * W + x) and the compact list.  A plane pointer that is nullptr is not written.
struct RtTexelParams {
    const rt_triangle* slots;   // the live leaf-ordered slots (RtMeshParams::tris)
    uint32_t num_slots;
    int32_t W, H;
    int32_t* owner;             // the lowest covering slot, INT32_MAX = none: cleared, then atomicMin
    int32_t* prim;              // owner, RT_GUIDE_PRIM_NONE = none
    int32_t* src[2];            // the dilation's ping-pong pair: src_i lives in src[i & 1]
    float* bary;                // 2 floats
    float* pos;                 // 3 floats
    float* nrm;                 // 3 floats
    uint32_t* counts;           // owned texels per workgroup of kTexelBlock texels, then (after the scan) the list position of the workgroup's first
    uint32_t blocks;            // ceil(W * H / kTexelBlock)
    uint32_t* length;           // one word: the list's length
    int32_t* rank;              // per texel: its position in the list (owned texels only)
    uint32_t* list;             // the owned texels, ascending
    float* list_pos;            // 3 floats per list entry
    float* list_nrm;            // 3 floats per list entry
};

// The planes and the compact per-entry arrays of a bake; Wd = rtGatherWidth(mode).
struct RtTexelBakeParams {
    const int32_t* src;         // the dilated source plane
    const int32_t* rank;
    const uint32_t* list;
    uint32_t length;
    uint32_t texels;            // W * H
    int32_t Wd;
    float* acc_plane;           // Wd floats per texel, or nullptr
    float* out_plane;           // Wd floats per texel, or nullptr
    uint32_t* rays_plane;       // one word per texel, or nullptr
    float* acc;                 // Wd floats per list entry (RtGatherParams::acc of chunk k0 is acc + k0 * Wd), or nullptr
    float* out;
    uint32_t* nrays;
};

// Clears owner, then one wave per slot: atomicMin of the slot over the texels of its clipped UV box that it covers.
hipError_t rt_launch_texel_coverage(const RtTexelParams& p, hipStream_t stream);
// One lane per texel: prim, src[0], bary, pos, nrm and the workgroup's owned count.
hipError_t rt_launch_texel_resolve(const RtTexelParams& p, hipStream_t stream);
// Dilation iteration i (1-based): src[(i - 1) & 1] -> src[i & 1].
hipError_t rt_launch_texel_dilate(const RtTexelParams& p, int i, hipStream_t stream);
// The exclusive scan of counts (one workgroup) with the total in *length: the one word the host reads back, to size the list.
hipError_t rt_launch_texel_scan(const RtTexelParams& p, hipStream_t stream);
// One lane per texel: rank, list and - where list_pos is not nullptr - list_pos, list_nrm.
hipError_t rt_launch_texel_compact(const RtTexelParams& p, hipStream_t stream);
// One lane per (list entry, direction) of the chunk g describes - g.k0 the chunk's first list entry, g.pos / g.nrm its first packed point -: the point's index k
// is list[g.k0 + kp].  Fills g.org, g.dir, g.ids, g.t_max where they are not nullptr.
hipError_t rt_launch_texel_dirs(const RtGatherParams& g, const uint32_t* list, hipStream_t stream);
// One lane per list entry: acc of the entry from acc_plane (the sums a call with first > 0 resumes from).
hipError_t rt_launch_texel_fetch(const RtTexelBakeParams& b, hipStream_t stream);
// One lane per texel: out_plane through src and rank; acc_plane and rays_plane at owned texels, 0 elsewhere.
hipError_t rt_launch_texel_scatter(const RtTexelBakeParams& b, hipStream_t stream);
