// rt_refine.h — the parameter block and the launchers of refineFrame (include/rt_api.h): the adaptive frame's per-pixel state, the selection of
// the pixels that get another batch, their list in cost order, the batch arrays the pixel kernels (rt_params.h, RtPixelBatch) run over, the update of the
// statistics and the planes for the caller.  Its own header, as the other passes' are: no other kernel translation unit sees it, so their objects do not
// change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"

// words[]: the class histogram, the per-class cursors of the scatter, the length of the list.  Cleared on the stream before the select kernels.
enum { kRefineClasses = 32, kRefineHist = 0, kRefineCursor = kRefineClasses, kRefineTotal = 2 * kRefineClasses, kRefineWords = 2 * kRefineClasses + 1 };

struct RtRefineParams {
    // the frame's state: planes of nx * ny entries, pixel id = j * nx + i
    uint4* state;               // (colour sum bits, xorshift word): renderPixels' state
    int32_t* n;                 // samples so far
    float2* mom;                // (M1, M2) of the batch means' luminance
    uint32_t* rays;             // closest-hit queries of the pixel's last batch
    float* lum;                 // lum(mean) after the pixel's last batch: l of its next update, l' of its error
    uint8_t* flag;              // this call's unconverged(p)
    uint8_t* cls;               // this call's active(p) ? cls(p) + 1 : 0
    uint32_t* list;             // the pixel ids of the pass, dearest class first
    uint32_t* words;
    // one chunk of the list as the pixel kernels read and write it: entries [chunk_first, chunk_first + chunk_n)
    int32_t* b_ij;
    int32_t* b_first;
    uint32_t* b_state;
    uint32_t* b_rays;
    uint32_t chunk_first, chunk_n;
    // the planes for the caller, nullptr = not requested (samples is the n plane itself)
    rt_vec3* out;
    float* err;
    int32_t nx, ny;
    int32_t batch, min_batches, max_samples, flags;
    float threshold;
    int32_t cost_order;         // 0: one class, the list in ascending pixel order (RT_REFINE_ORDER=0, measurements only)
};

// Select: (a) unconverged(p) from the statistics into p.flag; (b) dilation, sample cap and class into p.cls, the class histogram into p.words; (c) the list:
// class offsets by a scan over the 32 classes, positions by wave ballots, its length into p.words[kRefineTotal].  Returns the hipError_t of the last launch.
hipError_t rt_launch_refine_select(const RtRefineParams& p, hipStream_t stream);
// ij, first = n and the 16-byte state of the chunk's entries into the batch arrays.
hipError_t rt_launch_refine_gather(const RtRefineParams& p, hipStream_t stream);
// The chunk's states and rays back into the planes, and the update of n, M1, M2, lum.
hipError_t rt_launch_refine_update(const RtRefineParams& p, hipStream_t stream);
// mean and err planes, where requested.
hipError_t rt_launch_refine_deliver(const RtRefineParams& p, hipStream_t stream);
