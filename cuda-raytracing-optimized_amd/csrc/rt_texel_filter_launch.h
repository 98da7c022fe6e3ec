// rt_texel_filter_launch.h — the parameter block and the launchers of filterTexels (include/rt_api.h, "filtering texels"): the prologue that
// packs what a tap reads into 16-byte records, one a-trous launch per iteration and the scatter through the dilated source plane.  The arithmetic is
// rt_texel_filter.h (which the CPU twin compiles too); the raster in front of it is rasterTexels' own (rt_texels.h).  Its own header, as the other passes'
// are: no other kernel translation unit sees it, so their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"

// What marks the records of an unowned texel: the bits of rec[t].w.  The prologue stores an owned texel's r2 with every NaN made the canonical quiet one
// (a NaN only ever fails the reach test, whatever its payload), so no owned texel carries these bits.
constexpr uint32_t kFilterUnowned = 0xffffffffu;

// Whole-atlas device buffers of one filterTexels call, n = W * H texels, t = y * W + x.  What a tap reads is three 16-byte records (C = 1: two and a float):
//   rec[t] = (n.xyz, r2 - or kFilterUnowned)      rec[n + t] = (P.xyz, rz)      col: the values, see below
// rec never changes after the prologue; col is the ping-pong pair of the iterations.  The values of C = 1 are one float per texel (col as float*); those of
// C = 3 one float4 (rgb, unused); those of C = 27 nine float4 planes, group g = channels 3g .. 3g+2 at col[g * n + t].
struct RtTexelFilterParams {
    const rt_triangle* slots;   // the live leaf-ordered slots
    const int32_t* owner;       // the raster's owner plane: the lowest covering slot, INT32_MAX = none
    const int32_t* src;         // the raster's source plane after `dilate` iterations
    int32_t W, H, C;            // C = rtGatherWidth(mode): 1, 3 or 27
    int32_t normal_squarings;
    float sigma_d, sigma_z, sigma_c;
    const float* in;            // C floats per texel (read at owned texels only)
    float* out;                 // C floats per texel
    float4* rec;                // 2 * n
    void* col[2];               // see above
};

// One lane per texel: rec and col[0].
hipError_t rt_launch_texel_filter_prologue(const RtTexelFilterParams& p, hipStream_t stream);
// Iteration `it` (stride 1 << it): col[it & 1] -> col[~it & 1] at owned texels.
hipError_t rt_launch_texel_filter_iteration(const RtTexelFilterParams& p, int it, hipStream_t stream);
// One lane per texel: out(t) = col[iterations & 1] at src(t), zeros where src(t) == -1.
hipError_t rt_launch_texel_filter_scatter(const RtTexelFilterParams& p, int iterations, hipStream_t stream);
