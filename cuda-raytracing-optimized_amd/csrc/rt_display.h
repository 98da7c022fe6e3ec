// rt_display.h — the parameter block and the launchers of displayFrame (include/rt_api.h): the luminance histogram of the input frame, the
// median and the adapted exposure from it, and the transform exposure -> tone map -> sRGB -> dither -> RGBA bytes.  Its own header, as the other passes' are:
// no other kernel translation unit sees it, so their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_api.h"

// `state` is two floats on the device: state[0] = E, the adapted exposure (E' of the next RT_DISPLAY_AUTO_EXPOSURE call: it stays there between calls),
// state[1] = E_used of this call.  Written by the resolve kernel, read by the transform behind it on the same stream; null without auto exposure.
struct RtDisplayParams {
    const rt_vec3* in;          // the linear frame, row 0 = bottom
    uint32_t* out;              // one word per pixel: R | G << 8 | B << 16 | 255 << 24 (the bytes R, G, B, 255 in memory)
    uint32_t* hist;             // RT_DISPLAY_BINS counts; cleared on the stream before the histogram kernel
    float* state;
    int32_t nx, ny;
    int32_t flags, tonemap;
    int32_t adapted;            // 1: state[0] holds the E of a previous call; 0: the first call after a reset
    float exposure, adapt;
};

// (a) The histogram of lum(in) into p.hist: per workgroup in the LDS, then one global atomic per non-zero bin.  Each launcher returns the hipError_t of its launch.
hipError_t rt_launch_display_histogram(const RtDisplayParams& p, hipStream_t stream);
// (b) One workgroup: prefix sum, median bin, target, E and E_used into p.state.
hipError_t rt_launch_display_resolve(const RtDisplayParams& p, hipStream_t stream);
// (c) One pixel per lane: 12 bytes in, one word out.  E_used is p.state[1], or p.exposure by value where p.state is null.
hipError_t rt_launch_display_transform(const RtDisplayParams& p, hipStream_t stream);
