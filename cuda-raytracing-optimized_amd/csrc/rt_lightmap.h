// rt_lightmap.h — the parameter blocks and the launchers of sampleTexels / renderLightmap (include/rt_api.h, "sampling texels"): the lookup
// kernel over a chunk of the caller's hits, and around the unchanged closest-hit ray kernel (k_rays_mesh<false>, rt_launch_rays_mesh) the generator of a
// chunk of centre rays and the shade kernel.  The lookup's arithmetic is rt_texel_sample.h (which the CPU twin compiles too).  Its own header, as the other
// passes' are: no other kernel translation unit sees it, so their objects do not change with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_params.h"

constexpr int kLightmapBlock = 256;

// The texel planes a lookup reads and how: W x H texels of rtGatherWidth(mode) floats, row 0 first, on the device.
struct RtTexelSource {
    const float* planes;
    int32_t W, H, mode;
    int32_t bilinear;           // RT_SAMPLE_BILINEAR
};

// One chunk of sampleTexels: n hits on the device.
struct RtSampleParams {
    const rt_triangle* slots;   // the live leaf-ordered slots
    uint32_t num_slots;
    RtTexelSource src;
    const int32_t* prim;        // n
    const float* uv;            // n x 2
    const float* normal;        // n x 3, or nullptr (SH9 needs it)
    float* out;                 // n x 3
    uint8_t* valid;             // n, or nullptr
    uint32_t* count;            // one word: += the valid hits of the chunk
    int32_t n;
};

// One chunk of renderLightmap: pixels [first, first + n) of the whole image, pixel id = row * nx + column, row 0 at the bottom.  org / dir are the ray
// buffers the generator fills and the ray kernel and the shade kernel read; t / prim / normal / uv are the ray kernel's planes.
struct RtLightmapParams {
    float* org;                 // n x 3
    float* dir;                 // n x 3
    const float* t;             // n
    const int32_t* prim;        // n
    const float* normal;        // n x 3
    const float* uv;            // n x 2
    uint32_t num_slots;
    RtTexelSource src;
    int32_t albedo;             // RT_LIGHTMAP_ALBEDO
    float floor_value[3];
    rt_vec3* out;               // n
    uint32_t first;
    int32_t n;
};

// One lane per hit: out, valid and the count.
hipError_t rt_launch_sample_texels(const RtSampleParams& p, hipStream_t stream);
// One lane per pixel of the chunk: renderGuides' centre ray into org / dir (of the scene's block: camera and image size).
hipError_t rt_launch_lightmap_rays(const RtMeshParams& p, const RtLightmapParams& l, hipStream_t stream);
// One lane per pixel of the chunk: the lookup at a triangle hit, floor_value at a floor hit, the sky at a miss; with `albedo` times RT_GUIDE_ALBEDO's value.
hipError_t rt_launch_lightmap_shade(const RtMeshParams& p, const RtLightmapParams& l, hipStream_t stream);
