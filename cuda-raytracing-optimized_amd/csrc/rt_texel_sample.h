// rt_texel_sample.h — the lookup of sampleTexels / renderLightmap (include/rt_api.h, "sampling texels": the definition is stated there, once) as plain C++:
// no kernel and no HIP call in here, so the device kernels (rt_kernels_lightmap.hip) and the CPU twin (host/rt_texel_sample_host.cpp, rtSampleTexelsHost)
// compile the same text.  Both are built with -ffp-contract=off: every operation below is one fp32 rounding, operands in the order written; a comparison
// with a NaN is false.  tests/lightmap_reference.py restates it in numpy, independently.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_api.h"

#ifndef RT_SAMPLE_FN
#define RT_SAMPLE_FN static inline
#endif

// A hit is valid iff its prim is a slot of the live array whose v[0].x is not +-inf (the sentinel of the leaf padding; a NaN there is valid).
RT_SAMPLE_FN bool rt_sample_valid(const rt_triangle* slots, uint32_t num_slots, int32_t p) {
    if (p < 0 || (uint32_t)p >= num_slots) return false;
    const float x = slots[p].v[0].e[0];
    return !(x == INFINITY || x == -INFINITY);
}

// The atlas point of (hu, hv) on a triangle whose six texture coordinates are tc: mesh_texel's two lines, not wrapped.
RT_SAMPLE_FN void rt_sample_atlas_point(const float* tc, float hu, float hv, float* tcu, float* tcv) {
    const float w0 = 1 - hu - hv;
    *tcu = (hu * tc[2] + hv * tc[4] + w0 * tc[0]);
    *tcv = (hu * tc[3] + hv * tc[5] + w0 * tc[1]);
}

// Nearest: the texel column (row) of the atlas coordinate c in an atlas of n columns (rows).  A NaN gives 0.
RT_SAMPLE_FN int rt_sample_nearest(float c, int n) {
    float f = c * (float)n;
    f = f > 0.0f ? f : 0.0f;
    f = f < (float)(n - 1) ? f : (float)(n - 1);
    return (int)f;
}

// Bilinear: the two columns (rows) i0, i1 and the weight a of i1, clamped to the edge.  A NaN gives (0, 0, 0).
RT_SAMPLE_FN void rt_sample_linear(float c, int n, int* i0, int* i1, float* a) {
    float f = c * (float)n - 0.5f;
    f = f > -1.0f ? f : -1.0f;
    f = f < (float)n ? f : (float)n;
    const float f0 = floorf(f);
    *a = f - f0;
    const int k = (int)f0;                                      // -1 .. n
    *i0 = k < 0 ? 0 : k > n - 1 ? n - 1 : k;
    *i1 = k + 1 < 0 ? 0 : k + 1 > n - 1 ? n - 1 : k + 1;
}

// The taps of one hit: texel indices t[k] = y*W + x (not yet times C) and weights, in the order c00, c10, c01, c11; nearest has one tap and no weight.
struct RtSampleTaps {
    size_t t[4];
    float w[4];
    int bilinear;
};

RT_SAMPLE_FN void rt_sample_taps(float tcu, float tcv, int W, int H, int bilinear, RtSampleTaps* s) {
    s->bilinear = bilinear;
    if (!bilinear) {
        const int x = rt_sample_nearest(tcu, W), y = rt_sample_nearest(tcv, H);
        s->t[0] = s->t[1] = s->t[2] = s->t[3] = (size_t)y * W + x;
        s->w[0] = s->w[1] = s->w[2] = s->w[3] = 0.0f;
        return;
    }
    int x0, x1, y0, y1;
    float ax, ay;
    rt_sample_linear(tcu, W, &x0, &x1, &ax);
    rt_sample_linear(tcv, H, &y0, &y1, &ay);
    s->t[0] = (size_t)y0 * W + x0; s->t[1] = (size_t)y0 * W + x1;
    s->t[2] = (size_t)y1 * W + x0; s->t[3] = (size_t)y1 * W + x1;
    s->w[0] = ((1 - ax) * (1 - ay)); s->w[1] = (ax * (1 - ay));
    s->w[2] = ((1 - ax) * ay); s->w[3] = (ax * ay);
}

// c[j] of the definition: the plane value j of the hit, C floats per texel.
RT_SAMPLE_FN float rt_sample_channel(const float* planes, int C, const RtSampleTaps* s, int j) {
    if (!s->bilinear) return planes[s->t[0] * C + j];
    return s->w[0] * planes[s->t[0] * C + j] + s->w[1] * planes[s->t[1] * C + j] + s->w[2] * planes[s->t[2] * C + j] + s->w[3] * planes[s->t[3] * C + j];
}

// The value e (3 floats) of the taps in `mode`.  SH9 walks the coefficient index and accumulates the three channels, as the definition's left-to-right
// sum allows: a lane holds the four taps of one coefficient at a time, never 4 x 27 values.  nrm is read in SH9 only.
RT_SAMPLE_FN void rt_sample_value(const float* planes, int mode, const RtSampleTaps* s, const float* nrm, float* e) {
    if (mode == RT_GATHER_IRRADIANCE) {
        for (int ch = 0; ch < 3; ch++) e[ch] = rt_sample_channel(planes, 3, s, ch);
        return;
    }
    if (mode == RT_GATHER_VISIBILITY) {
        e[0] = e[1] = e[2] = rt_sample_channel(planes, 1, s, 0);
        return;
    }
    const float X = nrm[0], Y = nrm[1], Z = nrm[2];
    const float k[9] = { 0.282095f, 0.325735f, 0.325735f, 0.325735f, 0.273137f, 0.273137f, 0.078848f, 0.273137f, 0.136568f };
    const float b[9] = { 1.0f, Y, Z, X, (X * Y), (Y * Z), (3.0f * (Z * Z) - 1.0f), (X * Z), (X * X - Y * Y) };
    for (int ch = 0; ch < 3; ch++) e[ch] = k[0] * rt_sample_channel(planes, 27, s, ch);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 1; i < 9; i++)
        for (int ch = 0; ch < 3; ch++) e[ch] = e[ch] + k[i] * (rt_sample_channel(planes, 27, s, 3 * i + ch) * b[i]);
    for (int ch = 0; ch < 3; ch++) e[ch] = e[ch] > 0.0f ? e[ch] : 0.0f;
}

// The whole lookup of one hit: false (and e = 0) for an invalid one.
RT_SAMPLE_FN bool rt_sample_lookup(const rt_triangle* slots, uint32_t num_slots, int32_t p, float hu, float hv, const float* nrm, int W, int H, int mode,
                                   int bilinear, const float* planes, float* e) {
    e[0] = e[1] = e[2] = 0.0f;
    if (!rt_sample_valid(slots, num_slots, p)) return false;
    float tc[6], tcu, tcv;
    for (int i = 0; i < 6; i++) tc[i] = slots[p].texCoords[i];
    rt_sample_atlas_point(tc, hu, hv, &tcu, &tcv);
    RtSampleTaps s;
    rt_sample_taps(tcu, tcv, W, H, bilinear, &s);
    rt_sample_value(planes, mode, &s, nrm, e);
    return true;
}
