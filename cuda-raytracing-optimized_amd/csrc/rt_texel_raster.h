// rt_texel_raster.h — the UV-atlas raster of rasterTexels / bakeTexels (include/rt_api.h, "baking texels": the definition is stated there, once) as plain C++:
// no kernel and no HIP call in here, so the device kernels (rt_kernels_texels.hip) and the CPU twin (host/rt_texels_host.cpp, rtRasterTexelsHost) compile the
// same text.  Both are built with -ffp-contract=off and a correctly rounded division and square root: every operation below is one fp32 rounding, operands in
// the order written; a comparison with a NaN is false.  tests/texels_reference.py restates it in numpy, independently.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/rt_api.h"

#ifndef RT_TEXEL_FN
#define RT_TEXEL_FN static inline
#endif

// The sample point of texel (x, y) of a W x H atlas.
RT_TEXEL_FN void rt_texel_sample(int x, int y, int W, int H, float* s) {
    s[0] = ((float)x + 0.5f) / (float)W;
    s[1] = ((float)y + 0.5f) / (float)H;
}

// A slot is a candidate unless its v[0].x is +-inf (the sentinel of the leaf padding; a NaN there is a candidate).
RT_TEXEL_FN bool rt_texel_candidate(const rt_triangle* t) {
    const float x = t->v[0].e[0];
    return !(x == INFINITY || x == -INFINITY);
}

// The UV box of a triangle: box = (umin, umax, vmin, vmax), each from vertex a, then b, then c by < / >.  A NaN in a makes the bound a NaN: the box test
// below then fails at every texel.
RT_TEXEL_FN void rt_texel_box(const float* tc, float* box) {
    float umin = tc[0], umax = tc[0], vmin = tc[1], vmax = tc[1];
    if (tc[2] < umin) umin = tc[2];
    if (tc[4] < umin) umin = tc[4];
    if (tc[2] > umax) umax = tc[2];
    if (tc[4] > umax) umax = tc[4];
    if (tc[3] < vmin) vmin = tc[3];
    if (tc[5] < vmin) vmin = tc[5];
    if (tc[3] > vmax) vmax = tc[3];
    if (tc[5] > vmax) vmax = tc[5];
    box[0] = umin; box[1] = umax; box[2] = vmin; box[3] = vmax;
}

// Box test and inside test of the sample point s against the UV triangle tc; h = (hu, hv) where it returns true.
RT_TEXEL_FN bool rt_texel_cover(const float* tc, const float* box, const float* s, float* h) {
    if (!(box[0] <= s[0] && s[0] <= box[1] && box[2] <= s[1] && s[1] <= box[3])) return false;
    const float ax = tc[0], ay = tc[1], bx = tc[2], by = tc[3], cx = tc[4], cy = tc[5];
    const float d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    if (!(d != 0.0f)) return false;
    const float w1 = (s[0] - ax) * (cy - ay) - (s[1] - ay) * (cx - ax);
    const float w2 = (bx - ax) * (s[1] - ay) - (by - ay) * (s[0] - ax);
    const float hu = w1 / d, hv = w2 / d;
    const float w0 = 1.0f - hu - hv;
    if (!(hu >= 0.0f && hv >= 0.0f && w0 >= 0.0f)) return false;
    h[0] = hu; h[1] = hv;
    return true;
}

// Position and geometric normal of the owner at (hu, hv): cross and unit are renderMotion's (rt_api.h).
RT_TEXEL_FN void rt_texel_resolve(const rt_triangle* t, const float* h, float* pos, float* nrm) {
    float e1[3], e2[3];
    for (int k = 0; k < 3; k++) {
        e1[k] = t->v[1].e[k] - t->v[0].e[k];
        e2[k] = t->v[2].e[k] - t->v[0].e[k];
        pos[k] = t->v[0].e[k] + h[0] * e1[k] + h[1] * e2[k];
    }
    const float c[3] = { e1[1] * e2[2] - e1[2] * e2[1], -(e1[0] * e2[2] - e1[2] * e2[0]), e1[0] * e2[1] - e1[1] * e2[0] };
    const float l = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    nrm[0] = c[0] / l; nrm[1] = c[1] / l; nrm[2] = c[2] / l;
}

// One texel of one dilation iteration: the source of t = (x, y) from the previous plane.
RT_TEXEL_FN int32_t rt_texel_dilate(const int32_t* prev, int x, int y, int W, int H) {
    const int32_t own = prev[(size_t)y * W + x];
    if (own != -1) return own;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const int32_t q = prev[(size_t)qy * W + qx];
            if (q != -1) return q;
        }
    return -1;
}

// The texel columns (or rows) [*lo, *hi] a walk over the box bound [bmin, bmax] has to visit in an atlas of n columns: the exact range padded by one texel per
// side and clipped to the atlas; empty (*lo > *hi) where the bound is a NaN or lies outside.  Only a bound of the walk: the box test decides.
RT_TEXEL_FN void rt_texel_span(float bmin, float bmax, int n, int* lo, int* hi) {
    *lo = 0; *hi = -1;
    if (!(bmin <= bmax)) return;
    const float a = floorf(bmin * (float)n) - 1.0f, b = floorf(bmax * (float)n) + 1.0f;
    if (a > (float)(n - 1) || b < 0.0f) return;
    *lo = a < 0.0f ? 0 : (int)a;
    *hi = b > (float)(n - 1) ? n - 1 : (int)b;
}
