// rt_texel_filter.h — the footprint and the tap of filterTexels (include/rt_api.h, "filtering texels": the definition is stated there, once) as plain C++: no
// kernel, no HIP type and no HIP call in here, so the device kernels (rt_kernels_texel_filter.hip) and the CPU twin (host/rt_texel_filter_host.cpp,
// rtFilterTexelsHost) compile the same text.  Both are built with -ffp-contract=off and a correctly rounded division and square root: every operation below is
// one fp32 rounding, operands in the order written; a comparison with a NaN is false.  tests/texel_filter_reference.py restates it in numpy, twice.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/rt_api.h"

#ifndef RT_FILTER_FN
#define RT_FILTER_FN static inline
#endif

// max(x, 0): a NaN gives 0, a zero of either sign +0.
RT_FILTER_FN float rt_filter_max0(float x) { return x > 0.0f ? x : 0.0f; }

// The 5 x 5 B3-spline kernel: h = K[|dx|] * K[|dy|] (every product is exact).
RT_FILTER_FN float rt_filter_kernel(int dx, int dy) {
    const float K[3] = { 0.375f, 0.25f, 0.0625f };
    return K[dx < 0 ? -dx : dx] * K[dy < 0 ? -dy : dy];
}

// The footprint of a texel owned by triangle t in a W x H atlas: r2 = sigma_d^2 times the squared world length of one texel step, rz = 1 / (sigma_z times that
// length).  d is the raster's.  A degenerate footprint (f2 of 0, inf or NaN) needs no special case: see rt_api.h.
RT_FILTER_FN void rt_filter_footprint(const rt_triangle* t, int W, int H, float sigma_d, float sigma_z, float* r2, float* rz) {
    const float ax = t->texCoords[0], ay = t->texCoords[1], bx = t->texCoords[2], by = t->texCoords[3], cx = t->texCoords[4], cy = t->texCoords[5];
    const float d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    const float ux = (cy - ay) / d, vx = (ay - by) / d, uy = (ax - cx) / d, vy = (bx - ax) / d;
    float Gx[3], Gy[3];
    for (int k = 0; k < 3; k++) {
        const float e1 = t->v[1].e[k] - t->v[0].e[k], e2 = t->v[2].e[k] - t->v[0].e[k];
        Gx[k] = (ux * e1 + vx * e2) / (float)W;
        Gy[k] = (uy * e1 + vy * e2) / (float)H;
    }
    const float f2 = 0.5f * ((Gx[0] * Gx[0] + Gx[1] * Gx[1] + Gx[2] * Gx[2]) + (Gy[0] * Gy[0] + Gy[1] * Gy[1] + Gy[2] * Gy[2]));
    *r2 = (sigma_d * sigma_d) * f2;
    *rz = 1.0f / (sigma_z * sqrtf(f2));
}

// rc of iteration `it`: 1 / (sigma_c * 2^-it)^2 (the scaling is exact, barring underflow); 0 where sigma_c <= 0 (the colour weight is off).
RT_FILTER_FN float rt_filter_rc(float sigma_c, int it) {
    if (!(sigma_c > 0.0f)) return 0.0f;
    const float sc = sigma_c * (1.0f / (float)(1 << it));
    return 1.0f / (sc * sc);
}

// A tap that is not the centre, q inside the atlas and owned: *w = h * wn * wz (without the colour weight); returns the reach test.  k2 = (float)((dx*dx +
// dy*dy) * s * s).  np, Pp, r2, rz are the centre's, nq, Pq the tap's.  `squarings` is a constant where the caller is straight-line code.
RT_FILTER_FN bool rt_filter_tap(const float* np, const float* Pp, float r2, float rz, const float* nq, const float* Pq, float h, float k2, int squarings,
                                float* w) {
    const float e[3] = { Pq[0] - Pp[0], Pq[1] - Pp[1], Pq[2] - Pp[2] };
    const float d2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    const bool reach = d2 <= r2 * k2;
    float wn = rt_filter_max0(np[0] * nq[0] + np[1] * nq[1] + np[2] * nq[2]);
    for (int i = 0; i < squarings; i++) wn = wn * wn;
    const float pd = fabsf(np[0] * e[0] + np[1] * e[1] + np[2] * e[2]);
    float wz = rt_filter_max0(1.0f - pd * rz);
    wz = wz * wz;
    *w = h * wn * wz;
    return reach;
}

// The colour weight over the leading L = min(C, 3) floats of the centre's and the tap's values.
RT_FILTER_FN float rt_filter_colour(const float* cp, const float* cq, int L, float rc) {
    const float d0 = cp[0] - cq[0];
    float dd = d0 * d0;
    if (L == 3) {
        const float d1 = cp[1] - cq[1], d2 = cp[2] - cq[2];
        dd = dd + d1 * d1 + d2 * d2;
    }
    float wc = rt_filter_max0(1.0f - dd * rc);
    return wc * wc;
}
