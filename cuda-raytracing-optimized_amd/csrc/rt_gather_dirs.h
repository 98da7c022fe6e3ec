// rt_gather_dirs.h — the direction generator of gatherRadiance (include/rt_api.h, "gathering at points": the definition is stated there, once) as plain C++: no
// kernel and no HIP call in here, so the device kernel (rt_kernels_gather.hip) and the CPU twin (host/rt_gather_host.cpp, rtGatherDirectionsHost) compile the
// same text.  Both are built with -ffp-contract=off and a correctly rounded division and square root: every operation below is one fp32 rounding, operands in
// the order written.  tests/gather_reference.py restates it in numpy, independently.  (The hash, the seed and rnd are rt_device.h's; that header is
// device-only and every render kernel object depends on it, so the host twin's copies live here.)
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/rt_api.h"

#ifndef RT_GATHER_FN
#define RT_GATHER_FN static inline
#endif

RT_GATHER_FN uint32_t rt_gather_wang_hash(uint32_t seed) {      // rnd.h:31-39
    seed = (seed ^ 61u) ^ (seed >> 16);
    seed *= 9u;
    seed = seed ^ (seed >> 4);
    seed *= 0x27d4eb2du;
    seed = seed ^ (seed >> 15);
    return seed;
}
RT_GATHER_FN uint32_t rt_gather_pixel_seed(uint32_t id) {       // kernels.cu:541-542
    return (rt_gather_wang_hash(id) * 336343633u) | 1u;
}
RT_GATHER_FN float rt_gather_rnd(uint32_t* state) {             // rnd.h:5-18
    uint32_t x = *state;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 15;
    *state = x;
    return (float)(x & 0xFFFFFF) / 16777216.0f;
}

// g of ray (k, m): k the point's index in the caller's list, m the direction's index in 0 .. dirs_total - 1
RT_GATHER_FN uint32_t rt_gather_id(uint32_t base_id, uint32_t k, uint32_t dirs_total, uint32_t m) {
    return base_id + (uint32_t)((uint64_t)k * dirs_total + m);
}

// Origin o and raw direction D of the ray with id g at the point (P, N).  N is not read in RT_GATHER_SH9 (it may be NULL).  The rejection loop is the only
// loop: the seed is odd and xorshift32 never reaches 0 from a non-zero word, so the stream never stands still.
RT_GATHER_FN void rt_gather_ray(int mode, const float* P, const float* N, float bias, uint32_t g, float* o, float* D) {
    float nn[3] = { 0.0f, 0.0f, 0.0f };
    if (mode == RT_GATHER_SH9) {
        o[0] = P[0]; o[1] = P[1]; o[2] = P[2];
    } else {
        const float l = sqrtf(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
        for (int a = 0; a < 3; a++) {
            nn[a] = N[a] / l;
            o[a] = P[a] + bias * nn[a];
        }
    }
    uint32_t wd = rt_gather_pixel_seed(~g);
    float x, y, z, l2;
    do {                                                        // rnd.h:41-49, with the zero vector rejected as well
        x = 2.0f * rt_gather_rnd(&wd) - 1.0f;
        y = 2.0f * rt_gather_rnd(&wd) - 1.0f;
        z = 2.0f * rt_gather_rnd(&wd) - 1.0f;
        l2 = x * x + y * y + z * z;
    } while (!(l2 < 1.0f) || l2 == 0.0f);
    const float l = sqrtf(l2);
    const float u[3] = { x / l, y / l, z / l };
    if (mode == RT_GATHER_SH9) {
        D[0] = u[0]; D[1] = u[1]; D[2] = u[2];
    } else {
        D[0] = nn[0] + u[0]; D[1] = nn[1] + u[1]; D[2] = nn[2] + u[2];
        if (D[0] == 0.0f && D[1] == 0.0f && D[2] == 0.0f) { D[0] = nn[0]; D[1] = nn[1]; D[2] = nn[2]; }
    }
}

// y_0 .. y_8 of the raw direction D = (X, Y, Z)
RT_GATHER_FN void rt_gather_sh9(const float* D, float* y) {
    const float X = D[0], Y = D[1], Z = D[2];
    y[0] = 0.282095f;
    y[1] = 0.488603f * Y;
    y[2] = 0.488603f * Z;
    y[3] = 0.488603f * X;
    y[4] = 1.092548f * (X * Y);
    y[5] = 1.092548f * (Y * Z);
    y[6] = 0.315392f * (3.0f * (Z * Z) - 1.0f);
    y[7] = 1.092548f * (X * Z);
    y[8] = 0.546274f * (X * X - Y * Y);
}
