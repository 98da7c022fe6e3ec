// rt_renorm.h — unit_vector (vec3.h:194) of a direction that is a unit vector already, without the square root and the three divisions.
//
// hit() rebuilds the ray from the path (kernels.cu:325-360, ray.h:9), so every traced ray normalises a direction that start_sample / shade stored as
// unit(v) one step earlier.  The bits of that second normalisation are part of the image, and they are almost always a trivial function of the input: this
// header returns them from the class of s2 and one fused multiply-add per component.  Plain C++: no kernel and no HIP call in here, so a host program that
// includes it runs the same code as the render kernels (tests/renorm_dump.cpp, tests/test_renorm.py).
//
// PARITY only: the un-fused products of s2 and the IEEE quotient it replaces are those of the -ffp-contract=off objects.  The FAST objects keep unit().
//
// The argument, every step of it enumerated on the host (tests/renorm_dump.cpp; `--exhaustive` walks all 2^32 patterns per divisor):
//
//   1. s2 -> l2.  Write eps = 2^-24 (the spacing of floats below 1; above 1 it is 2 eps) and k = bits(s2) - bits(1.0f).  sqrtf is correctly rounded, so
//      for the ten values of s2 next to 1 (k = -6 .. 3) l2 = sqrtf(s2) = 1 + t eps with
//          k = -6, -5    t = -3    l2 = 0x3f7ffffd
//          k = -4, -3    t = -2    l2 = 0x3f7ffffe
//          k = -2, -1    t = -1    l2 = 0x3f7fffff
//          k =  0,  1    t =  0    l2 = 0x3f800000
//          k =  2,  3    t =  2    l2 = 0x3f800001
//      i.e. t = (k >> 1) + (k >= 2).  k = -7 gives 1 - 4 eps and k = 4 gives 1 + 4 eps: neither is handled, and neither is mapped to a t (the range test).
//   2. x -> RN(x / l2).  Division is per component, so for a fixed l2 the quotient is a function of one float.  x / l2 = x + x (1 / l2 - 1), and for each
//      of the five divisors there is a float r next to 1 / l2 - 1 for which the ONE rounding of fmaf(x, r, x) is the rounding of the quotient for EVERY
//      finite non-zero float x - denormals, the binade edges and the overflow at the top included (a neighbour of r one step to either side fails for 2
//      in 10^7; an infinite x, whose s2 is not a handled one, would give inf - inf for r <= 0):
//          t = -3   r = 0x34400003 = 3 eps + 12 eps^2          t = -1   r = 0x33800001 = eps + 2 eps^2          t = 2   r = 0xb3fffffe = -2 eps + 4 eps^2
//          t = -2   r = 0x34000001 = 2 eps +  4 eps^2          t =  0   r = 0
//      These five are the roundings of -d + 1.125 d^2 for d = t eps (the true 1 / l2 - 1 is -d + d^2 - ...; the factor 1.125 moves each onto the float
//      that works), which is how rt_renorm_r computes them: both products exact, one rounding.
//      What it looks like in bits (`--runs` prints it): t = -1 adds 1 to the magnitude bits of every float; t = -2 adds 1 below the mantissa 0x3fffff and 2
//      from there; t = -3 adds 2 below 0x555553, 3 from there and 2 at 0x7fffff (the quotient enters the next binade, whose steps are twice the size);
//      t = 2 subtracts 1 for the mantissas 1 .. 0x400001, 2 from there and 2 at 0 (the lower binade, half the step).
//   3. Zeros.  fmaf keeps the sign of a zero except for t = 2, where r < 0 makes -0 into +0.  A vector with a zero component takes the plain path
//      (its squares are at hand: one minimum and one comparison; a component below 2^-75, whose square is zero, goes with it).  The render path's
//      directions - a hit normal plus a random offset, a reflection, a refraction - have no zero components outside hand-made inputs.
//   4. Everything else.  Any other s2 - a direction that is not unit (the subsurface event of the dormant presets, the raw directions of the ray queries and
//      the probes), an infinity, a NaN - takes the plain path: a / sqrt(s2), today's code.
#pragma once

#include <stdint.h>

#ifndef RT_RENORM_FN
#define RT_RENORM_FN static inline
#endif

struct RtRenorm3 { float x, y, z; };

RT_RENORM_FN uint32_t rt_renorm_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
RT_RENORM_FN float rt_renorm_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

constexpr uint32_t kRenormOne = 0x3f800000u;           // bits(1.0f)
constexpr int kRenormKMin = -6, kRenormKMax = 3;       // the handled s2: bits(1.0f) + k

// is s2 one of the ten handled values?
RT_RENORM_FN bool rt_renorm_handled(float s2) { return rt_renorm_bits(s2) - (kRenormOne + (uint32_t)kRenormKMin) <= (uint32_t)(kRenormKMax - kRenormKMin); }
// t of a handled s2: sqrtf(s2) == 1 + t * 2^-24
RT_RENORM_FN int rt_renorm_t(float s2) { const int k = (int)(rt_renorm_bits(s2) - kRenormOne); return (k >> 1) + (k >= 2 ? 1 : 0); }
// the divisor that t stands for (the tests hold it against sqrtf)
RT_RENORM_FN float rt_renorm_l2(int t) { return 1.0f + (float)t * 0x1p-24f; }
// the multiplier of step 2 for t = -3 .. 0 and 2
RT_RENORM_FN float rt_renorm_r(int t) { const float d = (float)t * 0x1p-24f; return __builtin_fmaf(d, (float)t * 0x1.2p-24f, -d); }
// RN(x / l2) for every float x, r = rt_renorm_r(t); a zero keeps its sign unless r < 0
RT_RENORM_FN float rt_renorm_component(float x, float r) { return __builtin_fmaf(x, r, x); }

// The exact path: true and *out = unit(a) when s2 is handled and no component is zero, false (and *out of no meaning) otherwise.  Straight-line code: the
// kernels run it for every lane and branch once, on whether any lane with a ray got false.
RT_RENORM_FN bool rt_renorm_exact(float x, float y, float z, RtRenorm3* out) {
    const float xx = x * x, yy = y * y, zz = z * z;
    const float s2 = xx + yy + zz;                                                              // vec3.h:35-36, the reference's roundings
    const float r = rt_renorm_r(rt_renorm_t(s2));
    out->x = rt_renorm_component(x, r);
    out->y = rt_renorm_component(y, r);
    out->z = rt_renorm_component(z, r);
    const float least = __builtin_fminf(xx, __builtin_fminf(yy, zz));
    return rt_renorm_handled(s2) && least > 0.0f;
}

// the plain path: vec3.h:194 as written
RT_RENORM_FN RtRenorm3 rt_renorm_plain(float x, float y, float z) {
    const float l2 = __builtin_sqrtf(x * x + y * y + z * z);
    return { x / l2, y / l2, z / l2 };
}

// unit_vector(a), bit for bit
RT_RENORM_FN RtRenorm3 rt_renorm_unit(float x, float y, float z) {
    RtRenorm3 r;
    if (rt_renorm_exact(x, y, z, &r)) return r;
    return rt_renorm_plain(x, y, z);
}
