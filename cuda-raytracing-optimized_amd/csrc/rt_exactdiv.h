// rt_exactdiv.h — the bounce's IEEE divisions by a divisor that is special, without the compiler's 11-instruction expansion per quotient.
//
// Every traced ray that hits divides the two roots of sphereHit by a = dot(dn, dn) (intersections.h:98,100), the three components of the hit offset by the
// radius (intersections.h:95) and the three components of the bounce direction by its length (vec3.h:194).  hipcc expands each correctly rounded quotient
// into v_div_scale x 2, v_rcp, five v_fma, v_mul, v_div_fmas, v_div_fixup.  The divisors are special: `a` is one of a handful of floats next to 1, and the
// three components of a vec3 / float share their divisor.  Plain C++: no kernel and no HIP call in here, so a host program that includes it runs the same
// code as the render kernels (tests/exactdiv_dump.cpp, tests/test_exactdiv.py).  The one thing the host cannot run is v_rcp_f32: the seed of form C is an
// argument, and the host check holds the twin for the seed RN(1 / l) (form C below says what that does and does not show).
//
// PARITY only: the quotients replaced are the IEEE ones of the -ffp-contract=off objects.  The FAST objects keep what they have.
//
// Form B: x / a in one fused multiply-add (the two roots of sphere_hit_exact).
//   a = dot(dn, dn) of a re-normalised direction.  Write eps = 2^-24 and k = bits(a) - bits(1.0f): a = 1 + k eps for k <= 0 and 1 + 2 k eps for k > 0.  Among
//   4 M directions unit(n + random_in_unit_sphere), re-normalised as hit() does, k is -4 .. 2 and nothing else (`exactdiv_dump --ahist`).  x / a =
//   x + x (1 / a - 1), and for each of the seven a there is a float r next to 1 / a - 1 for which the ONE rounding of fmaf(x, r, x) is the rounding of the
//   quotient for every float x bar the exceptions below - a statement about 7 x 2^32 cases, enumerated (`exactdiv_dump --exhaustive-a`), not derived:
//          k = -4   r = 0x34800002          k = -2   r = 0x34000001          k = 1   r = 0xb3fffffe
//          k = -3   r = 0x34400003          k = -1   r = 0x33800001          k = 2   r = 0xb47ffffc          k = 0   r = 0
//   These are the roundings of -d + 1.125 d^2 for d = a - 1 (exact: a is next to 1), which is how rt_exdiv_a_r computes them - as rt_renorm.h does for its
//   divisors: both products exact, one rounding.  The test holds the computed r to the seven enumerated words.
//   The exceptions, and no others: for k > 0 (r < 0) x = -0 gives +0 where the quotient is -0, and for k >= 0 (r <= 0) x = +-inf gives NaN (inf - inf,
//   inf * 0) where the quotient is inf.
//   Neither can change a result of sphere_hit_exact: a root `temp` counts only if temp > t_min && temp <= t_max.  A zero of either sign fails temp > t_min
//   for any t_min >= 0 (setRenderOptions refuses a negative t_min; rt_api.h: the caller of the ray queries owes 0 <= tmin).  An infinity and a NaN both
//   fail temp <= t_max (t_max is a hit distance or at most FLT_MAX).  A rejected root's bits go nowhere.
//   Any other a - a raw direction's, an unhandled k - keeps the division, under one branch.
//
// Form C: (x, y, z) / l with ONE reciprocal (unit() of a direction that is not unit yet; vec3 / float).
//   This is the compiler's own sequence with the part that depends on the divisor alone done once.  For q = x / l the AMDGPU back end emits (LowerFDIV32)
//          ls = v_div_scale(l, l, x)    xs = v_div_scale(x, l, x)
//          y0 = v_rcp(ls)    e = fma(-ls, y0, 1)    y = fma(e, y0, y0)
//          q0 = xs * y    q1 = fma(fma(-ls, q0, xs), y, q0)    q = v_div_fixup(v_div_fmas(fma(-ls, q1, xs), y, q1), l, x)
//   The ISA manual ("AMD Instinct MI300 / CDNA3 Instruction Set Architecture", VOP3 opcodes V_DIV_SCALE_F32, V_DIV_FMAS_F32, V_DIV_FIXUP_F32; CDNA4 keeps
//   them) gives the conditions: V_DIV_SCALE_F32 returns its first operand unchanged and VCC clear unless an operand is zero, exponent(x) - exponent(l) >= 96,
//   l is denormal, 1 / l is denormal (exponent(l) >= 253) or x / l is denormal (exponent(x) - exponent(l) <= -126, given the first two); V_DIV_FMAS_F32 is
//   the plain fma when VCC is clear; V_DIV_FIXUP_F32 returns its first operand, with the quotient's sign, unless an operand is NaN, infinite or zero, or the
//   quotient underflows (exponent(x) - exponent(l) < -150) or overflows.  So for finite non-zero x and l with both |x| and l in [2^-40, 2^40] (exponents
//   differ by at most 80 either way, the quotient is normal; a negative divisor is left to the plain path: a comparison without a modifier takes its
//   bound as a literal, one with |l| would need it in a register) the expansion IS
//          y0 = rcp(l)   e = fma(-l, y0, 1)   y = fma(e, y0, y0)                          once per divisor
//          q0 = x * y    q1 = fma(fma(-l, q0, x), y, q0)    q = fma(fma(-l, q1, x), y, q1)   per component
//   instruction for instruction on the same values: the same bits by construction, whatever v_rcp_f32 returns (the sign of q is that of the quotient: q is
//   within a few ulps of it and not zero).  18 instructions and one quarter-rate v_rcp_f32 where there were 33 and three; no v_div_scale, so no VCC write and
//   none of the wait states (s_nop) in front of v_div_fmas.  The host has no v_rcp_f32, so the twin takes y0 as an argument: `exactdiv_dump --shared` holds
//   q to x / l for the seed RN(1 / l) - a check of the transcription, not a new theorem - and counts the two neighbouring seeds apart (a seed 0.5 .. 1 ulp
//   from 1 / l misses the quotient for about 1 numerator in 10^8: that the division is correctly rounded is a property of the instruction's actual
//   results, the plain operator's as much as this form's).  What holds the device is rtProbeExactDiv: this form beside the plain operator, bit for bit.
//   Guard (rt_exdiv3_window / rt_exdiv_unit_window): every operand inside the window, tested so that a NaN, an infinity or a zero anywhere fails it.  Anything
//   else takes the plain operators under one branch.  The square root inside unit() is not touched.
//
// Where: the folded kinds of the sphere kernel's cost-ordered dispatch (rt_device.h, the template switch XD).  Every other kernel - the first dispatch, the
// general form, the diagnostic kinds, the ray queries, the guides, the mesh kernels - keeps the plain operators and compiles to what it was.
// rt_exdiv3 under rt_exdiv3_window, the form over a divisor of any size, was measured on the hit normal's (hp - c) / radius and did not pay on top of the
// other two: no kernel uses it; the probe and the host check hold it.  With the divisor's part taken out of the ray step altogether - rt_exdiv3_y: the
// refined reciprocal of a sphere's radius is stored beside the radius when the scene is staged - the same quotients do pay: the four-wave
// folded kinds use it for the hit normal.
#pragma once

#include <stdint.h>

#ifndef RT_EXDIV_FN
#define RT_EXDIV_FN static inline
#endif

struct RtExdiv3 { float x, y, z; };

RT_EXDIV_FN uint32_t rt_exdiv_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
RT_EXDIV_FN float rt_exdiv_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// ---- form B ---------------------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kExdivOne = 0x3f800000u;             // bits(1.0f)
constexpr int kExdivKMin = -4, kExdivKMax = 2;          // the handled a: bits(1.0f) + k

// is a one of the seven handled values?
RT_EXDIV_FN bool rt_exdiv_a_handled(float a) { return rt_exdiv_bits(a) - (kExdivOne + (uint32_t)kExdivKMin) <= (uint32_t)(kExdivKMax - kExdivKMin); }
// the multiplier of a handled a (of no meaning for any other)
RT_EXDIV_FN float rt_exdiv_a_r(float a) { const float d = a - 1.0f; return __builtin_fmaf(d, d * 1.125f, -d); }
// RN(x / a), r = rt_exdiv_a_r(a), bar the exceptions of the header
RT_EXDIV_FN float rt_exdiv_a_quot(float x, float r) { return __builtin_fmaf(x, r, x); }

// ---- form C ---------------------------------------------------------------------------------------------------------------------------------------------
constexpr float kExdivLo = 0x1p-40f, kExdivHi = 0x1p40f;       // the window of |x|, |y|, |z|, |l|

// the refined reciprocal that the three components share; y0 = v_rcp_f32(l) on the device
RT_EXDIV_FN float rt_exdiv_recip(float l, float y0) { return __builtin_fmaf(__builtin_fmaf(-l, y0, 1.0f), y0, y0); }
// RN(x / l) inside the window, y = rt_exdiv_recip(l, .)
RT_EXDIV_FN float rt_exdiv_component(float x, float l, float y) {
    const float q0 = x * y;
    const float q1 = __builtin_fmaf(__builtin_fmaf(-l, q0, x), y, q0);
    return __builtin_fmaf(__builtin_fmaf(-l, q1, x), y, q1);
}
RT_EXDIV_FN RtExdiv3 rt_exdiv3(float x, float y, float z, float l, float y0) {
    const float r = rt_exdiv_recip(l, y0);
    return { rt_exdiv_component(x, l, r), rt_exdiv_component(y, l, r), rt_exdiv_component(z, l, r) };
}
// rt_exdiv3 with the refined reciprocal given: y = rt_exdiv_recip(l, v_rcp_f32(l)) depends on the divisor alone, so a divisor that is a constant of the
// scene (a sphere's radius under the hit normal, intersections.h:95) has it computed once, when the scene is staged, and each hit runs the fifteen
// per-component instructions and no reciprocal.  Same bits as rt_exdiv3, hence as the plain operator inside the window: y is the same three instructions on
// the same value, and v_rcp_f32 returns the same result for the same input on the same device whenever it runs.  The host check (`exactdiv_dump --shared`)
// holds the transcription; the device is held by rtProbeExactDivStored, which computes y in one launch and the quotients in a second from the stored y.
RT_EXDIV_FN RtExdiv3 rt_exdiv3_y(float x, float y, float z, float l, float yr) {
    return { rt_exdiv_component(x, l, yr), rt_exdiv_component(y, l, yr), rt_exdiv_component(z, l, yr) };
}
// What is stored beside a divisor: its refined reciprocal, or - the divisor outside the window - a NaN, the marker that fails rt_exdiv3_window_y
RT_EXDIV_FN float rt_exdiv_stored(float l, float y0) {
    return (l >= kExdivLo && l <= kExdivHi) ? rt_exdiv_recip(l, y0) : rt_exdiv_float(0x7fc00000u);
}
// the guard of rt_exdiv3_y: rt_exdiv3_window on the numerators, the divisor's part of it read off the stored word (a NaN is not equal to itself)
RT_EXDIV_FN bool rt_exdiv3_window_y(float x, float y, float z, float yr) {
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y), az = __builtin_fabsf(z);
    const float sum = ax + ay + az, least = __builtin_fminf(ax, __builtin_fminf(ay, az));
    return sum <= kExdivHi && least >= kExdivLo && yr == yr;
}
// the guard of vec3 / float: the sum of the magnitudes bounds each of them from above and is NaN / inf when one of them is; the minimum bounds them from below
// (fminf drops a NaN, the sum does not)
RT_EXDIV_FN bool rt_exdiv3_window(float x, float y, float z, float l) {
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y), az = __builtin_fabsf(z);
    const float sum = ax + ay + az, least = __builtin_fminf(ax, __builtin_fminf(ay, az));
    return sum <= kExdivHi && least >= kExdivLo && l >= kExdivLo && l <= kExdivHi;
}
// the guard of unit(), on what unit() has at hand: the three squares and their sum s2 (l = sqrtf(s2)).  s2 in [2^-60, 2^60] puts l in [2^-30, 2^30] and every
// |component| at most l (1 + 2^-22); the least square >= 2^-80 puts every |component| at or above 2^-40.  A NaN or an infinity anywhere makes s2 one.
RT_EXDIV_FN bool rt_exdiv_unit_window(float xx, float yy, float zz, float s2) {
    return s2 >= 0x1p-60f && s2 <= 0x1p60f && __builtin_fminf(xx, __builtin_fminf(yy, zz)) >= 0x1p-80f;
}
