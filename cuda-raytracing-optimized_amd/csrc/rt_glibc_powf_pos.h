/* rt_glibc_powf_pos.h — powf(x, y) for x >= 0 (or NaN) and a finite, positive y, as glibc's libm computes it: the text of rt_glibc_powf.h with the exponent a
 * variable.  displayFrame (include/rt_api.h) encodes sRGB with powf(s, 0.416666667f), exactly as rtLinearToSRGB (host/rt_harness.cpp) does with libm's; this
 * header lets the device compute those bits.
 *
 * The algorithm, the fused operations and the two tables are the ones rt_glibc_powf.h documents (glibc 2.35, sysdeps/ieee754/flt-32/e_powf.c, the __powf_fma
 * build); that header is included for its tables and stays as it is.  What differs from its body:
 *   - `(double)y *` where `5.0 *` stands: y log2(x) is one rounded fp64 product of the exact conversion of y;
 *   - zeroinfnan(x) returns x * x: +0 for a zero of either sign, +inf for +inf, NaN for a NaN (e_powf.c with y > 0);
 *   - no sign handling: x < 0 is outside the contract (e_powf.c would return NaN for a non-integer y), so SIGN_BIAS is gone.
 * y itself is never special here (finite, > 0), so e_powf.c's zeroinfnan(y) block is not restated.
 *
 * Pinned by tests/test_display_api.py: this text compiled for the host (tests/display_powf_twin.c) equals libm's powf(x, 0.416666667f) in every bit on ALL
 * floats of [0, 1.0000002], on every 61st bit pattern of [0, +inf] and for NaN.
 *
 * One text for the device and a host compile: the includer defines RT_POWF_FN (and may define RT_POWF_TABLE) as for rt_glibc_powf.h.
 */
#ifndef RT_GLIBC_POWF_POS_H
#define RT_GLIBC_POWF_POS_H

#include "rt_glibc_powf.h"

/* log2_tab / exp2_tab: rt_powf_log2_tab / rt_powf_exp2_tab, or a copy of them */
RT_POWF_FN float rt_glibc_powf_pos_tab(float x, float y, const double* log2_tab, const uint64_t* exp2_tab) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double A0 = 0x1.27616c9496e0bp-2, A1 = -0x1.71969a075c67ap-2, A2 = 0x1.ec70a6ca7baddp-2, A3 = -0x1.7154748bef6c8p-1, A4 = 0x1.71547652ab82bp0;
    const double C0 = 0x1.c6af84b912394p-5, C1 = 0x1.ebfce50fac4f3p-3, C2 = 0x1.62e42ff0c52d6p-1, SHIFT = 0x1.8p+47;
    union { float f; uint32_t u; } fb;
    union { double d; uint64_t u; } db;
    uint32_t ix;
    fb.f = x;
    ix = fb.u;
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {            /* x < 0x1p-126, or inf, or NaN */
        if (2u * ix - 1u >= 2u * 0x7f800000u - 1u) return x * x;    /* zeroinfnan(ix) */
        fb.f = fb.f * 0x1p23f;                                      /* subnormal: normalise so that the exponent becomes negative */
        ix = (fb.u & 0x7fffffffu) - (23u << 23);
    }
    {
        const uint32_t tmp = ix - 0x3f330000u;
        const int i = (int)((tmp >> 19) & 15u);
        const uint32_t top = tmp & 0xff800000u;
        const int k = (int32_t)top >> 23;
        double z, r, r2, r4, p, q, v, ylogx, kd;
        uint64_t ki, t;
        fb.u = ix - top;
        z = (double)fb.f;
        r = __builtin_fma(z, log2_tab[2 * i], -1.0);
        q = log2_tab[2 * i + 1] + (double)k;
        r2 = r * r;
        v = __builtin_fma(r, A0, A1);
        p = __builtin_fma(r, A2, A3);
        q = __builtin_fma(r, A4, q);
        r4 = r2 * r2;
        q = __builtin_fma(r2, p, q);
        ylogx = (double)y * __builtin_fma(v, r4, q);                /* y * log2(x): one rounded product */
        db.d = ylogx;
        if (((db.u >> 47) & 0xffffu) >= 0x80bfu) {                  /* |y log2 x| >= 126 */
            if (ylogx > 0x1.fffffffd1d571p+6) return __builtin_inff();      /* __math_oflowf */
            if (ylogx <= -150.0) return 0.0f;                               /* __math_uflowf */
            if (ylogx < -149.0) return 0x1p-149f;                           /* __math_may_uflowf */
        }
        kd = ylogx + SHIFT;
        db.d = kd;
        ki = db.u;
        kd -= SHIFT;
        r = ylogx - kd;
        t = exp2_tab[ki & 31u] + (ki << 47);
        z = __builtin_fma(r, C0, C1);
        r2 = r * r;
        v = __builtin_fma(r, C2, 1.0);
        v = __builtin_fma(z, r2, v);
        db.u = t;
        return (float)(v * db.d);
    }
}

RT_POWF_FN float rt_glibc_powf_pos(float x, float y) { return rt_glibc_powf_pos_tab(x, y, rt_powf_log2_tab, rt_powf_exp2_tab); }

#endif
