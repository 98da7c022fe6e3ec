// exactdiv_stored_dump — csrc/rt_exactdiv.h's stored-reciprocal form (rt_exdiv_stored, rt_exdiv3_y, rt_exdiv3_window_y: the hit normal of the folded sphere
// kinds) against the plain float division, bit for bit, on the host.  Plain C++ (compile with -ffp-contract=off).  The companion of exactdiv_dump.cpp, whose
// `--shared` cases it enumerates again - the same divisors, seeds and numerators - through the functions that take the reciprocal as a stored word.
// tests/test_exactdiv_stored.py drives it.
//
//   --shared D STRIDE    per divisor (the benchmark's radii 0.2, 1, 1000 and 0.5, then D mantissas spread over [1, 2) times 2^e, e cycling through the window)
//                        and per seed (RN(1 / l): held; its two neighbours: counted): the word is stored once, then the mantissas of x (every STRIDE-th, the
//                        first and last 600 always) of one binade go through rt_exdiv3_y in both signs, in each of the three components
//   --marker             divisors at and beyond both ends of the window, zero, negative, infinite, NaN: the stored word is the marker exactly outside the
//                        window, and the guard lets the form through exactly where rt_exdiv3_window does
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_exactdiv.h"

static uint32_t bits(float f) { return rt_exdiv_bits(f); }
static float flt(uint32_t u) { return rt_exdiv_float(u); }
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }      // (any NaN equals any NaN: the payload is never looked at)
static volatile float g_one = 1.0f;
static float quot(float x, float d) { return x / (d * g_one); }                               // a division the compiler cannot turn into anything else

// the seeds of exactdiv_dump.cpp: RN(1 / l), its neighbour on the side of the true reciprocal, its neighbour on the far side
static void seeds_of(float l, float* y0) {
    const float y = 1.0f / l;
    const float res = fmaf(-l, y, 1.0f);
    const bool up = (res > 0.0f) == (y > 0.0f);
    y0[0] = y; y0[1] = flt(bits(y) + (up ? 1u : (uint32_t)-1)); y0[2] = flt(bits(y) + (up ? (uint32_t)-1 : 1u));
}
struct Count { unsigned long long checked = 0, bad = 0, near_bad = 0, far_bad = 0, guard_bad = 0; };
static void check_divisor(float l, int exp_x, uint32_t stride, Count& c) {
    float y0[3];
    seeds_of(l, y0);
    for (int s = 0; s < 3; s++) {
        const float stored = rt_exdiv_stored(l, y0[s]);                      // once per divisor, as the scene is staged
        if (!same(stored, rt_exdiv_recip(l, y0[s]))) c.guard_bad++;           // (every divisor here is inside the window: the word is the reciprocal)
        const float other = 3.0f;
        auto one = [&](uint32_t m) {
            for (uint32_t sg = 0; sg < 2; sg++) {
                const float x = flt((sg << 31) | ((uint32_t)exp_x << 23) | m);
                if (s == 0) c.checked++;
                const RtExdiv3 a = rt_exdiv3_y(x, other, -x, l, stored);
                const bool ok = same(a.x, quot(x, l)) && same(a.y, quot(other, l)) && same(a.z, quot(-x, l));
                if (!ok) { if (s == 0) c.bad++; else if (s == 1) c.near_bad++; else c.far_bad++; }
                if (rt_exdiv3_window_y(x, other, -x, stored) != rt_exdiv3_window(x, other, -x, l)) c.guard_bad++;
            }
        };
        if (stride == 1) { for (uint32_t m = 0; m < (1u << 23); m++) one(m); continue; }
        for (uint32_t m = 0; m < 600; m++) { one(m); one((1u << 23) - 1 - m); }
        for (uint32_t m = 600; m < (1u << 23) - 600; m += stride) one(m);
    }
}
// divisor d of exactdiv_dump.cpp's --shared: a mantissa spread over the binade, its exponent and the exponent of x cycling through the window
static float divisor_of(long d, int* exp_x) {
    uint32_t m;
    if (d < 64) m = (uint32_t)d; else if (d < 128) m = (1u << 23) - 1 - (uint32_t)(d - 64);
    else m = (uint32_t)(((unsigned long long)(d - 128) * 0x9E3779B1ull) & 0x7FFFFFu);
    const int el = 127 - 40 + (int)(d % 81), ex = 127 - 40 + (int)((d * 7 + 3) % 80);
    *exp_x = ex;
    return flt(((uint32_t)el << 23) | (el == 127 + 40 ? 0u : m));
}
static void mode_shared(long D, uint32_t stride) {
    Count total;
    const float radii[] = { 0.2f, 1.0f, 1000.0f, 0.5f };                     // (exactdiv_dump's fifth, -0.5, is outside this form: the marker, below)
    for (float l : radii) {
        Count c;
        check_divisor(l, 126, 1, c);
        printf("l %08x checked %llu bad %llu near_bad %llu far_bad %llu guard_bad %llu\n", bits(l), c.checked, c.bad, c.near_bad, c.far_bad, c.guard_bad);
        total.checked += c.checked; total.bad += c.bad; total.near_bad += c.near_bad; total.far_bad += c.far_bad; total.guard_bad += c.guard_bad;
    }
    for (long d = 0; d < D; d++) { int ex; const float l = divisor_of(d, &ex); check_divisor(l, ex, stride, total); }
    printf("divisors %ld stride %u checked %llu bad %llu near_bad %llu far_bad %llu guard_bad %llu\n", D + 4, stride, total.checked, total.bad, total.near_bad,
           total.far_bad, total.guard_bad);
}

static void mode_marker() {
    const float lo = kExdivLo, hi = kExdivHi;
    const float ls[] = { lo, flt(bits(lo) - 1), flt(bits(lo) + 1), hi, flt(bits(hi) - 1), flt(bits(hi) + 1), 0.0f, -0.0f, -0.5f, INFINITY, -INFINITY, NAN, 1e-42f, 0x1p45f, 0x1p-45f, 0.2f };
    const float xs[][3] = { { 1.0f, -2.0f, 3.0f }, { 0.0f, 1.0f, 1.0f }, { 1.0f, lo, 1.0f }, { 1.0f, flt(bits(lo) - 1), 1.0f }, { hi, 1.0f, 1.0f }, { NAN, 1.0f, 1.0f }, { 1.0f, 1.0f, -INFINITY } };
    for (float l : ls) {
        const float stored = rt_exdiv_stored(l, 1.0f / l);
        const bool in = l >= lo && l <= hi;
        int guard_bad = 0, bad = 0;
        for (const auto& x : xs) {
            const bool g = rt_exdiv3_window_y(x[0], x[1], x[2], stored);
            guard_bad += g != rt_exdiv3_window(x[0], x[1], x[2], l);
            if (g) {
                const RtExdiv3 q = rt_exdiv3_y(x[0], x[1], x[2], l, stored);
                bad += !same(q.x, quot(x[0], l)) + !same(q.y, quot(x[1], l)) + !same(q.z, quot(x[2], l));
            }
        }
        printf("l %08x in %d marker %d guard_bad %d bad %d\n", bits(l), in ? 1 : 0, stored != stored ? 1 : 0, guard_bad, bad);
    }
}

int main(int argc, char** argv) {
    const char* m = argc > 1 ? argv[1] : "";
    if (!strcmp(m, "--shared") && argc > 3) mode_shared(atol(argv[2]), (uint32_t)strtoul(argv[3], nullptr, 10));
    else if (!strcmp(m, "--marker")) mode_marker();
    else { fprintf(stderr, "usage: exactdiv_stored_dump --shared D STRIDE | --marker\n"); return 2; }
    return 0;
}
