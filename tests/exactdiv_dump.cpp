// exactdiv_dump — csrc/rt_exactdiv.h against the plain float division it replaces, bit for bit, on the host.  Plain C++ (compile with -ffp-contract=off): the
// header's functions are the ones the PARITY kernels run.  tests/test_exactdiv.py drives the quick modes; the exhaustive ones are run by hand.
//
//   --words                  k = -6 .. 4: bits(a), handled, the computed r
//   --quot-a                 form B, per handled a: two binades around 1, the lowest and the highest binade, the denormals (both signs) and the special values
//   --exhaustive-a           form B, per handled a: all 2^32 patterns of x
//   --ahist N SEED           k of a = dot(dn, dn) over N twice-normalised bounce directions unit(n + random_in_unit_sphere)
//   --shared D STRIDE        form C, per divisor (the benchmark's radii, then D mantissas spread over [1, 2) times 2^e, e cycling through the window) and per
//                            seed (RN(1 / l): held; its two neighbours: counted): the mantissas of x (every STRIDE-th, the first and last 600 always) in one binade
//   --exhaustive-shared D    the same with every mantissa, over D divisors, on all hardware threads
//   --window                 the guards from both sides of each edge, and the quotient on the inside
//   --vectors N SEED         form C on N un-normalised bounce vectors against a / sqrtf(s2)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "rt_exactdiv.h"

static uint32_t bits(float f) { return rt_exdiv_bits(f); }
static float flt(uint32_t u) { return rt_exdiv_float(u); }
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }      // (any NaN equals any NaN: the payload is never looked at)
static volatile float g_one = 1.0f;
static float quot(float x, float d) { return x / (d * g_one); }                               // a division the compiler cannot turn into anything else

static uint32_t g_rng;
static float rnd() { uint32_t x = g_rng; x ^= x << 13; x ^= x >> 17; x ^= x << 15; g_rng = x; return (float)(x & 0xFFFFFF) / 16777216.0f; }
static void in_unit_sphere(float* p) { do { for (int k = 0; k < 3; k++) p[k] = 2.0f * rnd() - 1.0f; } while (p[0] * p[0] + p[1] * p[1] + p[2] * p[2] >= 1.0f); }
static void unit3(const float* v, float* o) { const float l = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); for (int k = 0; k < 3; k++) o[k] = v[k] / l; }

struct BCount { unsigned long long checked = 0, bad = 0, zero_sign = 0, inf_nan = 0; };
// one x of form B: classes of mismatch - the sign of a zero, an infinite x, anything else
static void check_b(float x, float a, float r, BCount& c) {
    const float q = quot(x, a), f = rt_exdiv_a_quot(x, r);
    c.checked++;
    if (same(q, f)) return;
    if (x == 0.0f) c.zero_sign++;
    else if (isinf(x)) c.inf_nan++;
    else c.bad++;
}

static void mode_words() {
    for (int k = -6; k <= 4; k++) {
        const float a = flt(kExdivOne + (uint32_t)k);
        printf("%d %08x %d %08x\n", k, bits(a), rt_exdiv_a_handled(a) ? 1 : 0, bits(rt_exdiv_a_r(a)));
    }
}

static void mode_quot_a(bool exhaustive) {
    for (int k = kExdivKMin; k <= kExdivKMax; k++) {
        const float a = flt(kExdivOne + (uint32_t)k), r = rt_exdiv_a_r(a);
        BCount total;
        if (exhaustive) {
            const unsigned nt = std::max(1u, std::thread::hardware_concurrency());
            std::vector<BCount> part(nt);
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t] {
                const unsigned long long lo = (1ull << 32) * t / nt, hi = (1ull << 32) * (t + 1) / nt;
                for (unsigned long long u = lo; u < hi; u++) check_b(flt((uint32_t)u), a, r, part[t]);
            });
            for (auto& t : th) t.join();
            for (auto& p : part) { total.checked += p.checked; total.bad += p.bad; total.zero_sign += p.zero_sign; total.inf_nan += p.inf_nan; }
        } else {
            const uint32_t exps[] = { 0, 126, 127 };                        // the denormals and the two binades around 1: every mantissa
            for (uint32_t e : exps) for (uint32_t s = 0; s < 2; s++) for (uint32_t m = 0; m < (1u << 23); m++) check_b(flt((s << 31) | (e << 23) | m), a, r, total);
            const uint32_t ends[] = { 1, 254 };                             // the lowest and the highest binade: 4096 mantissas at either end
            for (uint32_t e : ends) for (uint32_t s = 0; s < 2; s++) for (uint32_t m = 0; m < 4096; m++) {
                check_b(flt((s << 31) | (e << 23) | m), a, r, total);
                check_b(flt((s << 31) | (e << 23) | ((1u << 23) - 1 - m)), a, r, total);
            }
            const uint32_t special[] = { 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x7f7fffffu, 0xff7fffffu };
            for (uint32_t u : special) check_b(flt(u), a, r, total);
        }
        printf("%d a %08x r %08x checked %llu bad %llu zero_sign %llu inf_nan %llu\n", k, bits(a), bits(r), total.checked, total.bad, total.zero_sign, total.inf_nan);
    }
}

static void mode_ahist(long n, uint32_t seed) {
    g_rng = seed | 1u;
    long hist[32] = { 0 }, other = 0;
    for (long i = 0; i < n; i++) {
        float nrm[3], rs[3], v[3], u[3], dn[3];
        in_unit_sphere(rs); unit3(rs, nrm);                              // a hit normal
        in_unit_sphere(rs);
        for (int k = 0; k < 3; k++) v[k] = nrm[k] + rs[k];
        unit3(v, u); unit3(u, dn);                                       // shade stores unit(v), hit() normalises it again
        const float a = dn[0] * dn[0] + dn[1] * dn[1] + dn[2] * dn[2];
        const int k = (int)(bits(a) - kExdivOne);
        if (k >= -16 && k < 16) hist[k + 16]++; else other++;
    }
    for (int k = -16; k < 16; k++) if (hist[k + 16]) printf("%d %ld\n", k, hist[k + 16]);
    printf("other %ld\n", other);
}

// The seeds of form C.  The host has no v_rcp_f32: the twin is held to the quotient for the seed RN(1 / l) (the condition), and the two neighbours are
// counted apart, for the record - the one on the side of the true reciprocal (within 1 ulp of it, v_rcp_f32's stated bound) and the one on the far side
// (up to 1.5 ulp).  On the device the sequence is the compiler's own on whatever the instruction returns: the probe holds that (rtProbeExactDiv).
static int seeds_of(float l, float* y0) {
    const float y = 1.0f / l;
    const float res = fmaf(-l, y, 1.0f);                                 // its sign says on which side of y the true reciprocal lies
    const bool up = (res > 0.0f) == (y > 0.0f);                          // |1 / l| > |y|
    y0[0] = y; y0[1] = flt(bits(y) + (up ? 1u : (uint32_t)-1)); y0[2] = flt(bits(y) + (up ? (uint32_t)-1 : 1u));
    return 1;
}
struct CCount { unsigned long long checked = 0, bad = 0, near_bad = 0, far_bad = 0; };
static void check_c_divisor(float l, int exp_x, uint32_t stride, CCount& c) {
    float y0[3];
    seeds_of(l, y0);
    for (int s = 0; s < 3; s++) {
        const float y = rt_exdiv_recip(l, y0[s]);
        auto one = [&](uint32_t m) {
            for (uint32_t sg = 0; sg < 2; sg++) {
                const float x = flt((sg << 31) | ((uint32_t)exp_x << 23) | m);
                if (s == 0) c.checked++;
                if (!same(quot(x, l), rt_exdiv_component(x, l, y))) { if (s == 0) c.bad++; else if (s == 1) c.near_bad++; else c.far_bad++; }
            }
        };
        if (stride == 1) { for (uint32_t m = 0; m < (1u << 23); m++) one(m); continue; }
        for (uint32_t m = 0; m < 600; m++) { one(m); one((1u << 23) - 1 - m); }
        for (uint32_t m = 600; m < (1u << 23) - 600; m += stride) one(m);
    }
}
// divisor d of D: a mantissa spread over the binade (the 64 smallest and 64 largest first), its exponent and the exponent of x cycling through the window
static float divisor_of(long d, long D, int* exp_x) {
    uint32_t m;
    if (d < 64) m = (uint32_t)d; else if (d < 128) m = (1u << 23) - 1 - (uint32_t)(d - 64);
    else m = (uint32_t)(((unsigned long long)(d - 128) * 0x9E3779B1ull) & 0x7FFFFFu);
    const int el = 127 - 40 + (int)(d % 81), ex = 127 - 40 + (int)((d * 7 + 3) % 80);      // |l| in [2^-40, 2^40], |x| in [2^-40, 2^40)
    *exp_x = ex;
    (void)D;
    return flt(((uint32_t)el << 23) | (el == 127 + 40 ? 0u : m));
}
static void mode_shared(long D, uint32_t stride, bool threads) {
    CCount total;
    const float radii[] = { 0.2f, 1.0f, 1000.0f, 0.5f, -0.5f };
    for (float l : radii) {
        CCount c;
        check_c_divisor(l, 126, 1, c);
        printf("l %08x checked %llu bad %llu near_bad %llu far_bad %llu\n", bits(l), c.checked, c.bad, c.near_bad, c.far_bad);
        total.checked += c.checked; total.bad += c.bad; total.near_bad += c.near_bad; total.far_bad += c.far_bad;
    }
    const unsigned nt = threads ? std::max(1u, std::thread::hardware_concurrency()) : 1u;
    std::vector<CCount> part(nt);
    std::atomic<long> next(0);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t] {
        for (long d = next++; d < D; d = next++) { int ex; const float l = divisor_of(d, D, &ex); check_c_divisor(l, ex, stride, part[t]); }
    });
    for (auto& t : th) t.join();
    for (auto& p : part) { total.checked += p.checked; total.bad += p.bad; total.near_bad += p.near_bad; total.far_bad += p.far_bad; }
    printf("divisors %ld stride %u checked %llu bad %llu near_bad %llu far_bad %llu\n", D + 5, stride, total.checked, total.bad, total.near_bad, total.far_bad);
}

static void mode_window() {
    // vec3 / float: (x, y, z, l) -> inside?; on the inside the quotient is held as well
    const float lo = kExdivLo, hi = kExdivHi, below = flt(bits(lo) - 1), above = flt(bits(hi) + 1), third = flt(bits(hi / 4.0f));
    const float inf = INFINITY, nan = NAN;
    const float rows[][4] = {
        { lo, lo, lo, lo }, { lo, lo, lo, hi }, { third, third, third, lo }, { third, -third, third, hi }, { 1.0f, -2.0f, 3.0f, 0.2f }, { 1.0f, 2.0f, 3.0f, -0.2f },
        { below, 1.0f, 1.0f, 1.0f }, { 1.0f, below, 1.0f, 1.0f }, { 1.0f, 1.0f, -below, 1.0f }, { 1.0f, 1.0f, 1.0f, below }, { 1.0f, 1.0f, 1.0f, above },
        { hi, 1.0f, 1.0f, 1.0f }, { above, lo, lo, 1.0f }, { 0.0f, 1.0f, 1.0f, 1.0f }, { 1.0f, -0.0f, 1.0f, 1.0f }, { 1.0f, 1.0f, 1.0f, 0.0f },
        { nan, 1.0f, 1.0f, 1.0f }, { 1.0f, nan, 1.0f, 1.0f }, { 1.0f, 1.0f, nan, 1.0f }, { 1.0f, 1.0f, 1.0f, nan }, { inf, 1.0f, 1.0f, 1.0f }, { 1.0f, 1.0f, -inf, 1.0f },
        { 1.0f, 1.0f, 1.0f, inf }, { 1e-30f, 1.0f, 1.0f, 1.0f }, { 1.0f, 1.0f, 1.0f, 1e-45f },
    };
    for (const auto& r : rows) {
        const bool in = rt_exdiv3_window(r[0], r[1], r[2], r[3]);
        int bad = 0;
        if (in) {
            float y0[3];
            const int ns = seeds_of(r[3], y0);
            for (int s = 0; s < ns; s++) {
                const RtExdiv3 q = rt_exdiv3(r[0], r[1], r[2], r[3], y0[s]);
                bad += !same(q.x, quot(r[0], r[3])) + !same(q.y, quot(r[1], r[3])) + !same(q.z, quot(r[2], r[3]));
            }
        }
        printf("div3 %08x %08x %08x %08x in %d bad %d\n", bits(r[0]), bits(r[1]), bits(r[2]), bits(r[3]), in ? 1 : 0, bad);
    }
    // unit(): the vector -> inside?
    const float t30 = 0x1p30f, t40 = 0x1p-40f, t30m = 0x1p-30f;
    const float vec[][3] = {
        { 0.3f, -0.4f, 0.5f }, { t30 * 0.5f, t30 * 0.5f, t30 * 0.5f }, { t30, t30, t30 }, { t30m, t30m * 0.25f, t30m * 0.25f }, { t30m * 0.5f, t30m * 0.5f, t30m * 0.5f },
        { 1.0f, t40, 1.0f }, { 1.0f, flt(bits(t40) - 1), 1.0f }, { 1.0f, 0.0f, 1.0f }, { -0.0f, 1.0f, 1.0f }, { nan, 1.0f, 1.0f }, { 1.0f, inf, 1.0f }, { 1.0f, 1.0f, -inf },
        { 1e-25f, 1.0f, 1.0f }, { 0x1p30f, 1.0f, 1.0f }, { 0x1p29f, 1.0f, 1.0f },
    };
    for (const auto& v : vec) {
        const float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2], s2 = xx + yy + zz;
        const bool in = rt_exdiv_unit_window(xx, yy, zz, s2);
        int bad = 0, inside3 = 0;
        if (in) {
            const float l = sqrtf(s2);
            inside3 = rt_exdiv3_window(v[0], v[1], v[2], l) ? 1 : 0;      // the unit guard implies the general one
            float y0[3];
            const int ns = seeds_of(l, y0);
            for (int s = 0; s < ns; s++) {
                const RtExdiv3 q = rt_exdiv3(v[0], v[1], v[2], l, y0[s]);
                bad += !same(q.x, quot(v[0], l)) + !same(q.y, quot(v[1], l)) + !same(q.z, quot(v[2], l));
            }
        }
        printf("unit %08x %08x %08x in %d general %d bad %d\n", bits(v[0]), bits(v[1]), bits(v[2]), in ? 1 : 0, inside3, bad);
    }
}

static void mode_vectors(long n, uint32_t seed) {
    g_rng = seed | 1u;
    long unit_n = 0, plain = 0, bad = 0;
    for (long i = 0; i < n; i++) {
        float nrm[3], rs[3], v[3];
        in_unit_sphere(rs); unit3(rs, nrm);
        in_unit_sphere(rs);
        const float scale = (i & 7) == 7 ? 0.3f : 1.0f;                  // (metal fuzz: a scaled offset)
        for (int k = 0; k < 3; k++) v[k] = nrm[k] + scale * rs[k];
        const float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2], s2 = xx + yy + zz, l = sqrtf(s2);
        unit_n++;
        if (!rt_exdiv_unit_window(xx, yy, zz, s2)) { plain++; continue; }
        float y0[3];
        const int ns = seeds_of(l, y0);
        for (int s = 0; s < ns; s++) {
            const RtExdiv3 q = rt_exdiv3(v[0], v[1], v[2], l, y0[s]);
            if (!same(q.x, quot(v[0], l)) || !same(q.y, quot(v[1], l)) || !same(q.z, quot(v[2], l))) bad++;
        }
    }
    printf("unit %ld plain %ld bad %ld\n", unit_n, plain, bad);
}

int main(int argc, char** argv) {
    const char* m = argc > 1 ? argv[1] : "";
    if (!strcmp(m, "--words")) mode_words();
    else if (!strcmp(m, "--quot-a")) mode_quot_a(false);
    else if (!strcmp(m, "--exhaustive-a")) mode_quot_a(true);
    else if (!strcmp(m, "--ahist") && argc > 3) mode_ahist(atol(argv[2]), (uint32_t)strtoul(argv[3], nullptr, 10));
    else if (!strcmp(m, "--shared") && argc > 3) mode_shared(atol(argv[2]), (uint32_t)strtoul(argv[3], nullptr, 10), false);
    else if (!strcmp(m, "--exhaustive-shared") && argc > 2) mode_shared(atol(argv[2]), 1, true);
    else if (!strcmp(m, "--window")) mode_window();
    else if (!strcmp(m, "--vectors") && argc > 3) mode_vectors(atol(argv[2]), (uint32_t)strtoul(argv[3], nullptr, 10));
    else { fprintf(stderr, "usage: exactdiv_dump --words | --quot-a | --exhaustive-a | --ahist N SEED | --shared D STRIDE | --exhaustive-shared D | --window | --vectors N SEED\n"); return 2; }
    return 0;
}
