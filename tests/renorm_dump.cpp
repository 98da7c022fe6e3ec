// renorm_dump.cpp — csrc/rt_renorm.h on the host, against the plain float operators (tests/test_renorm.py, tests/test_gpu_renorm.py).
// Plain C++, compiled with -ffp-contract=off; no kernel and no HIP call.
//
//   --classes                    k = -9 .. 6: bits(s2), bits(sqrtf(s2)), class (5 when s2 is not handled), then for a handled s2 t, bits(l2), bits(r)
//   --runs                       per class, the runs of d = bits(x / l2) - bits(x) over the 2^23 mantissas of [1, 2): "class m_first d ..."
//   --components                 per class: every mantissa of three binades around 1 and of the two lowest normal binades, every denormal, +-0 and 300
//                                patterns on each side of every threshold in every binade, both signs: rt_renorm_component against x / l2
//   --vectors N SEED             N bounce directions unit(n + p) and a list of inputs that are not unit: rt_renorm_unit against a / sqrtf(s2)
//   --sample SEED PER_CLASS N    hex triples: bounce directions by rejection until every class has PER_CLASS, filled up to N, then the edge inputs
//   (no argument)                hex triples on stdin -> "ox oy oz px py pz exact class" per line: rt_renorm_unit, the plain operators, the path taken
//   --exhaustive                 per class all 2^32 patterns (minutes): mismatches of rt_renorm_component among the finite non-zero patterns, and among the rest
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_renorm.h"

static uint32_t fb(float f) { return rt_renorm_bits(f); }
static float bf(uint32_t u) { return rt_renorm_float(u); }

// x / l2 with both operands opaque to the optimiser: the division instruction, never a folded constant or a reciprocal
static float plain_div(float x, float l2) { volatile float a = x, b = l2; return a / b; }

static bool same(float a, float b) { return fb(a) == fb(b) || (std::isnan(a) && std::isnan(b)); }

// the classes: t of rt_renorm.h in the order of the divisors
static const int kT[5] = { -3, -2, -1, 0, 2 };
constexpr uint32_t kRenormClasses = 5;
static uint32_t class_of(float s2) {
    if (!rt_renorm_handled(s2)) return kRenormClasses;
    for (uint32_t c = 0; c < kRenormClasses; c++) if (kT[c] == rt_renorm_t(s2)) return c;
    return kRenormClasses + 1;      // (a t outside the table: the tests would see it)
}

// ---- the path's random numbers (rnd.h) and a bounce direction as shade builds it -----------------------------------------------------------------
static float rnd_pm1(uint32_t& s) { s ^= s << 13; s ^= s >> 17; s ^= s << 15; return 2.0f * ((float)(s & 0xFFFFFF) / 16777216.0f) - 1.0f; }
struct V { float x, y, z; };
static V in_sphere(uint32_t& s) { V p; do { p.x = rnd_pm1(s); p.y = rnd_pm1(s); p.z = rnd_pm1(s); } while (p.x * p.x + p.y * p.y + p.z * p.z >= 1.0f); return p; }
static V unit_plain(V a) { const RtRenorm3 r = rt_renorm_plain(a.x, a.y, a.z); return { r.x, r.y, r.z }; }
static V bounce(uint32_t& s) {
    const V n = unit_plain(in_sphere(s));            // a hit normal
    const V p = in_sphere(s);
    return unit_plain({ n.x + p.x, n.y + p.y, n.z + p.z });     // material.h:27-31, then ray.h:9
}

static std::vector<V> edge_inputs() {
    std::vector<V> v;
    const V u = { 0.6f, -0.64f, 0.48f };
    for (float len : { 0.5f, 2.0f, 1e-20f, 1e20f, 0.99999f, 1.00001f }) v.push_back({ u.x * len, u.y * len, u.z * len });
    v.push_back({ 0.0f, 0.0f, 0.0f });
    v.push_back({ INFINITY, 0.5f, 0.5f });
    v.push_back({ 0.5f, -INFINITY, 0.5f });
    v.push_back({ NAN, 0.5f, 0.5f });
    v.push_back({ 0.5f, 0.5f, NAN });
    for (float one : { 1.0f, -1.0f })
        for (float zero : { 0.0f, -0.0f }) { v.push_back({ one, zero, -zero }); v.push_back({ zero, one, zero }); v.push_back({ -zero, zero, one }); }
    v.push_back({ 0.6f, 0.8f, -0.0f });
    v.push_back({ 0.6f, 0.0f, -0.8f });
    // unit vectors with a tiny component: denormal, the lowest normal binades (their squares are zero: the plain path)
    for (uint32_t tiny : { 1u, 0x00400001u, 0x007fffffu, 0x00800000u, 0x00ffffffu, 0x01000000u, 0x01000001u, 0x81000000u, 0x80000001u })
        for (float big : { 1.0f, bf(0x3f7fffffu), bf(0x3f800001u), bf(0x3f7ffffeu), bf(0x3f7ffffdu) }) {
            v.push_back({ bf(tiny), big, bf(tiny) }); v.push_back({ big, bf(tiny), 0.25f * big * 0x1p-60f }); v.push_back({ bf(tiny), bf(tiny ^ 0x80000000u), -big });
        }
    // every class through components at the thresholds: x on a threshold, y chosen so that s2 walks through the handled values
    for (uint32_t m : { 0u, 1u, 2u, 0x3ffffeu, 0x3fffffu, 0x400000u, 0x400001u, 0x400002u, 0x555552u, 0x555553u, 0x555554u, 0x7ffffeu, 0x7fffffu })
        for (int e = 120; e <= 126; e++) {
            const float x = bf(((uint32_t)e << 23) | m);
            const float y0 = std::sqrt(1.0f - x * x);
            for (int d = -12; d <= 12; d++) { v.push_back({ x, bf(fb(y0) + (uint32_t)d), 0x1p-40f }); v.push_back({ -0x1p-30f, -bf(fb(y0) + (uint32_t)d), x }); }
        }
    return v;
}

static void print_hex(V a) { printf("%08x %08x %08x\n", fb(a.x), fb(a.y), fb(a.z)); }

static int classes() {
    for (int k = -9; k <= 6; k++) {
        const float s2 = bf(kRenormOne + (uint32_t)k);
        volatile float s = s2;
        const float root = std::sqrt(s);
        const uint32_t cls = class_of(s2);
        printf("%d %08x %08x %u", k, fb(s2), fb(root), cls);
        if (cls < kRenormClasses) printf(" %d %08x %08x", rt_renorm_t(s2), fb(rt_renorm_l2(rt_renorm_t(s2))), fb(rt_renorm_r(rt_renorm_t(s2))));
        printf("\n");
    }
    return 0;
}

static int runs() {
    for (uint32_t cls = 0; cls < kRenormClasses; cls++) {
        const float l2 = rt_renorm_l2(kT[cls]);
        printf("%u", cls);
        int prev = 1 << 30;
        for (uint32_t m = 0; m < (1u << 23); m++) {
            const uint32_t b = kRenormOne | m;
            const int d = (int)(fb(plain_div(bf(b), l2)) - b);
            if (d != prev) { printf(" %06x %d", m, d); prev = d; }
        }
        printf("\n");
    }
    return 0;
}

struct Tally { unsigned long long checked = 0, bad = 0; uint32_t first_bad = 0; };
static void check(Tally& t, float r, float l2, uint32_t bits) {
    for (uint32_t sign : { 0u, 0x80000000u }) {
        const uint32_t b = bits | sign;
        t.checked++;
        if (fb(rt_renorm_component(bf(b), r)) != fb(plain_div(bf(b), l2))) { if (!t.bad++) t.first_bad = b; }
    }
}

static int components() {
    for (uint32_t cls = 0; cls < kRenormClasses; cls++) {
        const float l2 = rt_renorm_l2(kT[cls]), r = rt_renorm_r(kT[cls]);
        Tally t;
        for (uint32_t e : { 126u, 127u, 128u, 1u, 2u, 0u })                                    // (0: the denormals; +0 and -0 are counted apart, below)
            for (uint32_t m = e ? 0u : 1u; m < (1u << 23); m++) check(t, r, l2, (e << 23) | m);
        for (uint32_t e = 0; e <= 254; e++)
            for (uint32_t thr : { 0u, 0x3fffffu, 0x400001u, 0x555553u, 0x7fffffu })
                for (int d = -300; d <= 300; d++) { const uint32_t b = (e << 23) | ((thr + (uint32_t)d) & 0x7fffffu); if (b) check(t, r, l2, b); }
        // the zeros: the quotient keeps the sign; the multiply-add does unless r < 0, where -0 becomes +0 (why a zero component takes the plain path)
        const bool quotient_keeps = fb(plain_div(0.0f, l2)) == 0u && fb(plain_div(-0.0f, l2)) == 0x80000000u;
        const bool fma_keeps = fb(rt_renorm_component(0.0f, r)) == 0u && fb(rt_renorm_component(-0.0f, r)) == 0x80000000u;
        printf("%u %08x r %08x checked %llu bad %llu first %08x zero_quotient %d zero_fma %d\n", cls, fb(l2), fb(r), t.checked, t.bad, t.first_bad, (int)quotient_keeps, (int)fma_keeps);
    }
    return 0;
}

static int vectors(long n, uint32_t seed) {
    unsigned long long bad = 0, plain_unit = 0, hist[kRenormClasses + 1] = {};
    uint32_t s = seed | 1u;
    V first_bad = { 0, 0, 0 };
    auto one = [&](V a, bool is_unit) {
        const RtRenorm3 got = rt_renorm_unit(a.x, a.y, a.z), want = rt_renorm_plain(a.x, a.y, a.z);
        RtRenorm3 tmp;
        const bool exact = rt_renorm_exact(a.x, a.y, a.z, &tmp);
        if (is_unit) {
            const uint32_t cls = class_of(a.x * a.x + a.y * a.y + a.z * a.z);
            hist[cls < kRenormClasses ? cls : kRenormClasses]++;
            plain_unit += !exact;
        }
        if (!(same(got.x, want.x) && same(got.y, want.y) && same(got.z, want.z))) { if (!bad++) first_bad = a; }
    };
    for (long i = 0; i < n; i++) one(bounce(s), true);
    const std::vector<V> edges = edge_inputs();
    for (const V& a : edges) one(a, false);
    printf("unit %ld edges %zu bad %llu plain_unit %llu first_bad %08x %08x %08x hist", n, edges.size(), bad, plain_unit, fb(first_bad.x), fb(first_bad.y), fb(first_bad.z));
    for (unsigned long long h : hist) printf(" %llu", h);
    printf("\n");
    return 0;
}

static int sample(uint32_t seed, long per_class, long n) {
    uint32_t s = seed | 1u;
    long have[kRenormClasses + 1] = {}, total = 0;
    auto short_of = [&] { for (uint32_t c = 0; c < kRenormClasses; c++) if (have[c] < per_class) return true; return false; };
    // first what the rare classes need (and as many vectors outside the classes), by rejection; then whatever comes, up to n
    while (short_of()) {
        const V a = bounce(s);
        const uint32_t c = class_of(a.x * a.x + a.y * a.y + a.z * a.z);
        long& h = have[c < kRenormClasses ? c : kRenormClasses];
        if (h >= per_class) continue;
        h++; print_hex(a); total++;
    }
    for (; total < n; total++) print_hex(bounce(s));
    for (const V& a : edge_inputs()) print_hex(a);
    return 0;
}

static int filter() {
    uint32_t x, y, z;
    while (scanf("%x %x %x", &x, &y, &z) == 3) {
        const RtRenorm3 got = rt_renorm_unit(bf(x), bf(y), bf(z)), want = rt_renorm_plain(bf(x), bf(y), bf(z));
        RtRenorm3 tmp;
        const bool exact = rt_renorm_exact(bf(x), bf(y), bf(z), &tmp);
        const uint32_t cls = class_of(bf(x) * bf(x) + bf(y) * bf(y) + bf(z) * bf(z));
        printf("%08x %08x %08x %08x %08x %08x %d %u\n", fb(got.x), fb(got.y), fb(got.z), fb(want.x), fb(want.y), fb(want.z), (int)exact, cls < kRenormClasses ? cls : kRenormClasses);
    }
    return 0;
}

static int exhaustive() {
    for (uint32_t cls = 0; cls < kRenormClasses; cls++) {
        const float l2 = rt_renorm_l2(kT[cls]), r = rt_renorm_r(kT[cls]);
        unsigned long long bad_in = 0, bad_out = 0, in = 0;
        uint32_t b = 0;
        do {
            const float want = plain_div(bf(b), l2), got = rt_renorm_component(bf(b), r);
            const bool differs = !same(got, want);
            // (apart: the two zeros, which the exact path hands to the plain operators, and the infinities and NaNs, whose s2 is not a handled one)
            if ((b & 0x7fffffffu) != 0u && (b & 0x7f800000u) != 0x7f800000u) { in++; bad_in += differs; } else bad_out += differs;
        } while (++b != 0);
        printf("%u %08x r %08x finite_nonzero %llu bad %llu bad_among_zeros_inf_nan %llu\n", cls, fb(l2), fb(r), in, bad_in, bad_out);
        fflush(stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "--classes")) return classes();
    if (argc >= 2 && !strcmp(argv[1], "--runs")) return runs();
    if (argc >= 2 && !strcmp(argv[1], "--components")) return components();
    if (argc >= 4 && !strcmp(argv[1], "--vectors")) return vectors(atol(argv[2]), (uint32_t)strtoul(argv[3], nullptr, 0));
    if (argc >= 5 && !strcmp(argv[1], "--sample")) return sample((uint32_t)strtoul(argv[2], nullptr, 0), atol(argv[3]), atol(argv[4]));
    if (argc >= 2 && !strcmp(argv[1], "--exhaustive")) return exhaustive();
    if (argc == 1) return filter();
    fprintf(stderr, "usage: see the head of tests/renorm_dump.cpp\n");
    return 2;
}
