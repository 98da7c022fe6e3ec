/* The device's powf of displayFrame (cuda-raytracing-optimized_amd/csrc/rt_glibc_powf_pos.h) compiled for the host and held against THIS machine's libm and
 * against librt_host.so's rtLinearToSRGB.  Built by tests/test_display_api.py into its temporary directory; not part of any library. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <string.h>

#define RT_POWF_FN static inline
#include "../cuda-raytracing-optimized_amd/csrc/rt_glibc_powf_pos.h"

uint32_t rtLinearToSRGB(float x);                               /* librt_host.so */

static const float kGamma = 0.416666667f;

float display_twin_powf(float x, float y) { return rt_glibc_powf_pos(x, y); }

/* displayFrame's encoding of one channel (no dither) with the twin's powf */
uint32_t display_twin_code(float y) {
    float s = y > 0.0f ? y : 0.0f, t;
    s = 1.055f * rt_glibc_powf_pos(s, kGamma) - 0.055f;
    s = s > 0.0f ? s : 0.0f;
    t = s * 255.9f;
    return t >= 255.0f ? 255u : (uint32_t)t;
}

typedef struct { uint64_t lo, hi, stride; int codes; long bad, bad_codes; uint32_t first_bad; } job;

static void* worker(void* arg) {
    job* j = (job*)arg;
    for (uint64_t u = j->lo; u < j->hi; u += j->stride) {
        const uint32_t w = (uint32_t)u;
        float x, t, l;
        uint32_t tb, lb;
        memcpy(&x, &w, 4);
        t = rt_glibc_powf_pos(x, kGamma);
        l = powf(x, kGamma);
        memcpy(&tb, &t, 4);
        memcpy(&lb, &l, 4);
        if (tb != lb && !(t != t && l != l)) {                   /* NaN against NaN: any payload */
            if (!j->bad) j->first_bad = w;
            j->bad++;
        }
        if (j->codes && display_twin_code(x) != rtLinearToSRGB(x)) {
            if (!j->bad && !j->bad_codes) j->first_bad = w;
            j->bad_codes++;
        }
    }
    return 0;
}

/* Over the bit patterns lo, lo + stride, .. below hi (all of them >= 0 as floats, or NaN): the number whose twin result differs from libm's
 * powf(x, 0.416666667f) in any bit; with codes != 0 also, in *bad_codes, the number whose 8-bit code differs from rtLinearToSRGB's (the caller keeps that
 * range to finite x below 2^40, where the C conversion is defined).  *first_bad receives one offending bit pattern. */
long display_twin_mismatches(uint64_t lo, uint64_t hi, uint64_t stride, int threads, int codes, uint32_t* first_bad, long* bad_codes) {
    pthread_t th[64];
    job jb[64];
    long bad = 0;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    const uint64_t steps = (hi - lo + stride - 1) / stride, per = (steps + threads - 1) / threads;
    for (int k = 0; k < threads; k++) {
        jb[k].lo = lo + (uint64_t)k * per * stride;
        jb[k].hi = jb[k].lo + per * stride < hi ? jb[k].lo + per * stride : hi;
        jb[k].stride = stride; jb[k].codes = codes; jb[k].bad = 0; jb[k].bad_codes = 0; jb[k].first_bad = 0;
        pthread_create(&th[k], 0, worker, &jb[k]);
    }
    *bad_codes = 0;
    for (int k = 0; k < threads; k++) {
        pthread_join(th[k], 0);
        if ((jb[k].bad || jb[k].bad_codes) && !bad && !*bad_codes) *first_bad = jb[k].first_bad;
        bad += jb[k].bad;
        *bad_codes += jb[k].bad_codes;
    }
    return bad;
}
