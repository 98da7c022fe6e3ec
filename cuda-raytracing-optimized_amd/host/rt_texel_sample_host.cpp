// rtSampleTexelsHost (include/rt_host.h): sampleTexels on the CPU.  The lookup is csrc/rt_texel_sample.h, the text the device kernels compile: this file is
// built with -ffp-contract=off.  The twin walks the hits in order; it has no bake or filter to take a plane from.
#include "../../include/rt_api.h"
#include "../../include/rt_host.h"

#include "../csrc/rt_texel_sample.h"

extern "C" int rtSampleTexelsHost(const rt_triangle* tris, uint32_t numTris, int n, const int32_t* prim, const float* uv, const float* normal, int W, int H,
                                  int mode, const float* planes, int flags, float* out, uint8_t* valid) {
    // what sampleTexels refuses (and a NULL `planes`, with or without a FROM flag): nothing is written
    if (n < 0 || W < 1 || H < 1 || W > RT_TEXEL_MAX_SIZE || H > RT_TEXEL_MAX_SIZE) return -1;
    if (mode != RT_GATHER_IRRADIANCE && mode != RT_GATHER_SH9 && mode != RT_GATHER_VISIBILITY) return -1;
    if ((flags & ~RT_SAMPLE_BILINEAR) != 0 || !planes) return -1;
    if (n == 0) return 0;
    if ((!tris && numTris > 0) || !prim || !uv || !out || (mode == RT_GATHER_SH9 && !normal)) return -1;
    const float zero[3] = { 0.0f, 0.0f, 0.0f };
    int count = 0;
    for (int k = 0; k < n; k++) {
        const bool ok = rt_sample_lookup(tris, numTris, prim[k], uv[2 * (size_t)k], uv[2 * (size_t)k + 1], mode == RT_GATHER_SH9 ? normal + 3 * (size_t)k : zero,
                                         W, H, mode, flags & RT_SAMPLE_BILINEAR, planes, out + 3 * (size_t)k);
        if (valid) valid[k] = ok ? 1 : 0;
        count += ok ? 1 : 0;
    }
    return count;
}
