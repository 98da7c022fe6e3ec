// rtFilterTexelsHost (include/rt_host.h): filterTexels on the CPU, on top of rtRasterTexelsHost.  The footprint and the tap are csrc/rt_texel_filter.h, the
// text the device kernels compile: this file is built with -ffp-contract=off, and x86-64's sqrtf and division are correctly rounded.  The twin walks the
// definition of rt_api.h ("filtering texels") as it is written: every owned texel, the 25 taps dy outer and dx inner, a dropped tap skipped.
#include "../../include/rt_api.h"
#include "../../include/rt_host.h"

#include <cmath>
#include <cstddef>
#include <vector>

#include "../csrc/rt_texel_filter.h"

extern "C" int rtFilterTexelsHost(const rt_triangle* tris, uint32_t numTris, int W, int H, int dilate, int mode, const float* in, float* out, int iterations,
                                  int normal_squarings, float sigma_d, float sigma_z, float sigma_c) {
    // what filterTexels refuses (but a NULL `in`: the twin has no bake to take it from): nothing is written
    if (W < 1 || H < 1 || W > RT_TEXEL_MAX_SIZE || H > RT_TEXEL_MAX_SIZE || dilate < 0 || dilate > RT_TEXEL_MAX_DILATE) return -1;
    if (mode != RT_GATHER_IRRADIANCE && mode != RT_GATHER_SH9 && mode != RT_GATHER_VISIBILITY) return -1;
    if ((!tris && numTris > 0) || !in || !out) return -1;
    if (iterations < 1 || iterations > RT_DENOISE_MAX_ITERATIONS || normal_squarings < 0 || normal_squarings > RT_DENOISE_MAX_SQUARINGS) return -1;
    if (!std::isfinite(sigma_d) || sigma_d <= 0.0f || !std::isfinite(sigma_z) || sigma_z <= 0.0f || !std::isfinite(sigma_c)) return -1;
    const int C = mode == RT_GATHER_IRRADIANCE ? 3 : mode == RT_GATHER_SH9 ? 27 : 1, L = C < 3 ? C : 3;
    const size_t n = (size_t)W * H;
    std::vector<int32_t> prim(n), src(n);
    std::vector<float> pos(3 * n), nrm(3 * n), r2(n), rz(n);
    const int owned = rtRasterTexelsHost(tris, numTris, W, H, dilate, prim.data(), src.data(), nullptr, pos.data(), nrm.data());
    if (owned < 0) return -1;
    std::vector<float> cur(n * C, 0.0f), next(n * C, 0.0f);
    for (size_t t = 0; t < n; t++) {
        if (prim[t] == RT_GUIDE_PRIM_NONE) continue;                    // `in` is read at owned texels only
        rt_filter_footprint(tris + prim[t], W, H, sigma_d, sigma_z, &r2[t], &rz[t]);
        for (int j = 0; j < C; j++) cur[t * C + j] = in[t * C + j];
    }
    std::vector<float> sum(C);
    for (int it = 0; it < iterations; it++) {
        const int s = 1 << it;
        const float rc = rt_filter_rc(sigma_c, it);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t p = (size_t)y * W + x;
                if (prim[p] == RT_GUIDE_PRIM_NONE) continue;
                const float* cp = &cur[p * C];
                float wsum = 0.0f;
                for (int j = 0; j < C; j++) sum[j] = 0.0f;
                for (int dy = -2; dy <= 2; dy++)
                    for (int dx = -2; dx <= 2; dx++) {
                        const float h = rt_filter_kernel(dx, dy);
                        size_t q = p;
                        float w = h;
                        if (dx != 0 || dy != 0) {
                            const int qx = x + dx * s, qy = y + dy * s;
                            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                            q = (size_t)qy * W + qx;
                            if (prim[q] == RT_GUIDE_PRIM_NONE) continue;
                            if (!rt_filter_tap(&nrm[3 * p], &pos[3 * p], r2[p], rz[p], &nrm[3 * q], &pos[3 * q], h, (float)((dx * dx + dy * dy) * s * s),
                                               normal_squarings, &w))
                                continue;
                            if (sigma_c > 0.0f) w = w * rt_filter_colour(cp, &cur[q * C], L, rc);
                        }
                        for (int j = 0; j < C; j++) sum[j] = sum[j] + w * cur[q * C + j];
                        wsum = wsum + w;
                    }
                for (int j = 0; j < C; j++) next[p * C + j] = sum[j] / wsum;
            }
        cur.swap(next);
    }
    for (size_t t = 0; t < n; t++)
        for (int j = 0; j < C; j++) out[t * C + j] = src[t] == -1 ? 0.0f : cur[(size_t)src[t] * C + j];
    return owned;
}
