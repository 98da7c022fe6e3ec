// rt_display_host.cpp — rtDisplayFrameHost (librt_host.so): displayFrame's definition (include/rt_api.h) in plain C++ with libm's powf, for a host without
// a GPU and as the CPU twin the device kernels (csrc/rt_kernels_display.hip) are held against.  Compiled without contraction, like the rest of this library:
// every fp32 operation below is one rounded operation, in the order written.
#include "../../include/rt_api.h"
#include "../../include/rt_host.h"

#include <cmath>
#include <cstring>

namespace {

const uint8_t kBayer8[8][8] = RT_DISPLAY_BAYER8;
const int kBinBias = (127 - 16) << 3;

inline float lum(const float* x) { return 0.2126f * x[0] + 0.7152f * x[1] + 0.0722f * x[2]; }
inline float max0(float x) { return x > 0.0f ? x : 0.0f; }

inline uint32_t bits_of(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
inline float float_of(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

}  // namespace

extern "C" int rtDisplayFrameHost(const rt_vec3* in, uint8_t* out_rgba, int nx, int ny, int flags, int tonemap, float exposure, float adapt, float* E_state,
                                  uint32_t* hist) {
    const int known = RT_DISPLAY_TOP_DOWN | RT_DISPLAY_DITHER | RT_DISPLAY_AUTO_EXPOSURE;
    if (!in || !out_rgba || nx <= 0 || ny <= 0 || (flags & ~known) != 0 || tonemap < RT_TONEMAP_NONE || tonemap > RT_TONEMAP_ACES) return -1;
    if (!std::isfinite(exposure) || !(exposure > 0.0f) || !std::isfinite(adapt) || !(adapt > 0.0f) || adapt > 1.0f) return -1;
    const size_t npix = (size_t)nx * (size_t)ny;
    float E_used = exposure;
    if (flags & RT_DISPLAY_AUTO_EXPOSURE) {
        uint32_t own[RT_DISPLAY_BINS];
        uint32_t* h = hist ? hist : own;
        memset(h, 0, RT_DISPLAY_BINS * sizeof(uint32_t));
        for (size_t q = 0; q < npix; q++) {
            const float l = lum(in[q].e);
            const int b = (int)(bits_of(l) >> 20) - kBinBias;
            if (std::isfinite(l) && l > 0.0f && b >= 0) h[b < RT_DISPLAY_BINS - 1 ? b : RT_DISPLAY_BINS - 1]++;
        }
        uint64_t total = 0, cum = 0;
        for (int k = 0; k < RT_DISPLAY_BINS; k++) total += h[k];
        float target = 1.0f;
        if (total != 0) {
            int m = 0;
            for (;; m++) {
                cum += h[m];
                if (2 * cum >= total) break;
            }
            target = RT_DISPLAY_KEY / float_of(((uint32_t)(m + kBinBias) << 20) | (1u << 19));
        }
        float E = target;
        if (E_state && !std::isnan(*E_state)) E = *E_state + adapt * (target - *E_state);
        if (E_state) *E_state = E;
        E_used = E * exposure;
    }
    for (int j = 0; j < ny; j++) {
        uint8_t* row = out_rgba + (size_t)((flags & RT_DISPLAY_TOP_DOWN) ? ny - 1 - j : j) * nx * 4;
        for (int i = 0; i < nx; i++) {
            const float* c = in[(size_t)j * nx + i].e;
            float y[3] = { c[0] * E_used, c[1] * E_used, c[2] * E_used };
            if (tonemap == RT_TONEMAP_REINHARD) {
                const float den = 1.0f + max0(lum(y));
                for (int k = 0; k < 3; k++) y[k] = y[k] / den;
            } else if (tonemap == RT_TONEMAP_ACES) {
                for (int k = 0; k < 3; k++) {
                    const float a = max0(y[k]);
                    y[k] = (a * (2.51f * a + 0.03f)) / (a * (2.43f * a + 0.59f) + 0.14f);
                }
            }
            const float d = ((float)kBayer8[j & 7][i & 7] + 0.5f) / 64.0f;
            for (int k = 0; k < 3; k++) {
                float s = max0(y[k]);
                s = max0(1.055f * powf(s, 0.416666667f) - 0.055f);
                const float t = (flags & RT_DISPLAY_DITHER) ? s * 255.0f + d : s * 255.9f;
                row[4 * i + k] = t >= 255.0f ? 255 : (uint8_t)(uint32_t)t;
            }
            row[4 * i + 3] = 255;
        }
    }
    return 0;
}
