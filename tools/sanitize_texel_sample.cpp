// tools/sanitize_texel_sample.cpp — a stand-alone driver of rtSampleTexelsHost (host/rt_texel_sample_host.cpp, which compiles csrc/rt_texel_sample.h, the
// text of the device lookup) for a run under AddressSanitizer + UBSan: heap arrays sized exactly, so a texel index or a hit index one past its plane is a
// report.  Inputs: random, NaN, inf and denormal UVs and plane values, prims inside, outside and on sentinel slots, every width, both filters, atlases down to
// 1 x 1.  Build and run (no GPU, nothing preloaded):
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -std=c++14 tools/sanitize_texel_sample.cpp \
//       cuda-raytracing-optimized_amd/host/rt_texel_sample_host.cpp -o build/sanitize_texel_sample && build/sanitize_texel_sample
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../include/rt_api.h"
#include "../include/rt_host.h"

int main() {
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> uni(-2.0f, 3.0f);
    const float special[] = { NAN, INFINITY, -INFINITY, 1e-40f, -1e-40f, 1.4e-45f, 0.0f, -0.0f, 1e30f, -1e30f, 3.4e38f, 0.5f, 1.0f };
    const int nspecial = (int)(sizeof special / sizeof special[0]);
    auto value = [&]() { return (rng() % 4 == 0) ? special[rng() % nspecial] : uni(rng); };
    const int sizes[][2] = { { 1, 1 }, { 1, 5 }, { 5, 1 }, { 16, 16 }, { 37, 23 } };
    const int modes[] = { RT_GATHER_IRRADIANCE, RT_GATHER_SH9, RT_GATHER_VISIBILITY };
    const int widths[] = { 3, 27, 1 };
    long long hits = 0, valid_hits = 0;
    for (const auto& size : sizes)
        for (int m = 0; m < 3; m++)
            for (int flags = 0; flags < 2; flags++) {
                const int W = size[0], H = size[1], C = widths[m], numTris = 19, n = 4099;
                std::vector<rt_triangle> tris(numTris);
                for (auto& t : tris) {
                    memset(&t, 0, sizeof t);
                    for (int k = 0; k < 3; k++)
                        for (int a = 0; a < 3; a++) t.v[k].e[a] = uni(rng);
                    for (int k = 0; k < 6; k++) t.texCoords[k] = value();
                }
                tris[3].v[0].e[0] = INFINITY; tris[7].v[0].e[0] = -INFINITY; tris[11].v[0].e[0] = NAN;
                std::vector<float> planes((size_t)W * H * C), uv(2 * (size_t)n), nrm(3 * (size_t)n), out(3 * (size_t)n);
                std::vector<int32_t> prim(n);
                std::vector<uint8_t> valid(n);
                for (auto& v : planes) v = value();
                for (auto& v : uv) v = value();
                for (auto& v : nrm) v = value();
                const int32_t odd[] = { -1, -2, numTris, numTris + 1, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min(), 3, 7, 11 };
                for (int k = 0; k < n; k++) prim[k] = (rng() % 5 == 0) ? odd[rng() % 9] : (int32_t)(rng() % numTris);
                const int count = rtSampleTexelsHost(tris.data(), numTris, n, prim.data(), uv.data(), nrm.data(), W, H, modes[m], planes.data(), flags, out.data(),
                                                     valid.data());
                int sum = 0;
                for (int k = 0; k < n; k++) {
                    sum += valid[k];
                    if (!valid[k] && (out[3 * k] != 0.0f || out[3 * k + 1] != 0.0f || out[3 * k + 2] != 0.0f)) { printf("an invalid hit with a value\n"); return 1; }
                }
                if (count != sum || count <= 0 || count >= n) { printf("count %d against %d valid bytes\n", count, sum); return 1; }
                hits += n; valid_hits += count;
            }
    printf("rtSampleTexelsHost: %lld hits, %lld valid, 5 atlas sizes x 3 widths x 2 filters: clean\n", hits, valid_hits);
    return 0;
}
