// rtRasterTexelsHost and rtAtlasGrid (include/rt_host.h): the UV-atlas raster of rasterTexels / bakeTexels on the CPU, and a trivial atlas for meshes without
// unique UVs.  The raster's arithmetic is csrc/rt_texel_raster.h, the text the device kernels compile: this file is built with -ffp-contract=off, and x86-64's
// sqrtf and division are correctly rounded.  The twin walks every candidate slot over every texel of its clipped UV box in ascending slot order and keeps the
// first to cover a texel - the lowest covering slot, what the device's atomicMin leaves.
#include "../../include/rt_api.h"
#include "../../include/rt_host.h"

#include <cmath>
#include <cstddef>
#include <vector>

#include "../csrc/rt_texel_raster.h"

extern "C" int rtRasterTexelsHost(const rt_triangle* tris, uint32_t numTris, int W, int H, int dilate, int32_t* prim, int32_t* src, float* bary, float* pos,
                                  float* nrm) {
    // what rasterTexels refuses: nothing is written
    if (W < 1 || H < 1 || W > RT_TEXEL_MAX_SIZE || H > RT_TEXEL_MAX_SIZE || dilate < 0 || dilate > RT_TEXEL_MAX_DILATE) return -1;
    if ((!tris && numTris > 0) || (!prim && !src && !bary && !pos && !nrm)) return -1;
    const size_t n = (size_t)W * H;
    std::vector<int32_t> owner(n, RT_GUIDE_PRIM_NONE);
    for (uint32_t k = 0; k < numTris; k++) {
        const rt_triangle* t = tris + k;
        if (!rt_texel_candidate(t)) continue;
        float box[4];
        int x0, x1, y0, y1;
        rt_texel_box(t->texCoords, box);
        rt_texel_span(box[0], box[1], W, &x0, &x1);
        rt_texel_span(box[2], box[3], H, &y0, &y1);
        for (int y = y0; y <= y1; y++)
            for (int x = x0; x <= x1; x++) {
                int32_t& o = owner[(size_t)y * W + x];
                if (o != RT_GUIDE_PRIM_NONE) continue;                  // a lower slot covers it
                float s[2], h[2];
                rt_texel_sample(x, y, W, H, s);
                if (rt_texel_cover(t->texCoords, box, s, h)) o = (int32_t)k;
            }
    }
    int owned = 0;
    std::vector<int32_t> cur(src || dilate > 0 ? n : 0), next(dilate > 0 ? n : 0);
    for (size_t i = 0; i < n; i++) {
        const int32_t o = owner[i];
        float h[2] = { 0.0f, 0.0f }, P[3] = { 0.0f, 0.0f, 0.0f }, N[3] = { 0.0f, 0.0f, 0.0f };
        if (o != RT_GUIDE_PRIM_NONE) {
            owned++;
            if (bary || pos || nrm) {
                float box[4], s[2];
                rt_texel_box(tris[o].texCoords, box);
                rt_texel_sample((int)(i % (size_t)W), (int)(i / (size_t)W), W, H, s);
                rt_texel_cover(tris[o].texCoords, box, s, h);
                rt_texel_resolve(tris + o, h, P, N);
            }
        }
        if (prim) prim[i] = o;
        if (!cur.empty()) cur[i] = o != RT_GUIDE_PRIM_NONE ? (int32_t)i : -1;
        if (bary) { bary[2 * i] = h[0]; bary[2 * i + 1] = h[1]; }
        if (pos) { pos[3 * i] = P[0]; pos[3 * i + 1] = P[1]; pos[3 * i + 2] = P[2]; }
        if (nrm) { nrm[3 * i] = N[0]; nrm[3 * i + 1] = N[1]; nrm[3 * i + 2] = N[2]; }
    }
    if (src) {
        for (int it = 0; it < dilate; it++) {
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) next[(size_t)y * W + x] = rt_texel_dilate(cur.data(), x, y, W, H);
            cur.swap(next);
        }
        for (size_t i = 0; i < n; i++) src[i] = cur[i];
    }
    return owned;
}

extern "C" int rtAtlasGrid(rt_triangle* tris, int n, float margin) {
    if (!tris || n < 1 || !(margin >= 0.0f && margin < 0.25f)) return 0;
    const int pairs = (n + 1) / 2;
    int cells = 1;
    while ((long long)cells * cells < pairs) cells++;
    const float cs = 1.0f / (float)cells, m = margin * cs, m3 = 3.0f * m;
    for (int i = 0; i < n; i++) {
        const int q = i / 2;
        const float u0 = (float)(q % cells) * cs, v0 = (float)(q / cells) * cs;
        const float u1 = u0 + cs, v1 = v0 + cs;
        float* tc = tris[i].texCoords;
        if ((i & 1) == 0) {                                             // the lower-left half
            tc[0] = u0 + m; tc[1] = v0 + m;
            tc[2] = u1 - m3; tc[3] = v0 + m;
            tc[4] = u0 + m; tc[5] = v1 - m3;
        } else {                                                        // the upper-right half
            tc[0] = u1 - m; tc[1] = v1 - m;
            tc[2] = u0 + m3; tc[3] = v1 - m;
            tc[4] = u1 - m; tc[5] = v0 + m3;
        }
    }
    return cells;
}
