// rtGatherDirectionsHost (include/rt_host.h): the direction generator of gatherRadiance on the CPU.  The arithmetic is csrc/rt_gather_dirs.h, the text the
// device kernel compiles: this file is built with -ffp-contract=off, and x86-64's sqrtf and division are correctly rounded.
#include "../../include/rt_api.h"
#include "../../include/rt_host.h"

#include <cmath>
#include <cstddef>

#include "../csrc/rt_gather_dirs.h"

extern "C" void rtGatherDirectionsHost(int n, const float* pos, const float* nrm, int mode, int first, int dirs, int dirs_total, uint32_t base_id, float bias,
                                       float* org, float* dir, uint32_t* ids) {
    // what rtGatherDirections refuses: nothing is written
    if (n <= 0 || !pos || (mode != RT_GATHER_IRRADIANCE && mode != RT_GATHER_SH9 && mode != RT_GATHER_VISIBILITY)) return;
    if ((mode != RT_GATHER_SH9 && !nrm) || dirs < 1 || first < 0 || (long long)first + dirs > dirs_total || dirs_total > RT_GATHER_MAX_DIRS) return;
    if ((!org && !dir && !ids) || !std::isfinite(bias)) return;
    for (int k = 0; k < n; k++)
        for (int j = 0; j < dirs; j++) {
            const size_t e = (size_t)k * dirs + j;
            const uint32_t g = rt_gather_id(base_id, (uint32_t)k, (uint32_t)dirs_total, (uint32_t)(first + j));
            float o[3], D[3];
            rt_gather_ray(mode, pos + 3 * (size_t)k, mode == RT_GATHER_SH9 ? nullptr : nrm + 3 * (size_t)k, bias, g, o, D);
            if (org) { org[3 * e] = o[0]; org[3 * e + 1] = o[1]; org[3 * e + 2] = o[2]; }
            if (dir) { dir[3 * e] = D[0]; dir[3 * e + 1] = D[1]; dir[3 * e + 2] = D[2]; }
            if (ids) ids[e] = g;
        }
}
