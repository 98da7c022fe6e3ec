// mesh_plan_dump.cpp — runs plan_mesh (rt_mesh_plan.h) on the cases of tests/test_mesh_plan.py: plain C++, no kernel, no HIP call, no GPU.
// stdin: one case per line, the integers named in kInputs below (a pointer field: 0 = null, else present).  stdout: one line per case, the plan's fields
// in the order of kOutputs.  `--fields` prints the two lists instead, for the test to hold its own lists against.
#include <cstdio>
#include <cstring>

#include "rt_mesh_plan.h"

static const char* const kInputs =
    "nx rows ns queue dbg counters lean_ok floor_on sentinels leaf_ofs leaf_tri nppl first_leaf rng_mode px_state px_rays ord_rec order ord_state ord_rays "
    "acc_first p1_segments xcd_queues variant cus mesh_lean mesh_tile_order mesh_two mesh_split mesh_heavy mesh_rounds mesh_rev mesh_chain_thr mesh_chain_lanes mesh_chain_frac";
static const char* const kOutputs =
    "error frame trav dbg stats lean grid_x grid_y threads lds stride stride1 min_traversing min_traversing1 leaf_thr leaf_thr1 split chain_top_thr xcd_queues";
constexpr int kInputCount = 35;

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "--fields") == 0) {
        printf("%s\n%s\n", kInputs, kOutputs);
        return 0;
    }
    static unsigned char present[64];      // what a non-null pointer field points to (plan_mesh reads no pointee)
    long long v[kInputCount];
    for (;;) {
        for (int i = 0; i < kInputCount; i++)
            if (scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 1;       // end of input; a partial line is an error
        auto ptr = [&](int i) { return v[i] ? (void*)present : nullptr; };
        RtMeshParams p;
        memset(&p, 0, sizeof p);
        int k = 0;
        p.nx = (int32_t)v[k++];
        p.part.local_rows = (int32_t)v[k++];
        p.ns = (int32_t)v[k++];
        p.queue = (uint32_t*)ptr(k++);
        p.dbg = (unsigned long long*)ptr(k++);
        p.counters = (RtCounters*)ptr(k++);
        p.lean_ok = (int32_t)v[k++];
        p.floor_on = (int32_t)v[k++];
        p.leaf_sentinels_trailing = (int32_t)v[k++];
        p.leaf_ofs = (const uint32_t*)ptr(k++);
        p.leaf_tri = (const float4*)ptr(k++);
        p.nppl = (uint32_t)v[k++];
        p.first_leaf = (uint32_t)v[k++];
        p.rng_mode = (int32_t)v[k++];
        p.px_state = (float4*)ptr(k++);
        p.px_rays = (uint32_t*)ptr(k++);
        p.ord_rec = (float4*)ptr(k++);
        p.order = (uint32_t*)ptr(k++);
        p.ord_state = (float4*)ptr(k++);
        p.ord_rays = (uint32_t*)ptr(k++);
        p.acc_first = (int32_t)v[k++];
        p.p1_segments = (int32_t)v[k++];
        p.xcd_queues = (int32_t)v[k++];
        const int variant = (int)(uint32_t)v[k++];
        const int cus = (int)v[k++];
        RtSwitches sw;
        sw.mesh_lean = v[k++] != 0;
        sw.mesh_tile_order = v[k++] != 0;
        sw.mesh_two = v[k++] != 0;
        sw.mesh_split = (int)v[k++];
        sw.mesh_heavy = (int)v[k++];
        sw.mesh_rounds = (int)v[k++];
        sw.mesh_rev = v[k++] != 0;
        sw.mesh_chain_thr = (int)v[k++];
        sw.mesh_chain_lanes = (int)v[k++];
        sw.mesh_chain_frac = (int)v[k++];
        if (k != kInputCount) return 2;
        const MeshPlan pl = plan_mesh(p, variant, sw, cus);
        printf("%d %d %d %d %d %d %u %u %d %zu %u %u %d %d %d %d %d %d %d\n", (int)pl.error, (int)pl.frame, pl.trav, (int)pl.dbg, (int)pl.stats, (int)pl.lean, pl.grid_x, pl.grid_y,
               pl.threads, pl.lds, pl.stride, pl.stride1, pl.min_traversing, pl.min_traversing1, pl.leaf_thr, pl.leaf_thr1, pl.split, pl.chain_top_thr, pl.xcd_queues);
    }
}
