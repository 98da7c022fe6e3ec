// rt_mesh_plan.h — what a mesh frame launches: the constants the mesh launcher (rt_kernels_mesh.hip) and its persistent kernel share, the named bit fields of
// the kernel's two packed arguments, and plan_mesh, which decides a frame's launches before anything is issued.  No kernel and no HIP call in here: a plain C++
// program that includes this header runs the plan on a machine without a GPU (tests/mesh_plan_dump.cpp, tests/test_mesh_plan.py).
#pragma once

#include "rt_params.h"

#ifndef RT_MESH_WG_WAVES
#define RT_MESH_WG_WAVES 4          // waves per workgroup (experiment: 16 = one workgroup per CU, one LDS copy of the tables)
#endif
#ifndef RT_MESH_LEAN_WAVES
#define RT_MESH_LEAN_WAVES 4        // waves per SIMD of the lean instantiation (its launch bound)
#endif
constexpr int kWavesPerWg = RT_MESH_WG_WAVES;
constexpr int kThreads = 64 * kWavesPerWg;
constexpr int kMinTraversing = 40;          // classic traversal: TRAVERSE while at least this many lanes still have nodes to visit
constexpr uint32_t kLeafCntLds = 32768;     // leaves whose triangle counts the default kernel keeps in the LDS (one byte each, beside its 5 KB of pair-round scratch)

// The kernel argument leaf_thr: the leaf threshold and, for the second dispatch of a two-dispatch frame (PHASE 2), its scheduling constants.
constexpr BitField kLeafThr = { 0, 0xFF };              // the leaf loop runs as soon as this many lanes wait at a leaf
constexpr BitField kLeafHeavyClasses = { 8, 0xF };      // cost classes counted as expensive and spread over the first fills (RtSwitches::mesh_heavy; 0 = off) ...
constexpr BitField kLeafSpreadRounds = { 12, 0xF };     // ... of this many times the lanes in flight (mesh_rounds)
constexpr BitField kLeafChainLanes = { 16, 0xFF };      // pixels of list 0 per chain wave (mesh_chain_lanes; 0 = no chain waves)
constexpr BitField kLeafChainFrac = { 24, 0xF };        // chain waves only while list 0 is below pixels >> this (mesh_chain_frac)
// The kernel argument min_traversing.
constexpr BitField kMinTravLanes = { 0, 0xFF };         // keep traversing while at least this many lanes have nodes left
constexpr BitField kMinTravSegments = { 8, 1 };         // first dispatch (PHASE 1): the permutation moves row segments of 8 pixels

enum class MeshFrame {
    Tiles,          // the first kernel: one tile per wave (variant 1)
    TwoDispatch,    // the cost-ordered frame: samples [0, split) of every pixel, the ordering pass, then the rest longest first
    Single,         // one dispatch of whole pixels
};
enum class MeshPlanError { None, NoQueue };

// What a frame launches, decided by plan_mesh before anything is issued.
struct MeshPlan {
    MeshPlanError error = MeshPlanError::None;      // NoQueue: the persistent kernel without RtMeshParams::queue - nothing is issued
    MeshFrame frame = MeshFrame::Single;
    // the instantiation of k_render_mesh_queue (both dispatches of a two-dispatch frame take the same)
    int trav = 0;
    bool dbg = false, stats = false, lean = false;
    unsigned grid_x = 1, grid_y = 1;
    int threads = kThreads;
    size_t lds = 0;
    uint32_t stride = 1;            // scattered order: ~0.618 x total, coprime with total (1 = tile-major); two dispatches: the second's (0xFFFFFFFF = cheapest first)
    uint32_t stride1 = 1;           // ... of the first dispatch
    int min_traversing = 0;         // the kernel's min_traversing word: the single dispatch, or the second of two
    int min_traversing1 = 0;        // ... of the first dispatch
    int leaf_thr = 0;               // the kernel's leaf_thr word: the single dispatch, or the second of two
    int leaf_thr1 = 0;              // ... of the first dispatch
    int split = 0;                  // two dispatches: samples of the first
    int chain_top_thr = 0;          // ... and what the ordering pass takes for list 0: pixels from 16 x this many cost units per sample (the chains)
    int xcd_queues = 0;             // ... and the sets of cost lists and queue counters of the ordering pass and the second dispatch (RtMeshParams::xcd_queues)
};

// variant: bits 0..7  0 = persistent state-machine kernel (default), 1 = first kernel (one tile per wave);
//          bits 8..15 workgroups per CU of the persistent kernel (0 = default 4);
//          bits 16..23 keep traversing while at least this many lanes have nodes left (0 = default: 24, classic 40);
//          bits 24..25 traversal of the persistent kernel: 0 = thresholded while-while (default), 1 = classic while-while;
//          bits 26..31 leaf threshold of the former (0 = default: one full pair round).
// cus: the device's compute units.
inline MeshPlan plan_mesh(const RtMeshParams& p, int variant, const RtSwitches& sw, int cus) {
    MeshPlan pl;
    if ((variant & 0xFF) == 1) {
        pl.frame = MeshFrame::Tiles;
        pl.grid_x = (p.nx + 8 * kWavesPerWg - 1) / (8 * kWavesPerWg);
        pl.grid_y = (p.part.local_rows + 7) / 8;
        return pl;
    }
    if (!p.queue) { pl.error = MeshPlanError::NoQueue; return pl; }
    const bool classic = ((variant >> 24) & 3) == 1;
    pl.trav = classic ? 1 : 0;
    // the diagnostic instantiation (DBG) when the phase counters are asked for, else the counting one (STATS: the reference's ray statistics as device atomics)
    // when counters are, else the lean one where the scene allows it
    pl.dbg = p.dbg != nullptr;
    pl.stats = !pl.dbg && p.counters != nullptr;
    pl.lean = sw.mesh_lean && !classic && !p.dbg && !p.counters && p.lean_ok && !p.floor_on && p.leaf_sentinels_trailing && p.leaf_ofs && p.leaf_tri &&
              p.nppl >= 1u && p.nppl <= 16u && p.first_leaf <= kLeafCntLds;
    int wg_per_cu = (variant >> 8) & 0xFF;
    // (a workgroup of four waves puts one on every SIMD, so the default is the instantiation's launch bound in waves per SIMD: 4 at 128 VGPRs - the pair rounds
    // spill at 96 -, the classic traversal 5 at 96)
    if (wg_per_cu == 0) wg_per_cu = pl.lean ? RT_MESH_LEAN_WAVES : (classic ? 5 : 4);
    const long long total_px = (long long)((p.nx + 7) / 8) * ((p.part.local_rows + 7) / 8) * 64;
    const long long useful = (total_px + kThreads - 1) / kThreads;                // never more lanes than pixels
    long long blocks = (long long)cus * wg_per_cu * 4 / kWavesPerWg;
    if (blocks > useful) blocks = useful;
    if (blocks < 1) blocks = 1;
    pl.grid_x = (unsigned)blocks;
    if (total_px > 64 && !sw.mesh_tile_order) pl.stride = rt_coprime_stride((unsigned long long)total_px);
    int min_traversing = (variant >> 16) & 0xFF;
    if (min_traversing == 0) min_traversing = classic ? kMinTraversing : 24;    // measured: 16 -> 409, 20 -> 435, 24 -> 446, 32 -> 429 Msamples/s
    int leaf_thr = (variant >> 26) & 0x3F;
    // default leaf threshold = one full pair round: 64 / nppl waiting rays (12 at 5 triangles per leaf).  Measured on C4 with full rounds
    // only: 8 -> 607, 12 -> 648, 16 -> 616, 24 -> 541 Msamples/s (round 1, with partial rounds: 16 -> 610).
    if (leaf_thr == 0) leaf_thr = (p.nppl >= 1u && p.nppl <= 16u) ? (int)(64u / p.nppl) : 16;
    pl.min_traversing = kMinTravLanes.put(min_traversing);
    pl.leaf_thr = kLeafThr.put(leaf_thr);
    pl.lds = (!classic && p.leaf_ofs && p.first_leaf <= kLeafCntLds) ? (size_t)((p.first_leaf + 15u) & ~15u) : 0;      // the leaf-count table
    // The cost-ordered frame in two dispatches (template parameter PHASE): reference RNG stream, no diagnostics, enough samples for the first few to be a small part.
    // RT_MESH_TWO=0: the single scattered dispatch (A/B); RT_MESH_SPLIT=<n>: samples of the first dispatch.
    // (a continuation pass of a progressive frame, p.acc_first > 0, takes the single dispatch: PHASE 0 resumes every pixel from p.acc_state)
    const bool parked_buffers = p.px_state && p.px_rays && (p.ord_rec || (p.order && p.ord_state && p.ord_rays));
    const bool two = sw.mesh_two && !classic && !p.dbg && !p.counters && p.rng_mode == RT_RNG_REFERENCE_STREAM && parked_buffers && p.acc_first == 0 &&
                     p.ns >= 4 * sw.mesh_split && p.nx <= 65535 && p.part.local_rows <= 65535;
    if (!two) return pl;
    pl.frame = MeshFrame::TwoDispatch;
    pl.split = sw.mesh_split;
    pl.chain_top_thr = sw.mesh_chain_thr;
    // The first dispatch: the single dispatch's order and words, or (p.p1_segments) row segments of 8 pixels scattered - its stride coprime with total / 8
    pl.stride1 = pl.stride;
    pl.min_traversing1 = pl.min_traversing;
    pl.leaf_thr1 = pl.leaf_thr;
    if (p.p1_segments && total_px > 512 && !sw.mesh_tile_order) {
        pl.stride1 = rt_coprime_stride((unsigned long long)total_px >> 3);
        pl.min_traversing1 |= kMinTravSegments.put(1);
    }
    // The second dispatch: the lists longest first (RT_MESH_REV=1: cheapest first), its scheduling constants beside the leaf threshold
    // (cheapest first takes ONE queue for the machine: a wave that has emptied its XCD's queue takes the other queues' pixels from the front of their lists,
    // their own waves from the back, by one counter - with a queue per XCD the two would meet, pixels traced twice and pixels never traced)
    pl.xcd_queues = p.xcd_queues;
    if (sw.mesh_rev) {
        pl.stride = 0xFFFFFFFFu;
        pl.xcd_queues = 0;
    }
    pl.leaf_thr |= kLeafHeavyClasses.put(sw.mesh_heavy & kLeafHeavyClasses.mask) | kLeafSpreadRounds.put(sw.mesh_rounds & kLeafSpreadRounds.mask) |
                   kLeafChainLanes.put(sw.mesh_chain_lanes) | kLeafChainFrac.put(sw.mesh_chain_frac);
    return pl;
}
