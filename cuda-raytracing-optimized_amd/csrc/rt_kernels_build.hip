// rt_kernels_build.hip — the BVH rebuild behind rebuildBvh (include/rt_api.h, "editing the scene"): the host builder of rt_bvh.cpp
// (full-sweep SAH over a fixed complete tree) restated level by level, so that every decision is the same comparison of the same fp32 values.
//
//   gather   leaf counts (leading non-sentinels) -> exclusive scan -> triangle i = the i-th visible slot: src[i], box (6 planes), the three centroid keys
//   sort x3  stable LSD radix sort (4 passes of 8 bits) of (monotone image of cent[axis], -0 as +0), starting from index order: ties end by index
//   level    per axis a forward and a backward segmented min / max scan of the boxes along the sorted list -> area left and right of every cut;
//            cost per (axis, cut); argmin of (cost, axis, cut) per node as an integer minimum of one 64-bit key; the left set flagged through the winning
//            axis's list; a stable partition of all three lists (an exclusive scan of the flags); the children's ranges
//   emit     the 64-byte triangles into the second slot buffer in the order of the parent's winning axis, sentinels elsewhere, old_slot, leaf count bytes
//
// Every scan is three launches - tile scan, a scan of the tile aggregates by one workgroup per list, apply - and a pass reads what the pass before it wrote,
// in stream order: no flags, no waits and no look-back between the workgroups of a launch.  The only atomics are integer ones whose result does not depend
// on the order of arrival (LDS histogram counters, a 64-bit minimum).  Segments run from the whole array (the root) to empty: one code path, every loop bound
// uniform in the workgroup and every barrier reached by every lane.  Built like display.o: no contraction, so area and cost round as the host's do.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_build.h"

namespace {

constexpr uint32_t kT = kBuildTile;     // lanes of a workgroup = elements of a tile
static_assert(kT == 256, "the radix scatter ranks four waves of 64 lanes, the scans take log2(256) steps");
constexpr unsigned long long kNoKey = ~0ull;

__host__ __device__ inline uint32_t tiles_of(uint32_t len) { return len == 0 ? 1u : (len + kT - 1) / kT; }

// ---- the workspace -------------------------------------------------------------------------------------------------------------------------------------
struct Work {
    uint32_t *cnt, *base, *src, *key, *ord, *G, *node, *left, *nbeg, *nend, *nsplit, *waxis, *hist, *agg;
    float *box, *area, *segagg, *segcarry;
    unsigned long long* best;
    uint32_t hist_len, agg_stride, nt;
};

size_t carve(Work& w, uint32_t* base, uint32_t n, uint32_t first_leaf) {
    size_t at = 0;
    auto take = [&](size_t words) { uint32_t* p = base ? base + at : nullptr; at += (words + 1) & ~(size_t)1; return p; };
    const size_t n1 = n ? n : 1, nl = first_leaf;
    w.nt = tiles_of(n);
    w.hist_len = 256u * w.nt;
    const size_t longest = nl > w.hist_len ? nl : w.hist_len;
    w.agg_stride = tiles_of((uint32_t)longest);
    w.best = reinterpret_cast<unsigned long long*>(take(2 * nl));
    w.cnt = take(nl); w.base = take(nl); w.src = take(n1);
    w.box = reinterpret_cast<float*>(take(6 * n1));
    w.key = take(6 * n1); w.ord = take(6 * n1);
    w.area = reinterpret_cast<float*>(take(6 * n1));
    w.G = take(3 * n1); w.node = take(2 * n1); w.left = take(n1);
    w.nbeg = take(2 * nl); w.nend = take(2 * nl); w.nsplit = take(nl); w.waxis = take(nl);
    w.hist = take(3 * (size_t)w.hist_len);
    w.agg = take(3 * (size_t)w.agg_stride);
    w.segagg = reinterpret_cast<float*>(take(6 * 7 * (size_t)w.nt));
    w.segcarry = reinterpret_cast<float*>(take(6 * 7 * (size_t)w.nt));
    return at;
}

// ---- plain exclusive scans of uint32 lists (grid.y lists) ----------------------------------------------------------------------------------------------
struct ScanArgs {
    const uint32_t* src; uint32_t src_stride;      // value(p) of list y = src[y * src_stride + p], or
    const uint32_t* idx; uint32_t idx_stride;      // (idx != nullptr) src[idx[y * idx_stride + p]]
    uint32_t* out; uint32_t out_stride;            // exclusive prefix sums
    uint32_t* agg; uint32_t agg_stride;            // tile aggregates, then their exclusive scan
    uint32_t len;
};

__device__ inline uint32_t scan_value(const ScanArgs& a, uint32_t y, uint32_t p) {
    if (p >= a.len) return 0u;
    return a.idx ? a.src[a.idx[(size_t)y * a.idx_stride + p]] : a.src[(size_t)y * a.src_stride + p];
}

// inclusive sums over the workgroup's lanes; s holds kT words
__device__ inline uint32_t block_scan_incl(uint32_t v, uint32_t* s) {
    const uint32_t tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kT; d *= 2) {
        const uint32_t t = tid >= d ? s[tid - d] : 0u;
        __syncthreads();
        v += t;
        s[tid] = v;
        __syncthreads();
    }
    return v;
}

__global__ void __launch_bounds__(kT) k_scan_reduce(const ScanArgs a) {
    __shared__ uint32_t s[kT];
    const uint32_t y = blockIdx.y, t = blockIdx.x;
    const uint32_t incl = block_scan_incl(scan_value(a, y, t * kT + threadIdx.x), s);
    if (threadIdx.x == kT - 1) a.agg[(size_t)y * a.agg_stride + t] = incl;
}

__global__ void __launch_bounds__(kT) k_scan_carry(uint32_t* agg, uint32_t agg_stride, uint32_t ntiles) {
    __shared__ uint32_t s[kT];
    uint32_t* g = agg + (size_t)blockIdx.x * agg_stride;
    uint32_t running = 0;
    for (uint32_t c = 0; c < ntiles; c += kT) {            // (uniform: ntiles is the launch's)
        const uint32_t t = c + threadIdx.x;
        const uint32_t v = t < ntiles ? g[t] : 0u;
        const uint32_t incl = block_scan_incl(v, s);
        if (t < ntiles) g[t] = running + incl - v;
        running += s[kT - 1];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kT) k_scan_apply(const ScanArgs a) {
    __shared__ uint32_t s[kT];
    const uint32_t y = blockIdx.y, t = blockIdx.x, p = t * kT + threadIdx.x;
    const uint32_t v = scan_value(a, y, p);
    const uint32_t incl = block_scan_incl(v, s);
    if (p < a.len) a.out[(size_t)y * a.out_stride + p] = a.agg[(size_t)y * a.agg_stride + t] + incl - v;
}

// ---- gather --------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT) k_leaf_count(const rt_triangle* slots, uint32_t first_leaf, uint32_t nppl, uint32_t* cnt) {
    const uint32_t leaf = blockIdx.x * kT + threadIdx.x;
    if (leaf >= first_leaf) return;
    uint32_t c = 0;
    while (c < nppl && !isinf(slots[(size_t)leaf * nppl + c].v[0].e[0])) c++;
    cnt[leaf] = c;
}

__device__ inline uint32_t centroid_key(float c) {
    uint32_t u = __float_as_uint(c);
    if (u == 0x80000000u) u = 0u;                           // -0 sorts as +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(kT) k_gather(const rt_triangle* slots, uint32_t first_leaf, uint32_t nppl, uint32_t n, const uint32_t* cnt, const uint32_t* base,
                                               uint32_t* src, float* box, uint32_t* key, uint32_t* ord, uint32_t* node) {
    const uint32_t leaf = blockIdx.x * kT + threadIdx.x;
    if (leaf >= first_leaf) return;
    const uint32_t c = cnt[leaf], b = base[leaf];
    for (uint32_t k = 0; k < c; k++) {
        const uint32_t i = b + k;
        if (i >= n) return;                                 // (the host counted the same slots: never taken)
        const size_t s = (size_t)leaf * nppl + k;
        const rt_triangle& t = slots[s];
        src[i] = (uint32_t)s;
        node[i] = 1u;
        for (int a = 0; a < 3; a++) {
            const float p0 = t.v[0].e[a], p1 = t.v[1].e[a], p2 = t.v[2].e[a];
            const float lo = fminf(fminf(p0, p1), p2), hi = fmaxf(fmaxf(p0, p1), p2);
            box[(size_t)a * n + i] = lo;
            box[(size_t)(3 + a) * n + i] = hi;
            key[(size_t)a * n + i] = centroid_key(0.5f * (lo + hi));
            ord[(size_t)a * n + i] = i;
        }
    }
}

__global__ void k_root(uint32_t n, uint32_t* nbeg, uint32_t* nend) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { nbeg[1] = 0; nend[1] = n; }
}

// ---- radix sort: one pass = histogram, scan of (digit, tile) counts, stable scatter ---------------------------------------------------------------------
__global__ void __launch_bounds__(kT) k_radix_hist(const uint32_t* key, uint32_t n, uint32_t shift, uint32_t* hist, uint32_t hist_len, uint32_t nt) {
    __shared__ uint32_t s[256];
    const uint32_t a = blockIdx.y, t = blockIdx.x, p = t * kT + threadIdx.x;
    s[threadIdx.x] = 0;
    __syncthreads();
    if (p < n) atomicAdd(&s[(key[(size_t)a * n + p] >> shift) & 255u], 1u);
    __syncthreads();
    hist[(size_t)a * hist_len + (size_t)threadIdx.x * nt + t] = s[threadIdx.x];
}

__global__ void __launch_bounds__(kT) k_radix_scatter(const uint32_t* key_in, const uint32_t* ord_in, uint32_t* key_out, uint32_t* ord_out, uint32_t n,
                                                      uint32_t shift, const uint32_t* hist, uint32_t hist_len, uint32_t nt) {
    __shared__ uint32_t s_cnt[4][256];
    const uint32_t a = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, p = t * kT + tid;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    for (uint32_t w = 0; w < 4; w++) s_cnt[w][tid] = 0;
    __syncthreads();
    const bool valid = p < n;
    const uint32_t k = valid ? key_in[(size_t)a * n + p] : 0u;
    const uint32_t o = valid ? ord_in[(size_t)a * n + p] : 0u;
    const uint32_t d = (k >> shift) & 255u;
    unsigned long long same = __ballot(valid);             // the lanes of this wave with this lane's digit
    for (uint32_t bit = 0; bit < 8; bit++) {
        const bool on = (d >> bit) & 1u;
        const unsigned long long b = __ballot(on);
        same &= on ? b : ~b;
    }
    const uint32_t before = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && before == 0) s_cnt[wave][d] = (uint32_t)__popcll(same);
    __syncthreads();
    if (valid) {
        uint32_t pos = hist[(size_t)a * hist_len + (size_t)d * nt + t] + before;
        for (uint32_t w = 0; w < wave; w++) pos += s_cnt[w][d];
        if (pos < n) {                                      // (always: the scanned counts of n keys)
            key_out[(size_t)a * n + pos] = k;
            ord_out[(size_t)a * n + pos] = o;
        }
    }
}

// ---- segmented box scans -------------------------------------------------------------------------------------------------------------------------------
__device__ inline void box_identity(float (&b)[6]) { b[0] = b[1] = b[2] = INFINITY; b[3] = b[4] = b[5] = -INFINITY; }
__device__ inline void box_merge(float (&b)[6], const float (&o)[6]) {
    for (int a = 0; a < 3; a++) { b[a] = fminf(b[a], o[a]); b[3 + a] = fmaxf(b[3 + a], o[3 + a]); }
}
// Box::area of rt_bvh.cpp: every operation rounded on its own, operands in that order
__device__ inline float box_area(const float (&b)[6]) {
    if (b[3] < b[0]) return 0.0f;
    const float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
    return 2.0f * (dx * dy + dy * dz + dz * dx);
}

// Inclusive segmented min / max scan over the workgroup's lanes: f = "a segment starts at this lane" on entry, "... at or before this lane, inside the tile"
// on return; lanes still without a start take `carry`, the scan's value before the tile.  *agg_f / agg (lane kT-1's, before the carry) are the tile's aggregate.
__device__ inline void block_seg_scan(float (&b)[6], uint32_t& f, const float (&carry)[6], float (*s_box)[kT], uint32_t* s_f, float (&agg)[6], uint32_t& agg_f) {
    const uint32_t tid = threadIdx.x;
    for (int c = 0; c < 6; c++) s_box[c][tid] = b[c];
    s_f[tid] = f;
    __syncthreads();
    for (uint32_t d = 1; d < kT; d *= 2) {
        float nb[6]; uint32_t nf = 0;
        box_identity(nb);
        if (tid >= d) { for (int c = 0; c < 6; c++) nb[c] = s_box[c][tid - d]; nf = s_f[tid - d]; }
        __syncthreads();
        if (!f) box_merge(b, nb);
        f |= nf;
        for (int c = 0; c < 6; c++) s_box[c][tid] = b[c];
        s_f[tid] = f;
        __syncthreads();
    }
    for (int c = 0; c < 6; c++) agg[c] = s_box[c][kT - 1];
    agg_f = s_f[kT - 1];
    __syncthreads();                                        // (the caller may write s_box again)
    if (!f) box_merge(b, carry);
}

// list y of the six: axis = y % 3, backward = y / 3.  A backward list is the forward one read from its end (logical index q <-> position n - 1 - q).
struct SegArgs {
    const float* box; const uint32_t* ord; const uint32_t* node;
    float* agg; float* carry;       // [6][nt][7]: box, start flag
    float* area;                    // [6][n]
    uint32_t n, nt;
};

__device__ inline void seg_load(const SegArgs& a, uint32_t y, uint32_t q, float (&b)[6], uint32_t& f) {
    box_identity(b);
    f = 0;
    if (q >= a.n) return;
    const uint32_t axis = y % 3u, back = y / 3u;
    const uint32_t p = back ? a.n - 1 - q : q;
    const uint32_t i = a.ord[(size_t)axis * a.n + p];
    for (int c = 0; c < 6; c++) b[c] = a.box[(size_t)c * a.n + i];
    if (q == 0) f = 1;
    else f = a.node[p] != a.node[back ? p + 1 : p - 1];
}

__global__ void __launch_bounds__(kT) k_seg_reduce(const SegArgs a) {
    __shared__ float s_box[6][kT];
    __shared__ uint32_t s_f[kT];
    const uint32_t y = blockIdx.y, t = blockIdx.x;
    float b[6], carry[6], agg[6]; uint32_t f, agg_f;
    seg_load(a, y, t * kT + threadIdx.x, b, f);
    box_identity(carry);
    block_seg_scan(b, f, carry, s_box, s_f, agg, agg_f);
    if (threadIdx.x == 0) {
        float* o = a.agg + ((size_t)y * a.nt + t) * 7;
        for (int c = 0; c < 6; c++) o[c] = agg[c];
        o[6] = __uint_as_float(agg_f);
    }
}

__global__ void __launch_bounds__(kT) k_seg_carry(const SegArgs a) {
    __shared__ float s_box[6][kT];
    __shared__ uint32_t s_f[kT];
    const uint32_t y = blockIdx.x, tid = threadIdx.x;
    float running[6];
    box_identity(running);
    for (uint32_t c0 = 0; c0 < a.nt; c0 += kT) {           // (uniform)
        const uint32_t t = c0 + tid;
        float b[6], agg[6]; uint32_t f = 0, agg_f;
        box_identity(b);
        if (t < a.nt) {
            const float* in = a.agg + ((size_t)y * a.nt + t) * 7;
            for (int c = 0; c < 6; c++) b[c] = in[c];
            f = __float_as_uint(in[6]);
        }
        block_seg_scan(b, f, running, s_box, s_f, agg, agg_f);
        for (int c = 0; c < 6; c++) s_box[c][tid] = b[c];  // inclusive, the carry merged: tile t + 1 starts from it
        __syncthreads();
        if (t < a.nt) {
            float* o = a.carry + ((size_t)y * a.nt + t) * 7;
            for (int c = 0; c < 6; c++) o[c] = tid == 0 ? running[c] : s_box[c][tid - 1];
        }
        for (int c = 0; c < 6; c++) running[c] = s_box[c][kT - 1];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kT) k_seg_apply(const SegArgs a) {
    __shared__ float s_box[6][kT];
    __shared__ uint32_t s_f[kT];
    const uint32_t y = blockIdx.y, t = blockIdx.x, q = t * kT + threadIdx.x;
    float b[6], carry[6], agg[6]; uint32_t f, agg_f;
    seg_load(a, y, q, b, f);
    const float* cin = a.carry + ((size_t)y * a.nt + t) * 7;
    for (int c = 0; c < 6; c++) carry[c] = cin[c];
    block_seg_scan(b, f, carry, s_box, s_f, agg, agg_f);
    if (q < a.n) {
        const uint32_t p = (y / 3u) ? a.n - 1 - q : q;
        a.area[(size_t)y * a.n + p] = box_area(b);
    }
}

// ---- the cut of a node ---------------------------------------------------------------------------------------------------------------------------------
// Builder::build's bounds of the left half: m triangles, `leaves` leaf slots below the node
__device__ inline void cut_bounds(uint32_t m, uint32_t leaves, uint32_t nppl, uint32_t& lo, uint32_t& hi) {
    const unsigned long long cap = (unsigned long long)(leaves / 2) * nppl;
    const uint32_t cap_half = cap > 0xffffffffull ? 0xffffffffu : (uint32_t)cap;
    const uint32_t least = m > 1 ? 1u : 0u;
    lo = m > cap_half ? m - cap_half : 0u;
    if (lo < least) lo = least;
    const uint32_t most = m > 1 ? m - 1 : m;
    hi = cap_half < most ? cap_half : most;
}

struct LevelArgs {
    const uint32_t* ord; const uint32_t* node; const float* area;
    uint32_t* nbeg; uint32_t* nend; uint32_t* nsplit; uint32_t* waxis; uint32_t* left;
    unsigned long long* best;
    uint32_t n, leaves, nppl, level_first;     // leaves: leaf slots below a node of this level; level_first: the level's first heap index (= its node count)
};

__global__ void __launch_bounds__(kT) k_cost(const LevelArgs a) {
    __shared__ unsigned long long s_key[kT];
    __shared__ uint32_t s_node;
    const uint32_t axis = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * kT + tid;
    unsigned long long key = kNoKey;
    uint32_t idx = 0;
    if (p < a.n) {
        idx = a.node[p];
        const uint32_t b = a.nbeg[idx], e = a.nend[idx], m = e - b, cut = p - b + 1;
        uint32_t lo, hi;
        cut_bounds(m, a.leaves, a.nppl, lo, hi);
        if (cut >= (lo > 1 ? lo : 1u) && cut <= hi) {
            const float left = a.area[(size_t)axis * a.n + p];
            const float right = p + 1 < e ? a.area[(size_t)(3 + axis) * a.n + p + 1] : 0.0f;
            const float cost = left * (float)cut + right * (float)(m - cut);
            if (cost < INFINITY)                            // (a NaN never wins; costs are >= 0, so their bits order as they do, -0 taken as +0)
                key = ((unsigned long long)__float_as_uint(cost + 0.0f) << 32) | ((unsigned long long)axis << 30) | cut;
        }
    }
    if (tid == 0) s_node = idx;
    __syncthreads();
    const uint32_t first = s_node;                          // the node of the tile's first element: its lanes are reduced here, the others go on their own
    s_key[tid] = (p < a.n && idx == first) ? key : kNoKey;
    __syncthreads();
    for (uint32_t d = kT / 2; d > 0; d /= 2) {
        if (tid < d && s_key[tid + d] < s_key[tid]) s_key[tid] = s_key[tid + d];
        __syncthreads();
    }
    if (tid == 0 && blockIdx.x * kT < a.n && s_key[0] != kNoKey) atomicMin(&a.best[first], s_key[0]);
    if (p < a.n && idx != first && key != kNoKey) atomicMin(&a.best[idx], key);
}

__global__ void __launch_bounds__(kT) k_nodes(const LevelArgs a) {
    const uint32_t j = blockIdx.x * kT + threadIdx.x;
    if (j >= a.level_first) return;
    const uint32_t idx = a.level_first + j;
    const uint32_t b = a.nbeg[idx], e = a.nend[idx], m = e - b;
    uint32_t nl = 0, axis = 0;
    if (m > 0) {
        uint32_t lo, hi;
        cut_bounds(m, a.leaves, a.nppl, lo, hi);
        const unsigned long long key = a.best[idx];
        uint32_t cut = (m + 1) / 2;
        if (key != kNoKey) { axis = (uint32_t)(key >> 30) & 3u; cut = (uint32_t)key & 0x3fffffffu; }
        nl = cut < lo ? lo : cut;
        nl = nl > hi ? hi : nl;
    }
    a.waxis[idx] = axis;
    a.nsplit[idx] = b + nl;
    a.nbeg[2 * idx] = b;      a.nend[2 * idx] = b + nl;
    a.nbeg[2 * idx + 1] = b + nl; a.nend[2 * idx + 1] = e;
}

__global__ void __launch_bounds__(kT) k_mark(const LevelArgs a) {
    const uint32_t axis = blockIdx.y, p = blockIdx.x * kT + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t idx = a.node[p];
    if (a.waxis[idx] == axis) a.left[a.ord[(size_t)axis * a.n + p]] = p < a.nsplit[idx] ? 1u : 0u;
}

__global__ void __launch_bounds__(kT) k_partition(const LevelArgs a, const uint32_t* G, uint32_t* ord_out, uint32_t* node_out) {
    const uint32_t axis = blockIdx.y, p = blockIdx.x * kT + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t idx = a.node[p], b = a.nbeg[idx], split = a.nsplit[idx];
    const uint32_t i = a.ord[(size_t)axis * a.n + p];
    const uint32_t lefts = G[(size_t)axis * a.n + p] - G[(size_t)axis * a.n + b];     // left triangles of the node before p
    const uint32_t q = a.left[i] ? b + lefts : split + (p - b) - lefts;
    if (q < a.n) ord_out[(size_t)axis * a.n + q] = i;     // (always: q stays inside the node's range)
    if (axis == 0) node_out[p] = 2 * idx + (p >= split ? 1u : 0u);
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT) k_fill(const rt_triangle* in, rt_triangle* out, int32_t* old_slot, uint32_t num_tris, uint32_t slots) {
    const uint32_t s = blockIdx.x * kT + threadIdx.x;
    if (s >= num_tris) return;
    if (s >= slots) { out[s] = in[s]; old_slot[s] = (int32_t)s; return; }
    uint32_t* w = reinterpret_cast<uint32_t*>(out + s);    // sentinel_triangle(): nine +inf, everything else zero
    for (int k = 0; k < 16; k++) w[k] = k < 9 ? 0x7f800000u : 0u;
    old_slot[s] = -1;
}

__global__ void __launch_bounds__(kT) k_emit(const rt_triangle* in, rt_triangle* out, int32_t* old_slot, const uint32_t* ord, const uint32_t* node,
                                             const uint32_t* nbeg, const uint32_t* waxis, const uint32_t* src, uint32_t n, uint32_t first_leaf, uint32_t nppl) {
    const uint32_t axis = blockIdx.y, p = blockIdx.x * kT + threadIdx.x;
    if (p >= n) return;
    const uint32_t leaf = node[p];                          // a heap index of the leaf level
    if (leaf < first_leaf || leaf >= 2 * first_leaf) return;                  // (never)
    if (waxis[leaf / 2] != axis) return;
    const uint32_t k = p - nbeg[leaf];
    if (k >= nppl) return;                                                    // (never: the cuts keep every leaf within nppl)
    const size_t s = (size_t)(leaf - first_leaf) * nppl + k;
    const uint32_t from = src[ord[(size_t)axis * n + p]];
    const uint4* i4 = reinterpret_cast<const uint4*>(in + from);
    uint4* o4 = reinterpret_cast<uint4*>(out + s);
    for (int c = 0; c < 4; c++) o4[c] = i4[c];
    old_slot[s] = (int32_t)from;
}

__global__ void __launch_bounds__(kT) k_leaf_bytes(const uint32_t* nbeg, const uint32_t* nend, uint32_t first_leaf, uint32_t* leaf_ofs) {
    const uint32_t w = blockIdx.x * kT + threadIdx.x;
    if (w >= (first_leaf + 3) / 4) return;
    uint32_t word = 0;
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t leaf = 4 * w + k;
        if (leaf < first_leaf) word |= ((nend[first_leaf + leaf] - nbeg[first_leaf + leaf]) & 255u) << (8 * k);
    }
    leaf_ofs[w] = word;
}

}  // namespace

size_t rt_build_workspace_words(uint32_t n, uint32_t first_leaf) {
    Work w;
    return carve(w, nullptr, n, first_leaf);
}

hipError_t rt_launch_rebuild(const RtBuildParams& p, hipStream_t stream) {
    Work w;
    carve(w, p.work, p.n, p.first_leaf);
    const uint32_t n = p.n, nt = w.nt, nl = p.first_leaf;
    const uint32_t leaf_tiles = tiles_of(nl);
#define RT_BUILD_LAUNCH(kernel, grid, ...)                                              \
    do {                                                                                \
        hipLaunchKernelGGL(kernel, grid, dim3(kT), 0, stream, __VA_ARGS__);             \
        const hipError_t e_ = hipGetLastError();                                        \
        if (e_ != hipSuccess) return e_;                                                \
    } while (0)
    auto scan = [&](const ScanArgs& a, uint32_t lists) -> hipError_t {
        const uint32_t tiles = tiles_of(a.len);
        RT_BUILD_LAUNCH(k_scan_reduce, dim3(tiles, lists), a);
        RT_BUILD_LAUNCH(k_scan_carry, dim3(lists), a.agg, a.agg_stride, tiles);
        RT_BUILD_LAUNCH(k_scan_apply, dim3(tiles, lists), a);
        return hipSuccess;
    };
    hipError_t e = hipMemsetAsync(w.best, 0xff, (size_t)nl * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;

    // gather
    RT_BUILD_LAUNCH(k_leaf_count, dim3(leaf_tiles), p.slots_in, nl, p.nppl, w.cnt);
    {
        const ScanArgs a = { w.cnt, 0, nullptr, 0, w.base, 0, w.agg, w.agg_stride, nl };
        if ((e = scan(a, 1)) != hipSuccess) return e;
    }
    uint32_t* key[2] = { w.key, w.key + 3 * (size_t)(n ? n : 1) };
    uint32_t* ord[2] = { w.ord, w.ord + 3 * (size_t)(n ? n : 1) };
    uint32_t* node[2] = { w.node, w.node + (size_t)(n ? n : 1) };
    RT_BUILD_LAUNCH(k_gather, dim3(leaf_tiles), p.slots_in, nl, p.nppl, n, w.cnt, w.base, w.src, w.box, key[0], ord[0], node[0]);
    RT_BUILD_LAUNCH(k_root, dim3(1), n, w.nbeg, w.nend);

    // sort: four stable passes, ending in buffer 0
    int cur = 0;
    for (uint32_t shift = 0; shift < 32; shift += 8) {
        RT_BUILD_LAUNCH(k_radix_hist, dim3(nt, 3), key[cur], n, shift, w.hist, w.hist_len, nt);
        const ScanArgs a = { w.hist, w.hist_len, nullptr, 0, w.hist, w.hist_len, w.agg, w.agg_stride, w.hist_len };
        if ((e = scan(a, 3)) != hipSuccess) return e;
        RT_BUILD_LAUNCH(k_radix_scatter, dim3(nt, 3), key[cur], ord[cur], key[cur ^ 1], ord[cur ^ 1], n, shift, w.hist, w.hist_len, nt);
        cur ^= 1;
    }

    // the levels
    int ncur = 0;
    for (uint32_t level_first = 1; level_first < nl; level_first *= 2) {
        const SegArgs s = { w.box, ord[cur], node[ncur], w.segagg, w.segcarry, w.area, n, nt };
        RT_BUILD_LAUNCH(k_seg_reduce, dim3(nt, 6), s);
        RT_BUILD_LAUNCH(k_seg_carry, dim3(6), s);
        RT_BUILD_LAUNCH(k_seg_apply, dim3(nt, 6), s);
        const LevelArgs a = { ord[cur], node[ncur], w.area, w.nbeg, w.nend, w.nsplit, w.waxis, w.left, w.best, n, nl / level_first, p.nppl, level_first };
        RT_BUILD_LAUNCH(k_cost, dim3(nt, 3), a);
        RT_BUILD_LAUNCH(k_nodes, dim3(tiles_of(level_first)), a);
        RT_BUILD_LAUNCH(k_mark, dim3(nt, 3), a);
        const ScanArgs g = { w.left, 0, ord[cur], n, w.G, n, w.agg, w.agg_stride, n };
        if ((e = scan(g, 3)) != hipSuccess) return e;
        RT_BUILD_LAUNCH(k_partition, dim3(nt, 3), a, w.G, ord[cur ^ 1], node[ncur ^ 1]);
        cur ^= 1; ncur ^= 1;
    }

    // emit
    RT_BUILD_LAUNCH(k_fill, dim3(tiles_of(p.num_tris)), p.slots_in, p.slots_out, p.old_slot, p.num_tris, nl * p.nppl);
    RT_BUILD_LAUNCH(k_emit, dim3(nt, 3), p.slots_in, p.slots_out, p.old_slot, ord[cur], node[ncur], w.nbeg, w.waxis, w.src, n, nl, p.nppl);
    if (p.leaf_ofs) RT_BUILD_LAUNCH(k_leaf_bytes, dim3(tiles_of((nl + 3) / 4)), w.nbeg, w.nend, nl, p.leaf_ofs);
#undef RT_BUILD_LAUNCH
    return hipSuccess;
}
