// rt_kernels_update.hip — the BVH refit behind updateTriangles (include/rt_api.h, "editing the scene"): every node box, every axis-grouped child-pair record
// and every compact leaf record of a mesh scene from the triangles as they now lie on the device.  DESIGN.md 3.17 has the decomposition and the measurements.
//
// The definition is rt_api.h's and host/rt_bvh.cpp (rtRefitBvhArrays) is its CPU twin: min'(lo, p) = p < lo ? p : lo, max'(hi, p) = p > hi ? p : hi, slots,
// vertices and axes in order, the right child compared against the left.  Only comparisons and selects, and one rounded fp32 subtraction per component of a
// leaf record's edges: this translation unit is compiled like the PARITY objects (-ffp-contract=off), once.
//
// The tree is complete and heap-indexed, so a level is a contiguous run of nodes [T, 2T) and 256 consecutive nodes of it are the leaves of a subtree of
// height 8 whose nodes are contiguous on every level above.  One kernel, two entry forms:
//   FROM_TRIS   (bottom)  a workgroup owns 256 consecutive leaves: (a) lanes stride over its 256 * nppl slots and rewrite the compact leaf records of the real
//                         ones, (b) one lane per leaf computes the leaf's box into the LDS, (c) eight levels are reduced in the LDS, a barrier between them.
//   !FROM_TRIS  (upper)   the same from 256 consecutive nodes of level [T, 2T), read back from the node array, for the next eight levels.
// Every lane that computes a node stores its 24 bytes, and for an internal node the 96-byte record of its two children, which it has just read.  A level of
// fewer than 256 nodes is a lower subtree: T < 256 gives one workgroup of T inputs and log2(T) levels, by the same code.  Nothing is shared between workgroups
// of a launch: no atomics, no flags; a pass reads what the pass before it wrote, in stream order.  Node 0 and record 0 are never touched.
// Every barrier is reached by all lanes of its workgroup (the loop bounds are uniform); the grid is exactly T / inputs workgroups, so no workgroup is idle.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_update.h"

namespace {

constexpr uint32_t kRefitThreads = 256;

__device__ __forceinline__ bool is_inf(float x) { return (__float_as_uint(x) & 0x7fffffffu) == 0x7f800000u; }
__device__ __forceinline__ float min1(float lo, float p) { return p < lo ? p : lo; }
__device__ __forceinline__ float max1(float hi, float p) { return p > hi ? p : hi; }

template <bool FROM_TRIS>
__global__ void __launch_bounds__(kRefitThreads) k_refit(const RtRefitParams P, const uint32_t T) {
    // the subtree's boxes as a local heap (root 1, inputs at [nl, 2 nl)), one plane per component (lo.xyz, hi.xyz): a lane reads its two children as one float2
    __shared__ __attribute__((aligned(8))) float s_box[6][2 * kRefitThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t nl = T < kRefitThreads ? T : kRefitThreads;  // inputs of this workgroup: a power of two, at least 2
    const uint32_t first = blockIdx.x * nl;                     // its first input, counted from T

    if (FROM_TRIS) {
        const size_t slot0 = (size_t)first * P.nppl;
        if (P.leaf_rec) {                                       // (a) (nppl <= 255 where the records exist: nl * nppl fits 32 bits)
            const uint32_t nslots = nl * P.nppl;
            for (uint32_t q = t; q < nslots; q += kRefitThreads) {
                const rt_triangle* tr = P.slots + slot0 + q;
                const float v0x = tr->v[0].e[0];
                if (is_inf(v0x)) continue;                      // a sentinel's record stays zero
                const float v0y = tr->v[0].e[1], v0z = tr->v[0].e[2];
                const float e1x = tr->v[1].e[0] - v0x, e1y = tr->v[1].e[1] - v0y, e1z = tr->v[1].e[2] - v0z;
                const float e2x = tr->v[2].e[0] - v0x, e2y = tr->v[2].e[1] - v0y, e2z = tr->v[2].e[2] - v0z;
                float4* rec = P.leaf_rec + (slot0 + q) * 3;
                rec[0] = make_float4(v0x, v0y, v0z, e1x);
                rec[1] = make_float4(e1y, e1z, e2x, e2y);
                rec[2] = make_float4(e2z, __uint_as_float((uint32_t)tr->meshID), 0.0f, 0.0f);
            }
        }
        if (t < nl) {                                           // (b)
            float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
            const rt_triangle* tr = P.slots + slot0 + (size_t)t * P.nppl;
            for (uint32_t k = 0; k < P.nppl; k++) {
                if (is_inf(tr[k].v[0].e[0])) break;
                for (int v = 0; v < 3; v++)
                    for (int a = 0; a < 3; a++) {
                        const float p = tr[k].v[v].e[a];
                        lo[a] = min1(lo[a], p);
                        hi[a] = max1(hi[a], p);
                    }
            }
            float2* node = reinterpret_cast<float2*>(P.nodes + (size_t)(T + first + t) * 6);
            node[0] = make_float2(lo[0], lo[1]);
            node[1] = make_float2(lo[2], hi[0]);
            node[2] = make_float2(hi[1], hi[2]);
            for (int a = 0; a < 3; a++) { s_box[a][nl + t] = lo[a]; s_box[3 + a][nl + t] = hi[a]; }
        }
    } else if (t < nl) {
        const float2* node = reinterpret_cast<const float2*>(P.nodes + (size_t)(T + first + t) * 6);
        const float2 n0 = node[0], n1 = node[1], n2 = node[2];
        s_box[0][nl + t] = n0.x; s_box[1][nl + t] = n0.y; s_box[2][nl + t] = n1.x;
        s_box[3][nl + t] = n1.y; s_box[4][nl + t] = n2.x; s_box[5][nl + t] = n2.y;
    }
    __syncthreads();

    const uint32_t root = (T + first) / nl;                     // the subtree's root in the tree
    for (uint32_t w = nl >> 1; w >= 1; w >>= 1) {               // (c) the local level of w nodes [w, 2w); its children are [2w, 4w)
        if (t < w) {
            const uint32_t j = w + t;
            const size_t g = (size_t)root * w + t;              // node j in the tree
            float L[6], R[6], n[6];
            for (int c = 0; c < 6; c++) {
                const float2 lr = *reinterpret_cast<const float2*>(&s_box[c][2 * j]);
                L[c] = lr.x; R[c] = lr.y;
            }
            for (int a = 0; a < 3; a++) {
                n[a] = R[a] < L[a] ? R[a] : L[a];
                n[3 + a] = R[3 + a] > L[3 + a] ? R[3 + a] : L[3 + a];
            }
            for (int c = 0; c < 6; c++) s_box[c][j] = n[c];
            float2* node = reinterpret_cast<float2*>(P.nodes + g * 6);
            node[0] = make_float2(n[0], n[1]);
            node[1] = make_float2(n[2], n[3]);
            node[2] = make_float2(n[4], n[5]);
            float4* rec = reinterpret_cast<float4*>(P.axis + g * 24);
            for (int a = 0; a < 3; a++) {                       // rt_params.h, bvh_axis: {min_L, min_R, max_L, max_R | max_L, max_R, min_L, min_R}
                rec[2 * a] = make_float4(L[a], R[a], L[3 + a], R[3 + a]);
                rec[2 * a + 1] = make_float4(L[3 + a], R[3 + a], L[a], R[a]);
            }
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t rt_launch_refit(const RtRefitParams& p, hipStream_t stream) {
    uint32_t T = p.first_leaf;
    if (T < 2 || (T & (T - 1)) != 0 || T > (1u << 30) || p.nppl == 0 || !p.slots || !p.nodes || !p.axis) return hipErrorInvalidValue;
    for (bool bottom = true; T > 1; bottom = false) {
        const uint32_t nl = T < kRefitThreads ? T : kRefitThreads;
        if (bottom) hipLaunchKernelGGL(k_refit<true>, dim3(T / nl), dim3(kRefitThreads), 0, stream, p, T);
        else hipLaunchKernelGGL(k_refit<false>, dim3(T / nl), dim3(kRefitThreads), 0, stream, p, T);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        T /= nl;
    }
    return hipSuccess;
}
