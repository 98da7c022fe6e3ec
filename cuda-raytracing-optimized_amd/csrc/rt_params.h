// rt_params.h — kernel argument blocks and the launch entry points each kernel TU exports.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <optional>
#include <string>

#include "../../include/rt_types.h"
#include "../../include/rt_api.h"

// Row partition of the image over devices / processes: the image is cut into
// stripes of `stripe_rows` rows; stripe k belongs to part (k % world).  A device renders its
// stripes into a COMPACT buffer of `local_rows` rows; local row lr maps to global row
//   j = ((lr / stripe_rows) * world + rank) * stripe_rows + lr % stripe_rows.
// Pixel seeds always use the GLOBAL pixel id, so the assembled image does not depend on the partition.
// Spheres per group of the sphere kernel (slots [g * kSphereGroup, (g + 1) * kSphereGroup) share one bounding box); 16 or 32.
// Measured on C2: a ray enters ~1.1 group boxes whatever their size (8: 1.34, 16: 1.32, 32: 1.19 for primary rays), so the
// sphere tests per ray grow with the group while the box tests shrink: 16 -> 5100 Msamples/s, 32 -> 4950.
constexpr int kSphereGroupShift = 4;
constexpr int kSphereGroup = 1 << kSphereGroupShift;
constexpr int kCellCount = 64;                          // cells per axis of the group boxes' cell tables (RtSphereParams::cell_on)
constexpr int kCellWordsMax = 8;                        // the tables hold one bit per group in up to 8 words per cell: scenes of up to 256 groups (4096 spheres)
// Words per cell for a scene of n_groups groups (0 = no tables: too many groups).  The tables - 6 x kCellCount x words words = rt_cell_f4 float4 - lie behind
// the 3 x n_groups box entries of RtSphereParams::groups and are staged into the LDS with them; host and kernels size them with this one function.
__host__ __device__ inline int rt_cell_words(int n_groups) { const int w = (n_groups + 31) / 32; return w <= kCellWordsMax ? w : 0; }
// float4 entries of the tables: 3 axes x 2 kinds (begins / ends) x kCellCount cells x words
__host__ __device__ inline int rt_cell_f4(int n_groups) { return (6 * kCellCount * rt_cell_words(n_groups)) / 4; }

struct RtPartition {
    int32_t stripe_rows;
    int32_t rank;
    int32_t world;
    int32_t local_rows;
};

struct RtCounters {             // device-side, optional
    unsigned long long rays;
    unsigned long long prim_tests;
    unsigned long long node_visits;
    unsigned long long shadow_rays;
    unsigned long long exec_tests;   // sphere tests actually executed per lane in the lane-parallel scan (after group culling)
    unsigned long long box_tests;    // sphere scenes: group / node box slab tests executed
    unsigned long long ref_stats[RT_STAT_COUNT];   // the reference's STATS counters, kernels.cu:47-67
};

struct RtSphereParams {
    rt_camera cam;
    int32_t nx, ny, ns, max_depth;
    int32_t n;                  // spheres
    int32_t n_padded;           // slots: multiple of 64; slots are grouped 16 by 16 (pad slots can never be hit)
    int32_t n_groups;           // n_padded / 16
    int32_t n_big_groups;       // groups [0, n_big_groups) hold the big spheres: always scanned
    int32_t n_big;              // real big spheres: slots [0, n_big)
    const float4* spheres;      // the kernel's sphere image: slot k at index k + k/16 (one pad entry per group of 16: LDS banks), (cx, cy, cz, radius*radius);
                                // n_padded + n_groups entries, spatially sorted (see rt_scene_layout.h layout_spheres)
    const float*  rad;          // n_padded: radius of slot k (the hit normal divides by it, intersections.h:95)
    int32_t fb_global_rows;     // 1 = `fb` is the WHOLE image (the pinned host framebuffer, written over the bus as pixels finish): rows are global, not local
    const struct RtSphereParams* self;   // a device copy of this struct (launcher): the kernel re-reads what it needs once per sample / pixel from it
    int32_t basic_materials;    // 1 = every material is RT_DIFFUSE, RT_METAL or RT_GLASS (no look preset): the lean shading instantiation may run (material_scatter<BASIC>)
    int32_t global_scene;       // 1 = the scene does not fit the LDS: the kernels read these arrays from global memory (L2) instead of staging them
    const float4* groups;       // 3 x n_groups: the tight AABB of each group, one entry per axis (lo, hi, lo, -), then the rt_cell_f4(n_groups) entries of the cell
                                // tables (below).  The boxes are not inflated: the culling is exact through the per-ray margin of make_box_ray
    // per-ray culling margin (exactness of the culling for ANY ray origin, see make_box_ray): centre and radius of the
    // small spheres' centres, k1 = K eps / (2 r_min), k2 = sqrt(K eps), k3 = slab-test rounding per unit of coordinate,
    // coord_max = largest |coordinate| of any group box
    float cull_cx, cull_cy, cull_cz, cull_radius, cull_k1, cull_k2, cull_k3, cull_coord_max;
    float box_shared_lo, box_shared_hi;   // that extent
    int32_t box_shared_axis;    // 1 + axis on which every (non-empty) group box has the same extent (spheres resting on a plane), 0 = none: see group_needs
    float pair_k0;              // 2 * kPairSlack * (largest radius of the grouped spheres)^2: see the pair rounds of scan_pairs
    // Cell tables of the group boxes (scenes of up to 32 x kCellWordsMax groups; see group_needs_cells): behind the 3 x n_groups box entries of `groups` lie, for
    // each of the three axes, kCellCount cells over the boxes' extent on that axis and per cell two sets of rt_cell_words(n_groups) words each (bit g of word
    // g / 32 = small group g): the boxes that begin at or below the cell, the boxes that end at or above it.  Index: (((2 axis + kind) kCellCount + cell) words
    // + word.  cell = x * cell_scale[axis] + cell_off[axis].  cell_axes: bit a = axis a's table can reject something (not every box has the same extent there:
    // spheres resting on a horizontal plane leave bit 1 clear).  ubox: the union of the group boxes (lo.xyz, hi.xyz) the ray is clipped to first.
    int32_t cell_on;
    int32_t cell_axes;
    float cell_scale[3], cell_off[3];
    float ubox[6];
    const float4* mat_color;    // n_padded x (r, g, b, param)
    const int32_t* mat_type;    // n_padded
    const int32_t* orig;        // n_padded: caller's sphere index of the slot, INT_MAX for pad slots
    const int32_t* slot_of;     // n: slot of the caller's sphere index
    rt_vec3* fb;                // compact framebuffer: local_rows x nx
    RtPartition part;
    int32_t sky;
    int32_t rr;
    int32_t rng_mode;
    float   t_min;
    RtCounters* counters;       // nullptr = off
    uint32_t* queue;            // one zero-initialised word: next unassigned pixel (persistent-wave kernels)
    unsigned long long* wave_dbg;   // nullptr, or 8 x u64 per wave: diagnostic time stamps (RT_WAVE_DEBUG)
    uint32_t* order;            // 3 * padded pixel count words: work-order lists built by the classify pre-pass
    int32_t spw;                // samples per work item (= ns in the reference-stream mode: one item per pixel)
    int32_t chunks;             // work items per pixel = ceil(ns / spw)
    rt_vec3* partial;           // chunks > 1: local_rows * nx * chunks un-normalised partial sums
    // two-phase rendering of the reference-stream mode (see rt_kernels_spheres.hip, "cost-ordered second phase"):
    int32_t phase;              // 0 = single launch; 1 = first samples [0, s_split) -> per-pixel state; 2 = resume [s_split, ns)
    int32_t s_split;            // samples rendered by phase 1
    int32_t chain_top_thr;      // 16 x rays per sample from which a pixel goes to chain list 0 (the longest chains; see kChainClasses)
    int32_t poison_fb;          // 1 = `fb` is the host framebuffer (fb_global_rows) and this frame must start from NaN in the rows of this partition member: the
                                // frame's first dispatch (which stores no pixel) fills them, or a small kernel in front of a single dispatch (poison_rows)
    float4* px_state;           // local_rows * nx: (col.xyz, rng bits) after phase 1
    uint32_t* px_rays;          // local_rows * nx: rays traced by phase 1
    float4* ord_state;          // the same two, copied by the ordering pass into QUEUE order (index = position in `order`): a lane that fetches a pixel in phase 2
    uint32_t* ord_rays;         // reads its list entry, state and ray count with three independent loads (by pixel they hang behind the list entry: one more round trip)
    // Traffic forms of the two-dispatch frame (round 4, NS-2; sphere launcher only - the mesh launcher leaves all three at 0):
    float4* ord_rec;            // != nullptr: the ordering pass writes ONE 32-byte record per queue position instead of the three arrays above - (col.xyz, rng bits |
                                // row << 16 | column, rays, 0, 0) at ord_rec[2 pos], [2 pos + 1]: one sector per pixel written and read, not three.  (Measured and dropped:
                                // 24-byte records as three 8-byte pieces - 8 MB less per frame, the frame 4 % slower.)
    int32_t xcd_queues;         // 8: one set of cost lists and queue counters per XCD (P.queue + 64 x, kXcdQueueWords); a pixel belongs to the XCD
                                // rt_xcd_of_pixel(local row, nx, column) - a hash of (local row * nx + column) >> 5 -, so the 32 pixels of three adjacent 128-byte framebuffer lines are finished by waves behind ONE
                                // L2, which merges their 12-byte stores into whole lines (`fb` in device memory).  0 / 1: one queue for the machine
    int32_t p1_tile_major;      // 1: the first dispatch hands out its two-sample items in tile-major order (a wave parks the pixels of two adjacent 8x8 tiles: its 16-byte
                                // states fill whole lines) instead of scattered
    // Progressive rendering (runRendererProgressive, rt_api.h): a pass adds samples [acc_first, ns) to every pixel.  acc_state / acc_rays (local_rows * nx,
    // nullptr = not a progressive pass) hold (col.xyz, rng bits) and the rays traced since sample 0 of every pixel, written by the PHASE 0 and PHASE 2 kernels
    // when a pixel is finished.  acc_first > 0: the pass continues them - PHASE 0 loads the parked state at fetch instead of starting the pixel; the
    // two-dispatch frame skips its first dispatch and orders the pixels by acc_rays over acc_first samples (plan_spheres).
    float4* acc_state;
    uint32_t* acc_rays;
    int32_t acc_first;
    // The cost map (runRenderer, reference stream in whole pixels; nullptr = none): local_rows * nx ray totals of the last frame that recorded them.  A frame
    // records through acc_rays (with acc_state null and acc_first 0: the PHASE 0 and PHASE 2 kernels store a finished pixel's rays there, and nothing else);
    // a frame handed a valid map - cost_samples > 0: the samples per pixel of the frame that recorded it - is ordered by cost_rays and runs as ONE
    // cost-ordered dispatch, without the measuring first dispatch (plan_spheres: OrderedSingle).  Only a hint: the result does not depend on the work order.
    uint32_t* cost_rays;
    int32_t cost_samples;
};
constexpr int kXcdQueueWords = 64;      // words per queue block: [0] general counter [1] chain counter [2] middle-tier counter [3] first position of this XCD's lists in
                                        // `order` [4 .. 4 + 18) list lengths [22 .. 22 + 18) fill cursors
constexpr int kXcdQueues = 8;
// (the unit index hashed, not its low bits: an image 256 k pixels wide - 3840 - would give every XCD the same columns of every row)
__host__ __device__ inline uint32_t rt_xcd_of_pixel(uint32_t local_row, uint32_t nx, uint32_t column) {
#ifdef RT_XCD_PLAIN
    return ((local_row * nx + column) >> 5) & 7u;
#else
    return ((((local_row * nx + column) >> 5) * 2654435761u) >> 29) & 7u;
#endif
}

struct RtMeshParams {
    rt_camera cam;
    int32_t nx, ny, ns, max_depth;
    const rt_triangle* tris;
    const float4* bvh4;         // heap-indexed nodes viewed as float4 texels: child pair of node i at texels 3i..3i+2
    const float* bvh_axis;      // the same child pairs, one 96-byte record per internal node i, grouped by AXIS: for a in x,y,z the eight floats
                                // {min_L, min_R, max_L, max_R | max_L, max_R, min_L, min_R} (L = node 2i, R = node 2i+1): a ray reads one float4 per
                                // axis, the first (1/dir >= 0) or the second (1/dir < 0), and gets (near_L, near_R, far_L, far_R) - the swap of
                                // intersections.h:30 done by the address (default kernel only)
    const float4* leaf_tri;     // compact leaf records for the pair rounds of the default kernel: per triangle SLOT (leaf x nppl + k) 3 float4 = (v0.xyz, e1.x | e1.yz, e2.xy |
                                // e2.z, -, -, -) with e1 = v1 - v0, e2 = v2 - v0 rounded as intersections.h:56-57 rounds them; sentinel slots are zero and never read;
                                // nullptr = not built (a leaf with a real triangle behind a sentinel)
    const uint32_t* leaf_ofs;   // number of real triangles of every leaf, one BYTE per leaf (packed four to a word; staged into the LDS by the kernel)
    uint32_t first_leaf;
    uint32_t nppl;
    int32_t leaf_sentinels_trailing;   // host-checked: no real triangle behind a sentinel in any leaf (pair rounds allowed)
    int32_t lean_ok;            // host-checked: every material is RT_DIFFUSE / RT_METAL / RT_GLASS and untextured (the lean instantiation may run)
    rt_bbox bounds;
    const rt_material* materials;
    const float* const* tex_data;
    const int32_t* tex_width;
    const int32_t* tex_height;
    rt_vec3* fb;
    RtPartition part;
    int32_t sky;
    int32_t nee;
    int32_t rr;
    int32_t rng_mode;
    float   t_min;
    rt_sphere light;
    rt_vec3 lightColor;
    int32_t floor_on;           // rt_render_options.floor: rays that miss the mesh are tested against `floor` (kernels.cu:341-345 re-enabled)
    rt_plane floor;             // kernel_scene.floor
    RtCounters* counters;
    uint32_t* queue;
    unsigned long long* dbg;    // diagnostics (RT_WAVE_DEBUG): 16 phase counters summed over all waves, or nullptr
    // cost-ordered frame in two dispatches (reference RNG stream; rt_launch_mesh_*): the first renders samples [0, s_split) of every pixel and parks (colour sum,
    // stream position) and the rays it took; rt_order_pixels_by_cost sorts the pixels by that cost into queue order; the second resumes them longest first
    int32_t s_split;
    float4* px_state;           // local_rows * nx
    uint32_t* px_rays;          // local_rows * nx
    uint32_t* order;            // queue position -> (local row << 16 | column)
    float4* ord_state;          // the parked state in queue order
    uint32_t* ord_rays;
    // the traffic forms of the two-dispatch frame, as in RtSphereParams (ord_rec, xcd_queues; p1_segments = its p1_tile_major == 2)
    float4* ord_rec;
    int32_t xcd_queues;
    int32_t p1_segments;
    // Progressive rendering, as in RtSphereParams: (col.xyz, rng bits) of every pixel after the samples so far (written by PHASE 0 and PHASE 2 when a pixel
    // is finished; nullptr = not a progressive pass); acc_first > 0: PHASE 0 resumes them at sample acc_first (a continuation takes no two-dispatch frame)
    float4* acc_state;
    int32_t acc_first;
};

// A bit-field of a packed kernel argument (the sphere kernel's cfg / chain_cfg / caps, the mesh kernel's leaf_thr / min_traversing: rt_mesh_plan.h): the
// launcher packs it with put, the kernel reads it with get, both by the field's name.
struct BitField {
    int shift, mask;
    constexpr int put(int value) const { return value << shift; }            // (the launcher has checked the range)
    constexpr int get(int word) const { return (word >> shift) & mask; }
};

// A field of a render kernel's parameter block (its first argument: offset 0 of the kernarg segment), loaded where it is used.  The base is opaque to the
// optimiser, so it cannot hoist the load to the kernel's head and hold the value in SGPRs for the life of the wave: the progressive-pass fields are read
// once per pixel, and held they cost the persistent kernels SGPR and VGPR spills (the six-wave kernel 6 -> 17 spilled VGPRs).
template <typename T>
__device__ __forceinline__ T rt_cold_arg(size_t offset) {
    unsigned long long base = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(base));
    return *reinterpret_cast<const __attribute__((address_space(4))) T*>(base + offset);
}

// LDS the sphere kernel needs for a scene of n spheres (n_padded slots).
size_t rt_sphere_kernel_lds_bytes(int n_padded, int n);
// The ordering pass of the two-dispatch frames (rt_kernels_spheres.hip, k_order_by_cost; also used by the mesh launcher): reads px_rays / px_state / s_split /
// chain_top_thr / nx / part.local_rows of `q`, writes order / ord_state / ord_rays (all valid pixels, descending cost class, scattered inside a class) and the
// list lengths into q.queue[4..]; q.queue must have been zeroed on `stream` before.  q.s_split == 0: the cost is the last frame's map (q.cost_rays over
// q.cost_samples samples) and every record written is a fresh pixel - no colour, the pixel's seed, no rays - for a PHASE 2 that starts at sample 0.
hipError_t rt_order_pixels_by_cost(const RtSphereParams& q, hipStream_t stream);

// RT_TUNE as given: its text (for the error message) and its first n comma-separated fields; the sphere launcher puts them over its defaults and validates.
struct RtTune {
    std::string text;
    int n = 0;
    int v[9] = {};
};

// The library's environment switches (A/B measurements and diagnostics), host only.  rt_read_switches() (rt_renderer.hip) is the one
// reader: render_frame (a frame of runRenderer, a pass of runRendererProgressive) reads them once at its start and hands that copy to the launchers, so a
// switch holds for a whole frame or pass and a change takes effect from the next one; initRendererSpheres, setExternalFramebuffer and cleanupRenderer read the fields they use the same way.  The initialisers are the
// defaults (DESIGN.md names the measurement behind each); the reader applies the clamps.
struct RtSwitches {
    // the two-dispatch frames of both kernels
    bool xcd_queues = true;             // RT_XCD_QUEUES=0: one set of cost lists and queue counters for the machine instead of one per XCD
    bool ord_packed = true;             // RT_ORD_PACKED=0: the parked state in three arrays instead of one 32-byte record per queue position
    int p1_tile = 2;                    // RT_P1_TILE: first dispatch 0 scattered, 1 tile-major (spheres only), 2 scattered row segments (out of 0..2: 0)
    std::optional<std::string> wave_debug;      // RT_WAVE_DEBUG=<file>: the diagnostic instantiation, per-wave time stamps / phase counters -> file
    // the renderer
    bool fb_direct = false;             // RT_FB_DIRECT: sphere scenes deliver finished pixels straight into the pinned host framebuffer
    bool fb_poison = true;              // RT_FB_POISON=0: ... without NaN-poisoning it first
    bool box_cells = true;              // RT_BOX_CELLS=0: no cell-table prefilter (initRendererSpheres)
    bool compact_leaves = true;         // RT_COMPACT_LEAVES=0: the mesh leaf tests read the caller's triangles
    bool ext_fb_no_register = false;    // RT_EXT_FB_NO_REGISTER=1: setExternalFramebuffer takes its cannot-page-lock fallback
    bool cleanup_device_reset = false;  // RT_CLEANUP_DEVICE_RESET=1: cleanupRenderer ends with hipDeviceReset
    int cost_reuse = 1;                 // RT_COST_REUSE: sphere frames 0 = neither record nor reuse the per-pixel cost map (every frame measures), 1 = reuse it until
                                        // setCamera changes the camera, 2 = across setCamera too (A/B: tools/bench_orbit.py)
    int pixels_waves = 0;               // RT_PIXELS_WAVES=<w>: renderPixels and radianceRays launch at most w waves (0 = no cap; tests: the refill path with a few hundred entries)
    bool refine_order = true;           // RT_REFINE_ORDER=0: refineFrame hands its list to the pixel kernels in ascending pixel order, not dearest first (A/B: tools/bench_refine.py)
    // the sphere launcher
    int top_thr = 384;                 // RT_TOP_THR: 16 x rays per sample from which a pixel goes to chain list 0 (24; below 320: the default)
    bool basic = true;                  // RT_BASIC=0 / RT_ONEPASS=0: keep the general shading code / pass loop where the lean kinds would do
    bool onepass = true;
    long long lean6_pixels = 2600000;   // RT_LEAN6_PIXELS: pixels per device from which the lean kernel runs six waves per SIMD (0 = never)
    bool hybrid_two = false;            // RT_HYBRID_TWO=1: the cost-ordered two dispatches for the hybrid copy too
    int mid_waves = 0, mid_cap = 16;    // RT_MID=waves,pixels: the middle tier (k_render_spheres_queue, role 1; 0 waves = off); the launcher validates
    bool chain_single = true;           // RT_CHAIN_SINGLE=0: chain waves grab more than one pixel at a time
    bool single_ray = true;             // RT_SINGLE_RAY=0: no scan_single for waves with one live ray
    int pool = 4;                       // RT_POOL: queue positions a normal wave reserves per grab (second dispatch)
    bool wave_debug_light = false;      // RT_WAVE_DEBUG_LIGHT=1: time stamps only (the production kernel of the benchmark scene)
    bool wave_debug_phase = false;      // RT_WAVE_DEBUG_PHASE=1: the time line of the first dispatch instead of the second
    std::optional<RtTune> tune;         // RT_TUNE: the chain tier's scheduling constants (experiments)
    // the mesh launcher
    bool mesh_lean = true;              // RT_MESH_LEAN=0: keep the general kernel
    bool mesh_tile_order = false;       // RT_MESH_ORDER=t: tile-major pixel order (stride 1)
    bool mesh_two = true;               // RT_MESH_TWO=0: the single scattered dispatch
    int mesh_split = 2;                 // RT_MESH_SPLIT: samples of the first dispatch (at least 1; 1: 903, 2: 911, 4: 893, 8: 866 Msamples/s on C4,
                                        // profiles/r04_ab_mesh_two_b.txt)
    int mesh_heavy = 5;                 // RT_MESH_HEAVY: PHASE 2: cost classes counted as expensive (>= 1.6 x the mean pixel) and spread over the first fills
                                        // (0 = off) ...
    int mesh_rounds = 2;                // RT_MESH_ROUNDS: ... of this many times the lanes in flight.  C4, A/B in one call (profiles/r04_sweep_mesh_spread*.txt):
                                        // lists as they lie 907, 5 classes over 1 / 2 / 3 / 5 fills 972 / 937-987 / 954 / 938, 4 classes 969 / 967, 6 classes
                                        // 903 / 945, 7 classes 905-919 Msamples/s
    bool mesh_rev = false;              // RT_MESH_REV=1: cheapest pixels first (experiment)
    int mesh_chain_thr = 448;           // RT_MESH_CHAIN_THR: PHASE 2: list 0 = pixels from 16 x this many cost units per sample (the mean pixel of C4 has ~100):
                                        // the chains, see "Chain waves" (at least 17)
    int mesh_chain_lanes = 6;           // RT_MESH_CHAIN_LANES: pixels of list 0 per chain wave (0 = no chain waves; at most 64)
    int mesh_chain_frac = 8;            // RT_MESH_CHAIN_FRAC: chain waves only while list 0 is below pixels >> this (& 0xF; tests: 0)
    std::optional<std::string> mesh_diag_file;  // RT_MESH_DIAG_FILE=<file>: per-pixel items of the second dispatch (RT_MESH_TAIL_DIAG builds only)
};
RtSwitches rt_read_switches();

// The golden-ratio stride of n items: ~0.618 n, coprime with n, so that i -> i * stride mod n scatters neighbouring items over different waves.
inline uint32_t rt_coprime_stride(unsigned long long n) {
    auto gcd = [](unsigned long long a, unsigned long long b) { while (b) { const unsigned long long t = a % b; a = b; b = t; } return a; };
    unsigned long long cand = (unsigned long long)((double)n * 0.6180339887) | 1ull;
    while (gcd(cand, n) != 1ull) cand += 2;
    return (uint32_t)(cand % n);
}

// Each returns the hipError_t of the launch.  `variant` selects a kernel variant (0 = default); `sw`: the frame's switches.
// Sphere launchers: p.self must point to a device copy of `p` that is complete on `stream` before the launch (the renderer owns it).
hipError_t rt_launch_spheres_parity(const RtSphereParams& p, int variant, const RtSwitches& sw, hipStream_t stream);
hipError_t rt_launch_spheres_fast(const RtSphereParams& p, int variant, const RtSwitches& sw, hipStream_t stream);
hipError_t rt_launch_mesh_parity(const RtMeshParams& p, int variant, const RtSwitches& sw, hipStream_t stream);
hipError_t rt_launch_mesh_fast(const RtMeshParams& p, int variant, const RtSwitches& sw, hipStream_t stream);
// The launch report (rtLastLaunches, rt_api.h): the launchers note every render-kernel launch with the template arguments of the instantiation they launched
// (RT_KERNEL_* family and the RT_LAUNCH_* words up to RT_LAUNCH_BLOCKS); the renderer adds the device and the fp mode of the frame.  Host bookkeeping only.
void rt_note_launch(int family, int phase, int cls, int chunked, int dbg, int scene, int lean, int threads, unsigned blocks);
// ... and the form of the cost-ordered sphere dispatch it launched (rtLastSphereForm; rt_sphere_form.h)
void rt_note_sphere_form(int form);

// First-hit guide planes (renderGuides, rt_api.h): compact device planes of part.local_rows x nx entries, nullptr = not requested.  The guide kernels
// (k_guides_spheres / k_guides_mesh) exist in the PARITY objects only - one arithmetic for both fp modes - and read of the parameter block what a
// centre ray needs: camera, image size, partition, scene arrays, t_min, sky (mesh: bounds, materials, textures, floor).
struct RtGuidePlanes {
    float* albedo;              // 3 floats per pixel
    float* normal;              // 3 floats per pixel
    float* depth;
    int32_t* prim;
    int32_t* nodes;             // mesh scenes only
};
hipError_t rt_launch_guides_spheres(const RtSphereParams& p, const RtGuidePlanes& g, hipStream_t stream);
hipError_t rt_launch_guides_mesh(const RtMeshParams& p, const RtGuidePlanes& g, hipStream_t stream);

// Batched ray queries (traceRays / occludedRays, rt_api.h): one chunk of caller's rays on the device.  org / dir hold n x 3 floats, t_min / t_max n floats or
// nullptr (= t_min_default, respectively FLT_MAX for every ray).  Output planes of n entries (normal n x 3, uv n x 2), nullptr = not stored; the closest-hit
// kernels write t / prim / normal / uv / nodes, the any-hit kernels `occluded` alone.  The ray kernels (k_rays_spheres / k_rays_mesh) exist in the PARITY
// objects only, like the guide kernels, and read of the scene's parameter block the scene arrays alone (mesh: bounds, floor): no camera, no image size, no
// partition.
struct RtRayBatch {
    const float* org;
    const float* dir;
    const float* t_min;
    const float* t_max;
    float* t;
    int32_t* prim;
    float* normal;
    float* uv;
    int32_t* nodes;             // mesh scenes only
    uint8_t* occluded;          // any-hit
    int32_t n;
    float t_min_default;        // rt_render_options.t_min
};
hipError_t rt_launch_rays_spheres(const RtSphereParams& p, const RtRayBatch& b, bool any, hipStream_t stream);
hipError_t rt_launch_rays_mesh(const RtMeshParams& p, const RtRayBatch& b, bool any, hipStream_t stream);

// A list of pixels (renderPixels, rt_api.h): one chunk of the caller's list on the device.  ij holds n x 2 words (column, row from the bottom); ns / first n
// words each or nullptr (= ns_all, respectively 0 for every entry); state n x 4 words - (colour sum bits, xorshift word), read by an entry whose first
// sample is not 0, written by every entry - or nullptr; out n x 3 floats = sum / (first + count) or nullptr; rays n words or nullptr.  queue: one zeroed
// word, the next unassigned entry.  The pixel kernels (k_pixels_spheres / k_pixels_mesh) exist in both fp objects - they are the frame's arithmetic - and
// read of the scene's parameter block the scene, the camera, the image size, max_depth and the options of a frame (sky, t_min, rr; mesh: nee, light, floor);
// nothing of its partition, framebuffer, queue, parked or progressive state.  max_waves: RT_PIXELS_WAVES, 0 = as many as stay resident.
struct RtPixelBatch {
    const int32_t* ij;
    const int32_t* ns;
    const int32_t* first;
    uint32_t* state;
    rt_vec3* out;
    uint32_t* rays;
    uint32_t* queue;
    int32_t n;
    int32_t ns_all;
};
hipError_t rt_launch_pixels_spheres_parity(const RtSphereParams& p, const RtPixelBatch& b, int max_waves, hipStream_t stream);
hipError_t rt_launch_pixels_spheres_fast(const RtSphereParams& p, const RtPixelBatch& b, int max_waves, hipStream_t stream);
hipError_t rt_launch_pixels_mesh_parity(const RtMeshParams& p, const RtPixelBatch& b, int max_waves, hipStream_t stream);
hipError_t rt_launch_pixels_mesh_fast(const RtMeshParams& p, const RtPixelBatch& b, int max_waves, hipStream_t stream);

// A list of the caller's own rays (radianceRays, rt_api.h): one chunk of the list on the device.  org / dir hold n x 3 floats (dir raw: the kernel normalises
// it once); ids n words - the seed id of each ray - or nullptr (= id0 + the entry's index in the chunk: id0 is the chunk's first index in the caller's list);
// ns / first / state / out / rays / queue as in RtPixelBatch.  The radiance kernels (k_radiance_spheres / k_radiance_mesh) exist in both fp objects and read
// of the scene's parameter block the scene, max_depth and the options of a path (sky, t_min, rr; mesh: nee, light, floor): no camera, no image size, no
// partition.  max_waves: RT_PIXELS_WAVES, 0 = as many as stay resident.
struct RtRadianceBatch {
    const float* org;
    const float* dir;
    const uint32_t* ids;
    const int32_t* ns;
    const int32_t* first;
    uint32_t* state;
    rt_vec3* out;
    uint32_t* rays;
    uint32_t* queue;
    int32_t n;
    int32_t ns_all;
    uint32_t id0;
};
hipError_t rt_launch_radiance_spheres_parity(const RtSphereParams& p, const RtRadianceBatch& b, int max_waves, hipStream_t stream);
hipError_t rt_launch_radiance_spheres_fast(const RtSphereParams& p, const RtRadianceBatch& b, int max_waves, hipStream_t stream);
hipError_t rt_launch_radiance_mesh_parity(const RtMeshParams& p, const RtRadianceBatch& b, int max_waves, hipStream_t stream);
hipError_t rt_launch_radiance_mesh_fast(const RtMeshParams& p, const RtRadianceBatch& b, int max_waves, hipStream_t stream);
