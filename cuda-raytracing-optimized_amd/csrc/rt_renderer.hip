// rt_renderer.hip — host runtime behind the C-ABI of include/rt_api.h (librt_mi355x.so).
//
// Replaces the host half of /root/reference/kernels.cu: the global RenderContext (:69-145),
// initRenderer (:571-650), runRenderer (:652-664), cleanupRenderer (:666-680) and check_cuda
// (:27-38).  Same contract: one global context, synchronous render, void returns, exit(99) on any
// runtime failure.  MI355X differences:
//   * the framebuffer handed to the caller is pinned host memory; each device renders into a compact
//     device buffer and its stripes are gathered with plain hipMemcpy2DAsync (no managed memory
//     page migration, no RCCL);
//   * the image can be split into interleaved row stripes over several devices of this process
//     (options.devices) and/or over several processes (options.part_rank/part_world);
//   * the BVH is read with plain 16-byte global loads (no texture object);
//   * the kernel is timed with HIP events on the stream it is launched on (getRenderStats).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_params.h"
#include "rt_scene_layout.h"
#include "rt_denoise.h"
#include "rt_accumulate.h"
#include "rt_preview.h"
#include "rt_motion.h"
#include "rt_display.h"
#include "rt_update.h"
#include "rt_build.h"
#include "rt_refine.h"
#include "rt_gather.h"
#include "rt_texels.h"
#include "rt_texel_filter_launch.h"
#include "rt_lightmap.h"

namespace {

#define HIP_CHECK(expr) hip_check((expr), #expr, __FILE__, __LINE__)

void hip_check(hipError_t result, const char* func, const char* file, int line) {   // kernels.cu:27-38
    if (result != hipSuccess) {
        fprintf(stderr, "HIP error = %s at %s:%d '%s' \n", hipGetErrorString(result), file, line, func);
        (void)hipDeviceReset();                                     // kernels.cu:34-35: reset before exiting
        exit(99);
    }
}

[[noreturn]] void rt_fail(const char* msg, const char* who = "") {
    fprintf(stderr, "rt error: %s%s\n", who, msg);
    exit(99);
}

// Device memory: every allocation of a DeviceState / PassState goes through dev_alloc, which notes the pointer in its owner's `owned`, and
// free_device / free_pass release what that record holds - a buffer cannot be allocated without being freed.  The record is plain data walked by those functions
// only, never by a destructor: exit(99) runs the destructors of the globals below with buffers live, and nothing of HIP may be called then; the states stay copyable.
template <typename T>
T* dev_alloc(std::vector<void*>& owned, size_t count) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, count * sizeof(T)));
    owned.push_back(p);
    return static_cast<T*>(p);
}

template <typename T>
void dev_release(std::vector<void*>& owned, T*& p) {       // one buffer, before it is allocated again with another size
    if (!p) return;
    owned.erase(std::find(owned.begin(), owned.end(), static_cast<void*>(p)));
    HIP_CHECK(hipFree(p));
    p = nullptr;
}

void dev_release_all(std::vector<void*>& owned) {
    for (void* p : owned) HIP_CHECK(hipFree(p));
    owned.clear();
}

template <typename T>
T* upload(std::vector<void*>& owned, const std::vector<T>& v) {
    if (v.empty()) return nullptr;
    T* p = dev_alloc<T>(owned, v.size());
    HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
}

struct DeviceState {
    int device = 0;
    std::vector<void*> owned;           // every device allocation of this state (dev_alloc)
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    hipEvent_t ev_upd_start = nullptr, ev_upd_stop = nullptr;   // around the refit kernels of updateTriangles (rtLastUpdateMs): a frame's and the guides' timings stay theirs
    hipEvent_t ev_reb_start = nullptr, ev_reb_stop = nullptr;   // around the build + refit kernels of rebuildBvh (rtLastRebuildMs)
    RtSphereParams* d_params = nullptr; // device copy of the sphere kernel's parameter block (RtSphereParams::self), one per DeviceState
    RtSphereParams* h_params = nullptr; // its pinned staging copy (the source of the asynchronous upload must outlive the call)
    // sphere scene
    float4* d_spheres = nullptr;
    float* d_rad = nullptr;
    float4* d_mat_color = nullptr;
    int32_t* d_mat_type = nullptr;
    float4* d_groups = nullptr;
    int32_t* d_orig = nullptr;
    int32_t* d_slot_of = nullptr;
    // mesh scene
    rt_triangle* d_tris = nullptr;
    float4* d_bvh = nullptr;
    float* d_bvh_axis = nullptr;
    float4* d_leaf_tri = nullptr;
    uint32_t* d_leaf_ofs = nullptr;
    rt_material* d_materials = nullptr;
    rt_triangle* d_tris_alt = nullptr;  // rebuildBvh: the second slot buffer (the rebuilt order is written there, then the two are swapped),
    int32_t* d_old_slot = nullptr;      // the permutation of the last rebuild and
    uint32_t* d_build_work = nullptr;   // the build's workspace of build_words words; allocated by the first rebuild on this device
    size_t build_words = 0;
    float** d_tex_data = nullptr;
    int32_t* d_tex_width = nullptr;
    int32_t* d_tex_height = nullptr;
    // output
    rt_vec3* d_fb = nullptr;
    size_t fb_rows = 0;
    RtCounters* d_counters = nullptr;
    uint32_t* d_queue = nullptr;
    unsigned long long* d_wave_dbg = nullptr;
    uint32_t* d_order = nullptr;
    rt_vec3* d_partial = nullptr;
    size_t partial_bytes = 0;
    // The parked state of the two-dispatch frames: allocated by the first frame that can take them, in the form its switches select (parked_buffers)
    float4* d_px_state = nullptr;       // two-phase rendering: per-pixel (col, rng) and rays after the first samples
    uint32_t* d_px_rays = nullptr;
    float4* d_ord_state = nullptr;      // ... and their copies in queue order (RtSphereParams::ord_state / ord_rays)
    uint32_t* d_ord_rays = nullptr;
    float4* d_ord_rec = nullptr;        // ... or as one 32-byte record per queue position (RtSphereParams::ord_rec)
    // The cost map of sphere frames (RtSphereParams::cost_rays): the rays of every local pixel in the last runRenderer frame that recorded them, allocated
    // by the first such frame.  cost_samples: that frame's samples per pixel, 0 = nothing recorded yet; cost_key: what the map depends on beside the
    // device state itself (a new init or another partition builds new device states) - see cost_key_of.
    uint32_t* d_cost_rays = nullptr;
    int cost_samples = 0;
    std::array<int, 11> cost_key = {};
    float4* d_acc_state = nullptr;      // progressive frame (runRendererProgressive): per local pixel (col, rng) after the samples so far, and (sphere scenes)
    uint32_t* d_acc_rays = nullptr;     // the rays they took; allocated by the first pass on this device
    void* d_guide[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };     // first-hit guide planes (renderGuides), plane k = bit k of the mask: allocated by the
                                        // first call that asks for the plane on this device
};

constexpr size_t kGuideBytes[5] = { 12, 12, 4, 4, 4 };      // bytes per pixel of the guide planes: albedo, normal, depth, prim, nodes

struct RenderContext {
    bool initialised = false;
    bool is_spheres = false;
    int nx = 0, ny = 0, max_depth = 0;
    rt_camera cam;
    rt_render_options opt;
    rt_vec3* h_fb = nullptr;            // pinned, nx*ny, handed to the caller
    rt_vec3* h_ext = nullptr;           // caller-owned framebuffer (setExternalFramebuffer), or null
    bool ext_registered = false;        // h_ext is page-locked and device-mapped (hipHostRegister succeeded): the kernels may store into it directly
    // The scene as the kernels read it (rt_scene_layout.h): the host copies of its arrays (so devices can be (re)configured by setRenderOptions) and its
    // constants in parameter-block form, the start of every parameter block (sphere_params / mesh_params).  One of the two is in use (is_spheres).
    SphereLayout sphere;
    MeshLayout mesh;
    std::vector<DeviceState> devs;
    rt_render_stats stats;
    int prog_samples = 0;               // samples per pixel of the progressive frame so far (rtProgressiveSamples)
    int camera_moves = 0;               // setCamera calls that changed the camera: part of a cost map's key (cost_key_of)
    int scene_edits = 0;                // updateTriangles / updateMaterials / updateSpheres calls that changed the scene: likewise
    bool refit_stale = false;           // the devices' nodes, child-pair records and leaf records are newer than mesh.bvh / bvh_axis / leaf_tri (fetch_refit)
    double update_ms = 0.0;             // rtLastUpdateMs
    double rebuild_ms = 0.0;            // rtLastRebuildMs
    double guides_ms = 0.0;             // rtLastGuidesMs
    double denoise_ms = 0.0;            // rtLastDenoiseMs
    double accumulate_ms = 0.0;         // rtLastAccumulateMs
    double preview_ms = 0.0;            // rtLastPreviewMs
    double display_ms = 0.0;            // rtLastDisplayMs
    double rays_ms = 0.0;               // rtLastRaysMs
    double pixels_ms = 0.0;             // rtLastPixelsMs
    double radiance_ms = 0.0;           // rtLastRadianceMs
    double gather_ms = 0.0;             // rtLastGatherMs
    double texels_ms = 0.0;             // rtLastTexelsMs
    double bake_ms = 0.0;               // rtLastBakeMs
    double filter_ms = 0.0;             // rtLastFilterMs
    double sample_ms = 0.0;             // rtLastSampleMs
    double lightmap_ms = 0.0;           // rtLastLightmapMs
    double motion_ms = 0.0;             // rtLastMotionMs
};

// What the whole-image preview passes (denoiseFrame, accumulateFrame, previewFrame) each hold on the device: buffers for the whole image on ONE device, the first in-process
// device, whatever rows that device renders, with guide planes and events of their own (a frame's and the guides' timings stay what they were).  A pass shares
// nothing with the other pass or with renderGuides - neither can disturb the history.  Allocated by the pass's first call (begin_pass), freed by free_pass
// (cleanupRenderer, every init*, a setRenderOptions that changes the device layout).
struct PassState {
    int device = -1;
    size_t npix = 0;
    std::vector<void*> owned;           // its device allocations (dev_alloc)
    float* d_guide[4] = { nullptr, nullptr, nullptr, nullptr };     // albedo, normal, depth, prim of the whole image, this call's camera
    rt_vec3* d_in = nullptr;
    rt_vec3* d_out = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
};

struct DenoiseState : PassState {
    float4* d_rec = nullptr;            // RtDenoiseParams::rec
    float4* d_col[2] = { nullptr, nullptr };
};

struct AccumulateState : PassState {
    float* d_history = nullptr;         // N(p) as a plane for the caller
    float4* d_rec[2] = { nullptr, nullptr };                        // the two record sets (rt_accumulate.h), 3 * npix each
    int newest = 0;                     // the set the last call wrote: the next call's history
    int frames = 0;                     // calls since the last reset (rtHistoryFrames); 0 = the next call has no history
    rt_camera prev_cam;                 // the camera of the last call
};

RenderContext g_ctx;     // kernels.cu:145: one global context per process
// previewFrame: a history of its own (the record sets of rt_preview.h with their moment planes), the a-trous pair and the two planes for the caller.
struct PreviewState : PassState {
    float* d_history = nullptr;         // N(p) as a plane for the caller
    float* d_variance = nullptr;        // var(p) of stage V as a plane for the caller
    float4* d_rec[2] = { nullptr, nullptr };                        // the two record sets, 3 * npix each
    float2* d_mom[2] = { nullptr, nullptr };                        // their luminance moments
    float4* d_col[2] = { nullptr, nullptr };                        // RtPreviewParams::col
    int newest = 0;                     // the set the last call wrote: the next call's history
    int frames = 0;                     // calls since the last reset (rtPreviewFrames); 0 = the next call has no history
    rt_camera prev_cam;                 // the camera of the last call
};

// displayFrame: no guide planes and no rt_vec3 output (begin_pass is told so): the RGBA words and the histogram with the two exposure words behind it are its own.
// E' of the auto exposure stays on the device (d_words); `adapted` says whether it holds one.  The host keeps what the helpers report.
struct DisplayState : PassState {
    uint32_t* d_rgba = nullptr;         // RtDisplayParams::out, one word per pixel
    uint32_t* d_words = nullptr;        // RtDisplayParams::hist (RT_DISPLAY_BINS words), then RtDisplayParams::state (E, E_used)
    uint32_t h_words[RT_DISPLAY_BINS + 2] = {};     // d_words after the last RT_DISPLAY_AUTO_EXPOSURE call (rtDisplayHistogram)
    bool adapted = false;               // d_words holds the E of a previous call: the next one blends
    float last_exposure = 1.0f;         // rtLastExposure
};

// What every query call (traceRays / occludedRays, renderPixels, radianceRays, refineFrame, gatherRadiance) holds: the first in-process device, its allocations there and an event pair of
// its own, created with the device list (setup_devices) - the timings of a frame, the guides, the passes and the other queries stay what they were.
// Released by free_pass where the passes' buffers are.
struct QueryState {
    int device = -1;
    std::vector<void*> owned;           // its device allocations (dev_alloc)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
};

// traceRays / occludedRays, renderPixels and radianceRays: the device buffers of one chunk of the caller's items, each grown to the largest chunk that asked for it
// (run_chunks), by a table of what a buffer holds per item and which way it crosses the bus.  Rays: four inputs, five closest-hit planes, the any-hit bytes.
// Pixels: three inputs, the stream states (read and written), two outputs - and the queue word of the pixel kernels.  Radiance rays: five inputs, then as pixels.
enum { kUp = 1, kDown = 2 };
struct ChunkBuffer {
    size_t bytes;                       // per item
    int dir;                            // kUp: uploaded in front of the launch, kDown: downloaded behind it
};
enum { kRayOrg = 0, kRayDir, kRayTMin, kRayTMax, kRayT, kRayPrim, kRayNormal, kRayUv, kRayNodes, kRayOccluded, kRayBuffers };
enum { kPixIj = 0, kPixNs, kPixFirst, kPixState, kPixOut, kPixRays, kPixBuffers };
enum { kRadOrg = 0, kRadDir, kRadIds, kRadNs, kRadFirst, kRadState, kRadOut, kRadRays, kRadBuffers };
constexpr int kChunkBuffers = kRayBuffers;
constexpr size_t kRayChunk = RT_RAY_CHUNK;      // rays per upload - kernel - download round: 65 bytes per ray, so at most ~273 MB of device memory whatever the batch
constexpr size_t kPixelChunk = RT_PIXEL_CHUNK;  // pixels per upload - kernel - download round: 48 bytes per pixel
struct ChunkState : QueryState {
    char* d_buf[kChunkBuffers] = {};
    size_t cap[kChunkBuffers] = {};     // items d_buf[k] holds
    uint32_t* d_queue = nullptr;        // RtPixelBatch::queue (renderPixels), RtRadianceBatch::queue (radianceRays)
};

// refineFrame: the adaptive frame's per-pixel state for the WHOLE image, the list of a pass and the batch arrays of one chunk of it (rt_refine.h), with a
// queue word of its own beside the pixel list's.  Allocated by the first call.  The host keeps what the helpers report and what decides whether the next
// call starts a new frame.
struct RefineState : QueryState {
    RtRefineParams planes = {};         // the device pointers (everything else of the block is filled per call)
    uint32_t* d_queue = nullptr;        // RtPixelBatch::queue
    size_t chunk_cap = 0;               // entries the batch arrays hold
    int passes = 0;                     // sampling calls since the last reset; 0 = the next call starts at sample 0
    int batch = 0;                      // the frame's batch (fixed by its first call)
    long long samples = 0;              // rtRefineSamples
    uint32_t last_len = 0;              // the length of the last call's list (rtRefineLastList)
    double ms = 0.0;                    // rtLastRefineMs
};

// rtMarkPose / renderMotion (rt_motion.h): the marked pose of the scene and the motion planes of the pass that runs, on the first in-process device.  Nothing is
// allocated before the first rtMarkPose or renderMotion; released by free_pass where the passes' buffers are, which also drops the mark (the state back to its
// initial values).  The planes are one set for all passes: a pass fills them in front of its own kernels, on the one stream every pass runs on.
struct PoseState : QueryState {
    bool marked = false;                // rtPoseMarked
    size_t count = 0;                   // slots / spheres of the mark
    rt_triangle* d_mark = nullptr;      // mesh scenes: the leaf-ordered slots as rtMarkPose saw them, in the layout of the live array, and
    rt_triangle* d_mark_alt = nullptr;  // the second buffer a rebuild gathers them into (then the two are swapped); allocated by the first such rebuild
    std::vector<float4> h_mark;         // sphere scenes: (center, radius) in the caller's order as rtMarkPose saw them, and
    float4* d_mark_sph = nullptr;       // their device copy;
    float4* d_live_sph = nullptr;       // the same for the spheres as they are now, uploaded when a pass finds it older than the last edit:
    int live_edits = -1;                // RenderContext::scene_edits of that upload
    float4* d_planes = nullptr;         // RtMotionParams::planes, 2 * npix
    float2* d_screen = nullptr;         // RtMotionParams::screen, npix; allocated by the first renderMotion that asks for it
};

// renderMotion: a pass without input and output frames (begin_pass is told so): the guide planes and the events are what it takes from the shared path.
struct MotionState : PassState {
    std::vector<float4> h_planes;       // the staging copy of PoseState::d_planes the caller's 3-float planes are filled from
};

// gatherRadiance / rtGatherDirections (rt_gather.h): the device arrays of one chunk of the caller's points - five per point, seven per ray of the chunk -, each
// grown to the largest chunk that asked for it, and the queue word of the radiance kernels.  Its own buffers: radianceRays' and the ray queries' stay theirs.
enum { kGatPos = 0, kGatNrm, kGatAcc, kGatOut, kGatNrays, kGatOrg, kGatDir, kGatIds, kGatTMax, kGatL, kGatRays, kGatOccluded, kGatBuffers };
struct GatherState : QueryState {
    char* d_buf[kGatBuffers] = {};
    size_t cap[kGatBuffers] = {};       // bytes d_buf[k] holds
    uint32_t* d_queue = nullptr;        // RtRadianceBatch::queue
};

// rasterTexels / bakeTexels (rt_texels.h): the raster's planes and work words, the compact list with its per-entry arrays, the planes a bake scatters into and
// the seven per-ray arrays of one chunk of the list, each grown to the largest call that asked for it, and the queue word of the radiance kernels.  Its own
// buffers: gatherRadiance's stay gatherRadiance's.
enum { kTexOwner = 0, kTexPrim, kTexSrc0, kTexSrc1, kTexBary, kTexPos, kTexNrm, kTexCounts, kTexRank, kTexList, kTexListPos, kTexListNrm,
       kTexAccPlane, kTexOutPlane, kTexRaysPlane, kTexAcc, kTexOut, kTexNrays,
       kTexOrg, kTexDir, kTexIds, kTexTMax, kTexL, kTexRays, kTexOccluded,
       kFltRec, kFltCol0, kFltCol1, kFltIn, kFltOut, kTexBuffers };
struct TexelState : QueryState {
    char* d_buf[kTexBuffers] = {};
    size_t cap[kTexBuffers] = {};       // bytes d_buf[k] holds
    uint32_t* d_length = nullptr;       // RtTexelParams::length
    uint32_t* d_queue = nullptr;        // RtRadianceBatch::queue
    int out_W = 0, out_H = 0, out_mode = -1;    // what d_buf[kTexOutPlane] holds: the out plane of the last bakeTexels, if that asked for out (out_W > 0);
                                        // in g_filter: what d_buf[kFltOut] holds, the out plane of the last filterTexels
};

// sampleTexels / renderLightmap (rt_lightmap.h): the arrays of one chunk of hits (prim, uv, normal up; out, valid down), or of one chunk of pixels (the ray
// buffers, the ray kernel's four planes, the frame's chunk), the uploaded texel planes and the word the valid hits are counted in.  One state per call:
// neither shares buffers or events with the other or with any other query.
enum { kLmPrim = 0, kLmUv, kLmNormal, kLmOut, kLmValid, kLmOrg, kLmDir, kLmT, kLmPlanes, kLmBuffers };
struct LightmapState : QueryState {
    char* d_buf[kLmBuffers] = {};
    size_t cap[kLmBuffers] = {};        // bytes d_buf[k] holds
    uint32_t* d_count = nullptr;        // RtSampleParams::count
};

DenoiseState g_denoise;
AccumulateState g_accumulate;
PreviewState g_preview;
DisplayState g_display;
PoseState g_pose;
MotionState g_motion;
ChunkState g_rays, g_pixels, g_radiance;
RefineState g_refine;
GatherState g_gather;
TexelState g_texels;
// filterTexels (rt_texel_filter_launch.h): a raster of its own (the raster's entries of a second TexelState), the two records per texel, the ping-pong pair of
// the values and the caller's planes (kFlt*).  Its own buffers and events: rasterTexels' and bakeTexels' stay theirs.
TexelState g_filter;
LightmapState g_sample, g_lightmap;

// The adaptive frame back to "the next refineFrame starts at sample 0" (rtResetRefine, setCamera, setRenderOptions, the scene edits); the buffers stay.
void reset_refine() {
    g_refine.passes = 0;
    g_refine.batch = 0;
    g_refine.samples = 0;
    g_refine.last_len = 0;
}

// The state of displayFrame's auto exposure back to "adapt from nothing" (rtResetDisplay, setRenderOptions); the buffers stay.
void reset_display() {
    g_display.adapted = false;
    memset(g_display.h_words, 0, RT_DISPLAY_BINS * sizeof(uint32_t));
}

// rtLastLaunches: the records of the last runRenderer (RT_LAUNCH_WORDS each) and the device / fp mode of the launcher being called
std::vector<int32_t> g_launches;
int g_launch_device = 0, g_launch_fp = 0;
int g_sphere_form = RT_SPHERE_FORM_NONE;        // rtLastSphereForm

void default_options(rt_render_options* o, int spheres) {
    memset(o, 0, sizeof *o);
    o->sky = spheres ? RT_SKY_GRADIENT : RT_SKY_CONST_GREY;     // kernels.cu:419-424
    o->nee = spheres ? 0 : 1;                                   // kernels.cu:16 SHADOW
    o->rr = spheres ? 0 : 1;                                    // kernels.cu:14 RUSSIAN_ROULETTE
    o->t_min = spheres ? 0.001f : 0.01f;                        // kernels.cu:19 EPSILON
    o->rng = RT_RNG_REFERENCE_STREAM;
    o->fp = RT_FP_PARITY;
    o->light.center.e[0] = (float)52.514355;                    // kernels.cu:93
    o->light.center.e[1] = (float)715.686951;
    o->light.center.e[2] = (float)-272.620972;
    o->light.radius = 50.0f;
    o->lightColor.e[0] = o->lightColor.e[1] = o->lightColor.e[2] = 20.0f;   // kernels.cu:94
    o->stripe_rows = 8;
    o->num_devices = 0;                                         // 0 = the process's current HIP device
    o->part_rank = 0;
    o->part_world = 1;
}

void free_device(DeviceState& d) {
    HIP_CHECK(hipSetDevice(d.device));
    if (d.stream) HIP_CHECK(hipStreamSynchronize(d.stream));
    dev_release_all(d.owned);
    if (d.h_params) HIP_CHECK(hipHostFree(d.h_params));
    if (d.ev_start) HIP_CHECK(hipEventDestroy(d.ev_start));
    if (d.ev_stop) HIP_CHECK(hipEventDestroy(d.ev_stop));
    if (d.ev_upd_start) HIP_CHECK(hipEventDestroy(d.ev_upd_start));
    if (d.ev_upd_stop) HIP_CHECK(hipEventDestroy(d.ev_upd_stop));
    if (d.ev_reb_start) HIP_CHECK(hipEventDestroy(d.ev_reb_start));
    if (d.ev_reb_stop) HIP_CHECK(hipEventDestroy(d.ev_reb_stop));
    if (d.stream) HIP_CHECK(hipStreamDestroy(d.stream));
    d = DeviceState();
}

// A pass's buffers and events, and the whole state back to its initial values: also without allocations, for the accumulator's frames / newest / prev_cam.
template <typename State>
void free_pass(State& n) {
    if (n.device >= 0) {
        int current = 0;
        HIP_CHECK(hipGetDevice(&current));
        HIP_CHECK(hipSetDevice(n.device));
        HIP_CHECK(hipDeviceSynchronize());
        dev_release_all(n.owned);
        if (n.ev_start) HIP_CHECK(hipEventDestroy(n.ev_start));
        if (n.ev_stop) HIP_CHECK(hipEventDestroy(n.ev_stop));
        HIP_CHECK(hipSetDevice(current));
    }
    n = State();
}

// Rows of the image owned by partition member `rank` of `world` with stripes of `sr` rows.
int local_rows_of(int ny, int sr, int rank, int world) {
    int rows = 0;
    const int nstripes = (ny + sr - 1) / sr;
    for (int k = rank; k < nstripes; k += world) rows += std::min(sr, ny - k * sr);
    return rows;
}

// The host mirrors of what the refit kernels write.  updateTriangles keeps mesh.tris and the scene bounds current itself; the nodes, the child-pair records and
// the leaf records - tens of MB for a large mesh, against the few microseconds of the refit - are fetched from the first device when the host next reads
// them: by setup_devices, which uploads the scene from the mirrors.  Every device holds the same refitted arrays and the update calls are blocking.
void fetch_refit() {
    RenderContext& c = g_ctx;
    if (!c.refit_stale) return;
    const DeviceState& d = c.devs[0];
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    HIP_CHECK(hipSetDevice(d.device));
    HIP_CHECK(hipMemcpy(c.mesh.bvh.data(), d.d_bvh, c.mesh.bvh.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(c.mesh.bvh_axis.data(), d.d_bvh_axis, c.mesh.bvh_axis.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (!c.mesh.leaf_tri.empty()) HIP_CHECK(hipMemcpy(c.mesh.leaf_tri.data(), d.d_leaf_tri, c.mesh.leaf_tri.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_CHECK(hipSetDevice(current));
    c.refit_stale = false;
}

// The sphere scene's arrays on device state `d` from the host copies (setup_devices, updateSpheres: the grouping may have changed their sizes).
void upload_sphere_arrays(DeviceState& d) {
    const RenderContext& c = g_ctx;
    dev_release(d.owned, d.d_spheres); dev_release(d.owned, d.d_rad); dev_release(d.owned, d.d_mat_color); dev_release(d.owned, d.d_mat_type);
    dev_release(d.owned, d.d_groups); dev_release(d.owned, d.d_orig); dev_release(d.owned, d.d_slot_of);
    d.d_spheres = upload(d.owned, c.sphere.spheres);
    d.d_rad = upload(d.owned, c.sphere.rad);
    d.d_mat_color = upload(d.owned, c.sphere.mat_color);
    d.d_mat_type = upload(d.owned, c.sphere.mat_type);
    d.d_groups = upload(d.owned, c.sphere.groups);
    d.d_orig = upload(d.owned, c.sphere.orig);
    d.d_slot_of = upload(d.owned, c.sphere.slot_of);
}

// (Re)creates the per-device state for the device list in g_ctx.opt.
void setup_devices() {
    RenderContext& c = g_ctx;
    fetch_refit();                                          // (the scene is uploaded from the host mirrors below)
    free_pass(g_denoise);                                   // (its buffers live on the first device of the list being replaced)
    free_pass(g_accumulate);                                // (so do the history's)
    free_pass(g_preview);
    free_pass(g_display);
    free_pass(g_motion);
    free_pass(g_pose);                                      // (the marked pose goes with it)
    free_pass(g_rays);
    free_pass(g_pixels);
    free_pass(g_radiance);
    free_pass(g_refine);
    free_pass(g_gather);
    free_pass(g_texels);
    free_pass(g_filter);
    free_pass(g_sample);
    free_pass(g_lightmap);
    for (DeviceState& d : c.devs) free_device(d);
    c.devs.clear();
    int count = 0;
    HIP_CHECK(hipGetDeviceCount(&count));
    int nd = c.opt.num_devices <= 0 ? 1 : c.opt.num_devices;
    if (nd > RT_MAX_DEVICES) rt_fail("too many devices");
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    for (int k = 0; k < nd; k++) {
        DeviceState d;
        d.device = (c.opt.num_devices <= 0) ? current : c.opt.devices[k];
        if (d.device < 0 || d.device >= count) rt_fail("device index out of range");
        HIP_CHECK(hipSetDevice(d.device));
        HIP_CHECK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreate(&d.ev_start));
        HIP_CHECK(hipEventCreate(&d.ev_stop));
        HIP_CHECK(hipEventCreate(&d.ev_upd_start));
        HIP_CHECK(hipEventCreate(&d.ev_upd_stop));
        HIP_CHECK(hipEventCreate(&d.ev_reb_start));
        HIP_CHECK(hipEventCreate(&d.ev_reb_stop));
        if (c.is_spheres) {
            d.d_params = dev_alloc<RtSphereParams>(d.owned, 1);
            HIP_CHECK(hipHostMalloc((void**)&d.h_params, sizeof(RtSphereParams), hipHostMallocDefault));
            upload_sphere_arrays(d);
        } else {
            d.d_tris = upload(d.owned, c.mesh.tris);
            d.d_bvh = upload(d.owned, c.mesh.bvh);
            d.d_bvh_axis = upload(d.owned, c.mesh.bvh_axis);
            d.d_leaf_tri = upload(d.owned, c.mesh.leaf_tri);
            d.d_leaf_ofs = upload(d.owned, c.mesh.leaf_ofs);
            d.d_materials = upload(d.owned, c.mesh.materials);
            if (!c.mesh.tex.empty()) {
                std::vector<float*> ptrs;
                for (const std::vector<float>& t : c.mesh.tex) ptrs.push_back(upload(d.owned, t));
                d.d_tex_data = upload(d.owned, ptrs);
                d.d_tex_width = upload(d.owned, c.mesh.tex_w);
                d.d_tex_height = upload(d.owned, c.mesh.tex_h);
            }
        }
        const int world = c.opt.part_world * nd, rank = c.opt.part_rank * nd + k;
        d.fb_rows = (size_t)local_rows_of(c.ny, c.opt.stripe_rows, rank, world);
        if (d.fb_rows > 0) {
            const size_t pixels = d.fb_rows * c.nx;
            const size_t padded = (size_t)((c.nx + 7) / 8) * ((d.fb_rows + 7) / 8) * 64;
            d.d_fb = dev_alloc<rt_vec3>(d.owned, pixels);
            d.d_order = dev_alloc<uint32_t>(d.owned, 3 * padded);       // work-order lists of the persistent kernels: 3 x (pixels padded to 8x8 tiles)
        }
        d.d_counters = dev_alloc<RtCounters>(d.owned, 1);
        HIP_CHECK(hipMemset(d.d_counters, 0, sizeof(RtCounters)));
        d.d_queue = dev_alloc<uint32_t>(d.owned, (size_t)kXcdQueues * kXcdQueueWords);     // one block of queue words per XCD (rt_params.h)
        HIP_CHECK(hipMemset(d.d_queue, 0, sizeof(uint32_t) * kXcdQueues * kXcdQueueWords));
        c.devs.push_back(d);
    }
    HIP_CHECK(hipSetDevice(c.devs[0].device));              // the query calls' own event pairs, on the device they run on
    for (QueryState* q : std::initializer_list<QueryState*>{ &g_rays, &g_pixels, &g_radiance, &g_refine, &g_gather, &g_texels, &g_filter, &g_sample, &g_lightmap }) {
        q->device = c.devs[0].device;
        HIP_CHECK(hipEventCreate(&q->ev_start));
        HIP_CHECK(hipEventCreate(&q->ev_stop));
    }
    HIP_CHECK(hipSetDevice(current));
}

void validate_options(const rt_render_options& o) {
    if (o.stripe_rows <= 0 || (o.stripe_rows % 8) != 0) rt_fail("stripe_rows must be a positive multiple of 8");
    if (o.part_world < 1 || o.part_rank < 0 || o.part_rank >= o.part_world) rt_fail("bad part_rank/part_world");
    if (o.num_devices < 0 || o.num_devices > RT_MAX_DEVICES) rt_fail("bad num_devices");
    if (!(o.t_min >= 0.0f)) rt_fail("t_min must be >= 0");
    if (o.sky != RT_SKY_CONST_GREY && o.sky != RT_SKY_GRADIENT) rt_fail("bad sky mode");
    if (o.rng != RT_RNG_REFERENCE_STREAM && o.rng != RT_RNG_COUNTER) rt_fail("bad rng mode");
    if (o.fp != RT_FP_PARITY && o.fp != RT_FP_FAST) rt_fail("bad fp mode");
}

void common_init(const rt_camera& cam, rt_vec3** fb, int nx, int ny, int maxDepth) {
    RenderContext& c = g_ctx;
    if (nx <= 0 || ny <= 0 || (long long)nx * ny > (1ll << 30)) rt_fail("bad image size");
    if (!fb) rt_fail("fb out-parameter is null");
    c.nx = nx; c.ny = ny;
    c.max_depth = maxDepth > 255 ? 255 : maxDepth;      // uint8_t bounce, helper_structs.h:58
    c.cam = cam;
    HIP_CHECK(hipHostMalloc((void**)&c.h_fb, (size_t)nx * ny * sizeof(rt_vec3), hipHostMallocDefault));   // kernels.cu:578-580
    memset(c.h_fb, 0, (size_t)nx * ny * sizeof(rt_vec3));
    *fb = c.h_fb;
    memset(&c.stats, 0, sizeof c.stats);
    c.prog_samples = 0;
    setup_devices();
    c.initialised = true;
}

// What initRendererSpheres and updateSpheres do with the caller's arrays: the checks, the slot layout and the decision where the kernels read the scene from.
void build_sphere_scene(const char* fn, const rt_sphere* spheres, const rt_material* materials, int n) {
    RenderContext& c = g_ctx;
    for (int k = 0; k < n; k++)
        if (materials[k].type < RT_DIFFUSE || materials[k].type >= RT_MATERIAL_TYPE_COUNT) rt_fail(": bad material type", fn);
    c.sphere = layout_spheres(spheres, materials, n, rt_read_switches().box_cells);
    // Scenes up to ~2100 spheres live in the LDS of every workgroup; larger ones are read from global memory (they stay in L2) by the
    // same kernel (no cost-ordered second phase, no sparse form beyond 4096 groups: slower per ray, same image).
    c.sphere.scene.global_scene = rt_sphere_kernel_lds_bytes(c.sphere.scene.n_padded, n) > 160 * 1024 ? 1 : 0;
    if (c.sphere.scene.n_padded > (1 << 24)) rt_fail(": more than 16 M sphere slots", fn);
}

void cleanup_impl() {
    RenderContext& c = g_ctx;
    free_pass(g_denoise);
    free_pass(g_accumulate);
    free_pass(g_preview);
    free_pass(g_display);
    free_pass(g_motion);
    free_pass(g_pose);                                      // (the marked pose goes with it)
    free_pass(g_rays);
    free_pass(g_pixels);
    free_pass(g_radiance);
    free_pass(g_refine);
    free_pass(g_gather);
    free_pass(g_texels);
    free_pass(g_filter);
    free_pass(g_sample);
    free_pass(g_lightmap);
    for (DeviceState& d : c.devs) free_device(d);
    c.devs.clear();
    if (c.h_ext) { if (c.ext_registered) HIP_CHECK(hipHostUnregister(c.h_ext)); c.h_ext = nullptr; c.ext_registered = false; }
    if (c.h_fb) HIP_CHECK(hipHostFree(c.h_fb));
    c = RenderContext();
}

}  // namespace

void rt_note_launch(int family, int phase, int cls, int chunked, int dbg, int scene, int lean, int threads, unsigned blocks) {
    const int32_t rec[RT_LAUNCH_WORDS] = { family, phase, cls, chunked, dbg, scene, lean, threads, (int32_t)blocks, g_launch_device, g_launch_fp };
    g_launches.insert(g_launches.end(), rec, rec + RT_LAUNCH_WORDS);
}
// (several devices render one frame under the same switches; should their forms ever differ, the general one is what is reported)
void rt_note_sphere_form(int form) { g_sphere_form = g_sphere_form == RT_SPHERE_FORM_NONE ? form : std::min(g_sphere_form, form); }

extern "C" {

int rtApiVersion(void) { return RT_API_VERSION; }

// sizeof of every struct that crosses this C-ABI, in the order of the RT_SIZEOF_* indices (rt_api.h).  A binding (the ctypes mirror, a cgo / JNI stub)
// compares them with its own view BEFORE the first call that passes one of them: getDefaultRenderOptions and getRenderStats write sizeof(struct)
// bytes through the caller's pointer, so a mirror that is shorter than the library's struct is a heap overrun, not an error message.
int rtStructSizes(int32_t* out, int n) {
    const int32_t sizes[RT_SIZEOF_COUNT] = {
        (int32_t)sizeof(rt_render_options), (int32_t)sizeof(rt_render_stats), (int32_t)sizeof(rt_camera), (int32_t)sizeof(rt_sphere),
        (int32_t)sizeof(rt_material), (int32_t)sizeof(rt_triangle), (int32_t)sizeof(rt_bvh_node), (int32_t)sizeof(rt_mesh),
        (int32_t)sizeof(rt_kernel_scene), (int32_t)sizeof(rt_stexture), (int32_t)sizeof(rt_plane), (int32_t)sizeof(rt_bbox), (int32_t)sizeof(rt_vec3) };
    for (int k = 0; k < n && k < RT_SIZEOF_COUNT; k++) out[k] = sizes[k];
    return RT_SIZEOF_COUNT;
}

int rtLastSphereForm(void) { return g_sphere_form; }

int rtLastLaunches(int32_t* out, int cap) {
    const int count = (int)(g_launches.size() / RT_LAUNCH_WORDS);
    const int n = std::min(count, std::max(cap, 0));
    if (out && n > 0) memcpy(out, g_launches.data(), (size_t)n * RT_LAUNCH_WORDS * sizeof(int32_t));
    return count;
}

int rtDeviceCount(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

void getDefaultRenderOptions(rt_render_options* opt, int is_sphere_scene) {
    if (!opt) return;
    default_options(opt, is_sphere_scene);
}

void initRenderer(const rt_kernel_scene sc, const rt_camera cam, rt_vec3** fb, int nx, int ny, int maxDepth) {
    if (g_ctx.initialised) cleanup_impl();
    RenderContext& c = g_ctx;
    if (!sc.m || !sc.m->tris || !sc.m->bvh || !sc.materials) rt_fail("initRenderer: null scene pointers");
    if (sc.m->numBvhNodes < 4 || (sc.m->numBvhNodes & 1)) rt_fail("initRenderer: numBvhNodes must be even and >= 4");
    if (sc.numPrimitivesPerLeaf <= 0) rt_fail("initRenderer: numPrimitivesPerLeaf must be positive");
    const uint32_t first_leaf = (uint32_t)sc.m->numBvhNodes / 2;                               // kernels.cu:614
    if ((unsigned long long)first_leaf * (unsigned)sc.numPrimitivesPerLeaf > sc.m->numTris)
        rt_fail("initRenderer: leaves * numPrimitivesPerLeaf exceeds numTris (traversal would read out of bounds)");
    if (first_leaf > (1u << 30)) rt_fail("initRenderer: BVH deeper than the 32-bit traversal bit-stack");
    c.is_spheres = false;
    default_options(&c.opt, 0);
    for (size_t k = 0; k < sc.m->numTris; k++)
        if (sc.m->tris[k].meshID >= sc.numMaterials && !std::isinf(sc.m->tris[k].v[0].e[0])) rt_fail("initRenderer: triangle meshID out of range");
    for (int t = 0; t < sc.numTextures; t++)
        if (!sc.textures[t].data || sc.textures[t].width <= 0 || sc.textures[t].height <= 0) rt_fail("initRenderer: bad texture");
    for (int k = 0; k < sc.numMaterials; k++)
        if (sc.materials[k].texId != -1 && (sc.materials[k].texId < 0 || sc.materials[k].texId >= sc.numTextures)) rt_fail("initRenderer: material texId out of range");
    c.mesh = layout_mesh(sc);
    common_init(cam, fb, nx, ny, maxDepth);
}

void initRendererSpheres(const rt_sphere* spheres, const rt_material* materials, int n,
                         const rt_camera cam, rt_vec3** fb, int nx, int ny, int maxDepth) {
    if (g_ctx.initialised) cleanup_impl();
    RenderContext& c = g_ctx;
    if (!spheres || !materials || n <= 0) rt_fail("initRendererSpheres: empty scene");
    c.is_spheres = true;
    default_options(&c.opt, 1);
    build_sphere_scene("initRendererSpheres", spheres, materials, n);
    common_init(cam, fb, nx, ny, maxDepth);
}

void setRenderOptions(const rt_render_options* opt) {
    RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("setRenderOptions before init");
    if (!opt) rt_fail("setRenderOptions: null");
    validate_options(*opt);
    const rt_render_options old = c.opt;
    c.opt = *opt;
    bool relayout = old.stripe_rows != opt->stripe_rows || old.part_rank != opt->part_rank ||
                    old.part_world != opt->part_world || old.num_devices != opt->num_devices;
    for (int k = 0; k < RT_MAX_DEVICES && !relayout; k++) relayout = old.devices[k] != opt->devices[k];
    if (relayout) setup_devices();
    c.prog_samples = 0;                                     // (any call: the options of the accumulated samples may differ)
    g_accumulate.frames = 0;                                // (likewise the history of accumulateFrame)
    g_preview.frames = 0;                                   // (and previewFrame's)
    reset_display();                                        // (and displayFrame's adapted exposure)
    reset_refine();                                         // (and the adaptive frame)
}

}  // extern "C"

namespace {

// The rows of in-process device k: member part_rank * devices + k of part_world * devices.
RtPartition partition_of(int k) {
    const RenderContext& c = g_ctx;
    const int nd = (int)c.devs.size();
    RtPartition part;
    part.stripe_rows = c.opt.stripe_rows;
    part.rank = c.opt.part_rank * nd + k;
    part.world = c.opt.part_world * nd;
    part.local_rows = (int)c.devs[k].fb_rows;
    return part;
}

// The whole image as one member's rows (the preview passes).
RtPartition whole_image_partition() {
    RtPartition part;
    part.stripe_rows = g_ctx.opt.stripe_rows;
    part.rank = 0;
    part.world = 1;
    part.local_rows = g_ctx.ny;
    return part;
}

// The parameter block of a kernel that works on rows `part` of the scene on device state `d`: the scene template, that device's scene arrays and what every
// kernel is given alike (camera, image size, partition, sky, t_min; meshes: the floor switch).  The only place a parameter block gets its scene pointers:
// a frame (render_frame) adds what belongs to a frame, the guide kernels (launch_guides) take it as it is.
RtSphereParams sphere_params(const DeviceState& d, const RtPartition& part) {
    const RenderContext& c = g_ctx;
    RtSphereParams p = c.sphere.scene;
    p.cam = c.cam; p.nx = c.nx; p.ny = c.ny;
    p.spheres = d.d_spheres; p.rad = d.d_rad; p.mat_color = d.d_mat_color; p.mat_type = d.d_mat_type;
    p.groups = d.d_groups; p.orig = d.d_orig; p.slot_of = d.d_slot_of;
    p.part = part; p.sky = c.opt.sky; p.t_min = c.opt.t_min;
    return p;
}

RtMeshParams mesh_params(const DeviceState& d, const RtPartition& part) {
    const RenderContext& c = g_ctx;
    RtMeshParams p = c.mesh.scene;
    p.cam = c.cam; p.nx = c.nx; p.ny = c.ny;
    p.tris = d.d_tris; p.bvh4 = d.d_bvh; p.bvh_axis = d.d_bvh_axis;
    p.materials = d.d_materials;
    p.tex_data = d.d_tex_data; p.tex_width = d.d_tex_width; p.tex_height = d.d_tex_height;
    p.part = part; p.sky = c.opt.sky; p.t_min = c.opt.t_min;
    p.floor_on = c.opt.floor ? 1 : 0;
    return p;
}

// ... plus what every path-tracing kernel takes from the options: what a path is.  The only place these fields are assigned: a frame (render_frame) and the
// pixel kernels (launch_pixels), which are bit-equal to it by contract, cannot disagree about them.
RtSphereParams sphere_path_params(const DeviceState& d, const RtPartition& part) {
    RtSphereParams p = sphere_params(d, part);
    p.max_depth = g_ctx.max_depth; p.rr = g_ctx.opt.rr; p.rng_mode = g_ctx.opt.rng;
    return p;
}

RtMeshParams mesh_path_params(const DeviceState& d, const RtPartition& part) {
    RtMeshParams p = mesh_params(d, part);
    p.max_depth = g_ctx.max_depth; p.rr = g_ctx.opt.rr; p.rng_mode = g_ctx.opt.rng;
    p.nee = g_ctx.opt.nee; p.light = g_ctx.opt.light; p.lightColor = g_ctx.opt.lightColor;
    return p;
}

// The first-hit guide kernel of the scene kind over rows `part`, into the compact planes `g` (renderGuides, begin_pass).
void launch_guides(const DeviceState& d, const RtPartition& part, const RtGuidePlanes& g) {
    HIP_CHECK(g_ctx.is_spheres ? rt_launch_guides_spheres(sphere_params(d, part), g, d.stream) : rt_launch_guides_mesh(mesh_params(d, part), g, d.stream));
}

// The pixel kernel of the scene kind and fp mode over the batch `b` (renderPixels, refineFrame): a frame's parameter block without anything a frame parks,
// records or reports, over the whole image as one member's rows.  max_waves: RtSwitches::pixels_waves as the call read it.
void launch_pixels(const DeviceState& d, const RtPixelBatch& b, int max_waves) {
    const bool fast = g_ctx.opt.fp == RT_FP_FAST;
    if (g_ctx.is_spheres) {
        const RtSphereParams p = sphere_path_params(d, whole_image_partition());
        HIP_CHECK(fast ? rt_launch_pixels_spheres_fast(p, b, max_waves, d.stream) : rt_launch_pixels_spheres_parity(p, b, max_waves, d.stream));
    } else {
        const RtMeshParams p = mesh_path_params(d, whole_image_partition());
        HIP_CHECK(fast ? rt_launch_pixels_mesh_fast(p, b, max_waves, d.stream) : rt_launch_pixels_mesh_parity(p, b, max_waves, d.stream));
    }
}

// The radiance kernel of the scene kind and fp mode over the batch `b` (radianceRays): the parameter block of launch_pixels - what a path is -, of which the
// kernel reads neither camera, image size nor partition.  max_waves: RtSwitches::pixels_waves as the call read it.
void launch_radiance(const DeviceState& d, const RtRadianceBatch& b, int max_waves) {
    const bool fast = g_ctx.opt.fp == RT_FP_FAST;
    if (g_ctx.is_spheres) {
        const RtSphereParams p = sphere_path_params(d, whole_image_partition());
        HIP_CHECK(fast ? rt_launch_radiance_spheres_fast(p, b, max_waves, d.stream) : rt_launch_radiance_spheres_parity(p, b, max_waves, d.stream));
    } else {
        const RtMeshParams p = mesh_path_params(d, whole_image_partition());
        HIP_CHECK(fast ? rt_launch_radiance_mesh_fast(p, b, max_waves, d.stream) : rt_launch_radiance_mesh_parity(p, b, max_waves, d.stream));
    }
}

// The ray kernel of the scene kind over the batch `b` (traceRays / occludedRays, gatherRadiance's visibility): closest hit, or any hit.
void launch_rays(const DeviceState& d, const RtRayBatch& b, bool any) {
    HIP_CHECK(g_ctx.is_spheres ? rt_launch_rays_spheres(sphere_params(d, whole_image_partition()), b, any, d.stream)
                               : rt_launch_rays_mesh(mesh_params(d, whole_image_partition()), b, any, d.stream));
}

// The query calls (traceRays / occludedRays, renderPixels, radianceRays, refineFrame, gatherRadiance) differ in their arguments, buffers and kernels; the rest is here, once.

// What "defined per pixel" asks of the options in force (renderPixels, radianceRays, refineFrame), under the function's name `fn`.
void check_per_pixel(const char* fn) {
    const RenderContext& c = g_ctx;
    if (c.opt.rng != RT_RNG_REFERENCE_STREAM) rt_fail(": only the reference RNG stream is one sequential stream per pixel (RT_RNG_COUNTER sums sample chunks)", fn);
    if (c.opt.variant != 0) rt_fail(": only the default kernels' frame (variant 0) is defined per pixel", fn);
    if (c.is_spheres && c.opt.floor) rt_fail(": the floor plane is only defined for mesh scenes (kernel_scene.floor)", fn);
    if (c.is_spheres && c.opt.nee) rt_fail(": next-event estimation is only defined for mesh scenes", fn);
}

// Onto the query's device (the first in-process one: every device holds the whole scene, setup_devices); returns the device to restore (end_query).
int begin_query(const QueryState& q) {
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    HIP_CHECK(hipSetDevice(q.device));
    return current;
}

void end_query(int current) { HIP_CHECK(hipSetDevice(current)); }

// The HIP-event time between the query's two events, in milliseconds, once the stream they were recorded on has drained.
double query_ms(const QueryState& q) {
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, q.ev_start, q.ev_stop));
    return (double)ms;
}

// body(first, m) for every chunk [first, first + m) of n items, `chunk` at a time.
template <typename Body>
void for_chunks(size_t n, size_t chunk, Body body) {
    for (size_t first = 0; first < n; first += chunk) body(first, std::min(chunk, n - first));
}

// Buffer k of a state that keeps d_buf / cap in bytes (GatherState, TexelState), grown to `bytes`.
template <typename State>
char* grown_buffer(State& q, int k, size_t bytes) {
    if (q.cap[k] < bytes) {
        dev_release(q.owned, q.d_buf[k]);
        q.d_buf[k] = dev_alloc<char>(q.owned, bytes);
        q.cap[k] = bytes;
    }
    return q.d_buf[k];
}

// n items of the caller's arrays through a kernel on the query's device, chunk by chunk on that device's stream: the buffers of `table` whose host[k] is not
// NULL grown to the chunk, the queue word (with_queue) zeroed, the kUp buffers uploaded from item `first` of host[k], launch(dev, m) between the state's two
// events - dev[k] = the device buffer of host[k], NULL where host[k] is -, the kDown buffers downloaded to item `first`, and the stream drained: blocking, the
// caller's arrays are complete on return.  Nothing of a frame's, the guides' or the passes' state is read or written.  Returns the HIP-event time of the
// launches (not the copies), summed over the chunks, in milliseconds.
template <typename Launch>
double run_chunks(ChunkState& q, size_t n, size_t chunk, const ChunkBuffer* table, int buffers, void* const* host, bool with_queue, Launch launch) {
    const hipStream_t stream = g_ctx.devs[0].stream;
    const int current = begin_query(q);
    if (with_queue && !q.d_queue) q.d_queue = dev_alloc<uint32_t>(q.owned, 1);
    double ms_sum = 0.0;
    for_chunks(n, chunk, [&](size_t first, size_t m) {
        char* dev[kChunkBuffers] = {};
        for (int k = 0; k < buffers; k++) {
            if (!host[k]) continue;
            if (q.cap[k] < m) {
                dev_release(q.owned, q.d_buf[k]);
                q.d_buf[k] = dev_alloc<char>(q.owned, m * table[k].bytes);
                q.cap[k] = m;
            }
            dev[k] = q.d_buf[k];
        }
        if (with_queue) HIP_CHECK(hipMemsetAsync(q.d_queue, 0, sizeof(uint32_t), stream));
        for (int k = 0; k < buffers; k++)
            if (dev[k] && (table[k].dir & kUp))
                HIP_CHECK(hipMemcpyAsync(dev[k], static_cast<const char*>(host[k]) + first * table[k].bytes, m * table[k].bytes, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipEventRecord(q.ev_start, stream));
        launch(dev, m);
        HIP_CHECK(hipEventRecord(q.ev_stop, stream));
        for (int k = 0; k < buffers; k++)
            if (dev[k] && (table[k].dir & kDown))
                HIP_CHECK(hipMemcpyAsync(static_cast<char*>(host[k]) + first * table[k].bytes, dev[k], m * table[k].bytes, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));                // (the events are read per chunk)
        ms_sum += query_ms(q);
    });
    end_query(current);
    return ms_sum;
}

// The diagnostic buffer of RT_WAVE_DEBUG (8 words per wave, or the mesh kernel's phase counters): allocated on first use, cleared on the stream.
constexpr size_t kWaveDbgWords = (size_t)65536 * 8;
unsigned long long* wave_debug_buffer(DeviceState& d) {
    if (!d.d_wave_dbg) d.d_wave_dbg = dev_alloc<unsigned long long>(d.owned, kWaveDbgWords);
    HIP_CHECK(hipMemsetAsync(d.d_wave_dbg, 0, kWaveDbgWords * sizeof(unsigned long long), d.stream));
    return d.d_wave_dbg;
}

// gather: local stripe q (rows of a compact device plane of `px_bytes` per pixel) -> global stripe q*world + rank of the host plane `host` (nx*ny pixels), on the
// device's stream.  The framebuffer and the guide planes are delivered this way.
void deliver_stripes(const DeviceState& d, const RtPartition& part, char* host, const char* dev, size_t px_bytes) {
    const RenderContext& c = g_ctx;
    const size_t row_bytes = (size_t)c.nx * px_bytes;
    const size_t stripe_bytes = (size_t)part.stripe_rows * row_bytes;
    const size_t full = d.fb_rows / part.stripe_rows, rem = d.fb_rows % part.stripe_rows;
    char* dst0 = host + (size_t)part.rank * stripe_bytes;
    if (part.world == 1) {                                              // the whole image: one linear copy
        HIP_CHECK(hipMemcpyAsync(dst0, dev, d.fb_rows * row_bytes, hipMemcpyDeviceToHost, d.stream));
        return;
    }
    if (full > 0)
        HIP_CHECK(hipMemcpy2DAsync(dst0, (size_t)part.world * stripe_bytes, dev, stripe_bytes, stripe_bytes, full, hipMemcpyDeviceToHost, d.stream));
    if (rem > 0)
        HIP_CHECK(hipMemcpyAsync(dst0 + full * (size_t)part.world * stripe_bytes, dev + full * stripe_bytes, rem * row_bytes, hipMemcpyDeviceToHost, d.stream));
}

// The whole-image preview passes (denoiseFrame, accumulateFrame, previewFrame) differ in their own arguments, buffers, parameter block and kernels; the rest is here, once.

// The argument checks both have, under the function's name `fn`.  A pass calls it with one group of `which` at a time, between its own checks: a call with
// two bad arguments fails on the one that comes first in that function's list.
enum { kCheckInit = 1, kCheckOut = 2, kCheckFlags = 4, kCheckSigmaZ = 8, kCheckFloor = 16 };
void check_pass_args(const char* fn, int which, const rt_vec3* out, int flags, float sigma_z) {
    const RenderContext& c = g_ctx;
    if ((which & kCheckInit) && !c.initialised) rt_fail(" before init", fn);
    if ((which & kCheckOut) && !out) rt_fail(": out is null", fn);
    if ((which & kCheckFlags) && (flags & ~(RT_DENOISE_DEMODULATE | RT_DENOISE_SAME_PRIM)) != 0) rt_fail(": unknown flag bits", fn);
    if ((which & kCheckSigmaZ) && (!std::isfinite(sigma_z) || !(sigma_z > 0.0f))) rt_fail(": sigma_z must be finite and positive", fn);
    if ((which & kCheckFloor) && c.is_spheres && c.opt.floor) rt_fail(": the floor plane is only defined for mesh scenes (kernel_scene.floor)", fn);
}

// Up to a pass's own kernels, on the first in-process device (every device holds the whole scene, setup_devices): in NULL = the framebuffer being delivered
// into; the buffers every pass has, `alloc_own()` for the pass's own and the events, when the device or the image size is not the state's; the upload of `in`
// before anything is written (out may be in); the guide planes of the camera and options in force.  Returns the device to restore (end_pass).  The pass
// records n.ev_start in front of its kernels.  `without` names what a pass does not take (displayFrame): kPassNoGuides - no guide planes, no guide launch;
// kPassOwnOutput - no rt_vec3 output buffer, the pass delivers buffers of its own type (end_pass); kPassNoUpload - this call's input is on the device already.
// kPassNoInput - no input frame either (renderMotion).  `motion`: the pass reads the motion planes when a pose is marked (accumulateFrame and previewFrame with a
// history): the motion kernel runs behind the guide kernel; without a mark nothing is launched and nothing is allocated.
enum { kPassNoGuides = 1, kPassOwnOutput = 2, kPassNoUpload = 4, kPassNoInput = 8 };

// The caller's spheres (center, radius) in the caller's order, from the slot layout the kernels read (rt_scene_layout.h).
std::vector<float4> caller_spheres() {
    const SphereLayout& s = g_ctx.sphere;
    std::vector<float4> out((size_t)s.scene.n);
    for (size_t k = 0; k < out.size(); k++) {
        const int slot = s.slot_of[k];
        const float4 c = s.spheres[(size_t)(slot + slot / kSphereGroup)];
        out[k] = make_float4(c.x, c.y, c.z, s.rad[(size_t)slot]);
    }
    return out;
}

// Sphere scenes with a pose marked: the device copy of the caller-order spheres as they are now, uploaded again when an edit has made it stale.  The first
// in-process device is current.
void refresh_live_spheres() {
    const RenderContext& c = g_ctx;
    PoseState& m = g_pose;
    if (!m.marked || !c.is_spheres || m.live_edits == c.scene_edits) return;
    const DeviceState& d = c.devs[0];
    const std::vector<float4> live = caller_spheres();
    if (!m.d_live_sph) m.d_live_sph = dev_alloc<float4>(m.owned, m.count);
    HIP_CHECK(hipMemcpyAsync(m.d_live_sph, live.data(), m.count * sizeof(float4), hipMemcpyHostToDevice, d.stream));
    HIP_CHECK(hipStreamSynchronize(d.stream));              // (the source is a local; every pass is blocking: nothing on the stream still reads the old copy)
    m.live_edits = c.scene_edits;
}

// The motion kernel (rt_motion.h) over the guide planes of pass `n`, on the first in-process device, which is current: Pm and nm of the marked pose - P and n
// themselves without one - into the planes every pass shares, `screen` (with its camera C') on request.
void launch_motion(const PassState& n, bool screen, const rt_camera& prev_cam) {
    const RenderContext& c = g_ctx;
    const DeviceState& d = c.devs[0];
    PoseState& m = g_pose;
    m.device = d.device;
    if (!m.d_planes) m.d_planes = dev_alloc<float4>(m.owned, 2 * n.npix);
    if (screen && !m.d_screen) m.d_screen = dev_alloc<float2>(m.owned, n.npix);
    RtMotionParams q;
    memset(&q, 0, sizeof q);
    q.cam = c.cam; q.nx = c.nx; q.ny = c.ny;
    q.normal = n.d_guide[1]; q.depth = n.d_guide[2]; q.prim = reinterpret_cast<const int32_t*>(n.d_guide[3]);
    q.planes = m.d_planes; q.screen = screen ? m.d_screen : nullptr;
    refresh_live_spheres();
    if (m.marked && c.is_spheres) {
        q.live_sph = m.d_live_sph; q.mark_sph = m.d_mark_sph; q.count = (uint32_t)m.count;
    } else if (m.marked) {
        q.live = d.d_tris; q.mark = m.d_mark; q.count = (uint32_t)m.count;
    }
    HIP_CHECK(rt_launch_motion(q, prev_cam, d.stream));
}

template <typename State, typename AllocOwn>
int begin_pass(State& n, const rt_vec3* in, AllocOwn alloc_own, int without = 0, bool motion = false) {
    const RenderContext& c = g_ctx;
    if (!in) in = c.h_ext ? c.h_ext : c.h_fb;
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    const DeviceState& d = c.devs[0];
    HIP_CHECK(hipSetDevice(d.device));
    const size_t npix = (size_t)c.nx * c.ny;
    if (n.device != d.device || n.npix != npix) {
        free_pass(n);
        HIP_CHECK(hipSetDevice(d.device));
        n.device = d.device; n.npix = npix;
        if (!(without & kPassNoGuides))
            for (int q = 0; q < 4; q++) n.d_guide[q] = dev_alloc<float>(n.owned, npix * kGuideBytes[q] / sizeof(float));
        if (!(without & kPassNoInput)) n.d_in = dev_alloc<rt_vec3>(n.owned, npix);
        if (!(without & kPassOwnOutput)) n.d_out = dev_alloc<rt_vec3>(n.owned, npix);
        alloc_own();
        HIP_CHECK(hipEventCreate(&n.ev_start));
        HIP_CHECK(hipEventCreate(&n.ev_stop));
    }
    if (!(without & (kPassNoUpload | kPassNoInput))) HIP_CHECK(hipMemcpyAsync(n.d_in, in, npix * sizeof(rt_vec3), hipMemcpyHostToDevice, d.stream));
    if (!(without & kPassNoGuides))
        launch_guides(d, whole_image_partition(), { n.d_guide[0], n.d_guide[1], n.d_guide[2], reinterpret_cast<int32_t*>(n.d_guide[3]), nullptr });
    if (motion && g_pose.marked) launch_motion(n, false, c.cam);
    return current;
}

// The fields every pass's parameter block starts from, the rest zero.
template <typename Params>
Params pass_params(const PassState& n) {
    Params q;
    memset(&q, 0, sizeof q);
    q.cam = g_ctx.cam; q.nx = g_ctx.nx; q.ny = g_ctx.ny;
    q.albedo = n.d_guide[0]; q.normal = n.d_guide[1]; q.depth = n.d_guide[2]; q.prim = reinterpret_cast<const int32_t*>(n.d_guide[3]);
    q.in = n.d_in; q.out = n.d_out;
    return q;
}

// After a pass's kernels: the stop event, out (and the optional per-pixel planes of accumulateFrame and previewFrame, `d_history` -> `history` and
// `d_variance` -> `variance`) to the caller, complete on return: blocking.  A pass whose output is not an rt_vec3 frame (displayFrame) passes out = NULL and the
// `n_own` device-to-host copies `own` it delivers instead.  Returns the HIP-event time of the kernels in milliseconds.
struct PassCopy {
    void* host;
    const void* dev;
    size_t bytes;
};
double end_pass(const PassState& n, int current, rt_vec3* out, float* history = nullptr, const float* d_history = nullptr, float* variance = nullptr,
                const float* d_variance = nullptr, const PassCopy* own = nullptr, int n_own = 0) {
    const DeviceState& d = g_ctx.devs[0];
    HIP_CHECK(hipEventRecord(n.ev_stop, d.stream));
    if (out) HIP_CHECK(hipMemcpyAsync(out, n.d_out, n.npix * sizeof(rt_vec3), hipMemcpyDeviceToHost, d.stream));
    for (int k = 0; k < n_own; k++) HIP_CHECK(hipMemcpyAsync(own[k].host, own[k].dev, own[k].bytes, hipMemcpyDeviceToHost, d.stream));
    if (history) HIP_CHECK(hipMemcpyAsync(history, d_history, n.npix * sizeof(float), hipMemcpyDeviceToHost, d.stream));
    if (variance) HIP_CHECK(hipMemcpyAsync(variance, d_variance, n.npix * sizeof(float), hipMemcpyDeviceToHost, d.stream));
    HIP_CHECK(hipStreamSynchronize(d.stream));
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, n.ev_start, n.ev_stop));
    HIP_CHECK(hipSetDevice(current));
    return (double)ms;
}

// The parked state of a two-dispatch frame (both kernels), on the first frame that can take the two dispatches and in the one form that frame's switches
// select: 32-byte records (RT_ORD_PACKED, the default) or the three arrays.  A frame under the other form frees what it does not read: a 3840x2160 frame
// holds 20 + 32 bytes per pixel here instead of 20 + 20 + 32 from init on, and a device that never takes the two dispatches (counter stream, few samples,
// a scene in global memory) none of them.
void parked_buffers(DeviceState& d, bool packed) {
    const size_t nx = (size_t)g_ctx.nx;
    const size_t pixels = d.fb_rows * nx;
    const size_t padded = ((nx + 7) / 8) * ((d.fb_rows + 7) / 8) * 64;
    if (!d.d_px_state) d.d_px_state = dev_alloc<float4>(d.owned, pixels);
    if (!d.d_px_rays) d.d_px_rays = dev_alloc<uint32_t>(d.owned, pixels);
    if (packed) {
        dev_release(d.owned, d.d_ord_state);
        dev_release(d.owned, d.d_ord_rays);
        if (!d.d_ord_rec) d.d_ord_rec = dev_alloc<float4>(d.owned, padded * 2);
    } else {
        dev_release(d.owned, d.d_ord_rec);
        if (!d.d_ord_state) d.d_ord_state = dev_alloc<float4>(d.owned, padded);
        if (!d.d_ord_rays) d.d_ord_rays = dev_alloc<uint32_t>(d.owned, padded);
    }
}

// What a cost map depends on beside its device state: the image, the partition, what decides how many rays a pixel takes, and the camera.  Compared by
// value (setRenderOptions with equal fields, setCamera with the same camera change nothing); counters, variant, fp and the traffic switches are not in
// it: the ordering pass runs every frame under that frame's switches.  The camera is, because a moved camera's frame is slower ordered by the old map
// than measured; an edited scene (updateSpheres) likewise, whatever RT_COST_REUSE says - a 2-degree step of an orbit moves the long pixels by tens of pixels: 1200x800x16 spp 3.06 ms against 2.68 (DESIGN.md 3.15,
// tools/bench_orbit.py); RT_COST_REUSE=2 keeps the map across setCamera (that measurement, and the tests of a map that is wrong).
std::array<int, 11> cost_key_of(const RtPartition& part, bool with_camera) {
    const RenderContext& c = g_ctx;
    return { c.nx, c.ny, part.stripe_rows, part.rank, part.world, part.local_rows, c.max_depth, (int)c.opt.rr, (int)c.opt.rng, with_camera ? c.camera_moves : 0,
             c.scene_edits };
}

// Blocks until every device's stream has drained (kernels.cu:660-661: the calls are blocking) and returns the longest time between the two events each device
// recorded on it, in ms.  with_rows: only the devices that render rows of the image (the others recorded nothing).
double finish_devices(hipEvent_t DeviceState::*start, hipEvent_t DeviceState::*stop, bool with_rows) {
    double ms_max = 0.0;
    for (DeviceState& d : g_ctx.devs) {
        if (with_rows && d.fb_rows == 0) continue;
        HIP_CHECK(hipSetDevice(d.device));
        HIP_CHECK(hipStreamSynchronize(d.stream));
        float ms = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&ms, d.*start, d.*stop));
        ms_max = std::max(ms_max, (double)ms);
    }
    return ms_max;
}

// One frame of ns samples per pixel (runRenderer), or one pass of a progressive frame (progressive): samples [first, ns) of every pixel, continued from
// and parked into the device's accumulation buffers, the framebuffer = sum / ns.
void render_frame(int ns, int first, bool progressive) {
    RenderContext& c = g_ctx;
    const auto t0 = std::chrono::steady_clock::now();
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    const int nd = (int)c.devs.size();
    const size_t row_bytes = (size_t)c.nx * sizeof(rt_vec3);
    int64_t samples = 0;
    int launches = 0;
    g_launches.clear();
    g_sphere_form = RT_SPHERE_FORM_NONE;
    g_launch_fp = c.opt.fp;
    const RtSwitches sw = rt_read_switches();           // the environment switches of this frame

    for (int k = 0; k < nd; k++) {
        DeviceState& d = c.devs[k];
        if (d.fb_rows == 0) continue;
        HIP_CHECK(hipSetDevice(d.device));
        g_launch_device = d.device;
        const RtPartition part = partition_of(k);
        if (c.opt.counters) HIP_CHECK(hipMemsetAsync(d.d_counters, 0, sizeof(RtCounters), d.stream));
        int spw = ns, chunks = 1;               // sphere path, RT_RNG_COUNTER: samples per work item, work items per pixel
        if (c.is_spheres && c.opt.rng == RT_RNG_COUNTER && (c.opt.variant & 0xFF) == 0) {
            // default: 4 samples per item, but no more items than fill and balance the machine (~32 M): a 3840x2160x4096spp frame cut into 4-sample items
            // would be 8.5 G items and a 100 GB buffer of partial sums - it takes 3 items per pixel instead
            int want = c.opt.samples_per_item;
            if (want <= 0) {
                const long long pixels = std::max<long long>(1, (long long)d.fb_rows * c.nx);
                const long long max_chunks = std::max<long long>(1, (32ll << 20) / pixels);
                want = (int)std::max<long long>(4, (ns + max_chunks - 1) / max_chunks);
            }
            if (want < ns) { spw = want; chunks = (ns + want - 1) / want; }
        }
        const int vk = c.opt.variant & 0xFF, vcb = (c.opt.variant >> 16) & 0xFF;
        // Every kernel renders into the compact device framebuffer, which the copy engine delivers behind it (below).  RT_FB_DIRECT=1 (A/B): the default
        // sphere kernel stores finished pixels straight into the pinned host framebuffer instead (12 bytes each, spread over the whole frame time), with
        // no copy after the kernel.  (An external framebuffer that could not be page-locked is reached by the copy path only: see setExternalFramebuffer.)
        const bool fb_direct = c.is_spheres && c.max_depth > 0 && sw.fb_direct && vk == 0 && (vcb == 0 || vcb == 255) && chunks == 1 &&
                               (!c.h_ext || c.ext_registered);
        rt_vec3* const h_target = c.h_ext ? c.h_ext : c.h_fb;
        // Poison the framebuffer the kernel WRITES (all-ones = NaN): every pixel is written exactly once per frame, so a pixel the work
        // distribution lost shows up as NaN instead of as last frame's (correct-looking) value.  The compact device buffer is filled on the
        // render stream before the timed window; with direct delivery the HOST framebuffer's rows of this partition member are filled by the
        // device itself (RtSphereParams::poison_fb): by the frame's first dispatch, which stores no pixel (the bus writes ride beside its
        // compute: nothing in the frame), or by a small kernel in front of a single dispatch.
        if (!fb_direct && d.fb_rows > 0) HIP_CHECK(hipMemsetAsync(d.d_fb, 0xFF, d.fb_rows * row_bytes, d.stream));
        HIP_CHECK(hipEventRecord(d.ev_start, d.stream));
        if (c.max_depth <= 0) {
            HIP_CHECK(hipMemsetAsync(d.d_fb, 0, d.fb_rows * row_bytes, d.stream));     // loop of kernels.cu:402 never runs
        } else if (c.is_spheres) {
            RtSphereParams p = sphere_path_params(d, part);
            p.ns = ns;
            p.fb = d.d_fb;
            p.counters = c.opt.counters ? d.d_counters : nullptr;
            p.queue = d.d_queue;
            p.order = d.d_order;
            // work items: one per pixel in the reference-stream mode (a pixel's samples are one sequential RNG stream);
            // with the per-sample counter stream the samples are independent and a pixel is split into chunks
            p.spw = spw; p.chunks = chunks; p.partial = nullptr;
            // the two cost-ordered dispatches need the reference stream in whole pixels, the scene in the LDS and 8 samples (plan_spheres): their buffers from then on
            const bool whole_pixels = c.opt.rng == RT_RNG_REFERENCE_STREAM && chunks == 1 && vk == 0 && (vcb == 0 || vcb == 255) && !p.global_scene;
            if (whole_pixels && (ns >= 8 || progressive)) parked_buffers(d, sw.ord_packed);
            p.phase = 0; p.s_split = 0; p.px_state = d.d_px_state; p.px_rays = d.d_px_rays; p.ord_state = d.d_ord_state; p.ord_rays = d.d_ord_rays;
            if (progressive) { p.acc_state = d.d_acc_state; p.acc_rays = d.d_acc_rays; p.acc_first = first; }
            // The cost map: every such runRenderer frame records the rays of its pixels, and the next one is ordered by them if nothing the map depends on has
            // changed (RtSphereParams::cost_rays).  A progressive pass has its own accumulated rays: it neither reads nor writes the map.  RT_COST_REUSE=0: no map.
            if (whole_pixels && !progressive && sw.cost_reuse != 0 && ns <= RT_PROGRESSIVE_MAX_SAMPLES) {
                if (!d.d_cost_rays) {
                    d.d_cost_rays = dev_alloc<uint32_t>(d.owned, d.fb_rows * c.nx);
                    d.cost_samples = 0;
                }
                const std::array<int, 11> key = cost_key_of(part, sw.cost_reuse != 2);
                p.cost_rays = d.d_cost_rays;
                p.acc_rays = d.d_cost_rays;                         // (this frame's rays: the same buffer, written behind the ordering pass that reads it)
                p.cost_samples = key == d.cost_key ? d.cost_samples : 0;
                d.cost_key = key;
                d.cost_samples = ns;
            }
            p.chain_top_thr = sw.top_thr;
            // traffic forms of the two-dispatch frame (RtSphereParams::ord_rec / xcd_queues / p1_tile_major)
            p.ord_rec = sw.ord_packed ? d.d_ord_rec : nullptr;
            p.xcd_queues = sw.xcd_queues ? kXcdQueues : 0;
            p.p1_tile_major = sw.p1_tile;
            if (chunks > 1) {
                const size_t sums = d.fb_rows * c.nx * (size_t)p.chunks;
                if (sums * sizeof(rt_vec3) > d.partial_bytes) {
                    dev_release(d.owned, d.d_partial);
                    d.d_partial = dev_alloc<rt_vec3>(d.owned, sums);
                    d.partial_bytes = sums * sizeof(rt_vec3);
                }
                p.partial = d.d_partial;
            }
            // diagnostics: per-wave time stamps -> file (not in a progressive pass: PHASE 2's per-pixel time line would overwrite the parked state)
            if (sw.wave_debug && !progressive) p.wave_dbg = wave_debug_buffer(d);
            if (c.opt.nee) rt_fail("runRenderer: next-event estimation is only defined for mesh scenes");
            if (c.opt.floor) rt_fail("runRenderer: the floor plane is only defined for mesh scenes (kernel_scene.floor)");
            if (fb_direct) {
                void* dp = nullptr;
                HIP_CHECK(hipHostGetDevicePointer(&dp, (void*)h_target, 0));
                p.fb = reinterpret_cast<rt_vec3*>(dp);
                p.fb_global_rows = 1;
                p.poison_fb = sw.fb_poison ? 1 : 0;
            }
            // the device copy of the parameter block (RtSphereParams::self): owned by this DeviceState, refreshed by every frame from a pinned
            // staging copy (runRenderer is synchronous: the previous frame's upload has completed)
            p.self = d.d_params;
            *d.h_params = p;
            HIP_CHECK(hipMemcpyAsync(d.d_params, d.h_params, sizeof(RtSphereParams), hipMemcpyHostToDevice, d.stream));
            HIP_CHECK(c.opt.fp == RT_FP_FAST ? rt_launch_spheres_fast(p, c.opt.variant, sw, d.stream)
                                             : rt_launch_spheres_parity(p, c.opt.variant, sw, d.stream));
            launches++;
        } else {
            RtMeshParams p = mesh_path_params(d, part);
            p.ns = ns;
            p.leaf_tri = sw.compact_leaves ? d.d_leaf_tri : nullptr; p.leaf_ofs = sw.compact_leaves ? d.d_leaf_ofs : nullptr;
            p.fb = d.d_fb;
            if (c.opt.floor && (c.opt.variant & 0xFF) == 1) rt_fail("runRenderer: the floor plane is not built into the tile-per-wave A/B kernel (variant 1)");
            p.counters = c.opt.counters ? d.d_counters : nullptr;
            p.queue = d.d_queue;
            if (c.opt.rng == RT_RNG_REFERENCE_STREAM && sw.mesh_two && !c.opt.counters && first == 0) parked_buffers(d, sw.ord_packed);      // (rt_launch_mesh_*: its two dispatches)
            p.s_split = 0; p.px_state = d.d_px_state; p.px_rays = d.d_px_rays; p.order = d.d_order; p.ord_state = d.d_ord_state; p.ord_rays = d.d_ord_rays;
            if (progressive) { p.acc_state = d.d_acc_state; p.acc_first = first; }
            // the traffic forms of the two-dispatch frame, as for sphere scenes (the same switches; the mesh frame always renders into the device framebuffer)
            p.ord_rec = sw.ord_packed ? d.d_ord_rec : nullptr;
            p.xcd_queues = sw.xcd_queues ? kXcdQueues : 0;
            p.p1_segments = sw.p1_tile == 2 ? 1 : 0;
            if (sw.wave_debug) p.dbg = wave_debug_buffer(d);        // diagnostics: phase cycle / lane counters -> file
            HIP_CHECK(c.opt.fp == RT_FP_FAST ? rt_launch_mesh_fast(p, c.opt.variant, sw, d.stream)
                                             : rt_launch_mesh_parity(p, c.opt.variant, sw, d.stream));
            launches++;
        }
        HIP_CHECK(hipEventRecord(d.ev_stop, d.stream));

        if (!fb_direct) deliver_stripes(d, part, reinterpret_cast<char*>(h_target), reinterpret_cast<const char*>(d.d_fb), sizeof(rt_vec3));
        samples += (int64_t)d.fb_rows * c.nx * (ns - first);
    }

    const double kernel_ms = finish_devices(&DeviceState::ev_start, &DeviceState::ev_stop, true);
    rt_render_stats st;
    memset(&st, 0, sizeof st);
    for (int k = 0; k < nd; k++) {
        DeviceState& d = c.devs[k];
        if (d.fb_rows == 0) continue;
        HIP_CHECK(hipSetDevice(d.device));
        if (d.d_wave_dbg && sw.wave_debug) {
            std::vector<unsigned long long> h(kWaveDbgWords);
            HIP_CHECK(hipMemcpy(h.data(), d.d_wave_dbg, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            if (FILE* f = fopen(sw.wave_debug->c_str(), "wb")) { fwrite(h.data(), sizeof(unsigned long long), h.size(), f); fclose(f); }
            if (d.d_px_state && c.is_spheres) {                      // per-pixel time line of the second phase (see finish())
                std::vector<float> px((size_t)d.fb_rows * c.nx * 4);
                HIP_CHECK(hipMemcpy(px.data(), d.d_px_state, px.size() * sizeof(float), hipMemcpyDeviceToHost));
                const std::string path = *sw.wave_debug + ".px";
                if (FILE* f = fopen(path.c_str(), "wb")) { fwrite(px.data(), sizeof(float), px.size(), f); fclose(f); }
            }
        }
        if (c.opt.counters) {
            RtCounters h;
            HIP_CHECK(hipMemcpy(&h, d.d_counters, sizeof h, hipMemcpyDeviceToHost));
            st.rays += h.rays; st.prim_tests += h.prim_tests; st.node_visits += h.node_visits;
            st.exec_tests += h.exec_tests; st.shadow_rays += h.shadow_rays; st.box_tests += h.box_tests;
            for (int q = 0; q < RT_STAT_COUNT; q++) st.ref_stats[q] += h.ref_stats[q];
        }
    }
    HIP_CHECK(hipSetDevice(current));
    const auto t1 = std::chrono::steady_clock::now();
    st.kernel_ms = kernel_ms;
    st.total_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    st.samples = samples;
    st.num_launches = launches;
    c.stats = st;
}

}  // namespace

// The environment switches (rt_params.h: RtSwitches): the library's only reads of the environment.
namespace {

bool env_flag(const char* name, bool dflt) {            // "0" = off, any other value = on, unset = dflt
    const char* v = getenv(name);
    return v ? v[0] != '0' : dflt;
}

bool env_one(const char* name) {                        // on only as "1"
    const char* v = getenv(name);
    return v && v[0] == '1';
}

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

std::optional<std::string> env_str(const char* name) {
    const char* v = getenv(name);
    if (!v) return std::nullopt;
    return std::string(v);
}

}  // namespace

RtSwitches rt_read_switches() {
    RtSwitches s;
    s.xcd_queues = env_flag("RT_XCD_QUEUES", s.xcd_queues);
    s.ord_packed = env_flag("RT_ORD_PACKED", s.ord_packed);
    const int p1_tile = env_int("RT_P1_TILE", s.p1_tile);
    s.p1_tile = (p1_tile >= 0 && p1_tile <= 2) ? p1_tile : 0;
    s.wave_debug = env_str("RT_WAVE_DEBUG");

    s.fb_direct = env_flag("RT_FB_DIRECT", s.fb_direct);
    s.fb_poison = env_flag("RT_FB_POISON", s.fb_poison);
    s.box_cells = env_flag("RT_BOX_CELLS", s.box_cells);
    s.compact_leaves = env_flag("RT_COMPACT_LEAVES", s.compact_leaves);
    s.ext_fb_no_register = env_one("RT_EXT_FB_NO_REGISTER");
    s.cleanup_device_reset = env_one("RT_CLEANUP_DEVICE_RESET");
    const int cost_reuse = env_int("RT_COST_REUSE", s.cost_reuse);
    s.cost_reuse = (cost_reuse >= 0 && cost_reuse <= 2) ? cost_reuse : 1;
    s.pixels_waves = std::max(0, env_int("RT_PIXELS_WAVES", s.pixels_waves));
    s.refine_order = env_flag("RT_REFINE_ORDER", s.refine_order);

    const int top_thr = env_int("RT_TOP_THR", s.top_thr);
    if (top_thr >= 320) s.top_thr = top_thr;
    s.basic = env_flag("RT_BASIC", s.basic);
    s.onepass = env_flag("RT_ONEPASS", s.onepass);
    if (const auto v = env_str("RT_LEAN6_PIXELS")) s.lean6_pixels = atoll(v->c_str());
    s.hybrid_two = env_one("RT_HYBRID_TWO");
    if (const auto v = env_str("RT_MID")) sscanf(v->c_str(), "%d,%d", &s.mid_waves, &s.mid_cap);
    s.chain_single = env_flag("RT_CHAIN_SINGLE", s.chain_single);
    s.single_ray = env_flag("RT_SINGLE_RAY", s.single_ray);
    s.pool = env_int("RT_POOL", s.pool);
    s.wave_debug_light = env_one("RT_WAVE_DEBUG_LIGHT");
    s.wave_debug_phase = env_one("RT_WAVE_DEBUG_PHASE");
    if (const auto v = env_str("RT_TUNE")) {
        RtTune& t = s.tune.emplace();
        t.text = *v;
        t.n = std::max(0, sscanf(v->c_str(), "%d,%d,%d,%d,%d,%d,%d,%d,%d", &t.v[0], &t.v[1], &t.v[2], &t.v[3], &t.v[4], &t.v[5], &t.v[6], &t.v[7], &t.v[8]));
    }

    s.mesh_lean = env_flag("RT_MESH_LEAN", s.mesh_lean);
    const auto order = env_str("RT_MESH_ORDER");
    s.mesh_tile_order = order && (*order)[0] == 't';
    s.mesh_two = env_flag("RT_MESH_TWO", s.mesh_two);
    s.mesh_split = std::max(1, env_int("RT_MESH_SPLIT", s.mesh_split));
    s.mesh_heavy = env_int("RT_MESH_HEAVY", s.mesh_heavy);
    s.mesh_rounds = env_int("RT_MESH_ROUNDS", s.mesh_rounds);
    s.mesh_rev = env_one("RT_MESH_REV");
    s.mesh_chain_thr = std::max(17, env_int("RT_MESH_CHAIN_THR", s.mesh_chain_thr));
    s.mesh_chain_lanes = std::min(64, std::max(0, env_int("RT_MESH_CHAIN_LANES", s.mesh_chain_lanes)));
    s.mesh_chain_frac = env_int("RT_MESH_CHAIN_FRAC", s.mesh_chain_frac) & 0xF;
    s.mesh_diag_file = env_str("RT_MESH_DIAG_FILE");
    return s;
}

extern "C" {

void runRenderer(int ns, int tx, int ty) {
    (void)tx; (void)ty;     // CUDA block shape of the reference (main.cpp:69-70); the wave64 tile is fixed
    RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("runRenderer before init");
    if (ns <= 0) rt_fail("runRenderer: ns must be positive");
    render_frame(ns, 0, false);
}

void runRendererProgressive(int ns, int tx, int ty) {
    (void)tx; (void)ty;
    RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("runRendererProgressive before init");
    if (ns <= 0) rt_fail("runRendererProgressive: ns must be positive");
    if (c.opt.rng != RT_RNG_REFERENCE_STREAM) rt_fail("runRendererProgressive: only the reference RNG stream accumulates (RT_RNG_COUNTER sums sample chunks)");
    if (c.opt.variant != 0) rt_fail("runRendererProgressive: only the default kernels (variant 0) continue a frame");
    if (ns > RT_PROGRESSIVE_MAX_SAMPLES - c.prog_samples) rt_fail("runRendererProgressive: total samples per pixel above RT_PROGRESSIVE_MAX_SAMPLES");
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    for (DeviceState& d : c.devs) {                     // the accumulation buffers: on the first pass of this device state
        if (d.fb_rows == 0 || d.d_acc_state) continue;
        HIP_CHECK(hipSetDevice(d.device));
        d.d_acc_state = dev_alloc<float4>(d.owned, d.fb_rows * c.nx);
        if (c.is_spheres) d.d_acc_rays = dev_alloc<uint32_t>(d.owned, d.fb_rows * c.nx);
    }
    HIP_CHECK(hipSetDevice(current));
    const int first = c.prog_samples;
    render_frame(first + ns, first, true);
    c.prog_samples = first + ns;
}

int rtProgressiveSamples(void) { return g_ctx.prog_samples; }

void rtResetProgressive(void) { g_ctx.prog_samples = 0; }

void setCamera(const rt_camera* cam) {
    RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("setCamera before init");
    if (!cam) rt_fail("setCamera: null");
    if (memcmp(&c.cam, cam, sizeof(rt_camera)) != 0) c.camera_moves++;      // (the cost maps of sphere frames: cost_key_of)
    c.cam = *cam;                                           // read by every frame's parameter block; nothing of the scene depends on it
    c.prog_samples = 0;
    reset_refine();
}

// Scene edits (rt_api.h, "editing the scene").  Each call leaves every in-process device and the host mirrors with what a fresh init* of the
// edited scene would have built, resets the progressive frame and retires the sphere cost maps; nothing else a frame or a pass left behind is touched.
static void check_update(const char* fn, bool spheres) {
    const RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail(" before init", fn);
    if (c.is_spheres != spheres) rt_fail(spheres ? " needs a sphere scene (initRendererSpheres)" : " needs a mesh scene (initRenderer)", fn);
}

// The refit of the mesh tree over the slots device `d` holds, on its stream (updateTriangles, rebuildBvh).
static void launch_refit(const DeviceState& d) {
    RtRefitParams q;
    q.slots = d.d_tris; q.nodes = reinterpret_cast<float*>(d.d_bvh); q.axis = d.d_bvh_axis; q.leaf_rec = d.d_leaf_tri;
    q.first_leaf = g_ctx.mesh.scene.first_leaf; q.nppl = g_ctx.mesh.scene.nppl;
    HIP_CHECK(rt_launch_refit(q, d.stream));
}

static void scene_edited() {
    g_ctx.prog_samples = 0;                                 // as setCamera
    reset_refine();
    g_ctx.scene_edits++;                                    // (the cost maps of sphere frames: cost_key_of)
}

void updateTriangles(int first, int count, const rt_triangle* tris) {
    RenderContext& c = g_ctx;
    check_update("updateTriangles", false);
    if (first < 0 || count < 0 || (size_t)first + (size_t)count > c.mesh.tris.size()) rt_fail("updateTriangles: [first, first + count) must lie inside the numTris of init");
    if (count == 0) return;
    if (!tris) rt_fail("updateTriangles: tris is null");
    const uint32_t first_leaf = c.mesh.scene.first_leaf;
    if ((first_leaf & (first_leaf - 1)) != 0) rt_fail("updateTriangles: the refit needs a tree whose number of leaves is a power of two");
    for (int k = 0; k < count; k++) {
        const bool sentinel = std::isinf(tris[k].v[0].e[0]);
        if (sentinel != std::isinf(c.mesh.tris[(size_t)first + k].v[0].e[0])) rt_fail("updateTriangles: a slot's sentinel state (isinf(v[0].x)) must not change");
        if (!sentinel && tris[k].meshID >= c.mesh.materials.size()) rt_fail("updateTriangles: triangle meshID out of range");
    }
    std::copy(tris, tris + count, c.mesh.tris.begin() + first);
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    for (DeviceState& d : c.devs) {                         // every device holds the whole scene: count * 64 bytes over the bus and one refit each
        HIP_CHECK(hipSetDevice(d.device));
        HIP_CHECK(hipMemcpyAsync(d.d_tris + first, c.mesh.tris.data() + first, (size_t)count * sizeof(rt_triangle), hipMemcpyHostToDevice, d.stream));
        HIP_CHECK(hipEventRecord(d.ev_upd_start, d.stream));
        launch_refit(d);
        HIP_CHECK(hipEventRecord(d.ev_upd_stop, d.stream));
    }
    rt_bvh_node root;                                       // the scene bounds become node 1's box
    HIP_CHECK(hipSetDevice(c.devs[0].device));
    HIP_CHECK(hipMemcpyAsync(&root, reinterpret_cast<const char*>(c.devs[0].d_bvh) + sizeof(rt_bvh_node), sizeof root, hipMemcpyDeviceToHost, c.devs[0].stream));
    const double ms_max = finish_devices(&DeviceState::ev_upd_start, &DeviceState::ev_upd_stop, false);
    HIP_CHECK(hipSetDevice(current));
    c.mesh.scene.bounds.min = root.a;
    c.mesh.scene.bounds.max = root.b;
    c.refit_stale = true;
    c.update_ms = ms_max;
    scene_edited();
}

void updateMaterials(const rt_material* materials, int n) {
    RenderContext& c = g_ctx;
    check_update("updateMaterials", false);
    if (!materials) rt_fail("updateMaterials: materials is null");
    if (n != (int)c.mesh.materials.size()) rt_fail("updateMaterials: n must be the numMaterials of init");
    for (int k = 0; k < n; k++)
        if (materials[k].texId != -1 && (materials[k].texId < 0 || materials[k].texId >= (int)c.mesh.tex.size())) rt_fail("updateMaterials: material texId out of range");
    c.mesh.materials.assign(materials, materials + n);
    c.mesh.scene.lean_ok = mesh_lean_ok(c.mesh.materials);
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    for (DeviceState& d : c.devs) {
        HIP_CHECK(hipSetDevice(d.device));
        if (n > 0) HIP_CHECK(hipMemcpy(d.d_materials, c.mesh.materials.data(), (size_t)n * sizeof(rt_material), hipMemcpyHostToDevice));
    }
    HIP_CHECK(hipSetDevice(current));
    scene_edited();
}

void updateSpheres(const rt_sphere* spheres, const rt_material* materials, int n) {
    RenderContext& c = g_ctx;
    check_update("updateSpheres", true);
    if (!spheres || !materials) rt_fail("updateSpheres: spheres and materials must not be null");
    if (n != c.sphere.scene.n) rt_fail("updateSpheres: n must be the n of init");
    build_sphere_scene("updateSpheres", spheres, materials, n);
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    for (DeviceState& d : c.devs) {
        HIP_CHECK(hipSetDevice(d.device));
        upload_sphere_arrays(d);
    }
    HIP_CHECK(hipSetDevice(current));
    scene_edited();
}

int getMeshBvh(rt_bvh_node* nodes, int cap, rt_bbox* bounds) {
    const RenderContext& c = g_ctx;
    check_update("getMeshBvh", false);
    const int count = (int)(2 * c.mesh.scene.first_leaf);
    const int n = std::min(count, std::max(cap, 0));
    if (n > 0 && !nodes) rt_fail("getMeshBvh: nodes is null");
    if (n > 0) {
        int current = 0;
        HIP_CHECK(hipGetDevice(&current));
        HIP_CHECK(hipSetDevice(c.devs[0].device));
        HIP_CHECK(hipMemcpy(nodes, c.devs[0].d_bvh, (size_t)n * sizeof(rt_bvh_node), hipMemcpyDeviceToHost));
        HIP_CHECK(hipSetDevice(current));
    }
    if (bounds) *bounds = c.mesh.scene.bounds;
    return count;
}

double rtLastUpdateMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastUpdateMs before init");
    return g_ctx.update_ms;
}

// rebuildBvh (rt_api.h, "editing the scene"): the level-synchronous build of rt_kernels_build.hip into the second slot buffer, the swap, the
// refit of the new slots.  The host counts the visible triangles in its mirror (the build's n), applies the permutation to the mirror and takes the leaf
// count bytes back; the nodes, the child-pair records and the leaf records stay on the devices until a relayout asks for them (fetch_refit).
void rebuildBvh(int32_t* old_slot) {
    RenderContext& c = g_ctx;
    check_update("rebuildBvh", false);
    RtMeshParams& mp = c.mesh.scene;
    const uint32_t first_leaf = mp.first_leaf, per_leaf = mp.nppl;
    if ((first_leaf & (first_leaf - 1)) != 0) rt_fail("rebuildBvh: the rebuild needs a tree whose number of leaves is a power of two");
    const size_t slots = (size_t)first_leaf * per_leaf, num_tris = c.mesh.tris.size();
    size_t n = 0;
    for (uint32_t leaf = 0; leaf < first_leaf; leaf++)
        for (uint32_t k = 0; k < per_leaf && !std::isinf(c.mesh.tris[(size_t)leaf * per_leaf + k].v[0].e[0]); k++) n++;
    if (n > (size_t)RT_REBUILD_MAX_TRIS) rt_fail("rebuildBvh: more than RT_REBUILD_MAX_TRIS visible triangles");
    const bool records = per_leaf <= 255;                   // as layout_mesh: after a rebuild the sentinels trail in every leaf
    const size_t words = rt_build_workspace_words((uint32_t)n, first_leaf);
    std::vector<int32_t> from(num_tris);
    if (records) c.mesh.leaf_ofs.assign(((size_t)first_leaf + 3) / 4, 0u);
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    for (DeviceState& d : c.devs) {
        HIP_CHECK(hipSetDevice(d.device));
        if (!d.d_tris_alt) d.d_tris_alt = dev_alloc<rt_triangle>(d.owned, num_tris);
        if (!d.d_old_slot) d.d_old_slot = dev_alloc<int32_t>(d.owned, num_tris);
        if (d.build_words != words) {
            dev_release(d.owned, d.d_build_work);
            d.d_build_work = dev_alloc<uint32_t>(d.owned, words);
            d.build_words = words;
        }
        if (records && !d.d_leaf_tri) d.d_leaf_tri = dev_alloc<float4>(d.owned, slots * 3);
        if (records && !d.d_leaf_ofs) d.d_leaf_ofs = dev_alloc<uint32_t>(d.owned, ((size_t)first_leaf + 3) / 4);
        RtBuildParams b;
        b.slots_in = d.d_tris; b.slots_out = d.d_tris_alt; b.old_slot = d.d_old_slot; b.leaf_ofs = records ? d.d_leaf_ofs : nullptr; b.work = d.d_build_work;
        b.num_tris = (uint32_t)num_tris; b.first_leaf = first_leaf; b.nppl = per_leaf; b.n = (uint32_t)n;
        HIP_CHECK(hipEventRecord(d.ev_reb_start, d.stream));
        HIP_CHECK(rt_launch_rebuild(b, d.stream));
        std::swap(d.d_tris, d.d_tris_alt);
        if (d.d_leaf_tri) HIP_CHECK(hipMemsetAsync(d.d_leaf_tri, 0, slots * 3 * sizeof(float4), d.stream));   // (the refit writes the real slots only)
        launch_refit(d);
        HIP_CHECK(hipEventRecord(d.ev_reb_stop, d.stream));
        if (&d == &c.devs[0] && g_pose.marked) {            // the marked pose follows the permutation: one gather, behind the timed kernels
            PoseState& m = g_pose;
            if (!m.d_mark_alt) m.d_mark_alt = dev_alloc<rt_triangle>(m.owned, num_tris);
            HIP_CHECK(rt_launch_motion_gather(m.d_mark, m.d_mark_alt, d.d_old_slot, (uint32_t)num_tris, d.stream));
            std::swap(m.d_mark, m.d_mark_alt);
        }
    }
    const DeviceState& d0 = c.devs[0];
    rt_bvh_node root;
    HIP_CHECK(hipSetDevice(d0.device));
    HIP_CHECK(hipMemcpyAsync(&root, reinterpret_cast<const char*>(d0.d_bvh) + sizeof(rt_bvh_node), sizeof root, hipMemcpyDeviceToHost, d0.stream));
    HIP_CHECK(hipMemcpyAsync(from.data(), d0.d_old_slot, num_tris * sizeof(int32_t), hipMemcpyDeviceToHost, d0.stream));
    if (records) HIP_CHECK(hipMemcpyAsync(c.mesh.leaf_ofs.data(), d0.d_leaf_ofs, c.mesh.leaf_ofs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, d0.stream));
    const double ms_max = finish_devices(&DeviceState::ev_reb_start, &DeviceState::ev_reb_stop, false);
    HIP_CHECK(hipSetDevice(current));
    permute_triangles(c.mesh, from);                        // the host mirror of the triangles follows the permutation
    if (records) c.mesh.leaf_tri.resize(slots * 3);         // (fetch_refit fills it)
    mp.leaf_sentinels_trailing = 1;
    mp.bounds.min = root.a;
    mp.bounds.max = root.b;
    c.refit_stale = true;
    c.rebuild_ms = ms_max;
    if (old_slot) std::copy(from.begin(), from.end(), old_slot);
    scene_edited();
}

double rtLastRebuildMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastRebuildMs before init");
    return g_ctx.rebuild_ms;
}

// First-hit guide planes (rt_api.h).  Its own kernels, device planes and timing: nothing of a frame's state (framebuffer, stats, launch report, progressive
// accumulation, queue words, counters) is read or written.
void renderGuides(int mask, float* albedo, float* normal, float* depth, int32_t* prim, int32_t* nodes) {
    RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("renderGuides before init");
    constexpr int kAll = RT_GUIDE_ALBEDO | RT_GUIDE_NORMAL | RT_GUIDE_DEPTH | RT_GUIDE_PRIM | RT_GUIDE_NODES;
    if (mask == 0 || (mask & ~kAll) != 0) rt_fail("renderGuides: mask must name at least one RT_GUIDE_* plane and no unknown bit");
    void* const host[5] = { albedo, normal, depth, prim, nodes };
    for (int k = 0; k < 5; k++)
        if ((mask >> k & 1) && !host[k]) rt_fail("renderGuides: a requested plane has a null pointer");
    if ((mask & RT_GUIDE_NODES) && c.is_spheres) rt_fail("renderGuides: RT_GUIDE_NODES is only defined for mesh scenes");
    if (c.is_spheres && c.opt.floor) rt_fail("renderGuides: the floor plane is only defined for mesh scenes (kernel_scene.floor)");
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    const int nd = (int)c.devs.size();
    for (int k = 0; k < nd; k++) {
        DeviceState& d = c.devs[k];
        if (d.fb_rows == 0) continue;
        HIP_CHECK(hipSetDevice(d.device));
        const RtPartition part = partition_of(k);
        void* plane[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
        for (int q = 0; q < 5; q++) {
            if (!(mask >> q & 1)) continue;
            if (!d.d_guide[q]) d.d_guide[q] = dev_alloc<char>(d.owned, d.fb_rows * c.nx * kGuideBytes[q]);
            plane[q] = d.d_guide[q];
        }
        const RtGuidePlanes g = { static_cast<float*>(plane[0]), static_cast<float*>(plane[1]), static_cast<float*>(plane[2]),
                                  static_cast<int32_t*>(plane[3]), static_cast<int32_t*>(plane[4]) };
        HIP_CHECK(hipEventRecord(d.ev_start, d.stream));
        launch_guides(d, part, g);
        HIP_CHECK(hipEventRecord(d.ev_stop, d.stream));
        for (int q = 0; q < 5; q++)
            if (plane[q]) deliver_stripes(d, part, static_cast<char*>(host[q]), static_cast<const char*>(plane[q]), kGuideBytes[q]);
    }
    c.guides_ms = finish_devices(&DeviceState::ev_start, &DeviceState::ev_stop, true);      // blocking: the caller's arrays are complete on return
    HIP_CHECK(hipSetDevice(current));
}

double rtLastGuidesMs(void) { return g_ctx.guides_ms; }

// Batched ray queries (rt_api.h), through run_chunks: the four inputs (the bounds may be NULL) and the planes `out` names at kRayT.., the others NULL.
static void run_rays(int n, const float* org, const float* dir, const float* t_min, const float* t_max, void* const out[kRayBuffers], bool any) {
    RenderContext& c = g_ctx;
    const DeviceState& d = c.devs[0];
    static const ChunkBuffer table[kRayBuffers] = { { 12, kUp }, { 12, kUp }, { 4, kUp }, { 4, kUp }, { 4, kDown }, { 4, kDown }, { 12, kDown }, { 8, kDown },
                                                    { 4, kDown }, { 1, kDown } };
    void* host[kRayBuffers] = { const_cast<float*>(org), const_cast<float*>(dir), const_cast<float*>(t_min), const_cast<float*>(t_max) };
    std::copy(out + kRayT, out + kRayBuffers, host + kRayT);
    c.rays_ms = run_chunks(g_rays, (size_t)n, kRayChunk, table, kRayBuffers, host, false, [&](char* const* dev, size_t m) {
        auto in = [&](int k) { return reinterpret_cast<const float*>(dev[k]); };
        RtRayBatch b;
        b.org = in(kRayOrg); b.dir = in(kRayDir); b.t_min = in(kRayTMin); b.t_max = in(kRayTMax);
        b.t = reinterpret_cast<float*>(dev[kRayT]); b.prim = reinterpret_cast<int32_t*>(dev[kRayPrim]);
        b.normal = reinterpret_cast<float*>(dev[kRayNormal]); b.uv = reinterpret_cast<float*>(dev[kRayUv]);
        b.nodes = reinterpret_cast<int32_t*>(dev[kRayNodes]); b.occluded = reinterpret_cast<uint8_t*>(dev[kRayOccluded]);
        b.n = (int32_t)m;
        b.t_min_default = c.opt.t_min;
        launch_rays(d, b, any);
    });
}

// The checks the two calls share; returns false for the empty batch (nothing to do, nothing written).
static bool check_rays(const char* fn, int n, const float* org, const float* dir) {
    const RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail(" before init", fn);
    if (n < 0) rt_fail(": n is negative", fn);
    if (n == 0) return false;
    if (!org || !dir) rt_fail(": org and dir must not be null", fn);
    if (c.is_spheres && c.opt.floor) rt_fail(": the floor plane is only defined for mesh scenes (kernel_scene.floor)", fn);
    return true;
}

void traceRays(int n, const float* org, const float* dir, const float* t_min, const float* t_max, int mask,
               float* t, int32_t* prim, float* normal, float* uv, int32_t* nodes) {
    if (!check_rays("traceRays", n, org, dir)) return;
    constexpr int kAll = RT_RAY_T | RT_RAY_PRIM | RT_RAY_NORMAL | RT_RAY_UV | RT_RAY_NODES;
    if (mask == 0 || (mask & ~kAll) != 0) rt_fail("traceRays: mask must name at least one RT_RAY_* plane and no unknown bit");
    void* const planes[5] = { t, prim, normal, uv, nodes };
    for (int k = 0; k < 5; k++)
        if ((mask >> k & 1) && !planes[k]) rt_fail("traceRays: a requested plane has a null pointer");
    if ((mask & RT_RAY_NODES) && g_ctx.is_spheres) rt_fail("traceRays: RT_RAY_NODES is only defined for mesh scenes");
    void* out[kRayBuffers] = {};
    for (int k = 0; k < 5; k++) out[kRayT + k] = (mask >> k & 1) ? planes[k] : nullptr;
    run_rays(n, org, dir, t_min, t_max, out, false);
}

void occludedRays(int n, const float* org, const float* dir, const float* t_min, const float* t_max, uint8_t* occluded) {
    if (!g_ctx.initialised) rt_fail("occludedRays before init");
    if (!occluded) rt_fail("occludedRays: occluded is null");
    if (!check_rays("occludedRays", n, org, dir)) return;
    void* out[kRayBuffers] = {};
    out[kRayOccluded] = occluded;
    run_rays(n, org, dir, t_min, t_max, out, true);
}

double rtLastRaysMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastRaysMs before init");
    return g_ctx.rays_ms;
}

// A list of pixels (rt_api.h), through run_chunks with the queue word of the pixel kernels.  host[k] = the caller's array of buffer k, or NULL.
static void run_pixels(int n, int ns_all, void* const host[kPixBuffers]) {
    const int state_dir = host[kPixFirst] ? kUp | kDown : kDown;    // (the states go up only where an entry can continue one: `first` is given)
    const ChunkBuffer table[kPixBuffers] = { { 8, kUp }, { 4, kUp }, { 4, kUp }, { 16, state_dir }, { 12, kDown }, { 4, kDown } };
    const int max_waves = rt_read_switches().pixels_waves;
    g_ctx.pixels_ms = run_chunks(g_pixels, (size_t)n, kPixelChunk, table, kPixBuffers, host, true, [&](char* const* dev, size_t m) {
        RtPixelBatch b;
        b.ij = reinterpret_cast<const int32_t*>(dev[kPixIj]); b.ns = reinterpret_cast<const int32_t*>(dev[kPixNs]);
        b.first = reinterpret_cast<const int32_t*>(dev[kPixFirst]); b.state = reinterpret_cast<uint32_t*>(dev[kPixState]);
        b.out = reinterpret_cast<rt_vec3*>(dev[kPixOut]); b.rays = reinterpret_cast<uint32_t*>(dev[kPixRays]);
        b.queue = g_pixels.d_queue; b.n = (int32_t)m; b.ns_all = ns_all;
        launch_pixels(g_ctx.devs[0], b, max_waves);
    });
}

void renderPixels(int n, const int32_t* ij, int ns_all, const int32_t* ns, const int32_t* first, uint32_t* state, rt_vec3* out, uint32_t* rays) {
    const RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("renderPixels before init");
    if (n < 0) rt_fail("renderPixels: n is negative");
    if (n == 0) return;
    if (!ij) rt_fail("renderPixels: ij is null");
    if (!out && !state && !rays) rt_fail("renderPixels: out, state and rays are all null");
    if (first && !state) rt_fail("renderPixels: first needs state (the sums and stream words the pixels resume from)");
    check_per_pixel("renderPixels");
    for (int k = 0; k < n; k++) {                           // every entry, before anything is uploaded
        const long long cnt = ns ? ns[k] : ns_all, f = first ? first[k] : 0;
        if (ij[2 * (size_t)k] < 0 || ij[2 * (size_t)k] >= c.nx || ij[2 * (size_t)k + 1] < 0 || ij[2 * (size_t)k + 1] >= c.ny)
            rt_fail("renderPixels: a pixel lies outside [0, nx) x [0, ny)");
        if (cnt < 1) rt_fail("renderPixels: a pixel's sample count is below 1");
        if (f < 0) rt_fail("renderPixels: a pixel's first sample is negative");
        if (f + cnt > RT_PROGRESSIVE_MAX_SAMPLES) rt_fail("renderPixels: first + count above RT_PROGRESSIVE_MAX_SAMPLES");
        // (a pixel's seed is odd and xorshift32 never reaches 0 from it: a zero word is no state of any stream - and the one input on which the stream
        // stands still, so that the rejection loops of the lens and the diffuse bounce would never end on the device)
        if (f > 0 && state[4 * (size_t)k + 3] == 0u) rt_fail("renderPixels: a resumed pixel's stream word is 0 (not a state renderPixels returned)");
    }
    void* const host[kPixBuffers] = { const_cast<int32_t*>(ij), const_cast<int32_t*>(ns), const_cast<int32_t*>(first), state, out, rays };
    run_pixels(n, ns_all, host);
}

double rtLastPixelsMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastPixelsMs before init");
    return g_ctx.pixels_ms;
}

// A list of the caller's own rays (rt_api.h), through run_chunks with the queue word of the radiance kernels: RT_RAY_CHUNK rays at a time, 68
// bytes per ray.  host[k] = the caller's array of buffer k, or NULL.  A ray without ids is seeded by its index in the caller's list: the chunk's first index
// goes with the batch.
static void run_radiance(int n, int ns_all, void* const host[kRadBuffers]) {
    const int state_dir = host[kRadFirst] ? kUp | kDown : kDown;    // (the states go up only where an entry can continue one: `first` is given)
    const ChunkBuffer table[kRadBuffers] = { { 12, kUp }, { 12, kUp }, { 4, kUp }, { 4, kUp }, { 4, kUp }, { 16, state_dir }, { 12, kDown }, { 4, kDown } };
    const int max_waves = rt_read_switches().pixels_waves;
    size_t done = 0;                                        // rays of the chunks launched so far
    g_ctx.radiance_ms = run_chunks(g_radiance, (size_t)n, kRayChunk, table, kRadBuffers, host, true, [&](char* const* dev, size_t m) {
        RtRadianceBatch b;
        b.org = reinterpret_cast<const float*>(dev[kRadOrg]); b.dir = reinterpret_cast<const float*>(dev[kRadDir]);
        b.ids = reinterpret_cast<const uint32_t*>(dev[kRadIds]); b.ns = reinterpret_cast<const int32_t*>(dev[kRadNs]);
        b.first = reinterpret_cast<const int32_t*>(dev[kRadFirst]); b.state = reinterpret_cast<uint32_t*>(dev[kRadState]);
        b.out = reinterpret_cast<rt_vec3*>(dev[kRadOut]); b.rays = reinterpret_cast<uint32_t*>(dev[kRadRays]);
        b.queue = g_radiance.d_queue; b.n = (int32_t)m; b.ns_all = ns_all; b.id0 = (uint32_t)done;
        launch_radiance(g_ctx.devs[0], b, max_waves);
        done += m;
    });
}

void radianceRays(int n, const float* org, const float* dir, const uint32_t* ids, int ns_all, const int32_t* ns, const int32_t* first, uint32_t* state,
                  rt_vec3* out, uint32_t* rays) {
    const RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("radianceRays before init");
    if (n < 0) rt_fail("radianceRays: n is negative");
    if (n == 0) return;
    if (!org || !dir) rt_fail("radianceRays: org and dir must not be null");
    if (!out && !state && !rays) rt_fail("radianceRays: out, state and rays are all null");
    if (first && !state) rt_fail("radianceRays: first needs state (the sums and stream words the rays resume from)");
    check_per_pixel("radianceRays");
    for (int k = 0; k < n; k++) {                           // every entry, before anything is uploaded
        const long long cnt = ns ? ns[k] : ns_all, f = first ? first[k] : 0;
        if (cnt < 1) rt_fail("radianceRays: a ray's sample count is below 1");
        if (f < 0) rt_fail("radianceRays: a ray's first sample is negative");
        if (f + cnt > RT_PROGRESSIVE_MAX_SAMPLES) rt_fail("radianceRays: first + count above RT_PROGRESSIVE_MAX_SAMPLES");
        // (a zero word is no state of any stream, and the one on which the rejection loops would never end on the device: renderPixels)
        if (f > 0 && state[4 * (size_t)k + 3] == 0u) rt_fail("radianceRays: a resumed ray's stream word is 0 (not a state radianceRays returned)");
    }
    void* const host[kRadBuffers] = { const_cast<float*>(org), const_cast<float*>(dir), const_cast<uint32_t*>(ids), const_cast<int32_t*>(ns),
                                      const_cast<int32_t*>(first), state, out, rays };
    run_radiance(n, ns_all, host);
}

double rtLastRadianceMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastRadianceMs before init");
    return g_ctx.radiance_ms;
}

// Gathering at points (rt_api.h).  Per chunk of max(1, RT_RAY_CHUNK / dirs) points: pos / nrm (and acc where first > 0) go up, k_gather_dirs
// fills the batch arrays, the radiance kernels (launch_radiance) or the any-hit kernels (launch_rays) run over them, k_gather_reduce folds them per point, and
// acc / out / rays come down.  No per-ray datum crosses the bus.  Nothing of a frame's, a pass's, radianceRays' or the ray queries' state is read or written.
static int gather_width(int mode) {
    return mode == RT_GATHER_IRRADIANCE ? 3 : mode == RT_GATHER_SH9 ? 27 : mode == RT_GATHER_VISIBILITY ? 1 : 0;
}

int rtGatherWidth(int mode) {
    const int w = gather_width(mode);
    if (w == 0) rt_fail("rtGatherWidth: unknown mode");
    return w;
}

// The checks gatherRadiance and rtGatherDirections share, under the function's name `fn`; returns false for the empty list (nothing to do, nothing written).
static bool check_gather(const char* fn, int n, const float* pos, const float* nrm, int mode, int first, int dirs, int dirs_total, float bias) {
    const RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail(" before init", fn);
    if (n < 0) rt_fail(": n is negative", fn);
    if (n == 0) return false;
    if (!pos) rt_fail(": pos is null", fn);
    if (gather_width(mode) == 0) rt_fail(": unknown mode", fn);
    if (mode != RT_GATHER_SH9 && !nrm) rt_fail(": nrm is null (only RT_GATHER_SH9 ignores it)", fn);
    if (dirs < 1 || first < 0) rt_fail(": dirs must be at least 1 and first not negative", fn);
    if (dirs_total > RT_GATHER_MAX_DIRS) rt_fail(": dirs_total above RT_GATHER_MAX_DIRS", fn);
    if ((long long)first + dirs > dirs_total) rt_fail(": first + dirs above dirs_total", fn);
    if (!std::isfinite(bias)) rt_fail(": bias is not finite", fn);
    if (c.is_spheres && c.opt.floor) rt_fail(": the floor plane is only defined for mesh scenes (kernel_scene.floor)", fn);
    return true;
}

// Buffer k of the gather state, grown to `bytes`.
static char* gather_buffer(int k, size_t bytes) {
    return grown_buffer(g_gather, k, bytes);
}

// The parameter block of chunk [k0, k0 + pts) with the per-point inputs uploaded and the per-ray arrays `want` names (-1: none) allocated; the rest is nullptr.
static RtGatherParams gather_chunk(size_t k0, size_t pts, const float* pos, const float* nrm, int mode, int first, int dirs, int dirs_total, uint32_t base_id,
                                   float bias, std::initializer_list<int> want, hipStream_t stream) {
    const size_t nray = pts * (size_t)dirs;
    static const size_t ray_bytes[kGatBuffers] = { 0, 0, 0, 0, 0, 12, 12, 4, 4, 12, 4, 1 };
    char* dev[kGatBuffers] = {};
    for (int k : want)
        if (k >= 0) dev[k] = gather_buffer(k, nray * ray_bytes[k]);
    RtGatherParams p = {};
    float* d_pos = reinterpret_cast<float*>(gather_buffer(kGatPos, pts * 12));
    HIP_CHECK(hipMemcpyAsync(d_pos, pos + 3 * k0, pts * 12, hipMemcpyHostToDevice, stream));
    p.pos = d_pos;
    if (mode != RT_GATHER_SH9) {
        float* d_nrm = reinterpret_cast<float*>(gather_buffer(kGatNrm, pts * 12));
        HIP_CHECK(hipMemcpyAsync(d_nrm, nrm + 3 * k0, pts * 12, hipMemcpyHostToDevice, stream));
        p.nrm = d_nrm;
    }
    p.org = reinterpret_cast<float*>(dev[kGatOrg]); p.dir = reinterpret_cast<float*>(dev[kGatDir]);
    p.ids = reinterpret_cast<uint32_t*>(dev[kGatIds]); p.t_max = reinterpret_cast<float*>(dev[kGatTMax]);
    p.L = reinterpret_cast<rt_vec3*>(dev[kGatL]); p.rays = reinterpret_cast<uint32_t*>(dev[kGatRays]);
    p.occluded = reinterpret_cast<uint8_t*>(dev[kGatOccluded]);
    p.pts = (uint32_t)pts; p.dirs = (uint32_t)dirs; p.first = (uint32_t)first; p.dirs_total = (uint32_t)dirs_total;
    p.k0 = (uint32_t)k0; p.base_id = base_id; p.mode = mode; p.bias = bias;
    return p;
}

void gatherRadiance(int n, const float* pos, const float* nrm, int mode, int first, int dirs, int dirs_total, int ns, uint32_t base_id, float bias, float max_dist,
                    float* acc, float* out, uint32_t* rays) {
    RenderContext& c = g_ctx;
    if (!check_gather("gatherRadiance", n, pos, nrm, mode, first, dirs, dirs_total, bias)) return;
    if (first > 0 && !acc) rt_fail("gatherRadiance: first > 0 needs acc (the sums the points resume from)");
    if (!acc && !out && !rays) rt_fail("gatherRadiance: acc, out and rays are all null");
    if (std::isnan(max_dist) || max_dist < 0.0f) rt_fail("gatherRadiance: max_dist must not be a NaN or negative");
    const bool vis = mode == RT_GATHER_VISIBILITY;
    if (!vis) {
        if (ns < 1 || ns > RT_PROGRESSIVE_MAX_SAMPLES) rt_fail("gatherRadiance: ns must be 1 .. RT_PROGRESSIVE_MAX_SAMPLES");
        check_per_pixel("gatherRadiance");
    }
    GatherState& q = g_gather;
    const DeviceState& d = c.devs[0];
    const size_t W = (size_t)gather_width(mode), chunk = std::max<size_t>(1, kRayChunk / (size_t)dirs);
    const int max_waves = rt_read_switches().pixels_waves;
    const int current = begin_query(q);
    if (!q.d_queue) q.d_queue = dev_alloc<uint32_t>(q.owned, 1);
    double ms_sum = 0.0;
    for_chunks((size_t)n, chunk, [&](size_t k0, size_t pts) {
        RtGatherParams p = vis ? gather_chunk(k0, pts, pos, nrm, mode, first, dirs, dirs_total, base_id, bias, { kGatOrg, kGatDir, kGatTMax, kGatOccluded }, d.stream)
                               : gather_chunk(k0, pts, pos, nrm, mode, first, dirs, dirs_total, base_id, bias, { kGatOrg, kGatDir, kGatIds, kGatL, kGatRays }, d.stream);
        p.t_max_value = max_dist > 0.0f ? max_dist : FLT_MAX;
        if (acc || first > 0) p.acc = reinterpret_cast<float*>(gather_buffer(kGatAcc, pts * W * 4));
        if (out) p.out = reinterpret_cast<float*>(gather_buffer(kGatOut, pts * W * 4));
        if (rays) p.nrays = reinterpret_cast<uint32_t*>(gather_buffer(kGatNrays, pts * 4));
        if (first > 0) HIP_CHECK(hipMemcpyAsync(p.acc, acc + k0 * W, pts * W * 4, hipMemcpyHostToDevice, d.stream));
        HIP_CHECK(hipEventRecord(q.ev_start, d.stream));
        HIP_CHECK(rt_launch_gather_dirs(p, d.stream));
        if (vis) {
            RtRayBatch b = {};
            b.org = p.org; b.dir = p.dir; b.t_max = p.t_max; b.occluded = p.occluded;
            b.n = (int32_t)(pts * (size_t)dirs);
            b.t_min_default = c.opt.t_min;
            launch_rays(d, b, true);
        } else {
            HIP_CHECK(hipMemsetAsync(q.d_queue, 0, sizeof(uint32_t), d.stream));
            RtRadianceBatch b = {};
            b.org = p.org; b.dir = p.dir; b.ids = p.ids;
            b.out = p.L; b.rays = p.rays;
            b.queue = q.d_queue; b.n = (int32_t)(pts * (size_t)dirs); b.ns_all = ns;
            launch_radiance(d, b, max_waves);
        }
        HIP_CHECK(rt_launch_gather_reduce(p, d.stream));
        HIP_CHECK(hipEventRecord(q.ev_stop, d.stream));
        if (acc) HIP_CHECK(hipMemcpyAsync(acc + k0 * W, p.acc, pts * W * 4, hipMemcpyDeviceToHost, d.stream));
        if (out) HIP_CHECK(hipMemcpyAsync(out + k0 * W, p.out, pts * W * 4, hipMemcpyDeviceToHost, d.stream));
        if (rays) HIP_CHECK(hipMemcpyAsync(rays + k0, p.nrays, pts * 4, hipMemcpyDeviceToHost, d.stream));
        HIP_CHECK(hipStreamSynchronize(d.stream));              // (the events are read per chunk; blocking: the caller's arrays are complete on return)
        ms_sum += query_ms(q);
    });
    end_query(current);
    c.gather_ms = ms_sum;
}

void rtGatherDirections(int n, const float* pos, const float* nrm, int mode, int first, int dirs, int dirs_total, uint32_t base_id, float bias,
                        float* org, float* dir, uint32_t* ids) {
    if (!check_gather("rtGatherDirections", n, pos, nrm, mode, first, dirs, dirs_total, bias)) return;
    if (!org && !dir && !ids) rt_fail("rtGatherDirections: org, dir and ids are all null");
    GatherState& q = g_gather;
    const DeviceState& d = g_ctx.devs[0];
    const size_t chunk = std::max<size_t>(1, kRayChunk / (size_t)dirs);
    const int current = begin_query(q);
    for_chunks((size_t)n, chunk, [&](size_t k0, size_t pts) {
        RtGatherParams p = gather_chunk(k0, pts, pos, nrm, mode, first, dirs, dirs_total, base_id, bias,
                                              { org ? kGatOrg : -1, dir ? kGatDir : -1, ids ? kGatIds : -1 }, d.stream);
        HIP_CHECK(rt_launch_gather_dirs(p, d.stream));
        const size_t e0 = k0 * (size_t)dirs, m = pts * (size_t)dirs;
        if (org) HIP_CHECK(hipMemcpyAsync(org + 3 * e0, p.org, m * 12, hipMemcpyDeviceToHost, d.stream));
        if (dir) HIP_CHECK(hipMemcpyAsync(dir + 3 * e0, p.dir, m * 12, hipMemcpyDeviceToHost, d.stream));
        if (ids) HIP_CHECK(hipMemcpyAsync(ids + e0, p.ids, m * 4, hipMemcpyDeviceToHost, d.stream));
        HIP_CHECK(hipStreamSynchronize(d.stream));
    });
    end_query(current);
}

double rtLastGatherMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastGatherMs before init");
    return g_ctx.gather_ms;
}

// Baking texels (rt_api.h).  The raster runs over the first device's live slots: coverage, resolve, `dilate` dilation launches, the scan of the
// workgroup counts - then the one word that crosses the bus before the planes do, the length of the list - and, for a bake, the compaction.  A bake goes on
// chunk by chunk over the compact list as gatherRadiance goes over the caller's: k_texel_dirs fills the batch arrays, the radiance kernels (launch_radiance) or
// the any-hit kernels (launch_rays) run over them, k_gather_reduce folds them per list entry; the scatter writes the texel planes, which come down.  Nothing
// of a frame's, a pass's, gatherRadiance's or the other queries' state is read or written.
static char* texel_buffer(TexelState& q, int k, size_t bytes) {
    return grown_buffer(q, k, std::max<size_t>(bytes, 4));
}
static char* texel_buffer(int k, size_t bytes) { return texel_buffer(g_texels, k, bytes); }

static void check_texels(const char* fn, int W, int H, int dilate) {
    const RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail(" before init", fn);
    if (c.is_spheres) rt_fail(": only a mesh scene has a UV atlas", fn);
    if (W < 1 || H < 1 || W > RT_TEXEL_MAX_SIZE || H > RT_TEXEL_MAX_SIZE) rt_fail(": W and H must be 1 .. RT_TEXEL_MAX_SIZE", fn);
    if (dilate < 0 || dilate > RT_TEXEL_MAX_DILATE) rt_fail(": dilate must be 0 .. RT_TEXEL_MAX_DILATE", fn);
}

// The raster's kernels on the query's device (begin_query has run): the planes `want_*` name, src after `dilate` iterations in src[dilate & 1], and with
// `with_list` rank, list, list_pos and list_nrm, in the buffers and between the events of `q`.  *length = the owned texels, *ms_out the HIP-event time of the
// kernels.  Returns the block.
static RtTexelParams texel_raster(TexelState& q, double* ms_out, int W, int H, int dilate, bool want_prim, bool want_bary, bool want_pos, bool want_nrm,
                                  bool with_list, uint32_t* length) {
    RenderContext& c = g_ctx;
    const DeviceState& d = c.devs[0];
    const size_t n = (size_t)W * H;
    RtTexelParams p = {};
    p.slots = d.d_tris; p.num_slots = (uint32_t)c.mesh.tris.size();
    p.W = W; p.H = H;
    p.owner = reinterpret_cast<int32_t*>(texel_buffer(q, kTexOwner, n * 4));
    p.src[0] = reinterpret_cast<int32_t*>(texel_buffer(q, kTexSrc0, n * 4));
    if (dilate > 0) p.src[1] = reinterpret_cast<int32_t*>(texel_buffer(q, kTexSrc1, n * 4));
    if (want_prim) p.prim = reinterpret_cast<int32_t*>(texel_buffer(q, kTexPrim, n * 4));
    if (want_bary) p.bary = reinterpret_cast<float*>(texel_buffer(q, kTexBary, n * 8));
    if (want_pos) p.pos = reinterpret_cast<float*>(texel_buffer(q, kTexPos, n * 12));
    if (want_nrm) p.nrm = reinterpret_cast<float*>(texel_buffer(q, kTexNrm, n * 12));
    p.blocks = (uint32_t)((n + kTexelBlock - 1) / kTexelBlock);
    p.counts = reinterpret_cast<uint32_t*>(texel_buffer(q, kTexCounts, (size_t)p.blocks * 4));
    if (!q.d_length) q.d_length = dev_alloc<uint32_t>(q.owned, 1);
    p.length = q.d_length;
    HIP_CHECK(hipEventRecord(q.ev_start, d.stream));
    HIP_CHECK(rt_launch_texel_coverage(p, d.stream));
    HIP_CHECK(rt_launch_texel_resolve(p, d.stream));
    for (int i = 1; i <= dilate; i++) HIP_CHECK(rt_launch_texel_dilate(p, i, d.stream));
    HIP_CHECK(rt_launch_texel_scan(p, d.stream));
    HIP_CHECK(hipEventRecord(q.ev_stop, d.stream));
    HIP_CHECK(hipMemcpyAsync(length, q.d_length, sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
    HIP_CHECK(hipStreamSynchronize(d.stream));
    double ms = query_ms(q);
    if (with_list) {
        p.rank = reinterpret_cast<int32_t*>(texel_buffer(q, kTexRank, n * 4));
        p.list = reinterpret_cast<uint32_t*>(texel_buffer(q, kTexList, (size_t)*length * 4));
        p.list_pos = reinterpret_cast<float*>(texel_buffer(q, kTexListPos, (size_t)*length * 12));
        p.list_nrm = reinterpret_cast<float*>(texel_buffer(q, kTexListNrm, (size_t)*length * 12));
        HIP_CHECK(hipEventRecord(q.ev_start, d.stream));
        HIP_CHECK(rt_launch_texel_compact(p, d.stream));
        HIP_CHECK(hipEventRecord(q.ev_stop, d.stream));
        HIP_CHECK(hipStreamSynchronize(d.stream));
        ms += query_ms(q);
    }
    *ms_out = ms;
    return p;
}

int rasterTexels(int W, int H, int dilate, int32_t* prim, int32_t* src, float* bary, float* pos, float* nrm) {
    check_texels("rasterTexels", W, H, dilate);
    if (!prim && !src && !bary && !pos && !nrm) rt_fail("rasterTexels: prim, src, bary, pos and nrm are all null");
    TexelState& q = g_texels;
    const DeviceState& d = g_ctx.devs[0];
    const size_t n = (size_t)W * H;
    const int current = begin_query(q);
    uint32_t length = 0;
    const RtTexelParams p = texel_raster(q, &g_ctx.texels_ms, W, H, dilate, prim != nullptr, bary != nullptr, pos != nullptr, nrm != nullptr, false, &length);
    if (prim) HIP_CHECK(hipMemcpyAsync(prim, p.prim, n * 4, hipMemcpyDeviceToHost, d.stream));
    if (src) HIP_CHECK(hipMemcpyAsync(src, p.src[dilate & 1], n * 4, hipMemcpyDeviceToHost, d.stream));
    if (bary) HIP_CHECK(hipMemcpyAsync(bary, p.bary, n * 8, hipMemcpyDeviceToHost, d.stream));
    if (pos) HIP_CHECK(hipMemcpyAsync(pos, p.pos, n * 12, hipMemcpyDeviceToHost, d.stream));
    if (nrm) HIP_CHECK(hipMemcpyAsync(nrm, p.nrm, n * 12, hipMemcpyDeviceToHost, d.stream));
    HIP_CHECK(hipStreamSynchronize(d.stream));
    end_query(current);
    return (int)length;
}

int bakeTexels(int W, int H, int dilate, int mode, int first, int dirs, int dirs_total, int ns, uint32_t base_id, float bias, float max_dist,
               float* acc, float* out, uint32_t* rays, int32_t* prim, int32_t* src) {
    RenderContext& c = g_ctx;
    check_texels("bakeTexels", W, H, dilate);
    static const float unit_z[3] = { 0.0f, 0.0f, 1.0f };            // (the points are the raster's: what check_gather asks of a list holds)
    check_gather("bakeTexels", 1, unit_z, unit_z, mode, first, dirs, dirs_total, bias);
    if (first > 0 && !acc) rt_fail("bakeTexels: first > 0 needs acc (the sums the texels resume from)");
    if (!acc && !out && !rays) rt_fail("bakeTexels: acc, out and rays are all null");
    if (std::isnan(max_dist) || max_dist < 0.0f) rt_fail("bakeTexels: max_dist must not be a NaN or negative");
    const bool vis = mode == RT_GATHER_VISIBILITY;
    if (!vis) {
        if (ns < 1 || ns > RT_PROGRESSIVE_MAX_SAMPLES) rt_fail("bakeTexels: ns must be 1 .. RT_PROGRESSIVE_MAX_SAMPLES");
        check_per_pixel("bakeTexels");
    }
    TexelState& q = g_texels;
    const DeviceState& d = c.devs[0];
    const size_t n = (size_t)W * H, Wd = (size_t)gather_width(mode), chunk = std::max<size_t>(1, kRayChunk / (size_t)dirs);
    const int max_waves = rt_read_switches().pixels_waves;
    const int current = begin_query(q);
    if (!q.d_queue) q.d_queue = dev_alloc<uint32_t>(q.owned, 1);
    uint32_t length = 0;
    const RtTexelParams p = texel_raster(q, &c.texels_ms, W, H, dilate, prim != nullptr, false, false, false, true, &length);
    RtTexelBakeParams b = {};
    b.src = p.src[dilate & 1]; b.rank = p.rank; b.list = p.list;
    b.length = length; b.texels = (uint32_t)n; b.Wd = (int32_t)Wd;
    if (acc) {
        b.acc_plane = reinterpret_cast<float*>(texel_buffer(kTexAccPlane, n * Wd * 4));
        b.acc = reinterpret_cast<float*>(texel_buffer(kTexAcc, (size_t)length * Wd * 4));
    }
    if (out) {
        b.out_plane = reinterpret_cast<float*>(texel_buffer(kTexOutPlane, n * Wd * 4));
        b.out = reinterpret_cast<float*>(texel_buffer(kTexOut, (size_t)length * Wd * 4));
    }
    if (rays) {
        b.rays_plane = reinterpret_cast<uint32_t*>(texel_buffer(kTexRaysPlane, n * 4));
        b.nrays = reinterpret_cast<uint32_t*>(texel_buffer(kTexNrays, (size_t)length * 4));
    }
    double ms_sum = 0.0;
    if (first > 0) {
        HIP_CHECK(hipMemcpyAsync(b.acc_plane, acc, n * Wd * 4, hipMemcpyHostToDevice, d.stream));
        HIP_CHECK(hipEventRecord(q.ev_start, d.stream));
        HIP_CHECK(rt_launch_texel_fetch(b, d.stream));
        HIP_CHECK(hipEventRecord(q.ev_stop, d.stream));
        HIP_CHECK(hipStreamSynchronize(d.stream));
        ms_sum += query_ms(q);
    }
    for_chunks((size_t)length, chunk, [&](size_t k0, size_t pts) {
        const size_t nray = pts * (size_t)dirs;
        RtGatherParams g = {};
        g.pos = p.list_pos + 3 * k0; g.nrm = p.list_nrm + 3 * k0;
        if (b.acc) g.acc = b.acc + k0 * Wd;
        if (b.out) g.out = b.out + k0 * Wd;
        if (b.nrays) g.nrays = b.nrays + k0;
        g.org = reinterpret_cast<float*>(texel_buffer(kTexOrg, nray * 12)); g.dir = reinterpret_cast<float*>(texel_buffer(kTexDir, nray * 12));
        if (vis) {
            g.t_max = reinterpret_cast<float*>(texel_buffer(kTexTMax, nray * 4)); g.occluded = reinterpret_cast<uint8_t*>(texel_buffer(kTexOccluded, nray));
        } else {
            g.ids = reinterpret_cast<uint32_t*>(texel_buffer(kTexIds, nray * 4)); g.L = reinterpret_cast<rt_vec3*>(texel_buffer(kTexL, nray * 12));
            g.rays = reinterpret_cast<uint32_t*>(texel_buffer(kTexRays, nray * 4));
        }
        g.pts = (uint32_t)pts; g.dirs = (uint32_t)dirs; g.first = (uint32_t)first; g.dirs_total = (uint32_t)dirs_total;
        g.k0 = (uint32_t)k0; g.base_id = base_id; g.mode = mode; g.bias = bias;
        g.t_max_value = max_dist > 0.0f ? max_dist : FLT_MAX;
        HIP_CHECK(hipEventRecord(q.ev_start, d.stream));
        HIP_CHECK(rt_launch_texel_dirs(g, p.list, d.stream));
        if (vis) {
            RtRayBatch r = {};
            r.org = g.org; r.dir = g.dir; r.t_max = g.t_max; r.occluded = g.occluded;
            r.n = (int32_t)nray;
            r.t_min_default = c.opt.t_min;
            launch_rays(d, r, true);
        } else {
            HIP_CHECK(hipMemsetAsync(q.d_queue, 0, sizeof(uint32_t), d.stream));
            RtRadianceBatch r = {};
            r.org = g.org; r.dir = g.dir; r.ids = g.ids;
            r.out = g.L; r.rays = g.rays;
            r.queue = q.d_queue; r.n = (int32_t)nray; r.ns_all = ns;
            launch_radiance(d, r, max_waves);
        }
        HIP_CHECK(rt_launch_gather_reduce(g, d.stream));
        HIP_CHECK(hipEventRecord(q.ev_stop, d.stream));
        HIP_CHECK(hipStreamSynchronize(d.stream));              // (the events are read per chunk)
        ms_sum += query_ms(q);
    });
    HIP_CHECK(hipEventRecord(q.ev_start, d.stream));
    HIP_CHECK(rt_launch_texel_scatter(b, d.stream));
    HIP_CHECK(hipEventRecord(q.ev_stop, d.stream));
    if (acc) HIP_CHECK(hipMemcpyAsync(acc, b.acc_plane, n * Wd * 4, hipMemcpyDeviceToHost, d.stream));
    if (out) HIP_CHECK(hipMemcpyAsync(out, b.out_plane, n * Wd * 4, hipMemcpyDeviceToHost, d.stream));
    if (rays) HIP_CHECK(hipMemcpyAsync(rays, b.rays_plane, n * 4, hipMemcpyDeviceToHost, d.stream));
    if (prim) HIP_CHECK(hipMemcpyAsync(prim, p.prim, n * 4, hipMemcpyDeviceToHost, d.stream));
    if (src) HIP_CHECK(hipMemcpyAsync(src, b.src, n * 4, hipMemcpyDeviceToHost, d.stream));
    HIP_CHECK(hipStreamSynchronize(d.stream));                  // blocking: the caller's planes are complete on return
    ms_sum += query_ms(q);
    end_query(current);
    c.bake_ms = ms_sum;
    q.out_W = out ? W : 0; q.out_H = out ? H : 0; q.out_mode = out ? mode : -1;    // (what filterTexels with in == NULL reads where it lies)
    return (int)length;
}

double rtLastTexelsMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastTexelsMs before init");
    return g_ctx.texels_ms;
}

double rtLastBakeMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastBakeMs before init");
    return g_ctx.bake_ms;
}

// Filtering texels (rt_api.h).  A raster of its own over the first device's live slots (texel_raster into g_filter: g_texels, its planes and
// rtLastTexelsMs stay what they were), then the prologue, one launch per iteration and the scatter through the dilated source plane.  The values go up from
// the caller's plane - or, with in == NULL, are read where the last bakeTexels left its out plane - and the filtered plane comes down.
int filterTexels(int W, int H, int dilate, int mode, const float* in, float* out, int iterations, int normal_squarings, float sigma_d, float sigma_z,
                 float sigma_c) {
    RenderContext& c = g_ctx;
    check_texels("filterTexels", W, H, dilate);
    if (mode != RT_GATHER_IRRADIANCE && mode != RT_GATHER_SH9 && mode != RT_GATHER_VISIBILITY) rt_fail("filterTexels: unknown mode");
    if (!out) rt_fail("filterTexels: out is null");
    if (iterations < 1 || iterations > RT_DENOISE_MAX_ITERATIONS) rt_fail("filterTexels: iterations must be 1 .. RT_DENOISE_MAX_ITERATIONS");
    if (normal_squarings < 0 || normal_squarings > RT_DENOISE_MAX_SQUARINGS) rt_fail("filterTexels: normal_squarings must be 0 .. RT_DENOISE_MAX_SQUARINGS");
    if (!std::isfinite(sigma_d) || sigma_d <= 0.0f) rt_fail("filterTexels: sigma_d must be finite and > 0");
    if (!std::isfinite(sigma_z) || sigma_z <= 0.0f) rt_fail("filterTexels: sigma_z must be finite and > 0");
    if (!std::isfinite(sigma_c)) rt_fail("filterTexels: sigma_c must be finite");
    const size_t n = (size_t)W * H, Wd = (size_t)gather_width(mode);
    if (!in && (g_texels.out_W < 1 || g_texels.out_W != W || g_texels.out_H != H || gather_width(g_texels.out_mode) != (int)Wd))
        rt_fail("filterTexels: in is null and the last bakeTexels left no out plane of this W, H and width");
    TexelState& q = g_filter;
    const DeviceState& d = c.devs[0];
    const int current = begin_query(q);
    uint32_t length = 0;
    double ms = 0.0;
    const RtTexelParams p = texel_raster(q, &ms, W, H, dilate, false, false, false, false, false, &length);
    RtTexelFilterParams f = {};
    f.slots = p.slots; f.owner = p.owner; f.src = p.src[dilate & 1];
    f.W = W; f.H = H; f.C = (int32_t)Wd;
    f.normal_squarings = normal_squarings;
    f.sigma_d = sigma_d; f.sigma_z = sigma_z; f.sigma_c = sigma_c;
    const size_t values = Wd == 1 ? n * 4 : n * (Wd / 3) * sizeof(float4);
    f.rec = reinterpret_cast<float4*>(texel_buffer(q, kFltRec, 2 * n * sizeof(float4)));
    f.col[0] = texel_buffer(q, kFltCol0, values);
    f.col[1] = texel_buffer(q, kFltCol1, values);
    f.out = reinterpret_cast<float*>(texel_buffer(q, kFltOut, n * Wd * 4));
    if (in) {
        float* d_in = reinterpret_cast<float*>(texel_buffer(q, kFltIn, n * Wd * 4));
        HIP_CHECK(hipMemcpyAsync(d_in, in, n * Wd * 4, hipMemcpyHostToDevice, d.stream));
        f.in = d_in;
    } else {
        f.in = reinterpret_cast<const float*>(g_texels.d_buf[kTexOutPlane]);
    }
    HIP_CHECK(hipEventRecord(q.ev_start, d.stream));
    HIP_CHECK(rt_launch_texel_filter_prologue(f, d.stream));
    for (int it = 0; it < iterations; it++) HIP_CHECK(rt_launch_texel_filter_iteration(f, it, d.stream));
    HIP_CHECK(rt_launch_texel_filter_scatter(f, iterations, d.stream));
    HIP_CHECK(hipEventRecord(q.ev_stop, d.stream));
    HIP_CHECK(hipMemcpyAsync(out, f.out, n * Wd * 4, hipMemcpyDeviceToHost, d.stream));
    HIP_CHECK(hipStreamSynchronize(d.stream));                  // blocking: the caller's plane is complete on return
    ms += query_ms(q);
    end_query(current);
    c.filter_ms = ms;
    q.out_W = W; q.out_H = H; q.out_mode = mode;                // (what sampleTexels / renderLightmap with RT_TEXELS_FROM_FILTER read where it lies)
    return (int)length;
}

double rtLastFilterMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastFilterMs before init");
    return g_ctx.filter_ms;
}

// Sampling texels (rt_api.h).  sampleTexels: chunk by chunk, the caller's hits go up, k_sample_texels looks the planes up over the first
// device's live slots, out and valid come down; the valid hits are counted in one device word, read back at the end.  renderLightmap: chunk by chunk over the
// pixels of the whole image, k_lightmap_rays fills the ray buffers, the closest-hit ray kernel (launch_rays) runs over them, k_lightmap_shade turns its planes
// into the frame's chunk, which comes down.  The planes go up once per call - or are read where the last bakeTexels / filterTexels left them.  Nothing of a
// frame's, a pass's or another query's state is read or written.
constexpr int kSampleFlags = RT_SAMPLE_BILINEAR | RT_TEXELS_FROM_BAKE | RT_TEXELS_FROM_FILTER;

// The checks the two calls share, under the function's name `fn`: `known` = the flag bits the call takes.
static void check_texel_source(const char* fn, int W, int H, int mode, const float* planes, int flags, int known) {
    const RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail(" before init", fn);
    if (c.is_spheres) rt_fail(": only a mesh scene has a UV atlas", fn);
    if (W < 1 || H < 1 || W > RT_TEXEL_MAX_SIZE || H > RT_TEXEL_MAX_SIZE) rt_fail(": W and H must be 1 .. RT_TEXEL_MAX_SIZE", fn);
    if (gather_width(mode) == 0) rt_fail(": unknown mode", fn);
    if ((flags & ~known) != 0) rt_fail(": unknown flag bits", fn);
    const bool bake = (flags & RT_TEXELS_FROM_BAKE) != 0, filter = (flags & RT_TEXELS_FROM_FILTER) != 0;
    if (planes && (bake || filter)) rt_fail(": RT_TEXELS_FROM_BAKE / RT_TEXELS_FROM_FILTER with planes given", fn);
    if (!planes && bake == filter) rt_fail(": planes is null and not exactly one of RT_TEXELS_FROM_BAKE / RT_TEXELS_FROM_FILTER is set", fn);
    if (!planes) {
        const TexelState& t = bake ? g_texels : g_filter;
        if (t.out_W < 1 || t.out_W != W || t.out_H != H || gather_width(t.out_mode) != gather_width(mode))
            rt_fail(bake ? ": the last bakeTexels left no out plane of this W, H and width" : ": the last filterTexels left no out plane of this W, H and width", fn);
    }
}

static char* lightmap_buffer(LightmapState& q, int k, size_t bytes) {
    return grown_buffer(q, k, std::max<size_t>(bytes, 4));
}

// The planes of a call on the query's device (begin_query has run): uploaded into the state's own buffer, or where the named call left them.
static RtTexelSource texel_source(LightmapState& q, int W, int H, int mode, const float* planes, int flags, hipStream_t stream) {
    RtTexelSource s = {};
    s.W = W; s.H = H; s.mode = mode;
    s.bilinear = (flags & RT_SAMPLE_BILINEAR) ? 1 : 0;
    if (planes) {
        const size_t bytes = (size_t)W * H * (size_t)gather_width(mode) * 4;
        float* d_planes = reinterpret_cast<float*>(lightmap_buffer(q, kLmPlanes, bytes));
        HIP_CHECK(hipMemcpyAsync(d_planes, planes, bytes, hipMemcpyHostToDevice, stream));
        s.planes = d_planes;
    } else {
        s.planes = reinterpret_cast<const float*>((flags & RT_TEXELS_FROM_BAKE) ? g_texels.d_buf[kTexOutPlane] : g_filter.d_buf[kFltOut]);
    }
    return s;
}

// The parameter block of chunk [first, first + m) of sampleTexels with its inputs uploaded.
static RtSampleParams sample_chunk(LightmapState& q, const RtTexelSource& src, size_t first, size_t m, const int32_t* prim, const float* uv,
                                   const float* normal, bool want_valid, hipStream_t stream) {
    const RenderContext& c = g_ctx;
    RtSampleParams p = {};
    p.slots = c.devs[0].d_tris; p.num_slots = (uint32_t)c.mesh.tris.size();
    p.src = src;
    int32_t* d_prim = reinterpret_cast<int32_t*>(lightmap_buffer(q, kLmPrim, m * 4));
    float* d_uv = reinterpret_cast<float*>(lightmap_buffer(q, kLmUv, m * 8));
    HIP_CHECK(hipMemcpyAsync(d_prim, prim + first, m * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_uv, uv + 2 * first, m * 8, hipMemcpyHostToDevice, stream));
    p.prim = d_prim; p.uv = d_uv;
    if (src.mode == RT_GATHER_SH9) {
        float* d_nrm = reinterpret_cast<float*>(lightmap_buffer(q, kLmNormal, m * 12));
        HIP_CHECK(hipMemcpyAsync(d_nrm, normal + 3 * first, m * 12, hipMemcpyHostToDevice, stream));
        p.normal = d_nrm;
    }
    p.out = reinterpret_cast<float*>(lightmap_buffer(q, kLmOut, m * 12));
    if (want_valid) p.valid = reinterpret_cast<uint8_t*>(lightmap_buffer(q, kLmValid, m));
    p.count = q.d_count;
    p.n = (int32_t)m;
    return p;
}

int sampleTexels(int n, const int32_t* prim, const float* uv, const float* normal, int W, int H, int mode, const float* planes, int flags, float* out,
                 uint8_t* valid) {
    RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("sampleTexels before init");
    if (c.is_spheres) rt_fail("sampleTexels: only a mesh scene has a UV atlas");
    if (n < 0) rt_fail("sampleTexels: n is negative");
    if (n == 0) return 0;
    if (!prim || !uv || !out) rt_fail("sampleTexels: prim, uv and out must not be null");
    if (flags & RT_LIGHTMAP_ALBEDO) rt_fail("sampleTexels: RT_LIGHTMAP_ALBEDO is renderLightmap's flag");
    check_texel_source("sampleTexels", W, H, mode, planes, flags, kSampleFlags);
    if (mode == RT_GATHER_SH9 && !normal) rt_fail("sampleTexels: normal is null (RT_GATHER_SH9 reads it)");
    LightmapState& q = g_sample;
    const DeviceState& d = c.devs[0];
    const int current = begin_query(q);
    if (!q.d_count) q.d_count = dev_alloc<uint32_t>(q.owned, 1);
    HIP_CHECK(hipMemsetAsync(q.d_count, 0, sizeof(uint32_t), d.stream));
    const RtTexelSource src = texel_source(q, W, H, mode, planes, flags, d.stream);
    double ms_sum = 0.0;
    for_chunks((size_t)n, kRayChunk, [&](size_t first, size_t m) {
        const RtSampleParams p = sample_chunk(q, src, first, m, prim, uv, normal, valid != nullptr, d.stream);
        HIP_CHECK(hipEventRecord(q.ev_start, d.stream));
        HIP_CHECK(rt_launch_sample_texels(p, d.stream));
        HIP_CHECK(hipEventRecord(q.ev_stop, d.stream));
        HIP_CHECK(hipMemcpyAsync(out + 3 * first, p.out, m * 12, hipMemcpyDeviceToHost, d.stream));
        if (valid) HIP_CHECK(hipMemcpyAsync(valid + first, p.valid, m, hipMemcpyDeviceToHost, d.stream));
        HIP_CHECK(hipStreamSynchronize(d.stream));              // (the events are read per chunk; blocking: the caller's arrays are complete on return)
        ms_sum += query_ms(q);
    });
    uint32_t count = 0;
    HIP_CHECK(hipMemcpy(&count, q.d_count, sizeof count, hipMemcpyDeviceToHost));
    end_query(current);
    c.sample_ms = ms_sum;
    return (int)count;
}

double rtLastSampleMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastSampleMs before init");
    return g_ctx.sample_ms;
}

// The parameter block of chunk [first, first + m) of renderLightmap, its buffers grown to the chunk.
static RtLightmapParams lightmap_chunk(LightmapState& q, const RtTexelSource& src, size_t first, size_t m, int flags, const float floor_value[3]) {
    RtLightmapParams l = {};
    l.org = reinterpret_cast<float*>(lightmap_buffer(q, kLmOrg, m * 12));
    l.dir = reinterpret_cast<float*>(lightmap_buffer(q, kLmDir, m * 12));
    l.t = reinterpret_cast<float*>(lightmap_buffer(q, kLmT, m * 4));
    l.prim = reinterpret_cast<int32_t*>(lightmap_buffer(q, kLmPrim, m * 4));
    l.normal = reinterpret_cast<float*>(lightmap_buffer(q, kLmNormal, m * 12));
    l.uv = reinterpret_cast<float*>(lightmap_buffer(q, kLmUv, m * 8));
    l.num_slots = (uint32_t)g_ctx.mesh.tris.size();
    l.src = src;
    l.albedo = (flags & RT_LIGHTMAP_ALBEDO) ? 1 : 0;
    for (int a = 0; a < 3; a++) l.floor_value[a] = floor_value ? floor_value[a] : 1.0f;
    l.out = reinterpret_cast<rt_vec3*>(lightmap_buffer(q, kLmOut, m * 12));
    l.first = (uint32_t)first;
    l.n = (int32_t)m;
    return l;
}

void renderLightmap(int W, int H, int mode, const float* planes, int flags, const float floor_value[3], rt_vec3* out) {
    RenderContext& c = g_ctx;
    check_texel_source("renderLightmap", W, H, mode, planes, flags, kSampleFlags | RT_LIGHTMAP_ALBEDO);
    if (!out) rt_fail("renderLightmap: out is null");
    LightmapState& q = g_lightmap;
    const DeviceState& d = c.devs[0];
    const int current = begin_query(q);
    const RtTexelSource src = texel_source(q, W, H, mode, planes, flags, d.stream);
    const RtMeshParams scene = mesh_params(d, whole_image_partition());
    double ms_sum = 0.0;
    for_chunks((size_t)c.nx * c.ny, kRayChunk, [&](size_t first, size_t m) {
        const RtLightmapParams l = lightmap_chunk(q, src, first, m, flags, floor_value);
        RtRayBatch b = {};
        b.org = l.org; b.dir = l.dir;
        b.t = const_cast<float*>(l.t); b.prim = const_cast<int32_t*>(l.prim); b.normal = const_cast<float*>(l.normal); b.uv = const_cast<float*>(l.uv);
        b.n = l.n;
        b.t_min_default = c.opt.t_min;
        HIP_CHECK(hipEventRecord(q.ev_start, d.stream));
        HIP_CHECK(rt_launch_lightmap_rays(scene, l, d.stream));
        launch_rays(d, b, false);
        HIP_CHECK(rt_launch_lightmap_shade(scene, l, d.stream));
        HIP_CHECK(hipEventRecord(q.ev_stop, d.stream));
        HIP_CHECK(hipMemcpyAsync(out + first, l.out, m * 12, hipMemcpyDeviceToHost, d.stream));
        HIP_CHECK(hipStreamSynchronize(d.stream));              // (the events are read per chunk; blocking: the caller's frame is complete on return)
        ms_sum += query_ms(q);
    });
    end_query(current);
    c.lightmap_ms = ms_sum;
}

double rtLastLightmapMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastLightmapMs before init");
    return g_ctx.lightmap_ms;
}

// Adaptive sampling on the device (rt_api.h).  One call is one pass over the whole image on the first in-process device: select (rt_refine.h)
// builds the list, the pixel kernels of renderPixels trace `batch` more samples of its entries over device-resident batch arrays, chunk by chunk, update
// scatters the states back.  Of the pass only one word crosses the bus, and only downwards: the length of the list, which the launch of the pixel kernel
// needs on the host.  The launch is renderPixels' (launch_pixels); nothing of a frame's, a pass's or renderPixels' own state is read or written.
static void check_refine(const char* fn) {
    if (!g_ctx.initialised) rt_fail(" before init", fn);
}

int refineFrame(rt_vec3* out, int32_t* samples, float* error, int batch, int min_batches, int max_samples, float threshold, int flags) {
    RenderContext& c = g_ctx;
    RefineState& q = g_refine;
    check_refine("refineFrame");
    if (batch < 1) rt_fail("refineFrame: batch must be at least 1");
    if (min_batches < 2) rt_fail("refineFrame: min_batches must be at least 2 (the error needs two batch means)");
    if (max_samples < batch || max_samples > RT_PROGRESSIVE_MAX_SAMPLES) rt_fail("refineFrame: max_samples must be batch .. RT_PROGRESSIVE_MAX_SAMPLES");
    if (!std::isfinite(threshold) || threshold < 0.0f) rt_fail("refineFrame: threshold must be finite and not negative");
    if ((flags & ~RT_REFINE_DILATE) != 0) rt_fail("refineFrame: unknown flag bits");
    if (q.passes > 0 && batch != q.batch) rt_fail("refineFrame: batch differs from the frame's (it is fixed by the first call after a reset)");
    check_per_pixel("refineFrame");
    const DeviceState& d = c.devs[0];
    const size_t npix = (size_t)c.nx * c.ny, chunk = std::min(npix, kPixelChunk);
    const int current = begin_query(q);
    RtRefineParams& r = q.planes;
    if (!r.state) {
        r.state = dev_alloc<uint4>(q.owned, npix);
        r.n = dev_alloc<int32_t>(q.owned, npix);
        r.mom = dev_alloc<float2>(q.owned, npix);
        r.rays = dev_alloc<uint32_t>(q.owned, npix);
        r.lum = dev_alloc<float>(q.owned, npix);
        r.flag = dev_alloc<uint8_t>(q.owned, npix);
        r.cls = dev_alloc<uint8_t>(q.owned, npix);
        r.list = dev_alloc<uint32_t>(q.owned, npix);
        r.words = dev_alloc<uint32_t>(q.owned, kRefineWords);
        r.b_ij = dev_alloc<int32_t>(q.owned, 2 * chunk);
        r.b_first = dev_alloc<int32_t>(q.owned, chunk);
        r.b_state = dev_alloc<uint32_t>(q.owned, 4 * chunk);
        r.b_rays = dev_alloc<uint32_t>(q.owned, chunk);
        q.chunk_cap = chunk;
        q.d_queue = dev_alloc<uint32_t>(q.owned, 1);
    }
    if (out && !r.out) r.out = dev_alloc<rt_vec3>(q.owned, npix);
    if (error && !r.err) r.err = dev_alloc<float>(q.owned, npix);
    if (q.passes == 0) {                                    // a new frame: no samples, no statistics (a pixel with n = 0 starts from its seed, not from `state`)
        HIP_CHECK(hipMemsetAsync(r.n, 0, npix * sizeof(int32_t), d.stream));
        HIP_CHECK(hipMemsetAsync(r.mom, 0, npix * sizeof(float2), d.stream));
        HIP_CHECK(hipMemsetAsync(r.rays, 0, npix * sizeof(uint32_t), d.stream));
        HIP_CHECK(hipMemsetAsync(r.lum, 0, npix * sizeof(float), d.stream));
        q.batch = batch;
        q.samples = 0;
    }
    RtRefineParams p = r;
    p.out = out ? r.out : nullptr; p.err = error ? r.err : nullptr;
    p.nx = c.nx; p.ny = c.ny;
    p.batch = batch; p.min_batches = min_batches; p.max_samples = max_samples; p.flags = flags; p.threshold = threshold;
    const RtSwitches sw = rt_read_switches();
    p.cost_order = sw.refine_order ? 1 : 0;
    uint32_t total = 0;
    HIP_CHECK(hipEventRecord(q.ev_start, d.stream));
    HIP_CHECK(hipMemsetAsync(r.words, 0, kRefineWords * sizeof(uint32_t), d.stream));
    HIP_CHECK(rt_launch_refine_select(p, d.stream));
    HIP_CHECK(hipMemcpyAsync(&total, r.words + kRefineTotal, sizeof total, hipMemcpyDeviceToHost, d.stream));
    HIP_CHECK(hipStreamSynchronize(d.stream));              // the one readback of a pass: RtPixelBatch::n and the grid of the pixel kernel come from it
    if ((size_t)total > npix) rt_fail("refineFrame: the list is longer than the image");
    for_chunks(total, q.chunk_cap, [&](size_t first, size_t m) {
        p.chunk_first = (uint32_t)first;
        p.chunk_n = (uint32_t)m;
        HIP_CHECK(rt_launch_refine_gather(p, d.stream));
        HIP_CHECK(hipMemsetAsync(q.d_queue, 0, sizeof(uint32_t), d.stream));
        RtPixelBatch b;
        b.ij = p.b_ij; b.ns = nullptr; b.first = p.b_first; b.state = p.b_state; b.out = nullptr; b.rays = p.b_rays;
        b.queue = q.d_queue; b.n = (int32_t)m; b.ns_all = batch;
        launch_pixels(d, b, sw.pixels_waves);
        HIP_CHECK(rt_launch_refine_update(p, d.stream));
    });
    HIP_CHECK(hipEventRecord(q.ev_stop, d.stream));
    if (p.out || p.err) HIP_CHECK(rt_launch_refine_deliver(p, d.stream));
    if (out) HIP_CHECK(hipMemcpyAsync(out, p.out, npix * sizeof(rt_vec3), hipMemcpyDeviceToHost, d.stream));
    if (samples) HIP_CHECK(hipMemcpyAsync(samples, r.n, npix * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
    if (error) HIP_CHECK(hipMemcpyAsync(error, p.err, npix * sizeof(float), hipMemcpyDeviceToHost, d.stream));
    HIP_CHECK(hipStreamSynchronize(d.stream));              // blocking: the caller's planes are complete on return
    q.ms = query_ms(q);
    end_query(current);
    q.last_len = total;
    if (total > 0) {
        q.passes = std::min(q.passes, INT_MAX - 1) + 1;
        q.samples += (long long)total * batch;
    }
    return (int)total;
}

void rtResetRefine(void) {
    check_refine("rtResetRefine");
    reset_refine();
}

long long rtRefineSamples(void) {
    check_refine("rtRefineSamples");
    return g_refine.samples;
}

int rtRefineLastList(int32_t* ij, int cap) {
    check_refine("rtRefineLastList");
    const RefineState& q = g_refine;
    const size_t n = std::min((size_t)std::max(cap, 0), (size_t)q.last_len);
    if (ij && n > 0) {
        std::vector<uint32_t> ids(n);
        const int current = begin_query(q);
        HIP_CHECK(hipMemcpy(ids.data(), q.planes.list, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        end_query(current);
        for (size_t k = 0; k < n; k++) {
            ij[2 * k] = (int32_t)(ids[k] % (uint32_t)g_ctx.nx);
            ij[2 * k + 1] = (int32_t)(ids[k] / (uint32_t)g_ctx.nx);
        }
    }
    return (int)q.last_len;
}

double rtLastRefineMs(void) {
    check_refine("rtLastRefineMs");
    return g_refine.ms;
}

// Guide-driven preview denoiser (rt_api.h).  The filter needs neighbours across stripe boundaries, so it works on the whole image on the first
// in-process device (every device holds the whole scene, setup_devices) with buffers, guide planes and events of its own: like renderGuides it reads and
// writes nothing of a frame's state.
int rtDefaultDenoiseFlags(void) {
    if (!g_ctx.initialised) rt_fail("rtDefaultDenoiseFlags before init");
    return g_ctx.is_spheres ? (RT_DENOISE_DEMODULATE | RT_DENOISE_SAME_PRIM) : RT_DENOISE_DEMODULATE;     // one id = one object / one id = one triangle
}

void denoiseFrame(const rt_vec3* in, rt_vec3* out, int iterations, int flags, int normal_squarings, float sigma_z, float sigma_c) {
    check_pass_args("denoiseFrame", kCheckInit | kCheckOut, out, flags, sigma_z);
    if (iterations < 1 || iterations > RT_DENOISE_MAX_ITERATIONS) rt_fail("denoiseFrame: iterations must be 1 .. RT_DENOISE_MAX_ITERATIONS");
    if (normal_squarings < 0 || normal_squarings > RT_DENOISE_MAX_SQUARINGS) rt_fail("denoiseFrame: normal_squarings must be 0 .. RT_DENOISE_MAX_SQUARINGS");
    check_pass_args("denoiseFrame", kCheckFlags | kCheckSigmaZ, out, flags, sigma_z);
    if (!std::isfinite(sigma_c)) rt_fail("denoiseFrame: sigma_c must be finite (<= 0 switches the colour weight off)");
    check_pass_args("denoiseFrame", kCheckFloor, out, flags, sigma_z);
    DenoiseState& n = g_denoise;
    const int current = begin_pass(n, in, [&n] {
        n.d_rec = dev_alloc<float4>(n.owned, 2 * n.npix);
        n.d_col[0] = dev_alloc<float4>(n.owned, n.npix);
        n.d_col[1] = dev_alloc<float4>(n.owned, n.npix);
    });
    RtDenoiseParams q = pass_params<RtDenoiseParams>(n);
    q.rec = n.d_rec; q.col[0] = n.d_col[0]; q.col[1] = n.d_col[1];
    q.flags = flags; q.normal_squarings = normal_squarings; q.sigma_z = sigma_z; q.sigma_c = sigma_c;
    const hipStream_t stream = g_ctx.devs[0].stream;
    HIP_CHECK(hipEventRecord(n.ev_start, stream));
    HIP_CHECK(rt_launch_denoise_prologue(q, stream));
    for (int it = 0; it < iterations; it++) HIP_CHECK(rt_launch_denoise_iteration(q, it, it == iterations - 1, stream));
    g_ctx.denoise_ms = end_pass(n, current, out);
}

double rtLastDenoiseMs(void) { return g_ctx.denoise_ms; }

// Temporal accumulation (rt_api.h).  Like the denoiser: the whole image on the first in-process device, guide planes of its own for the
// camera and options in force, buffers and events of its own.  The history - the last call's camera and the newest record set - stays on the device.
void accumulateFrame(const rt_vec3* in, rt_vec3* out, float* history, int flags, int max_history, float sigma_z, float normal_min) {
    check_pass_args("accumulateFrame", kCheckInit | kCheckOut | kCheckFlags, out, flags, sigma_z);
    if (max_history < 1 || max_history > RT_ACCUM_MAX_HISTORY) rt_fail("accumulateFrame: max_history must be 1 .. RT_ACCUM_MAX_HISTORY");
    check_pass_args("accumulateFrame", kCheckSigmaZ, out, flags, sigma_z);
    if (!std::isfinite(normal_min) || normal_min < -1.0f || normal_min > 1.0f) rt_fail("accumulateFrame: normal_min must be finite and in [-1, 1]");
    check_pass_args("accumulateFrame", kCheckFloor, out, flags, sigma_z);
    AccumulateState& n = g_accumulate;
    const int current = begin_pass(n, in, [&n] {
        n.d_history = dev_alloc<float>(n.owned, n.npix);
        n.d_rec[0] = dev_alloc<float4>(n.owned, 3 * n.npix);
        n.d_rec[1] = dev_alloc<float4>(n.owned, 3 * n.npix);
    }, 0, n.frames > 0);
    RtAccumulateParams q = pass_params<RtAccumulateParams>(n);
    q.history = history ? n.d_history : nullptr;
    q.prev = n.d_rec[n.newest]; q.next = n.d_rec[n.newest ^ 1];
    q.flags = flags; q.has_history = n.frames > 0 ? 1 : 0;
    q.max_history = (float)max_history; q.sigma_z = sigma_z; q.normal_min = normal_min;
    q.motion = n.frames > 0 && g_pose.marked ? g_pose.d_planes : nullptr;
    const hipStream_t stream = g_ctx.devs[0].stream;
    HIP_CHECK(hipEventRecord(n.ev_start, stream));
    HIP_CHECK(rt_launch_accumulate(q, n.prev_cam, stream));
    g_ctx.accumulate_ms = end_pass(n, current, out, history, n.d_history);
    n.newest ^= 1;
    n.prev_cam = g_ctx.cam;
    if (n.frames < INT_MAX) n.frames++;
}

void rtResetHistory(void) {
    if (!g_ctx.initialised) rt_fail("rtResetHistory before init");
    g_accumulate.frames = 0;
}

int rtHistoryFrames(void) {
    if (!g_ctx.initialised) rt_fail("rtHistoryFrames before init");
    return g_accumulate.frames;
}

double rtLastAccumulateMs(void) { return g_ctx.accumulate_ms; }

// Variance-guided accumulate + filter in one device pass (rt_api.h).  Like the two passes it fuses: the whole image on the first in-process
// device, guide planes of its own (one guide pass, not two), buffers and events of its own, a history of its own.  The accumulated frame never leaves the device.
void previewFrame(const rt_vec3* in, rt_vec3* out, float* history, float* variance, int flags, int max_history, int iterations, int normal_squarings,
                  float sigma_z, float normal_min, float sigma_l) {
    check_pass_args("previewFrame", kCheckInit | kCheckOut | kCheckFlags, out, flags, sigma_z);
    if (max_history < 1 || max_history > RT_ACCUM_MAX_HISTORY) rt_fail("previewFrame: max_history must be 1 .. RT_ACCUM_MAX_HISTORY");
    if (iterations < 1 || iterations > RT_DENOISE_MAX_ITERATIONS) rt_fail("previewFrame: iterations must be 1 .. RT_DENOISE_MAX_ITERATIONS");
    if (normal_squarings < 0 || normal_squarings > RT_DENOISE_MAX_SQUARINGS) rt_fail("previewFrame: normal_squarings must be 0 .. RT_DENOISE_MAX_SQUARINGS");
    check_pass_args("previewFrame", kCheckSigmaZ, out, flags, sigma_z);
    if (!std::isfinite(normal_min) || normal_min < -1.0f || normal_min > 1.0f) rt_fail("previewFrame: normal_min must be finite and in [-1, 1]");
    if (!std::isfinite(sigma_l) || !(sigma_l > 0.0f)) rt_fail("previewFrame: sigma_l must be finite and positive");
    check_pass_args("previewFrame", kCheckFloor, out, flags, sigma_z);
    PreviewState& n = g_preview;
    const int current = begin_pass(n, in, [&n] {
        n.d_history = dev_alloc<float>(n.owned, n.npix);
        n.d_variance = dev_alloc<float>(n.owned, n.npix);
        for (int k = 0; k < 2; k++) {
            n.d_rec[k] = dev_alloc<float4>(n.owned, 3 * n.npix);
            n.d_mom[k] = dev_alloc<float2>(n.owned, n.npix);
            n.d_col[k] = dev_alloc<float4>(n.owned, n.npix);
        }
    }, 0, n.frames > 0);
    RtPreviewParams q = pass_params<RtPreviewParams>(n);
    q.history = history ? n.d_history : nullptr;
    q.variance = variance ? n.d_variance : nullptr;
    q.prev = n.d_rec[n.newest]; q.next = n.d_rec[n.newest ^ 1];
    q.prev_mom = n.d_mom[n.newest]; q.next_mom = n.d_mom[n.newest ^ 1];
    q.col[0] = n.d_col[0]; q.col[1] = n.d_col[1];
    q.flags = flags; q.has_history = n.frames > 0 ? 1 : 0; q.normal_squarings = normal_squarings;
    q.max_history = (float)max_history; q.sigma_z = sigma_z; q.normal_min = normal_min; q.sigma_l = sigma_l;
    q.motion = n.frames > 0 && g_pose.marked ? g_pose.d_planes : nullptr;
    const hipStream_t stream = g_ctx.devs[0].stream;
    HIP_CHECK(hipEventRecord(n.ev_start, stream));
    HIP_CHECK(rt_launch_preview_temporal(q, n.prev_cam, stream));
    HIP_CHECK(rt_launch_preview_variance(q, stream));
    for (int it = 0; it < iterations; it++) HIP_CHECK(rt_launch_preview_iteration(q, it, it == iterations - 1, stream));
    g_ctx.preview_ms = end_pass(n, current, out, history, n.d_history, variance, n.d_variance);
    n.newest ^= 1;
    n.prev_cam = g_ctx.cam;
    if (n.frames < INT_MAX) n.frames++;
}

void rtResetPreview(void) {
    if (!g_ctx.initialised) rt_fail("rtResetPreview before init");
    g_preview.frames = 0;
}

int rtPreviewFrames(void) {
    if (!g_ctx.initialised) rt_fail("rtPreviewFrames before init");
    return g_preview.frames;
}

double rtLastPreviewMs(void) { return g_ctx.preview_ms; }

// The marked pose and the motion planes (rt_api.h).  The mark is a copy of the scene's geometry on the first in-process device, where the
// passes run: the triangle slots device to device, the spheres from the host's layout.  A second rtMarkPose overwrites it.
void rtMarkPose(void) {
    RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("rtMarkPose before init");
    const DeviceState& d = c.devs[0];
    PoseState& m = g_pose;
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    HIP_CHECK(hipSetDevice(d.device));
    m.device = d.device;
    if (c.is_spheres) {
        m.h_mark = caller_spheres();
        m.count = m.h_mark.size();
        if (!m.d_mark_sph) m.d_mark_sph = dev_alloc<float4>(m.owned, m.count);
        HIP_CHECK(hipMemcpyAsync(m.d_mark_sph, m.h_mark.data(), m.count * sizeof(float4), hipMemcpyHostToDevice, d.stream));
    } else {
        m.count = c.mesh.tris.size();
        if (!m.d_mark) m.d_mark = dev_alloc<rt_triangle>(m.owned, m.count);
        HIP_CHECK(hipMemcpyAsync(m.d_mark, d.d_tris, m.count * sizeof(rt_triangle), hipMemcpyDeviceToDevice, d.stream));
    }
    HIP_CHECK(hipStreamSynchronize(d.stream));
    HIP_CHECK(hipSetDevice(current));
    m.marked = true;
}

void rtClearPose(void) {
    if (!g_ctx.initialised) rt_fail("rtClearPose before init");
    g_pose.marked = false;                                  // (the buffers stay for the next mark)
}

int rtPoseMarked(void) {
    if (!g_ctx.initialised) rt_fail("rtPoseMarked before init");
    return g_pose.marked ? 1 : 0;
}

void renderMotion(int mask, const rt_camera* prev_cam, float* prev_pos, float* prev_normal, float* screen) {
    RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("renderMotion before init");
    constexpr int kAll = RT_MOTION_POS | RT_MOTION_NORMAL | RT_MOTION_SCREEN;
    if (mask == 0 || (mask & ~kAll) != 0) rt_fail("renderMotion: mask must name at least one RT_MOTION_* plane and no unknown bit");
    float* const host[3] = { prev_pos, prev_normal, screen };
    for (int k = 0; k < 3; k++)
        if ((mask >> k & 1) && !host[k]) rt_fail("renderMotion: a requested plane has a null pointer");
    if (c.is_spheres && c.opt.floor) rt_fail("renderMotion: the floor plane is only defined for mesh scenes (kernel_scene.floor)");
    MotionState& n = g_motion;
    const int current = begin_pass(n, nullptr, [] {}, kPassOwnOutput | kPassNoInput);
    const bool with_screen = (mask & RT_MOTION_SCREEN) != 0;
    refresh_live_spheres();                                 // (in front of the start event: the time is the kernel's alone)
    HIP_CHECK(hipEventRecord(n.ev_start, c.devs[0].stream));
    launch_motion(n, with_screen, prev_cam ? *prev_cam : c.cam);
    n.h_planes.resize(2 * n.npix);
    PassCopy own[2] = { { n.h_planes.data(), g_pose.d_planes, 2 * n.npix * sizeof(float4) }, { screen, g_pose.d_screen, n.npix * sizeof(float2) } };
    c.motion_ms = end_pass(n, current, nullptr, nullptr, nullptr, nullptr, nullptr, own, with_screen ? 2 : 1);
    for (int k = 0; k < 2; k++) {
        if (!(mask >> k & 1)) continue;
        const float4* src = n.h_planes.data() + (size_t)k * n.npix;
        for (size_t p = 0; p < n.npix; p++) { host[k][3 * p] = src[p].x; host[k][3 * p + 1] = src[p].y; host[k][3 * p + 2] = src[p].z; }
    }
}

double rtLastMotionMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastMotionMs before init");
    return g_ctx.motion_ms;
}

// The display transform (rt_api.h).  Through the passes' shared path, without guide planes: the whole image on the first in-process device, the
// RGBA words and the histogram its own buffers.  With RT_DISPLAY_FROM_PREVIEW the input is previewFrame's output buffer where that call left it.
void displayFrame(const rt_vec3* in, uint8_t* out_rgba, int flags, int tonemap, float exposure, float adapt) {
    RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("displayFrame before init");
    if (!out_rgba) rt_fail("displayFrame: out_rgba is null");
    constexpr int kAll = RT_DISPLAY_TOP_DOWN | RT_DISPLAY_DITHER | RT_DISPLAY_AUTO_EXPOSURE | RT_DISPLAY_FROM_PREVIEW;
    if ((flags & ~kAll) != 0) rt_fail("displayFrame: unknown flag bits");
    if (tonemap != RT_TONEMAP_NONE && tonemap != RT_TONEMAP_REINHARD && tonemap != RT_TONEMAP_ACES) rt_fail("displayFrame: unknown tonemap");
    if (!std::isfinite(exposure) || !(exposure > 0.0f)) rt_fail("displayFrame: exposure must be finite and positive");
    if (!std::isfinite(adapt) || !(adapt > 0.0f) || adapt > 1.0f) rt_fail("displayFrame: adapt must be finite and in (0, 1]");
    const bool from_preview = (flags & RT_DISPLAY_FROM_PREVIEW) != 0, auto_exposure = (flags & RT_DISPLAY_AUTO_EXPOSURE) != 0;
    if (from_preview && in) rt_fail("displayFrame: RT_DISPLAY_FROM_PREVIEW takes in = NULL");
    if (from_preview && g_preview.frames == 0) rt_fail("displayFrame: RT_DISPLAY_FROM_PREVIEW without a previewFrame since init or the last reset of its history");
    DisplayState& n = g_display;
    const int current = begin_pass(n, in, [&n] {
        n.d_rgba = dev_alloc<uint32_t>(n.owned, n.npix);
        n.d_words = dev_alloc<uint32_t>(n.owned, RT_DISPLAY_BINS + 2);
    }, kPassNoGuides | kPassOwnOutput | (from_preview ? kPassNoUpload : 0));
    RtDisplayParams q;
    memset(&q, 0, sizeof q);
    q.in = from_preview ? g_preview.d_out : n.d_in;
    q.out = n.d_rgba; q.hist = n.d_words;
    q.state = auto_exposure ? reinterpret_cast<float*>(n.d_words + RT_DISPLAY_BINS) : nullptr;
    q.nx = c.nx; q.ny = c.ny; q.flags = flags; q.tonemap = tonemap; q.adapted = n.adapted ? 1 : 0;
    q.exposure = exposure; q.adapt = adapt;
    const hipStream_t stream = c.devs[0].stream;
    HIP_CHECK(hipEventRecord(n.ev_start, stream));
    if (auto_exposure) {
        HIP_CHECK(hipMemsetAsync(n.d_words, 0, RT_DISPLAY_BINS * sizeof(uint32_t), stream));
        HIP_CHECK(rt_launch_display_histogram(q, stream));
        HIP_CHECK(rt_launch_display_resolve(q, stream));
    }
    HIP_CHECK(rt_launch_display_transform(q, stream));
    const PassCopy own[2] = { { out_rgba, n.d_rgba, n.npix * sizeof(uint32_t) }, { n.h_words, n.d_words, sizeof n.h_words } };
    c.display_ms = end_pass(n, current, nullptr, nullptr, nullptr, nullptr, nullptr, own, auto_exposure ? 2 : 1);
    if (auto_exposure) {
        n.adapted = true;
        memcpy(&n.last_exposure, &n.h_words[RT_DISPLAY_BINS + 1], sizeof(float));
    } else {
        n.last_exposure = exposure;
    }
}

float rtLastExposure(void) {
    if (!g_ctx.initialised) rt_fail("rtLastExposure before init");
    return g_display.last_exposure;
}

int rtDisplayHistogram(uint32_t* out, int cap) {
    if (!g_ctx.initialised) rt_fail("rtDisplayHistogram before init");
    const int n = std::min(std::max(cap, 0), RT_DISPLAY_BINS);
    if (out && n > 0) memcpy(out, g_display.h_words, (size_t)n * sizeof(uint32_t));
    return RT_DISPLAY_BINS;
}

void rtResetDisplay(void) {
    if (!g_ctx.initialised) rt_fail("rtResetDisplay before init");
    reset_display();
}

double rtLastDisplayMs(void) {
    if (!g_ctx.initialised) rt_fail("rtLastDisplayMs before init");
    return g_ctx.display_ms;
}

void setExternalFramebuffer(rt_vec3* fb) {
    RenderContext& c = g_ctx;
    if (!c.initialised) rt_fail("setExternalFramebuffer before init");
    if (c.h_ext) { if (c.ext_registered) HIP_CHECK(hipHostUnregister(c.h_ext)); c.h_ext = nullptr; c.ext_registered = false; }
    if (fb) {
        // Page-locking the caller's memory (a /dev/shm mapping shared by the ranks of a node, bench.py) lets the kernels deliver finished pixels
        // straight into it.  If the runtime refuses (locked-memory limit of the account, a mapping it cannot pin) the job must not die on its first
        // multi-GPU node: the renderer falls back to its compact device buffer and plain device-to-host copies of this member's stripes into the
        // (pageable) memory - slower by the copy, same image.  RT_EXT_FB_NO_REGISTER=1 forces that path (tests).
        hipError_t e = rt_read_switches().ext_fb_no_register ? hipErrorNotSupported
                                                             : hipHostRegister(fb, (size_t)c.nx * c.ny * sizeof(rt_vec3), hipHostRegisterDefault);
        if (e != hipSuccess) {
            (void)hipGetLastError();                                 // (clear the sticky error: it has been handled)
            fprintf(stderr, "rt warning: setExternalFramebuffer could not page-lock the caller's framebuffer (%s): stripes are copied into it "
                            "from the device buffer instead of being stored by the kernel\n", hipGetErrorString(e));
        }
        c.ext_registered = e == hipSuccess;
        c.h_ext = fb;
    }
}

void getRenderStats(rt_render_stats* out) {
    if (out) *out = g_ctx.stats;
}

void cleanupRenderer(void) {
    if (!g_ctx.initialised) return;
    cleanup_impl();
    // kernels.cu:679 ends with cudaDeviceReset().  A reset destroys EVERY context of the process on that device - also the one of a
    // host that shares the process (PyTorch in bench.py, a viewer) - so it is opt-in here: RT_CLEANUP_DEVICE_RESET=1 mirrors the reference.
    if (rt_read_switches().cleanup_device_reset) (void)hipDeviceReset();
}

}  // extern "C"
