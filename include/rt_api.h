/*
 * rt_api.h — C-ABI of librt_mi355x.so, the MI355X-native replacement for the host API of the
 * reference renderer (/root/reference/kernels.h:6-8, defined in kernels.cu:571-680).
 *
 * The first three entry points are the reference's own symbols, with byte-identical signatures
 * (struct layouts in rt_types.h); the rest are additive.  No torch types, no C++ types.
 *
 * Error convention (kernels.cu:27-38): every function returns void; any HIP runtime failure
 * prints "HIP error = <string> at <file>:<line> '<expr>'" on stderr and calls exit(99).
 * Misuse (run before init, bad sizes) prints "rt error: ..." and exit(99) as well.
 *
 * State (kernels.cu:145): one global render context per process; not re-entrant; the caller is
 * single-threaded.  runRenderer is synchronous; on return *fb is host-readable.
 */
#ifndef RT_API_H
#define RT_API_H

#include "rt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- reference symbols ------------------------------------------------------------------- */

/* replaces kernels.cu:571-650.  Deep-copies sc.m->tris, sc.m->bvh, sc.materials and
 * sc.textures[i].data to the device (borrowed only for the duration of the call), allocates the
 * framebuffer (nx*ny vec3, linear RGB, row 0 = bottom row) and returns it through *fb.  The
 * framebuffer is host memory owned by the renderer, valid until cleanupRenderer. */
void initRenderer(const rt_kernel_scene sc, const rt_camera cam, rt_vec3** fb, int nx, int ny, int maxDepth);

/* replaces kernels.cu:652-664.  Renders ns samples per pixel into the framebuffer; blocking.
 * tx,ty are the reference's CUDA block shape (main.cpp:69-70); accepted and ignored — the
 * wave64 tile shape is fixed by the kernel. May be called repeatedly: same image every time.
 * Leaves the progressive frame (runRendererProgressive) as it was. */
void runRenderer(int ns, int tx, int ty);

/* replaces kernels.cu:666-680.  Frees everything, the framebuffer included. */
void cleanupRenderer(void);

/* --- additive symbols -------------------------------------------------------------------- */

/* Sphere scenes (the README-era benchmark; kernel_scene has no sphere array,
 * helper_structs.h:217-228).  materials[k] belongs to spheres[k].  Defaults for this path:
 * gradient sky, NEE off, RR off, t_min 0.001. */
void initRendererSpheres(const rt_sphere* spheres, const rt_material* materials, int n,
                         const rt_camera cam, rt_vec3** fb, int nx, int ny, int maxDepth);

/* Fills *opt with the defaults of the mesh path (is_sphere_scene = 0: kernels.cu:13-24,93-94)
 * or of the sphere path (is_sphere_scene = 1). */
void getDefaultRenderOptions(rt_render_options* opt, int is_sphere_scene);

/* Takes effect for the following runRenderer calls.  Call after init*. */
void setRenderOptions(const rt_render_options* opt);

/* Makes the following runRenderer calls deliver into caller-owned host memory (nx*ny vec3) instead of the
 * library's own framebuffer: the buffer is page-locked with hipHostRegister and becomes the target of the
 * device-to-host stripe copies.  Used for the multi-process host gather: every rank passes the same shared
 * mapping and writes only the stripes it owns.  NULL switches back.  The caller keeps ownership.
 * If the runtime cannot page-lock the memory, a warning is printed and the stripes are copied into it as pageable
 * memory (same image, no direct delivery by the kernel): never a reason to exit. */
void setExternalFramebuffer(rt_vec3* fb);

/* Timing / counters of the last runRenderer. */
void getRenderStats(rt_render_stats* out);

/* Number of HIP devices visible to the process (0 if none). Never exits. */
int rtDeviceCount(void);

/* Library/ABI version: major*1000 + minor.  Bumped whenever rt_render_options or rt_render_stats (or any other struct of rt_types.h)
 * changes size or layout; a binding refuses a library whose version differs from the RT_API_VERSION it was written against. */
#define RT_API_VERSION 1002
int rtApiVersion(void);

/* sizeof of every struct that crosses this boundary, as the LIBRARY was compiled: out[RT_SIZEOF_*], at most n entries written; returns
 * RT_SIZEOF_COUNT.  getDefaultRenderOptions / getRenderStats write sizeof(struct) bytes through the caller's pointer, so a binding checks
 * these against its own mirror before the first such call (the Python mirror does so in load_renderer(): a mismatch is an ImportError). */
enum { RT_SIZEOF_RENDER_OPTIONS = 0, RT_SIZEOF_RENDER_STATS, RT_SIZEOF_CAMERA, RT_SIZEOF_SPHERE, RT_SIZEOF_MATERIAL, RT_SIZEOF_TRIANGLE,
       RT_SIZEOF_BVH_NODE, RT_SIZEOF_MESH, RT_SIZEOF_KERNEL_SCENE, RT_SIZEOF_STEXTURE, RT_SIZEOF_PLANE, RT_SIZEOF_BBOX, RT_SIZEOF_VEC3,
       RT_SIZEOF_COUNT };
int rtStructSizes(int32_t* out, int n);

/* Launch report of the last runRenderer: one record of RT_LAUNCH_WORDS int32 per render-kernel launch, in launch order, over all
 * in-process devices.  The helper kernels of a frame (cost ordering, centre-ray classification, framebuffer poison, chunk sums) are not
 * listed.  Writes min(cap, count) records to out (out may be NULL when cap is 0) and returns count.  Host-side bookkeeping only.
 * Each record names the template instantiation that was LAUNCHED:
 *   [RT_LAUNCH_FAMILY]  RT_KERNEL_SPHERE_QUEUE  k_render_spheres_queue<PHASE, CLS, CHUNKED, DBG, SCENE, LEAN>
 *                       RT_KERNEL_SPHERE_TILES  k_render_spheres_tiles<LEGACY>          (LEGACY in the CLS word, the rest 0)
 *                       RT_KERNEL_MESH_QUEUE    k_render_mesh_queue<TRAV, DBG, STATS, LEAN, PHASE>
 *                                               (TRAV in the CLS word: 1 = classic while-while; DBG | STATS << 1 in the DBG word; LEAN 0 / 1)
 *                       RT_KERNEL_MESH_TILES    k_render_mesh<VARIANT>                  (VARIANT in the CLS word, the rest 0)
 *   [RT_LAUNCH_PHASE] .. [RT_LAUNCH_LEAN]  the template arguments above (bools as 0 / 1)
 *   [RT_LAUNCH_THREADS] threads per workgroup   [RT_LAUNCH_BLOCKS] workgroups launched
 *   [RT_LAUNCH_DEVICE]  HIP device ordinal      [RT_LAUNCH_FP]     rt_render_options.fp of the frame (RT_FP_PARITY / RT_FP_FAST) */
/* --- progressive rendering ------------------------------------------------------------------------------------------------
 * A progressive frame adds samples to every pixel across calls.  Each pixel's samples are one sequential RNG stream (kernels.cu:541-548): a pass
 * continues every pixel's stream and running colour sum where the previous pass left them (kept on the device, per device over its local rows) and
 * stores their mean.  Reference RNG stream only (RT_RNG_REFERENCE_STREAM, variant 0), PARITY and FAST, sphere and mesh scenes, every row partition and
 * device list, direct and copy-engine delivery, counters on or off.  RT_RNG_COUNTER is refused: runRenderer adds that stream's sample chunks in chunk
 * order (not one sequential sum), so a progressive total could not match it bit for bit.
 *
 * The accumulation is reset (the next pass starts at sample 0) by every init*, cleanupRenderer, setRenderOptions (any call), setCamera and
 * rtResetProgressive.  setExternalFramebuffer does not reset it: the next pass delivers the whole image to the new target.  runRenderer neither reads nor
 * changes it: a pass after a runRenderer continues where the previous pass stopped.  The accumulation buffers (16 + 4 bytes per local pixel) are
 * allocated by the first pass on each device and freed by cleanupRenderer (or a setRenderOptions that changes the device layout).
 * getRenderStats / rtLastLaunches after a pass describe THAT pass: samples = pixels x ns, its launches, kernel time, rays and counters. */

/* Adds ns samples per pixel to the progressive frame and leaves in the framebuffer (library-owned or external) the mean of ALL samples accumulated
 * since the last reset.  Blocking, like runRenderer; tx, ty ignored.  PARITY fp mode: after calls with ns_1 .. ns_k the framebuffer is bit-identical to
 * runRenderer(ns_1 + .. + ns_k).  Misuse (rt error, exit 99): before init, ns <= 0, RT_RNG_COUNTER, variant != 0, a total above
 * RT_PROGRESSIVE_MAX_SAMPLES (the cost ordering of a pass sums the rays of a pixel's 3x3 window over all its samples in 32 bits). */
#define RT_PROGRESSIVE_MAX_SAMPLES 65536
void runRendererProgressive(int ns, int tx, int ty);
/* Samples per pixel accumulated so far; 0 after init / reset. */
int rtProgressiveSamples(void);
/* The next runRendererProgressive starts again at sample 0. */
void rtResetProgressive(void);
/* Replaces the camera for the following frames (runRenderer and passes) without re-uploading the scene; resets the progressive frame. */
void setCamera(const rt_camera* cam);

/* --- first-hit guide planes ------------------------------------------------------------------------------------------------
 * Per-pixel features of the scene for a denoiser, a compositor, picking and a traversal-cost view.  For pixel (i, j) (j = global row, row 0 = bottom, like the
 * framebuffer) the CENTRE RAY is get_ray (camera.h:8-12) without the lens offset and without jitter:
 *     u = ((float)i + 0.5f) / (float)nx,  v = ((float)j + 0.5f) / (float)ny,  origin = cam.origin,  dir = unit(lower_left_corner + u*horizontal + v*vertical - origin)
 * and its first hit is found exactly as bounce 0 of a path finds it (hit(), kernels.cu:325-360, which normalises dir once more for the intersection tests,
 * the hit point and the normal's orientation; t_min = rt_render_options.t_min; the light sphere is never hit; sphere scenes: on equal t the lower caller
 * index wins; mesh scenes: scene bounds, hitBvh, then kernel_scene.floor with rt_render_options.floor = 1).  All arithmetic fp32 under the PARITY rules, in
 * both fp modes.  Planes of nx * ny entries, row 0 = bottom:
 *   RT_GUIDE_ALBEDO  3 x float  hit: the albedo the first bounce's material_scatter works with - texture lookup or material.color for RT_DIFFUSE / RT_METAL /
 *                               RT_GLASS (sphere scenes: materials[k].color); presets: hex 0x511845 for RT_FLOOR_COAT, RT_FLOOR_DIFFUSE and the floor plane, the
 *                               checker colour at the hit point for RT_FLOOR_CHECKER, the model's base colour for RT_MODEL_COAT / RT_MODEL_DIFFUSE, (1, 1, 1)
 *                               for RT_MODEL_GLOSSY / GLASS / TINTEDGLASS / SSS;  miss: the sky colour of dir (rt_render_options.sky)
 *   RT_GUIDE_NORMAL  3 x float  hit: the shading normal of hit() - (p - center) / radius, unit(cross(v1 - v0, v2 - v0)) or floor.norm, turned against the
 *                               ray; p = origin + t * direction;  miss: (0, 0, 0)
 *   RT_GUIDE_DEPTH   float      hit: t, the distance along the unit direction;  miss: FLT_MAX
 *   RT_GUIDE_PRIM    int32      hit: the caller's sphere index, the triangle's index in mesh.tris, RT_GUIDE_PRIM_FLOOR;  miss: RT_GUIDE_PRIM_NONE
 *   RT_GUIDE_NODES   int32      mesh scenes only: internal BVH nodes visited by that closest-hit query (the reference's STATS count); 0 for a ray that misses
 *                               the scene bounds; a ray that misses inside the bounds still carries its count
 * They depend on scene, camera, nx, ny, t_min, sky, floor and the row partition only.
 *
 * renderGuides fills caller-owned host arrays (pageable is fine), one per plane named in `mask`, NULL for the others; blocking.  Like an external framebuffer,
 * only the rows this process owns (stripe_rows, part_rank / part_world, all in-process devices) are written and the rest is left untouched, so ranks can fill
 * one shared mapping.  Works after either init*, follows setCamera and setRenderOptions; setExternalFramebuffer has no effect on it.  It changes nothing an
 * existing call observes: framebuffer, getRenderStats, rtLastLaunches, the progressive frame and rtProgressiveSamples stay as they were.  Misuse (rt error,
 * exit 99): before init, mask 0 or with unknown bits, a requested plane whose pointer is NULL, RT_GUIDE_NODES on a sphere scene, rt_render_options.floor = 1 on a
 * sphere scene (as runRenderer refuses it).  The device planes (at most
 * 36 bytes per local pixel) are allocated by the first call on each device, only for the planes requested, and freed by cleanupRenderer and by a
 * setRenderOptions that changes the device layout. */
enum { RT_GUIDE_ALBEDO = 1, RT_GUIDE_NORMAL = 2, RT_GUIDE_DEPTH = 4, RT_GUIDE_PRIM = 8, RT_GUIDE_NODES = 16 };
enum { RT_GUIDE_PRIM_NONE = -1, RT_GUIDE_PRIM_FLOOR = -2 };
void renderGuides(int mask, float* albedo, float* normal, float* depth, int32_t* prim, int32_t* nodes);
/* HIP-event time of the guide kernel of the last renderGuides in milliseconds, the largest over the in-process devices; 0 before the first call. */
double rtLastGuidesMs(void);

/* --- guide-driven preview denoiser ----------------------------------------------------------------------------------------
 * Turns a low-sample frame (runRendererProgressive, runRenderer) into a usable preview on the device: an edge-avoiding a-trous wavelet filter (Dammertz et al.
 * 2010, the spatial half of SVGF) steered by the guide planes above.  All arithmetic is fp32 with + - * / max abs only, every product and sum rounded on its
 * own (no FMA), operands in the order written, so the result is defined bit for bit (DESIGN.md 3.11 has the reasons for the weights).  Per pixel p = (i, j):
 * prim, n, a, t are the guide planes; valid(p) = prim(p) != RT_GUIDE_PRIM_NONE (the floor is valid); P(p)[k] = origin[k] + t * d[k] with d the centre ray's
 * direction normalised once more (the p of RT_GUIDE_NORMAL); rz(p) = 1 / (sigma_z * t(p)); with RT_DENOISE_DEMODULATE m(p)[k] = max(a(p)[k],
 * RT_DENOISE_ALBEDO_FLOOR) and c0(p)[k] = in(p)[k] / m(p)[k], without it c0 = in (no division, no multiplication at the end).
 * Iteration it = 0 .. iterations-1: s = 1 << it, K = {0.375, 0.25, 0.0625}, and with sigma_c > 0: sc = sigma_c * 2^-it, rc = 1 / (sc * sc).  For every valid p:
 *     sum = (0,0,0); wsum = 0
 *     for dy = -2..2 (outer), dx = -2..2 (inner):
 *         q = (i + dx*s, j + dy*s);  the tap adds nothing if q is outside the image or !valid(q)
 *         h = K[|dx|] * K[|dy|]
 *         if dx == 0 and dy == 0:  w = h
 *         else:
 *             dn = n(p).x*n(q).x + n(p).y*n(q).y + n(p).z*n(q).z;  wn = max(dn, 0);  normal_squarings times: wn = wn * wn
 *             e = P(q) - P(p);  pd = |n(p).x*e.x + n(p).y*e.y + n(p).z*e.z|;  wz = max(1 - pd * rz(p), 0);  wz = wz * wz
 *             w = h * wn * wz                                                       (left to right)
 *             if sigma_c > 0:  dc = c(p) - c(q);  d2 = dc.x*dc.x + dc.y*dc.y + dc.z*dc.z;  wc = max(1 - d2 * rc, 0);  wc = wc * wc;  w = w * wc
 *             if RT_DENOISE_SAME_PRIM and prim(p) != prim(q):  w = 0
 *         sum[k] += w * c(q)[k];  wsum += w
 *     c'(p)[k] = sum[k] / wsum                                                      (wsum >= 9/64: the centre tap)
 * c is the previous iteration's plane, c' the next.  At the end out(p)[k] = c(p)[k] * m(p)[k].  Pixels with !valid(p) copy in(p) to out(p) bit for bit and are
 * never a tap.  max(x, 0) is x > 0 ? x : 0 (0 for a NaN).  Non-finite input is not treated specially; denormal products are kept.
 *
 * denoiseFrame: `in` = nx*ny rt_vec3, row 0 = bottom, any host memory; NULL = the framebuffer the renderer currently delivers into (the external one if set,
 * else the library's own).  `out` = nx*ny rt_vec3 of caller-owned host memory, never NULL; it may be `in` (the input is uploaded before anything is written).
 * Blocking.  The filter needs neighbours across stripe boundaries, so it always works on the WHOLE image on ONE device, the first in-process device, whatever
 * stripe_rows, num_devices, part_rank and part_world are (it computes whole-image guide planes there itself); a multi-rank caller denoises on one rank after
 * its gather.  Follows setCamera and setRenderOptions (t_min, sky, floor) as the guides do.  Like renderGuides it changes nothing an existing call observes:
 * framebuffer (unless passed as `out`), getRenderStats, rtLastLaunches, the progressive frame, rtProgressiveSamples and rtLastGuidesMs stay as they were.  Its
 * device buffers (120 bytes per pixel) are allocated by the first call and freed by cleanupRenderer, every init* and a setRenderOptions that changes the
 * device layout.  Defaults: iterations 5, normal_squarings 5, sigma_z 0.01f, sigma_c 1.0f, flags = rtDefaultDenoiseFlags: DEMODULATE | SAME_PRIM for sphere
 * scenes (one id = one object), DEMODULATE for mesh scenes (one id = one triangle).  sigma_c is the noise scale of the demodulated colour and the caller's to
 * follow, roughly proportional to 1 / sqrt(samples per pixel); sigma_c <= 0 switches the colour weight off.  Misuse (rt error, exit 99): before init,
 * out NULL, iterations outside 1 .. RT_DENOISE_MAX_ITERATIONS, normal_squarings outside 0 .. RT_DENOISE_MAX_SQUARINGS, unknown flag bits, sigma_z not finite
 * or <= 0, sigma_c not finite, rt_render_options.floor = 1 on a sphere scene. */
enum { RT_DENOISE_DEMODULATE = 1, RT_DENOISE_SAME_PRIM = 2 };
#define RT_DENOISE_MAX_ITERATIONS 8
#define RT_DENOISE_MAX_SQUARINGS  7
#define RT_DENOISE_ALBEDO_FLOOR   0.01f
/* The default flags for the scene that is initialised; rt error before init. */
int rtDefaultDenoiseFlags(void);
void denoiseFrame(const rt_vec3* in, rt_vec3* out, int iterations, int flags, int normal_squarings, float sigma_z, float sigma_c);
/* HIP-event time of the kernels of the last denoiseFrame (prologue + iterations with the fused epilogue; not its guide kernel, not the copies) in milliseconds;
 * 0 before the first call. */
double rtLastDenoiseMs(void);

/* --- temporal accumulation for a moving camera --------------------------------------------------------------------------------
 * The temporal half of SVGF, of which denoiseFrame is the spatial half: while the camera moves, every valid pixel of the new 1 spp frame is reprojected into
 * the previous call's frame through its world-space hit point, the four pixels around that position are checked against the previous frame's geometry, and
 * what passes is blended into the new sample with a per-pixel history length N.  The loop of a camera move is setCamera, runRenderer(1), accumulateFrame,
 * denoiseFrame.  All arithmetic is fp32 with + - * / abs floor min only, every operation rounded on its own (no FMA), operands in the order
 * written, a comparison with a NaN false, dot(a,b) = a.x*b.x + a.y*b.y + a.z*b.z evaluated left to right; min(a,b) is a < b ? a : b.  So the result is
 * defined bit for bit.  For the current call prim, n, a, t, valid(p), P(p), rz(p) = 1 / (sigma_z * t(p)), m(p) and c0(p) are exactly the denoiser's above.
 * C' (o', llc', horizontal', vertical', u', v', w') is the camera of the previous call; P', n', prim', c' and N' are the planes the previous call stored.
 *     L = llc' - o';  Lu = dot(L,u');  Lv = dot(L,v');  Lw = dot(L,w');  Hl = dot(horizontal',u');  Vl = dot(vertical',v')
 * For every valid p = (i, j):
 *     e = P(p) - o';  ea = dot(e,u');  eb = dot(e,v');  ec = dot(e,w')
 *     r = Lw / ec;  s = (ea*r - Lu) / Hl;  tt = (eb*r - Lv) / Vl
 *     x = s*(float)nx - 0.5f;  y = tt*(float)ny - 0.5f
 *     candidate = r > 0 && x >= -1 && x < nx && y >= -1 && y < ny
 *     x0 = floorf(x); fx = x - x0; i0 = (int)x0     (the same for y: y0, fy, j0)
 *     sum = (0,0,0); nsum = 0; wsum = 0
 *     for dy = 0,1 (outer), dx = 0,1 (inner):
 *         q = (i0+dx, j0+dy);  bw = (dx ? fx : 1 - fx) * (dy ? fy : 1 - fy)
 *         the tap adds nothing unless ALL of these hold:  q inside the image;  N'(q) > 0;  abs(dot(n(p), P'(q) - P(p))) * rz(p) < 1;
 *             dot(n(p), n'(q)) >= normal_min;  with the SAME_PRIM flag: prim(p) == prim'(q)
 *         sum[k] += bw * c'(q)[k];  nsum += bw * N'(q);  wsum += bw
 *     if candidate && wsum > 0:
 *         h[k] = sum[k]/wsum;  N = min(nsum/wsum + 1, (float)max_history);  al = 1/N;  c(p)[k] = h[k] + al * (c0(p)[k] - h[k])
 *     else:
 *         c(p) = c0(p);  N = 1
 *     out(p)[k] = c(p)[k] * m(p)[k]                                          (no multiplication without the DEMODULATE flag)
 * Pixels with !valid(p) copy in(p) to out(p) bit for bit and store N = 0, so they are never a tap of the next call.  The first call after a reset takes the
 * else branch everywhere.  Every call stores P, n, prim, c and N of its frame as the next call's history and its camera as the next C'.  Non-finite input is
 * not treated specially.  With max_history = M a pixel that keeps its history converges to the mean of its last M frames' worth of samples (al = 1/N).
 *
 * A still camera gains nothing: the seed of a pixel's sample stream depends on the pixel alone, so a camera that does not move renders the same noise in every
 * frame and the blend returns it.  Accumulation pays off when the image moves by about a pixel or more per frame; a still camera is what
 * runRendererProgressive is for.  A scene edit (updateTriangles, updateMaterials, updateSpheres below) keeps this history and previewFrame's: what moved
 * is rejected pixel by pixel by the plane-distance, normal and (with SAME_PRIM) primitive tests above, what stayed keeps its history; rtResetHistory /
 * rtResetPreview are there for a caller who wants a clean start after an edit.  rtMarkPose in front of the edit lets what moved keep its history too
 * ("the marked pose" below).
 *
 * accumulateFrame: `in`, `out` as denoiseFrame's - `in` NULL = the framebuffer the renderer currently delivers into, `out` caller-owned and never NULL, `out`
 * may be `in`; blocking.  `history` = NULL, or nx*ny floats that receive N(p).  flags = the denoiser's bits with the same meaning, default
 * rtDefaultDenoiseFlags(); the other defaults are max_history 32, sigma_z 0.01f, normal_min 0.9f.  Like the denoiser it works on the WHOLE image on the first
 * in-process device, whatever the partition is, and computes whole-image guide planes there itself for the camera and options in force.  It changes nothing
 * an existing call observes: the framebuffer (unless passed as `out`), getRenderStats, rtLastLaunches, the progressive frame, rtProgressiveSamples,
 * rtLastGuidesMs, rtLastDenoiseMs and the result of a later denoiseFrame stay as they were; and denoiseFrame and renderGuides do not disturb the history.
 * The history lives on the device (156 bytes per pixel with the call's buffers: two sets of three 16-byte records, guide planes, input, output, N): allocated
 * by the first call, freed where the denoiser's buffers are.  It is reset - the next call has no history - by every init*, cleanupRenderer, rtResetHistory
 * and every setRenderOptions call; setCamera, setExternalFramebuffer, runRenderer*, renderGuides and denoiseFrame do not reset it.
 * Misuse (rt error, exit 99): before init, out NULL, unknown flag bits, max_history outside 1 .. RT_ACCUM_MAX_HISTORY, sigma_z not finite or <= 0,
 * normal_min not finite or outside [-1, 1], rt_render_options.floor = 1 on a sphere scene; rtResetHistory or rtHistoryFrames before init. */
#define RT_ACCUM_MAX_HISTORY 1024
void accumulateFrame(const rt_vec3* in, rt_vec3* out, float* history, int flags, int max_history, float sigma_z, float normal_min);
/* The next accumulateFrame has no history. */
void rtResetHistory(void);
/* accumulateFrame calls since the last reset; 0 after init / reset. */
int rtHistoryFrames(void);
/* HIP-event time of the kernel of the last accumulateFrame (not its guide kernel, not the copies) in milliseconds; 0 before the first call. */
double rtLastAccumulateMs(void);

/* --- variance-guided accumulate + filter, one device pass ----------------------------------------------------------------------
 * previewFrame is accumulateFrame and denoiseFrame in one call with what SVGF (Schied et al. 2017) puts between them: the first two moments of the luminance
 * are accumulated with the colour, a per-pixel variance comes from them - from the 7 x 7 neighbourhood where the history is shorter than
 * RT_PREVIEW_MIN_HISTORY - and that variance, not a caller's sigma_c, sets the colour width of the a-trous filter pixel by pixel and is filtered along with the
 * colour.  The accumulated frame stays on the device and the guide kernel runs once.  The loop of a camera move is setCamera, runRenderer(1), previewFrame
 * (INTEGRATION.md 2).  All arithmetic is fp32 with + - * / abs floor min max sqrt only, every operation rounded on its own (no FMA), operands in the order
 * written, sqrt correctly rounded, max(x, 0) = x > 0 ? x : 0, a comparison with a NaN false, so the result is defined bit for bit.
 * lum(x) = 0.2126f*x[0] + 0.7152f*x[1] + 0.0722f*x[2], left to right.  valid, P, rz, m, c0, n, prim are the denoiser's above.
 * Stage T (temporal) is accumulateFrame's definition word for word for c(p) and N(p), with C', P', n', prim', c', N', M1', M2' the camera and the planes the
 * previous previewFrame stored, and two more accumulated quantities:
 *     l0 = lum(c0(p));  q0 = l0*l0;  in the tap loop additionally  m1sum += bw * M1'(q);  m2sum += bw * M2'(q)
 *     if blended:  h1 = m1sum/wsum;  M1 = h1 + al * (l0 - h1);  h2 = m2sum/wsum;  M2 = h2 + al * (q0 - h2)          else:  M1 = l0;  M2 = q0
 * Every call stores P, n, prim, c, N, M1, M2 of its frame and its camera for the next call; c is the UNFILTERED accumulated colour.
 * Stage V (variance), for every valid p:
 *     if N(p) >= RT_PREVIEW_MIN_HISTORY:  var = max(M2 - M1*M1, 0)
 *     else:
 *         s1 = s2 = ws = 0
 *         for dy = -3..3 (outer), dx = -3..3 (inner):
 *             q = (i + dx, j + dy);  the tap adds nothing if q is outside the image or !valid(q)
 *             if dx == 0 and dy == 0:  w = 1
 *             else:  w = wn * wz, wn and wz exactly the denoiser's (normal_squarings, rz(p));  if RT_DENOISE_SAME_PRIM and prim(p) != prim(q):  w = 0
 *             s1 += w * M1(q);  s2 += w * M2(q);  ws += w
 *         a1 = s1/ws;  a2 = s2/ws;  var = max(a2 - a1*a1, 0) * (4.0f / N(p))
 * Stage A (a-trous) on the pair (c, var), it = 0 .. iterations-1, s = 1 << it, K and h the denoiser's.  For every valid p:
 *     rl = 1 / (sigma_l * sqrt(var(p)) + RT_PREVIEW_LUM_EPS);  lp = lum(c(p));  sum = (0,0,0);  vsum = 0;  wsum = 0
 *     the 25 taps in the denoiser's order, under its validity rules:
 *         if dx == 0 and dy == 0:  w = h
 *         else:
 *             w = h * wn * wz                                                       (left to right)
 *             wl = max(1 - abs(lp - lum(c(q))) * rl, 0);  wl = wl * wl;  w = w * wl
 *             if RT_DENOISE_SAME_PRIM and prim(p) != prim(q):  w = 0
 *         sum[k] += w * c(q)[k];  vsum += (w*w) * var(q);  wsum += w
 *     c'(p)[k] = sum[k] / wsum;  var'(p) = vsum / (wsum*wsum)
 * At the end out(p)[k] = c(p)[k] * m(p)[k] (no multiplication without RT_DENOISE_DEMODULATE).  Pixels with !valid(p) copy in(p) to out(p) bit for bit, store
 * N = 0, have variance 0 and are never a tap of any stage.  Non-finite input is not treated specially.
 *
 * previewFrame: `in`, `out` and `history` exactly as accumulateFrame's - `in` NULL = the framebuffer the renderer currently delivers into, `out` caller-owned
 * and never NULL, `out` may be `in`, `history` NULL or nx*ny floats that receive N(p); blocking.  `variance` = NULL, or nx*ny floats that receive var(p) of
 * stage V (0 without a first hit).  Defaults: flags rtDefaultDenoiseFlags(), max_history 32, iterations 5, normal_squarings 5, sigma_z 0.01f, normal_min 0.9f,
 * sigma_l 4.0f.  It works on the WHOLE image on the first in-process device and keeps a history of its own, independent of accumulateFrame's: neither call
 * disturbs the other, nor denoiseFrame, renderGuides, the framebuffer (unless passed as `out`), getRenderStats, rtLastLaunches, the progressive frame or the
 * other rtLast*Ms values.  Its history is reset where accumulateFrame's is - every init*, cleanupRenderer, every setRenderOptions - and by rtResetPreview; its
 * device buffers (208 bytes per pixel) are allocated by the first call and freed where the other passes' are.  Misuse (rt error, exit 99): before init, out
 * NULL, unknown flag bits, max_history outside 1 .. RT_ACCUM_MAX_HISTORY, iterations outside 1 .. RT_DENOISE_MAX_ITERATIONS, normal_squarings outside
 * 0 .. RT_DENOISE_MAX_SQUARINGS, sigma_z not finite or <= 0, normal_min not finite or outside [-1, 1], sigma_l not finite or <= 0, rt_render_options.floor = 1
 * on a sphere scene; rtResetPreview or rtPreviewFrames before init. */
#define RT_PREVIEW_MIN_HISTORY 4.0f     /* below it the variance is the spatial estimate */
#define RT_PREVIEW_LUM_EPS     1e-4f
void   previewFrame(const rt_vec3* in, rt_vec3* out, float* history, float* variance, int flags, int max_history,
                    int iterations, int normal_squarings, float sigma_z, float normal_min, float sigma_l);
void   rtResetPreview(void);      /* the next previewFrame has no history */
int    rtPreviewFrames(void);     /* calls since the last reset */
double rtLastPreviewMs(void);     /* HIP-event time of its kernels (not the guide kernel, not the copies); 0 before the first call */

/* --- display transform: exposure, tone map, sRGB bytes ------------------------------------------------------------------------
 * displayFrame turns a linear fp32 frame into the 8-bit sRGB picture a viewer, a video encoder or rtWritePPM (rt_host.h) wants, on the device: 4 bytes per pixel
 * come back instead of 12, and the one powf per channel runs there.  The loop of a camera move becomes setCamera, runRenderer(1), previewFrame, displayFrame
 * with RT_DISPLAY_FROM_PREVIEW.  All arithmetic is fp32, every operation rounded on its own (no FMA), operands in the order written, a
 * comparison with a NaN false, max(a, b) = a > b ? a : b; lum is previewFrame's; powf is glibc's (csrc/rt_glibc_powf_pos.h restates it for the device).  So the
 * bytes are defined bit for bit, and rtDisplayFrameHost (rt_host.h) computes the same ones without a GPU.
 * Exposure:  without RT_DISPLAY_AUTO_EXPOSURE E_used = exposure; with it E_used = E * exposure, E from the next stage.
 * Auto exposure, over the INPUT frame.  For every pixel p:
 *     l = lum(in(p));  b = (int)(bits(l) >> 20) - ((127 - 16) << 3)                  (8 bins per octave over 2^-16 .. 2^16)
 *     p is counted in bin min(b, RT_DISPLAY_BINS - 1) iff l is finite, l > 0 and b >= 0
 *     T = the sum of the bins.  T == 0: target = 1.  Else m = the smallest bin with 2 * cum(m) >= T (integers; cum(m) = bins 0 .. m),
 *         Lmed = the float with bits ((m + ((127 - 16) << 3)) << 20) | (1 << 19) (the middle of bin m),  target = RT_DISPLAY_KEY / Lmed
 *     the first RT_DISPLAY_AUTO_EXPOSURE call after a reset: E = target;  otherwise, E' being the E of the previous such call: E = E' + adapt * (target - E')
 * The counts are integers: the result does not depend on the order in which pixels are counted.
 * Per pixel p = (i, j) and channel k:
 *     x[k] = in(p)[k] * E_used
 *     RT_TONEMAP_NONE:      y[k] = x[k]
 *     RT_TONEMAP_REINHARD:  y[k] = x[k] / (1 + max(lum(x), 0))
 *     RT_TONEMAP_ACES:      a = max(x[k], 0);  y[k] = (a * (2.51f*a + 0.03f)) / (a * (2.43f*a + 0.59f) + 0.14f)            (Narkowicz's fit)
 *     s = max(y[k], 0)  (a NaN gives 0);  s = max(1.055f * powf(s, 0.416666667f) - 0.055f, 0);  t = s * 255.9f              (rtLinearToSRGB's lines)
 *     with RT_DISPLAY_DITHER instead  t = s * 255.0f + ((float)B[j & 7][i & 7] + 0.5f) / 64.0f,  B = RT_DISPLAY_BAYER8, (i, j) the INPUT coordinates
 *     u[k] = t >= 255.0f ? 255 : (uint32)t
 * The bytes of a pixel are u[0], u[1], u[2], 255.  Row 0 is the bottom row, as in the framebuffer; RT_DISPLAY_TOP_DOWN writes input row j to output row
 * ny - 1 - j (the order of a PPM or a video frame).  The clamp before the conversion is part of the definition: rtLinearToSRGB converts first, and C leaves
 * (uint32_t) of a float from 2^32 up undefined - x86-64 returns garbage there, and 0 for +inf, where this call returns 255.  The two agree on every finite
 * input below 2^40 (tests/test_display_api.py).  -inf and NaN encode to 0.
 *
 * displayFrame: `in` = nx*ny rt_vec3, row 0 = bottom, any host memory; NULL = the framebuffer the renderer currently delivers into.  With
 * RT_DISPLAY_FROM_PREVIEW `in` must be NULL and the source is the output of the last previewFrame, still on the device: nothing is uploaded.  `out_rgba` =
 * nx*ny*4 bytes of caller-owned host memory, never NULL.  Blocking.  Like the preview passes it works on the WHOLE image on the first in-process device,
 * whatever the partition is.  It changes nothing an existing call observes: the framebuffer, getRenderStats, rtLastLaunches, the progressive frame, the
 * histories of accumulateFrame and previewFrame and every other rtLast*Ms stay as they were.  Its state is E' and the last histogram: reset - the next
 * RT_DISPLAY_AUTO_EXPOSURE call adapts from nothing, the histogram is zero - by every init*, cleanupRenderer, every setRenderOptions and rtResetDisplay; a call
 * without RT_DISPLAY_AUTO_EXPOSURE neither reads nor changes it.  E' lives on the device.  The device buffers (16 bytes per pixel and RT_DISPLAY_BINS + 2 words)
 * are allocated by the first call and freed where the other passes' are.  Defaults: flags 0, RT_TONEMAP_NONE, exposure 1, adapt 1.
 * Misuse (rt error, exit 99): before init (the four helpers below as well), out_rgba NULL, unknown flag bits, an unknown tonemap, exposure not finite or <= 0,
 * adapt not finite or outside (0, 1], RT_DISPLAY_FROM_PREVIEW with `in` non-NULL or without a previewFrame since init / the last reset of its history. */
enum { RT_DISPLAY_TOP_DOWN = 1, RT_DISPLAY_DITHER = 2, RT_DISPLAY_AUTO_EXPOSURE = 4, RT_DISPLAY_FROM_PREVIEW = 8 };
enum { RT_TONEMAP_NONE = 0, RT_TONEMAP_REINHARD = 1, RT_TONEMAP_ACES = 2 };
#define RT_DISPLAY_BINS 256
#define RT_DISPLAY_KEY  0.18f
/* the 8 x 8 ordered-dither (Bayer) matrix, 0 .. 63, rows B[0] .. B[7]: the initialiser of an array [8][8] */
#define RT_DISPLAY_BAYER8 { {  0, 32,  8, 40,  2, 34, 10, 42 }, { 48, 16, 56, 24, 50, 18, 58, 26 }, { 12, 44,  4, 36, 14, 46,  6, 38 }, \
                            { 60, 28, 52, 20, 62, 30, 54, 22 }, {  3, 35, 11, 43,  1, 33,  9, 41 }, { 51, 19, 59, 27, 49, 17, 57, 25 }, \
                            { 15, 47,  7, 39, 13, 45,  5, 37 }, { 63, 31, 55, 23, 61, 29, 53, 21 } }
void   displayFrame(const rt_vec3* in, uint8_t* out_rgba, int flags, int tonemap, float exposure, float adapt);
float  rtLastExposure(void);                       /* E_used of the last displayFrame; 1 before the first */
int    rtDisplayHistogram(uint32_t* out, int cap); /* the bins of the last RT_DISPLAY_AUTO_EXPOSURE call (zero after a reset): min(cap, RT_DISPLAY_BINS) words; returns RT_DISPLAY_BINS */
void   rtResetDisplay(void);                       /* the next RT_DISPLAY_AUTO_EXPOSURE call adapts from nothing */
double rtLastDisplayMs(void);                      /* HIP-event time of its kernels (not the copies); 0 before the first call */

/* --- batched ray queries: the caller's own rays -----------------------------------------------------------------------------
 * traceRays finds the first hit of n rays of the caller's, occludedRays says for each whether anything lies between its bounds: picking, autofocus (the t under
 * the cursor is the camera's focus_dist), fitting a camera to a model, visibility and ambient-occlusion probes, light placement, collision tests.  rtCentreRays
 * (rt_host.h) turns a pixel into the ray renderGuides sends through it.  For ray k: o = org[3k..3k+2], d = dir[3k..3k+2], tmin = t_min[k] or, with t_min NULL,
 * rt_render_options.t_min; tmax = t_max[k] or, with t_max NULL, FLT_MAX.
 *   Direction   the ray is the reference's ray(o, d) (ray.h:9): dn = d / sqrt(d.x*d.x + d.y*d.y + d.z*d.z), and every distance is along dn.  The caller's
 *               direction is raw and is normalised ONCE (the guide kernels normalise the centre ray, already unit, a second time: a caller who wants their
 *               bits passes the unit direction, as rtCentreRays returns it).
 *   Arithmetic  fp32 under the PARITY rules, in both fp modes.  The light sphere is never hit.
 *   Spheres     closest = tmax; for s = 0 .. n_spheres-1 in the caller's order: x = sphereHit(s, ray, tmin, closest) (intersections.h:85-104); if x < closest:
 *               closest = x, prim = s.  So on equal t the lower caller index wins, as in renderGuides, and a hit at tmax itself is none.
 *   Meshes      if hit_bbox(scene bounds, ray, tmax) fails the ray misses and nodes = 0.  Otherwise x = hitBvh(ray, tmin, tmax, is_shadow = 0)
 *               (kernels.cu:154-224): a hit iff x < tmax.  On a miss with rt_render_options.floor = 1: x = planeHit(kernel_scene.floor, ray, tmin, tmax), a hit
 *               iff x < FLT_MAX, prim = RT_GUIDE_PRIM_FLOOR.  The floor is tested against the ray's own tmax (hit() passes FLT_MAX there: the two agree
 *               whenever tmax is FLT_MAX).
 * Planes of n entries; prim and normal have the meaning and the encoding of RT_GUIDE_PRIM and RT_GUIDE_NORMAL:
 *   RT_RAY_T       float      hit: the distance along dn;  miss: FLT_MAX
 *   RT_RAY_PRIM    int32      hit: the caller's sphere index, the triangle's index in mesh.tris, RT_GUIDE_PRIM_FLOOR;  miss: RT_GUIDE_PRIM_NONE
 *   RT_RAY_NORMAL  3 x float  hit: the shading normal of hit() - (p - center) / radius, unit(cross(v1 - v0, v2 - v0)) or floor.norm - turned against dn, with
 *                             p = o + t * dn;  miss: (0, 0, 0)
 *   RT_RAY_UV      2 x float  hit of a triangle: hitU, hitV of triangleHit (intersections.h:54-83);  a sphere, the floor, a miss: (0, 0)
 *   RT_RAY_NODES   int32      mesh scenes only: internal BVH nodes visited by that query, as RT_GUIDE_NODES: 0 for a ray that misses the scene bounds, and a
 *                             ray that misses inside the bounds still carries its count
 * occludedRays writes one byte per ray.  Sphere scenes: 1 iff some sphere has sphereHit(s, ray, tmin, tmax) < FLT_MAX (whatever the scan order).  Mesh scenes:
 * 1 iff the bounds test passes and hitBvh(ray, tmin, tmax, is_shadow = 1) < tmax.  The floor never occludes, exactly as the reference's shadow rays never
 * test it.
 * The caller owes 0 <= tmin < tmax, neither a NaN, and d finite and non-zero.  A tmax above FLT_MAX (+inf, a caller's "no bound") is taken as FLT_MAX:
 * everything above is stated with min(tmax, FLT_MAX) (taken literally, tmax = +inf would accept the FLT_MAX a miss returns as a hit).  Rays are not
 * validated one by one: a ray that breaks this gets an unspecified result, the call still returns, and every other ray's result is unaffected.
 *
 * Both calls are blocking and answer in the caller's ray order.  org and dir hold n x 3 floats; t_min and t_max n floats each, or NULL.  The outputs are
 * caller-owned host arrays (pageable is fine): traceRays takes one per plane named in `mask` and NULL for the others - t, prim, nodes of n entries, normal of
 * n x 3, uv of n x 2 floats - and nothing is written through a pointer whose plane is not named.  All rays run on the first in-process device, whatever
 * stripe_rows, num_devices, part_rank and part_world are (every device holds the whole scene), RT_RAY_CHUNK = 1 << 22 rays at a time - upload, kernel,
 * download -, so the device buffers (65 bytes per ray of the largest chunk seen, only for the arrays that were passed) stay below ~273 MB; they are freed
 * where the passes' buffers are: cleanupRenderer, every init*, a setRenderOptions that changes the device layout.  The calls follow setRenderOptions (t_min
 * as the default, floor) and do not depend on the camera, nx, ny or setCamera.  They change nothing an existing call observes: the framebuffer, getRenderStats,
 * rtLastLaunches, the progressive frame, the histories of accumulateFrame / previewFrame / displayFrame and every other rtLast*Ms stay as they were.  n == 0
 * returns at once: nothing is written and rtLastRaysMs stays as it was.  Misuse (rt error, exit 99): before init (rtLastRaysMs as well), n < 0, org or dir
 * NULL with n > 0, mask 0 or with unknown bits, a requested plane whose pointer is NULL, RT_RAY_NODES on a sphere scene, occluded NULL,
 * rt_render_options.floor = 1 on a sphere scene. */
enum { RT_RAY_T = 1, RT_RAY_PRIM = 2, RT_RAY_NORMAL = 4, RT_RAY_UV = 8, RT_RAY_NODES = 16 };
#define RT_RAY_CHUNK (1 << 22)
void   traceRays(int n, const float* org, const float* dir, const float* t_min, const float* t_max, int mask,
                 float* t, int32_t* prim, float* normal, float* uv, int32_t* nodes);
void   occludedRays(int n, const float* org, const float* dir, const float* t_min, const float* t_max, uint8_t* occluded);
double rtLastRaysMs(void);   /* HIP-event time of the ray kernels of the last traceRays / occludedRays (not the copies), summed over its chunks; 0 before the first */

/* --- path-tracing a list of pixels: a region after an edit, the pixel under the cursor, a caller-driven adaptive loop ------------------
 * renderPixels path-traces n caller-chosen pixels of the image of init* with a caller-chosen number of samples each, and can continue a pixel's stream
 * where an earlier call stopped.  Every pixel is defined by what runRenderer stores there:
 *   Pixel k        (i, j) = (ij[2k], ij[2k+1]): column, then row with 0 = bottom - rtCentreRays' convention.  Duplicates and any order are allowed; every
 *                  entry is answered independently, in the caller's order.
 *   Sample range   c = ns ? ns[k] : ns_all samples are rendered for pixel k: samples f .. f+c-1 of that pixel's stream, f = first ? first[k] : 0.
 *   f == 0         the reference's per-pixel loop (kernels.cu:541-568): the seed from the global pixel id j*nx + i, ONE sequential xorshift stream over
 *                  the pixel's samples, sum += sample in sample order.
 *   f > 0          state[4k .. 4k+2] are the bits of the fp32 colour sum after f samples, state[4k+3] is the stream's xorshift word: the pixel resumes from
 *                  them (what a call with `state` returned for the same pixel after f samples; nothing else is checked).
 *   Outputs        out, state and rays may each be NULL.  state (read for f > 0, written if non-NULL: in place) receives the sum and the word after sample
 *                  f+c-1;  out[k] = sum / (float)(f + c);  rays[k] = the closest-hit queries of these c samples - the `rays` of getRenderStats with
 *                  counters = 1, shadow rays not included.
 * The frame's options hold: camera, max_depth, t_min, sky, nee, rr, light, floor.  In RT_FP_PARITY out[k] is bit-identical to the pixel runRenderer(f + c)
 * stores at (i, j), for any split of f + c into calls; in RT_FP_FAST the FAST objects' arithmetic runs: the same estimate with no bit promise, as for
 * runRenderer itself.  The result does not depend on stripe_rows, part_rank / part_world or the device list: all pixels run on the first in-process device,
 * as the ray queries do, RT_PIXEL_CHUNK pixels at a time - upload, kernel, download -; the device buffers (48 bytes per pixel of the largest chunk seen,
 * only for the arrays that were passed) are freed where the ray buffers are.  The call is blocking and follows setCamera, setRenderOptions and the scene
 * edits.  It changes nothing an existing call observes: the framebuffer, getRenderStats, rtLastLaunches, rtLastSphereForm, the progressive frame and
 * rtProgressiveSamples, the cost map of sphere frames, every history and every other rtLast*Ms stay as they were.  n == 0 returns at once: nothing is
 * written and rtLastPixelsMs stays as it was.  Misuse (rt error, exit 99), checked on the host before anything is uploaded: before init (rtLastPixelsMs as
 * well), n < 0, ij NULL, out, state and rays all NULL, a pixel outside [0, nx) x [0, ny), c < 1 or f < 0, f + c > RT_PROGRESSIVE_MAX_SAMPLES, first given
 * without state, a resumed pixel (f > 0) whose stream word is 0 (no stream ever holds it: the xorshift would stand still), RT_RNG_COUNTER or variant != 0
 * (as runRendererProgressive refuses them), rt_render_options.floor = 1 or nee = 1 on a sphere scene (as runRenderer refuses them). */
#define RT_PIXEL_CHUNK (1 << 22)
void   renderPixels(int n, const int32_t* ij, int ns_all, const int32_t* ns, const int32_t* first,
                    uint32_t* state, rt_vec3* out, uint32_t* rays);
double rtLastPixelsMs(void);   /* HIP-event time of the pixel kernels of the last renderPixels, summed over its chunks; 0 before the first */

/* --- path-tracing the caller's own rays: light probes, cube maps at a point, lightmap and vertex bakes, a camera model of the caller's own ---------
 * radianceRays answers "how much light arrives at this point from this direction" for n caller-chosen rays: the whole path tracer of a frame behind a ray
 * that does not come from the camera, with a caller-chosen number of samples each, resumable like renderPixels.
 *   Ray k          o = org[3k .. 3k+2], d = dir[3k .. 3k+2].  d is raw and is normalised once: dn = d / sqrt(d.x*d.x + d.y*d.y + d.z*d.z), traceRays' rule.
 *                  The caller owes a finite o and a finite, non-zero d; rays are not validated one by one.  Duplicates and any order are allowed; every
 *                  entry is answered independently, in the caller's order.
 *   Seed id        id = ids ? ids[k] : (uint32_t)k - k the index in the caller's list, whatever the chunking.  Two entries with one id and one ray are equal.
 *   Sample range   c = ns ? ns[k] : ns_all samples are traced for ray k: samples f .. f+c-1 of that ray's stream, f = first ? first[k] : 0.
 *   f == 0         the stream word starts at the reference's seed of `id` (kernels.cu:541-542), the sum at 0: ONE sequential xorshift stream over the ray's
 *                  samples, sum += sample in sample order.
 *   f > 0          state[4k .. 4k+2] are the bits of the fp32 colour sum after f samples, state[4k+3] is the stream's xorshift word: the ray resumes from
 *                  them (what a call with `state` returned for the same ray after f samples; nothing else is checked).
 *   Sample         in this order: two rnd() draws, discarded (the jitter draws of kernels.cu:549-550); one random_in_unit_disk, discarded (the lens draw of
 *                  camera.h: its rejection loop as it stands, however many words it takes); then the loop of color() (kernels.cu:397-531) from origin o
 *                  with direction dn, specular = false, inside = false, attenuation 1, under the options in force: max_depth, t_min, sky, rr, and for
 *                  meshes nee, light, floor and the textures; sum += colour.  With max_depth <= 0 a sample draws its head and is black, without a ray.
 *   Outputs        out, state and rays may each be NULL, not all three.  state (read for f > 0, written if non-NULL: in place) receives the sum and the word
 *                  after sample f+c-1;  out[k] = sum / (float)(f + c);  rays[k] = the closest-hit queries of these c samples, shadow rays not included.
 * The head of a sample burns the camera's draws so that a ray is exactly a one-pixel render through a pinhole at o: for o and T without negative-zero
 * coordinates and d = fl(T - o), ray (o, d, id) at f + c samples is bit-identical in RT_FP_PARITY to the pixel with global id `id` that runRenderer(f + c)
 * stores under rtPinholeCamera(o, T) (rt_host.h), for any split of f + c into calls.  That gives the call a CPU oracle and a check inside the library, for
 * about five RNG words per sample against a path of rays.  In RT_FP_FAST the FAST objects' arithmetic runs: the same estimate with no bit promise.
 * The result does not depend on the camera, nx, ny, setCamera, stripe_rows, part_rank / part_world or the device list: all rays run on the first in-process
 * device, RT_RAY_CHUNK rays at a time - upload, kernel, download -; the device buffers (68 bytes per ray of the largest chunk seen - org 12, dir 12, ids 4,
 * ns 4, first 4, state 16, out 12, rays 4 -, only for the arrays that were passed) are freed where the ray buffers are.  The call is blocking and follows
 * setRenderOptions, the scene edits and rebuildBvh.  RT_PIXELS_WAVES caps its waves as it caps renderPixels'.  It changes nothing an existing call observes:
 * the framebuffer, getRenderStats, rtLastLaunches, rtLastSphereForm, the progressive frame and rtProgressiveSamples, the cost map of sphere frames, every
 * history and every other rtLast*Ms stay as they were.  n == 0 returns at once: nothing is written and rtLastRadianceMs stays as it was.  Misuse (rt error,
 * exit 99), checked on the host before anything is uploaded: before init (rtLastRadianceMs as well), n < 0, org or dir NULL, out, state and rays all NULL,
 * c < 1 or f < 0, f + c > RT_PROGRESSIVE_MAX_SAMPLES, first given without state, a resumed ray (f > 0) whose stream word is 0, RT_RNG_COUNTER or
 * variant != 0, rt_render_options.floor = 1 or nee = 1 on a sphere scene (the frame conditions renderPixels refuses). */
void   radianceRays(int n, const float* org, const float* dir, const uint32_t* ids, int ns_all, const int32_t* ns,
                    const int32_t* first, uint32_t* state, rt_vec3* out, uint32_t* rays);
double rtLastRadianceMs(void);   /* HIP-event time of the radiance kernels of the last radianceRays, summed over its chunks; 0 before the first */

/* --- gathering at points: irradiance, SH9 and visibility per point - probes, lightmap and vertex bakes, an AO / indirect-light plane ---------
 * gatherRadiance answers "what arrives at this point" for n caller-named points: the device draws the directions, traces them with the kernels of
 * radianceRays (RT_GATHER_IRRADIANCE, RT_GATHER_SH9) or occludedRays (RT_GATHER_VISIBILITY), unchanged, and reduces them per point in a fixed order.  Only the
 * points go up and only per-point results come back.  All arithmetic of the generator and of the reduction is fp32, every operation rounded on its own (no
 * FMA), operands in the order written, sqrt and / correctly rounded, dot(a, b) = a.x*b.x + a.y*b.y + a.z*b.z from left to right - in both fp modes.
 *   Point k        the index in the caller's list, whatever the chunking.  P = pos[3k .. 3k+2], N = nrm[3k .. 3k+2].  The caller owes finite P and, outside
 *                  SH9, a finite, non-zero N; points are not validated one by one.
 *   Origin         IRRADIANCE, VISIBILITY: Nn = N / sqrt(dot(N, N)) (three divisions), o[a] = P[a] + bias * Nn[a] - computed also when bias is 0.
 *                  SH9: o = P; nrm and bias are ignored, nrm may be NULL.
 *   Direction m    m = first .. first+dirs-1.  g = base_id + (uint32_t)((uint64_t)k * dirs_total + m), modulo 2^32.  The direction stream is the xorshift
 *                  word wd = pixel_seed(~g) (kernels.cu:541-542); rnd is rnd.h:5-18.  Drawn as rnd.h:41-49 draws: repeat { x = 2*rnd(wd) - 1; y likewise;
 *                  z likewise; l2 = x*x + y*y + z*z } while (!(l2 < 1) || l2 == 0) - the zero rejection is added to the reference's loop so that u is
 *                  always defined -; u = (x, y, z) / sqrt(l2) (three divisions).
 *                  IRRADIANCE, VISIBILITY: D = Nn + u, and D = Nn where all three components of that sum are zero: a cosine-distributed direction about Nn.
 *                  SH9: D = u, uniform on the sphere.
 *   Ray (k, m)     IRRADIANCE, SH9: exactly radianceRays' ray (o, D, id = g) at ns samples from sample 0: L = its out, r = its rays.  Its path stream is
 *                  pixel_seed(g), the direction stream pixel_seed(~g): the two do not share words.  (Ids near 2^31 make ~g meet other rays' g: harmless, but
 *                  that ray's directions are correlated with another ray's path.)
 *                  VISIBILITY: exactly occludedRays' ray (o, D, tmin = rt_render_options.t_min, tmax = max_dist > 0 ? max_dist : FLT_MAX):
 *                  v = occluded ? 0.0f : 1.0f, r = 0; ns is ignored.
 *   Reduction      per point, m ascending.  A starts at 0 when first == 0 (acc is not read then), else at acc[k*W ..]; W = rtGatherWidth(mode).
 *                  IRRADIANCE (W = 3)   A[c] += L[c].
 *                  SH9 (W = 27)         A[3i + c] += L[c] * y_i (the product rounded, then added), i = 0 .. 8, with D = (X, Y, Z) raw:
 *                                       y0 = 0.282095f             y1 = 0.488603f * Y          y2 = 0.488603f * Z            y3 = 0.488603f * X
 *                                       y4 = 1.092548f * (X * Y)   y5 = 1.092548f * (Y * Z)    y6 = 0.315392f * (3.0f * (Z * Z) - 1.0f)
 *                                       y7 = 1.092548f * (X * Z)   y8 = 0.546274f * (X * X - Y * Y)
 *                  VISIBILITY (W = 1)   A[0] += v (exact: the counts stay below 2^24).
 *   Outputs        acc, out (W floats per point) and rays (one word per point) may each be NULL, not all three.  acc receives A.  With M = (float)(first + dirs):
 *                  out[k*W + j] = A[j] / M (IRRADIANCE, VISIBILITY), (A[j] * 12.566371f) / M (SH9).  rays[k] = the sum of this call's r.
 * So first / acc resume a point the way `state` resumes a ray: any split of dirs_total into calls is bit-identical to one call.  IRRADIANCE is irradiance / pi -
 * the radiance a white Lambertian surface at the point would reflect; SH9 the nine real spherical-harmonic coefficients of the incoming radiance per channel
 * (coefficient i of channel c at 3i + c); VISIBILITY cosine-weighted openness, i.e. ambient occlusion within max_dist.  Over the planes of renderGuides (hit
 * point = origin + depth * d, with the normal plane) the same call gives an ambient-occlusion or indirect-light plane.
 * The call is blocking and runs on the first in-process device, max(1, RT_RAY_CHUNK / dirs) points at a time - upload, generate, trace, reduce, download -;
 * the device buffers (per ray of the largest chunk seen: org 12, dir 12, and ids 4, out 12, rays 4 = 44 bytes in the radiance modes, t_max 4, occluded 1 = 29
 * bytes in VISIBILITY; per point: pos 12, nrm 12, acc 4W, out 4W, rays 4) are its own and are freed where the ray buffers are.  It follows setRenderOptions,
 * the scene edits and rebuildBvh; RT_PIXELS_WAVES caps its path waves as it caps radianceRays'.  It changes nothing another call observes: the framebuffer,
 * getRenderStats, rtLastLaunches, the progressive frame, every history, the buffers of radianceRays and traceRays and every other rtLast*Ms (rtLastRadianceMs
 * and rtLastRaysMs included) stay as they were.  n == 0 returns at once: nothing is written and rtLastGatherMs stays as it was.
 * rtGatherDirections runs the generator kernel alone and downloads it: entry k*dirs + (m - first) of org (3 floats), dir (3 floats, raw D) and ids (g); each
 * pointer may be NULL, not all three.  rtGatherDirectionsHost (rt_host.h) is its CPU twin.  rtGatherWidth needs no init and never exits for a known mode.
 * Misuse (rt error, exit 99), checked on the host before any device work: before init (rtLastGatherMs as well), n < 0, pos NULL, nrm NULL outside SH9, an
 * unknown mode, dirs < 1 or first < 0, first + dirs > dirs_total, dirs_total > RT_GATHER_MAX_DIRS, first > 0 without acc, acc, out and rays all NULL (org, dir
 * and ids all NULL), bias not finite, max_dist a NaN or negative; in the radiance modes ns outside 1 .. RT_PROGRESSIVE_MAX_SAMPLES and every frame condition
 * radianceRays refuses; in every mode rt_render_options.floor = 1 on a sphere scene. */
enum { RT_GATHER_IRRADIANCE = 0, RT_GATHER_SH9 = 1, RT_GATHER_VISIBILITY = 2 };
#define RT_GATHER_MAX_DIRS 65536
int    rtGatherWidth(int mode);          /* floats per point in acc / out: 3, 27, 1; never exits for a known mode */
void   gatherRadiance(int n, const float* pos, const float* nrm, int mode, int first, int dirs, int dirs_total, int ns, uint32_t base_id,
                      float bias, float max_dist, float* acc, float* out, uint32_t* rays);
void   rtGatherDirections(int n, const float* pos, const float* nrm, int mode, int first, int dirs, int dirs_total,
                          uint32_t base_id, float bias, float* org, float* dir, uint32_t* ids);   /* the generator kernel alone, downloaded */
double rtLastGatherMs(void);   /* HIP-event time of generator + trace + reduce of the last gatherRadiance, summed over its chunks; 0 before the first */

/* --- baking texels: the mesh's UV atlas rasterised on the device, a gather per covered texel, texel planes back ---------------------------------
 * rasterTexels turns the live triangles' texCoords and an atlas size into texel points; bakeTexels does that and gathers at them with gatherRadiance's
 * generator, kernels and reduction, scatters the results back into texel planes and dilates the chart borders.  Nothing goes up (but acc, to resume); only
 * texel planes come back.  Mesh scenes only.  All arithmetic is fp32, in both fp modes: every operation is rounded on its own (no FMA), operands are in the
 * order written, / and sqrt are correctly rounded, a comparison with a NaN is false.
 * The raster.  Atlas W x H, with 1 <= W, H <= RT_TEXEL_MAX_SIZE (8192).
 *   Texel          t = y*W + x.  Row 0 is v near 0, which is the row the renderer's own texture lookup addresses first.
 *   Sample point   s = (((float)x + 0.5f) / (float)W, ((float)y + 0.5f) / (float)H).  UVs are not wrapped.  What lies outside [0,1]^2 is clipped.
 *   Candidates     every slot k in [0, numTris) of the live leaf-ordered triangle array whose v[0].x is not +-inf.  This is the index RT_GUIDE_PRIM reports.
 *                  It follows updateTriangles and rebuildBvh.
 *   UV vertices    a = tc[0..1], b = tc[2..3], c = tc[4..5].  This is the order mesh_texel uses: weight hu on b, hv on c.
 *   Box test       (part of the definition, so that a texel walk bounded by the triangle's UV box is exact, not merely conservative):
 *                  umin <= s.x && s.x <= umax && vmin <= s.y && s.y <= vmax.  The bounds are the min / max of the three vertices by < / >: each starts at
 *                  a's coordinate, then takes b's, then c's where that is smaller (larger).
 *   Inside test    d = (b.x-a.x)*(c.y-a.y) - (b.y-a.y)*(c.x-a.x).  !(d != 0) covers nothing.
 *                  w1 = (s.x-a.x)*(c.y-a.y) - (s.y-a.y)*(c.x-a.x)
 *                  w2 = (b.x-a.x)*(s.y-a.y) - (b.y-a.y)*(s.x-a.x)
 *                  hu = w1/d; hv = w2/d; w0 = 1 - hu - hv
 *                  covered iff hu >= 0 && hv >= 0 && w0 >= 0.  Edges and vertices are inclusive.
 *   Owner          prim(t) is the lowest covering slot.  No slot gives RT_GUIDE_PRIM_NONE.
 *   Resolve        for an owned texel: bary = (hu, hv) of the owner, recomputed with the same lines.
 *                  pos[k] = v0[k] + hu*(v1[k]-v0[k]) + hv*(v2[k]-v0[k]), left to right.
 *                  nrm = unit(cross(v1-v0, v2-v0)), with renderMotion's cross and unit (three divisions).  The geometric normal is by winding and is not
 *                  turned.  An unowned texel gets zeros.
 *   Dilation       dilate in 0 .. RT_TEXEL_MAX_DILATE (16).  src_0(t) = t if owned, else -1.  Iteration i, for every t with src_{i-1}(t) == -1: scan
 *                  dy = -1,0,1 (outer) and dx = -1,0,1 (inner) inside the image.  Take the first q with src_{i-1}(q) != -1 and set src_i(t) = src_{i-1}(q).
 *                  If there is none, src_i(t) = -1.  Owned texels keep themselves.  The planes are ping-ponged, so the order of evaluation is free.
 * Known: two triangles that share a UV edge each evaluate that edge with their own rounding.  A texel centre within an ulp of the edge can be claimed by
 * neither.  Dilation fills it.
 * Both calls return the number of owned texels.  Every plane pointer may be NULL.  For rasterTexels not all may be NULL; for bakeTexels not all of acc / out /
 * rays.  Planes are caller-owned host arrays of W*H entries, row 0 first: prim and src one int32, bary 2 floats, pos and nrm 3 floats, acc and out
 * rtGatherWidth(mode) floats, rays one word.  src is the plane after `dilate` iterations.
 * bakeTexels.  Point k is the texel index t, whatever the compaction or chunking.  P = pos(t), N = nrm(t).  Everything else is gatherRadiance's definition
 * word for word: origin and direction, g = base_id + (uint32_t)((uint64_t)t * dirs_total + m), the reduction, M, and W = rtGatherWidth(mode).
 *   Bit promise    In RT_FP_PARITY the result at every owned texel is bit-identical to gatherRadiance over the W*H points (pos(t), nrm(t)) at entry t, with any
 *                  finite filler at unowned entries, in every mode.  RT_GATHER_VISIBILITY is bit-identical in both fp modes.  The radiance modes in RT_FP_FAST
 *                  are the same estimate with no bit promise, because the compacted batch puts other rays into a wave.
 *   Outputs        acc and rays: written at owned texels, 0 elsewhere.  acc is read at owned texels when first > 0.  Any split of dirs_total into calls equals
 *                  one call.  out(t) is the value of src(t), and zeros where src(t) == -1.
 * Only owned texels are traced.  The call is blocking and runs on the first in-process device.  It chunks the compact list by max(1, RT_RAY_CHUNK / dirs)
 * points.  It follows setRenderOptions, the scene edits and rebuildBvh; RT_PIXELS_WAVES caps its path waves as it caps gatherRadiance's.  It changes nothing
 * another call observes: what gatherRadiance leaves alone, and gatherRadiance's own buffers and rtLastGatherMs.  The device buffers are its own and are freed
 * where the query buffers are.  Per texel of the largest atlas seen: owner 4, src 4 (8 with dilate > 0), the work word of a workgroup of 256 texels, and
 * where asked for prim 4, bary 8, pos 12, nrm 12 (rasterTexels); for a bake rank 4 and where asked for acc 4W, out 4W, rays 4.  Per owned texel of a bake:
 * list 4, pos 12, nrm 12, and where asked for acc 4W, out 4W, rays 4.  Per ray of the largest chunk: gatherRadiance's 44 bytes in the radiance modes, 29 in
 * VISIBILITY.  One word, the list's length, is read back between the raster and the bake.
 * rtRasterTexelsHost (rt_host.h) is the raster's CPU twin; rtAtlasGrid there gives a mesh without unique UVs a trivial atlas.
 * Misuse (rt error, exit 99), checked on the host before any device work: before init (rtLastTexelsMs and rtLastBakeMs as well), a sphere scene, W or H
 * outside 1 .. RT_TEXEL_MAX_SIZE, dilate outside 0 .. RT_TEXEL_MAX_DILATE, all planes NULL (bakeTexels: acc, out and rays), and for bakeTexels everything
 * gatherRadiance refuses for the same arguments. */
#define RT_TEXEL_MAX_SIZE 8192
#define RT_TEXEL_MAX_DILATE 16
int    rasterTexels(int W, int H, int dilate, int32_t* prim, int32_t* src, float* bary, float* pos, float* nrm);
int    bakeTexels(int W, int H, int dilate, int mode, int first, int dirs, int dirs_total, int ns, uint32_t base_id,
                  float bias, float max_dist, float* acc, float* out, uint32_t* rays, int32_t* prim, int32_t* src);
double rtLastTexelsMs(void);   /* raster + resolve + dilate + compact kernels of the last rasterTexels / bakeTexels */
double rtLastBakeMs(void);     /* generator + trace + reduce + scatter of the last bakeTexels, summed over chunks */

/* --- filtering texels: an edge-aware, chart-aware denoise of baked texel planes, on the device ----------------------------------------------------
 * filterTexels is the last stage of a bake: an a-trous filter (denoiseFrame's skeleton: 25 taps, stride 2^it, compact max(1 - x, 0)^2 weights) over the texel
 * planes bakeTexels writes, steered by what the raster knows of every texel - position, geometric normal and the world length of a texel step - instead of a
 * camera's guide planes.  Neighbours on the atlas grid are not neighbours on a surface: charts metres apart lie side by side, so a tap is accepted only within
 * reach (below).  Mesh scenes only.  All arithmetic is fp32, in both fp modes: every operation is rounded on its own (no FMA), operands are in the order
 * written, / and sqrt are correctly rounded, a comparison with a NaN is false, max(x, 0) = x > 0 ? x : 0, dot is evaluated left to right.
 * Planes      C = rtGatherWidth(mode) floats per texel (1, 3 or 27), t = y*W + x, row 0 first: exactly bakeTexels' out planes.  A caller with an RGB plane of
 *             their own passes RT_GATHER_IRRADIANCE.
 * Raster      rasterTexels' definition word for word, over the live slots, recomputed by the call: owned(t), the owner slot, P(t) = pos(t), n(t) = nrm(t) (the
 *             geometric normal by winding, not turned) and src(t) after `dilate` iterations.
 * Footprint   of an owned texel p, whose owner has UV vertices a, b, c, world vertices v0, v1, v2 and the raster's d;  e1 = v1 - v0, e2 = v2 - v0:
 *                 ux = (c.y-a.y)/d;  vx = (a.y-b.y)/d;  uy = (a.x-c.x)/d;  vy = (b.x-a.x)/d
 *                 Gx[k] = (ux*e1[k] + vx*e2[k]) / (float)W        Gy[k] = (uy*e1[k] + vy*e2[k]) / (float)H
 *                 f2 = 0.5f * (dot(Gx,Gx) + dot(Gy,Gy))           (the squared world length of one texel step)
 *                 r2(p) = (sigma_d*sigma_d) * f2                   rz(p) = 1 / (sigma_z * sqrt(f2))
 * Iteration   it = 0 .. iterations-1:  s = 1 << it;  K = {0.375, 0.25, 0.0625};  with sigma_c > 0: sc = sigma_c * 2^-it, rc = 1/(sc*sc);  c_0 = in.
 *             For every owned p = (x, y):
 *                 sum[0..C-1] = 0; wsum = 0
 *                 for dy = -2..2 (outer), dx = -2..2 (inner):
 *                     q = (x + dx*s, y + dy*s);  h = K[|dx|] * K[|dy|]
 *                     dx == 0 && dy == 0:  w = h
 *                     else the tap ADDS NOTHING (dropped, not weighted by zero) unless all hold:
 *                             q inside the atlas;  owned(q);
 *                             e = P(q) - P(p);  d2 = dot(e,e);  d2 <= r2(p) * (float)((dx*dx + dy*dy) * s * s)     (the reach test)
 *                         dn = dot(n(p), n(q));  wn = max(dn, 0);  normal_squarings times: wn = wn*wn
 *                         pd = abs(dot(n(p), e));  wz = max(1 - pd * rz(p), 0);  wz = wz*wz
 *                         w = h * wn * wz                                                      (left to right)
 *                         if sigma_c > 0:  L = min(C, 3);  dc[j] = c(p)[j] - c(q)[j], j < L;  dd = sum of dc[j]*dc[j] left to right;
 *                                          wc = max(1 - dd * rc, 0);  wc = wc*wc;  w = w * wc
 *                     sum[j] += w * c(q)[j] for every j < C;  wsum += w
 *                 c'(p)[j] = sum[j] / wsum                                                     (wsum >= 9/64: the centre tap)
 *             The colour weight looks at the leading min(C, 3) floats - the RGB of IRRADIANCE, the DC coefficient's RGB of SH9, the scalar of VISIBILITY -
 *             and every channel is filtered with that one weight.  The reach test is what makes the filter chart-aware: a tap k texels away is accepted
 *             only within sigma_d times the world distance k texels span at p, so two charts packed side by side fail it even where they are coplanar with
 *             equal normals.  A degenerate footprint (f2 of 0, inf or NaN: a triangle without world or UV extent, or an overflow) is handled by the rules
 *             above without a special case: f2 = NaN fails every reach test, f2 = 0 passes only taps at P(p) itself and gives them the plane weight 0
 *             (1 - 0 * inf is a NaN), f2 = inf passes every tap whose d2 is no NaN, with the plane weight 1 where pd is finite.  The centre tap always counts.
 * Output      out(t)[j] = c_final(src(t))[j], and zeros where src(t) == -1: bakeTexels' rule for out, so the chart borders are re-dilated from the filtered
 *             values.  `in` is read at owned texels only: whatever it holds elsewhere (the old dilation, NaNs) has no influence.  Non-finite values at
 *             owned texels are not treated specially: a NaN or an inf spreads to every texel that accepts it as a tap with a weight that is not 0 (inf * 0
 *             is a NaN too: with a weight of exactly 0), by up to 2 * (2^iterations - 1) texels per axis, as in denoiseFrame.  Returns the owned texels.
 * in          any host memory of W*H*C floats, or NULL: the out plane of the last bakeTexels call, where it lies on the device - nothing is uploaded (the
 *             pattern of RT_DISPLAY_FROM_PREVIEW).  That call must have asked for out, with this W, H and a mode of this width; a bakeTexels without out
 *             leaves nothing to take, and so does everything that frees the texel buffers (cleanupRenderer, setRenderOptions with another device list).
 *             A NULL in is taken as it is, even if the scene was edited after the bake: the raster is the live one.  out is caller-owned, never NULL, and
 *             may be in.
 * The call is blocking and runs on the first in-process device.  It follows the scene edits and rebuildBvh.  It changes nothing another call observes:
 * rtLastTexelsMs, rtLastBakeMs, rtLastGatherMs, the buffers of rasterTexels / bakeTexels / gatherRadiance and everything those calls leave alone stay as they
 * were: buffers, events and the raster are its own, freed where the query buffers are.  Per texel of the largest atlas seen: owner 4, src 4 (8 with dilate >
 * 0), the work word of a workgroup of 256 texels, two 16-byte records, the ping-pong pair of the values - 2 x 4 bytes for C = 1, 2 x 16 per three channels
 * otherwise (the fourth float of a record is unused) -, out 4C and, unless in is NULL, in 4C.
 * Defaults (DESIGN.md 3.32 has the measurement that chose them): iterations 3, normal_squarings 5, sigma_d 2.0f, sigma_z 2.0f, sigma_c 0.5f - sigma_c is in
 * the units of the values and the caller's to follow, roughly 2 / sqrt(dirs * ns) (0.5 is that of 16 directions, one sample); <= 0 switches the colour
 * weight off.
 * rtFilterTexelsHost (rt_host.h) is the CPU twin.
 * Misuse (rt error, exit 99), checked on the host before any device work: before init (rtLastFilterMs as well), a sphere scene, what rasterTexels refuses for
 * W, H and dilate, an unknown mode, out NULL, iterations outside 1 .. RT_DENOISE_MAX_ITERATIONS, normal_squarings outside 0 .. RT_DENOISE_MAX_SQUARINGS,
 * sigma_d or sigma_z not finite or <= 0, sigma_c not finite, in NULL without a recorded bake plane or with one of another W, H or width. */
#define RT_FILTER_ITERATIONS 3
#define RT_FILTER_SQUARINGS  5
#define RT_FILTER_SIGMA_D    2.0f
#define RT_FILTER_SIGMA_Z    2.0f
#define RT_FILTER_SIGMA_C    0.5f
int    filterTexels(int W, int H, int dilate, int mode, const float* in, float* out,
                    int iterations, int normal_squarings, float sigma_d, float sigma_z, float sigma_c);
double rtLastFilterMs(void);   /* raster + prologue + iterations + scatter kernels of the last filterTexels (not the copies); 0 before the first */

/* --- sampling texels: the planes of a bake looked up at hits, and the frame lit by them ------------------------------------------------------------
 * sampleTexels reads texel planes - bakeTexels' or filterTexels' out, or the caller's own - back onto the surface: at each hit of a list, the atlas point
 * of the hit, the texel (nearest) or the four texels around it (bilinear), and the value the mode stores.  renderLightmap is the frame built on it: one
 * centre ray and one first-hit traversal per pixel, the lookup, the albedo and the sky on the device; only the frame comes back.  Mesh scenes only.  All
 * arithmetic is fp32, in both fp modes: every operation is rounded on its own (no FMA), operands are in the order written, a comparison with a NaN is false.
 * Hit k       p = prim[k] with RT_RAY_PRIM's meaning: a slot of the live leaf-ordered triangle array;  (hu, hv) = uv[2k..] as RT_RAY_UV;  nrm = normal[3k..]
 *             as RT_RAY_NORMAL, read in RT_GATHER_SH9 only (NULL otherwise is fine).
 * Valid       iff 0 <= p < numTris and the slot's v[0].x is not +-inf.  An invalid hit (a miss, the floor, a prim past the array, a sentinel slot) writes
 *             out = (0, 0, 0) and valid = 0.  sampleTexels returns the number of valid hits.
 * Atlas point w0 = 1 - hu - hv;  tcu = hu*tc[2] + hv*tc[4] + w0*tc[0];  tcv = hu*tc[3] + hv*tc[5] + w0*tc[1]   (tc = the slot's texCoords: mesh_texel's two
 *             lines).  Not wrapped: the raster does not wrap either.
 * Nearest     (RT_SAMPLE_BILINEAR not set)  fx = tcu * (float)W;  fx = fx > 0 ? fx : 0   (a NaN gives 0);  fx = fx < (float)(W-1) ? fx : (float)(W-1);
 *             x = (int)fx;  y likewise from tcv and H;  c[j] = planes[(y*W + x)*C + j], C = rtGatherWidth(mode).
 * Bilinear    fx = tcu*(float)W - 0.5f;  fx = fx > -1 ? fx : -1   (a NaN gives -1);  fx = fx < (float)W ? fx : (float)W;  x0f = floorf(fx);  ax = fx - x0f;
 *             x0 = clamp((int)x0f, 0, W-1);  x1 = clamp((int)x0f + 1, 0, W-1);  y likewise: ay, y0, y1.  For every j < C, left to right:
 *                 c[j] = ((1-ax)*(1-ay))*c00[j] + (ax*(1-ay))*c10[j] + ((1-ax)*ay)*c01[j] + (ax*ay)*c11[j]        (cXY = the texel (xX, yY))
 *             The planes are read as they are: clamp to edge, no owner test.  Limit: across a chart border a tap reads whatever the plane holds there -
 *             the zeros of an unowned texel, or the neighbouring chart - unless the bake or filter that made the plane dilated it (dilate >= 1 covers the
 *             one texel a bilinear tap reaches).  A non-finite plane value reaches every hit that taps it (0 * inf is a NaN).
 * Value       3 floats.  RT_GATHER_IRRADIANCE: e = c.  RT_GATHER_VISIBILITY: e = (c0, c0, c0).  RT_GATHER_SH9: (X, Y, Z) = nrm, coefficient i of channel ch
 *             at c[3i + ch], left to right:
 *                 e[ch] = 0.282095f*c0 + 0.325735f*(c1*Y) + 0.325735f*(c2*Z) + 0.325735f*(c3*X)
 *                       + 0.273137f*(c4*(X*Y)) + 0.273137f*(c5*(Y*Z)) + 0.078848f*(c6*(3.0f*(Z*Z) - 1.0f))
 *                       + 0.273137f*(c7*(X*Z)) + 0.136568f*(c8*(X*X - Y*Y))
 *             then e[ch] = e[ch] > 0 ? e[ch] : 0.  These literals are the definition: gatherRadiance's basis constants times the cosine-lobe factors 1, 2/3
 *             and 1/4, so the SH9 value is "irradiance / pi at normal nrm", the quantity RT_GATHER_IRRADIANCE stores.  SH9 follows the turned shading normal
 *             the caller passes, so it serves both sides of a triangle; IRRADIANCE and VISIBILITY planes hold what the bake gathered on the winding side,
 *             whichever side the ray meets.
 * planes      host memory of W*H*C floats, row 0 first, or NULL with exactly one of RT_TEXELS_FROM_BAKE - the out plane of the last bakeTexels - and
 *             RT_TEXELS_FROM_FILTER - the out of the last filterTexels -, read where it lies on the device: filterTexels' in = NULL rules (the recorded W, H
 *             and width must match; a bake without out, and everything that frees the buffers, leaves nothing to take).  Either flag with planes given is
 *             misuse.
 * renderLightmap.  For every pixel (i, j) of the whole nx x ny image, whatever the row partition (as traceRays ignores it), the ray is renderGuides' centre
 * ray and its first hit exactly what traceRays returns for the ray rtCentreRays gives: tmin = rt_render_options.t_min, tmax = FLT_MAX, the floor with
 * rt_render_options.floor.  Triangle hit: L = e of the lookup with the pixel's prim, uv and normal.  Floor hit: L = floor_value (the plane is not in the
 * atlas; NULL = (1, 1, 1)).  Miss: out = RT_GUIDE_ALBEDO's miss value, the sky colour of the direction.  With RT_LIGHTMAP_ALBEDO a hit stores out[ch] = A[ch]
 * * L[ch], A = RT_GUIDE_ALBEDO's value of the pixel; without it out = L.  out is a caller-owned nx*ny frame, row 0 at the bottom: what denoiseFrame and
 * displayFrame take.
 *   Bit promise    out is bit-identical to the composition of renderGuides' ALBEDO plane, traceRays' PRIM, UV and NORMAL planes over rtCentreRays and the
 *                  lookup above.
 * Both calls are blocking and run on the first in-process device, RT_RAY_CHUNK hits (pixels) at a time.  They follow updateTriangles and rebuildBvh.  They
 * change nothing another call observes: buffers, events and timing slots are their own, freed where the query buffers are.  Per hit of the largest chunk:
 * 37 bytes (prim 4, uv 8, normal 12, out 12, valid 1); per pixel of the largest chunk: 64 (org 12, dir 12, t 4, prim 4, normal 12, uv 8, out 12); and the
 * planes, 4C bytes per texel, unless they are read where they lie.  n == 0 returns 0 at once.
 * rtSampleTexelsHost (rt_host.h) is the lookup's CPU twin.
 * Misuse (rt error, exit 99), checked on the host before any device work: before init (rtLastSampleMs and rtLastLightmapMs as well), a sphere scene, n < 0,
 * prim, uv or out NULL with n > 0, normal NULL in RT_GATHER_SH9, W or H outside 1 .. RT_TEXEL_MAX_SIZE, an unknown mode, unknown flag bits,
 * RT_LIGHTMAP_ALBEDO passed to sampleTexels, and the NULL / FROM rules above. */
enum { RT_SAMPLE_BILINEAR = 1, RT_LIGHTMAP_ALBEDO = 2, RT_TEXELS_FROM_BAKE = 4, RT_TEXELS_FROM_FILTER = 8 };
int    sampleTexels(int n, const int32_t* prim, const float* uv, const float* normal, int W, int H, int mode,
                    const float* planes, int flags, float* out, uint8_t* valid);
void   renderLightmap(int W, int H, int mode, const float* planes, int flags, const float floor_value[3], rt_vec3* out);
double rtLastSampleMs(void);     /* lookup kernels of the last sampleTexels, summed over chunks; 0 before the first */
double rtLastLightmapMs(void);   /* ray generator + trace + shade kernels of the last renderLightmap, summed over chunks; 0 before the first */

/* --- adaptive sampling: the samples go where the image is still noisy ---------------------------------------------------------------
 * refineFrame renders an adaptive frame: every pixel gets samples in batches until an estimate of its own error says it has enough.  The frame's state, the
 * selection, the list of a pass and the statistics live on the device; the pixel kernels of renderPixels trace the samples.  One call is one pass: select,
 * trace `batch` more samples for every selected pixel, update their statistics, deliver.  It returns the number of pixels it sampled; 0 means the frame is
 * finished under the call's parameters - nothing was traced, the planes are still delivered.  The caller's loop is  while (refineFrame(...)) {}  with
 * previewFrame / displayFrame in it as often as it likes.
 * All arithmetic is fp32, every operation rounded on its own (no FMA), operands in the order written, a comparison with a NaN false; lum is previewFrame's;
 * max(x, 0) = x < 0 ? 0 : x, so a NaN stays a NaN.  Counts are integers and enter as (float)count.  So every stored number is defined bit for bit
 * (tests/refine_reference.py restates this in numpy).
 * Per-pixel state:  sum(p) and the stream word (renderPixels' state), n(p) samples so far, M1(p), M2(p), l(p) = lum(mean(p)), rays(p) = the closest-hit
 *     queries of p's last batch.  After a reset n = 0, M1 = M2 = 0, rays = 0.
 * Update of a sampled pixel:  the pixel kernel continues p's stream by `batch` samples (renderPixels with first = n(p)).  n' = n + batch;
 *     mean(p)[k] = sum[k] / (float)n';  l' = lum(mean);  K = n' / batch
 *     y = l'  if n == 0,  else  y = (l' * (float)n' - l * (float)n) / (float)batch         (the luminance of the batch's own mean, recovered from the two means)
 *     M1 += y;  M2 += y*y
 * Error of a pixel, K = n / batch:
 *     K < 2:  err = FLT_MAX
 *     else:   a1 = M1 / (float)K;  a2 = M2 / (float)K;  v = max(a2 - a1*a1, 0) / (float)(K - 1);  r = max(l, 0) + RT_REFINE_LUM_EPS;  err = v / (r*r)
 *     (the relative variance of the mean, from the batch means)
 * Select, with the call's parameters:
 *     unconverged(p) = K(p) < min_batches || !(err(p) <= threshold*threshold)
 *     want(p) = unconverged(p);  with RT_REFINE_DILATE: some q of the 3 x 3 window around p, clipped to the image, is unconverged - one pixel's lucky early
 *               estimate must not leave a hole next to noise
 *     active(p) = want(p) && n(p) + batch <= max_samples
 *     So the first pass after a reset samples every pixel, and a pixel whose mean is not finite (err is a NaN) never converges and stops at max_samples.
 * List order:  cls(p) = 31 - clz(max(rays(p), 1)).  The pass hands the active pixels to the pixel kernel with cls descending - dearest first, so the long
 *     pixels do not start last; the order inside a class is unspecified, and no result depends on the order.
 * Outputs: three caller-owned host planes of nx*ny entries, row 0 = bottom, each may be NULL (with all three NULL nothing is downloaded): out = mean(p),
 * samples = n(p), error = err(p).  In RT_FP_PARITY out(p) is bit-identical to the pixel runRenderer(samples(p)) stores at p, and samples, error and the
 * return value are the same after any sequence of calls wherever the library runs; in RT_FP_FAST the same procedure runs on the FAST pixel kernels with no
 * bit promise, as for renderPixels.  threshold, min_batches, max_samples and flags act at selection only and may change from call to call (a max_samples
 * raised after a 0 return continues the frame); batch is fixed by the first call after a reset.
 * The frame is reset - the next call starts at sample 0 - by every init*, cleanupRenderer, every setRenderOptions, setCamera, every scene edit and rebuildBvh,
 * and rtResetRefine.  The call is blocking, works on the WHOLE image on the first in-process device whatever the partition is, and changes nothing another
 * call observes: the framebuffer, getRenderStats, rtLastLaunches, rtLastSphereForm, the progressive frame, the cost maps, every history, rtLastPixelsMs and
 * every other rtLast*Ms stay as they were.  Device memory: 42 bytes per pixel of state and list, 12 and 4 more for the out and error planes once asked for,
 * and 32 bytes per entry of one chunk of the list - lists above RT_PIXEL_CHUNK entries run in chunks -; allocated by the first call, freed where the pixel
 * buffers are.  Of a pass one word is read back before the pixel kernel is launched: the length of its list.
 * Misuse (rt error, exit 99), checked before any device work: any of the five calls before init, batch < 1, min_batches < 2, max_samples < batch or above
 * RT_PROGRESSIVE_MAX_SAMPLES, threshold not finite or < 0, unknown flag bits, a batch different from the frame's, and every frame condition renderPixels
 * refuses: RT_RNG_COUNTER, variant != 0, rt_render_options.floor = 1 or nee = 1 on a sphere scene. */
enum { RT_REFINE_DILATE = 1 };
#define RT_REFINE_LUM_EPS 1e-3f
int    refineFrame(rt_vec3* out, int32_t* samples, float* error, int batch, int min_batches, int max_samples, float threshold, int flags);
void   rtResetRefine(void);                    /* the next refineFrame starts at sample 0 */
long long rtRefineSamples(void);               /* samples traced since the last reset, all pixels */
int    rtRefineLastList(int32_t* ij, int cap); /* the list of the last call's pass, in the order it was handed to the kernel: min(cap, length) (i, j) pairs; returns its length */
double rtLastRefineMs(void);                   /* HIP-event time of select + pixel kernel + update of the last call, not the deliver kernel or the copies; 0 before the first */

/* --- editing the scene: move, recolour, animate without a new init ---------------------------------------------------------------
 * The calls below change the scene the renderer holds, in place, on every in-process device: a picked object (traceRays) is moved or recoloured, an
 * animation is played, without cleanupRenderer + init*.  The contract they share: after ANY sequence of them everything the library computes - runRenderer
 * in both fp modes, runRendererProgressive, renderGuides, traceRays / occludedRays, the preview passes, the counters = 1 statistics, node visits included -
 * is bit-identical to cleanupRenderer + init* with the edited scene followed by the same setRenderOptions and setCamera.  For a mesh the edited scene is the
 * edited triangles with the REFITTED tree: the tree's shape and the triangles' slots stay, every box is recomputed.  The refit, stated once:
 *   first_leaf = numBvhNodes / 2;  lo = min'(lo, p) means p < lo ? p : lo;  hi = max'(hi, p) means p > hi ? p : hi  (a NaN never wins; of two zeros of
 *   different sign the one met first stays, which the order below decides)
 *   Leaf L in [first_leaf, 2 * first_leaf):  lo = (+inf, +inf, +inf), hi = (-inf, -inf, -inf); for the slots k = 0 .. nppl-1 of tris[(L - first_leaf) * nppl + k]
 *     in order, stopping at the first sentinel (v[0].x is +-inf, as the traversal's leaf loop stops): for the vertices 0, 1, 2 and within a vertex the axes
 *     x, y, z:  lo[axis] = min'(lo[axis], p),  hi[axis] = max'(hi[axis], p).  An empty leaf keeps (+inf, -inf).
 *   Internal node i in [1, first_leaf), children L = 2i and R = 2i + 1, per axis:  lo = lo_R < lo_L ? lo_R : lo_L;  hi = hi_R > hi_L ? hi_R : hi_L.
 *   Node 0 is never read or written.  The scene bounds become node 1's box.
 * Only comparisons: the refitted tree is defined bit for bit.  rtRefitBvh / rtRefitBvhArrays (rt_host.h) compute it on the CPU, so "edit the triangles of a
 * host mesh, refit it" is the scene the CPU oracle renders, and in PARITY mode the device's frame equals the oracle's.  The device computes it in two to four
 * kernel launches whatever the size of the edit; the tree is always refitted as a whole.  A refit keeps every triangle in its slot: after
 * large moves the boxes overlap and rays visit more nodes - rebuildBvh (below) assigns the triangles to the leaves anew.
 *
 * updateTriangles  mesh scenes.  Replaces slots [first, first + count) of the leaf-ordered triangle array passed to initRenderer (count * 64 bytes cross the
 *                  bus) and refits on every in-process device.  Blocking.  count == 0 returns at once and changes nothing.  The caller owes finite vertices:
 *                  a NaN coordinate is ignored by the boxes and only that triangle's hits are unspecified.
 * updateMaterials  mesh scenes.  Replaces the material array (n = the numMaterials of init); the textures stay.
 * updateSpheres    sphere scenes.  Replaces spheres and materials (n = the n of init); the renderer's grouping of the spheres is rebuilt on the host.
 * getMeshBvh       mesh scenes.  The first device's current nodes: writes min(cap, numBvhNodes) nodes (nodes may be NULL when cap <= 0) and, unless bounds is NULL,
 *                  the scene bounds; returns numBvhNodes.
 * An edit resets the progressive frame, as setCamera does, and retires the cost maps of sphere frames.  It does NOT touch the framebuffer, getRenderStats,
 * rtLastLaunches, the histories of accumulateFrame / previewFrame (see there), displayFrame's adapted exposure and the other rtLast*Ms values.  A later
 * setRenderOptions that changes the device layout re-uploads the EDITED scene.
 * Misuse (rt error, exit 99): any of the five before init; updateTriangles / updateMaterials / getMeshBvh on a sphere scene, updateSpheres on a mesh scene;
 * first < 0, count < 0, first + count > numTris, a NULL pointer with count > 0 (updateMaterials, updateSpheres: any NULL pointer); a slot whose sentinel state
 * would change - isinf(v[0].x) must be the same before and after; a real triangle's meshID >= numMaterials; n different from init's; a material texId
 * (updateMaterials) or type (updateSpheres) that init* would refuse; updateTriangles on a tree whose number of leaves is not a power of two (every tree of
 * rtBuildBvh* is one). */
void   updateTriangles(int first, int count, const rt_triangle* tris);
void   updateMaterials(const rt_material* materials, int n);
void   updateSpheres(const rt_sphere* spheres, const rt_material* materials, int n);
int    getMeshBvh(rt_bvh_node* nodes, int cap, rt_bbox* bounds);
double rtLastUpdateMs(void);   /* HIP-event time of the refit kernels of the last updateTriangles (not the copies), the largest over the in-process devices; 0 before the first */

/* rebuildBvh       mesh scenes.  Re-splits the tree on every in-process device: the shape stays (numBvhNodes, first_leaf = numBvhNodes / 2, nppl, numTris),
 *                  the triangles are assigned to leaf slots anew, then the tree is refitted.  Blocking.  It is an edit: the contract above holds for any
 *                  sequence of edits and rebuilds - the rebuilt scene is the one rtRebuildBvh / rtRebuildBvhArrays (rt_host.h) compute on the CPU, bit for
 *                  bit, getMeshBvh and rtLastLaunches included - and what an edit resets or leaves alone is reset or left alone.  The rebuild, stated once:
 *   Input: the triangles the traversal can see - leaves 0 .. first_leaf-1 in order, within a leaf the slots k = 0 .. nppl-1 up to the first sentinel
 *     (isinf(v[0].x)) - are triangles i = 0 .. n-1 in that order.  A real triangle behind a sentinel is invisible to every ray; it is dropped (its slot
 *     becomes a sentinel).  Slots at or beyond first_leaf * nppl are not touched.
 *   Per triangle: box = min / max over the three vertices; cent[a] = 0.5f * (lo[a] + hi[a]) (one rounded add, one rounded multiply);
 *     area(box) = hi[0] < lo[0] ? 0 : 2.0f * (dx*dy + dy*dz + dz*dx) with d = hi - lo, every operation rounded on its own, operands in that order, no FMA.
 *     Boxes enter only through area and cent; an area does not depend on the sign of a zero and centroids are compared as numbers (-0 == +0), so the order
 *     in which a box is accumulated is free.
 *   Node idx with `leaves` leaf slots below it and the triangle set S, m = |S| (the root: all n, leaves = first_leaf):  capHalf = (leaves / 2) * nppl;
 *     lo = max(m - capHalf, m > 1 ? 1 : 0);  hi = min(capHalf, m > 1 ? m - 1 : m).  For axis 0, 1, 2 order S by (cent[axis], i);
 *     cost(axis, cut) = area(first cut) * (float)cut + area(the rest) * (float)(m - cut), the area of an empty rest being 0.0f.  The winner is the first
 *     (axis, cut), axis-major with cut ascending over [max(lo, 1), hi], whose cost is strictly below every earlier one and below +inf; a NaN cost never
 *     wins; without a winner axis 0 and cut (m + 1) / 2.  nl = min(max(cut, lo), hi); with m == 0, nl = 0.  The left child gets the first nl triangles
 *     of the winning axis's order, the right child the rest.
 *   Leaf L holds its triangles in the order of its parent's winning axis in slots 0 .., sentinels (all nine coordinates +inf, everything else zero) follow.
 *   Nodes 1 .. and the scene bounds: the refit (above) of the new slots.
 *                  old_slot, unless NULL, receives numTris entries: the slot the triangle now in slot s came from, -1 for a sentinel, s itself at or
 *                  beyond first_leaf * nppl.  The caller owes finite vertices, as for updateTriangles.  Adding or removing triangles stays a new init.
 *                  The device builds level by level; RT_REBUILD_TILE is the number of elements one workgroup of its scans covers.
 * Misuse (rt error, exit 99): either call before init; rebuildBvh on a sphere scene, on a tree whose number of leaves is not a power of two, or with more
 * than RT_REBUILD_MAX_TRIS visible triangles. */
#define RT_REBUILD_MAX_TRIS (1 << 24)
#define RT_REBUILD_TILE 256
void   rebuildBvh(int32_t* old_slot);
double rtLastRebuildMs(void);  /* HIP-event time of the build + refit kernels of the last rebuildBvh, the largest over the in-process devices; 0 before the first */

/* --- the marked pose: temporal passes that follow moving geometry, and the motion planes ---------------------------------------------
 * accumulateFrame and previewFrame reproject a pixel through its CURRENT hit point.  When an edit moves geometry between two frames that point is not where
 * the surface was when the history was stored: the taps are rejected, or - a small move - taken from the wrong surface point.  rtMarkPose remembers the
 * scene's geometry as it is now, "the previous frame's pose"; from then on both passes reproject every pixel through the point Pm its surface point had in
 * the marked pose and test their taps against (Pm, nm), so a moved object keeps its history.  The loop of an animated frame is rtMarkPose, updateTriangles /
 * updateSpheres (and rebuildBvh), setCamera, runRenderer(1), previewFrame, displayFrame.  renderMotion returns the planes themselves - for
 * a caller's own TAA, motion blur or a video encoder.  Without an rtMarkPose call nothing the library computes changes: no new kernel is launched, no new
 * buffer is allocated, and the passes run the kernels they ran before.
 * All arithmetic is fp32, every operation rounded on its own (no FMA), operands in the order written, dot evaluated left to right, a comparison with a NaN
 * false; cross(a, b) = (a.y*b.z - a.z*b.y, -(a.x*b.z - a.z*b.x), a.x*b.y - a.y*b.x); unit(a) = a / sqrt(a.x*a.x + a.y*a.y + a.z*a.z), three divisions.  So
 * the planes are defined bit for bit (tests/motion_reference.py restates this in numpy).  valid(p), t(p), n(p), prim(p) and P(p) = o + t*d
 * are accumulateFrame's own.  Per pixel p:
 *     !valid(p):                                       Pm = (0,0,0);  nm = (0,0,0)
 *     the floor;  no pose marked;  the marked slot is a sentinel (isinf(a0.x)):      Pm = P;  nm = n
 *     triangle slot s = prim(p), live vertices v0..v2, marked vertices a0..a2:
 *         all nine marked coordinates equal the live ones bit for bit:               Pm = P;  nm = n      (what did not move behaves exactly as before)
 *         otherwise:
 *             e1 = v1 - v0;  e2 = v2 - v0;  w = P - v0
 *             d11 = dot(e1,e1);  d12 = dot(e1,e2);  d22 = dot(e2,e2);  d1w = dot(e1,w);  d2w = dot(e2,w)
 *             den = d11*d22 - d12*d12;  bu = (d22*d1w - d12*d2w) / den;  bv = (d11*d2w - d12*d1w) / den
 *             Pm[k] = a0[k] + bu*(a1[k] - a0[k]) + bv*(a2[k] - a0[k])                 (left to right)
 *             gm = unit(cross(a1 - a0, a2 - a0));  nm = dot(cross(e1, e2), n(p)) < 0 ? -gm : gm        (the turn hit() gave the live normal)
 *         A degenerate live or marked triangle gives NaN planes: every comparison of the passes is then false and the pixel starts anew.
 *     sphere s = prim(p), live (c, r), marked (c', r'):
 *         the four words equal bit for bit:  Pm = P;  nm = n;      otherwise:  Pm[k] = c'[k] + ((P[k] - c[k]) / r) * r';  nm = n(p)
 *     screen, with C' = *prev_cam or, with prev_cam NULL, the current camera:  accumulateFrame's r, x, y computed from e = Pm - o' (the constants Lu .. Vl of
 *         C' as there);  screen(p) = (x - (float)i, y - (float)j) if valid(p) && r > 0, else (0, 0): where the previous camera saw the surface point, relative
 *         to the pixel, in pixels.
 * With a pose marked accumulateFrame and stage T of previewFrame take Pm(p), nm(p) in the place of P(p), n(p) in exactly three places: the reprojection
 * e = Pm - o', the tap's plane test abs(dot(nm, P'(q) - Pm)) * rz(p) < 1 and the tap's normal test dot(nm, n'(q)) >= normal_min.  Everything else is as it
 * was: rz(p) from t(p), the SAME_PRIM test, the blend, the records stored for the next call (the current P, n, prim, c, N, M1, M2), stages V and A.
 *
 * rtMarkPose     copies, on the first in-process device (where the passes run): mesh scenes - the leaf-ordered triangle slots, device to device, 64 bytes a
 *                slot; sphere scenes - the caller-order (center, radius) array, kept on the host and uploaded, 16 bytes a sphere.  A second call overwrites
 *                the mark.  The mark is dropped by every init*, cleanupRenderer, rtClearPose and a setRenderOptions that changes the device layout; setCamera,
 *                the update* calls, runRenderer* and every pass keep it, and any other setRenderOptions resets the histories as before and keeps it.
 *                rebuildBvh carries it along: slot s of the mark becomes the old mark of old_slot[s], a sentinel where old_slot[s] < 0 - one gather on the
 *                device - so "the previous pose of the triangle now in slot s" stays right.
 * renderMotion   fills the planes named in `mask`, caller-owned host arrays of nx*ny entries, row 0 = bottom: prev_pos = Pm (3 floats), prev_normal = nm
 *                (3 floats), screen (2 floats); nothing is written through a pointer whose plane is not named.  Blocking.  Like the passes it works on the
 *                WHOLE image on the first in-process device, whatever the partition is, follows setCamera, setRenderOptions and the edits, and changes
 *                nothing another call observes: the framebuffer, getRenderStats, rtLastLaunches, both histories, the progressive frame and every other
 *                rtLast*Ms stay as they were.
 * Device memory, from the first rtMarkPose or renderMotion on: the mark (twice for a mesh once a rebuild has carried it, and the live spheres beside the
 * marked ones), 32 bytes per pixel of motion planes shared by all passes, 8 more for `screen` once asked for, and renderMotion's guide planes (28 bytes per
 * pixel); freed where the passes' buffers are.  The motion kernel of a pass runs behind its guide kernel and, like that one, is not part of
 * rtLastAccumulateMs / rtLastPreviewMs.
 * Misuse (rt error, exit 99), checked before any device work: any of the six calls before init; mask 0 or with unknown bits; a named plane whose pointer
 * is NULL; rt_render_options.floor = 1 on a sphere scene. */
void   rtMarkPose(void);    /* remember the scene's geometry as it is now: "the previous frame's pose" */
void   rtClearPose(void);   /* forget it */
int    rtPoseMarked(void);  /* 0 / 1 */
enum { RT_MOTION_POS = 1, RT_MOTION_NORMAL = 2, RT_MOTION_SCREEN = 4 };
void   renderMotion(int mask, const rt_camera* prev_cam, float* prev_pos, float* prev_normal, float* screen);
double rtLastMotionMs(void); /* HIP-event time of the motion kernel of the last renderMotion alone (not its guide kernel, not the copies); 0 before the first */

enum { RT_KERNEL_SPHERE_QUEUE = 1, RT_KERNEL_SPHERE_TILES = 2, RT_KERNEL_MESH_QUEUE = 3, RT_KERNEL_MESH_TILES = 4 };
enum { RT_LAUNCH_FAMILY = 0, RT_LAUNCH_PHASE, RT_LAUNCH_CLS, RT_LAUNCH_CHUNKED, RT_LAUNCH_DBG, RT_LAUNCH_SCENE, RT_LAUNCH_LEAN,
       RT_LAUNCH_THREADS, RT_LAUNCH_BLOCKS, RT_LAUNCH_DEVICE, RT_LAUNCH_FP, RT_LAUNCH_WORDS };
int rtLastLaunches(int32_t* out, int cap);
/* The form of the cost-ordered sphere dispatch (the record with PHASE 2, CLS 2) of the last runRenderer or progressive pass.  That kernel exists in two forms
 * with the same template arguments and the same launch record: the general one, which decides the frame's switches at run time, and one compiled for the
 * default frame (a queue per XCD, packed parked records, no middle tier, the compact device framebuffer, no diagnostics), which the launcher takes whenever
 * the frame is that one.  Both render the same bits.  RT_SPHERE_FORM_NONE: the frame had no such dispatch.  Host-side bookkeeping only. */
enum { RT_SPHERE_FORM_NONE = -1, RT_SPHERE_FORM_GENERAL = 0, RT_SPHERE_FORM_DEFAULT = 1 };
int rtLastSphereForm(void);

#ifdef __cplusplus
}
#endif

#endif /* RT_API_H */
