/*
 * rt_host.h — C-ABI of librt_host.so: the host-side pieces that sit either side of the render
 * hot path in the reference's main.cpp / staircase_scene.h (camera construction, scene set-up,
 * BVH file + builder, PPM / .ref output, RMSE).  Plain C++ inside, no HIP, no torch: loads on a
 * machine without a GPU.
 *
 * Scene and camera are produced ONCE here and handed as data to every backend (HIP library,
 * CPU oracle), never recomputed per side.
 */
#ifndef RT_HOST_H
#define RT_HOST_H

#include "rt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* camera::camera, /root/reference/helper_structs.h:194-207 (runs on the host there too). */
void rtMakeCamera(const float lookfrom[3], const float lookat[3], const float vup[3], float vfov,
                  float aspect, float aperture, float focus_dist, rt_camera* out);

/* random_float, /root/reference/main.cpp:17-20: state = 214013*state + 2531011;
 * return ((state >> 16) & 0x7FFF) / 32767.f */
float rtRandomFloat(uint32_t* state);

/* C1: ground + glass + metal; camera lookfrom(0,0,1) lookat(0,0,-1) vfov 60
 * aperture 0 focus 2.  Writes 3 spheres / 3 materials; returns 3. */
int rtSceneThreeSpheres(rt_sphere* spheres, rt_material* materials, int cap, int nx, int ny, rt_camera* cam);

/* C2/C3/C5: the "Ray Tracing in One Weekend" cover scene as the README-era
 * renderer built it — ground, 22x22 grid of small spheres jittered by the main.cpp LCG
 * (seeded with `seed`, 0 for the benchmark), three big spheres: 488 spheres.  Camera
 * lookfrom(13,2,3) lookat(0,0,0) vfov 30 aperture 0.1 focus 10, aspect nx/ny.
 * Returns the number of spheres written (488), or -needed if cap is too small. */
int rtSceneRandomSpheres(uint32_t seed, rt_sphere* spheres, rt_material* materials, int cap,
                         int nx, int ny, rt_camera* cam);

/* setup_camera, /root/reference/staircase_scene.h:62-73. */
void rtStaircaseCamera(int nx, int ny, rt_camera* cam);

/* The centre rays of pixels ij[2k] = i (column), ij[2k+1] = j (row, 0 = bottom) of an nx x ny image, exactly as renderGuides defines them (rt_api.h):
 * u = ((float)i + 0.5f) / (float)nx, v = ((float)j + 0.5f) / (float)ny, org = cam.origin, dir = unit(lower_left_corner + u*horizontal + v*vertical - origin):
 * get_ray (camera.h:8-12) without the lens offset, bit for bit.  org and dir receive n x 3 floats: a cursor position becomes a pick ray or an autofocus ray
 * for traceRays without a GPU.  Pixels outside the image are computed like any other. */
void rtCentreRays(const rt_camera* cam, int nx, int ny, const int32_t* ij, int n, float* org, float* dir);

/* The camera that turns a frame's pixels into one ray: origin = o, lower_left_corner = target, every other field 0 (no extent, no lens).  Under it get_ray
 * (camera.h:8-12) returns origin o and direction target - o for every pixel and every jitter, because the jitter and the lens sample multiply zero vectors.
 * This is the equivalence radianceRays (rt_api.h) is defined by: for o and T without negative-zero coordinates and d = fl(T - o) per component, the ray
 * (o, d, id) of radianceRays at f + c samples is bit-identical to the pixel with global id `id` (= j*nx + i) that runRenderer(f + c) stores under
 * rtPinholeCamera(o, T) - whatever the image size, which only decides which ids exist.  A frame under this camera is a constant-direction image: useful as
 * the reference of a ray, not as a picture. */
void rtPinholeCamera(const float o[3], const float target[3], rt_camera* out);

/* ---- mesh scenes: BVH in the layout hitBvh expects (kernels.cu:154-224) ---- */

typedef struct rt_host_mesh rt_host_mesh;    /* opaque; owns tris + bvh */

/* Builds the complete-binary-tree BVH over `tris` (copied): heap-indexed nodes, root at index 1,
 * node 0 unused, leaves = power of two, nppl triangles per leaf padded with sentinel triangles
 * whose v[0].x is +inf (kernels.cu:202).  Returns NULL on bad arguments. */
rt_host_mesh* rtBuildBvh(const rt_triangle* tris, int num_tris, int nppl);
/* The same with `extra_levels` tree levels beyond the smallest complete tree that holds the triangles (rtBuildBvh: 1): more leaf
 * slots for the SAH cuts to use - fewer node visits and triangle tests per ray, twice the (small) arrays per level. */
rt_host_mesh* rtBuildBvhLevels(const rt_triangle* tris, int num_tris, int nppl, int extra_levels);

/* loadBVH, /root/reference/staircase_scene.h:75-101: file "BVH_00.04\0", int numTris,
 * triangle[numTris], int numBvhNodes, bvh_node[numBvhNodes], vec3 min, vec3 max, int nppl. */
rt_host_mesh* rtLoadBvhFile(const char* path);
int  rtSaveBvhFile(const rt_host_mesh* m, const char* path);        /* 0 on success */
void rtFreeMesh(rt_host_mesh* m);
/* Fills an rt_mesh view (pointers stay owned by m) and returns nppl. */
int  rtMeshView(const rt_host_mesh* m, rt_mesh* out);

/* The refit of rt_api.h ("editing the scene": the definition is stated there, once) on the CPU, in plain C++: every node 1 .. numBvhNodes-1 from the
 * triangles as they are now, bottom up, and *bounds (unless NULL) = node 1's box.  Node 0 is neither read nor written.  It is what updateTriangles computes
 * on the device, bit for bit: "edit the triangles in place, then refit" yields the scene the CPU oracle renders.  Returns 0, or -1 for arrays initRenderer
 * would refuse (a NULL pointer, numBvhNodes odd or below 4, nppl <= 0, (numBvhNodes / 2) * nppl > numTris, more than 2^30 leaves); nothing is written then. */
int rtRefitBvhArrays(const rt_triangle* tris, uint32_t numTris, rt_bvh_node* bvh, int numBvhNodes, int nppl, rt_bbox* bounds);
/* The same on an owned mesh: its nodes and bounds in place (views taken with rtMeshView before keep their pointers; take the bounds again). */
int rtRefitBvh(rt_host_mesh* m);

/* The rebuild of rt_api.h ("editing the scene": the definition is stated there, once) on the CPU, in place: the triangles the traversal can see, in slot order,
 * go through the builder of rtBuildBvhLevels with the tree's own leaf count (numBvhNodes / 2) and into the leaf slots it assigns; sentinels fill the rest of
 * slots 0 .. (numBvhNodes / 2) * nppl - 1, later slots are not touched; then the refit above.  It is what rebuildBvh computes on the device, bit for bit.
 * old_slot, unless NULL, receives numTris entries: the slot the triangle now in slot s came from, -1 for a sentinel, s itself at or beyond
 * (numBvhNodes / 2) * nppl.  Returns 0, or -1 for what rtRefitBvhArrays refuses or a leaf count that is not a power of two; nothing is written then. */
int rtRebuildBvhArrays(rt_triangle* tris, uint32_t numTris, rt_bvh_node* bvh, int numBvhNodes, int nppl, rt_bbox* bounds, int32_t* old_slot);
/* The same on an owned mesh (views taken with rtMeshView before keep their pointers; take the bounds again). */
int rtRebuildBvh(rt_host_mesh* m, int32_t* old_slot);

/* Procedural stand-in for the staircase asset (absent from the reference snapshot, SURVEY.md
 * §7.4 H6): a room with a flight of steps, a glass ball, a metal ball and boxes, sized to the
 * staircase camera and light of staircase_scene.h:62-73 / kernels.cu:93.  Writes up to cap
 * triangles and 20 materials (indices as staircase_scene.h:139-158, texId = -1 unless
 * with_textures); returns the triangle count (or -needed). `detail` >= 1 scales tessellation. */
int rtSceneStaircaseProcedural(int detail, rt_triangle* tris, int cap, rt_material* materials20);

/* ---- output / verification harness (main.cpp:25-60,105-128; staircase_scene.h:22-43) ---- */

uint32_t rtLinearToSRGB(float x);
/* P3 PPM, rows top to bottom (j = ny-1 .. 0). 0 on success. */
int rtWritePPM(const char* path, int nx, int ny, const rt_vec3* colors);
/* "REF_00.01\0", int nx, int ny, vec3[nx*ny]. 0 on success; load returns -1 missing/bad header, -2 size mismatch. */
int rtSaveReference(const char* path, int nx, int ny, const rt_vec3* colors);
int rtLoadReference(const char* path, rt_vec3* reference, int nx, int ny);
/* sqrt( sum_i sum_c (f-g)^2 / 3 / (nx*ny) ), accumulated in double. */
double rtRmse(const rt_vec3* f, const rt_vec3* g, int nx, int ny);

/* displayFrame's definition (rt_api.h: exposure, tone map, sRGB, dither, RGBA bytes; the RT_DISPLAY_* flags without RT_DISPLAY_FROM_PREVIEW, RT_TONEMAP_*) on
 * the CPU with libm's powf: the same bytes as the device call, for a host without a GPU.  in: nx*ny vec3, row 0 = bottom; out_rgba: nx*ny*4 bytes.  With
 * RT_DISPLAY_AUTO_EXPOSURE the state is the caller's: *E_state is E' on entry, a NaN meaning "adapt from nothing", and E on return (E_state NULL: adapt from
 * nothing, nothing kept); hist, unless NULL, receives the RT_DISPLAY_BINS bins.  Without the flag neither is touched.  Returns 0, or -1 for arguments
 * displayFrame would refuse (nothing is written then). */
int rtDisplayFrameHost(const rt_vec3* in, uint8_t* out_rgba, int nx, int ny, int flags, int tonemap, float exposure, float adapt, float* E_state,
                       uint32_t* hist);

/* The direction generator of gatherRadiance (rt_api.h, "gathering at points": the definition is stated there, once) on the CPU, in plain C++: what
 * rtGatherDirections downloads from the device, bit for bit - entry k*dirs + (m - first) of org (3 floats), dir (3 floats, raw D) and ids (g); each pointer
 * may be NULL.  No renderer state is read: for arguments rtGatherDirections would refuse (and for n == 0) nothing is written. */
void rtGatherDirectionsHost(int n, const float* pos, const float* nrm, int mode, int first, int dirs, int dirs_total,
                            uint32_t base_id, float bias, float* org, float* dir, uint32_t* ids);

/* The UV-atlas raster of rasterTexels / bakeTexels (rt_api.h, "baking texels": the definition is stated there, once) on the CPU, in plain C++, over the
 * caller's leaf-ordered triangle array (HostMesh tris, or what rtRebuildBvh left): what rasterTexels downloads from the device, bit for bit - prim and src one
 * int32 per texel, bary 2 floats, pos and nrm 3 floats, row 0 first; each pointer may be NULL, not all.  Returns the number of owned texels, or -1 for
 * arguments rasterTexels would refuse (nothing is written then).  No renderer state is read. */
int rtRasterTexelsHost(const rt_triangle* tris, uint32_t numTris, int W, int H, int dilate, int32_t* prim, int32_t* src, float* bary, float* pos, float* nrm);

/* filterTexels (rt_api.h, "filtering texels": the definition is stated there, once) on the CPU, in plain C++, on top of rtRasterTexelsHost over the caller's
 * leaf-ordered triangle array: what filterTexels downloads from the device, bit for bit - out, W*H*rtGatherWidth(mode) floats, row 0 first; it may be `in`.
 * Returns the number of owned texels, or -1 for arguments filterTexels would refuse and for in NULL - the twin has no bake to take a plane from - (nothing is
 * written then).  No renderer state is read. */
int rtFilterTexelsHost(const rt_triangle* tris, uint32_t numTris, int W, int H, int dilate, int mode, const float* in, float* out, int iterations,
                       int normal_squarings, float sigma_d, float sigma_z, float sigma_c);

/* sampleTexels (rt_api.h, "sampling texels": the definition is stated there, once) on the CPU, in plain C++, over the caller's leaf-ordered triangle array:
 * what sampleTexels downloads from the device, bit for bit - out, 3 floats per hit, and valid (may be NULL).  flags: RT_SAMPLE_BILINEAR or 0.  Returns the
 * number of valid hits, or -1 for arguments sampleTexels would refuse and for planes NULL - the twin has no bake or filter to take a plane from - (nothing is
 * written then).  No renderer state is read. */
int rtSampleTexelsHost(const rt_triangle* tris, uint32_t numTris, int n, const int32_t* prim, const float* uv, const float* normal, int W, int H, int mode,
                       const float* planes, int flags, float* out, uint8_t* valid);

/* A trivial non-overlapping atlas: overwrites texCoords of tris[0 .. n-1]; nothing else is touched (sentinel slots get coordinates too; the raster skips them).
 * fp32, every operation rounded on its own, operands in the order written:
 *   pairs = (n + 1) / 2;  cells = the smallest integer with cells * cells >= pairs;  cs = 1.0f / (float)cells;  m = margin * cs;  m3 = 3.0f * m
 *   triangle i lies in cell q = i / 2 at column q % cells, row q / cells:  u0 = (float)(q % cells) * cs;  v0 = (float)(q / cells) * cs;  u1 = u0 + cs;  v1 = v0 + cs
 *   i even, the lower-left half:   a = (u0 + m, v0 + m)   b = (u1 - m3, v0 + m)   c = (u0 + m, v1 - m3)
 *   i odd, the upper-right half:   a = (u1 - m, v1 - m)   b = (u0 + m3, v1 - m)   c = (u1 - m, v0 + m3)
 * so each half keeps m from the cell's border and 2m (along an axis) from the cell's diagonal: with margin > 0 and a texel smaller than m no texel centre is
 * covered twice.  Returns cells, or 0 (nothing written) for tris NULL, n < 1 or margin outside [0, 0.25). */
int rtAtlasGrid(rt_triangle* tris, int n, float margin);

#ifdef __cplusplus
}
#endif
#endif
