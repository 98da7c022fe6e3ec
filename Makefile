# Top-level build: everything is built IN-TREE so the artefacts travel with the repo snapshot.
#
#   cuda-raytracing-optimized_amd/librt_mi355x.so   HIP renderer behind the reference's C-ABI (gfx950 only)
#   cuda-raytracing-optimized_amd/librt_host.so     host-side scene / BVH / PPM / .ref harness (plain C++, no HIP)
#   oracle/liboracle.so, oracle/_ref/libref.so      CPU checker (test infrastructure; see oracle/Makefile)

PKG      := cuda-raytracing-optimized_amd
HIPCC    ?= hipcc
CXX      ?= g++
ARCH     ?= gfx950
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function
CSRC     := $(PKG)/csrc
HOST     := $(PKG)/host
OBJ      := build/obj

KERNEL_HDRS := $(CSRC)/rt_device.h $(CSRC)/rt_renorm.h $(CSRC)/rt_exactdiv.h $(CSRC)/rt_div64.h $(CSRC)/rt_glibc_sincosf.h $(CSRC)/rt_glibc_powf.h $(CSRC)/rt_params.h include/rt_types.h include/rt_api.h

all: $(PKG)/librt_mi355x.so $(PKG)/librt_host.so
	$(MAKE) -C oracle

$(OBJ):
	@mkdir -p $(OBJ)

# The two floating-point builds of each kernel TU: PARITY never contracts a*b+c into an FMA.
# -fno-slp-vectorize -fno-vectorize (PARITY kernels): the vectorisers pair the un-fused mul/add of two boxes / two spheres into v_pk_mul_f32 /
# v_pk_add_f32.  On gfx950 a packed mul/add issues in 4.56 cycles against 2 x 2.3 for the scalar pair (tools/valu_microbench.hip), so
# it gains nothing, and the register shuffles (v_mov) that feed it cost 20 % of the box test.  FAST keeps it: v_pk_fma_f32 does pay.
$(OBJ)/spheres_parity.o: $(CSRC)/rt_kernels_spheres.hip $(CSRC)/rt_sphere_form.h $(KERNEL_HDRS) | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRT_MODE_PARITY -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
$(OBJ)/spheres_fast.o: $(CSRC)/rt_kernels_spheres.hip $(CSRC)/rt_sphere_form.h $(KERNEL_HDRS) | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRT_MODE_FAST -ffp-contract=fast -fno-hip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize -fno-vectorize -c $< -o $@
$(OBJ)/mesh_parity.o: $(CSRC)/rt_kernels_mesh.hip $(CSRC)/rt_mesh_plan.h $(KERNEL_HDRS) | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRT_MODE_PARITY -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
$(OBJ)/mesh_fast.o: $(CSRC)/rt_kernels_mesh.hip $(CSRC)/rt_mesh_plan.h $(KERNEL_HDRS) | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRT_MODE_FAST -ffp-contract=fast -fno-hip-fp32-correctly-rounded-divide-sqrt -c $< -o $@
$(OBJ)/probe_parity.o: $(CSRC)/rt_probe.hip $(KERNEL_HDRS) include/rt_probe.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRT_MODE_PARITY -ffp-contract=off -c $< -o $@
$(OBJ)/probe_fast.o: $(CSRC)/rt_probe.hip $(KERNEL_HDRS) include/rt_probe.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRT_MODE_FAST -ffp-contract=fast -fno-hip-fp32-correctly-rounded-divide-sqrt -c $< -o $@
# The denoiser's kernels (denoiseFrame): one arithmetic, defined bit for bit, so one object built like the PARITY ones (no contraction, no vectorisers,
# the default correctly rounded divide / sqrt and fp32 denormals).  Its own TU and header: the objects above do not depend on it.
$(OBJ)/denoise.o: $(CSRC)/rt_kernels_denoise.hip $(CSRC)/rt_denoise.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The temporal accumulation's kernel (accumulateFrame): defined bit for bit as the denoiser is, so one object with the flags of denoise.o; the launcher's
# host arithmetic (the constants of the previous camera) is compiled under them too.  Its own TU and header: no other kernel object depends on it.
$(OBJ)/accumulate.o: $(CSRC)/rt_kernels_accumulate.hip $(CSRC)/rt_accumulate.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The kernels of previewFrame (temporal moments, variance, variance-guided a-trous): defined bit for bit as the two passes it fuses, so one object with the
# flags of denoise.o; the launcher's host arithmetic is compiled under them too.  Its own TU and header: no other kernel object depends on it.
$(OBJ)/preview.o: $(CSRC)/rt_kernels_preview.hip $(CSRC)/rt_preview.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The kernels of displayFrame (luminance histogram, exposure, tone map, sRGB bytes): defined bit for bit as the passes above, so one object with the flags of
# denoise.o.  Its powf is rt_glibc_powf_pos.h, which takes its tables from rt_glibc_powf.h without changing it.  Its own TU and header: no other kernel object
# depends on it.
$(OBJ)/display.o: $(CSRC)/rt_kernels_display.hip $(CSRC)/rt_display.h $(CSRC)/rt_glibc_powf_pos.h $(CSRC)/rt_glibc_powf.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The BVH refit of updateTriangles (node boxes, child-pair records, compact leaf records): comparisons, selects and one rounded subtraction per edge component,
# defined bit for bit as the passes above, so one object with the flags of display.o.  Its own TU and header: no other kernel object depends on it.
$(OBJ)/update.o: $(CSRC)/rt_kernels_update.hip $(CSRC)/rt_update.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The BVH rebuild of rebuildBvh (gather, radix sorts, per level segmented box scans, SAH costs, argmin, stable partition; emit): areas and costs are rounded
# operation by operation as the host builder's, so one object with the flags of display.o.  Its own TU and header: no other kernel object depends on it.
$(OBJ)/build.o: $(CSRC)/rt_kernels_build.hip $(CSRC)/rt_build.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The kernels of refineFrame around the pixel kernels (selection, class histogram, list compaction, statistics update, delivery): the error estimate is
# defined bit for bit as the passes above, so one object with the flags of display.o.  Its own TU and header: no other kernel object depends on it.
$(OBJ)/refine.o: $(CSRC)/rt_kernels_refine.hip $(CSRC)/rt_refine.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The kernels of rtMarkPose / renderMotion (the motion planes the temporal passes read with a pose marked; the gather that carries the mark through a rebuild):
# defined bit for bit as the passes above, so one object with the flags of accumulate.o; the launcher's host arithmetic is compiled under them too.  Its own
# TU and header: no other kernel object depends on it.
$(OBJ)/motion.o: $(CSRC)/rt_kernels_motion.hip $(CSRC)/rt_motion.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The kernels of gatherRadiance around the radiance and any-hit kernels (the directions of a chunk of points, the per-point reduction): defined bit for bit as
# the passes above, so one object with the flags of display.o.  The generator's arithmetic is rt_gather_dirs.h, which librt_host.so compiles too
# (rtGatherDirectionsHost).  Its own TU and headers: no other kernel object depends on it.
$(OBJ)/gather.o: $(CSRC)/rt_kernels_gather.hip $(CSRC)/rt_gather.h $(CSRC)/rt_gather_dirs.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The kernels of rasterTexels / bakeTexels (the UV-atlas raster, dilation, compaction, the indexed generator, the scatter): defined bit for bit as the passes
# above, so one object with the flags of gather.o.  The raster's arithmetic is rt_texel_raster.h, which librt_host.so compiles too (rtRasterTexelsHost); the
# generator's is rt_gather_dirs.h, unchanged.  Its own TU and headers: no other kernel object depends on it.
$(OBJ)/texels.o: $(CSRC)/rt_kernels_texels.hip $(CSRC)/rt_texels.h $(CSRC)/rt_texel_raster.h $(CSRC)/rt_gather.h $(CSRC)/rt_gather_dirs.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The kernels of filterTexels (the prologue that packs a texel's position, normal and footprint into records, the a-trous iterations, the scatter through the
# dilated source plane): defined bit for bit as the passes above, so one object with the flags of texels.o.  The filter's arithmetic is rt_texel_filter.h,
# which librt_host.so compiles too (rtFilterTexelsHost); the raster's is rt_texel_raster.h, unchanged.  Its own TU and headers: no other kernel object depends
# on it.
$(OBJ)/texel_filter.o: $(CSRC)/rt_kernels_texel_filter.hip $(CSRC)/rt_texel_filter.h $(CSRC)/rt_texel_filter_launch.h $(CSRC)/rt_texel_raster.h include/rt_types.h include/rt_api.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
# The kernels of sampleTexels / renderLightmap (the lookup of texel planes at hits; the generator of a chunk of centre rays and the shade kernel around the
# unchanged closest-hit ray kernel): defined bit for bit as the passes above, so one object with the flags of texels.o - and RT_MODE_PARITY, which selects in
# rt_device.h the forms of the centre ray, the albedo and the sky that the guide and ray kernels compile (they exist in the PARITY objects only).  The lookup's
# arithmetic is rt_texel_sample.h, which librt_host.so compiles too (rtSampleTexelsHost).  Its own TU and headers: no other kernel object depends on it.
$(OBJ)/lightmap.o: $(CSRC)/rt_kernels_lightmap.hip $(CSRC)/rt_lightmap.h $(CSRC)/rt_texel_sample.h $(KERNEL_HDRS) | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRT_MODE_PARITY -ffp-contract=off -fno-slp-vectorize -fno-vectorize -c $< -o $@
$(OBJ)/renderer.o: $(CSRC)/rt_renderer.hip $(CSRC)/rt_params.h $(CSRC)/rt_scene_layout.h $(CSRC)/rt_denoise.h $(CSRC)/rt_accumulate.h $(CSRC)/rt_preview.h $(CSRC)/rt_motion.h $(CSRC)/rt_display.h $(CSRC)/rt_update.h $(CSRC)/rt_build.h $(CSRC)/rt_refine.h $(CSRC)/rt_gather.h $(CSRC)/rt_texels.h $(CSRC)/rt_texel_filter_launch.h $(CSRC)/rt_lightmap.h include/rt_api.h include/rt_types.h | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

RT_OBJS := $(OBJ)/renderer.o $(OBJ)/probe_parity.o $(OBJ)/probe_fast.o $(OBJ)/spheres_parity.o $(OBJ)/spheres_fast.o $(OBJ)/mesh_parity.o $(OBJ)/mesh_fast.o $(OBJ)/denoise.o $(OBJ)/accumulate.o
RT_OBJS += $(OBJ)/preview.o
DISPLAY_OBJS := $(OBJ)/display.o
UPDATE_OBJS := $(OBJ)/update.o
BUILD_OBJS := $(OBJ)/build.o
REFINE_OBJS := $(OBJ)/refine.o
MOTION_OBJS := $(OBJ)/motion.o
GATHER_OBJS := $(OBJ)/gather.o
TEXELS_OBJS := $(OBJ)/texels.o
FILTER_OBJS := $(OBJ)/texel_filter.o
LIGHTMAP_OBJS := $(OBJ)/lightmap.o

$(PKG)/librt_mi355x.so: $(RT_OBJS) $(DISPLAY_OBJS) $(UPDATE_OBJS) $(BUILD_OBJS) $(REFINE_OBJS) $(MOTION_OBJS) $(GATHER_OBJS) $(TEXELS_OBJS) $(FILTER_OBJS) $(LIGHTMAP_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(RT_OBJS) $(DISPLAY_OBJS) $(UPDATE_OBJS) $(BUILD_OBJS) $(REFINE_OBJS) $(MOTION_OBJS) $(GATHER_OBJS) $(TEXELS_OBJS) $(FILTER_OBJS) $(LIGHTMAP_OBJS) -o $@

$(PKG)/librt_host.so: $(HOST)/rt_scenes.cpp $(HOST)/rt_bvh.cpp $(HOST)/rt_harness.cpp $(HOST)/rt_display_host.cpp $(HOST)/rt_gather_host.cpp $(HOST)/rt_texels_host.cpp $(HOST)/rt_texel_filter_host.cpp $(HOST)/rt_texel_sample_host.cpp $(CSRC)/rt_gather_dirs.h $(CSRC)/rt_texel_raster.h $(CSRC)/rt_texel_filter.h $(CSRC)/rt_texel_sample.h include/rt_host.h include/rt_types.h include/rt_api.h
	$(CXX) -O2 -ffp-contract=off -std=c++14 -Wall -fPIC -shared $(HOST)/rt_scenes.cpp $(HOST)/rt_bvh.cpp $(HOST)/rt_harness.cpp $(HOST)/rt_display_host.cpp $(HOST)/rt_gather_host.cpp $(HOST)/rt_texels_host.cpp $(HOST)/rt_texel_filter_host.cpp $(HOST)/rt_texel_sample_host.cpp -o $@

oracle: $(PKG)/librt_mi355x.so $(PKG)/librt_host.so
	$(MAKE) -C oracle

clean:
	rm -rf build/obj $(PKG)/librt_mi355x.so $(PKG)/librt_host.so
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
