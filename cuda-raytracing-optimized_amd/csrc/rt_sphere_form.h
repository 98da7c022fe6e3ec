// rt_sphere_form.h — the frame form of the sphere kernel's cost-ordered dispatch: which of a frame's switches k_render_spheres_queue carries as run-time state
// and which are compiled in.  The kinds of frame the sphere launcher (rt_kernels_spheres.hip, plan_spheres) knows and the rule by which it takes the folded
// form.  No kernel and no HIP call in here: a plain C++ program that includes this header runs the rule on a machine without a GPU
// (tests/sphere_form_dump.cpp, tests/test_sphere_form.py).
#pragma once

#include "rt_params.h"

enum class SphereFrame {
    Tiles,              // the tile kernel
    GlobalSingle,       // the scene in global memory: one scattered dispatch
    TwoDispatch,        // first samples of every pixel, k_order_by_cost, then the rest longest first
    TwoDispatchResume,  // a continuation pass of a progressive frame: the ordering pass and the second dispatch alone
    OrderedSingle,      // a frame ordered by the last frame's cost map: the ordering pass and ONE dispatch of whole pixels, longest first - no measuring dispatch
    ClassifiedSingle,   // k_classify_spheres, then one dispatch in its order
    PlainSingle,        // one dispatch, scattered or tile-major
};

// FORM of the cost-ordered dispatch (PHASE 2, CLS 2):
//   kSphereFormGeneral  every switch of the frame is decided in the kernel at run time, as in every other dispatch
//   kSphereFormDefault  compiled for the frame every production call renders: a queue per XCD, the parked state in 32-byte records, no middle tier, pixels
//                       stored into the compact device framebuffer, the scheduling constants (the kernel's cfg, chain_cfg and caps words) at their defaults as
//                       immediates.  The kernel has no code for anything else, so the rule below must hold in full.
constexpr int kSphereFormGeneral = RT_SPHERE_FORM_GENERAL, kSphereFormDefault = RT_SPHERE_FORM_DEFAULT;        // (rtLastSphereForm, rt_api.h, reports them)

// The form of the cost-ordered dispatch of a frame of kind `frame` (only the three kinds that have such a dispatch can take the folded form), rendered with
// parameter block `p` under the switches `sw`.  kind_folded: the plan's instantiation is one that is built in the folded form (the lean kinds of the full LDS
// copy, whole pixels); default_constants: the plan's scheduling words are the ones that kernel is compiled with (RT_POOL, RT_CHAIN_SINGLE, RT_SINGLE_RAY and
// the variant's scheduling bits at their defaults).  RT_XCD_QUEUES=0, RT_ORD_PACKED=0, RT_MID with waves, RT_FB_DIRECT=1, counters and RT_WAVE_DEBUG each select the general form; so does
// RT_TUNE: the tuning experiments are made on the kernel in which every constant is run-time state.
inline int sphere_frame_form(SphereFrame frame, const RtSphereParams& p, const RtSwitches& sw, bool kind_folded, bool default_constants) {
    const bool cost_ordered = frame == SphereFrame::TwoDispatch || frame == SphereFrame::OrderedSingle || frame == SphereFrame::TwoDispatchResume;
    const bool direct = p.fb_global_rows != 0 || p.poison_fb != 0;
    const bool diagnostics = p.counters != nullptr || p.wave_dbg != nullptr;
    return (cost_ordered && kind_folded && default_constants && p.xcd_queues == kXcdQueues && p.ord_rec != nullptr && sw.mid_waves == 0 && !sw.tune && !direct && !diagnostics) ? kSphereFormDefault
                                                                                                                                              : kSphereFormGeneral;
}
