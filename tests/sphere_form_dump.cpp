// sphere_form_dump.cpp — runs sphere_frame_form (rt_sphere_form.h) on the cases of tests/test_sphere_form.py: plain C++, no kernel, no HIP call, no GPU.
// stdin: one case per line, the integers named in kInputs below (a pointer field: 0 = null, else present).  stdout: one line per case, the form.
// `--fields` prints the list of inputs and the values of the two forms and of the frame kinds instead, for the test to hold its own against.
#include <cstdio>
#include <cstring>

#include "rt_sphere_form.h"

static const char* const kInputs = "frame kind_folded default_constants xcd_queues ord_rec mid_waves tune fb_global_rows poison_fb counters wave_dbg";
constexpr int kInputCount = 11;

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "--fields") == 0) {
        printf("%s\n%d %d\n%d %d %d %d %d %d %d\n", kInputs, kSphereFormGeneral, kSphereFormDefault, (int)SphereFrame::Tiles, (int)SphereFrame::GlobalSingle,
               (int)SphereFrame::TwoDispatch, (int)SphereFrame::TwoDispatchResume, (int)SphereFrame::OrderedSingle, (int)SphereFrame::ClassifiedSingle,
               (int)SphereFrame::PlainSingle);
        return 0;
    }
    static unsigned char present[64];      // what a non-null pointer field points to (the rule reads no pointee)
    long long v[kInputCount];
    for (;;) {
        for (int i = 0; i < kInputCount; i++)
            if (scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 1;       // end of input; a partial line is an error
        auto ptr = [&](int i) { return v[i] ? (void*)present : nullptr; };
        RtSphereParams p;
        memset(&p, 0, sizeof p);
        RtSwitches sw;
        int k = 0;
        const SphereFrame frame = (SphereFrame)v[k++];
        const bool kind_folded = v[k++] != 0;
        const bool default_constants = v[k++] != 0;
        p.xcd_queues = (int32_t)v[k++];
        p.ord_rec = (float4*)ptr(k++);
        sw.mid_waves = (int)v[k++];
        if (v[k++]) sw.tune = RtTune{};
        p.fb_global_rows = (int32_t)v[k++];
        p.poison_fb = (int32_t)v[k++];
        p.counters = (RtCounters*)ptr(k++);
        p.wave_dbg = (unsigned long long*)ptr(k++);
        if (k != kInputCount) return 2;
        printf("%d\n", sphere_frame_form(frame, p, sw, kind_folded, default_constants));
    }
}
