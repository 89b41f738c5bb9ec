// frames_check -- stand-alone host check of frames_share_camera
// (volumetricrenderer_amd/csrc/vr_internal.h), the predicate that sends a four-frame
// launch to the QUAD kernels: no libvr.so, no HIP runtime call, no device.
// `make check-frames` builds it with -fsanitize=address,undefined and runs it.
//
// Equal frames share a camera; a frame that differs from frame 0 in any compared
// field -- every element of it, by one ulp or one bit, a sign of zero included --
// does not; the target pointer and the step counter may differ; only four frames do.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "vr_internal.h"

using namespace vr;

namespace {

int g_fail = 0;
#define CHECK(...)                                                              \
    do {                                                                        \
        if (!(__VA_ARGS__)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__);  \
            ++g_fail;                                                           \
        }                                                                       \
    } while (0)

FrameArgs base_frame()
{
    FrameArgs f;
    std::memset(&f, 0, sizeof f);   // the padding too: the predicate must not read it
    float v = 0.125f;
    auto fill = [&](float* p, int n) { for (int i = 0; i < n; ++i) p[i] = (v += 0.375f); };
    fill(f.org, 3); fill(f.o, 3); fill(f.px, 3); fill(f.py, 3); fill(f.r2, 4); fill(f.r3, 4); fill(f.cam, 3);
    fill(&f.tap_T[0][0], 12);
    f.cam_mode = 1;
    f.empty_fill = 1;
    return f;
}

unsigned long long g_counters[4];
char g_pixels[4][16];

void reset(FrameArgs* fr)
{
    for (int k = 0; k < 4; ++k) {
        fr[k] = base_frame();
        fr[k].out = g_pixels[k];
        fr[k].step_counter = nullptr;
    }
}

// frame k's float array p (n elements) differing in turn: one ulp up, one ulp down, the sign
template <class Get>
void check_floats(const char* name, int n, Get get)
{
    FrameArgs fr[4];
    for (int k = 1; k < 4; ++k)
        for (int i = 0; i < n; ++i)
            for (int how = 0; how < 3; ++how) {
                reset(fr);
                float* p = get(fr[k]) + i;
                *p = how == 0 ? std::nextafterf(*p, INFINITY) : how == 1 ? std::nextafterf(*p, -INFINITY) : -*p;
                if (frames_share_camera(fr, 4)) {
                    std::printf("FAIL: %s[%d] of frame %d differs (%d) and the frames share a camera\n", name, i, k, how);
                    ++g_fail;
                }
            }
    // +0 and -0 are two cameras (the comparison is of bits), equal NaNs are one
    reset(fr);
    for (int k = 0; k < 4; ++k) get(fr[k])[0] = 0.0f;
    CHECK(frames_share_camera(fr, 4));
    get(fr[2])[0] = -0.0f;
    CHECK(!frames_share_camera(fr, 4));
    for (int k = 0; k < 4; ++k) get(fr[k])[0] = NAN;
    CHECK(frames_share_camera(fr, 4));
}

}  // namespace

int main()
{
    FrameArgs fr[4];

    // equal frames
    reset(fr);
    CHECK(frames_share_camera(fr, 4));
    for (int n = -1; n <= 3; ++n) CHECK(!frames_share_camera(fr, n));   // a pair or fewer: never

    // the per-frame fields
    reset(fr);
    for (int k = 0; k < 4; ++k) fr[k].step_counter = &g_counters[k];
    CHECK(frames_share_camera(fr, 4));
    fr[3].out = g_pixels[0];
    fr[1].step_counter = nullptr;
    CHECK(frames_share_camera(fr, 4));

    // each compared field in turn, every element, in every frame but the first
    check_floats("org", 3, [](FrameArgs& f) { return f.org; });
    check_floats("o", 3, [](FrameArgs& f) { return f.o; });
    check_floats("px", 3, [](FrameArgs& f) { return f.px; });
    check_floats("py", 3, [](FrameArgs& f) { return f.py; });
    check_floats("r2", 4, [](FrameArgs& f) { return f.r2; });
    check_floats("r3", 4, [](FrameArgs& f) { return f.r3; });
    check_floats("cam", 3, [](FrameArgs& f) { return f.cam; });
    check_floats("tap_T", 12, [](FrameArgs& f) { return &f.tap_T[0][0]; });
    for (int k = 1; k < 4; ++k) {
        reset(fr);
        fr[k].cam_mode = 0;
        CHECK(!frames_share_camera(fr, 4));
        reset(fr);
        fr[k].empty_fill = 0;
        CHECK(!frames_share_camera(fr, 4));
    }
    // frame 0 is the one the others are compared with
    reset(fr);
    fr[0].px[1] = std::nextafterf(fr[0].px[1], INFINITY);
    CHECK(!frames_share_camera(fr, 4));

    // which kernels have a QUAD instance: all but the general COL48 / BRICK4832 one with zero
    // offsets and no early-out
    for (int l : {(int)LAYOUT_COL48, (int)LAYOUT_BRICK4832, (int)LAYOUT_CORNERH})
        for (int early = 0; early < 2; ++early)
            for (int zo = 0; zo < 2; ++zo)
                for (int um = 0; um < 16; ++um) {
                    const bool u = u_kernel_channel(early != 0, zo != 0, um) >= 0;
                    const bool want = u || l == LAYOUT_CORNERH || early || !zo;
                    CHECK(quad_instance(l, early != 0, zo != 0, um) == want);
                }

    // the classification covers the struct: its fields' sizes add up to it (less padding
    // than one pointer), so a field the bindings of frames_share_camera would miss is also
    // missed here and shows
    constexpr size_t fields = sizeof(float) * (3 * 4 + 4 * 2 + 3 + 12) + 2 * sizeof(int) + 2 * sizeof(void*);
    static_assert(sizeof(FrameArgs) >= fields && sizeof(FrameArgs) - fields < sizeof(void*), "a field of FrameArgs is not classified");

    std::printf("frames_check: %s\n", g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
}
