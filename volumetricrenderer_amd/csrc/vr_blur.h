// vr_blur.h -- the box filter of vr_blur / vr_brush_blur_apply (include/vr.h;
// DESIGN.md sec. 5.2.7), stated once: the filter's argument check, its texel
// count and the rounded mean.  Plain integer C++ in the manner of vr_brush.h,
// which supplies everything else of the brush (inside test, weight, blend):
// the blur kernels (vr_paint.hip), the host statement (vr_brush.cpp) and the
// stand-alone check (tools/blur_check.cpp) include this file, so they cannot
// diverge.
//
// The sum of one channel over the (2h + 1)^3 texels around a texel, coordinates
// clamped to the volume, is at most 343 * 255 = 87465 for h = 3: 32 bits hold
// it, and 16 bits hold the partial sums over one and two axes (49 * 255).
#pragma once

#include "vr_brush.h"

namespace vr {
namespace blur {

// the texels of the filter: N = (2h + 1)^3 = 27, 125, 343
VR_BRUSH_FN unsigned count(int h)
{
    const unsigned w = 2u * (unsigned)h + 1u;
    return w * w * w;
}

// the mean of `sum` over the filter's texels, halves upwards: 0..255
VR_BRUSH_FN unsigned mean(unsigned sum, int h)
{
    const unsigned n = count(h);
    return (sum + n / 2u) / n;
}

// nullptr for a (brush, half_width) vr_blur accepts, else what is wrong with it
inline const char* invalid(const vr_brush* b, int half_width)
{
    if (const char* why = brush::invalid(b)) return why;
    if (b->op != VR_BRUSH_SET) return "op must be VR_BRUSH_SET";
    if (half_width < 1 || half_width > VR_BLUR_MAX_HALF) return "half_width outside 1..3";
    return nullptr;
}

}  // namespace blur
}  // namespace vr
