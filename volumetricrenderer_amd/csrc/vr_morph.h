// vr_morph.h -- the erode / dilate brush of vr_morph / vr_brush_morph_apply
// (include/vr.h), stated once: the argument check and
// the extremum of two bytes.  Plain integer C++ in the manner of vr_blur.h;
// vr_brush.h supplies everything else of the brush (inside test, weight,
// blend): the stage kernel (vr_paint.hip), the host statement (vr_brush.cpp)
// and the stand-alone check (tools/morph_check.cpp) include this file, so they
// cannot diverge.
//
// The structuring element is the (2h + 1)^3 cube, coordinates clamped to the
// volume.  The minimum (maximum) over a cube is the minimum over z of the
// minimum over y of the minimum over x, and a window may be covered by
// overlapping parts (min and max are idempotent), so every partial result is a
// byte and nothing is divided.
#pragma once

#include "vr_brush.h"

namespace vr {
namespace morph {

// the extremum of two bytes: the larger for VR_MORPH_DILATE, else the smaller
VR_BRUSH_FN unsigned pick(int op, unsigned a, unsigned b)
{
    return op == VR_MORPH_DILATE ? (a > b ? a : b) : (a < b ? a : b);
}

// nullptr for a (brush, op, half_width) vr_morph accepts, else what is wrong with it
inline const char* invalid(const vr_brush* b, int op, int half_width)
{
    if (const char* why = brush::invalid(b)) return why;
    if (b->op != VR_BRUSH_SET) return "brush op must be VR_BRUSH_SET";
    if (op != VR_MORPH_ERODE && op != VR_MORPH_DILATE) return "op is VR_MORPH_ERODE or VR_MORPH_DILATE";
    if (half_width < 1 || half_width > VR_MORPH_MAX_HALF) return "half_width outside 1..3";
    return nullptr;
}

}  // namespace morph
}  // namespace vr
