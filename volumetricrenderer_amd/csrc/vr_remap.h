// vr_remap.h -- the lookup-table brush and its tables: vr_remap / vr_remap_device
// / vr_brush_remap_apply, the builders vr_lut_identity / vr_lut_levels /
// vr_lut_compose and vr_stats_lut / vr_stats_lut_device (include/vr.h;
// DESIGN.md sec. 5.2.11), stated once: the argument checks, one entry of a
// levels table, and one entry of a table built from a histogram.  Plain
// integer C++ in the manner of vr_clone.h and vr_stats.h; vr_brush.h supplies
// everything else of the brush (inside test, weight, blend): the kernels
// (vr_paint.hip), the host statements (vr_brush.cpp) and the stand-alone
// check (tools/remap_check.cpp) include this file, so they cannot diverge.
//
// The remap brush is a source brush (sec. 5.2.10) whose per-texel value is
// v_c(t) = lut[c][old_c(t)]: new = blend(op, old, lut[c][old], w * strength[c]).
#pragma once

#include "vr_brush.h"

namespace vr {
namespace remap {

// nullptr for a channel mask the builders accept
inline const char* invalid_mask(int channel_mask)
{
    return channel_mask < 0 || channel_mask > 15 ? "channel_mask outside 0..15" : nullptr;
}

inline const char* invalid_kind(int kind)
{
    return kind != VR_LUT_EQUALIZE && kind != VR_LUT_STRETCH ? "bad kind" : nullptr;
}

// nullptr for the ranges vr_lut_levels accepts: 0 <= in_lo < in_hi <= 255, out_lo and out_hi in 0..255 in either order
inline const char* invalid_levels(int in_lo, int in_hi, int out_lo, int out_hi)
{
    if (in_lo < 0 || in_hi > 255 || in_lo >= in_hi) return "input range is not 0 <= in_lo < in_hi <= 255";
    if (out_lo < 0 || out_lo > 255 || out_hi < 0 || out_hi > 255) return "output range outside 0..255";
    return nullptr;
}

// floor(a / b) for b > 0, also for a negative a (vr_brush_line's rule)
VR_BRUSH_FN int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// one entry of a levels table (valid ranges): out_lo at and below in_lo, out_hi at and above in_hi, between them
// the nearest point of the line through the two, halves towards +infinity.  |2 (v - in_lo)(out_hi - out_lo)| < 2^17.
VR_BRUSH_FN unsigned levels_value(int v, int in_lo, int in_hi, int out_lo, int out_hi)
{
    if (v <= in_lo) return (unsigned)out_lo;
    if (v >= in_hi) return (unsigned)out_hi;
    const int den = in_hi - in_lo;
    return (unsigned)(out_lo + floor_div(2 * (v - in_lo) * (out_hi - out_lo) + den, 2 * den));
}

// What a channel's histogram says: lo and hi the lowest and highest non-empty bin (lo > hi: none), n the sum of
// the bins and cmin = cum(lo) = the lowest non-empty bin's count.  All sums are unsigned 64-bit.
struct Range {
    int lo, hi;
    uint64_t n, cmin;
};

// true when the channel's table is a function of the histogram, false when it is the identity: an unselected
// channel, an empty one, one with a single non-empty bin -- and, for VR_LUT_EQUALIZE, a histogram put together by
// hand whose sums wrap 64 bits so that n - cmin is 0 (a result of vr_brush_stats / vr_box_stats stays below 2^47).
VR_BRUSH_FN bool mapped(int kind, bool selected, const Range& r)
{
    if (!selected || r.lo >= r.hi) return false;
    return kind == VR_LUT_STRETCH || r.n - r.cmin != 0u;
}

// one entry of a mapped channel's table; cum = cum(v) = the sum of the bins up to and including v (VR_LUT_EQUALIZE
// only).  Below 2^47 nothing wraps and the result is 0..255; the byte is what the table stores.
VR_BRUSH_FN unsigned stats_value(int kind, int v, uint64_t cum, const Range& r)
{
    if (kind == VR_LUT_STRETCH) {
        if (v <= r.lo) return 0u;
        if (v >= r.hi) return 255u;
        const unsigned den = (unsigned)(r.hi - r.lo);
        return ((unsigned)(v - r.lo) * 255u + den / 2u) / den;
    }
    if (v < r.lo) return 0u;
    const uint64_t den = r.n - r.cmin;
    return (unsigned)(((cum - r.cmin) * 255u + den / 2u) / den) & 255u;
}

// vr_stats_lut (vr.h): validated arguments
inline void stats_lut(const vr_volume_stats* s, int kind, unsigned mask, vr_lut* out)
{
    for (int c = 0; c < 4; ++c) {
        Range r{256, -1, 0u, 0u};
        for (int v = 0; v < 256; ++v) {
            const uint64_t h = s->hist[c][v];
            if (!h) continue;
            if (r.lo > 255) { r.lo = v; r.cmin = h; }
            r.hi = v;
            r.n += h;
        }
        const bool map = mapped(kind, (mask >> c & 1u) != 0u, r);
        uint64_t cum = 0u;
        for (int v = 0; v < 256; ++v) {
            cum += s->hist[c][v];
            out->lut[c][v] = (uint8_t)(map ? stats_value(kind, v, cum, r) : (unsigned)v);
        }
    }
}

}  // namespace remap
}  // namespace vr
