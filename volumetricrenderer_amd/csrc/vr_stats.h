// vr_stats.h -- the statistics of vr_brush_stats / vr_box_stats (include/vr.h;
// DESIGN.md sec. 5.2.8), stated once: which texels count and with what weight,
// which channels are selected, what a texel adds to which field, and the
// summary's rounding.  Plain integer C++ in the manner of vr_brush.h, which
// supplies the ellipsoid: the kernel k_stats (vr_paint.hip), the host
// statements (vr_brush.cpp) and the stand-alone check (tools/stats_check.cpp)
// include this file, so they cannot diverge.
//
// Per inside texel: count += 1, weight += w (1..256), and per selected
// channel wsum += w * byte (<= 65280) and hist[byte] += 1.  A volume has fewer
// than 2^31 texels, so every 64-bit field stays below 2^47.
#pragma once

#include "vr_brush.h"

namespace vr {
namespace stats {

// the weight of every texel of a box (vr_box_stats): the hard edge's
constexpr unsigned kBoxWeight = 256u;

// The weight with which a texel counts, 0 = it does not: for a brush (ellipsoid != 0) the texel at Q = q of an
// ellipsoid S = s, for a box every texel.  An inside texel's weight is at least 1.
VR_BRUSH_FN unsigned texel_weight(int ellipsoid, uint64_t q, uint64_t s, int falloff)
{
    if (!ellipsoid) return kBoxWeight;
    return q <= s ? brush::weight(q, s, falloff) : 0u;
}

// bit c set = channel c is selected: vr_paint's rule, strength != 0
VR_BRUSH_FN unsigned brush_mask(const uint8_t strength[4])
{
    unsigned m = 0u;
    for (int c = 0; c < 4; ++c) m |= strength[c] ? 1u << c : 0u;
    return m;
}

VR_BRUSH_FN bool selected(unsigned mask, int c) { return (mask >> c & 1u) != 0u; }

// what an inside texel of weight w adds to wsum[c] of a selected channel that holds `byte`
VR_BRUSH_FN uint64_t wsum_term(unsigned w, unsigned byte) { return (uint64_t)(w * byte); }

// one inside texel into *s, on the host: t = its four bytes (an unselected channel's is not read)
inline void add_texel(vr_volume_stats* s, unsigned mask, unsigned w, const uint8_t* t)
{
    s->count += 1u;
    s->weight += w;
    for (int c = 0; c < 4; ++c) {
        if (!selected(mask, c)) continue;
        s->wsum[c] += wsum_term(w, t[c]);
        s->hist[c][t[c]] += 1u;
    }
}

// num / den rounded to the nearest, halves upwards (den > 0): the summary's means
VR_BRUSH_FN uint64_t rounded_div(uint64_t num, uint64_t den) { return (num + den / 2u) / den; }

// nullptr for a channel mask vr_box_stats accepts
inline const char* invalid_mask(int channel_mask)
{
    return channel_mask < 0 || channel_mask > 15 ? "channel_mask outside 0..15" : nullptr;
}

// vr_stats_summary (vr.h)
inline void summary(const vr_volume_stats* s, vr_volume_summary* out)
{
    for (int c = 0; c < 4; ++c) {
        uint64_t n = 0, vsum = 0;
        int lo = -1, hi = -1;
        for (int v = 0; v < 256; ++v) {
            const uint64_t h = s->hist[c][v];
            if (!h) continue;
            if (lo < 0) lo = v;
            hi = v;
            n += h;
            vsum += (uint64_t)v * h;
        }
        out->n[c] = n;
        out->min[c] = out->max[c] = out->mean[c] = out->wmean[c] = out->median[c] = 0;
        if (n == 0) continue;
        out->min[c] = lo;
        out->max[c] = hi;
        out->mean[c] = (int32_t)rounded_div(vsum, n);
        // an inside texel weighs at least 1, so weight >= count >= n > 0 in a result of the calls above; a struct
        // put together by hand with weight 0 gets 0
        out->wmean[c] = s->weight ? (int32_t)rounded_div(s->wsum[c], s->weight) : 0;
        uint64_t cum = 0;
        for (int v = lo; v <= hi; ++v) {
            cum += s->hist[c][v];
            if (2u * cum >= n) { out->median[c] = v; break; }
        }
    }
}

}  // namespace stats
}  // namespace vr
