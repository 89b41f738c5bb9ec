// vr_warp.h -- the liquify brush: vr_warp and its host statement
// vr_brush_warp_apply (include/vr.h), stated once: the
// argument check, the reach of a map over a brush, the 16.16 source position of
// a texel -- the affine position blended with the texel's own by the brush
// weight -- and the map of a push.  Plain integer C++ in the manner of
// vr_affine.h, which supplies the affine position, the outside test, the clamp
// and both filters; vr_brush.h supplies the inside test and the weight: the
// kernel (vr_paint.hip), the host statement (vr_brush.cpp) and the stand-alone
// check (tools/warp_check.cpp) include this file, so they cannot diverge.
//
// A = affine::position stays below 2^59 (vr_affine.h) and I = t << 16, t a texel
// of the volume or a corner of the brush's box (|t| < 2^31 + 2^8), below 2^48:
// D = A - I fits signed 64 bits.  D is affine in t, so its values at the 8
// corners of the unclipped box bound it at every texel under the brush; a map
// is accepted only when those are at most VR_WARP_MAX_DISP << 16 = 2^31 in
// magnitude, and with w <= 256 = 2^8 the product w * D stays at or below 2^39 --
// below 2^40.  (w * D) >> 8 lies between 0 and D, so P lies between I and A.
#pragma once

#include "vr_affine.h"

namespace vr {
namespace warp {

VR_BRUSH_FN int64_t identity(int t) { return (int64_t)t << 16; }

// D_a of the texel (tx, ty, tz), t = its coordinate on axis a: the displacement the map asks for
VR_BRUSH_FN int64_t displacement(const int32_t row[3], int32_t origin, const int32_t pivot[3], int tx, int ty, int tz, int t)
{
    return affine::position(row, origin, pivot, tx, ty, tz) - identity(t);
}

// P_a of a texel of weight w (1..256) whose displacement is d: >> is the arithmetic shift (floor); w = 256 gives I + D = A
VR_BRUSH_FN int64_t position(int t, int64_t d, unsigned w) { return identity(t) + (((int64_t)w * d) >> 8); }

// max |D_a| per axis over the 8 corners of the unclipped box [centre - radius, centre + radius] of a brush whose radii
// are valid (0..255)
inline void reach(const vr_brush* b, const vr_affine* m, int64_t out[3])
{
    for (int a = 0; a < 3; ++a) {
        out[a] = 0;
        for (int k = 0; k < 8; ++k) {
            int64_t t[3];
            for (int c = 0; c < 3; ++c) t[c] = (int64_t)b->centre[c] + (k >> c & 1 ? b->radius[c] : -b->radius[c]);
            int64_t p = (int64_t)m->origin[a];
            for (int c = 0; c < 3; ++c) p += (int64_t)m->m[a][c] * (t[c] - (int64_t)m->pivot[c]);
            const int64_t d = p - t[a] * 65536;
            const int64_t mag = d < 0 ? -d : d;
            if (mag > out[a]) out[a] = mag;
        }
    }
}

constexpr int64_t kMaxReach = (int64_t)VR_WARP_MAX_DISP << 16;

// nullptr for a (brush, map) vr_warp accepts, else what is wrong with it
inline const char* invalid(const vr_brush* b, const vr_affine* m)
{
    if (const char* why = affine::invalid(b, m)) return why;
    if (b->op != VR_BRUSH_SET) return "op must be VR_BRUSH_SET";
    int64_t r[3];
    reach(b, m, r);
    for (int a = 0; a < 3; ++a)
        if (r[a] > kMaxReach) return "displacement above VR_WARP_MAX_DISP texels under the brush";
    return nullptr;
}

// The map of a push: the content under the brush moves by +d (16.16 texels).  false when an origin leaves int32.
inline bool push(const int32_t centre[3], const int32_t d16[3], int filter, int border, vr_affine* out)
{
    vr_affine r{};
    for (int a = 0; a < 3; ++a) {
        const int64_t o = (int64_t)centre[a] * 65536 - (int64_t)d16[a];
        if (o > 2147483647ll || o < -2147483647ll - 1) return false;
        r.m[a][a] = VR_AFFINE_ONE;
        r.pivot[a] = centre[a];
        r.origin[a] = (int32_t)o;
    }
    r.filter = filter;
    r.border = border;
    *out = r;
    return true;
}

// The texels the box o, e (inside the volume) reads on axis a of the n texels: every P lies between the texel's own
// position and its affine one, so the hull of the box and of affine::read_range holds both texels of every position.
inline void read_range(const vr_affine* m, int a, const int o[3], const int e[3], int n, int* first, int* last_)
{
    affine::read_range(m, a, o, e, n, first, last_);
    if (o[a] < *first) *first = o[a];
    if (o[a] + e[a] - 1 > *last_) *last_ = o[a] + e[a] - 1;
}

}  // namespace warp
}  // namespace vr
