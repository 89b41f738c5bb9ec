// vr_brush.h -- the brush of vr_paint / vr_brush_apply (include/vr.h; DESIGN.md
// sec. 5.2.5), stated once: the argument check, the clipped bounding box, the
// ellipsoid weight and the per-channel blend.  Plain integer C++, host and
// device under hipcc and compilable as plain C++: the paint kernel
// (vr_paint.hip), the host statement (vr_brush.cpp) and the stand-alone check
// (tools/brush_check.cpp) include this file, so they cannot diverge.
//
// Offsets d = texel - centre, D_a = 2 radius[a] + 1, all in unsigned 64 bits:
//   S = Dx^2 Dy^2 Dz^2
//   Q = (2dx)^2 Dy^2 Dz^2 + (2dy)^2 Dx^2 Dz^2 + (2dz)^2 Dx^2 Dy^2
// inside iff |d_a| <= radius[a] on every axis and Q <= S.  At the largest
// radius (255) S = 511^6 < 2^54.2 and each term of Q <= 510^2 511^4 < 2^54, so
// Q < 2^55.6, and 256 Q is only formed for Q <= S: below 2^62.2.
#pragma once

#include <stdint.h>

#include "../../include/vr.h"

#if defined(__HIPCC__)
#define VR_BRUSH_FN __host__ __device__ inline
#else
#define VR_BRUSH_FN inline
#endif

namespace vr {
namespace brush {

// S and, per axis, the factor its (2d)^2 is multiplied by in Q
struct Terms {
    uint64_t s;
    uint64_t k[3];
};

VR_BRUSH_FN Terms terms(const int32_t radius[3])
{
    uint64_t d2[3];
    for (int a = 0; a < 3; ++a) {
        const uint64_t d = 2u * (uint64_t)radius[a] + 1u;
        d2[a] = d * d;
    }
    Terms t;
    t.k[0] = d2[1] * d2[2];
    t.k[1] = d2[0] * d2[2];
    t.k[2] = d2[0] * d2[1];
    t.s = d2[0] * t.k[0];
    return t;
}

// one axis' term of Q for the offset d (|d| <= radius)
VR_BRUSH_FN uint64_t axis_term(int d, uint64_t k)
{
    const uint64_t t = (uint64_t)(2 * (d < 0 ? -d : d));
    return t * t * k;
}

// the weight of an inside texel (q <= s): 256 for a hard edge, else 256 at the centre down to 1 on the rim
VR_BRUSH_FN unsigned weight(uint64_t q, uint64_t s, int falloff)
{
    return falloff ? 256u - (unsigned)((256u * q) / (s + 1u)) : 256u;
}

// the new byte of a channel: a = weight * strength (0..65280)
VR_BRUSH_FN unsigned blend(int op, unsigned old, unsigned value, unsigned a)
{
    if (op == VR_BRUSH_SET) return (old * (65280u - a) + value * a + 32640u) / 65280u;
    const unsigned d = (value * a + 32640u) / 65280u;
    if (op == VR_BRUSH_ADD) return old + d > 255u ? 255u : old + d;
    return old > d ? old - d : 0u;
}

// nullptr for a brush vr_paint accepts, else what is wrong with it
inline const char* invalid(const vr_brush* b)
{
    if (b->op != VR_BRUSH_SET && b->op != VR_BRUSH_ADD && b->op != VR_BRUSH_SUB) return "bad op";
    if (b->falloff != 0 && b->falloff != 1) return "bad falloff";
    for (int a = 0; a < 3; ++a)
        if (b->radius[a] < 0 || b->radius[a] > VR_BRUSH_MAX_RADIUS) return "radius outside 0..255";
    if (b->reserved[0] != 0 || b->reserved[1] != 0) return "reserved must be 0";
    return nullptr;
}

// [centre - radius, centre + radius] clipped to the nx x ny x nz volume, in 64 bits (the centre
// may be anywhere in int32); false, and a zero extent, when the brush misses the volume
inline bool clip(const vr_brush* b, int nx, int ny, int nz, int origin[3], int extent[3])
{
    const int n[3] = {nx, ny, nz};
    int64_t lo[3], hi[3];
    bool hit = true;
    for (int a = 0; a < 3; ++a) {
        lo[a] = (int64_t)b->centre[a] - b->radius[a];
        hi[a] = (int64_t)b->centre[a] + b->radius[a];
        if (lo[a] < 0) lo[a] = 0;
        if (hi[a] > n[a] - 1) hi[a] = n[a] - 1;
        if (lo[a] > hi[a]) hit = false;
    }
    for (int a = 0; a < 3; ++a) {
        origin[a] = hit ? (int)lo[a] : 0;
        extent[a] = hit ? (int)(hi[a] - lo[a] + 1) : 0;
    }
    return hit;
}

}  // namespace brush
}  // namespace vr
