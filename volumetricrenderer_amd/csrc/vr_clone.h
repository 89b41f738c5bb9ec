// vr_clone.h -- the brushes whose value is a texel: vr_clone / vr_brush_clone_apply
// and vr_stamp / vr_brush_stamp_apply / vr_stamp_box (include/vr.h; DESIGN.md
// sec. 5.2.10), stated once: the argument checks, the source coordinate of a
// cloned texel, the rule that picks the clone's device path, and the edited
// box of a stamp.  Plain integer C++ in the manner of vr_blur.h and vr_morph.h;
// vr_brush.h supplies everything else of the brush (inside test, weight,
// blend): the kernels (vr_paint.hip), the host statements (vr_brush.cpp) and
// the stand-alone check (tools/clone_check.cpp) include this file, so they
// cannot diverge.
//
// Every sum of two int32 is formed in 64 bits and clamped (or compared) there,
// so every offset and every placement origin is legal.
#pragma once

#include "vr_brush.h"

namespace vr {
namespace clone {

// the source coordinate of the texel coordinate t (0 <= t < n) on an axis of n texels: mapped, then
// clamped to the volume (clamp-to-edge).  Monotone in t: rising without the mirror, falling with it.
VR_BRUSH_FN int source(int t, int32_t offset, int32_t mirror, int n)
{
    const int64_t s = mirror ? (int64_t)offset - (int64_t)t : (int64_t)t + (int64_t)offset;
    return s < 0 ? 0 : s > (int64_t)(n - 1) ? n - 1 : (int)s;
}

// nullptr for a (brush, map) vr_clone accepts, else what is wrong with it
inline const char* invalid(const vr_brush* b, const vr_clone_map* m)
{
    if (const char* why = brush::invalid(b)) return why;
    for (int a = 0; a < 3; ++a)
        if (m->mirror[a] != 0 && m->mirror[a] != 1) return "mirror is 0 or 1";
    if (m->reserved[0] != 0 || m->reserved[1] != 0) return "map reserved must be 0";
    return nullptr;
}

// The path rule.  The texels of the clipped box o, e read the source range [min s_a, max s_a] per axis --
// source() at the two ends of the box, since it is monotone.  When that range misses the box on at least
// one axis no texel that is read is written, and one launch may go from the planes to the planes.
inline bool direct(const vr_clone_map* m, const int o[3], const int e[3], int nx, int ny, int nz)
{
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        const int s0 = source(o[a], m->offset[a], m->mirror[a], n[a]);
        const int s1 = source(o[a] + e[a] - 1, m->offset[a], m->mirror[a], n[a]);
        const int lo = s0 < s1 ? s0 : s1, hi = s0 < s1 ? s1 : s0;
        if (hi < o[a] || lo > o[a] + e[a] - 1) return true;
    }
    return false;
}

}  // namespace clone

namespace stamp {

// nullptr for a (brush, placement) vr_stamp accepts, else what is wrong with it
inline const char* invalid(const vr_brush* b, const vr_box* p)
{
    if (const char* why = brush::invalid(b)) return why;
    if (p->bx <= 0 || p->by <= 0 || p->bz <= 0) return "stamp extent must be positive";
    return nullptr;
}

// the edited box: the brush's clipped box (brush::clip) intersected with the placement
// [x, x + bx) x [y, y + by) x [z, z + bz), the ends formed in 64 bits; false, and a zero extent, when empty
inline bool clip(const vr_brush* b, const vr_box* p, int nx, int ny, int nz, int origin[3], int extent[3])
{
    int o[3], e[3];
    bool hit = brush::clip(b, nx, ny, nz, o, e);
    const int64_t p0[3] = {p->x, p->y, p->z}, pe[3] = {p->bx, p->by, p->bz};
    int64_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int a = 0; a < 3 && hit; ++a) {
        lo[a] = o[a] > p0[a] ? (int64_t)o[a] : p0[a];
        hi[a] = (int64_t)o[a] + e[a] < p0[a] + pe[a] ? (int64_t)o[a] + e[a] : p0[a] + pe[a];   // one past the end
        if (lo[a] >= hi[a]) hit = false;
    }
    for (int a = 0; a < 3; ++a) {
        origin[a] = hit ? (int)lo[a] : 0;
        extent[a] = hit ? (int)(hi[a] - lo[a]) : 0;
    }
    return hit;
}

}  // namespace stamp
}  // namespace vr
