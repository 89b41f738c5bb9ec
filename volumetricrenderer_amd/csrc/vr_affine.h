// vr_affine.h -- the transform paste: vr_stamp_affine / vr_clone_affine and
// their host statements (include/vr.h), stated once:
// the argument check, the 16.16 source position of a destination texel, the
// outside test and the clamp, the nearest texel, the trilinear weights and
// their exact sum, and the rule that picks the clone's device path.  Plain
// integer C++ in the manner of vr_clone.h; vr_brush.h supplies everything else
// of the brush (inside test, weight, blend): the kernels (vr_paint.hip), the
// host statements (vr_brush.cpp) and the stand-alone check
// (tools/affine_check.cpp) include this file, so they cannot diverge.
//
// |m[a][b]| <= 2^24 and |t - pivot| < 2^32: a product stays below 2^56 and a
// position, three of them and an int32 origin, below 2^59 -- signed 64 bits.
#pragma once

#include "vr_brush.h"

namespace vr {
namespace affine {

// nullptr for a (brush, map) the affine calls accept, else what is wrong with it
inline const char* invalid(const vr_brush* b, const vr_affine* m)
{
    if (const char* why = brush::invalid(b)) return why;
    if (m->filter != VR_FILTER_NEAREST && m->filter != VR_FILTER_LINEAR) return "bad filter";
    if (m->border != VR_BORDER_CLAMP && m->border != VR_BORDER_SKIP) return "bad border";
    if (m->reserved != 0) return "map reserved must be 0";
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c)
            if (m->m[a][c] > VR_AFFINE_MAX_COEFF || m->m[a][c] < -VR_AFFINE_MAX_COEFF) return "coefficient above 256.0 in magnitude";
    return nullptr;
}

// nullptr for a source extent vr_stamp_affine accepts
inline const char* invalid_extent(int sbx, int sby, int sbz)
{
    if (sbx < 1 || sby < 1 || sbz < 1 || sbx > VR_AFFINE_MAX_EXTENT || sby > VR_AFFINE_MAX_EXTENT || sbz > VR_AFFINE_MAX_EXTENT)
        return "source extent outside 1..32768";
    return nullptr;
}

// one term of a position: the coefficient times the texel coordinate's offset from the pivot
VR_BRUSH_FN int64_t term(int32_t coeff, int t, int32_t pivot)
{
    return (int64_t)coeff * ((int64_t)t - (int64_t)pivot);
}

// P_a of the destination texel (tx, ty, tz): row = m[a], origin = origin[a]
VR_BRUSH_FN int64_t position(const int32_t row[3], int32_t origin, const int32_t pivot[3], int tx, int ty, int tz)
{
    return (int64_t)origin + term(row[0], tx, pivot[0]) + term(row[1], ty, pivot[1]) + term(row[2], tz, pivot[2]);
}

// the last position of an axis of n texels
VR_BRUSH_FN int64_t last(int n) { return (int64_t)(n - 1) << 16; }

VR_BRUSH_FN bool outside(int64_t p, int n) { return p < 0 || p > last(n); }

VR_BRUSH_FN int64_t clamp(int64_t p, int n) { return p < 0 ? 0 : p > last(n) ? last(n) : p; }

// the nearest texel of a clamped position: at most n - 1, since the last position has no fraction
VR_BRUSH_FN int nearest(int64_t p) { return (int)(p >> 16) + ((p & 0xFFFF) >= 0x8000 ? 1 : 0); }

// the two texels of a clamped position on an axis of n texels and the weight of the second (the first's is 256 - f).
// A second texel of weight 0 is the first again: the value is the same, and no texel outside read_range is touched
// -- a position clamped to 0 from below would otherwise name texel 1.
struct Axis {
    int i, j;
    unsigned f;
};
VR_BRUSH_FN Axis linear_weights(int64_t p, int n)
{
    Axis r;
    r.i = (int)(p >> 16);
    r.f = (unsigned)(p >> 8) & 255u;
    r.j = r.f == 0u || r.i + 1 > n - 1 ? r.i : r.i + 1;
    return r;
}

// The trilinear value of the corner bytes c[z][y][x] (0 = i, 1 = j): x, then y, then z, nothing rounded in between.
// The x sums are at most 255 * 2^8, the y sums 255 * 2^16, the last 255 * 2^24 + 2^23 < 2^32.
VR_BRUSH_FN unsigned linear_yz(unsigned x00, unsigned x01, unsigned x10, unsigned x11, unsigned fy, unsigned fz)
{
    const unsigned y0 = x00 * (256u - fy) + x01 * fy, y1 = x10 * (256u - fy) + x11 * fy;   // x_zy
    return (y0 * (256u - fz) + y1 * fz + (1u << 23)) >> 24;
}
VR_BRUSH_FN unsigned linear_value(const unsigned c[2][2][2], unsigned fx, unsigned fy, unsigned fz)
{
    const unsigned gx = 256u - fx;
    return linear_yz(c[0][0][0] * gx + c[0][0][1] * fx, c[0][1][0] * gx + c[0][1][1] * fx, c[1][0][0] * gx + c[1][0][1] * fx,
                     c[1][1][0] * gx + c[1][1][1] * fx, fy, fz);
}

// The texels an o, e box of destination texels reads on axis a of a source of n texels: the positions of its 8
// corners bound every position in it (P is affine in t), [lo >> 16, (hi >> 16) + 1] holds both texels of every
// LINEAR position and [(lo + 0x8000) >> 16, (hi + 0x8000) >> 16] the nearest of every NEAREST one; clamped to the
// source, as the positions are (VR_BORDER_CLAMP) or as the texels that are read at all lie (VR_BORDER_SKIP).
inline void read_range(const vr_affine* m, int a, const int o[3], const int e[3], int n, int* first, int* last_)
{
    int64_t lo = 0, hi = 0;
    for (int k = 0; k < 8; ++k) {
        const int64_t p = position(m->m[a], m->origin[a], m->pivot, k & 1 ? o[0] + e[0] - 1 : o[0], k & 2 ? o[1] + e[1] - 1 : o[1],
                                   k & 4 ? o[2] + e[2] - 1 : o[2]);
        if (k == 0 || p < lo) lo = p;
        if (k == 0 || p > hi) hi = p;
    }
    int64_t r0, r1;
    if (m->filter == VR_FILTER_LINEAR) { r0 = lo >> 16; r1 = (hi >> 16) + 1; }
    else { r0 = (lo + 0x8000) >> 16; r1 = (hi + 0x8000) >> 16; }
    *first = (int)(r0 < 0 ? 0 : r0 > n - 1 ? n - 1 : r0);
    *last_ = (int)(r1 < 0 ? 0 : r1 > n - 1 ? n - 1 : r1);
}

// The path rule of vr_clone_affine: when the read range misses the clipped box o, e on at least one axis no texel
// that is read is written, and one launch may go from the planes to the planes.
inline bool direct(const vr_affine* m, const int o[3], const int e[3], int nx, int ny, int nz)
{
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        int lo, hi;
        read_range(m, a, o, e, n[a], &lo, &hi);
        if (hi < o[a] || lo > o[a] + e[a] - 1) return true;
    }
    return false;
}

}  // namespace affine
}  // namespace vr
