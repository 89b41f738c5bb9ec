// vr_brush.cpp -- vr_brush_box and vr_brush_apply: the brush of vr_paint on
// the host (include/vr.h); vr_brush_line: the dabs of a
// drag, for vr_paint_stroke (sec. 5.2.6); vr_brush_blur_apply: the box-filter
// brush of vr_blur on the host (sec. 5.2.7; the mean is vr_blur.h's);
// vr_brush_morph_apply: the erode / dilate brush of vr_morph on the host
// (sec. 5.2.9; the argument check and the extremum are vr_morph.h's);
// vr_brush_rank_apply: the median / rank-filter brush of vr_rank on the host
// (sec. 5.2.12; the argument check and the selection are vr_rank.h's);
// vr_brush_stats_host, vr_box_stats_host and vr_stats_summary: the statistics
// under a brush or in a box (sec. 5.2.8; the arithmetic is vr_stats.h's);
// vr_brush_clone_apply, vr_brush_stamp_apply and vr_stamp_box: the brushes
// whose value is a texel, on the host (sec. 5.2.10; the checks, the source
// coordinate and the edited box are vr_clone.h's); vr_brush_remap_apply,
// vr_lut_identity, vr_lut_levels, vr_lut_compose and vr_stats_lut: the
// lookup-table brush on the host and its table builders (sec. 5.2.11; the
// checks and the entries of a table are vr_remap.h's); vr_brush_stamp_affine_apply,
// vr_brush_clone_affine_apply, vr_affine_direct, vr_affine_identity and
// vr_affine_place: the transform paste on the host and its map builders
// (sec. 5.2.13; the checks, the positions and the filters are vr_affine.h's);
// vr_brush_fill_apply: the flood-fill brush of vr_fill on the host (sec.
// 5.2.14; the checks and the passable test are vr_fill.h's);
// vr_brush_warp_apply, vr_warp_reach and vr_warp_push: the liquify brush of
// vr_warp on the host and its push map (sec. 5.2.15; the checks, the reach and
// the weighted position are vr_warp.h's).
//
// Pure host code in integers: no context, no device, no HIP call.  The
// arithmetic is vr_brush.h's, which the paint kernel (vr_paint.hip) includes
// too; vr_brush_apply is its CPU statement, what vr_paint must reproduce bit
// for bit.  Every statement is one walk over the clipped box (walk), the
// brushes through paint with their own value of a texel, and what a brush reads
// of the bytes before the call is a Snapshot.  tools/brush_check.cpp compiles
// this file alone (-DVR_BRUSH_STANDALONE, which only drops the vr_last_error
// text) under the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "vr_affine.h"
#include "vr_blur.h"
#include "vr_brush.h"
#include "vr_clone.h"
#include "vr_fill.h"
#include "vr_morph.h"
#include "vr_rank.h"
#include "vr_remap.h"
#include "vr_stats.h"
#include "vr_warp.h"

#ifdef VR_BRUSH_STANDALONE
namespace {
vr_status fail(vr_status st, const char*, ...) { return st; }
}
#else
#include "vr_ctx.h"
using vrapi::fail;
#endif

namespace {

vr_status check(const char* fn, const vr_brush* b, int nx, int ny, int nz)
{
    if (!b) return fail(VR_ERR_INVALID, "%s: null argument", fn);
    if (const char* why = vr::brush::invalid(b)) return fail(VR_ERR_INVALID, "%s: %s", fn, why);
    if (nx <= 0 || ny <= 0 || nz <= 0) return fail(VR_ERR_INVALID, "%s: bad extent %dx%dx%d", fn, nx, ny, nz);
    return VR_OK;
}

// The same for a brush with a check of its own (vr_blur.h, vr_morph.h, ...): all_set = no pointer is null, and
// invalid() -- which may then read them -- is nullptr or what is wrong.
template <class Invalid>
vr_status check(const char* fn, bool all_set, Invalid invalid, int nx, int ny, int nz)
{
    if (!all_set) return fail(VR_ERR_INVALID, "%s: null argument", fn);
    if (const char* why = invalid()) return fail(VR_ERR_INVALID, "%s: %s", fn, why);
    if (nx <= 0 || ny <= 0 || nz <= 0) return fail(VR_ERR_INVALID, "%s: bad extent %dx%dx%d", fn, nx, ny, nz);
    return VR_OK;
}

// The walk of every statement below: the box o, e (a brush's clipped box or a part of it, so every offset is
// within the radius: at most 255 in magnitude) in ascending z, y, x.  rw = row(y, z) once per row that the y and z
// terms of Q leave inside the ellipsoid S = t.s, then texel(rw, x, y, z, q) for every texel of that row with its Q:
// what q > S means is the caller's rule.
template <class Row, class Texel>
void walk(const vr_brush* b, const vr::brush::Terms& t, const int o[3], const int e[3], Row row, Texel texel)
{
    for (int z = o[2]; z < o[2] + e[2]; ++z) {
        const uint64_t qz = vr::brush::axis_term((int)((int64_t)z - b->centre[2]), t.k[2]);
        for (int y = o[1]; y < o[1] + e[1]; ++y) {
            const uint64_t qyz = qz + vr::brush::axis_term((int)((int64_t)y - b->centre[1]), t.k[1]);
            if (qyz > t.s) continue;
            const auto rw = row(y, z);
            for (int x = o[0]; x < o[0] + e[0]; ++x)
                texel(rw, x, y, z, qyz + vr::brush::axis_term((int)((int64_t)x - b->centre[0]), t.k[0]));
        }
    }
}

// The brush over the box o, e of the volume, in place: the walk, a texel outside the ellipsoid left alone, and per
// channel with strength != 0 the blend of the old byte with value(c, old), where value = texel(rw, x, y, z) is
// made once per inside texel and holds by value what that texel's channels share.
template <class Row, class Texel>
void paint(const vr_brush* b, int op, const int o[3], const int e[3], uint8_t* rgba8, int nx, int ny, Row row, Texel texel)
{
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    const int falloff = b->falloff;
    const unsigned strength[4] = {b->strength[0], b->strength[1], b->strength[2], b->strength[3]};
    walk(b, t, o, e, row, [&](const auto& rw, int x, int y, int z, uint64_t q) {
        if (q > t.s) return;
        const unsigned w = vr::brush::weight(q, t.s, falloff);
        uint8_t* p = rgba8 + ((((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) + (size_t)x) * 4;
        const auto value = texel(rw, x, y, z);
        for (int c = 0; c < 4; ++c) {
            if (!strength[c]) continue;
            p[c] = (uint8_t)vr::brush::blend(op, p[c], value(c, (unsigned)p[c]), w * strength[c]);
        }
    });
}

const auto no_row = [](int, int) { return 0; };

// The bytes before the call: a copy of the box lo, ext (inside it) of an nx x ny x nz RGBA8 array, addressed by
// the array's coordinates.
struct Snapshot {
    int n[3], lo[3], ext[3];
    std::vector<uint8_t> bytes;

    Snapshot(const uint8_t* rgba8, int nx, int ny, int nz, const int lo_[3], const int ext_[3])
        : n{nx, ny, nz}, lo{lo_[0], lo_[1], lo_[2]}, ext{ext_[0], ext_[1], ext_[2]},
          bytes((size_t)ext_[0] * (size_t)ext_[1] * (size_t)ext_[2] * 4)
    {
        // byte stores may alias the members: the row length and the pointers are locals
        const size_t row_bytes = (size_t)ext_[0] * 4;
        uint8_t* dst = bytes.data();
        for (int z = 0; z < ext_[2]; ++z)
            for (int y = 0; y < ext_[1]; ++y, dst += row_bytes) {
                const uint8_t* src = rgba8 + (((size_t)(lo_[2] + z) * (size_t)ny + (size_t)(lo_[1] + y)) * (size_t)nx + (size_t)lo_[0]) * 4;
                for (size_t i = 0; i < row_bytes; ++i) dst[i] = src[i];
            }
    }
    // the copied part of the array's row (y, z): texel lo[0] first
    const uint8_t* row(int y, int z) const
    {
        return &bytes[((size_t)(z - lo[2]) * (size_t)ext[1] + (size_t)(y - lo[1])) * (size_t)ext[0] * 4];
    }
    // a texel of the array, clamped to it: inside the copy for every neighbour of a texel of a box whose halo it holds
    unsigned at(int x, int y, int z, int c) const
    {
        x = x < 0 ? 0 : x > n[0] - 1 ? n[0] - 1 : x;
        y = y < 0 ? 0 : y > n[1] - 1 ? n[1] - 1 : y;
        z = z < 0 ? 0 : z > n[2] - 1 ? n[2] - 1 : z;
        return row(y, z)[(size_t)(x - lo[0]) * 4 + (size_t)c];
    }
};

// the box o, e and its halo of h texels, inside the volume
void halo_box(const int o[3], const int e[3], int h, int nx, int ny, int nz, int lo[3], int ext[3])
{
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        lo[a] = o[a] - h < 0 ? 0 : o[a] - h;
        const int hi = o[a] + e[a] - 1 + h > n[a] - 1 ? n[a] - 1 : o[a] + e[a] - 1 + h;
        ext[a] = hi - lo[a] + 1;
    }
}

// The neighbourhood brushes (blur, morph, rank) on checked arguments: a SET brush whose value, per texel and
// channel, is f(before, x, y, z, c) of the bytes BEFORE the call.  The clipped box and its halo of h texels are
// copied first and f reads the copy, so no value sees a byte this call wrote (Jacobi).
template <class F>
vr_status neighbourhood_apply(const vr_brush* b, int h, uint8_t* rgba8, int nx, int ny, int nz, F f)
{
    int o[3], e[3], lo[3], ext[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    halo_box(o, e, h, nx, ny, nz, lo, ext);
    const Snapshot before(rgba8, nx, ny, nz, lo, ext);
    paint(b, VR_BRUSH_SET, o, e, rgba8, nx, ny, no_row, [&](int, int x, int y, int z) {
        return [f, &before, x, y, z](int c, unsigned) { return f(before, x, y, z, c); };
    });
    return VR_OK;
}

// The transform paste on checked arguments (vr_affine.h): the brush over its clipped box o, e of the volume with the
// value of a texel resampled from `src`, an RGBA8 array of n[0] x n[1] x n[2] texels.  What the box reads of it (a box
// inside the source: read_range) is copied first and every value reads the copy.  A texel outside the source is
// left alone (VR_BORDER_SKIP) or reads the clamped position.
void affine_apply(const vr_brush* b, const vr_affine* m, const int o[3], const int e[3], const uint8_t* src, const int n[3],
                  uint8_t* rgba8, int nx, int ny)
{
    int lo[3], ext[3];
    for (int a = 0; a < 3; ++a) {
        int hi;
        vr::affine::read_range(m, a, o, e, n[a], &lo[a], &hi);
        ext[a] = hi - lo[a] + 1;
    }
    const Snapshot before(src, n[0], n[1], n[2], lo, ext);
    const auto byte = [&](int x, int y, int z, int c) -> unsigned { return before.row(y, z)[(size_t)(x - lo[0]) * 4 + (size_t)c]; };
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    const bool linear = m->filter == VR_FILTER_LINEAR, skip = m->border == VR_BORDER_SKIP;
    walk(b, t, o, e, no_row, [&](int, int x, int y, int z, uint64_t q) {
        if (q > t.s) return;
        int64_t p[3];
        bool out = false;
        for (int a = 0; a < 3; ++a) {
            p[a] = vr::affine::position(m->m[a], m->origin[a], m->pivot, x, y, z);
            out = out || vr::affine::outside(p[a], n[a]);
            p[a] = vr::affine::clamp(p[a], n[a]);
        }
        if (out && skip) return;
        const unsigned w = vr::brush::weight(q, t.s, b->falloff);
        uint8_t* d = rgba8 + ((((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) + (size_t)x) * 4;
        vr::affine::Axis ax[3];
        int s[3];
        for (int a = 0; a < 3; ++a) {
            ax[a] = vr::affine::linear_weights(p[a], n[a]);
            s[a] = vr::affine::nearest(p[a]);
        }
        for (int c = 0; c < 4; ++c) {
            if (!b->strength[c]) continue;
            unsigned v;
            if (linear) {
                unsigned corner[2][2][2];
                for (int k = 0; k < 8; ++k)
                    corner[k >> 2][k >> 1 & 1][k & 1] = byte(k & 1 ? ax[0].j : ax[0].i, k & 2 ? ax[1].j : ax[1].i, k & 4 ? ax[2].j : ax[2].i, c);
                v = vr::affine::linear_value(corner, ax[0].f, ax[1].f, ax[2].f);
            } else {
                v = byte(s[0], s[1], s[2], c);
            }
            d[c] = (uint8_t)vr::brush::blend(b->op, d[c], v, w * b->strength[c]);
        }
    });
}

// The liquify brush on checked arguments (vr_warp.h): the brush over its clipped box o, e of the volume with the value of
// a texel resampled from the volume itself at the position the weight leaves between the texel's own and its affine
// one.  What the box reads (vr_warp.h read_range) is copied first and every value reads the copy (Jacobi).
void warp_apply(const vr_brush* b, const vr_affine* m, const int o[3], const int e[3], uint8_t* rgba8, const int n[3])
{
    int lo[3], ext[3];
    for (int a = 0; a < 3; ++a) {
        int hi;
        vr::warp::read_range(m, a, o, e, n[a], &lo[a], &hi);
        ext[a] = hi - lo[a] + 1;
    }
    const Snapshot before(rgba8, n[0], n[1], n[2], lo, ext);
    const auto byte = [&](int x, int y, int z, int c) -> unsigned { return before.row(y, z)[(size_t)(x - lo[0]) * 4 + (size_t)c]; };
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    const bool linear = m->filter == VR_FILTER_LINEAR, skip = m->border == VR_BORDER_SKIP;
    walk(b, t, o, e, no_row, [&](int, int x, int y, int z, uint64_t q) {
        if (q > t.s) return;
        const unsigned w = vr::brush::weight(q, t.s, b->falloff);
        const int tc[3] = {x, y, z};
        int64_t p[3];
        bool out = false;
        for (int a = 0; a < 3; ++a) {
            p[a] = vr::warp::position(tc[a], vr::warp::displacement(m->m[a], m->origin[a], m->pivot, x, y, z, tc[a]), w);
            out = out || vr::affine::outside(p[a], n[a]);
            p[a] = vr::affine::clamp(p[a], n[a]);
        }
        if (out && skip) return;
        uint8_t* d = rgba8 + ((((size_t)z * (size_t)n[1] + (size_t)y) * (size_t)n[0]) + (size_t)x) * 4;
        vr::affine::Axis ax[3];
        int s[3];
        for (int a = 0; a < 3; ++a) {
            ax[a] = vr::affine::linear_weights(p[a], n[a]);
            s[a] = vr::affine::nearest(p[a]);
        }
        for (int c = 0; c < 4; ++c) {
            if (!b->strength[c]) continue;
            unsigned v;
            if (linear) {
                unsigned corner[2][2][2];
                for (int k = 0; k < 8; ++k)
                    corner[k >> 2][k >> 1 & 1][k & 1] = byte(k & 1 ? ax[0].j : ax[0].i, k & 2 ? ax[1].j : ax[1].i, k & 4 ? ax[2].j : ax[2].i, c);
                v = vr::affine::linear_value(corner, ax[0].f, ax[1].f, ax[2].f);
            } else {
                v = byte(s[0], s[1], s[2], c);
            }
            d[c] = (uint8_t)vr::brush::blend(VR_BRUSH_SET, d[c], v, 256u * b->strength[c]);
        }
    });
}

}  // namespace

extern "C" {

// The liquify brush on the host (include/vr.h): the CPU statement of vr_warp.
vr_status vr_brush_warp_apply(const vr_brush* b, const vr_affine* m, uint8_t* rgba8, int nx, int ny, int nz)
{
    if (vr_status st = check("vr_brush_warp_apply", b && m && rgba8, [&] { return vr::warp::invalid(b, m); }, nx, ny, nz)) return st;
    int o[3], e[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    const int n[3] = {nx, ny, nz};
    warp_apply(b, m, o, e, rgba8, n);
    return VR_OK;
}

vr_status vr_warp_reach(const vr_brush* b, const vr_affine* m, int32_t reach16[3])
{
    if (!b || !m || !reach16) return fail(VR_ERR_INVALID, "vr_warp_reach: null argument");
    if (const char* why = vr::affine::invalid(b, m)) return fail(VR_ERR_INVALID, "vr_warp_reach: %s", why);
    int64_t r[3];
    vr::warp::reach(b, m, r);
    for (int a = 0; a < 3; ++a) reach16[a] = r[a] > 2147483647ll ? 2147483647 : (int32_t)r[a];
    return VR_OK;
}

vr_status vr_warp_push(const int32_t centre[3], const int32_t d16[3], int filter, int border, vr_affine* out)
{
    if (!centre || !d16 || !out) return fail(VR_ERR_INVALID, "vr_warp_push: null argument");
    if (filter != VR_FILTER_NEAREST && filter != VR_FILTER_LINEAR) return fail(VR_ERR_INVALID, "vr_warp_push: bad filter");
    if (border != VR_BORDER_CLAMP && border != VR_BORDER_SKIP) return fail(VR_ERR_INVALID, "vr_warp_push: bad border");
    if (!vr::warp::push(centre, d16, filter, border, out)) return fail(VR_ERR_INVALID, "vr_warp_push: an origin leaves the 16.16 range");
    return VR_OK;
}

// The transform paste of a HOST stamp on the host (include/vr.h): the CPU statement of vr_stamp_affine.
vr_status vr_brush_stamp_affine_apply(const vr_brush* b, const uint8_t* stamp, int sbx, int sby, int sbz, const vr_affine* m,
                                      uint8_t* rgba8, int nx, int ny, int nz)
{
    if (vr_status st = check("vr_brush_stamp_affine_apply", b && stamp && m && rgba8, [&] { return vr::affine::invalid(b, m); }, nx, ny, nz))
        return st;
    if (const char* why = vr::affine::invalid_extent(sbx, sby, sbz)) return fail(VR_ERR_INVALID, "vr_brush_stamp_affine_apply: %s", why);
    int o[3], e[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    const int n[3] = {sbx, sby, sbz};
    affine_apply(b, m, o, e, stamp, n, rgba8, nx, ny);
    return VR_OK;
}

// The transform paste of the volume's own texels on the host: the CPU statement of vr_clone_affine (Jacobi: the
// copy is taken before the first byte is written).
vr_status vr_brush_clone_affine_apply(const vr_brush* b, const vr_affine* m, uint8_t* rgba8, int nx, int ny, int nz)
{
    if (vr_status st = check("vr_brush_clone_affine_apply", b && m && rgba8, [&] { return vr::affine::invalid(b, m); }, nx, ny, nz))
        return st;
    int o[3], e[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    const int n[3] = {nx, ny, nz};
    affine_apply(b, m, o, e, rgba8, n, rgba8, nx, ny);
    return VR_OK;
}

vr_status vr_affine_direct(const vr_brush* b, const vr_affine* m, int nx, int ny, int nz, int* direct)
{
    if (vr_status st = check("vr_affine_direct", b && m && direct, [&] { return vr::affine::invalid(b, m); }, nx, ny, nz)) return st;
    int o[3], e[3];
    *direct = vr::brush::clip(b, nx, ny, nz, o, e) && vr::affine::direct(m, o, e, nx, ny, nz) ? 1 : 0;
    return VR_OK;
}

vr_status vr_affine_identity(vr_affine* out)
{
    if (!out) return fail(VR_ERR_INVALID, "vr_affine_identity: null argument");
    *out = vr_affine{};
    for (int a = 0; a < 3; ++a) out->m[a][a] = VR_AFFINE_ONE;
    return VR_OK;
}

// m = rint(inverse(forward) * 65536) by the adjugate: exact for the axis rotations and the powers of two
vr_status vr_affine_place(const double forward[9], const double src_centre[3], const int32_t dst_centre[3], int filter,
                          int border, vr_affine* out)
{
    if (!forward || !src_centre || !dst_centre || !out) return fail(VR_ERR_INVALID, "vr_affine_place: null argument");
    if (filter != VR_FILTER_NEAREST && filter != VR_FILTER_LINEAR) return fail(VR_ERR_INVALID, "vr_affine_place: bad filter");
    if (border != VR_BORDER_CLAMP && border != VR_BORDER_SKIP) return fail(VR_ERR_INVALID, "vr_affine_place: bad border");
    double big = 0.0;
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(forward[i])) return fail(VR_ERR_INVALID, "vr_affine_place: a non-finite entry");
        if (std::fabs(forward[i]) > big) big = std::fabs(forward[i]);
    }
    const double* f = forward;
    const double adj[9] = {f[4] * f[8] - f[5] * f[7], f[2] * f[7] - f[1] * f[8], f[1] * f[5] - f[2] * f[4],
                           f[5] * f[6] - f[3] * f[8], f[0] * f[8] - f[2] * f[6], f[2] * f[3] - f[0] * f[5],
                           f[3] * f[7] - f[4] * f[6], f[1] * f[6] - f[0] * f[7], f[0] * f[4] - f[1] * f[3]};
    const double det = f[0] * adj[0] + f[1] * adj[3] + f[2] * adj[6];
    if (!std::isfinite(det) || !(std::fabs(det) >= 1e-12 * big * big * big) || det == 0.0)
        return fail(VR_ERR_INVALID, "vr_affine_place: forward is singular");
    vr_affine r{};
    for (int i = 0; i < 9; ++i) {
        const double v = std::rint(adj[i] / det * (double)VR_AFFINE_ONE);
        if (!(std::fabs(v) <= (double)VR_AFFINE_MAX_COEFF))
            return fail(VR_ERR_INVALID, "vr_affine_place: a coefficient of the inverse is above 256.0 in magnitude");
        r.m[i / 3][i % 3] = (int32_t)v;
    }
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(src_centre[a])) return fail(VR_ERR_INVALID, "vr_affine_place: a non-finite entry");
        const double v = std::rint(src_centre[a] * (double)VR_AFFINE_ONE);
        if (!(std::fabs(v) <= 2147483647.0)) return fail(VR_ERR_INVALID, "vr_affine_place: src_centre leaves the 16.16 range");
        r.origin[a] = (int32_t)v;
        r.pivot[a] = dst_centre[a];
    }
    r.filter = filter;
    r.border = border;
    *out = r;
    return VR_OK;
}

vr_status vr_brush_box(const vr_brush* b, int nx, int ny, int nz, int origin[3], int extent[3])
{
    if (!origin || !extent) return fail(VR_ERR_INVALID, "vr_brush_box: null argument");
    if (vr_status st = check("vr_brush_box", b, nx, ny, nz)) return st;
    (void)vr::brush::clip(b, nx, ny, nz, origin, extent);
    return VR_OK;
}

vr_status vr_brush_apply(const vr_brush* b, uint8_t* rgba8, int nx, int ny, int nz)
{
    if (!rgba8) return fail(VR_ERR_INVALID, "vr_brush_apply: null argument");
    if (vr_status st = check("vr_brush_apply", b, nx, ny, nz)) return st;
    int o[3], e[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    const unsigned value[4] = {b->value[0], b->value[1], b->value[2], b->value[3]};
    paint(b, b->op, o, e, rgba8, nx, ny, no_row,
          [&](int, int, int, int) { return [&value](int c, unsigned) { return value[c]; }; });
    return VR_OK;
}

// The smoothing brush on the host (include/vr.h): a SET brush whose value, per texel and channel, is the box-filter
// mean of the bytes BEFORE the call.  The clipped box and its halo of half_width texels (inside the volume) are
// copied first and every sum reads the copy, so no mean sees a byte this call wrote (Jacobi).
vr_status vr_brush_blur_apply(const vr_brush* b, int half_width, uint8_t* rgba8, int nx, int ny, int nz)
{
    if (vr_status st = check("vr_brush_blur_apply", b && rgba8, [&] { return vr::blur::invalid(b, half_width); }, nx, ny, nz))
        return st;
    const int h = half_width;
    return neighbourhood_apply(b, h, rgba8, nx, ny, nz, [h](const Snapshot& before, int x, int y, int z, int c) {
        unsigned sum = 0;
        for (int dz = -h; dz <= h; ++dz)
            for (int dy = -h; dy <= h; ++dy)
                for (int dx = -h; dx <= h; ++dx) sum += before.at(x + dx, y + dy, z + dz, c);
        return vr::blur::mean(sum, h);
    });
}

// The statistics under the brush on the host (include/vr.h): vr_brush_apply's walk with vr_stats.h's sums in place
// of the blend.  *out is written only once nothing can be refused any more.
vr_status vr_brush_stats_host(const vr_brush* b, const uint8_t* rgba8, int nx, int ny, int nz, vr_volume_stats* out)
{
    if (!rgba8 || !out) return fail(VR_ERR_INVALID, "vr_brush_stats_host: null argument");
    if (vr_status st = check("vr_brush_stats_host", b, nx, ny, nz)) return st;
    *out = vr_volume_stats{};
    int o[3], e[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    const unsigned mask = vr::stats::brush_mask(b->strength);
    walk(b, t, o, e, no_row, [&](int, int x, int y, int z, uint64_t q) {
        const unsigned w = vr::stats::texel_weight(1, q, t.s, b->falloff);
        if (w) vr::stats::add_texel(out, mask, w, rgba8 + ((((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) + (size_t)x) * 4);
    });
    return VR_OK;
}

// The same over a texel box: every texel counts, with the hard edge's weight.
vr_status vr_box_stats_host(const uint8_t* rgba8, int nx, int ny, int nz, int x0, int y0, int z0, int bx, int by, int bz,
                            int channel_mask, vr_volume_stats* out)
{
    if (!rgba8 || !out) return fail(VR_ERR_INVALID, "vr_box_stats_host: null argument");
    if (nx <= 0 || ny <= 0 || nz <= 0) return fail(VR_ERR_INVALID, "vr_box_stats_host: bad extent %dx%dx%d", nx, ny, nz);
    if (bx <= 0 || by <= 0 || bz <= 0) return fail(VR_ERR_INVALID, "vr_box_stats_host: bad box extent %dx%dx%d", bx, by, bz);
    if (x0 < 0 || y0 < 0 || z0 < 0 || bx > nx - x0 || by > ny - y0 || bz > nz - z0)
        return fail(VR_ERR_INVALID, "vr_box_stats_host: box %dx%dx%d at (%d, %d, %d) leaves the %dx%dx%d volume", bx, by, bz,
                    x0, y0, z0, nx, ny, nz);
    if (const char* why = vr::stats::invalid_mask(channel_mask)) return fail(VR_ERR_INVALID, "vr_box_stats_host: %s", why);
    *out = vr_volume_stats{};
    for (int z = z0; z < z0 + bz; ++z)
        for (int y = y0; y < y0 + by; ++y) {
            const uint8_t* row = rgba8 + (((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) * 4;
            for (int x = x0; x < x0 + bx; ++x)
                vr::stats::add_texel(out, (unsigned)channel_mask, vr::stats::texel_weight(0, 0, 0, 0), row + (size_t)x * 4);
        }
    return VR_OK;
}

vr_status vr_stats_summary(const vr_volume_stats* s, vr_volume_summary* out)
{
    if (!s || !out) return fail(VR_ERR_INVALID, "vr_stats_summary: null argument");
    vr::stats::summary(s, out);
    return VR_OK;
}

// The erode / dilate brush on the host (include/vr.h): a SET brush whose value, per texel and channel, is the
// minimum / maximum over the texel's (2 half_width + 1)^3 cube of the bytes BEFORE the call.  As for the blur, the
// clipped box and its halo (inside the volume) are copied first and every extremum reads the copy (Jacobi).
vr_status vr_brush_morph_apply(const vr_brush* b, int op, int half_width, uint8_t* rgba8, int nx, int ny, int nz)
{
    if (vr_status st = check("vr_brush_morph_apply", b && rgba8, [&] { return vr::morph::invalid(b, op, half_width); }, nx, ny, nz))
        return st;
    const int h = half_width;
    // the extremum is chosen once, outside the loops: op is a constant in each instance
    const auto apply = [&](auto op_c) {
        return neighbourhood_apply(b, h, rgba8, nx, ny, nz, [h, op_c](const Snapshot& before, int x, int y, int z, int c) {
            unsigned m = before.at(x, y, z, c);
            for (int dz = -h; dz <= h; ++dz)
                for (int dy = -h; dy <= h; ++dy)
                    for (int dx = -h; dx <= h; ++dx) m = vr::morph::pick(op_c(), m, before.at(x + dx, y + dy, z + dz, c));
            return m;
        });
    };
    return op == VR_MORPH_DILATE ? apply(std::integral_constant<int, VR_MORPH_DILATE>{})
                                 : apply(std::integral_constant<int, VR_MORPH_ERODE>{});
}

// The clone brush on the host (include/vr.h): vr_brush_apply with the value of a texel read from the volume's own
// texel at the mapped, clamped position, as it was BEFORE the call.  The source range of the clipped box (a box
// inside the volume, no larger than the clipped box) is copied first and every value reads the copy (Jacobi).
vr_status vr_brush_clone_apply(const vr_brush* b, const vr_clone_map* m, uint8_t* rgba8, int nx, int ny, int nz)
{
    if (vr_status st = check("vr_brush_clone_apply", b && m && rgba8, [&] { return vr::clone::invalid(b, m); }, nx, ny, nz))
        return st;
    int o[3], e[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    const int n[3] = {nx, ny, nz};
    int lo[3], ext[3];   // what the box reads
    for (int a = 0; a < 3; ++a) {
        const int s0 = vr::clone::source(o[a], m->offset[a], m->mirror[a], n[a]);
        const int s1 = vr::clone::source(o[a] + e[a] - 1, m->offset[a], m->mirror[a], n[a]);
        lo[a] = s0 < s1 ? s0 : s1;
        ext[a] = (s0 < s1 ? s1 : s0) - lo[a] + 1;
    }
    const Snapshot before(rgba8, nx, ny, nz, lo, ext);
    const int off0 = m->offset[0], mir0 = m->mirror[0], lo0 = lo[0];
    paint(b, b->op, o, e, rgba8, nx, ny,
          [&](int y, int z) {   // the source row of the box row
              return before.row(vr::clone::source(y, m->offset[1], m->mirror[1], ny),
                                vr::clone::source(z, m->offset[2], m->mirror[2], nz));
          },
          [=](const uint8_t* srow, int x, int, int) {   // the source texel
              const uint8_t* s = srow + (size_t)(vr::clone::source(x, off0, mir0, nx) - lo0) * 4;
              return [s](int c, unsigned) -> unsigned { return s[c]; };
          });
    return VR_OK;
}

vr_status vr_stamp_box(const vr_brush* b, const vr_box* placement, int nx, int ny, int nz, int origin[3], int extent[3])
{
    if (vr_status st = check("vr_stamp_box", b && placement && origin && extent, [&] { return vr::stamp::invalid(b, placement); }, nx, ny, nz))
        return st;
    (void)vr::stamp::clip(b, placement, nx, ny, nz, origin, extent);
    return VR_OK;
}

// The stamp brush on the host (include/vr.h): vr_brush_apply over the edited box (vr_stamp_box) with the value of a
// texel read from the stamp texel that lies on it.  The part of the stamp over the edited box is copied first.
vr_status vr_brush_stamp_apply(const vr_brush* b, const uint8_t* stamp, const vr_box* placement, uint8_t* rgba8, int nx,
                               int ny, int nz)
{
    if (vr_status st = check("vr_brush_stamp_apply", b && stamp && placement && rgba8, [&] { return vr::stamp::invalid(b, placement); }, nx, ny, nz))
        return st;
    int o[3], e[3];
    if (!vr::stamp::clip(b, placement, nx, ny, nz, o, e)) return VR_OK;
    // the edited box lies inside the placement: its first texel's position in the stamp is not negative
    const int so[3] = {(int)((int64_t)o[0] - placement->x), (int)((int64_t)o[1] - placement->y),
                       (int)((int64_t)o[2] - placement->z)};
    const Snapshot copy(stamp, placement->bx, placement->by, placement->bz, so, e);
    const int o0 = o[0];
    paint(b, b->op, o, e, rgba8, nx, ny,
          [&](int y, int z) { return copy.row(so[1] + (y - o[1]), so[2] + (z - o[2])); },   // the stamp row on the box row
          [=](const uint8_t* srow, int x, int, int) {
              const uint8_t* s = srow + (size_t)(x - o0) * 4;
              return [s](int c, unsigned) -> unsigned { return s[c]; };
          });
    return VR_OK;
}

// The lookup-table brush on the host (include/vr.h): vr_brush_apply with the value of a texel read from the table at
// the texel's own old byte.  In place: a texel's new byte depends on that texel alone.
vr_status vr_brush_remap_apply(const vr_brush* b, const vr_lut* lut, uint8_t* rgba8, int nx, int ny, int nz)
{
    if (!lut || !rgba8) return fail(VR_ERR_INVALID, "vr_brush_remap_apply: null argument");
    if (vr_status st = check("vr_brush_remap_apply", b, nx, ny, nz)) return st;
    int o[3], e[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    paint(b, b->op, o, e, rgba8, nx, ny, no_row,
          [lut](int, int, int, int) { return [lut](int c, unsigned old) -> unsigned { return lut->lut[c][old]; }; });
    return VR_OK;
}

vr_status vr_lut_identity(vr_lut* out)
{
    if (!out) return fail(VR_ERR_INVALID, "vr_lut_identity: null argument");
    for (int c = 0; c < 4; ++c)
        for (int v = 0; v < 256; ++v) out->lut[c][v] = (uint8_t)v;
    return VR_OK;
}

vr_status vr_lut_levels(vr_lut* out, int channel_mask, int in_lo, int in_hi, int out_lo, int out_hi)
{
    if (!out) return fail(VR_ERR_INVALID, "vr_lut_levels: null argument");
    if (const char* why = vr::remap::invalid_mask(channel_mask)) return fail(VR_ERR_INVALID, "vr_lut_levels: %s", why);
    if (const char* why = vr::remap::invalid_levels(in_lo, in_hi, out_lo, out_hi))
        return fail(VR_ERR_INVALID, "vr_lut_levels: %s", why);
    for (int c = 0; c < 4; ++c) {
        if (!(channel_mask >> c & 1)) continue;
        for (int v = 0; v < 256; ++v) out->lut[c][v] = (uint8_t)vr::remap::levels_value(v, in_lo, in_hi, out_lo, out_hi);
    }
    return VR_OK;
}

// out may be first or then: the result is formed in a table of its own
vr_status vr_lut_compose(const vr_lut* first, const vr_lut* then, vr_lut* out)
{
    if (!first || !then || !out) return fail(VR_ERR_INVALID, "vr_lut_compose: null argument");
    vr_lut r;
    for (int c = 0; c < 4; ++c)
        for (int v = 0; v < 256; ++v) r.lut[c][v] = then->lut[c][first->lut[c][v]];
    *out = r;
    return VR_OK;
}

vr_status vr_stats_lut(const vr_volume_stats* stats, int kind, int channel_mask, vr_lut* out)
{
    if (!stats || !out) return fail(VR_ERR_INVALID, "vr_stats_lut: null argument");
    if (const char* why = vr::remap::invalid_kind(kind)) return fail(VR_ERR_INVALID, "vr_stats_lut: %s", why);
    if (const char* why = vr::remap::invalid_mask(channel_mask)) return fail(VR_ERR_INVALID, "vr_stats_lut: %s", why);
    vr::remap::stats_lut(stats, kind, (unsigned)channel_mask, out);
    return VR_OK;
}

// The median / rank-filter brush on the host (include/vr.h): a SET brush whose value, per texel and channel, is the
// rank-th smallest byte of the texel's (2 half_width + 1)^3 cube of the bytes BEFORE the call.  As for the blur and
// the morph, the clipped box and its halo (inside the volume) are copied first and every selection reads the copy
// (Jacobi); the selection is vr_rank.h's bisection, each count a plain loop over the cube.
vr_status vr_brush_rank_apply(const vr_brush* b, int rank, int half_width, uint8_t* rgba8, int nx, int ny, int nz)
{
    if (vr_status st = check("vr_brush_rank_apply", b && rgba8, [&] { return vr::rank::invalid(b, rank, half_width); }, nx, ny, nz))
        return st;
    const int h = half_width, count = vr::rank::window(h);
    const unsigned k = (unsigned)vr::rank::resolve(rank, h);
    unsigned cube[7 * 7 * 7];   // the neighbours of one texel and channel
    static_assert(VR_RANK_MAX_HALF == 3, "the cube holds the widest window");
    return neighbourhood_apply(b, h, rgba8, nx, ny, nz, [&](const Snapshot& before, int x, int y, int z, int c) {
        int i = 0;
        for (int dz = -h; dz <= h; ++dz)
            for (int dy = -h; dy <= h; ++dy)
                for (int dx = -h; dx <= h; ++dx) cube[i++] = before.at(x + dx, y + dy, z + dz, c);
        return vr::rank::select(k, [&](unsigned cand) {
            unsigned below = 0u;
            for (int j = 0; j < count; ++j) below += vr::rank::below(cube[j], cand);
            return below;
        });
    });
}

// The flood-fill brush on the host (include/vr.h): the passable mask of the clipped box from the bytes BEFORE the
// call, a breadth-first search with a queue from the seed over that mask (6-connectivity; a path never leaves the
// box's inside texels), then vr_brush_apply's blend on the texels it reached.  *report (optional) as vr_fill leaves
// it; a brush that misses the volume and a seed outside the clipped box give the empty one.
vr_status vr_brush_fill_apply(const vr_brush* b, const vr_fill_rule* rule, uint8_t* rgba8, int nx, int ny, int nz,
                              vr_fill_report* report)
{
    if (vr_status st = check("vr_brush_fill_apply", b && rule && rgba8, [&] { return vr::fill::invalid(b, rule); }, nx, ny, nz))
        return st;
    if (const char* why = vr::fill::invalid_seed(rule, nx, ny, nz)) return fail(VR_ERR_INVALID, "vr_brush_fill_apply: %s", why);
    vr_fill_report rep;
    vr::fill::empty_report(&rep, nx, ny, nz);
    int o[3], e[3];
    bool reached = vr::brush::clip(b, nx, ny, nz, o, e);
    for (int a = 0; a < 3; ++a) reached = reached && rule->seed[a] >= o[a] && rule->seed[a] - o[a] < e[a];
    if (!reached) {
        if (report) *report = rep;
        return VR_OK;
    }
    const auto texel = [&](int x, int y, int z) { return rgba8 + ((((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) + (size_t)x) * 4; };
    const auto at = [&](int x, int y, int z) { return ((size_t)(z - o[2]) * (size_t)e[1] + (size_t)(y - o[1])) * (size_t)e[0] + (size_t)(x - o[0]); };
    unsigned seed[4];
    for (int c = 0; c < 4; ++c) seed[c] = texel(rule->seed[0], rule->seed[1], rule->seed[2])[c];
    // 0: not passable, 1: passable, 2: of the region
    std::vector<uint8_t> state((size_t)e[0] * (size_t)e[1] * (size_t)e[2], 0);
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    walk(b, t, o, e, no_row, [&](int, int x, int y, int z, uint64_t q) {
        const uint8_t* p = texel(x, y, z);
        if (vr::fill::passable(*rule, seed, q <= t.s, [&](int c) -> unsigned { return p[c]; })) {
            state[at(x, y, z)] = 1;
            ++rep.passable;
        }
    });
    struct Texel { int x, y, z; };
    std::vector<Texel> queue;
    if (state[at(rule->seed[0], rule->seed[1], rule->seed[2])] == 1) {
        state[at(rule->seed[0], rule->seed[1], rule->seed[2])] = 2;
        queue.push_back(Texel{rule->seed[0], rule->seed[1], rule->seed[2]});
    }
    for (size_t head = 0; head < queue.size(); ++head) {
        const Texel cur = queue[head];
        const int p[3] = {cur.x, cur.y, cur.z};
        for (int a = 0; a < 3; ++a) {
            if (p[a] < rep.min[a]) rep.min[a] = p[a];
            if (p[a] > rep.max[a]) rep.max[a] = p[a];
            for (int d = -1; d <= 1; d += 2) {
                int n[3] = {cur.x, cur.y, cur.z};
                n[a] += d;
                if (n[a] < o[a] || n[a] - o[a] >= e[a]) continue;
                uint8_t& st = state[at(n[0], n[1], n[2])];
                if (st != 1) continue;
                st = 2;
                queue.push_back(Texel{n[0], n[1], n[2]});
            }
        }
    }
    rep.filled = queue.size();
    walk(b, t, o, e, no_row, [&](int, int x, int y, int z, uint64_t q) {
        if (q > t.s || state[at(x, y, z)] != 2) return;
        const unsigned w = vr::brush::weight(q, t.s, b->falloff);
        uint8_t* p = texel(x, y, z);
        for (int c = 0; c < 4; ++c) {
            if (!b->strength[c]) continue;
            p[c] = (uint8_t)vr::brush::blend(b->op, p[c], b->value[c], w * b->strength[c]);
        }
    });
    if (report) *report = rep;
    return VR_OK;
}

// The dabs of a drag (include/vr.h): n segments of at most `spacing` texels on the longest axis, dab i at the
// texel nearest to centre + i d / n.  |d_a| < 2^32 and i <= n <= 2^20: 2 i d_a + n stays below 2^54.
vr_status vr_brush_line(const vr_brush* b, const int32_t to[3], int spacing, int skip_first, vr_brush* out, int max_out,
                        int* out_count)
{
    if (out_count) *out_count = 0;
    if (!b || !to || !out_count) return fail(VR_ERR_INVALID, "vr_brush_line: null argument");
    if (const char* why = vr::brush::invalid(b)) return fail(VR_ERR_INVALID, "vr_brush_line: %s", why);
    if (spacing < 1) return fail(VR_ERR_INVALID, "vr_brush_line: spacing %d (at least 1)", spacing);
    if (skip_first != 0 && skip_first != 1) return fail(VR_ERR_INVALID, "vr_brush_line: skip_first %d", skip_first);
    if (max_out < 0) return fail(VR_ERR_INVALID, "vr_brush_line: max_out %d", max_out);
    if (!out && max_out > 0) return fail(VR_ERR_INVALID, "vr_brush_line: null out with max_out %d", max_out);
    int64_t d[3], longest = 0;
    for (int a = 0; a < 3; ++a) {
        d[a] = (int64_t)to[a] - b->centre[a];
        const int64_t m = d[a] < 0 ? -d[a] : d[a];
        if (m > longest) longest = m;
    }
    int64_t n = (longest + spacing - 1) / spacing;
    if (n < 1) n = 1;
    if (n > ((int64_t)1 << 20))
        return fail(VR_ERR_INVALID, "vr_brush_line: %lld segments (at most 2^20): a longer spacing, or split the drag",
                    (long long)n);
    const int64_t need = n + 1 - skip_first;
    *out_count = (int)need;
    if (need > max_out) return fail(VR_ERR_INVALID, "vr_brush_line: %lld dabs, room for %d", (long long)need, max_out);
    for (int64_t i = skip_first; i <= n; ++i) {
        vr_brush* o = out + (i - skip_first);
        *o = *b;
        for (int a = 0; a < 3; ++a) {
            const int64_t num = 2 * i * d[a] + n, den = 2 * n;
            const int64_t q = num >= 0 ? num / den : -((-num + den - 1) / den);   // floor
            o->centre[a] = (int32_t)(b->centre[a] + q);                           // between centre and to
        }
    }
    return VR_OK;
}

}  // extern "C"
