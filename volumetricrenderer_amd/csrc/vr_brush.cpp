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
// checks and the entries of a table are vr_remap.h's).
//
// Pure host code in integers: no context, no device, no HIP call.  The
// arithmetic is vr_brush.h's, which the paint kernel (vr_volume.hip) includes
// too; vr_brush_apply is its CPU statement, what vr_paint must reproduce bit
// for bit.  tools/brush_check.cpp compiles this file alone
// (-DVR_BRUSH_STANDALONE, which only drops the vr_last_error text) under the
// address and undefined-behaviour sanitizers.
#include <cstdint>
#include <vector>

#include "vr_blur.h"
#include "vr_brush.h"
#include "vr_clone.h"
#include "vr_morph.h"
#include "vr_rank.h"
#include "vr_remap.h"
#include "vr_stats.h"

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

}  // namespace

extern "C" {

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
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    // inside the clipped box every offset is within the radius: at most 255 in magnitude
    for (int z = o[2]; z < o[2] + e[2]; ++z) {
        const uint64_t qz = vr::brush::axis_term((int)((int64_t)z - b->centre[2]), t.k[2]);
        for (int y = o[1]; y < o[1] + e[1]; ++y) {
            const uint64_t qyz = qz + vr::brush::axis_term((int)((int64_t)y - b->centre[1]), t.k[1]);
            if (qyz > t.s) continue;
            uint8_t* row = rgba8 + (((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) * 4;
            for (int x = o[0]; x < o[0] + e[0]; ++x) {
                const uint64_t q = qyz + vr::brush::axis_term((int)((int64_t)x - b->centre[0]), t.k[0]);
                if (q > t.s) continue;
                const unsigned w = vr::brush::weight(q, t.s, b->falloff);
                for (int c = 0; c < 4; ++c) {
                    if (!b->strength[c]) continue;
                    uint8_t* p = row + (size_t)x * 4 + c;
                    *p = (uint8_t)vr::brush::blend(b->op, *p, b->value[c], w * b->strength[c]);
                }
            }
        }
    }
    return VR_OK;
}

// The smoothing brush on the host (include/vr.h): a SET brush whose value, per texel and channel, is the box-filter
// mean of the bytes BEFORE the call.  The clipped box and its halo of half_width texels (inside the volume) are
// copied first and every sum reads the copy, so no mean sees a byte this call wrote (Jacobi).
vr_status vr_brush_blur_apply(const vr_brush* b, int half_width, uint8_t* rgba8, int nx, int ny, int nz)
{
    if (!b || !rgba8) return fail(VR_ERR_INVALID, "vr_brush_blur_apply: null argument");
    if (const char* why = vr::blur::invalid(b, half_width)) return fail(VR_ERR_INVALID, "vr_brush_blur_apply: %s", why);
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(VR_ERR_INVALID, "vr_brush_blur_apply: bad extent %dx%dx%d", nx, ny, nz);
    int o[3], e[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    const int h = half_width, n[3] = {nx, ny, nz};
    int lo[3], ext[3];   // the box and its halo, inside the volume
    for (int a = 0; a < 3; ++a) {
        lo[a] = o[a] - h < 0 ? 0 : o[a] - h;
        const int hi = o[a] + e[a] - 1 + h > n[a] - 1 ? n[a] - 1 : o[a] + e[a] - 1 + h;
        ext[a] = hi - lo[a] + 1;
    }
    std::vector<uint8_t> before((size_t)ext[0] * (size_t)ext[1] * (size_t)ext[2] * 4);
    for (int z = 0; z < ext[2]; ++z)
        for (int y = 0; y < ext[1]; ++y) {
            const uint8_t* src = rgba8 + (((size_t)(lo[2] + z) * (size_t)ny + (size_t)(lo[1] + y)) * (size_t)nx + (size_t)lo[0]) * 4;
            uint8_t* dst = &before[((size_t)z * (size_t)ext[1] + (size_t)y) * (size_t)ext[0] * 4];
            for (size_t i = 0; i < (size_t)ext[0] * 4; ++i) dst[i] = src[i];
        }
    // a texel of the volume, clamped to it: inside the copy for every neighbour of a texel of the box
    auto at = [&](int x, int y, int z, int c) -> unsigned {
        x = x < 0 ? 0 : x > nx - 1 ? nx - 1 : x;
        y = y < 0 ? 0 : y > ny - 1 ? ny - 1 : y;
        z = z < 0 ? 0 : z > nz - 1 ? nz - 1 : z;
        return before[(((size_t)(z - lo[2]) * (size_t)ext[1] + (size_t)(y - lo[1])) * (size_t)ext[0] + (size_t)(x - lo[0])) * 4 + (size_t)c];
    };
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    for (int z = o[2]; z < o[2] + e[2]; ++z) {
        const uint64_t qz = vr::brush::axis_term((int)((int64_t)z - b->centre[2]), t.k[2]);
        for (int y = o[1]; y < o[1] + e[1]; ++y) {
            const uint64_t qyz = qz + vr::brush::axis_term((int)((int64_t)y - b->centre[1]), t.k[1]);
            if (qyz > t.s) continue;
            uint8_t* row = rgba8 + (((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) * 4;
            for (int x = o[0]; x < o[0] + e[0]; ++x) {
                const uint64_t q = qyz + vr::brush::axis_term((int)((int64_t)x - b->centre[0]), t.k[0]);
                if (q > t.s) continue;
                const unsigned w = vr::brush::weight(q, t.s, b->falloff);
                for (int c = 0; c < 4; ++c) {
                    if (!b->strength[c]) continue;
                    unsigned sum = 0;
                    for (int dz = -h; dz <= h; ++dz)
                        for (int dy = -h; dy <= h; ++dy)
                            for (int dx = -h; dx <= h; ++dx) sum += at(x + dx, y + dy, z + dz, c);
                    uint8_t* p = row + (size_t)x * 4 + c;
                    *p = (uint8_t)vr::brush::blend(VR_BRUSH_SET, *p, vr::blur::mean(sum, h), w * b->strength[c]);
                }
            }
        }
    }
    return VR_OK;
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
    for (int z = o[2]; z < o[2] + e[2]; ++z) {
        const uint64_t qz = vr::brush::axis_term((int)((int64_t)z - b->centre[2]), t.k[2]);
        for (int y = o[1]; y < o[1] + e[1]; ++y) {
            const uint64_t qyz = qz + vr::brush::axis_term((int)((int64_t)y - b->centre[1]), t.k[1]);
            if (qyz > t.s) continue;
            const uint8_t* row = rgba8 + (((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) * 4;
            for (int x = o[0]; x < o[0] + e[0]; ++x) {
                const uint64_t q = qyz + vr::brush::axis_term((int)((int64_t)x - b->centre[0]), t.k[0]);
                const unsigned w = vr::stats::texel_weight(1, q, t.s, b->falloff);
                if (w) vr::stats::add_texel(out, mask, w, row + (size_t)x * 4);
            }
        }
    }
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
    if (!b || !rgba8) return fail(VR_ERR_INVALID, "vr_brush_morph_apply: null argument");
    if (const char* why = vr::morph::invalid(b, op, half_width))
        return fail(VR_ERR_INVALID, "vr_brush_morph_apply: %s", why);
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(VR_ERR_INVALID, "vr_brush_morph_apply: bad extent %dx%dx%d", nx, ny, nz);
    int o[3], e[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    const int h = half_width, n[3] = {nx, ny, nz};
    int lo[3], ext[3];   // the box and its halo, inside the volume
    for (int a = 0; a < 3; ++a) {
        lo[a] = o[a] - h < 0 ? 0 : o[a] - h;
        const int hi = o[a] + e[a] - 1 + h > n[a] - 1 ? n[a] - 1 : o[a] + e[a] - 1 + h;
        ext[a] = hi - lo[a] + 1;
    }
    std::vector<uint8_t> before((size_t)ext[0] * (size_t)ext[1] * (size_t)ext[2] * 4);
    for (int z = 0; z < ext[2]; ++z)
        for (int y = 0; y < ext[1]; ++y) {
            const uint8_t* src = rgba8 + (((size_t)(lo[2] + z) * (size_t)ny + (size_t)(lo[1] + y)) * (size_t)nx + (size_t)lo[0]) * 4;
            uint8_t* dst = &before[((size_t)z * (size_t)ext[1] + (size_t)y) * (size_t)ext[0] * 4];
            for (size_t i = 0; i < (size_t)ext[0] * 4; ++i) dst[i] = src[i];
        }
    // a texel of the volume, clamped to it: inside the copy for every neighbour of a texel of the box
    auto at = [&](int x, int y, int z, int c) -> unsigned {
        x = x < 0 ? 0 : x > nx - 1 ? nx - 1 : x;
        y = y < 0 ? 0 : y > ny - 1 ? ny - 1 : y;
        z = z < 0 ? 0 : z > nz - 1 ? nz - 1 : z;
        return before[(((size_t)(z - lo[2]) * (size_t)ext[1] + (size_t)(y - lo[1])) * (size_t)ext[0] + (size_t)(x - lo[0])) * 4 + (size_t)c];
    };
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    for (int z = o[2]; z < o[2] + e[2]; ++z) {
        const uint64_t qz = vr::brush::axis_term((int)((int64_t)z - b->centre[2]), t.k[2]);
        for (int y = o[1]; y < o[1] + e[1]; ++y) {
            const uint64_t qyz = qz + vr::brush::axis_term((int)((int64_t)y - b->centre[1]), t.k[1]);
            if (qyz > t.s) continue;
            uint8_t* row = rgba8 + (((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) * 4;
            for (int x = o[0]; x < o[0] + e[0]; ++x) {
                const uint64_t q = qyz + vr::brush::axis_term((int)((int64_t)x - b->centre[0]), t.k[0]);
                if (q > t.s) continue;
                const unsigned w = vr::brush::weight(q, t.s, b->falloff);
                for (int c = 0; c < 4; ++c) {
                    if (!b->strength[c]) continue;
                    unsigned m = at(x, y, z, c);
                    for (int dz = -h; dz <= h; ++dz)
                        for (int dy = -h; dy <= h; ++dy)
                            for (int dx = -h; dx <= h; ++dx) m = vr::morph::pick(op, m, at(x + dx, y + dy, z + dz, c));
                    uint8_t* p = row + (size_t)x * 4 + c;
                    *p = (uint8_t)vr::brush::blend(VR_BRUSH_SET, *p, m, w * b->strength[c]);
                }
            }
        }
    }
    return VR_OK;
}

// The clone brush on the host (include/vr.h): vr_brush_apply with the value of a texel read from the volume's own
// texel at the mapped, clamped position, as it was BEFORE the call.  The source range of the clipped box (a box
// inside the volume, no larger than the clipped box) is copied first and every value reads the copy (Jacobi).
vr_status vr_brush_clone_apply(const vr_brush* b, const vr_clone_map* m, uint8_t* rgba8, int nx, int ny, int nz)
{
    if (!b || !m || !rgba8) return fail(VR_ERR_INVALID, "vr_brush_clone_apply: null argument");
    if (const char* why = vr::clone::invalid(b, m)) return fail(VR_ERR_INVALID, "vr_brush_clone_apply: %s", why);
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(VR_ERR_INVALID, "vr_brush_clone_apply: bad extent %dx%dx%d", nx, ny, nz);
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
    std::vector<uint8_t> before((size_t)ext[0] * (size_t)ext[1] * (size_t)ext[2] * 4);
    for (int z = 0; z < ext[2]; ++z)
        for (int y = 0; y < ext[1]; ++y) {
            const uint8_t* src = rgba8 + (((size_t)(lo[2] + z) * (size_t)ny + (size_t)(lo[1] + y)) * (size_t)nx + (size_t)lo[0]) * 4;
            uint8_t* dst = &before[((size_t)z * (size_t)ext[1] + (size_t)y) * (size_t)ext[0] * 4];
            for (size_t i = 0; i < (size_t)ext[0] * 4; ++i) dst[i] = src[i];
        }
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    for (int z = o[2]; z < o[2] + e[2]; ++z) {
        const uint64_t qz = vr::brush::axis_term((int)((int64_t)z - b->centre[2]), t.k[2]);
        const int sz = vr::clone::source(z, m->offset[2], m->mirror[2], nz);
        for (int y = o[1]; y < o[1] + e[1]; ++y) {
            const uint64_t qyz = qz + vr::brush::axis_term((int)((int64_t)y - b->centre[1]), t.k[1]);
            if (qyz > t.s) continue;
            const int sy = vr::clone::source(y, m->offset[1], m->mirror[1], ny);
            uint8_t* row = rgba8 + (((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) * 4;
            const uint8_t* srow = &before[((size_t)(sz - lo[2]) * (size_t)ext[1] + (size_t)(sy - lo[1])) * (size_t)ext[0] * 4];
            for (int x = o[0]; x < o[0] + e[0]; ++x) {
                const uint64_t q = qyz + vr::brush::axis_term((int)((int64_t)x - b->centre[0]), t.k[0]);
                if (q > t.s) continue;
                const unsigned w = vr::brush::weight(q, t.s, b->falloff);
                const int sx = vr::clone::source(x, m->offset[0], m->mirror[0], nx);
                for (int c = 0; c < 4; ++c) {
                    if (!b->strength[c]) continue;
                    uint8_t* p = row + (size_t)x * 4 + c;
                    *p = (uint8_t)vr::brush::blend(b->op, *p, srow[(size_t)(sx - lo[0]) * 4 + (size_t)c], w * b->strength[c]);
                }
            }
        }
    }
    return VR_OK;
}

vr_status vr_stamp_box(const vr_brush* b, const vr_box* placement, int nx, int ny, int nz, int origin[3], int extent[3])
{
    if (!b || !placement || !origin || !extent) return fail(VR_ERR_INVALID, "vr_stamp_box: null argument");
    if (const char* why = vr::stamp::invalid(b, placement)) return fail(VR_ERR_INVALID, "vr_stamp_box: %s", why);
    if (nx <= 0 || ny <= 0 || nz <= 0) return fail(VR_ERR_INVALID, "vr_stamp_box: bad extent %dx%dx%d", nx, ny, nz);
    (void)vr::stamp::clip(b, placement, nx, ny, nz, origin, extent);
    return VR_OK;
}

// The stamp brush on the host (include/vr.h): vr_brush_apply over the edited box (vr_stamp_box) with the value of a
// texel read from the stamp texel that lies on it.  The part of the stamp over the edited box is copied first.
vr_status vr_brush_stamp_apply(const vr_brush* b, const uint8_t* stamp, const vr_box* placement, uint8_t* rgba8, int nx,
                               int ny, int nz)
{
    if (!b || !stamp || !placement || !rgba8) return fail(VR_ERR_INVALID, "vr_brush_stamp_apply: null argument");
    if (const char* why = vr::stamp::invalid(b, placement)) return fail(VR_ERR_INVALID, "vr_brush_stamp_apply: %s", why);
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(VR_ERR_INVALID, "vr_brush_stamp_apply: bad extent %dx%dx%d", nx, ny, nz);
    int o[3], e[3];
    if (!vr::stamp::clip(b, placement, nx, ny, nz, o, e)) return VR_OK;
    // the edited box lies inside the placement: its first texel's position in the stamp is not negative
    const size_t so[3] = {(size_t)((int64_t)o[0] - placement->x), (size_t)((int64_t)o[1] - placement->y),
                          (size_t)((int64_t)o[2] - placement->z)};
    std::vector<uint8_t> copy((size_t)e[0] * (size_t)e[1] * (size_t)e[2] * 4);
    for (int z = 0; z < e[2]; ++z)
        for (int y = 0; y < e[1]; ++y) {
            const uint8_t* src = stamp + (((so[2] + (size_t)z) * (size_t)placement->by + so[1] + (size_t)y) * (size_t)placement->bx + so[0]) * 4;
            uint8_t* dst = &copy[((size_t)z * (size_t)e[1] + (size_t)y) * (size_t)e[0] * 4];
            for (size_t i = 0; i < (size_t)e[0] * 4; ++i) dst[i] = src[i];
        }
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    for (int z = o[2]; z < o[2] + e[2]; ++z) {
        const uint64_t qz = vr::brush::axis_term((int)((int64_t)z - b->centre[2]), t.k[2]);
        for (int y = o[1]; y < o[1] + e[1]; ++y) {
            const uint64_t qyz = qz + vr::brush::axis_term((int)((int64_t)y - b->centre[1]), t.k[1]);
            if (qyz > t.s) continue;
            uint8_t* row = rgba8 + (((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) * 4;
            const uint8_t* srow = &copy[((size_t)(z - o[2]) * (size_t)e[1] + (size_t)(y - o[1])) * (size_t)e[0] * 4];
            for (int x = o[0]; x < o[0] + e[0]; ++x) {
                const uint64_t q = qyz + vr::brush::axis_term((int)((int64_t)x - b->centre[0]), t.k[0]);
                if (q > t.s) continue;
                const unsigned w = vr::brush::weight(q, t.s, b->falloff);
                for (int c = 0; c < 4; ++c) {
                    if (!b->strength[c]) continue;
                    uint8_t* p = row + (size_t)x * 4 + c;
                    *p = (uint8_t)vr::brush::blend(b->op, *p, srow[(size_t)(x - o[0]) * 4 + (size_t)c], w * b->strength[c]);
                }
            }
        }
    }
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
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    for (int z = o[2]; z < o[2] + e[2]; ++z) {
        const uint64_t qz = vr::brush::axis_term((int)((int64_t)z - b->centre[2]), t.k[2]);
        for (int y = o[1]; y < o[1] + e[1]; ++y) {
            const uint64_t qyz = qz + vr::brush::axis_term((int)((int64_t)y - b->centre[1]), t.k[1]);
            if (qyz > t.s) continue;
            uint8_t* row = rgba8 + (((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) * 4;
            for (int x = o[0]; x < o[0] + e[0]; ++x) {
                const uint64_t q = qyz + vr::brush::axis_term((int)((int64_t)x - b->centre[0]), t.k[0]);
                if (q > t.s) continue;
                const unsigned w = vr::brush::weight(q, t.s, b->falloff);
                for (int c = 0; c < 4; ++c) {
                    if (!b->strength[c]) continue;
                    uint8_t* p = row + (size_t)x * 4 + c;
                    *p = (uint8_t)vr::brush::blend(b->op, *p, lut->lut[c][*p], w * b->strength[c]);
                }
            }
        }
    }
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
    if (!b || !rgba8) return fail(VR_ERR_INVALID, "vr_brush_rank_apply: null argument");
    if (const char* why = vr::rank::invalid(b, rank, half_width))
        return fail(VR_ERR_INVALID, "vr_brush_rank_apply: %s", why);
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(VR_ERR_INVALID, "vr_brush_rank_apply: bad extent %dx%dx%d", nx, ny, nz);
    int o[3], e[3];
    if (!vr::brush::clip(b, nx, ny, nz, o, e)) return VR_OK;
    const int h = half_width, n[3] = {nx, ny, nz};
    const unsigned k = (unsigned)vr::rank::resolve(rank, h);
    int lo[3], ext[3];   // the box and its halo, inside the volume
    for (int a = 0; a < 3; ++a) {
        lo[a] = o[a] - h < 0 ? 0 : o[a] - h;
        const int hi = o[a] + e[a] - 1 + h > n[a] - 1 ? n[a] - 1 : o[a] + e[a] - 1 + h;
        ext[a] = hi - lo[a] + 1;
    }
    std::vector<uint8_t> before((size_t)ext[0] * (size_t)ext[1] * (size_t)ext[2] * 4);
    for (int z = 0; z < ext[2]; ++z)
        for (int y = 0; y < ext[1]; ++y) {
            const uint8_t* src = rgba8 + (((size_t)(lo[2] + z) * (size_t)ny + (size_t)(lo[1] + y)) * (size_t)nx + (size_t)lo[0]) * 4;
            uint8_t* dst = &before[((size_t)z * (size_t)ext[1] + (size_t)y) * (size_t)ext[0] * 4];
            for (size_t i = 0; i < (size_t)ext[0] * 4; ++i) dst[i] = src[i];
        }
    // a texel of the volume, clamped to it: inside the copy for every neighbour of a texel of the box
    auto at = [&](int x, int y, int z, int c) -> unsigned {
        x = x < 0 ? 0 : x > nx - 1 ? nx - 1 : x;
        y = y < 0 ? 0 : y > ny - 1 ? ny - 1 : y;
        z = z < 0 ? 0 : z > nz - 1 ? nz - 1 : z;
        return before[(((size_t)(z - lo[2]) * (size_t)ext[1] + (size_t)(y - lo[1])) * (size_t)ext[0] + (size_t)(x - lo[0])) * 4 + (size_t)c];
    };
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    unsigned cube[7 * 7 * 7];   // the neighbours of one texel and channel
    static_assert(VR_RANK_MAX_HALF == 3, "the cube holds the widest window");
    const int count = vr::rank::window(h);
    for (int z = o[2]; z < o[2] + e[2]; ++z) {
        const uint64_t qz = vr::brush::axis_term((int)((int64_t)z - b->centre[2]), t.k[2]);
        for (int y = o[1]; y < o[1] + e[1]; ++y) {
            const uint64_t qyz = qz + vr::brush::axis_term((int)((int64_t)y - b->centre[1]), t.k[1]);
            if (qyz > t.s) continue;
            uint8_t* row = rgba8 + (((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx) * 4;
            for (int x = o[0]; x < o[0] + e[0]; ++x) {
                const uint64_t q = qyz + vr::brush::axis_term((int)((int64_t)x - b->centre[0]), t.k[0]);
                if (q > t.s) continue;
                const unsigned w = vr::brush::weight(q, t.s, b->falloff);
                for (int c = 0; c < 4; ++c) {
                    if (!b->strength[c]) continue;
                    int i = 0;
                    for (int dz = -h; dz <= h; ++dz)
                        for (int dy = -h; dy <= h; ++dy)
                            for (int dx = -h; dx <= h; ++dx) cube[i++] = at(x + dx, y + dy, z + dz, c);
                    const unsigned m = vr::rank::select(k, [&](unsigned cand) {
                        unsigned below = 0u;
                        for (int j = 0; j < count; ++j) below += vr::rank::below(cube[j], cand);
                        return below;
                    });
                    uint8_t* p = row + (size_t)x * 4 + c;
                    *p = (uint8_t)vr::brush::blend(VR_BRUSH_SET, *p, m, w * b->strength[c]);
                }
            }
        }
    }
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
