// vr_boxes_coalesce.cpp -- vr_boxes_coalesce (include/vr.h): vr_rects_coalesce
// restated for texel boxes.  Shortens a list of boxes to at most max_out whose
// union contains the list's: vr_paint_stroke rebuilds the device layouts over
// the result instead of over every dab's box, or over the stroke's bounding
// box, which for a diagonal stroke is far larger than its dabs.
//
// Pure host code: no context, no device, no HIP header.
// tools/boxes_check.cpp compiles this file alone (-DVR_BOXES_STANDALONE, which
// only drops the vr_last_error text) under the address and undefined-behaviour
// sanitizers.
//
// Edges and sums are 64-bit: x + bx may reach 2^31 - 1.  A volume may reach
// 2^93, so volumes and their differences are 128-bit.  The work is O(n^2) per
// merge, at most n - max_out merges.  Lists of up to VR_MAX_DABS boxes are
// worked on in a stack buffer (vr_paint_stroke allocates nothing).
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/vr.h"

#ifdef VR_BOXES_STANDALONE
namespace {
vr_status fail(vr_status st, const char*, ...) { return st; }
}
#else
#include "vr_ctx.h"
using vrapi::fail;
#endif

namespace {

typedef __int128 vol_t;

struct Box {
    int64_t lo[3], hi[3];
    vol_t volume() const { return (vol_t)(hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]); }
    bool holds(const Box& b) const
    {
        for (int a = 0; a < 3; ++a)
            if (b.lo[a] < lo[a] || b.hi[a] > hi[a]) return false;
        return true;
    }
};

Box hull(const Box& p, const Box& q)
{
    Box h;
    for (int a = 0; a < 3; ++a) {
        h.lo[a] = p.lo[a] < q.lo[a] ? p.lo[a] : q.lo[a];
        h.hi[a] = p.hi[a] > q.hi[a] ? p.hi[a] : q.hi[a];
    }
    return h;
}

}  // namespace

extern "C" vr_status vr_boxes_coalesce(const vr_box* in, int count, int max_out, vr_box* out, int* out_count)
try {
    if (count < 0) return fail(VR_ERR_INVALID, "vr_boxes_coalesce: count %d", count);
    if (max_out < 1) return fail(VR_ERR_INVALID, "vr_boxes_coalesce: max_out %d (at least 1)", max_out);
    if (count == 0) {
        if (out_count) *out_count = 0;
        return VR_OK;
    }
    if (!in || !out || !out_count) return fail(VR_ERR_INVALID, "vr_boxes_coalesce: null argument");
    for (int i = 0; i < count; ++i) {
        const vr_box& b = in[i];
        if (b.x < 0 || b.y < 0 || b.z < 0 || b.bx < 0 || b.by < 0 || b.bz < 0 || (int64_t)b.x + b.bx > INT32_MAX ||
            (int64_t)b.y + b.by > INT32_MAX || (int64_t)b.z + b.bz > INT32_MAX)
            return fail(VR_ERR_INVALID, "vr_boxes_coalesce: box %d, %dx%dx%d at (%d, %d, %d)", i, b.bx, b.by, b.bz, b.x,
                        b.y, b.z);
    }
    Box small[VR_MAX_DABS];
    std::vector<Box> large;
    Box* v = small;
    if (count > VR_MAX_DABS) {
        large.resize((size_t)count);
        v = large.data();
    }
    // the non-empty inputs that no other input contains, in order; of identical ones the first
    size_t m = 0;
    for (int i = 0; i < count; ++i) {
        const vr_box& r = in[i];
        if (r.bx == 0 || r.by == 0 || r.bz == 0) continue;
        const Box b{{r.x, r.y, r.z}, {(int64_t)r.x + r.bx, (int64_t)r.y + r.by, (int64_t)r.z + r.bz}};
        bool held = false;
        for (size_t k = 0; k < m && !held; ++k) held = v[k].holds(b);
        if (held) continue;
        size_t n = 0;
        for (size_t k = 0; k < m; ++k)   // b may contain earlier ones
            if (!b.holds(v[k])) v[n++] = v[k];
        m = n;
        v[m++] = b;
    }
    while (m > (size_t)max_out) {
        // the pair whose hull adds the least volume beyond its two boxes; ties: the lowest (i, j)
        size_t bi = 0, bj = 1;
        vol_t best = 0;
        bool have = false;
        for (size_t i = 0; i + 1 < m; ++i) {
            const vol_t vi = v[i].volume();
            for (size_t j = i + 1; j < m; ++j) {
                const vol_t add = hull(v[i], v[j]).volume() - vi - v[j].volume();
                if (!have || add < best) {
                    have = true;
                    best = add;
                    bi = i;
                    bj = j;
                }
            }
        }
        const Box h = hull(v[bi], v[bj]);
        size_t n = 0;
        for (size_t k = 0; k < m; ++k) {
            if (k == bi) v[n++] = h;
            else if (k != bj && !h.holds(v[k])) v[n++] = v[k];
        }
        m = n;
    }
    for (size_t k = 0; k < m; ++k)
        out[k] = vr_box{(int32_t)v[k].lo[0], (int32_t)v[k].lo[1], (int32_t)v[k].lo[2], (int32_t)(v[k].hi[0] - v[k].lo[0]),
                        (int32_t)(v[k].hi[1] - v[k].lo[1]), (int32_t)(v[k].hi[2] - v[k].lo[2])};
    *out_count = (int)m;
    return VR_OK;
} catch (const std::bad_alloc&) {
    return fail(VR_ERR_OOM, "vr_boxes_coalesce: out of host memory");
}
