// vr_rects_coalesce.cpp -- vr_rects_coalesce (include/vr.h): shorten a list of
// pixel rectangles to at most max_out whose union contains the list's, for the
// caller of vr_render_rects with more than VR_MAX_RECTS edits or many tiny ones.
//
// Pure host code: no context, no device, no HIP header.
// tools/rects_check.cpp compiles this file alone (-DVR_RECTS_STANDALONE, which
// only drops the vr_last_error text) under the address and undefined-behaviour
// sanitizers.
//
// Edges, sums and areas are 64-bit: x + width may reach 2^31 - 1 and an area
// 2^62.  The work is O(n^2) per merge, at most n - max_out merges.
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/vr.h"

#ifdef VR_RECTS_STANDALONE
namespace {
vr_status fail(vr_status st, const char*, ...) { return st; }
}
#else
#include "vr_ctx.h"
using vrapi::fail;
#endif

namespace {

struct Box {
    int64_t x0, y0, x1, y1;
    int64_t area() const { return (x1 - x0) * (y1 - y0); }
    bool holds(const Box& b) const { return x0 <= b.x0 && y0 <= b.y0 && b.x1 <= x1 && b.y1 <= y1; }
};

Box hull(const Box& a, const Box& b)
{
    return Box{a.x0 < b.x0 ? a.x0 : b.x0, a.y0 < b.y0 ? a.y0 : b.y0, a.x1 > b.x1 ? a.x1 : b.x1,
               a.y1 > b.y1 ? a.y1 : b.y1};
}

}  // namespace

extern "C" vr_status vr_rects_coalesce(const vr_rect* in, int count, int max_out, vr_rect* out, int* out_count)
try {
    if (count < 0) return fail(VR_ERR_INVALID, "vr_rects_coalesce: count %d", count);
    if (max_out < 1) return fail(VR_ERR_INVALID, "vr_rects_coalesce: max_out %d (at least 1)", max_out);
    if (count == 0) {
        if (out_count) *out_count = 0;
        return VR_OK;
    }
    if (!in || !out || !out_count) return fail(VR_ERR_INVALID, "vr_rects_coalesce: null argument");
    for (int i = 0; i < count; ++i) {
        const vr_rect& r = in[i];
        if (r.x < 0 || r.y < 0 || r.width < 0 || r.height < 0 || (int64_t)r.x + r.width > INT32_MAX ||
            (int64_t)r.y + r.height > INT32_MAX)
            return fail(VR_ERR_INVALID, "vr_rects_coalesce: rectangle %d, %dx%d at (%d, %d)", i, r.width, r.height, r.x,
                        r.y);
    }
    // the non-empty inputs that no other input contains, in order; of identical ones the first
    std::vector<Box> v;
    v.reserve((size_t)count);
    for (int i = 0; i < count; ++i) {
        const vr_rect& r = in[i];
        if (r.width == 0 || r.height == 0) continue;
        const Box b{r.x, r.y, (int64_t)r.x + r.width, (int64_t)r.y + r.height};
        bool held = false;
        for (const Box& k : v)
            if (k.holds(b)) {
                held = true;
                break;
            }
        if (held) continue;
        size_t n = 0;
        for (size_t k = 0; k < v.size(); ++k)   // b may contain earlier ones
            if (!b.holds(v[k])) v[n++] = v[k];
        v.resize(n);
        v.push_back(b);
    }
    while (v.size() > (size_t)max_out) {
        // the pair whose hull adds the least area beyond its two rectangles; ties: the lowest (i, j)
        size_t bi = 0, bj = 1;
        int64_t best = 0;
        bool have = false;
        for (size_t i = 0; i + 1 < v.size(); ++i) {
            const int64_t ai = v[i].area();
            for (size_t j = i + 1; j < v.size(); ++j) {
                const int64_t add = hull(v[i], v[j]).area() - ai - v[j].area();
                if (!have || add < best) {
                    have = true;
                    best = add;
                    bi = i;
                    bj = j;
                }
            }
        }
        const Box m = hull(v[bi], v[bj]);
        size_t n = 0;
        for (size_t k = 0; k < v.size(); ++k) {
            if (k == bi) v[n++] = m;
            else if (k != bj && !m.holds(v[k])) v[n++] = v[k];
        }
        v.resize(n);
    }
    for (size_t k = 0; k < v.size(); ++k)
        out[k] = vr_rect{(int32_t)v[k].x0, (int32_t)v[k].y0, (int32_t)(v[k].x1 - v[k].x0), (int32_t)(v[k].y1 - v[k].y0)};
    *out_count = (int)v.size();
    return VR_OK;
} catch (const std::bad_alloc&) {
    return fail(VR_ERR_OOM, "vr_rects_coalesce: out of host memory");
}
