// vr_fill.h -- the flood-fill brush of vr_fill / vr_brush_fill_apply
// (include/vr.h), stated once: the argument check, the
// range of a channel given the seed's byte, the passable test, the empty
// report, and the connected-component labelling of the device path -- find,
// union and the labelling of one 8 x 8 x 8 tile -- as templates over a small
// "how to load / atomic-min a label" policy.  Plain integer C++ in the manner
// of vr_rank.h; vr_brush.h supplies everything else of the brush (inside test,
// weight, blend): the kernels (vr_fill.hip), the host statement (vr_brush.cpp)
// and the stand-alone check (tools/fill_check.cpp, which runs the tiled
// sequence on the CPU) include this file, so they cannot diverge.
//
// Labels.  The clipped box's texels are numbered box-linearly, i = (z e_y + y)
// e_x + x < 511^3 < 2^27.  A label array L holds kNone for a texel that is not
// passable and otherwise a passable texel of the same component with L[i] <=
// i: a forest whose roots (L[i] == i) are the smallest members seen so far.
// A link only ever lowers an entry (atomic min), so every chain descends
// strictly and ends at a root; every loop below is nevertheless capped by the
// number of labels, so that a broken invariant ends as wrong bytes, never as
// a hang.
#pragma once

#include "vr_brush.h"

namespace vr {
namespace fill {

constexpr uint32_t kNone = 0xFFFFFFFFu;   // the label of a texel that is not passable
constexpr int kTile = 8;                  // the edge of a labelling tile
constexpr int kTileTexels = kTile * kTile * kTile;

// nullptr for a (brush, rule) vr_fill accepts in some volume, else what is wrong with it
inline const char* invalid(const vr_brush* b, const vr_fill_rule* r)
{
    if (const char* why = brush::invalid(b)) return why;
    if (r->relative != 0 && r->relative != 1) return "relative must be 0 or 1";
    if (r->reserved != 0) return "rule reserved must be 0";
    bool any = false;
    for (int c = 0; c < 4; ++c) {
        if (!r->select[c]) continue;
        any = true;
        if (r->relative == 0 && r->lo[c] > r->hi[c]) return "lo above hi on a selected channel";
    }
    return any ? nullptr : "no selected channel";
}

// the seed of a rule must be a texel of the volume
inline const char* invalid_seed(const vr_fill_rule* r, int nx, int ny, int nz)
{
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a)
        if (r->seed[a] < 0 || r->seed[a] >= n[a]) return "seed outside the volume";
    return nullptr;
}

// the bytes [*rlo, *rhi] a selected channel may hold, given the seed's byte of that channel
VR_BRUSH_FN void channel_range(int relative, unsigned seed, unsigned lo, unsigned hi, unsigned* rlo, unsigned* rhi)
{
    if (relative) {
        *rlo = seed > lo ? seed - lo : 0u;
        *rhi = seed + hi < 255u ? seed + hi : 255u;
    } else {
        *rlo = lo;
        *rhi = hi;
    }
}

// The test of a texel: `inside` is vr_brush.h's inside test clipped to the volume, seed[c] the seed texel's byte
// of channel c, byte(c) the texel's -- called for the selected channels only.
template <class Byte>
VR_BRUSH_FN bool passable(const vr_fill_rule& r, const unsigned seed[4], bool inside, Byte byte)
{
    if (!inside) return false;
    for (int c = 0; c < 4; ++c) {
        if (!r.select[c]) continue;
        unsigned rlo, rhi;
        channel_range(r.relative, seed[c], r.lo[c], r.hi[c], &rlo, &rhi);
        const unsigned b = byte(c);
        if (b < rlo || b > rhi) return false;
    }
    return true;
}

VR_BRUSH_FN void empty_report(vr_fill_report* rep, int nx, int ny, int nz)
{
    rep->filled = 0u;
    rep->passable = 0u;
    rep->min[0] = nx; rep->min[1] = ny; rep->min[2] = nz;
    rep->max[0] = rep->max[1] = rep->max[2] = -1;
}

// A label policy L has   uint32_t load(uint32_t i)   and   uint32_t fetch_min(uint32_t i, uint32_t v)   (the value
// before).  The root of passable texel i: the chain descends, `cap` = the number of labels bounds it.
template <class L>
VR_BRUSH_FN uint32_t find(L& lab, uint32_t i, uint32_t cap)
{
    for (uint32_t n = 0; n < cap; ++n) {
        const uint32_t p = lab.load(i);
        if (p >= i) break;   // a root (or a broken entry: stop)
        i = p;
    }
    return i;
}

// Join the components of passable texels a and b: the larger root is hung under the smaller with an atomic min.
// When the entry was no root any more -- another thread linked it meanwhile -- the min has kept the smaller of
// its parent and our root, and the join goes on between the two of them.
template <class L>
VR_BRUSH_FN void unite(L& lab, uint32_t a, uint32_t b, uint32_t cap)
{
    for (uint32_t n = 0; n < cap; ++n) {
        a = find(lab, a, cap);
        b = find(lab, b, cap);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = lab.fetch_min(a, b);
        if (old == a) return;
        a = old;
    }
}

// The labelling of one tile, over a policy for kTileTexels tile-local labels t = (lz kTile + ly) kTile + lx -- the
// order of the box-linear indices, so the smallest member is the same in both.  Three phases with a barrier (on the
// host: the end of a loop over t) between them: every t tile_init, every t tile_link, every t tile_root.
template <class L>
VR_BRUSH_FN void tile_init(L& lab, uint32_t t, bool pass)
{
    lab.store(t, pass ? t : kNone);
}

// a passable texel joins its passable neighbours at -1 on each axis inside the tile
template <class L>
VR_BRUSH_FN void tile_link(L& lab, uint32_t t)
{
    if (lab.load(t) == kNone) return;
    const uint32_t step[3] = {1u, (uint32_t)kTile, (uint32_t)(kTile * kTile)};
    for (int a = 0; a < 3; ++a) {
        if ((t / step[a]) % (uint32_t)kTile == 0u) continue;
        const uint32_t nb = t - step[a];
        if (lab.load(nb) != kNone) unite(lab, t, nb, (uint32_t)kTileTexels);
    }
}

// the tile-local label of the component's smallest member, or kNone
template <class L>
VR_BRUSH_FN uint32_t tile_root(L& lab, uint32_t t)
{
    return lab.load(t) == kNone ? kNone : find(lab, t, (uint32_t)kTileTexels);
}

// The merge of the tiles, for texel (x, y, z) of the box with extent e and box-linear labels: where the texel lies
// on its tile's low face of an axis and both it and its neighbour across that face are passable, the two join.
template <class L>
VR_BRUSH_FN void merge_texel(L& lab, const int e[3], int x, int y, int z)
{
    const int p[3] = {x, y, z};
    const uint32_t step[3] = {1u, (uint32_t)e[0], (uint32_t)e[0] * (uint32_t)e[1]};
    const uint32_t cap = step[2] * (uint32_t)e[2];
    const uint32_t i = ((uint32_t)z * (uint32_t)e[1] + (uint32_t)y) * (uint32_t)e[0] + (uint32_t)x;
    bool here = false, known = false;
    for (int a = 0; a < 3; ++a) {
        if (p[a] == 0 || p[a] % kTile != 0) continue;
        if (!known) { here = lab.load(i) != kNone; known = true; }
        if (!here) return;
        if (lab.load(i - step[a]) != kNone) unite(lab, i, i - step[a], cap);
    }
}

}  // namespace fill
}  // namespace vr
