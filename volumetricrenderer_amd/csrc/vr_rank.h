// vr_rank.h -- the median / rank-filter brush of vr_rank / vr_brush_rank_apply
// (include/vr.h), stated once: the argument check, the
// rank a call means, and the selection rule.  Plain integer C++ in the manner
// of vr_morph.h; vr_brush.h supplies everything else of the brush (inside
// test, weight, blend): the stage kernel (vr_paint.hip), the host statement
// (vr_brush.cpp) and the stand-alone check (tools/rank_check.cpp) include this
// file, so they cannot diverge.
//
// The neighbourhood is the (2h + 1)^3 cube, coordinates clamped to the volume,
// N = (2h + 1)^3 bytes with repetitions.  The rank-th smallest (0-based) of a
// multiset of bytes is the largest byte v with #{neighbours < v} <= rank: the
// count is monotone in v, it is 0 <= rank for v = 0, and for the answer m it
// is at most rank while for m + 1 it counts the rank-th element too.  So the
// byte is found by bisection from bit 7 down to bit 0, eight counts of
// "neighbours below a candidate", and ties need no rule.
#pragma once

#include "vr_brush.h"

namespace vr {
namespace rank {

// the neighbours of a texel: 27, 125 or 343
VR_BRUSH_FN int window(int half_width)
{
    const int w = 2 * half_width + 1;
    return w * w * w;
}

// the rank a call means: VR_RANK_MEDIAN is the middle of the window (13, 62, 171)
VR_BRUSH_FN int resolve(int rank, int half_width)
{
    return rank == VR_RANK_MEDIAN ? (window(half_width) - 1) / 2 : rank;
}

// what a neighbour byte adds to the count of a candidate
VR_BRUSH_FN unsigned below(unsigned v, unsigned cand)
{
    return v < cand ? 1u : 0u;
}

// one round of the bisection: `lo` holds the answer's bits above `bit`, `count` is the number of neighbours below
// lo | bit; the bit is kept when no more than `rank` neighbours lie below the candidate
VR_BRUSH_FN unsigned advance(unsigned lo, unsigned bit, unsigned count, unsigned rank)
{
    return count <= rank ? lo | bit : lo;
}

// the rank-th smallest byte; count_below(cand) is the number of neighbours v with below(v, cand)
template <typename CountBelow>
VR_BRUSH_FN unsigned select(unsigned rank, CountBelow count_below)
{
    unsigned lo = 0u;
    for (unsigned bit = 128u; bit != 0u; bit >>= 1) lo = advance(lo, bit, count_below(lo | bit), rank);
    return lo;
}

// nullptr for a (brush, rank, half_width) vr_rank accepts, else what is wrong with it
inline const char* invalid(const vr_brush* b, int rank, int half_width)
{
    if (const char* why = brush::invalid(b)) return why;
    if (b->op != VR_BRUSH_SET) return "brush op must be VR_BRUSH_SET";
    if (half_width < 1 || half_width > VR_RANK_MAX_HALF) return "half_width outside 1..3";
    if (rank != VR_RANK_MEDIAN && (rank < 0 || rank > window(half_width) - 1))
        return "rank outside 0..(2 half_width + 1)^3 - 1 and not VR_RANK_MEDIAN";
    return nullptr;
}

}  // namespace rank
}  // namespace vr
