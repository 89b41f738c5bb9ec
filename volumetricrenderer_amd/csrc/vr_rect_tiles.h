// vr_rect_tiles.h -- the tile map of a pixel rectangle, shared by the scissored
// march (vr_march_rect.hip) and the ray query (vr_march_query.hip): one wave per
// 8x8 tile, the tiles anchored at the rectangle's origin rounded down to a
// multiple of 8, four waves per workgroup, the grid sized from the rectangle;
// and the layout x wrap x EARLY choice of a grid kernel over that map.
// Include after vr_march_kernels.h.  Everything is in an anonymous namespace, so
// each translation unit keeps its own copy.
#pragma once
#include "vr_march_kernels.h"

namespace vr {
namespace {

// The frame pixel of this lane, or (a.width, 0) outside the rectangle.
// tiles_x = 8-px tile columns the rectangle spans from its anchor.
template <int LAYOUT>
__device__ __forceinline__ void rect_pixel(const MarchArgs& a, const RectArgs& rc, int* x, int* y)
{
    const int lane = threadIdx.x & 63;
    const int t = (int)blockIdx.x * (kThreads / 64) + (int)(threadIdx.x >> 6);
    const int ty = t / rc.tiles_x, tx = t - ty * rc.tiles_x;
    const int px = (rc.x0 & ~7) + tx * 8 + lane_x<LAYOUT>(lane);
    const int py = (rc.y0 & ~7) + ty * 8 + lane_y<LAYOUT>(lane);
    const bool in = px >= rc.x0 && px < rc.x1 && py >= rc.y0 && py < rc.y1;
    *x = in ? px : a.width;
    *y = in ? py : 0;
}

inline dim3 rect_grid(const RectArgs& rc)
{
    const long long waves = (long long)rc.tiles_x * (((rc.y1 + 7) >> 3) - (rc.y0 >> 3));
    return dim3((unsigned)((waves + 3) / 4));
}

// The layout x wrap x EARLY choice of march_rect, march_rects and march_query: launch(L, W, E, LDS bytes)
template <class F>
hipError_t with_rect_variant(const MarchArgs& a, int layout, int wrap, bool early, F&& launch)
{
    return with_layout_wrap<BuiltLayouts>(layout, wrap, [&](auto L, auto W) {
        return with_bool(early, [&](auto E) {
            launch(L, W, E, march_lds_bytes<L>(a));
            return hipGetLastError();
        });
    });
}

}  // namespace
}  // namespace vr
