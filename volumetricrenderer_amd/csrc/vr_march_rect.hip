// vr_march_rect.hip -- the scissored march of vr_render_rect (include/vr.h):
// the pixels of one rectangle of the frame, at a cost that follows the
// rectangle.
//
// One wave renders one 8x8 tile; the tiles are anchored at the rectangle's
// origin rounded down to a multiple of 8, so a pixel sits in the lane it has
// under vr_render's tilings.  The kernels are the shared device functions of
// vr_march_kernels.h (fast_prologue, march_pixel), vr_proc_kernels.h
// (march_pixel_proc, worley_table) and vr_march_common.h (add_steps,
// lane_x / lane_y) behind another tile map (rect_pixel, vr_rect_tiles.h):
// MarchArgs still describes the whole frame, so setup_ray and store_pixel
// compute frame coordinates as they do for vr_render, and a pixel's
// arithmetic is vr_render's.  A lane outside the rectangle is handed the
// pixel x = a.width: setup_ray marks it not live, and it neither stores nor
// counts.  The grid is sized from the rectangle, four waves per workgroup.
//
// vr_render_rects marches a list of rectangles in one launch (march_rects,
// march_proc_rects): the same tile anchoring per rectangle, the list by value
// in the kernel arguments (RectList), a pixel owned by the first rectangle
// that holds it.
//
// Built with -fno-slp-vectorize like vr_march.hip and vr_march_c8.hip
// (Makefile FLAGS_*), whose code generation these instantiations share.
#include "vr_march_kernels.h"
#include "vr_proc_kernels.h"
#include "vr_rect_tiles.h"

namespace vr {
namespace {

// No wave leaves before the prologue's barrier: the waves of a last, partly
// used workgroup march pixels outside the rectangle (not live).
template <int LAYOUT, int WRAP, bool EARLY>
__global__ __launch_bounds__(kThreads) void march_rect(const MarchArgs a, const RectArgs rc)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const FastCtx f = fast_prologue<LAYOUT>(a, lds);
    int x, y;
    rect_pixel<LAYOUT>(a, rc, &x, &y);
    const unsigned steps = march_pixel<LAYOUT, WRAP, EARLY>(a, f, x, y);
    if (a.step_counter) add_steps(a, steps);
}

// Procedural medium: shadow rays marched in place (any shadow_steps), the fBm
// hashing every corner (no lattice table), the Worley cells from LDS exactly
// where march_proc takes them (TABLE 1) -- no context scratch is read or written.
template <bool SHADOW, bool EARLY, int TABLE>
__global__ __launch_bounds__(kThreads) void march_proc_rect(const MarchArgs a, const RectArgs rc)
{
    extern __shared__ float4 wt_lds[];
    const float4* wt = worley_table<TABLE>(a.proc, wt_lds);
    int x, y;
    rect_pixel<0>(a, rc, &x, &y);
    const unsigned long long steps = march_pixel_proc<SHADOW, EARLY, TABLE>(a, wt, x, y);
    if (a.step_counter) add_steps(a, steps);
}

// vr_render_rects: wave t of the launch renders tile t of the list.  Its
// rectangle k (tile_begin[k] <= t < tile_begin[k + 1]) is wave-uniform and found
// with scalar loads from the kernel arguments.  A lane is live only if its
// pixel lies in rectangle k and in no rectangle j < k (ownership): a pixel that
// several rectangles cover is marched, stored and counted by the first of them
// alone.  Every other lane -- and every lane of a spare wave of the last
// workgroup -- is handed x = a.width, the not-live pixel; such a wave still
// reaches the prologue's barrier.
template <int LAYOUT>
__device__ __forceinline__ void rects_pixel(const MarchArgs& a, const RectList& rl, int* x, int* y)
{
    const int lane = threadIdx.x & 63;
    const unsigned t = __builtin_amdgcn_readfirstlane(blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6));
    const int count = rl.count;
    *x = a.width;
    *y = 0;
    if (t >= rl.tile_begin[count]) return;   // wave-uniform: a spare wave of the last workgroup
    int k = 0;
    while (k + 1 < count && t >= rl.tile_begin[k + 1]) ++k;
    const int x0 = rl.e[k][0], y0 = rl.e[k][1], x1 = rl.e[k][2], y1 = rl.e[k][3];
    const int tiles_x = ((x1 + 7) >> 3) - (x0 >> 3);
    const int tl = (int)(t - rl.tile_begin[k]);
    const int ty = tl / tiles_x, tx = tl - ty * tiles_x;
    const int px = (x0 & ~7) + tx * 8 + lane_x<LAYOUT>(lane);
    const int py = (y0 & ~7) + ty * 8 + lane_y<LAYOUT>(lane);
    bool own = px >= x0 && px < x1 && py >= y0 && py < y1;
    for (int j = 0; j < k; ++j)
        own = own && !(px >= rl.e[j][0] && px < rl.e[j][2] && py >= rl.e[j][1] && py < rl.e[j][3]);
    if (own) {
        *x = px;
        *y = py;
    }
}

template <int LAYOUT, int WRAP, bool EARLY>
__global__ __launch_bounds__(kThreads) void march_rects(const MarchArgs a, const RectList rl)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const FastCtx f = fast_prologue<LAYOUT>(a, lds);
    int x, y;
    rects_pixel<LAYOUT>(a, rl, &x, &y);
    const unsigned steps = march_pixel<LAYOUT, WRAP, EARLY>(a, f, x, y);
    if (a.step_counter) add_steps(a, steps);
}

template <bool SHADOW, bool EARLY, int TABLE>
__global__ __launch_bounds__(kThreads) void march_proc_rects(const MarchArgs a, const RectList rl)
{
    extern __shared__ float4 wt_lds[];
    const float4* wt = worley_table<TABLE>(a.proc, wt_lds);
    int x, y;
    rects_pixel<0>(a, rl, &x, &y);
    const unsigned long long steps = march_pixel_proc<SHADOW, EARLY, TABLE>(a, wt, x, y);
    if (a.step_counter) add_steps(a, steps);
}

inline dim3 rects_grid(const RectList& rl)
{
    return dim3((rl.tile_begin[rl.count] + 3u) / 4u);
}

// the grid's 2^31 limit, four waves per workgroup
inline bool rects_launchable(const RectList& rl)
{
    return rl.count >= 0 && rl.count <= kMaxRects && rl.tile_begin[rl.count] <= 0x7fffffffu;
}

}  // namespace

RectArgs rect_args(int x, int y, int width, int height)
{
    RectArgs rc{x, y, x + width, y + height, 0};
    rc.tiles_x = ((rc.x1 + 7) >> 3) - (rc.x0 >> 3);
    return rc;
}

hipError_t launch_march_rect(const MarchArgs& a, int layout, int wrap, bool early, const RectArgs& rc, hipStream_t s)
{
    if (rc.x1 <= rc.x0 || rc.y1 <= rc.y0) return hipSuccess;
    return with_rect_variant(a, layout, wrap, early, [&](auto L, auto W, auto E, size_t lds) {
        hipLaunchKernelGGL((march_rect<L, W, E>), rect_grid(rc), dim3(kThreads), lds, s, a, rc);
    });
}

// the fixed Worley geometry is also a valid runtime geometry (n = 9, pz = 83), as for march_proc
hipError_t launch_march_proc_rect(const MarchArgs& a, bool early, const RectArgs& rc, hipStream_t s)
{
    if (rc.x1 <= rc.x0 || rc.y1 <= rc.y0) return hipSuccess;
    return with_proc_variant(a, early, [&](auto S, auto E, auto T, size_t wt_bytes) {
        hipLaunchKernelGGL((march_proc_rect<S, E, T>), rect_grid(rc), dim3(kThreads), wt_bytes, s, a, rc);
    });
}

bool rect_list_add(RectList* rl, int x, int y, int width, int height)
{
    if (rl->count >= kMaxRects) return false;
    const int k = rl->count++;
    const RectArgs rc = rect_args(x, y, width, height);
    rl->e[k][0] = rc.x0; rl->e[k][1] = rc.y0; rl->e[k][2] = rc.x1; rl->e[k][3] = rc.y1;
    const unsigned long long tiles = (unsigned long long)rc.tiles_x * (unsigned)(((rc.y1 + 7) >> 3) - (rc.y0 >> 3));
    const unsigned long long end = rl->tile_begin[k] + tiles;
    rl->tile_begin[k + 1] = end > 0xffffffffull ? 0xffffffffu : (unsigned)end;   // refused by the launch
    return true;
}

hipError_t launch_march_rects(const MarchArgs& a, int layout, int wrap, bool early, const RectList& rl, hipStream_t s)
{
    if (!rects_launchable(rl)) return hipErrorInvalidValue;
    if (rl.count == 0) return hipSuccess;
    return with_rect_variant(a, layout, wrap, early, [&](auto L, auto W, auto E, size_t lds) {
        hipLaunchKernelGGL((march_rects<L, W, E>), rects_grid(rl), dim3(kThreads), lds, s, a, rl);
    });
}

hipError_t launch_march_proc_rects(const MarchArgs& a, bool early, const RectList& rl, hipStream_t s)
{
    if (!rects_launchable(rl)) return hipErrorInvalidValue;
    if (rl.count == 0) return hipSuccess;
    return with_proc_variant(a, early, [&](auto S, auto E, auto T, size_t wt_bytes) {
        hipLaunchKernelGGL((march_proc_rects<S, E, T>), rects_grid(rl), dim3(kThreads), wt_bytes, s, a, rl);
    });
}

}  // namespace vr
