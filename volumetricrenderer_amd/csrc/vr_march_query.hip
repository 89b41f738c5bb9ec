// vr_march_query.hip -- the march of vr_query_rect (include/vr.h): per pixel of
// one rectangle of the frame, the ray as vr_render marches it -- entry point,
// step vector, executed steps, optical depth, the pixel's value and the first
// step at which the accumulator passes a limit.
//
// The tile map is vr_march_rect.hip's (rect_pixel, vr_rect_tiles.h): one wave
// per 8x8 tile anchored at the rectangle's origin rounded down to a multiple of
// 8, so a pixel sits in the lane it has under vr_render; four waves per
// workgroup, the grid sized from the rectangle.  MarchArgs describes the whole
// frame with no pixel buffer: nothing here calls store_pixel or add_steps.
//
// march_pixel_query and march_pixel_proc_query restate the accumulation of
// march_pixel (vr_march_kernels.h) and march_pixel_proc (vr_proc_kernels.h)
// operation for operation -- the same taps through fetch_u / blend_u / tap, the
// same product order, f.scale on CORNERH and a.scale elsewhere, the same EARLY
// break -- so under -ffp-contract=off `value` is the render's fp32 bit for bit.
// Every grid layout runs the simple loop of the planar / corner path: what a
// tap fetches does not depend on when it is fetched, so the bricked layouts'
// prefetch pipeline changes no value.  The one addition per step is a compare
// of the accumulator in hand against QueryArgs.limit.
//
// A lane writes its record as four 16-byte stores; a lane outside the rectangle,
// or in a spare wave of the last workgroup, writes nothing and still reaches
// the prologue's barrier.
//
// Built with -fno-slp-vectorize like vr_march_rect.hip (Makefile FLAGS_*).
#include "vr_march_kernels.h"
#include "vr_proc_kernels.h"
#include "vr_rect_tiles.h"

namespace vr {
namespace {

// One vr_ray_record (64 bytes, include/vr.h) of the pixel (x, y) of the rectangle.
struct RayOut {
    int steps, hit_step;
    float value, optical_depth;
    float entry[3], step[3], hit[3];
};

__device__ __forceinline__ void store_record(const RectArgs& rc, const QueryArgs& q, int x, int y, const RayOut& o)
{
    uint4* p = reinterpret_cast<uint4*>(q.rec) + ((long long)(y - rc.y0) * q.pitch + (x - rc.x0)) * 4;
    p[0] = make_uint4((unsigned)o.steps, (unsigned)o.hit_step, __float_as_uint(o.value), __float_as_uint(o.optical_depth));
    p[1] = make_uint4(__float_as_uint(o.entry[0]), __float_as_uint(o.entry[1]), __float_as_uint(o.entry[2]), 0u);
    p[2] = make_uint4(__float_as_uint(o.step[0]), __float_as_uint(o.step[1]), __float_as_uint(o.step[2]), 0u);
    p[3] = make_uint4(__float_as_uint(o.hit[0]), __float_as_uint(o.hit[1]), __float_as_uint(o.hit[2]), 0u);
}

// The record of a ray after its march: i executed steps, accumulator-derived
// `value` and `at`, the hit (step h at point (hxy, hz)) or h = -1.  A pixel the
// box does not cover (r.n < 0) gets the background and zeros.
__device__ __forceinline__ RayOut ray_record(const Ray& r, int i, float value, float at, int h, f2 hxy, float hz)
{
    RayOut o{};
    o.steps = -1;
    o.hit_step = -1;
    if (r.n < 0) return o;   // value 0: what store_pixel writes there in VR_FMT_R32F
    o.steps = i;
    o.value = value;
    o.optical_depth = at;
    o.entry[0] = r.pxy.x; o.entry[1] = r.pxy.y; o.entry[2] = r.pz;
    o.step[0] = r.sxy.x; o.step[1] = r.sxy.y; o.step[2] = r.sz;
    if (h >= 0) {
        o.hit_step = h;
        o.hit[0] = hxy.x; o.hit[1] = hxy.y; o.hit[2] = hz;
    }
    return o;
}

// One ray of the grid path: march_pixel's setup, loop (frag.glsl:57-75) and
// epilogue (:76-79) with the record in place of the store.
template <int LAYOUT, int WRAP, bool EARLY>
__device__ __forceinline__ void march_pixel_query(const MarchArgs& a, const FastCtx& f, const RectArgs& rc,
                                                  const QueryArgs& q, int x, int y)
{
    const Ray r = setup_ray(a, x, y);
    const float uv[4] = {};
    f2 pxy = r.pxy;
    float pz = r.pz;
    float acc = 0.0f;
    int i = 0, h = -1;
    f2 hxy = f2{0.0f, 0.0f};
    float hz = 0.0f;
    for (; i < r.n; ++i) {
        float t0, t1, t2, t3;
        if constexpr (LAYOUT != LAYOUT_PLANAR) {
            t0 = blend_u<0, 0, LAYOUT>(fetch_u<0, 0, LAYOUT, false>(a, f, pxy, pz), uv);
            t1 = blend_u<0, 1, LAYOUT>(fetch_u<0, 1, LAYOUT, false>(a, f, pxy, pz), uv);
            t2 = blend_u<0, 2, LAYOUT>(fetch_u<0, 2, LAYOUT, false>(a, f, pxy, pz), uv);
            t3 = blend_u<0, 3, LAYOUT>(fetch_u<0, 3, LAYOUT, false>(a, f, pxy, pz), uv);
        } else {
            t0 = tap<LAYOUT, WRAP>(a, f, 0, pxy, pz);
            t1 = tap<LAYOUT, WRAP>(a, f, 1, pxy, pz);
            t2 = tap<LAYOUT, WRAP>(a, f, 2, pxy, pz);
            t3 = tap<LAYOUT, WRAP>(a, f, 3, pxy, pz);
        }
        acc = acc + ((t0 * t1) * (t2 + t3)) * (LAYOUT == LAYOUT_CORNERH ? f.scale : a.scale);   // :71-73
        if (h < 0 && acc > q.limit) {   // the first step whose accumulator passes the limit, at its sample point
            h = i;
            hxy = pxy;
            hz = pz;
        }
        pxy = pxy + r.sxy;                                                            // :74
        pz = pz + r.sz;
        if constexpr (EARLY) {
            if (acc > a.acc_limit) { ++i; break; }
        }
    }
    if (x < a.width) {   // inside the rectangle (rect_pixel), so inside the frame
        const float at = acc * a.step_size;                                          // :76
        const float g = 1.0f - spec_expf(a.density * fminf(-at, 0.0f));              // :79
        store_record(rc, q, x, y, ray_record(r, i, g, at, h, hxy, hz));
    }
}

// One ray of the procedural medium: march_pixel_proc's loop with the shadow
// rays marched in place; the limit is compared with the VIEW ray's accumulator.
template <bool SHADOW, bool EARLY, int TABLE>
__device__ __forceinline__ void march_pixel_proc_query(const MarchArgs& a, const float4* wt, const RectArgs& rc,
                                                       const QueryArgs& q, int x, int y)
{
    const Ray r = setup_ray(a, x, y);
    const ProcParams& p = a.proc;
    float P0 = r.pxy.x, P1 = r.pxy.y, P2 = r.pz;
    float acc = 0.0f, rad = 0.0f, tv = 1.0f;
    int i = 0, h = -1;
    f2 hxy = f2{0.0f, 0.0f};
    float hz = 0.0f;
    unsigned cells = 0;
    const DensityK dk = density_k<TABLE>(p, a.scale);
    for (; i < r.n; ++i) {
        const float rho = proc_density<TABLE, false, true>(p, dk, wt, P0, P1, P2, cells);
        if constexpr (SHADOW) {
            if (rho > 0.0f) {
                float q0 = P0, q1 = P1, q2 = P2, sl = 0.0f;
                for (int j = 0; j < p.shadow_steps; ++j) {
                    q0 = q0 + p.lstep[0]; q1 = q1 + p.lstep[1]; q2 = q2 + p.lstep[2];
                    if (q0 >= 0.0f && q0 <= 1.0f && q1 >= 0.0f && q1 <= 1.0f && q2 >= 0.0f && q2 <= 1.0f)
                        sl = sl + proc_density<TABLE>(p, dk, wt, q0, q1, q2, cells);
                }
                const float tl = spec_expf(-(sl * p.od));
                rad = fmaf((tv * (rho * p.od)), tl, rad);
            }
        }
        acc = acc + rho;
        if constexpr (SHADOW) tv = spec_expf(-(acc * p.od));
        if (h < 0 && acc > q.limit) {
            h = i;
            hxy = f2{P0, P1};
            hz = P2;
        }
        P0 = P0 + r.sxy.x; P1 = P1 + r.sxy.y; P2 = P2 + r.sz;
        if constexpr (EARLY) {
            if (acc > a.acc_limit) { ++i; break; }
        }
    }
    if (x < a.width)
        store_record(rc, q, x, y, ray_record(r, i, proc_epilogue<SHADOW>(a, acc, rad), acc * a.step_size, h, hxy, hz));
}

// No wave leaves before the prologue's barrier (march_rect).
template <int LAYOUT, int WRAP, bool EARLY>
__global__ __launch_bounds__(kThreads) void march_query(const MarchArgs a, const RectArgs rc, const QueryArgs q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const FastCtx f = fast_prologue<LAYOUT>(a, lds);
    int x, y;
    rect_pixel<LAYOUT>(a, rc, &x, &y);
    march_pixel_query<LAYOUT, WRAP, EARLY>(a, f, rc, q, x, y);
}

// The Worley cells from LDS exactly where march_proc_rect takes them (TABLE 1), the fBm
// hashing every corner: no context scratch is read or written.
template <bool SHADOW, bool EARLY, int TABLE>
__global__ __launch_bounds__(kThreads) void march_proc_query(const MarchArgs a, const RectArgs rc, const QueryArgs q)
{
    extern __shared__ float4 wt_lds[];
    const float4* wt = worley_table<TABLE>(a.proc, wt_lds);
    int x, y;
    rect_pixel<0>(a, rc, &x, &y);
    march_pixel_proc_query<SHADOW, EARLY, TABLE>(a, wt, rc, q, x, y);
}

}  // namespace

hipError_t launch_march_query(const MarchArgs& a, int layout, int wrap, bool early, const RectArgs& rc, const QueryArgs& q,
                              hipStream_t s)
{
    if (rc.x1 <= rc.x0 || rc.y1 <= rc.y0) return hipSuccess;
    return with_rect_variant(a, layout, wrap, early, [&](auto L, auto W, auto E, size_t lds) {
        hipLaunchKernelGGL((march_query<L, W, E>), rect_grid(rc), dim3(kThreads), lds, s, a, rc, q);
    });
}

hipError_t launch_march_proc_query(const MarchArgs& a, bool early, const RectArgs& rc, const QueryArgs& q, hipStream_t s)
{
    if (rc.x1 <= rc.x0 || rc.y1 <= rc.y0) return hipSuccess;
    return with_proc_variant(a, early, [&](auto S, auto E, auto T, size_t wt_bytes) {
        hipLaunchKernelGGL((march_proc_query<S, E, T>), rect_grid(rc), dim3(kThreads), wt_bytes, s, a, rc, q);
    });
}

}  // namespace vr
