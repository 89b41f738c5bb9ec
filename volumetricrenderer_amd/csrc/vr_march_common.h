// vr_march_common.h -- what the grid march (vr_march_kernels.h) and the
// procedural medium (vr_proc_kernels.h) share: the ray setup, the
// render-target store, the spec's exp, the ray epilogue, the tap coordinate,
// the lane -> pixel map of a wave tile,
// the ring tile order, the step counter and the VR_TIMELINE recorder.  No
// kernel lives here, so a translation unit compiles only the kernels of the
// headers it includes.  Everything is in an anonymous namespace, so each
// translation unit keeps its own copy.
#pragma once
#include "vr_internal.h"

namespace vr {
namespace {

constexpr int kThreads = 256;       // 4 waves

typedef float f2 __attribute__((ext_vector_type(2)));

// exp(x) for x <= 0, the fma-only polynomial of the spec.
__device__ __forceinline__ float spec_expf(float x)
{
    if (x < -80.0f) return 0.0f;
    float k = rintf(x * 1.44269504088896341f);
    float r = fmaf(k, -0.693359375f, x);
    r = fmaf(k, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = fmaf(p, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    p = fmaf(p, r * r, r);
    p = p + 1.0f;
    return p * __int_as_float(((int)k + 127) << 23);
}

// Per-ray state after ray setup (frag.glsl:36-55).
struct Ray {
    bool live;     // pixel exists (inside the target and the frame)
    int n;         // steps (frag.glsl:46); -1 = not covered
    f2 pxy;        // box-normalised ray point (frag.glsl:49-54)
    float pz;
    f2 sxy;        // step vector (frag.glsl:45, 54)
    float sz;
};

__device__ __forceinline__ Ray setup_ray(const MarchArgs& a, int x, int orow)
{
    Ray r{};
    r.n = -1;
    const bool inside = x < a.width && orow < a.out_rows;
    int y = 0;
    if (inside) {
        const int bl = orow / a.band_rows;
        y = set_band(bl, a.band_first, a.band_stride, a.band_flip) * a.band_rows + (orow - bl * a.band_rows);
    }
    r.live = inside && y < a.height;
    if (!r.live) return r;
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    const float v0 = fmaf(fy, a.py[0], fmaf(fx, a.px[0], a.o[0]));
    const float v1 = fmaf(fy, a.py[1], fmaf(fx, a.px[1], a.o[1]));
    const float v2 = fmaf(fy, a.py[2], fmaf(fx, a.px[2], a.o[2]));
    const float len = sqrtf(fmaf(v2, v2, fmaf(v1, v1, v0 * v0)));
    float d0 = v0 / len, d1 = v1 / len, d2 = v2 / len;
    // IntersectAABB, frag.glsl:18-27
    float ta0 = (a.box_min[0] - a.org[0]) / d0, tb0 = (a.box_max[0] - a.org[0]) / d0;
    float ta1 = (a.box_min[1] - a.org[1]) / d1, tb1 = (a.box_max[1] - a.org[1]) / d1;
    float ta2 = (a.box_min[2] - a.org[2]) / d2, tb2 = (a.box_max[2] - a.org[2]) / d2;
    float tn = fmaxf(fmaxf(fminf(ta0, tb0), fminf(ta1, tb1)), fminf(ta2, tb2));
    float tf = fminf(fminf(fmaxf(ta0, tb0), fmaxf(ta1, tb1)), fmaxf(ta2, tb2));
    if (!(tn <= tf)) return r;
    float pi0 = fmaf(d0, tn, a.org[0]), pi1 = fmaf(d1, tn, a.org[1]), pi2 = fmaf(d2, tn, a.org[2]);
    // coverage: the front-face fragment survives clipping (0 <= z <= w)
    const float zc = fmaf(a.r2[2], pi2, fmaf(a.r2[1], pi1, fmaf(a.r2[0], pi0, a.r2[3])));
    const float wc = fmaf(a.r3[2], pi2, fmaf(a.r3[1], pi1, fmaf(a.r3[0], pi0, a.r3[3])));
    if (!(wc > 0.0f && zc >= 0.0f && zc <= wc)) return r;
    float c0 = a.org[0], c1 = a.org[1], c2 = a.org[2];
    if (a.cam_mode) {
        // CameraPosition is not the View eye: pi is the rasterised front-face
        // point (vert.glsl:20); the fragment's ray leaves CameraPosition through
        // it (frag.glsl:36-38), and IntersectAABB runs again from there
        c0 = a.cam[0]; c1 = a.cam[1]; c2 = a.cam[2];
        const float f0 = pi0 - c0, f1 = pi1 - c1, f2 = pi2 - c2;
        const float fl = sqrtf(fmaf(f2, f2, fmaf(f1, f1, f0 * f0)));
        d0 = f0 / fl; d1 = f1 / fl; d2 = f2 / fl;
        ta0 = (a.box_min[0] - c0) / d0; tb0 = (a.box_max[0] - c0) / d0;
        ta1 = (a.box_min[1] - c1) / d1; tb1 = (a.box_max[1] - c1) / d1;
        ta2 = (a.box_min[2] - c2) / d2; tb2 = (a.box_max[2] - c2) / d2;
        tn = fmaxf(fmaxf(fminf(ta0, tb0), fminf(ta1, tb1)), fminf(ta2, tb2));
        tf = fminf(fminf(fmaxf(ta0, tb0), fmaxf(ta1, tb1)), fmaxf(ta2, tb2));
        pi0 = fmaf(d0, tn, c0); pi1 = fmaf(d1, tn, c1); pi2 = fmaf(d2, tn, c2);
    }
    const float po0 = fmaf(d0, tf, c0), po1 = fmaf(d1, tf, c1), po2 = fmaf(d2, tf, c2);
    const float e0 = po0 - pi0, e1 = po1 - pi1, e2 = po2 - pi2;
    const float dist = sqrtf(fmaf(e2, e2, fmaf(e1, e1, e0 * e0)));
    const float q = dist / a.step_size;                                   // :46
    // int(NaN) (a degenerate camera on the fragment) is undefined in GLSL: 0 here
    r.n = q >= (float)a.max_steps ? a.max_steps : q >= 0.0f ? (int)q : 0;
    r.pxy = f2{(pi0 - a.box_min[0]) / a.box_range[0], (pi1 - a.box_min[1]) / a.box_range[1]};   // :49-54
    r.pz = (pi2 - a.box_min[2]) / a.box_range[2];
    r.sxy = f2{(a.step_size * d0) / a.box_range[0], (a.step_size * d1) / a.box_range[1]};       // :45
    r.sz = (a.step_size * d2) / a.box_range[2];
    return r;
}

// Render-target store: grey g (frag.glsl:80), uncovered pixels keep the
// clear colour (0,0,0,1) (VulkanRenderPass.cpp:17-24).  Formats 3-5 store the
// R channel only (include/vr.h grey targets).
__device__ __forceinline__ void store_pixel(const MarchArgs& a, int x, int orow, bool covered, float g)
{
    int trow = orow;
    if (a.bands_in_place) {   // the band's frame row (vr.h VR_TARGET_BANDS_IN_PLACE)
        const int bl = orow / a.band_rows;
        trow = set_band(bl, a.band_first, a.band_stride, a.band_flip) * a.band_rows + (orow - bl * a.band_rows);
    }
    char* row = (char*)a.out + (long long)trow * a.pitch;
    if (a.format == 0 || a.format == 5) {
        g = covered ? g : 0.0f;
        if (a.format == 0) reinterpret_cast<float4*>(row)[x] = make_float4(g, g, g, 1.0f);
        else reinterpret_cast<float*>(row)[x] = g;
    } else {
        unsigned int q = 0;
        if (covered) {
            float c = fminf(fmaxf(g, 0.0f), 1.0f);
            if (a.format == 2 || a.format == 4)
                c = c <= 0.0031308f ? c * 12.92f : fmaf(1.055f, powf(c, 1.0f / 2.4f), -0.055f);
            q = (unsigned int)rintf(c * 255.0f);
        }
        if (a.format <= 2) reinterpret_cast<unsigned int*>(row)[x] = q | (q << 8) | (q << 16) | 0xff000000u;
        else reinterpret_cast<unsigned char*>(row)[x] = (unsigned char)q;
    }
}

// A ray's epilogue (frag.glsl:76-79): the grey of its accumulated density.  A march ends with
//     if (r.live) store_pixel(a, x, orow, r.n >= 0, ray_grey(a, acc));
// The store is not folded into a helper of its own: one more level of inlining makes the
// compiler order store_pixel's byte packing differently.
__device__ __forceinline__ float ray_grey(const MarchArgs& a, float acc)
{
    const float at = acc * a.step_size;                              // :76
    return 1.0f - spec_expf(a.density * fminf(-at, 0.0f));           // :79
}

// Tap t at ray point P: the padded texel coordinate g = fma(P, S_t, T_t) (MarchArgs.tap_S;
// DESIGN.md sec. 3.2), xy as one packed fma and z as one fmaf.  ZO (MarchArgs.zero_offsets):
// every T is the literal 0.5.  Every march forms its coordinates here, so they agree bit for
// bit.  sz, tz: tap t's z scale and offset where they are not MarchArgs' (CORNERH keeps them in
// VGPRs, vr_march_kernels.h FastCtx).
struct TapPos {
    f2 gxy;
    float gz;
};
template <bool ZO>
__device__ __forceinline__ TapPos tap_pos(const MarchArgs& a, int t, f2 pxy, float pz, float sz, float tz)
{
    const f2 T = ZO ? f2{0.5f, 0.5f} : f2{a.tap_T[t][0], a.tap_T[t][1]};
    return TapPos{__builtin_elementwise_fma(pxy, f2{a.tap_S[t][0], a.tap_S[t][1]}, T), fmaf(pz, sz, ZO ? 0.5f : tz)};
}
template <bool ZO>
__device__ __forceinline__ TapPos tap_pos(const MarchArgs& a, int t, f2 pxy, float pz)
{
    return tap_pos<ZO>(a, t, pxy, pz, a.tap_S[t][2], a.tap_T[t][2]);
}

// Lane -> pixel inside an 8x8 wave tile.  Default row-major, so each 16-lane
// TA group of a narrow load (tools/tcp_calib.hip) is an 8x2 strip; compact
// 4x4 groups were measured no better for brick5 and 15 % slower for brick8's
// u16 loads.  BRICK5's 12-byte loads are looked up per 4 lanes, and there 2x2
// pixel quads (4x4 of them per tile) are 2.6 % faster at 512^3 than 4x1 rows
// (neutral for the other layouts, 20 % slower for planar).
// COL48 with 4x1 row or 1x4 column quads instead of 2x2: config 5 0.128-0.133
// ms against 0.126-0.129 (profiles/r03/ab_col48_lanemap.txt; arm removed).
template <int LAYOUT = 0>
__device__ __forceinline__ int lane_x(int lane)
{
    if constexpr (LAYOUT == LAYOUT_BRICK5 || LAYOUT == LAYOUT_ZPAIR || LAYOUT == LAYOUT_COL48Z || is_b4_family(LAYOUT)) return ((lane >> 2) & 3) * 2 + (lane & 1);
    else return lane & 7;
}
template <int LAYOUT = 0>
__device__ __forceinline__ int lane_y(int lane)
{
    if constexpr (LAYOUT == LAYOUT_BRICK5 || LAYOUT == LAYOUT_ZPAIR || LAYOUT == LAYOUT_COL48Z || is_b4_family(LAYOUT)) return (lane >> 4) * 2 + ((lane >> 1) & 1);
    else return lane >> 3;
}

// Ring order: position k is the k-th 8x8 tile of square rings around the
// tile (cx, cy) under the projected box centre, where rays are longest.  The
// longest-running waves start first (longest-processing-time order), so no
// long wave is left to run alone at the end.  Ring r >= 1 holds 8r tiles and
// starts at position (2r-1)^2; the caller drops tiles that are off the target.
__device__ __forceinline__ bool ring_tile(int k, int cx, int cy, int* tx, int* ty)
{
    if (k == 0) { *tx = cx; *ty = cy; return true; }
    const int r = (int)((sqrtf((float)k) + 1.0f) * 0.5f);
    const int j = k - (2 * r - 1) * (2 * r - 1), side = j / (2 * r), t = j - side * 2 * r;
    if (side == 0) { *tx = cx - r + t; *ty = cy - r; }
    else if (side == 1) { *tx = cx + r; *ty = cy - r + t; }
    else if (side == 2) { *tx = cx + r - t; *ty = cy + r; }
    else { *tx = cx - r; *ty = cy + r - t; }
    return true;
}

#ifdef VR_TIMELINE
// Timing experiments only (make timeline -> libvr_tl.so, tools/timeline.py):
// per wave of a regions launch, {start, end} in s_memrealtime ticks (100 MHz),
// the wave's XCD (blockIdx % 8), its SIMD / CU / SE (HW_ID) and its executed
// lane-steps.
constexpr int kTimelineWaves = 1 << 16;
__device__ unsigned long long g_timeline[kTimelineWaves][3];
__device__ __forceinline__ void timeline_record(unsigned long long t_begin, unsigned long long steps)
{
    for (int off = 32; off > 0; off >>= 1) steps += __shfl_xor(steps, off);
    const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();
    const int wid = (int)blockIdx.x * (int)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && wid < kTimelineWaves) {
        g_timeline[wid][0] = t_begin;
        g_timeline[wid][1] = t_end;
        // HW_ID (hwreg 4): wave slot [3:0], SIMD [5:4], pipe [7:6], CU [11:8], SH [12], SE [15:13]
        const unsigned hw = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
        g_timeline[wid][2] = (steps << 24) | ((unsigned long long)((hw >> 4) & 0xfffu) << 8) | (blockIdx.x & 7);
    }
}
#endif

__device__ __forceinline__ void add_steps(const MarchArgs& a, unsigned long long cnt)
{
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(a.step_counter, cnt);
}

}  // namespace
}  // namespace vr
