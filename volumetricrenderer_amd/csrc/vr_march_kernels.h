// vr_march_kernels.h -- device code of the grid march: the tap and blend
// helpers, the per-pixel march for the grid layouts, and the kernels with
// their templated launchers launch_lw and launch_frames_l.  Included by
// vr_march.hip (all launchers), vr_march_c8.hip (the CORNER8 / CORNERH
// launchers, a unit of their own), vr_march_slab.hip and
// vr_march_rect.hip.  The procedural medium is vr_proc_kernels.h; the ray
// setup, the store and the other parts both use are vr_march_common.h.
// Everything is in an anonymous namespace, so each translation unit keeps its
// own copy.
#pragma once
#include "vr_march_common.h"
#include "vr_noise.h"

namespace vr {
namespace {

constexpr int kTile = 16;           // static schedule: workgroup tile edge, pixels

__device__ __forceinline__ float lerp_(float a, float b, float t) { return fmaf(t, b - a, a); }
__device__ __forceinline__ f2 lerp2(f2 a, f2 b, f2 t) { return __builtin_elementwise_fma(t, b - a, a); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// floor(x) as int in one instruction, and x - floor(x) clamped below 1.0
// (v_fract_f32).  The spec defines the tap weight as
// fminf(g - floorf(g), 0x1.fffffep-1f), which is what v_fract_f32 returns.
__device__ __forceinline__ int cvt_flr(float x)
{
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ float fract_(float x) { return __builtin_amdgcn_fractf(x); }

// byte k of a dword as float: one v_cvt_f32_ubyteK.  Opaque on purpose: given
// (float)hi - (float)lo of two bytes, hipcc otherwise subtracts in packed
// int16 and converts the difference, which costs more instructions.
template <int K>
__device__ __forceinline__ float ubyte(unsigned v)
{
    float r;
    if constexpr (K == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(r) : "v"(v));
    else if constexpr (K == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(r) : "v"(v));
    else if constexpr (K == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(r) : "v"(v));
    else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

// VK_SAMPLER_ADDRESS_MODE_MIRRORED_REPEAT on an integer texel index
// (VulkanCore.cpp:683-685; Vulkan spec "Texel coordinate wrapping").
__device__ __forceinline__ int mirror_(int i, int n)
{
    int two = n + n;
    int m = i % two;
    m = m < 0 ? m + two : m;
    return m < n ? m : two - 1 - m;
}

// Trilinear blend of the 8 footprint texels, two lerps per packed op:
// x-lerps of (y0,z0|y0,z1) and (y1,z0|y1,z1), then y, then z.  Each element
// is the spec's fma(t, b - a, a), in the spec's order.
__device__ __forceinline__ float blend(f2 lo_a, f2 hi_a, f2 lo_b, f2 hi_b, float wx, float wy, float wz)
{
    const f2 xa = lerp2(lo_a, hi_a, f2{wx, wx});   // {x00, x01}
    const f2 xb = lerp2(lo_b, hi_b, f2{wx, wx});   // {x10, x11}
    const f2 y = lerp2(xa, xb, f2{wy, wy});        // {y0, y1}
    return lerp_(y.x, y.y, wz) * (1.0f / 255.0f);
}

// Per-launch state of a fast-layout tap: the channel's buffer descriptor and
// the LDS offset tables TX | TY | TZ (vr_internal.h Layout).
struct FastCtx {
    __amdgpu_buffer_rsrc_t rsrc[4];
    const unsigned* tx;
    const unsigned* ty;
    const unsigned* tz;
    const unsigned* tx3;   // COL48Z: channel 3's ZPAIR offset tables (a second set in LDS)
    const unsigned* ty3;
    const unsigned* tz3;
    float s1x16, s2x16;   // CORNERH: 16 (nx+1), 16 (nx+1)(ny+1) (byte strides of y, z)
    // CORNERH: the z tap constants and the sample scale pinned to VGPRs (an fp32
    // op reading an SGPR issues at ~4.1 instead of ~2.2 cycles, sec. 5.5)
    float sz[4], oz[4], scale;
};

// x-lerp of one CORNERH footprint row: fma(w, b - a, a) with the f16 pair
// {a, b - a} of dword q (a low, b - a high), converted exactly inside the
// one v_fma_mix_f32.  Equal to the spec's fmaf(w, b - a, a) bit for bit.
__device__ __forceinline__ float mix_lerp(float w, unsigned q)
{
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %2 op_sel:[0,1,0] op_sel_hi:[0,1,1]" : "=v"(r) : "v"(w), "v"(q));
    return r;
}

// A fast-layout tap in two parts: fetch (issue the loads, keep the weights)
// and blend.  The pipelined march issues step i+1's fetches before blending
// step i, so each wave keeps two steps of loads in flight.
struct TapRaw {
    unsigned q0, q1, q2, q3;
    float wx, wy, wz;
};
template <int LAYOUT>
__device__ __forceinline__ TapRaw tap_fetch(const FastCtx& f, int ch, float gx, float gy, float gz)
{
    TapRaw r{};
    if constexpr (LAYOUT == LAYOUT_CORNERH) {
        // floor(g) in fp32 and the weight g - floor(g): exact and equal to
        // v_fract_f32 because g >= 0 here (clamp_is_exact); the byte offset
        // 16 (a + (nx+1) b + (nx+1)(ny+1) c) is an integer below 2^28 with at
        // most 24 significant bits, so both fmas are exact
        const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
        r.wx = gx - fx; r.wy = gy - fy; r.wz = gz - fz;
        const unsigned off = (unsigned)fmaf(fz, f.s2x16, fmaf(fy, f.s1x16, fx * 16.0f));
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(f.rsrc[ch], off, 0, 0);
        r.q0 = v[0]; r.q1 = v[1]; r.q2 = v[2]; r.q3 = v[3];
        return r;
    }
    r.wx = fract_(gx); r.wy = fract_(gy); r.wz = fract_(gz);
    const unsigned off = f.tx[cvt_flr(gx)] + f.ty[cvt_flr(gy)] + f.tz[cvt_flr(gz)];
    if constexpr (LAYOUT == LAYOUT_CORNER8) {
        r.q0 = __builtin_amdgcn_raw_buffer_load_b32(f.rsrc[ch], off, 0, 0);
        r.q1 = __builtin_amdgcn_raw_buffer_load_b32(f.rsrc[ch], off + 4, 0, 0);
    } else if constexpr (LAYOUT == LAYOUT_BRICK5) {
        // R = 5: one load per z-slice, bytes off..off+6 (c000 c100 . . . c010
        // c110) and the same 25 bytes on.  Each is a dword-ALIGNED 12-byte
        // load from off & ~3 and two v_alignbyte_b32 that shift the slice
        // down by off & 3: an 8-byte load at a byte-granular offset costs
        // the L1 twice the tag lookups of a dword-aligned one, and a 12-byte
        // one costs the same as 8 bytes (tools/tcp_calib.hip, DESIGN.md
        // sec. 5.1): 0.264 -> 0.225 ms at 512^3, 0.195 -> 0.122 ms at 256^3.
        // Narrow row loads (4 x u16 or u32 per tap) were 20 % slower than the
        // byte-offset 8-byte loads: more instructions, more lookups.
        const unsigned o1 = off + 25;
        const auto s0 = __builtin_amdgcn_raw_buffer_load_b96(f.rsrc[ch], off & ~3u, 0, 0);
        const auto s1 = __builtin_amdgcn_raw_buffer_load_b96(f.rsrc[ch], o1 & ~3u, 0, 0);
        r.q0 = __builtin_amdgcn_alignbyte(s0[1], s0[0], off);
        r.q1 = __builtin_amdgcn_alignbyte(s0[2], s0[1], off);
        r.q2 = __builtin_amdgcn_alignbyte(s1[1], s1[0], o1);
        r.q3 = __builtin_amdgcn_alignbyte(s1[2], s1[1], o1);
    } else if constexpr (is_b4_family(LAYOUT)) {
        // R = 4: a slice's rows y and y+1 are the two dwords at off & ~3
        // (x = off & 3 <= 2), so one dword-aligned 8-byte load per z-slice,
        // the z+1 slice 16 bytes on (32 for BRICK488's 8-row slices): 2
        // dwords per lane and slice where BRICK5 needs 3.  q0/q2 = bytes x,
        // x+1 of row y, q1/q3 of row y+1.
        constexpr unsigned kZ = LAYOUT == LAYOUT_BRICK41616 ? 64u
                             : LAYOUT == LAYOUT_BRICK488 || LAYOUT == LAYOUT_BRICK4816 || LAYOUT == LAYOUT_BRICK4832 ||
                                      LAYOUT == LAYOUT_BRICK4864 || LAYOUT == LAYOUT_COL48 ? 32u : 16u;
        const unsigned a0 = off & ~3u;
        const auto s0 = __builtin_amdgcn_raw_buffer_load_b64(f.rsrc[ch], a0, 0, 0);
        const auto s1 = __builtin_amdgcn_raw_buffer_load_b64(f.rsrc[ch], a0 + kZ, 0, 0);
        r.q0 = __builtin_amdgcn_alignbyte(s0[1], s0[0], off);
        r.q1 = __builtin_amdgcn_alignbyte(s0[1], s0[1], off);
        r.q2 = __builtin_amdgcn_alignbyte(s1[1], s1[0], off);
        r.q3 = __builtin_amdgcn_alignbyte(s1[1], s1[1], off);
    } else if constexpr (LAYOUT == LAYOUT_ZPAIR) {
        // the whole footprint is the 16 bytes at off & ~3 (x = off & 3 <= 2):
        // dwords = rows (y,z) (y,z+1) (y+1,z) (y+1,z+1); one load per tap
        const auto s0 = __builtin_amdgcn_raw_buffer_load_b128(f.rsrc[ch], off & ~3u, 0, 0);
        r.q0 = __builtin_amdgcn_alignbyte(s0[0], s0[0], off);
        r.q2 = __builtin_amdgcn_alignbyte(s0[1], s0[1], off);
        r.q1 = __builtin_amdgcn_alignbyte(s0[2], s0[2], off);
        r.q3 = __builtin_amdgcn_alignbyte(s0[3], s0[3], off);
    } else if constexpr (LAYOUT == LAYOUT_BRICK8) {
        // R = 8: rows y and y+1 of a slice are 8 bytes apart, so one
        // dword-aligned 16-byte load from off & ~3 holds both (bytes off,
        // off+1, off+8, off+9); the z+1 slice is 64 bytes on.  Two loads per
        // tap instead of four byte-offset u16 loads: 0.271 -> 0.235 ms at
        // 512^3, 0.185 -> 0.119 ms at 128^3.
        const unsigned o1 = off + 64;
        const auto s0 = __builtin_amdgcn_raw_buffer_load_b128(f.rsrc[ch], off & ~3u, 0, 0);
        const auto s1 = __builtin_amdgcn_raw_buffer_load_b128(f.rsrc[ch], o1 & ~3u, 0, 0);
        r.q0 = __builtin_amdgcn_alignbyte(s0[1], s0[0], off);   // c000 c100 in bytes 0-1
        r.q1 = __builtin_amdgcn_alignbyte(s0[3], s0[2], off);   // c010 c110
        r.q2 = __builtin_amdgcn_alignbyte(s1[1], s1[0], o1);    // c001 c101
        r.q3 = __builtin_amdgcn_alignbyte(s1[3], s1[2], o1);    // c011 c111
    } else {
        constexpr int R = LAYOUT == LAYOUT_BRICK8 ? 8 : 16;
        r.q0 = __builtin_amdgcn_raw_buffer_load_b16(f.rsrc[ch], off, 0, 0);
        r.q1 = __builtin_amdgcn_raw_buffer_load_b16(f.rsrc[ch], off + R, 0, 0);
        r.q2 = __builtin_amdgcn_raw_buffer_load_b16(f.rsrc[ch], off + R * R, 0, 0);
        r.q3 = __builtin_amdgcn_raw_buffer_load_b16(f.rsrc[ch], off + R * R + R, 0, 0);
    }
    return r;
}
template <int LAYOUT>
__device__ __forceinline__ float tap_blend(const TapRaw& r)
{
    if constexpr (LAYOUT == LAYOUT_CORNERH) {
        // rows q0 (y0,z0) q1 (y1,z0) q2 (y0,z1) q3 (y1,z1): x-lerps, then y, then z
        const float x00 = mix_lerp(r.wx, r.q0), x10 = mix_lerp(r.wx, r.q1);
        const float x01 = mix_lerp(r.wx, r.q2), x11 = mix_lerp(r.wx, r.q3);
        const float y0 = lerp_(x00, x10, r.wy), y1 = lerp_(x01, x11, r.wy);
        return lerp_(y0, y1, r.wz) * (1.0f / 255.0f);
    } else if constexpr (LAYOUT == LAYOUT_CORNER8) {
        return blend(f2{ubyte<0>(r.q0), ubyte<0>(r.q1)}, f2{ubyte<1>(r.q0), ubyte<1>(r.q1)},
                     f2{ubyte<2>(r.q0), ubyte<2>(r.q1)}, f2{ubyte<3>(r.q0), ubyte<3>(r.q1)}, r.wx, r.wy, r.wz);
    } else if constexpr (LAYOUT == LAYOUT_BRICK5) {
        return blend(f2{ubyte<0>(r.q0), ubyte<0>(r.q2)}, f2{ubyte<1>(r.q0), ubyte<1>(r.q2)},
                     f2{ubyte<1>(r.q1), ubyte<1>(r.q3)}, f2{ubyte<2>(r.q1), ubyte<2>(r.q3)}, r.wx, r.wy, r.wz);
    } else {
        return blend(f2{ubyte<0>(r.q0), ubyte<0>(r.q2)}, f2{ubyte<1>(r.q0), ubyte<1>(r.q2)},
                     f2{ubyte<0>(r.q1), ubyte<0>(r.q3)}, f2{ubyte<1>(r.q1), ubyte<1>(r.q3)}, r.wx, r.wy, r.wz);
    }
}
// One trilinear tap of one channel from a fast layout, at padded texel
// coordinate g (floor(g) = base texel + 1, fract(g) = weight).  Loads go
// through a range-checked buffer descriptor: an offset outside the plane
// reads 0 instead of faulting.
template <int LAYOUT>
__device__ __forceinline__ float tap_fast(const FastCtx& f, int ch, float gx, float gy, float gz)
{
    return tap_blend<LAYOUT>(tap_fetch<LAYOUT>(f, ch, gx, gy, gz));
}

template <int LAYOUT, bool ZO = false>
__device__ __forceinline__ TapRaw tap_fetch_at(const MarchArgs& a, const FastCtx& f, int t, f2 pxy, float pz)
{
    const TapPos g = LAYOUT == LAYOUT_CORNERH ? tap_pos<ZO>(a, t, pxy, pz, f.sz[t], f.oz[t]) : tap_pos<ZO>(a, t, pxy, pz);
    return tap_fetch<LAYOUT>(f, t, g.gxy.x, g.gxy.y, g.gz);
}

// One trilinear tap from the planar layout with full wrap semantics.
template <int WRAP>
__device__ __forceinline__ float tap_planar(const uint8_t* __restrict__ pl, const MarchArgs& a, float gx,
                                            float gy, float gz)
{
    const float wx = fract_(gx), wy = fract_(gy), wz = fract_(gz);
    const int ix = cvt_flr(gx) - 1, iy = cvt_flr(gy) - 1, iz = cvt_flr(gz) - 1;
    int i0, i1, j0, j1, k0, k1;
    if constexpr (WRAP == WRAP_CLAMP) {
        i0 = clampi(ix, 0, a.nx - 1); i1 = clampi(ix + 1, 0, a.nx - 1);
        j0 = clampi(iy, 0, a.ny - 1); j1 = clampi(iy + 1, 0, a.ny - 1);
        k0 = clampi(iz, 0, a.nz - 1); k1 = clampi(iz + 1, 0, a.nz - 1);
    } else {
        i0 = mirror_(ix, a.nx); i1 = mirror_(ix + 1, a.nx);
        j0 = mirror_(iy, a.ny); j1 = mirror_(iy + 1, a.ny);
        k0 = mirror_(iz, a.nz); k1 = mirror_(iz + 1, a.nz);
    }
    const int r00 = (k0 * a.ny + j0) * a.nx, r10 = (k0 * a.ny + j1) * a.nx;
    const int r01 = (k1 * a.ny + j0) * a.nx, r11 = (k1 * a.ny + j1) * a.nx;
    return blend(f2{ubyte<0>(pl[r00 + i0]), ubyte<0>(pl[r01 + i0])}, f2{ubyte<0>(pl[r00 + i1]), ubyte<0>(pl[r01 + i1])},
                 f2{ubyte<0>(pl[r10 + i0]), ubyte<0>(pl[r11 + i0])}, f2{ubyte<0>(pl[r10 + i1]), ubyte<0>(pl[r11 + i1])},
                 wx, wy, wz);
}

// Tap t at ray point P: padded texel coordinate g = fma(P, S_t, T_t).
template <int LAYOUT, int WRAP>
__device__ __forceinline__ float tap(const MarchArgs& a, const FastCtx& f, int t, f2 pxy, float pz)
{
    const TapPos g = tap_pos<false>(a, t, pxy, pz);
    if constexpr (LAYOUT == LAYOUT_PLANAR)
        return tap_planar<WRAP>(a.vol + (size_t)t * a.plane_stride, a, g.gxy.x, g.gxy.y, g.gz);
    else
        return tap_fast<LAYOUT>(f, t, g.gxy.x, g.gxy.y, g.gz);
}

// One ray of the grid path: setup, the march (frag.glsl:57-75), the
// epilogue (:76-80) and the store.  Returns the executed steps.
// The brick layouts run software-pipelined: step i+1's loads are issued
// before step i is blended, so a wave has two steps of gathers in flight.
// This costs VGPRs (67-73, 6-7 waves/SIMD) and is still faster: at 512^3
// brick5 0.334 -> 0.280 ms (before the aligned loads), brick8 unchanged.
// Fetching two steps ahead spilled to scratch and was 2.6x slower.  CORNER8 (the cache-resident
// layout, one load per tap) is not: 0.51 -> 0.56 ms at 3840x2160x256.
// Forcing 6 or 8 waves/SIMD (amdgpu_waves_per_eu) was slower in every case,
// with or without pipelining.
//
// Taps of a march with uniform channels UM (MarchArgs.umask): a uniform
// channel's tap is the constant uv[T], with no load.  Every march fills uv[] with the same
// four lines at its top; they stay written out, because the early-out QUAD instances
// compile to other code when the lines come from a helper (profiles/quadmode).
// COL48Z: taps 0-2 are COL48's, tap 3 ZPAIR's (its own tables and plane).
template <int UM, int T, int LAYOUT, bool ZO>
__device__ __forceinline__ TapRaw fetch_u(const MarchArgs& a, const FastCtx& f, f2 pxy, float pz)
{
    if constexpr ((UM >> T) & 1) {
        return TapRaw{};
    } else if constexpr (LAYOUT == LAYOUT_COL48Z) {
        if constexpr (T == 3) {
            FastCtx g = f;
            g.tx = f.tx3; g.ty = f.ty3; g.tz = f.tz3;
            return tap_fetch_at<LAYOUT_ZPAIR, ZO>(a, g, T, pxy, pz);
        } else {
            return tap_fetch_at<LAYOUT_COL48, ZO>(a, f, T, pxy, pz);
        }
    } else {
        return tap_fetch_at<LAYOUT, ZO>(a, f, T, pxy, pz);
    }
}
template <int UM, int T, int LAYOUT>
__device__ __forceinline__ float blend_u(const TapRaw& c, const float* uv)
{
    if constexpr ((UM >> T) & 1) return uv[T];
    else if constexpr (LAYOUT == LAYOUT_COL48Z) return tap_blend<T == 3 ? LAYOUT_ZPAIR : LAYOUT_COL48>(c);
    else return tap_blend<LAYOUT>(c);
}
template <int LAYOUT, int WRAP, bool EARLY, bool ZO = false, int UM = 0>
__device__ __forceinline__ unsigned march_pixel(const MarchArgs& a, const FastCtx& f, int x, int orow)
{
    const Ray r = setup_ray(a, x, orow);
    float uv[4] = {};
    if constexpr (UM != 0)
        for (int t = 0; t < 4; ++t)
            if ((UM >> t) & 1) uv[t] = noise::in_vgpr(a.uval[t]);
    if constexpr (LAYOUT != LAYOUT_PLANAR && LAYOUT != LAYOUT_CORNER8 && LAYOUT != LAYOUT_CORNERH) {
        f2 pxy = r.pxy;
        float pz = r.pz;
        float acc = 0.0f;
        int i = 0;
        if (r.n > 0) {
            TapRaw c0 = fetch_u<UM, 0, LAYOUT, ZO>(a, f, pxy, pz), c1 = fetch_u<UM, 1, LAYOUT, ZO>(a, f, pxy, pz);
            TapRaw c2 = fetch_u<UM, 2, LAYOUT, ZO>(a, f, pxy, pz), c3 = fetch_u<UM, 3, LAYOUT, ZO>(a, f, pxy, pz);
            for (; i < r.n; ++i) {
                const f2 cxy = pxy;
                const float cz = pz;
                pxy = pxy + r.sxy;                                                        // :74
                pz = pz + r.sz;
                // the last step re-fetches its own (in-box) point: no branch
                const bool more = i + 1 < r.n;
                const f2 qxy = more ? pxy : cxy;
                const float qz = more ? pz : cz;
                const TapRaw n0 = fetch_u<UM, 0, LAYOUT, ZO>(a, f, qxy, qz), n1 = fetch_u<UM, 1, LAYOUT, ZO>(a, f, qxy, qz);
                const TapRaw n2 = fetch_u<UM, 2, LAYOUT, ZO>(a, f, qxy, qz), n3 = fetch_u<UM, 3, LAYOUT, ZO>(a, f, qxy, qz);
                const float t0 = blend_u<UM, 0, LAYOUT>(c0, uv), t1 = blend_u<UM, 1, LAYOUT>(c1, uv);
                const float t2 = blend_u<UM, 2, LAYOUT>(c2, uv), t3 = blend_u<UM, 3, LAYOUT>(c3, uv);
                acc = acc + ((t0 * t1) * (t2 + t3)) * a.scale;                           // :71-73
                c0 = n0; c1 = n1; c2 = n2; c3 = n3;
                if constexpr (EARLY) {
                    if (acc > a.acc_limit) { ++i; break; }
                }
            }
        }
        if (r.live) store_pixel(a, x, orow, r.n >= 0, ray_grey(a, acc));                  // :76-79
        return r.n > 0 ? (unsigned)i : 0u;
    }
    f2 pxy = r.pxy;
    float pz = r.pz;
    float acc = 0.0f;
    int i = 0;
    for (; i < r.n; ++i) {
        float t0, t1, t2, t3;
        if constexpr (LAYOUT != LAYOUT_PLANAR) {
            t0 = blend_u<UM, 0, LAYOUT>(fetch_u<UM, 0, LAYOUT, ZO>(a, f, pxy, pz), uv);
            t1 = blend_u<UM, 1, LAYOUT>(fetch_u<UM, 1, LAYOUT, ZO>(a, f, pxy, pz), uv);
            t2 = blend_u<UM, 2, LAYOUT>(fetch_u<UM, 2, LAYOUT, ZO>(a, f, pxy, pz), uv);
            t3 = blend_u<UM, 3, LAYOUT>(fetch_u<UM, 3, LAYOUT, ZO>(a, f, pxy, pz), uv);
        } else {
            t0 = tap<LAYOUT, WRAP>(a, f, 0, pxy, pz);
            t1 = tap<LAYOUT, WRAP>(a, f, 1, pxy, pz);
            t2 = tap<LAYOUT, WRAP>(a, f, 2, pxy, pz);
            t3 = tap<LAYOUT, WRAP>(a, f, 3, pxy, pz);
        }
        acc = acc + ((t0 * t1) * (t2 + t3)) * (LAYOUT == LAYOUT_CORNERH ? f.scale : a.scale);   // :71-73
        pxy = pxy + r.sxy;                                                            // :74
        pz = pz + r.sz;
        if constexpr (EARLY) {
            if (acc > a.acc_limit) { ++i; break; }
        }
    }
    if (r.live) store_pixel(a, x, orow, r.n >= 0, ray_grey(a, acc));                  // :76-79
    return r.n > 0 ? (unsigned)i : 0u;
}

// ---- the QUAD kernels' split fetch (option quad_split) ----
// In a QUAD kernel the four lanes of a quad hold one ray (regions_frames_body), so a
// tap_fetch there loads the same two 8-byte slices four times over.  Here the march runs
// in pairs of steps and the quad splits a pair's fetch: quad lane fl loads z-slice fl & 1
// (+ (fl & 1) * kZ) of step a + (fl >> 1) -- one b64 instruction per tap and pair where
// tap_fetch issues four, all in the tap's own channel plane, so the descriptor and its
// range check are tap_fetch's.  The loading lane shifts its slice down by its own off & 3
// and packs the four footprint texels into one dword: bytes 0, 1 = row y at x, x + 1,
// bytes 2, 3 = row y + 1.  A consumer reads byte K of quad lane J's dword through DPP
// quad_perm [J, J, J, J]: no LDS, no further memory instruction.
//
// Every lane still marches its own ray: it advances the point by the same repeated adds
// as march_pixel, computes the weights of both steps from it, blends both and updates acc
// in march_pixel's order: step a + 1's term is added only where the ray has that step and
// step a's sum did not pass acc_limit, so acc takes march_pixel's values one after the
// other.  Only the lane's own step goes through cvt_flr, the offset tables and the load.
//
// The exchange needs every lane of a quad active wherever one is.  That holds because the
// lanes of a quad share the ray: r.n, the early-out and the edge-of-frame case are the
// same in all four, so a quad takes every branch below as one.
//
// The one cross-lane primitive: v of the quad lanes a quad_perm control names (vr_internal.h
// quad_perm_ctrl; quad_lane_ctrl(J) names lane J in all four).
template <int CTRL>
__device__ __forceinline__ unsigned quad_read(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
template <int J>
__device__ __forceinline__ float quad_lane_f(float v)
{
    return __builtin_bit_cast(float, quad_read<quad_lane_ctrl(J)>(__builtin_bit_cast(unsigned, v)));
}
// byte K of v as float.  Not ubyte<K>(): the compiler folds quad_read's DPP move into
// this v_cvt_f32_ubyteK, which it cannot do through an asm statement, and it keeps the
// wait states between the pack and the DPP read
template <int K>
__device__ __forceinline__ float ubyte_of(unsigned v) { return (float)((v >> (8 * K)) & 0xffu); }
// blend()'s first four arguments from a footprint's two packed z-slices (split_pack), z0 and z1,
// each read from the quad lane that loaded it.  The weights are not passed through here: a
// caller that forms them in the blend's argument list (split_blend) keeps them after the converts.
struct Footprint {
    f2 lo_a, hi_a, lo_b, hi_b;
};
__device__ __forceinline__ Footprint packed_footprint(unsigned z0, unsigned z1)
{
    return Footprint{f2{ubyte_of<0>(z0), ubyte_of<0>(z1)}, f2{ubyte_of<1>(z0), ubyte_of<1>(z1)},
                     f2{ubyte_of<2>(z0), ubyte_of<2>(z1)}, f2{ubyte_of<3>(z0), ubyte_of<3>(z1)}};
}

// one lane's part of a step pair's fetch of one tap: its slice, and the offset whose low bits shift it
struct SliceRaw {
    unsigned s0, s1, off;
};
template <int UM, int T, bool ZO>
__device__ __forceinline__ SliceRaw split_fetch(const MarchArgs& a, const FastCtx& f, f2 pxy, float pz, unsigned zoff)
{
    if constexpr ((UM >> T) & 1) {
        return SliceRaw{};
    } else {
        const TapPos g = tap_pos<ZO>(a, T, pxy, pz);
        const unsigned off = f.tx[cvt_flr(g.gxy.x)] + f.ty[cvt_flr(g.gxy.y)] + f.tz[cvt_flr(g.gz)];
        const auto s = __builtin_amdgcn_raw_buffer_load_b64(f.rsrc[T], (off & ~3u) + zoff, 0, 0);
        return SliceRaw{s[0], s[1], off};
    }
}
__device__ __forceinline__ unsigned split_pack(const SliceRaw& r)
{
    const unsigned q0 = __builtin_amdgcn_alignbyte(r.s1, r.s0, r.off);   // bytes 0, 1: row y at x, x + 1
    const unsigned q1 = __builtin_amdgcn_alignbyte(r.s1, r.s1, r.off);   // row y + 1
    return __builtin_amdgcn_perm(q1, q0, 0x05040100u);
}
// tap T of the pair's step H (0, 1) at the ray point (pxy, pz): the slices are quad lanes 2H and 2H + 1's
template <int UM, int T, int H, bool ZO>
__device__ __forceinline__ float split_blend(const MarchArgs& a, unsigned pk, f2 pxy, float pz, const float* uv)
{
    if constexpr ((UM >> T) & 1) {
        return uv[T];
    } else {
        const TapPos g = tap_pos<ZO>(a, T, pxy, pz);
        const Footprint p = packed_footprint(quad_read<quad_lane_ctrl(2 * H)>(pk), quad_read<quad_lane_ctrl(2 * H + 1)>(pk));
        return blend(p.lo_a, p.hi_a, p.lo_b, p.hi_b, fract_(g.gxy.x), fract_(g.gxy.y), fract_(g.gz));
    }
}
// march_pixel for quad lane fl of a QUAD kernel (COL48 / BRICK4832).  Software-pipelined
// like march_pixel, by pairs: the loads of steps i + 2, i + 3 are issued before steps i,
// i + 1 are blended.  A lane whose own step lies past the ray's last one loads the pair's
// first point again, which is in the box: no load names a point outside it.
template <int LAYOUT, bool EARLY, bool ZO, int UM>
__device__ __forceinline__ void march_pixel_quad_split(const MarchArgs& a, const FastCtx& f, int x, int orow, int fl)
{
    static_assert(quad_split_layout(LAYOUT), "the packed slice is the b4 family's with 32-byte z-slices");
    const Ray r = setup_ray(a, x, orow);
    float uv[4] = {};
    if constexpr (UM != 0)
        for (int t = 0; t < 4; ++t)
            if ((UM >> t) & 1) uv[t] = noise::in_vgpr(a.uval[t]);
    float acc = 0.0f;
    if (r.n > 0) {
        const bool hi = (fl & 2) != 0;             // this lane loads for the pair's second step
        const unsigned zoff = (fl & 1) * kSplitZ;   // and this z-slice of it
        f2 axy = r.pxy, bxy = r.pxy + r.sxy;        // the points of steps i and i + 1       // :74
        float az = r.pz, bz = r.pz + r.sz;
        bool mine = hi && 1 < r.n;
        f2 qxy = mine ? bxy : axy;
        float qz = mine ? bz : az;
        SliceRaw c0 = split_fetch<UM, 0, ZO>(a, f, qxy, qz, zoff), c1 = split_fetch<UM, 1, ZO>(a, f, qxy, qz, zoff);
        SliceRaw c2 = split_fetch<UM, 2, ZO>(a, f, qxy, qz, zoff), c3 = split_fetch<UM, 3, ZO>(a, f, qxy, qz, zoff);
        for (int i = 0;;) {
            const f2 cxy = bxy + r.sxy, dxy = cxy + r.sxy;   // steps i + 2 and i + 3
            const float cz = bz + r.sz, dz = cz + r.sz;
            mine = i + 2 + (hi ? 1 : 0) < r.n;
            qxy = mine ? (hi ? dxy : cxy) : axy;
            qz = mine ? (hi ? dz : cz) : az;
            const SliceRaw n0 = split_fetch<UM, 0, ZO>(a, f, qxy, qz, zoff), n1 = split_fetch<UM, 1, ZO>(a, f, qxy, qz, zoff);
            const SliceRaw n2 = split_fetch<UM, 2, ZO>(a, f, qxy, qz, zoff), n3 = split_fetch<UM, 3, ZO>(a, f, qxy, qz, zoff);
            const unsigned p0 = split_pack(c0), p1 = split_pack(c1), p2 = split_pack(c2), p3 = split_pack(c3);
            bool stop = false;
            {
                const float t0 = split_blend<UM, 0, 0, ZO>(a, p0, axy, az, uv), t1 = split_blend<UM, 1, 0, ZO>(a, p1, axy, az, uv);
                const float t2 = split_blend<UM, 2, 0, ZO>(a, p2, axy, az, uv), t3 = split_blend<UM, 3, 0, ZO>(a, p3, axy, az, uv);
                acc = acc + ((t0 * t1) * (t2 + t3)) * a.scale;                           // :71-73
                if constexpr (EARLY) stop = acc > a.acc_limit;
            }
            __builtin_amdgcn_sched_barrier(0);
            {
                // the pair's second step counts where the ray has it and the first did not end the
                // march; its term is formed either way, so a pair is one block with its loads on top
                const float t0 = split_blend<UM, 0, 1, ZO>(a, p0, bxy, bz, uv), t1 = split_blend<UM, 1, 1, ZO>(a, p1, bxy, bz, uv);
                const float t2 = split_blend<UM, 2, 1, ZO>(a, p2, bxy, bz, uv), t3 = split_blend<UM, 3, 1, ZO>(a, p3, bxy, bz, uv);
                const float both = acc + ((t0 * t1) * (t2 + t3)) * a.scale;
                acc = i + 1 < r.n && !stop ? both : acc;
                if constexpr (EARLY) stop = acc > a.acc_limit;
            }
            i += 2;
            if (stop || i >= r.n) break;
            c0 = n0; c1 = n1; c2 = n2; c3 = n3;
            axy = cxy; az = cz;
            bxy = dxy; bz = dz;
        }
    }
    if (r.live) store_pixel(a, x, orow, r.n >= 0, ray_grey(a, acc));                  // :76-79
}

// ---- the QUAD kernels' step rounds (option quad_steps) ----
// The split fetch above shares a quad's loads and leaves its arithmetic fourfold: every lane
// forms the coordinates, the weights and the blend of both steps of a pair.  Here the march
// runs in rounds of four steps and quad lane fl owns step base + fl: it fetches that step
// as fetch_u does (both z-slices, two b64 loads per loaded tap -- per quad and tap the pieces
// the split fetch asks for over two pairs), blends it with blend_u and forms the step's term
// ((t0 * t1) * (t2 + t3)) * scale as march_pixel does, rounded on the owning lane.  The term
// is the only value that crosses lanes: every lane reads the round's four through DPP
// quad_perm [J, J, J, J] and adds them to its own acc in step order (quad_round_accumulate),
// so acc takes march_pixel's values one after the other, and every lane keeps its own acc,
// early-out and store.  This is march_pixel_split<K>'s scheme with DPP in place of __shfl.
//
// Every lane advances the ray point by march_pixel's chain of single adds, four per round,
// and picks its own step's point from the chain; a point is never formed as p0 + k * s.  A
// lane whose step lies past the ray's last one takes the current round's first point, which
// is in the box: no load names a point outside it.
//
// The exchange needs every lane of a quad active wherever one is.  That holds for the reason
// given above march_pixel_quad_split: the lanes of a quad share the ray, so r.n, the
// early-out (each lane adds the same four terms in the same order) and the edge-of-frame
// case are the same in all four, and a quad takes every branch below as one.
//
// Software-pipelined like march_pixel, by rounds: the loads of round base + 4 are issued
// before round base is blended, two rounds of 2 x b64 x loaded taps in flight per lane.
//
// The fetch is tap_fetch's for these layouts (fetch_u / tap_fetch_at: the same coordinates,
// offset and two b64 loads) with the shift by off & 3 left to the consumer: tap_fetch shifts
// in the round that loads, which makes that round wait for its own look-ahead loads.  A
// StepRaw carries the loaded dwords over the loop's back edge and step_tap turns it into
// the TapRaw that blend_u takes.
struct StepRaw {
    unsigned s00, s01, s10, s11, off;
    float wx, wy, wz;
};
// ---- the step rounds' paired fetch (option quad_pairs) ----
// A step_fetch instruction names one z-slice of the round's four steps, up to four 128-byte
// lines per quad; a split_fetch instruction names both slices of two steps, which are 32 bytes
// apart and mostly share a line.  With QUAD_PAIRS the round keeps its one blend per lane and takes
// the split fetch's address pattern.  The owner side is unchanged: lane fl forms its own step's
// coordinates, weights and offset.  The loads are dealt again (vr_internal.h pair_load_step /
// pair_load_slice): instruction A serves steps base + 0 and base + 1, B base + 2 and base + 3,
// and in each quad lane fl loads z-slice fl & 1 of the instruction's step fl >> 1, at the owning
// lane's offset, read through DPP.  Per quad, tap and round these are the eight pieces the
// lanes load without it, each once; every owner's offset is in the plane (a lane past the
// ray's end takes the round's first point), so the descriptor and its range check are
// tap_fetch's.  The StepRaw then holds A's dwords in s00, s01, B's in s10, s11, and in off the
// loaded steps' off & 3: A's in bits 0-1, B's from bit 2 up.
//
// The round that consumes the loads shifts and packs them (pair_blend): the loader shifts its
// slice by the loaded step's off & 3 and packs the footprint's four texels into one dword
// (split_pack), and owner j reads slice z of its step from instruction pair_owner_instr(j),
// quad lane pair_owner_lane(j, z), and blends with its own weights in split_blend's form -- the
// floats tap_blend sees.  Every DPP read has an active source for the reason given above
// march_pixel_quad_split.
template <int UM, int T, bool ZO, int QM>
__device__ __forceinline__ StepRaw step_fetch(const MarchArgs& a, const FastCtx& f, f2 pxy, float pz, int fl)
{
    if constexpr ((UM >> T) & 1) {
        return StepRaw{};
    } else {
        const TapPos g = tap_pos<ZO>(a, T, pxy, pz);
        const unsigned off = f.tx[cvt_flr(g.gxy.x)] + f.ty[cvt_flr(g.gxy.y)] + f.tz[cvt_flr(g.gz)];
        if constexpr (quad_paired(QM)) {
            const unsigned zoff = (unsigned)pair_load_slice(fl) * kSplitZ;
            // the owner aligns, the loader adds its slice: one v_add_u32 with a DPP source per address
            const unsigned al = off & ~3u;
            const auto sa = __builtin_amdgcn_raw_buffer_load_b64(f.rsrc[T], quad_read<pair_load_ctrl(0)>(al) + zoff, 0, 0);
            const auto sb = __builtin_amdgcn_raw_buffer_load_b64(f.rsrc[T], quad_read<pair_load_ctrl(1)>(al) + zoff, 0, 0);
            const unsigned sh = (quad_read<pair_load_ctrl(0)>(off) & 3u) | (quad_read<pair_load_ctrl(1)>(off) << 2);
            return StepRaw{sa[0], sa[1], sb[0], sb[1], sh, fract_(g.gxy.x), fract_(g.gxy.y), fract_(g.gz)};
        } else {
            const auto s0 = __builtin_amdgcn_raw_buffer_load_b64(f.rsrc[T], off & ~3u, 0, 0);
            const auto s1 = __builtin_amdgcn_raw_buffer_load_b64(f.rsrc[T], (off & ~3u) + kSplitZ, 0, 0);
            return StepRaw{s0[0], s0[1], s1[0], s1[1], off, fract_(g.gxy.x), fract_(g.gxy.y), fract_(g.gz)};
        }
    }
}
__device__ __forceinline__ TapRaw step_tap(const StepRaw& r)
{
    return TapRaw{__builtin_amdgcn_alignbyte(r.s01, r.s00, r.off), __builtin_amdgcn_alignbyte(r.s01, r.s01, r.off),
                  __builtin_amdgcn_alignbyte(r.s11, r.s10, r.off), __builtin_amdgcn_alignbyte(r.s11, r.s11, r.off),
                  r.wx, r.wy, r.wz};
}
template <int UM, int T>
__device__ __forceinline__ float pair_blend(const StepRaw& r, int fl, const float* uv)
{
    if constexpr ((UM >> T) & 1) {
        return uv[T];
    } else {
        const unsigned pa = split_pack(SliceRaw{r.s00, r.s01, r.off}), pb = split_pack(SliceRaw{r.s10, r.s11, r.off >> 2});
        const unsigned a0 = quad_read<pair_owner_ctrl(0)>(pa), b0 = quad_read<pair_owner_ctrl(0)>(pb);
        const unsigned a1 = quad_read<pair_owner_ctrl(1)>(pa), b1 = quad_read<pair_owner_ctrl(1)>(pb);
        const bool second = pair_owner_instr(fl) != 0;
        const Footprint p = packed_footprint(second ? b0 : a0, second ? b1 : a1);
        return blend(p.lo_a, p.hi_a, p.lo_b, p.hi_b, r.wx, r.wy, r.wz);
    }
}

template <int LAYOUT, bool EARLY, bool ZO, int UM, int QM>
__device__ __forceinline__ void march_pixel_quad_steps(const MarchArgs& a, const FastCtx& f, int x, int orow, int fl)
{
    static_assert(quad_split_layout(LAYOUT) && quad_rounds(QM), "built for the layouts of the split fetch");
    constexpr bool PAIRS = quad_paired(QM);
    const Ray r = setup_ray(a, x, orow);
    float uv[4] = {};
    if constexpr (UM != 0)
        for (int t = 0; t < 4; ++t)
            if ((UM >> t) & 1) uv[t] = noise::in_vgpr(a.uval[t]);
    float acc = 0.0f;
    if (r.n > 0) {
        // the point of step base + fl out of the chain's four
        const auto own = [fl](auto p0, auto p1, auto p2, auto p3) { return fl & 2 ? (fl & 1 ? p3 : p2) : (fl & 1 ? p1 : p0); };
        f2 axy = r.pxy;                                         // the points of steps base .. base + 3   // :74
        float az = r.pz;
        f2 bxy = axy + r.sxy, cxy = bxy + r.sxy, dxy = cxy + r.sxy;
        float bz = az + r.sz, cz = bz + r.sz, dz = cz + r.sz;
        bool mine = fl < r.n;
        f2 qxy = mine ? own(axy, bxy, cxy, dxy) : axy;
        float qz = mine ? own(az, bz, cz, dz) : az;
        StepRaw c0 = step_fetch<UM, 0, ZO, QM>(a, f, qxy, qz, fl), c1 = step_fetch<UM, 1, ZO, QM>(a, f, qxy, qz, fl);
        StepRaw c2 = step_fetch<UM, 2, ZO, QM>(a, f, qxy, qz, fl), c3 = step_fetch<UM, 3, ZO, QM>(a, f, qxy, qz, fl);
        for (int base = 0;;) {
            const f2 exy = dxy + r.sxy, fxy = exy + r.sxy, gxy = fxy + r.sxy, hxy = gxy + r.sxy;   // steps base + 4 .. base + 7
            const float ez = dz + r.sz, fz = ez + r.sz, gz = fz + r.sz, hz = gz + r.sz;
            mine = base + 4 + fl < r.n;
            qxy = mine ? own(exy, fxy, gxy, hxy) : axy;
            qz = mine ? own(ez, fz, gz, hz) : az;
            const StepRaw n0 = step_fetch<UM, 0, ZO, QM>(a, f, qxy, qz, fl), n1 = step_fetch<UM, 1, ZO, QM>(a, f, qxy, qz, fl);
            const StepRaw n2 = step_fetch<UM, 2, ZO, QM>(a, f, qxy, qz, fl), n3 = step_fetch<UM, 3, ZO, QM>(a, f, qxy, qz, fl);
            const float t0 = PAIRS ? pair_blend<UM, 0>(c0, fl, uv) : blend_u<UM, 0, LAYOUT>(step_tap(c0), uv);
            const float t1 = PAIRS ? pair_blend<UM, 1>(c1, fl, uv) : blend_u<UM, 1, LAYOUT>(step_tap(c1), uv);
            const float t2 = PAIRS ? pair_blend<UM, 2>(c2, fl, uv) : blend_u<UM, 2, LAYOUT>(step_tap(c2), uv);
            const float t3 = PAIRS ? pair_blend<UM, 3>(c3, fl, uv) : blend_u<UM, 3, LAYOUT>(step_tap(c3), uv);
            const float term = ((t0 * t1) * (t2 + t3)) * a.scale;                        // :71-73
            // the look-ahead loads stay above this line: without it the compiler sinks them below the
            // loop's exit test, into the branch that goes round again, and waits for them there
            __builtin_amdgcn_sched_barrier(0);
            bool stop;
            acc = quad_round_accumulate<EARLY>(acc, quad_lane_f<0>(term), quad_lane_f<1>(term), quad_lane_f<2>(term),
                                               quad_lane_f<3>(term), base, r.n, a.acc_limit, &stop);
            base += 4;
            if (stop || base >= r.n) break;
            c0 = n0; c1 = n1; c2 = n2; c3 = n3;
            axy = exy; az = ez;
            dxy = hxy; dz = hz;
        }
    }
    if (r.live) store_pixel(a, x, orow, r.n >= 0, ray_grey(a, acc));                  // :76-79
}

// Kernel prologue for the fast layouts: buffer descriptors (wave-uniform,
// from kernargs only) and the per-axis offset tables, built in LDS by the
// whole workgroup.  The tables are the only LDS use and are read-only after
// the barrier.
template <int LAYOUT>
__device__ __forceinline__ FastCtx fast_prologue(const MarchArgs& a, unsigned* lds)
{
    FastCtx f{};
    if constexpr (LAYOUT == LAYOUT_CORNERH) {
        // no offset tables: the index is arithmetic (tap_fetch)
        for (int c = 0; c < 4; ++c)
            f.rsrc[c] = __builtin_amdgcn_make_buffer_rsrc((void*)(a.vol + (size_t)c * a.plane_stride), (short)0,
                                                          (int)a.plane_stride, 0x00020000);
        f.s1x16 = (float)(16 * a.geom.nbx);
        f.s2x16 = (float)(16 * a.geom.nbx) * (float)a.geom.nby;
        for (int c = 0; c < 4; ++c) {
            f.sz[c] = noise::in_vgpr(a.tap_S[c][2]);
            f.oz[c] = noise::in_vgpr(a.tap_T[c][2]);
        }
        f.scale = noise::in_vgpr(a.scale);
    } else if constexpr (LAYOUT == LAYOUT_COL48Z) {
        for (int c = 0; c < 4; ++c)
            f.rsrc[c] = __builtin_amdgcn_make_buffer_rsrc((void*)(a.vol + (size_t)c * a.plane_stride), (short)0,
                                                          (int)(c < 3 ? a.plane_stride : a.plane3_bytes), 0x00020000);
        const int nx1 = a.nx + 1, ny1 = a.ny + 1, nz1 = a.nz + 1, n3 = nx1 + ny1 + nz1;
        for (int i = threadIdx.x; i < 2 * n3; i += (int)blockDim.x) {
            const int set = i >= n3, j = i - set * n3;
            const int axis = j < nx1 ? 0 : j < nx1 + ny1 ? 1 : 2;
            const int pos = axis == 0 ? j : axis == 1 ? j - nx1 : j - nx1 - ny1;
            lds[i] = set ? axis_offset(a.geom3, LAYOUT_ZPAIR, axis, pos) : axis_offset(a.geom, LAYOUT_COL48, axis, pos);
        }
        __syncthreads();
        f.tx = lds;
        f.ty = lds + nx1;
        f.tz = lds + nx1 + ny1;
        f.tx3 = lds + n3;
        f.ty3 = lds + n3 + nx1;
        f.tz3 = lds + n3 + nx1 + ny1;
    } else if constexpr (LAYOUT != LAYOUT_PLANAR) {
        for (int c = 0; c < 4; ++c)
            f.rsrc[c] = __builtin_amdgcn_make_buffer_rsrc((void*)(a.vol + (size_t)c * a.plane_stride), (short)0,
                                                          (int)a.plane_stride, 0x00020000);
        const int nx1 = a.nx + 1, ny1 = a.ny + 1, nz1 = a.nz + 1;
        for (int i = threadIdx.x; i < nx1 + ny1 + nz1; i += (int)blockDim.x) {
            const int axis = i < nx1 ? 0 : i < nx1 + ny1 ? 1 : 2;
            const int pos = axis == 0 ? i : axis == 1 ? i - nx1 : i - nx1 - ny1;
            lds[i] = axis_offset(a.geom, LAYOUT, axis, pos);   // once per workgroup
        }
        __syncthreads();
        f.tx = lds;
        f.ty = lds + nx1;
        f.tz = lds + nx1 + ny1;
    }
    return f;
}

// Static schedule: one 16x16 tile per workgroup, one 8x8 sub-tile per wave.
// Tile rows are dealt to XCDs round-robin: XCD x (= blockIdx % 8 under the
// observed dispatch, a speed-only assumption) walks tile rows x, x+8, ...
template <int LAYOUT, int WRAP, bool EARLY>
__global__ __launch_bounds__(kThreads) void march_grid(const MarchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int k = j / a.tiles_x, tx = j - k * a.tiles_x;
    const int ty = xcd + 8 * k;
    if (ty >= a.tiles_y) return;   // whole workgroup: uniform, before the barrier
    const FastCtx f = fast_prologue<LAYOUT>(a, lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = tx * kTile + (wave & 1) * 8 + lane_x<LAYOUT>(lane);
    const int orow = ty * kTile + (wave >> 1) * 8 + lane_y<LAYOUT>(lane);
    const unsigned steps = march_pixel<LAYOUT, WRAP, EARLY>(a, f, x, orow);
    if (a.step_counter) add_steps(a, steps);
}

// Strided schedule: wave g (of nw) renders 8x8 tiles g, g + nw, g + 2nw, ...
// of the row-major tile grid.  Its tiles sit 1/T of the image apart, so the
// per-wave (and per-SIMD) work evens out without atomics.
template <int LAYOUT, int WRAP, bool EARLY>
__global__ __launch_bounds__(kThreads) void march_strided(const MarchArgs a, int nw)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const FastCtx f = fast_prologue<LAYOUT>(a, lds);
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int tiles_x8 = (a.width + 7) >> 3, rows8 = (a.out_rows + 7) >> 3;
    const int ntiles = tiles_x8 * rows8;
    unsigned long long steps = 0;
    for (int t = g; t < ntiles; t += nw) {
        const int ty = t / tiles_x8, tx = t - ty * tiles_x8;
        steps += march_pixel<LAYOUT, WRAP, EARLY>(a, f, tx * 8 + lane_x<LAYOUT>(lane), ty * 8 + lane_y<LAYOUT>(lane));
    }
    if (a.step_counter) add_steps(a, steps);
}

// Ring schedule: wave k renders the k-th 8x8 tile of square rings around the
// tile (cx, cy) under the projected box centre, inside-out (ring_tile,
// vr_march_common.h); waves whose tile is off the target exit at once.
template <int LAYOUT, int WRAP, bool EARLY, bool ZO>
__global__ __launch_bounds__(kThreads) void march_rings(const MarchArgs a, int cx, int cy, int nw, int npos)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const FastCtx f = fast_prologue<LAYOUT>(a, lds);
    const int lane = threadIdx.x & 63;
    const int tiles_x8 = (a.width + 7) >> 3, rows8 = (a.out_rows + 7) >> 3;
    unsigned long long steps = 0;
    // wave g takes ring positions g, g + nw, ... (nw = all waves): fewer
    // workgroups, so fewer LDS-table prologues, in the same inside-out order
    for (int k = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); k < npos; k += nw) {
        int tx, ty;
        ring_tile(k, cx, cy, &tx, &ty);
        if (tx >= 0 && tx < tiles_x8 && ty >= 0 && ty < rows8)
            steps += march_pixel<LAYOUT, WRAP, EARLY, ZO>(a, f, tx * 8 + lane_x<LAYOUT>(lane),
                                                      ty * 8 + lane_y<LAYOUT>(lane));
    }
    if (a.step_counter) add_steps(a, steps);
}

// Regions schedule: each XCD renders one host-built list of 8x8 tiles, a few
// contiguous angular wedges of the frame around the box centre with equal
// estimated work, inside-out (vr_api.cpp build_regions).  Rays of neighbouring
// tiles read the same 128-B bricks, so keeping neighbours on one XCD lets its
// L2 serve them once: the lines the eight L2s fetch per 1080p frame at 512^3
// drop from ~900 MB (ring positions dealt round-robin over XCDs) to ~620 MB
// (DESIGN.md sec. 5.3).  XCD = blockIdx % 8 is a speed-only assumption.
// WGW waves per workgroup (option wg_waves): the waves of one workgroup run on
// one CU and share its L1, and they render consecutive list entries.
// The regions lists' empty tiles (MarchArgs.empty_fill; vr_internal.h
// tile_is_empty): XCD x's entries [marched, count) after the marched ones.
// Wave w of the XCD writes the uncovered value -- what the march stores for a
// ray that misses (setup_ray, store_pixel) -- to the pixels of entries
// marched + w, marched + w + nwx, ...: one store per lane, no ray setup.
__device__ __forceinline__ void fill_empty_tiles(const MarchArgs& a, const unsigned* __restrict__ tiles, int begin,
                                                 int marched, int count, int w, int nwx)
{
    const int lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
    for (int k = marched + w; w < nwx && k < count; k += nwx) {
        const unsigned t = tiles[begin + k];
        const int x = (int)(t & 0xffffu) * 8 + lx, orow = (int)(t >> 16) * 8 + ly;
        if (x < a.width && orow < a.out_rows) {
            const int bl = orow / a.band_rows;
            const int y = set_band(bl, a.band_first, a.band_stride, a.band_flip) * a.band_rows + (orow - bl * a.band_rows);
            if (y < a.height) store_pixel(a, x, orow, false, 0.0f);
        }
    }
}

template <int LAYOUT, int WRAP, bool EARLY, bool ZO, int WGW, int UM>
__device__ __forceinline__ void regions_body(const MarchArgs& a, const unsigned* __restrict__ tiles, const int* __restrict__ hdr, int nwx,
                                             unsigned* lds)
{
    const int xcd = blockIdx.x & 7;
    const int w = (int)(blockIdx.x >> 3) * WGW + (threadIdx.x >> 6);
    const int begin = hdr[xcd], all = hdr[xcd + 1] - begin;
    const int count = a.empty_fill ? min(hdr[kRegionWork + xcd], all) : all;   // marched entries
    if (a.empty_fill) fill_empty_tiles(a, tiles, begin, count, all, w, nwx);
    if ((int)(blockIdx.x >> 3) * WGW >= count) return;   // whole workgroup, before the barrier
#ifdef VR_TIMELINE
    const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
#endif
    const FastCtx f = fast_prologue<LAYOUT>(a, lds);
    const int lane = threadIdx.x & 63;
    unsigned long long steps = 0;
    for (int k = w; w < nwx && k < count; k += nwx) {   // the grid rounds nwx up to whole workgroups
        const unsigned t = tiles[begin + k];
        const int tx = (int)(t & 0xffffu), ty = (int)(t >> 16);
        steps += march_pixel<LAYOUT, WRAP, EARLY, ZO, UM>(a, f, tx * 8 + lane_x<LAYOUT>(lane),
                                                          ty * 8 + lane_y<LAYOUT>(lane));
    }
#ifdef VR_TIMELINE
    timeline_record(t_begin, steps);
#endif
    if (a.step_counter) add_steps(a, steps);
}
template <int LAYOUT, int WRAP, bool EARLY, bool ZO, int WGW = kThreads / 64>
__global__ __launch_bounds__(64 * WGW) void march_regions(const MarchArgs a, const unsigned* __restrict__ tiles,
                                                         const int* __restrict__ hdr, int nwx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    regions_body<LAYOUT, WRAP, EARLY, ZO, WGW, 0>(a, tiles, hdr, nwx, lds);
}
// with uniform channels UM (march_pixel's fetch_u / blend_u).
// The _u kernels built for 5 waves per SIMD (amdgpu_waves_per_eu): config 5
// 0.198 ms against 0.127 (profiles/r03/ab_uniform_5waves.txt), so no attribute.
template <int LAYOUT, int WRAP, bool EARLY, bool ZO, int UM>
__global__ __launch_bounds__(kThreads) void march_regions_u(const MarchArgs a, const unsigned* __restrict__ tiles,
                                                           const int* __restrict__ hdr, int nwx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    regions_body<LAYOUT, WRAP, EARLY, ZO, kThreads / 64, UM>(a, tiles, hdr, nwx, lds);
}

// ---- NF queued frames in one launch (vr_render_pair: 2, vr_render_group: 4;
// DESIGN.md sec. 5.1.7 - 5.1.9) ----
// The regions schedule over one list and one header (frame 0's) for NF frames: a wave takes
// (list entry, frame f) and marches the entry with frame f's arguments, so the frames read
// an entry's bricks at the same moment on the same XCD.  The frames travel as one MarchArgs
// (frame 0's: the launch's common part) and FrameArgs fr[NF] (vr_internal.h).  There is one
// copy of the march: wave f's MarchArgs is the common part with fr[f] laid over it -- scalar
// loads at the wave-uniform index f -- and equals what a plain render of frame f passes.
// A workgroup is 4 waves = 4 / NF entry waves x NF frames; XCD x's entry wave w takes the
// entries w, w + nwx, ...
//   NF 4:         f = the wave; workgroup g is entry wave g -- all four readers of an
//                 entry's bricks sit behind one L1
//   NF 2, deal 0: f = the wave's parity in its workgroup -- a workgroup is 2 consecutive
//                 entry waves x 2 frames, both readers on one CU (L1 and L2)
//   NF 2, deal 1: f = the workgroup's parity on its XCD -- a workgroup keeps 4 consecutive
//                 entry waves (the 2x2 supertile) of one frame; L2 only (option pair_deal)
// QM (vr_internal.h QuadMode) says how an NF 4 launch uses the lanes of a quad; each mode is
// the one above it and one thing more (quad_is_quad, quad_splits, quad_rounds, quad_paired):
//   QUAD_NONE:    the list above
//   QUAD_FRAMES:  frames whose cameras the host has proved equal (vr_internal.h
//                 frames_share_camera).  The four waves of workgroup g
//                 all take entry wave g's entries; wave w marches the 4x4-pixel quadrant
//                 (w & 1, w >> 1) of the 8x8 tile, and lane l is frame l & 3 at the pixel
//                 ((l >> 2) & 3, l >> 4) of it.  The four lanes of a quad -- the unit the
//                 texture addresser looks a b64 load up by -- march one ray and present one
//                 address, where four waves used to present it one after the other.  The ray
//                 runs on the common arguments; a lane's own part is its target pointer.
//                 Steps are not counted: the host sends a counted launch down the NF 4 path.
//   QUAD_SPLIT:   COL48 / BRICK4832 only (option quad_split): the same
//                 mapping, and the quad's lanes split the loads of two steps between them
//                 (march_pixel_quad_split) instead of each issuing all of them.
//   QUAD_STEPS:   the same launches (option quad_steps): the quad's lanes
//                 each fetch and blend one step of four and exchange the terms
//                 (march_pixel_quad_steps).
//   QUAD_PAIRS:   the same launches (option quad_pairs): a round's loads are
//                 issued in slice pairs, a split launch's addresses (march_pixel_quad_steps<QUAD_PAIRS>).
template <int LAYOUT, int WRAP, bool EARLY, bool ZO, int UM, int NF, int QM = QUAD_NONE>
__device__ __forceinline__ void regions_frames_body(const FramesArgs<NF>& g, const unsigned* __restrict__ tiles,
                                                    const int* __restrict__ hdr, int nwx, int deal, unsigned* lds)
{
    static_assert(NF == 2 || NF == 4, "a 4-wave workgroup is 4 / NF entry waves x NF frames");
    static_assert(QM == quad_kernel_mode(LAYOUT, NF, EARLY, ZO, UM, QM), "a mode this kernel has (a quad of lanes is four frames)");
    const int xcd = blockIdx.x & 7, wg = (int)(blockIdx.x >> 3);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int fr = wave, first = wg, w = wg;   // the frame, the workgroup's first entry wave, this wave's
    if constexpr (NF == 2) {
        fr = deal ? (wg & 1) : (wave & 1);
        first = deal ? (wg >> 1) * 4 : wg * 2;
        w = first + (deal ? wave : (wave >> 1));
    }
    const int begin = hdr[xcd], all = hdr[xcd + 1] - begin;
    const int marched = min(hdr[kRegionWork + xcd], all);
    MarchArgs a = g.c;   // this wave's frame (QUAD: the fill's wave = frame set only; the march's is q below)
    set_frame(&a, g.fr[fr]);
    const int count = a.empty_fill ? marched : all;
    if (a.empty_fill) fill_empty_tiles(a, tiles, begin, count, all, w, nwx);
    bool every = g.fr[0].empty_fill;   // the largest of the frames' marched counts: marched <= all
    for (int k = 1; k < NF; ++k) every = every && g.fr[k].empty_fill;
    if (first >= (every ? marched : all)) return;   // whole workgroup, before the barrier
    FastCtx f = fast_prologue<LAYOUT>(g.c, lds);   // volume and layout geometry: the frames' common part
    const int lane = threadIdx.x & 63;
    if constexpr (quad_is_quad(QM)) {
        // fr[0..3] equal the common part in all but the target and the counter: the ray and
        // the prologue (CORNERH's oz too) are the common part's, in SGPRs
        MarchArgs q = g.c;
        const int fl = lane & 3;
        void* out = g.fr[0].out;
        for (int k = 1; k < NF; ++k) out = fl == k ? g.fr[k].out : out;
        q.out = out;
        const int qx = (wave & 1) * 4 + ((lane >> 2) & 3), qy = (wave >> 1) * 4 + (lane >> 4);
        const int qcount = g.c.empty_fill ? marched : all;
        // no step count: a launch with a step counter takes the other instance (render_frames),
        // which keeps the two VGPRs of the per-lane sum out of this one
        for (int k = wg; wg < nwx && k < qcount; k += nwx) {
            const unsigned t = tiles[begin + k];
            const int tx = (int)(t & 0xffffu), ty = (int)(t >> 16);
            if constexpr (quad_rounds(QM)) march_pixel_quad_steps<LAYOUT, EARLY, ZO, UM, QM>(q, f, tx * 8 + qx, ty * 8 + qy, fl);
            else if constexpr (quad_splits(QM)) march_pixel_quad_split<LAYOUT, EARLY, ZO, UM>(q, f, tx * 8 + qx, ty * 8 + qy, fl);
            else (void)march_pixel<LAYOUT, WRAP, EARLY, ZO, UM>(q, f, tx * 8 + qx, ty * 8 + qy);
        }
        return;
    }
    if constexpr (LAYOUT == LAYOUT_CORNERH)   // the one per-frame part of the prologue
        for (int c = 0; c < 4; ++c) f.oz[c] = noise::in_vgpr(a.tap_T[c][2]);
    unsigned long long steps = 0;
    for (int k = w; w < nwx && k < count; k += nwx) {
        const unsigned t = tiles[begin + k];
        const int tx = (int)(t & 0xffffu), ty = (int)(t >> 16);
        steps += march_pixel<LAYOUT, WRAP, EARLY, ZO, UM>(a, f, tx * 8 + lane_x<LAYOUT>(lane),
                                                          ty * 8 + lane_y<LAYOUT>(lane));
    }
    if (a.step_counter) add_steps(a, steps);
}
// The occupancy floor of each instance is vr_internal.h quad_waves_floor's table (the _u kernels have no early-out).
template <int LAYOUT, int WRAP, bool EARLY, bool ZO, int NF, int QM = QUAD_NONE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(quad_waves_floor(QM, ZO, EARLY))))
void march_regions_frames(const FramesArgs<NF> g, const unsigned* __restrict__ tiles, const int* __restrict__ hdr, int nwx, int deal)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    regions_frames_body<LAYOUT, WRAP, EARLY, ZO, 0, NF, QM>(g, tiles, hdr, nwx, deal, lds);
}
template <int LAYOUT, int WRAP, bool EARLY, bool ZO, int UM, int NF, int QM = QUAD_NONE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(quad_waves_floor(QM, ZO, false))))
void march_regions_frames_u(const FramesArgs<NF> g, const unsigned* __restrict__ tiles, const int* __restrict__ hdr, int nwx, int deal)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    regions_frames_body<LAYOUT, WRAP, EARLY, ZO, UM, NF, QM>(g, tiles, hdr, nwx, deal, lds);
}


// ---- step-split rays (regions schedule) ----
// A wave whose rays march alone on their SIMD waits ~110 dependent memory
// round trips (the longest ray's steps): with a small share of the frame per
// GPU (N GPUs strong-scaled) there are too few waves to hide that.  Here K
// lanes share one ray: lane k computes the terms of steps k, k+K, k+2K, ...
// and the K terms of each round are added to `acc` in step order, so the sum
// is frag.glsl:71-73's sequential one, bit for bit.  A lane reaches its own
// ray points by the same sequence of fp32 adds as the reference loop (k adds,
// then K per round): P_i is never formed as P_0 + i*step.  The K lanes of a
// ray share n, so they loop, shuffle and stop together.  Lanes beyond the
// last step fetch the ray's entry point (in the box) and their terms are not
// added.
template <int LAYOUT, bool EARLY, bool ZO, int K, int UM = 0>
__device__ __forceinline__ unsigned march_pixel_split(const MarchArgs& a, const FastCtx& f, int x, int orow,
                                                      int k, int ray_lane)
{
    constexpr int R = 64 / K;
    const Ray r = setup_ray(a, x, orow);
    float uv[4] = {};
    if constexpr (UM != 0)
        for (int t = 0; t < 4; ++t)
            if ((UM >> t) & 1) uv[t] = noise::in_vgpr(a.uval[t]);
    const int n = r.n;
    f2 pxy = r.pxy;
    float pz = r.pz;
    for (int j = 0; j < k; ++j) { pxy = pxy + r.sxy; pz = pz + r.sz; }   // this lane's first step
    float acc = 0.0f;
    int i = 0;
    if (n > 0) {
        const bool mine0 = k < n;
        TapRaw c0 = fetch_u<UM, 0, LAYOUT, ZO>(a, f, mine0 ? pxy : r.pxy, mine0 ? pz : r.pz);
        TapRaw c1 = fetch_u<UM, 1, LAYOUT, ZO>(a, f, mine0 ? pxy : r.pxy, mine0 ? pz : r.pz);
        TapRaw c2 = fetch_u<UM, 2, LAYOUT, ZO>(a, f, mine0 ? pxy : r.pxy, mine0 ? pz : r.pz);
        TapRaw c3 = fetch_u<UM, 3, LAYOUT, ZO>(a, f, mine0 ? pxy : r.pxy, mine0 ? pz : r.pz);
        for (int base = 0; base < n; base += K) {
            for (int j = 0; j < K; ++j) { pxy = pxy + r.sxy; pz = pz + r.sz; }   // step base + K + k
            const bool mine = base + K + k < n;
            const f2 qxy = mine ? pxy : r.pxy;
            const float qz = mine ? pz : r.pz;
            const TapRaw n0 = fetch_u<UM, 0, LAYOUT, ZO>(a, f, qxy, qz), n1 = fetch_u<UM, 1, LAYOUT, ZO>(a, f, qxy, qz);
            const TapRaw n2 = fetch_u<UM, 2, LAYOUT, ZO>(a, f, qxy, qz), n3 = fetch_u<UM, 3, LAYOUT, ZO>(a, f, qxy, qz);
            const float t0 = blend_u<UM, 0, LAYOUT>(c0, uv), t1 = blend_u<UM, 1, LAYOUT>(c1, uv);
            const float t2 = blend_u<UM, 2, LAYOUT>(c2, uv), t3 = blend_u<UM, 3, LAYOUT>(c3, uv);
            const float term = ((t0 * t1) * (t2 + t3)) * a.scale;                        // :71-73
            bool stop = false;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float tj = __shfl(term, ray_lane + j * R);
                if (base + j < n && !stop) {
                    acc = acc + tj;
                    ++i;
                    if constexpr (EARLY) stop = acc > a.acc_limit;
                }
            }
            if constexpr (EARLY) {
                if (stop) break;
            }
            c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        }
    }
    if (r.live && k == 0) store_pixel(a, x, orow, n >= 0, ray_grey(a, acc));
    return (n > 0 && k == 0) ? (unsigned)i : 0u;
}

// Regions schedule with step-split rays: an 8x8 tile is K sub-blocks of 64/K
// rays (8x8, 8x4, 4x4, 4x2 pixels), one per wave; wave w of its XCD's nwx
// renders the units (tile, sub-block) w, w + nwx, ...  Lane = k * (64/K) + ray,
// so 4 adjacent lanes are a 2x2 pixel quad at the same step offset.
template <int LAYOUT, bool EARLY, bool ZO, int K, int UM = 0>
__global__ __launch_bounds__(kThreads) void march_regions_split(const MarchArgs a, const unsigned* __restrict__ tiles,
                                                               const int* __restrict__ hdr, int nwx)
{
    constexpr int R = 64 / K, SW = K >= 4 ? 4 : 8, SH = R / SW, NSX = 8 / SW;
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const int xcd = blockIdx.x & 7;
    const int w = (int)(blockIdx.x >> 3) * (kThreads / 64) + (threadIdx.x >> 6);
    const int begin = hdr[xcd], all = hdr[xcd + 1] - begin;
    const int marched = a.empty_fill ? min(hdr[kRegionWork + xcd], all) : all;
    if (a.empty_fill) fill_empty_tiles(a, tiles, begin, marched, all, w, nwx);
    const int units = marched * K;
    if ((int)(blockIdx.x >> 3) * (kThreads / 64) >= units) return;   // whole workgroup, before the barrier
    const FastCtx f = fast_prologue<LAYOUT>(a, lds);
#ifdef VR_TIMELINE
    const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
#endif
    const int lane = threadIdx.x & 63, k = lane / R, rho = lane % R;
    const int px = ((rho >> 2) % (SW / 2)) * 2 + (rho & 1), py = ((rho >> 2) / (SW / 2)) * 2 + ((rho >> 1) & 1);
    unsigned long long steps = 0;
    for (int u = w; w < nwx && u < units; u += nwx) {
        const unsigned t = tiles[begin + u / K];
        const int s = u % K;
        const int x = (int)(t & 0xffffu) * 8 + (s % NSX) * SW + px, orow = (int)(t >> 16) * 8 + (s / NSX) * SH + py;
        steps += march_pixel_split<LAYOUT, EARLY, ZO, K, UM>(a, f, x, orow, k, rho);
    }
#ifdef VR_TIMELINE
    timeline_record(t_begin, steps);
#endif
    if (a.step_counter) add_steps(a, steps);
}

// sc.split (2, 4 or 8) lanes per ray; one uniform channel: no loads for it (has_u_kernels)
template <int L>
hipError_t launch_regions_split(const MarchArgs& a, bool early, const Schedule& sc, size_t lds, hipStream_t s)
{
    const dim3 grid((unsigned)(8 * ((sc.map.nwx + 3) / 4))), block(kThreads);
    return with_value<2, 4, 8>(sc.split, [&](auto K) {
        auto launch = [&](auto E, auto Z, auto U) {
            hipLaunchKernelGGL((march_regions_split<L, E, Z, K, U>), grid, block, lds, s, a, sc.tiles, sc.hdr, sc.map.nwx);
            return hipGetLastError();
        };
        if constexpr (has_u_kernels(L))
            if (u_kernel_channel(early, a.zero_offsets, a.umask) >= 0)
                return with_value<1, 2, 4, 8>(a.umask, [&](auto U) { return launch(std::false_type{}, std::true_type{}, U); },
                                              hipErrorInvalidValue);
        return with_bool(early, [&](auto E) {
            return with_bool(a.zero_offsets, [&](auto Z) { return launch(E, Z, std::integral_constant<int, 0>{}); });
        });
    }, hipErrorInvalidValue);
}

// XCD-row schedule: one 8x8 tile per wave, 4 horizontally adjacent tiles per
// workgroup.  8-px tile rows are dealt to XCDs round-robin: XCD x walks rows
// x, x+8, ... (blockIdx % 8, speed-only).  Rows interleave, so the balance
// holds, and a row's neighbours share one L2.
template <int LAYOUT, int WRAP, bool EARLY>
__global__ __launch_bounds__(kThreads) void march_xcdrows(const MarchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const int tiles_x8 = (a.width + 7) >> 3, rows8 = (a.out_rows + 7) >> 3;
    const int groups = (tiles_x8 + 3) >> 2;
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int k = j / groups, gx = j - k * groups;
    const int ty = xcd + 8 * k;
    if (ty >= rows8) return;   // whole workgroup, before the barrier
    const FastCtx f = fast_prologue<LAYOUT>(a, lds);
    const int lane = threadIdx.x & 63, tx = gx * 4 + (threadIdx.x >> 6);
    unsigned long long steps = 0;
    if (tx < tiles_x8) steps = march_pixel<LAYOUT, WRAP, EARLY>(a, f, tx * 8 + lane_x<LAYOUT>(lane), ty * 8 + lane_y<LAYOUT>(lane));
    if (a.step_counter) add_steps(a, steps);
}

// Queue schedule: persistent waves pull 8x8 tiles from 8 queues, one per
// XCD group (blockIdx % 8, speed-only).  Queue q owns the 16-row tile pairs
// p = q, q+8, ..., walked column by column.  heads[] is zeroed by a memset
// before every launch.  Every wave leaves once its queue is drained, so the
// grid always completes.
template <int LAYOUT, int WRAP, bool EARLY>
__global__ __launch_bounds__(kThreads) void march_queue(const MarchArgs a, int* __restrict__ heads)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const FastCtx f = fast_prologue<LAYOUT>(a, lds);
    const int q = blockIdx.x & 7, lane = threadIdx.x & 63;
    const int tiles_x8 = (a.width + 7) >> 3, rows8 = (a.out_rows + 7) >> 3;
    const int pairs = (rows8 + 1) >> 1;
    const int per_pair = 2 * tiles_x8;
    const int count = q < pairs ? ((pairs - q + 7) >> 3) * per_pair : 0;
    unsigned long long steps = 0;
    for (;;) {
        int k = 0;
        if (lane == 0) k = atomicAdd(&heads[q], 1);
        k = __shfl(k, 0);
        if (k >= count) break;
        const int m = k / per_pair, rem = k - m * per_pair;
        const int row8 = 2 * (q + 8 * m) + (rem & 1), tx = rem >> 1;
        if (row8 >= rows8) continue;
        steps += march_pixel<LAYOUT, WRAP, EARLY>(a, f, tx * 8 + lane_x<LAYOUT>(lane), row8 * 8 + lane_y<LAYOUT>(lane));
    }
    if (a.step_counter) add_steps(a, steps);
}

template <int L, int W>
hipError_t launch_lw(const MarchArgs& a, bool early, const Schedule& sc, hipStream_t s)
{
    const size_t lds = march_lds_bytes<L>(a);
    const dim3 block(kThreads);
    const bool zo = a.zero_offsets;
    // the regions march, one lane per ray, G waves per workgroup: XCD x runs sc.map.nwx waves
    auto regions = [&](auto G) {
        const dim3 grid((unsigned)(8 * ((sc.map.nwx + G - 1) / G)));
        return with_bool(early, [&](auto E) { return with_bool(zo, [&](auto Z) {
            hipLaunchKernelGGL((march_regions<L, W, E, Z, G>), grid, dim3(64 * G), lds, s, a, sc.tiles, sc.hdr, sc.map.nwx);
            return hipGetLastError();
        }); });
    };
#if VR_EXPERIMENTS
    if (sc.kind == SCHED_STRIDED) {
        const int tiles = ((a.width + 7) >> 3) * ((a.out_rows + 7) >> 3);
        const int tpw = sc.tiles_per_wave > 0 ? sc.tiles_per_wave : 1;
        const int nw = (tiles + tpw - 1) / tpw;
        const dim3 grid((nw + 3) / 4);
        return with_bool(early, [&](auto E) {
            hipLaunchKernelGGL((march_strided<L, W, E>), grid, block, lds, s, a, 4 * (int)grid.x);
            return hipGetLastError();
        });
    }
#endif
    if (sc.kind == SCHED_RINGS) {
        const int tiles_x8 = (a.width + 7) >> 3, rows8 = (a.out_rows + 7) >> 3;
        const int cx = min(max(sc.center_x >> 3, 0), tiles_x8 - 1), cy = min(max(sc.center_y >> 3, 0), rows8 - 1);
        const int R = max(max(cx, tiles_x8 - 1 - cx), max(cy, rows8 - 1 - cy));
        const int npos = (2 * R + 1) * (2 * R + 1);
        const int tpw = sc.tiles_per_wave > 0 ? sc.tiles_per_wave : 1;
        const dim3 grid((unsigned)(((npos + tpw - 1) / tpw + 3) / 4));
        const int nw = 4 * (int)grid.x;
        return with_bool(early, [&](auto E) { return with_bool(zo, [&](auto Z) {
            hipLaunchKernelGGL((march_rings<L, W, E, Z>), grid, block, lds, s, a, cx, cy, nw, npos);
            return hipGetLastError();
        }); });
    }
    if constexpr (is_b4_family(L) || L == LAYOUT_ZPAIR || L == LAYOUT_CORNER8 || L == LAYOUT_CORNERH ||
                  L == LAYOUT_COL48Z) {
        if (sc.kind == SCHED_REGIONS && sc.split > 1) return launch_regions_split<L>(a, early, sc, lds, s);
    }
#if VR_EXPERIMENTS
    if constexpr (L == LAYOUT_COL48 || L == LAYOUT_BRICK4832 || L == LAYOUT_CORNERH) {
        if (sc.kind == SCHED_REGIONS && (sc.wg_waves == 8 || sc.wg_waves == 16))
            return with_value<8, 16>(sc.wg_waves, regions, hipErrorInvalidValue);
    }
#endif
    if constexpr (has_u_kernels(L)) {
        // one uniform channel (the reference recipe's G, TestMain.cpp:60/76):
        // its loads are skipped; other masks run the general kernel (exact too)
        const dim3 grid((unsigned)(8 * ((sc.map.nwx + 3) / 4)));
        if (sc.kind == SCHED_REGIONS && u_kernel_channel(early, zo, a.umask) >= 0)
            return with_value<1, 2, 4, 8>(a.umask, [&](auto U) {
                hipLaunchKernelGGL((march_regions_u<L, W, false, true, U>), grid, block, lds, s, a, sc.tiles, sc.hdr, sc.map.nwx);
                return hipGetLastError();
            }, hipErrorInvalidValue);
#ifdef VR_UM_EXPERIMENT
        if (sc.kind == SCHED_REGIONS && !early && zo && a.umask == 10) {   // G and A (timing experiment)
            hipLaunchKernelGGL((march_regions_u<L, W, false, true, 10>), grid, block, lds, s, a, sc.tiles, sc.hdr, sc.map.nwx);
            return hipGetLastError();
        }
#endif
    }
    if (sc.kind == SCHED_REGIONS) return regions(std::integral_constant<int, 4>{});
#if VR_EXPERIMENTS
    if (sc.kind == SCHED_XCDROWS) {
        const int groups = (((a.width + 7) >> 3) + 3) >> 2, rows8 = (a.out_rows + 7) >> 3;
        const dim3 grid(8 * ((rows8 + 7) / 8) * groups);
        return with_bool(early, [&](auto E) {
            hipLaunchKernelGGL((march_xcdrows<L, W, E>), grid, block, lds, s, a);
            return hipGetLastError();
        });
    }
    if (sc.kind == SCHED_QUEUE) {
        hipError_t e = hipMemsetAsync(sc.heads, 0, 32, s);
        if (e != hipSuccess) return e;
        const dim3 grid(256 * sc.waves_per_simd);
        return with_bool(early, [&](auto E) {
            hipLaunchKernelGGL((march_queue<L, W, E>), grid, block, lds, s, a, sc.heads);
            return hipGetLastError();
        });
    }
#endif
    const dim3 grid(a.num_blocks);
    return with_bool(early, [&](auto E) {
        hipLaunchKernelGGL((march_grid<L, W, E>), grid, block, lds, s, a);
        return hipGetLastError();
    });
}

// The multi-frame launch (march_regions_frames): the kernels of launch_lw's one-lane regions
// dispatch above -- one uniform channel (_u) or the general kernel -- for nf = 2 or 4 frames.
// The caller has checked that the frames share the plan and everything but the per-frame
// arguments (vr_render.cpp), that sc is a regions schedule without split, slab or wide
// workgroups, and that L is one of FrameLayouts.  XCD x runs
// sc.map.nwx entry waves, 4 / NF to a workgroup (regions_frames_body).
// quad (QuadMode): how the launch uses the lanes of a quad -- the same grid in every mode.  The
// kernel is instantiated with quad_kernel_mode (vr_internal.h) of every request; a request that
// function cuts down (other than QUAD_NONE for nf = 2 or an instance quad_instance excludes, past
// QUAD_FRAMES for a layout without the split fetch) is refused: the caller asks for the mode it
// gets, having proved frames_share_camera.
template <int L, int W>
hipError_t launch_frames_l(const MarchArgs& a, const FrameArgs* fr, int nf, bool early, const Schedule& sc, int deal, int quad,
                           hipStream_t s)
{
    if (quad_kernel_mode(L, nf, early, a.zero_offsets != 0, a.umask, quad) != quad) return hipErrorInvalidValue;   // no such kernel
    return with_value<2, kGroupFrames>(nf, [&](auto NF) { return with_value<QUAD_NONE, QUAD_FRAMES, QUAD_SPLIT, QUAD_STEPS, QUAD_PAIRS>(quad, [&](auto QD) {
        FramesArgs<NF> g;
        g.c = a;
        for (int k = 0; k < NF; ++k) g.fr[k] = fr[k];
        const size_t lds = march_lds_bytes<L>(a);
        const dim3 block(kThreads);
        static_assert(has_u_kernels(L), "every multi-frame layout has the _u kernels");
        static_assert(kThreads == 64 * 4, "a workgroup is 4 / NF entry waves x NF frames");
        const int nwx = sc.map.nwx;
        const int dl = NF == 4 ? 0 : deal;   // the four-frame kernel has one deal
        const dim3 grid((unsigned)(NF == 4 ? 8 * nwx : dl ? 16 * ((nwx + 3) / 4) : 8 * ((nwx + 1) / 2)));
        if (u_kernel_channel(early, a.zero_offsets, a.umask) >= 0)
            return with_value<1, 2, 4, 8>(a.umask, [&](auto U) {
                hipLaunchKernelGGL((march_regions_frames_u<L, W, false, true, U, NF, quad_kernel_mode(L, NF, false, true, U, QD)>), grid, block, lds, s, g, sc.tiles, sc.hdr, nwx, dl);
                return hipGetLastError();
            }, hipErrorInvalidValue);
        return with_bool(early, [&](auto E) { return with_bool(a.zero_offsets, [&](auto Z) {
            hipLaunchKernelGGL((march_regions_frames<L, W, E, Z, NF, quad_kernel_mode(L, NF, E, Z, 0, QD)>), grid, block, lds, s, g, sc.tiles, sc.hdr, nwx, dl);
            return hipGetLastError();
        }); });
    }, hipErrorInvalidValue); }, hipErrorInvalidValue);   // no kernel for this many frames or this mode
}

}  // namespace
}  // namespace vr
