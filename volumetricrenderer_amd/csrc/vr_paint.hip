// vr_paint.hip -- the brush kernels and their launchers: the edits applied in
// place to the installed volume's planar planes (vr_paint, vr_paint_stroke,
// vr_blur, vr_morph, vr_rank, vr_clone, vr_stamp, vr_remap, vr_stamp_affine,
// vr_clone_affine, vr_warp) and the statistics under a brush or in a box
// (vr_brush_stats, vr_box_stats, vr_stats_lut_device).  The arithmetic is the
// brush headers', which the host statements (vr_brush.cpp) include too: every
// kernel here reproduces its statement bit for bit.
#include <algorithm>
#include <cstddef>

#include "vr_affine.h"
#include "vr_blur.h"
#include "vr_brush.h"
#include "vr_clone.h"
#include "vr_internal.h"
#include "vr_morph.h"
#include "vr_rank.h"
#include "vr_remap.h"
#include "vr_stats.h"
#include "vr_volume_kernels.h"
#include "vr_warp.h"

namespace vr {
namespace {

__device__ __forceinline__ unsigned wave_index()   // of the workgroup, in a scalar register
{
    return (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// the first texel of the box's row (y, z) in a plane
__device__ __forceinline__ long long box_row(const PaintArgs& a, int y, int z)
{
    return ((long long)(a.o[2] + z) * a.ny + (a.o[1] + y)) * a.nx + a.o[0];
}

// The walk of the brush kernels with a thread per texel of the box (k_paint_planar's, below): rw = row(r, y, z)
// once per wave (index `wave`, wave-uniform: wave_index()) and box row r = (y, z) that the y and z terms of Q leave inside the ellipsoid, then
// texel(rw, x, q) on every lane whose texel x of that row, at Q = q, is inside.  Nothing returns early: a wave
// without a row falls through, so every thread reaches the barriers of the kernel around the walk.
template <class Row, class Texel>
__device__ __forceinline__ void walk_rows(const PaintArgs& a, unsigned wave, Row row, Texel texel)
{
    constexpr unsigned kWaves = kBlock / 64;
    const int lane = threadIdx.x & 63;
    const unsigned rows = (unsigned)a.e[1] * (unsigned)a.e[2];   // <= 511^2
    for (unsigned r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
        const int z = (int)(r / (unsigned)a.e[1]), y = (int)(r - (unsigned)z * (unsigned)a.e[1]);
        const unsigned long long qyz = brush::axis_term(a.d0[1] + y, a.k[1]) + brush::axis_term(a.d0[2] + z, a.k[2]);
        if (qyz > a.s) continue;
        const auto rw = row(r, y, z);
        for (int x = lane; x < a.e[0]; x += 64) {
            const unsigned long long q = qyz + brush::axis_term(a.d0[0] + x, a.k[0]);
            if (q > a.s) continue;
            texel(rw, x, q);
        }
    }
}

// the tail of a texel's channel: a store only where the byte changed, and the new byte into the thread's lo / hi
__device__ __forceinline__ void commit(uint8_t* p, unsigned old, unsigned nw, unsigned& lo, unsigned& hi)
{
    if (nw != old) *p = (uint8_t)nw;
    lo = min(lo, nw);
    hi = max(hi, nw);
}

// vr_paint: blend a brush (vr.h vr_brush; the arithmetic is vr_brush.h's, in
// integers and exact) into the planes, in place, over its bounding box clipped
// to the volume.  One thread per texel of the box: a wave takes a box row
// (y, z) at a time, consecutive lanes on consecutive x.  Q's y and z terms
// belong to the row -- wave-uniform, computed once per row, and a row they
// already put outside the ellipsoid costs nothing more; a texel outside it is
// left before any load.  An inside texel loads one byte per painted channel
// (strength != 0), blends, and stores only where the byte changed.  The NEW
// bytes go into mm as k_update_planar's do: a channel the brush leaves alone
// folds nothing, and a result equal to the old byte lies inside the range
// already, so neither can cost a uniform channel its bit.
__global__ __launch_bounds__(kBlock) void k_paint_planar(PaintArgs a, uint8_t* __restrict__ dst,
                                                         unsigned* __restrict__ mm)
{
    const long long plane = (long long)a.nx * a.ny * a.nz;
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    walk_rows(
        a, wave_index(), [&](unsigned, int y, int z) -> uint8_t* { return dst + box_row(a, y, z); },
        [&](uint8_t* __restrict__ row, int x, unsigned long long q) {
            const unsigned w = brush::weight(q, a.s, a.falloff);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                uint8_t* p = row + x + c * plane;
                const unsigned old = *p;
                commit(p, old, brush::blend(a.op, old, a.value[c], w * a.strength[c]), lo[c], hi[c]);
            }
        });
    fold_minmax(lo, hi, mm);
}

// vr_paint_stroke: the dabs of a (vr_internal.h StrokeArgs: validated, every one
// reaches the volume) applied in list order, as that many k_paint_planar
// launches would, with every texel loaded and stored once.  Ordered overlapping
// read-modify-writes need no atomics and no order between workgroups when every
// texel has exactly ONE owner thread:
//  * the work items are the rows (y, z) of each dab's clipped box; a wave takes
//    a row, consecutive lanes consecutive x, as in k_paint_planar;
//  * a texel reached through dab i's row is owned there iff no dab j < i has a
//    clipped box that holds it (else dab j's row reaches it too, and the lowest
//    such j owns it);
//  * the owner applies, in index order, every dab k >= i whose ellipsoid holds
//    the texel -- no dab below i can, their boxes do not hold it -- keeping each
//    painted channel's byte in a register from its one load to its one store
//    (only where the final byte differs); the final byte goes into lo / hi.
// Which dabs' boxes hold a row (y, z) is wave-uniform: lane k keeps dab k's y
// and z range, one compare per lane and a ballot give the 64-bit set in scalar
// registers, and the walk over its bits, the dabs' Terms and the y / z terms of
// Q are scalar work.  A candidate whose y / z terms already pass S costs a row
// nothing further; per lane there remain the x range and Q of the others.
__global__ __launch_bounds__(kBlock) void k_paint_stroke(StrokeArgs a, uint8_t* __restrict__ dst,
                                                         unsigned* __restrict__ mm)
{
    constexpr unsigned kWaves = kBlock / 64;
    const long long plane = (long long)a.nx * a.ny * a.nz;
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int cy = 0, ry = -1, cz = 0, rz = -1;   // lane k: dab k's rows (no dab: holds nothing)
    if (lane < a.count) {
        cy = a.dab[lane].centre[1]; ry = a.dab[lane].radius[1];
        cz = a.dab[lane].centre[2]; rz = a.dab[lane].radius[2];
    }
    const unsigned rows = a.row_begin[a.count];
    int i = 0;   // the dab of row r: a wave's rows ascend
    for (unsigned r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
        while (r >= a.row_begin[i + 1]) ++i;
        // dab i's clipped box (vr_brush.h clip; the centre is within a radius of the volume, so ints do)
        const vr_brush& bi = a.dab[i];
        const int x0 = max(bi.centre[0] - bi.radius[0], 0), x1 = min(bi.centre[0] + bi.radius[0], a.nx - 1);
        const int y0 = max(bi.centre[1] - bi.radius[1], 0), y1 = min(bi.centre[1] + bi.radius[1], a.ny - 1);
        const int z0 = max(bi.centre[2] - bi.radius[2], 0);
        const unsigned ey = (unsigned)(y1 - y0 + 1), rr = r - a.row_begin[i];
        const int z = z0 + (int)(rr / ey), y = y0 + (int)(rr % ey);
        const unsigned long long holds = __ballot(abs(y - cy) <= ry && abs(z - cz) <= rz);   // bit i is set
        const unsigned long long below = (1ull << i) - 1ull;
        uint8_t* __restrict__ row = dst + ((long long)z * a.ny + y) * a.nx;
        for (int x = x0 + lane; x <= x1; x += 64) {
            bool owned = true;
            for (unsigned long long m = holds & below; m; m &= m - 1ull) {
                const vr_brush& bj = a.dab[__builtin_ctzll(m)];
                owned = owned && abs(x - bj.centre[0]) > bj.radius[0];
            }
            if (__ballot(owned) == 0ull) continue;
            unsigned cur[4] = {0u, 0u, 0u, 0u}, old[4] = {0u, 0u, 0u, 0u}, have = 0u;   // have: the channels loaded
            for (unsigned long long m = holds & ~below; m; m &= m - 1ull) {
                const vr_brush& b = a.dab[__builtin_ctzll(m)];
                const brush::Terms t = brush::terms(b.radius);
                const unsigned long long qyz = brush::axis_term(y - b.centre[1], t.k[1]) +
                                               brush::axis_term(z - b.centre[2], t.k[2]);
                if (qyz > t.s) continue;
                const int dx = x - b.centre[0];
                if (!owned || abs(dx) > b.radius[0]) continue;
                const unsigned long long q = qyz + brush::axis_term(dx, t.k[0]);
                if (q > t.s) continue;
                const unsigned w = brush::weight(q, t.s, b.falloff);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (b.strength[c] == 0u) continue;
                    if (!(have & (1u << c))) {
                        old[c] = cur[c] = row[x + c * plane];
                        have |= 1u << c;
                    }
                    cur[c] = brush::blend(b.op, cur[c], b.value[c], w * b.strength[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (!(have & (1u << c))) continue;
                if (cur[c] != old[c]) row[x + c * plane] = (uint8_t)cur[c];
                lo[c] = min(lo[c], cur[c]);
                hi[c] = max(hi[c], cur[c]);
            }
        }
    }
    fold_minmax(lo, hi, mm);
}

// vr_blur, first launch: the new byte of every texel
// inside the brush, from the planes AS THEY ARE -- read only -- to the staging
// slabs (one per painted channel, shaped like the clipped box, x fastest).
// Nothing a mean reads is written by this launch, so the result does not
// depend on the order of the workgroups (a Jacobi step); k_blur_commit moves
// the bytes to the planes afterwards.
//
// A workgroup takes a kBlurTX x kBlurTY x kBlurTZ tile of the box; thread t
// owns the column (x, y) = (t % kBlurTX, t / kBlurTX) of it and its kBlurTZ
// texels.  The ellipsoid test and the weights need no memory: a tile with no
// texel inside leaves before any load.  Per painted channel:
//  1. the tile and its halo of H texels, coordinates clamped to the volume, go
//     from the plane to LDS once -- byte loads, the plane rows start at any
//     byte; consecutive lanes on consecutive x;
//  2. x: four adjacent sums of 2H + 1 bytes from the NW dwords that hold their
//     4 + 2H bytes, one 8-byte store of four 16-bit sums (<= 7 * 255);
//  3. y: a thread per (x, z) column of those slides the window over the
//     kBlurTY + 2H values it has read once; 16-bit sums (<= 49 * 255);
//  4. z: the owner slides the window over its column's kBlurTZ + 2H values --
//     the 32-bit sum, vr_blur.h's mean, the brush's SET blend with the old
//     byte (still in the staged tile), one byte store per inside texel.
// Lanes of a wave read consecutive 16-bit (or, in step 2, 32-bit) LDS words:
// no bank holds two different words of a lane group.
constexpr int kBlurTX = 32, kBlurTY = 8, kBlurTZ = 8;
static_assert(kBlurTX * kBlurTY == kBlock && kBlurTX % 4 == 0, "a thread per (x, y) column of the tile");

// The stage kernels' tiles of tx x ty x tz texels cover the clipped box, x fastest: how many there are (a workgroup
// each), and the first texel, in the box, of workgroup blockIdx.x's.
long long stage_tiles(const PaintArgs& a, int tx, int ty, int tz)
{
    return (long long)((a.e[0] + tx - 1) / tx) * ((a.e[1] + ty - 1) / ty) * ((a.e[2] + tz - 1) / tz);
}
struct Tile {
    int x, y, z;
};
__device__ __forceinline__ Tile tile_origin(const PaintArgs& a, int tx, int ty, int tz)
{
    const int ntx = (a.e[0] + tx - 1) / tx, nty = (a.e[1] + ty - 1) / ty;
    const int bt = blockIdx.x;
    return Tile{(bt % ntx) * tx, (bt / ntx % nty) * ty, (bt / (ntx * nty)) * tz};
}

template <int H>
__global__ __launch_bounds__(kBlock) void k_blur_stage(PaintArgs a, const uint8_t* __restrict__ src,
                                                       uint8_t* __restrict__ stage)
{
    constexpr int W = 2 * H + 1;
    constexpr int XH = kBlurTX + 2 * H, YH = kBlurTY + 2 * H, ZH = kBlurTZ + 2 * H;
    constexpr int XP = (XH + 3) / 4 * 4;    // the staged rows' pitch: whole dwords
    constexpr int NW = (4 + 2 * H + 3) / 4;   // dwords that hold the bytes of four adjacent x sums
    static_assert(kBlurTX - 4 + 4 * NW <= XP, "step 2 reads inside its row");
    __shared__ uint32_t raw32[ZH * YH * XP / 4];
    __shared__ __align__(8) uint16_t sx[ZH * YH * kBlurTX];
    __shared__ uint16_t sxy[ZH * kBlurTY * kBlurTX];
    uint8_t* raw = reinterpret_cast<uint8_t*>(raw32);

    const int tid = threadIdx.x, lx = tid % kBlurTX, ly = tid / kBlurTX;
    const Tile t0 = tile_origin(a, kBlurTX, kBlurTY, kBlurTZ);
    const int tx0 = t0.x, ty0 = t0.y, tz0 = t0.z;
    const int x = tx0 + lx, y = ty0 + ly;   // in the box

    // the weights of the owned texels: 0 outside the ellipsoid or the box (an inside texel's is at least 1)
    unsigned wgt[kBlurTZ];
    const bool column = x < a.e[0] && y < a.e[1];
    const unsigned long long qxy =
        column ? brush::axis_term(a.d0[0] + x, a.k[0]) + brush::axis_term(a.d0[1] + y, a.k[1]) : 0ull;
    bool any = false;
#pragma unroll
    for (int z = 0; z < kBlurTZ; ++z) {
        wgt[z] = 0u;
        if (column && tz0 + z < a.e[2]) {
            const unsigned long long q = qxy + brush::axis_term(a.d0[2] + tz0 + z, a.k[2]);
            if (q <= a.s) wgt[z] = brush::weight(q, a.s, a.falloff);
        }
        any = any || wgt[z] != 0u;
    }
    if (!__syncthreads_or(any ? 1 : 0)) return;

    const long long plane = (long long)a.nx * a.ny * a.nz;
    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
    int k = 0;   // the channel's slab
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        if (a.strength[c] == 0u) continue;
        const uint8_t* __restrict__ p = src + c * plane;
        for (int i = tid; i < ZH * YH * XH; i += kBlock) {
            const int xi = i % XH, t = i / XH, yi = t % YH, zi = t / YH;
            const int gx = clampi(a.o[0] + tx0 - H + xi, 0, a.nx - 1), gy = clampi(a.o[1] + ty0 - H + yi, 0, a.ny - 1),
                      gz = clampi(a.o[2] + tz0 - H + zi, 0, a.nz - 1);
            raw[(zi * YH + yi) * XP + xi] = p[((long long)gz * a.ny + gy) * a.nx + gx];
        }
        __syncthreads();
        for (int i = tid; i < ZH * YH * (kBlurTX / 4); i += kBlock) {
            const int xq = i % (kBlurTX / 4), r = i / (kBlurTX / 4);   // r: the row (zi, yi)
            const uint32_t* w32 = raw32 + r * (XP / 4) + xq;
            unsigned b[4 * NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const uint32_t v = w32[j];
                b[4 * j] = v & 255u; b[4 * j + 1] = (v >> 8) & 255u; b[4 * j + 2] = (v >> 16) & 255u; b[4 * j + 3] = v >> 24;
            }
            unsigned s0 = 0u;
#pragma unroll
            for (int j = 0; j < W; ++j) s0 += b[j];
            const unsigned s1 = s0 - b[0] + b[W], s2 = s1 - b[1] + b[W + 1], s3 = s2 - b[2] + b[W + 2];
            *reinterpret_cast<uint2*>(&sx[r * kBlurTX + 4 * xq]) = make_uint2(s0 | (s1 << 16), s2 | (s3 << 16));
        }
        __syncthreads();
        for (int i = tid; i < ZH * kBlurTX; i += kBlock) {
            const int xx = i % kBlurTX, zi = i / kBlurTX;
            const uint16_t* col = sx + zi * YH * kBlurTX + xx;
            unsigned v[YH];
#pragma unroll
            for (int j = 0; j < YH; ++j) v[j] = col[j * kBlurTX];
            unsigned s = 0u;
#pragma unroll
            for (int j = 0; j < W; ++j) s += v[j];
#pragma unroll
            for (int yo = 0; yo < kBlurTY; ++yo) {
                if (yo > 0) s += v[yo + W - 1] - v[yo - 1];
                sxy[(zi * kBlurTY + yo) * kBlurTX + xx] = (uint16_t)s;
            }
        }
        __syncthreads();
        {
            const uint16_t* col = sxy + ly * kBlurTX + lx;
            unsigned v[ZH];
#pragma unroll
            for (int j = 0; j < ZH; ++j) v[j] = col[j * kBlurTY * kBlurTX];
            unsigned s = 0u;
#pragma unroll
            for (int j = 0; j < W; ++j) s += v[j];
            uint8_t* __restrict__ out = stage + (size_t)k * slab;
#pragma unroll
            for (int z = 0; z < kBlurTZ; ++z) {
                if (z > 0) s += v[z + W - 1] - v[z - 1];
                if (wgt[z] == 0u) continue;
                const unsigned old = raw[((z + H) * YH + ly + H) * XP + lx + H];
                const unsigned nw = brush::blend(VR_BRUSH_SET, old, blur::mean(s, H), wgt[z] * a.strength[c]);
                out[((size_t)(tz0 + z) * (size_t)a.e[1] + (size_t)y) * (size_t)a.e[0] + (size_t)x] = (uint8_t)nw;
            }
        }
        ++k;
        __syncthreads();   // the next channel rewrites the tile
    }
}

// vr_blur, second launch: k_paint_planar's rows and lanes, with the new byte
// of an inside texel loaded from the staging slabs (k_blur_stage wrote exactly
// those) instead of blended: a store only where it differs from the old byte,
// and the new bytes folded into mm.
__global__ __launch_bounds__(kBlock) void k_blur_commit(PaintArgs a, const uint8_t* __restrict__ stage,
                                                        uint8_t* __restrict__ dst, unsigned* __restrict__ mm)
{
    const long long plane = (long long)a.nx * a.ny * a.nz;
    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    struct Rows {
        uint8_t* __restrict__ row;
        const uint8_t* __restrict__ srow;
    };
    walk_rows(
        a, wave_index(), [&](unsigned r, int y, int z) { return Rows{dst + box_row(a, y, z), stage + (size_t)r * (size_t)a.e[0]}; },
        [&](const Rows& rw, int x, unsigned long long) {
            int k = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                uint8_t* p = rw.row + x + c * plane;
                commit(p, *p, rw.srow[(size_t)k * slab + (size_t)x], lo[c], hi[c]);
                ++k;
            }
        });
    fold_minmax(lo, hi, mm);
}

// vr_morph, first launch: k_blur_stage's contract --
// the planes read only, the new byte of every inside texel to the staging
// slabs in the same shape, so k_blur_commit follows unchanged -- with the
// minimum (erode) or maximum (dilate) over the (2H + 1)^3 cube as the value.
//
// Every partial result is a byte, so the kernel works on dwords of four
// adjacent x throughout.  A dword is split once into its even and its odd
// bytes, each pair in the 16-bit halves of a register (Quad), and the extremum
// of two Quads is two packed 16-bit instructions for four texels.  Min and max
// are idempotent, so a window is covered by overlapping parts: pairs, pairs of
// pairs, and two of those (morph_window) -- 2, 3, 3 extrema per output for
// W = 3, 5, 7.
//
// The tile is k_blur_stage's, kMorphTX x kMorphTY x kMorphTZ = 32 x 8 x 8;
// thread t owns the four x of dword t % 8 in row t / 8 % 8 at the two z of its
// wave (t / 64).  A tile with no texel inside leaves before any load.  Per
// painted channel:
//  1. tile and halo, coordinates clamped to the volume, from the plane to LDS:
//     four byte loads and ONE dword store per lane (the plane rows start at
//     any byte);
//  2. the owners take their old bytes into registers; x: a lane per dword of a
//     staged row reads the NW dwords that hold its 4 + 2H bytes and stores the
//     four extrema as one dword -- the pairs of even bytes (2k, 2k + 2) and of
//     odd bytes (2k + 1, 2k + 3) are the operands, 2H + 1 packed extrema;
//  3. y: a lane per (dword, z row, half of the tile's y) reads 4 + 2H dwords
//     down the column and stores four; the result overwrites the staged tile,
//     which nothing reads any more;
//  4. z: the owner reads 2 + 2H dwords down its column, blends (the brush's
//     SET blend) and stores the new bytes of its inside texels: one dword
//     where all four are inside and the address allows it, else bytes.
// The z pitch of both partial arrays is padded by 8 dwords: the four z rows
// that a 32-lane group of step 3 touches then fall on different banks.
constexpr int kMorphTX = 32, kMorphTY = 8, kMorphTZ = 8;
constexpr int kMorphQ = kMorphTX / 4;   // dwords per tile row
static_assert(kMorphQ * kMorphTY * (kMorphTZ / 2) == kBlock && kMorphTY % 4 == 0, "a thread per dword and z pair of the tile");

typedef unsigned short morph_u16x2 __attribute__((ext_vector_type(2)));
struct Quad {
    morph_u16x2 e, o;   // bytes 0, 2 and bytes 1, 3 of a dword
};

template <bool DILATE>
__device__ __forceinline__ morph_u16x2 morph_ext(morph_u16x2 a, morph_u16x2 b)
{
    return DILATE ? __builtin_elementwise_max(a, b) : __builtin_elementwise_min(a, b);
}
template <bool DILATE>
__device__ __forceinline__ uint32_t morph_ext(uint32_t a, uint32_t b)   // two 16-bit lanes in a dword
{
    return __builtin_bit_cast(uint32_t, morph_ext<DILATE>(__builtin_bit_cast(morph_u16x2, a), __builtin_bit_cast(morph_u16x2, b)));
}
template <bool DILATE>
__device__ __forceinline__ Quad morph_ext(Quad a, Quad b)
{
    return Quad{morph_ext<DILATE>(a.e, b.e), morph_ext<DILATE>(a.o, b.o)};
}
__device__ __forceinline__ Quad morph_split(uint32_t v)
{
    return Quad{__builtin_bit_cast(morph_u16x2, v & 0x00ff00ffu), __builtin_bit_cast(morph_u16x2, (v >> 8) & 0x00ff00ffu)};
}
__device__ __forceinline__ uint32_t morph_join(Quad q)
{
    return __builtin_bit_cast(uint32_t, q.e) | (__builtin_bit_cast(uint32_t, q.o) << 8);
}

// out[j] = the extremum of in[j .. j + W - 1], W = 3, 5 or 7
template <int W, int N, bool DILATE>
__device__ __forceinline__ void morph_window(const Quad (&in)[N + W - 1], Quad (&out)[N])
{
    constexpr int L = N + W - 1;
    Quad m2[L - 1];
#pragma unroll
    for (int j = 0; j < L - 1; ++j) m2[j] = morph_ext<DILATE>(in[j], in[j + 1]);
    if constexpr (W < 4) {
#pragma unroll
        for (int j = 0; j < N; ++j) out[j] = morph_ext<DILATE>(m2[j], m2[j + W - 2]);
    } else {
        Quad m4[L - 3];
#pragma unroll
        for (int j = 0; j < L - 3; ++j) m4[j] = morph_ext<DILATE>(m2[j], m2[j + 2]);
#pragma unroll
        for (int j = 0; j < N; ++j) out[j] = morph_ext<DILATE>(m4[j], m4[j + W - 4]);
    }
}

// The weights of the texels a thread of k_morph_stage / k_rank_stage owns -- four adjacent x from (x, y, z) on, at z
// and z + 1, in the box: 0 outside the ellipsoid or the box (an inside texel's is at least 1).
struct QuadWeights {
    unsigned w[2][4];   // [z offset][x offset]
};
__device__ __forceinline__ QuadWeights quad_weights(const PaintArgs& a, int x, int y, int z)
{
    QuadWeights r;
    const unsigned long long qy = y < a.e[1] ? brush::axis_term(a.d0[1] + y, a.k[1]) : 0ull;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r.w[i][j] = 0u;
            if (y < a.e[1] && z + i < a.e[2] && x + j < a.e[0]) {
                const unsigned long long q =
                    qy + brush::axis_term(a.d0[0] + x + j, a.k[0]) + brush::axis_term(a.d0[2] + z + i, a.k[2]);
                if (q <= a.s) r.w[i][j] = brush::weight(q, a.s, a.falloff);
            }
        }
    return r;
}

// Step 1 of k_morph_stage / k_rank_stage: the tile at t of the box and its halo of H texels, coordinates clamped to
// the volume, from the plane p to LDS dwords -- rows of XPW dwords, slices ZPITCH dwords apart.  Four byte loads and
// ONE dword store per lane (the plane rows start at any byte).
template <int H, int ZPITCH>
__device__ __forceinline__ void load_tile_halo(const PaintArgs& a, const uint8_t* __restrict__ p, Tile t, uint32_t* raw32)
{
    constexpr int XH = kMorphTX + 2 * H, YH = kMorphTY + 2 * H, ZH = kMorphTZ + 2 * H;
    constexpr int XPW = (XH + 3) / 4;
    for (int i = threadIdx.x; i < ZH * YH * XPW; i += kBlock) {
        const int xw = i % XPW, r = i / XPW, yi = r % YH, zi = r / YH;
        const int gy = clampi(a.o[1] + t.y - H + yi, 0, a.ny - 1), gz = clampi(a.o[2] + t.z - H + zi, 0, a.nz - 1);
        const uint8_t* __restrict__ row = p + ((long long)gz * a.ny + gy) * a.nx;
        const int gx = a.o[0] + t.x - H + 4 * xw;
        uint32_t v = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) v |= (uint32_t)row[clampi(gx + j, 0, a.nx - 1)] << (8 * j);
        raw32[i + zi * (ZPITCH - YH * XPW)] = v;   // = zi * ZPITCH + yi * XPW + xw
    }
}

template <int H, bool DILATE>
__global__ __launch_bounds__(kBlock) void k_morph_stage(PaintArgs a, const uint8_t* __restrict__ src,
                                                        uint8_t* __restrict__ stage)
{
    constexpr int W = 2 * H + 1;
    constexpr int XH = kMorphTX + 2 * H, YH = kMorphTY + 2 * H, ZH = kMorphTZ + 2 * H;
    constexpr int XPW = (XH + 3) / 4;      // dwords of a staged row
    constexpr int NW = (H + 1) / 2 + 1;    // dwords that hold the 4 + 2H bytes of four adjacent windows
    constexpr int RAW = ZH * YH * XPW;     // the staged tile, in dwords
    constexpr int EXZ = YH * kMorphQ + 8;  // z pitch of the x extrema
    constexpr int EXYZ = kMorphTY * kMorphQ + 8;   // z pitch of the x-y extrema
    static_assert(kMorphQ - 1 + NW <= XPW, "step 2 reads inside its row");
    static_assert(ZH * EXYZ <= RAW, "the x-y extrema fit in the staged tile they overwrite");
    __shared__ uint32_t lds[RAW + ZH * EXZ];
    uint32_t* const raw32 = lds;
    uint32_t* const ex = lds + RAW;
    uint32_t* const exy = lds;

    const int tid = threadIdx.x, xq = tid % kMorphQ, ly = tid / kMorphQ % kMorphTY, zp = tid / (kMorphQ * kMorphTY);
    const Tile t0 = tile_origin(a, kMorphTX, kMorphTY, kMorphTZ);
    const int x = t0.x + 4 * xq, y = t0.y + ly, z = t0.z + 2 * zp;   // the first owned texel, in the box

    const QuadWeights qw = quad_weights(a, x, y, z);
    const unsigned (&wgt)[2][4] = qw.w;
    bool any = false;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) any = any || wgt[i][j] != 0u;
    if (!__syncthreads_or(any ? 1 : 0)) return;

    const long long plane = (long long)a.nx * a.ny * a.nz;
    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
    int k = 0;   // the channel's slab
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        if (a.strength[c] == 0u) continue;
        load_tile_halo<H, YH * XPW>(a, src + c * plane, t0, raw32);
        __syncthreads();
        uint32_t old[2];   // the owned texels' bytes before the call
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t* w32 = raw32 + ((2 * zp + i + H) * YH + ly + H) * XPW + xq;
            old[i] = (uint32_t)((((unsigned long long)w32[1] << 32) | w32[0]) >> (8 * H));
        }
        for (int i = tid; i < ZH * YH * kMorphQ; i += kBlock) {
            const int q = i % kMorphQ, r = i / kMorphQ, yi = r % YH, zi = r / YH;   // r: the row (zi, yi)
            const uint32_t* w32 = raw32 + r * XPW + q;
            uint32_t ev[NW], od[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const uint32_t v = w32[j];
                ev[j] = v & 0x00ff00ffu;
                od[j] = (v >> 8) & 0x00ff00ffu;
            }
            // pe[n] = bytes (2n, 2n + 2), po[n] = bytes (2n + 1, 2n + 3) of the row from the dword's first byte on
            uint32_t pe[H + 1], po[H + 1];
#pragma unroll
            for (int n = 0; n <= H; ++n) {
                pe[n] = n % 2 ? (ev[n / 2] >> 16) | (ev[n / 2 + 1] << 16) : ev[n / 2];
                po[n] = n % 2 ? (od[n / 2] >> 16) | (od[n / 2 + 1] << 16) : od[n / 2];
            }
            // texels 0 and 2 see bytes 0..2H and 2..2H + 2: pe[0..H] and po[0..H - 1]; texels 1 and 3: po[0..H], pe[1..H]
            uint32_t both = morph_ext<DILATE>(pe[1], po[0]);
#pragma unroll
            for (int n = 1; n < H; ++n) both = morph_ext<DILATE>(both, morph_ext<DILATE>(pe[n + 1], po[n]));
            ex[zi * EXZ + yi * kMorphQ + q] = morph_ext<DILATE>(both, pe[0]) | (morph_ext<DILATE>(both, po[H]) << 8);
        }
        __syncthreads();
        for (int i = tid; i < ZH * kMorphQ * (kMorphTY / 4); i += kBlock) {
            const int q = i % kMorphQ, t = i / kMorphQ, zi = t % ZH, yq = t / ZH;
            const uint32_t* col = ex + zi * EXZ + 4 * yq * kMorphQ + q;
            Quad in[4 + W - 1], out[4];
#pragma unroll
            for (int j = 0; j < 4 + W - 1; ++j) in[j] = morph_split(col[j * kMorphQ]);
            morph_window<W, 4, DILATE>(in, out);
#pragma unroll
            for (int j = 0; j < 4; ++j) exy[zi * EXYZ + (4 * yq + j) * kMorphQ + q] = morph_join(out[j]);
        }
        __syncthreads();
        {
            const uint32_t* col = exy + 2 * zp * EXYZ + ly * kMorphQ + xq;
            Quad in[2 + W - 1], out[2];
#pragma unroll
            for (int j = 0; j < 2 + W - 1; ++j) in[j] = morph_split(col[j * EXYZ]);
            morph_window<W, 2, DILATE>(in, out);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if ((wgt[i][0] | wgt[i][1] | wgt[i][2] | wgt[i][3]) == 0u) continue;
                const uint32_t m = morph_join(out[i]);
                uint32_t nw = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    nw |= brush::blend(VR_BRUSH_SET, (old[i] >> (8 * j)) & 255u, (m >> (8 * j)) & 255u, wgt[i][j] * a.strength[c])
                          << (8 * j);
                uint8_t* __restrict__ o8 =
                    stage + (size_t)k * slab + ((size_t)(z + i) * (size_t)a.e[1] + (size_t)y) * (size_t)a.e[0] + (size_t)x;
                if (wgt[i][0] && wgt[i][1] && wgt[i][2] && wgt[i][3] && (reinterpret_cast<uintptr_t>(o8) & 3u) == 0u) {
                    *reinterpret_cast<uint32_t*>(o8) = nw;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (wgt[i][j]) o8[j] = (uint8_t)(nw >> (8 * j));
                }
            }
        }
        ++k;
        __syncthreads();   // the next channel rewrites the tile
    }
}

// vr_rank, first launch: k_blur_stage's contract -- the
// planes read only, the new byte of every inside texel to the staging slabs in
// the same shape, so k_blur_commit follows unchanged -- with the rank-th
// smallest byte of the (2H + 1)^3 cube as the value.  A rank is not separable:
// the selection runs over the whole cube, by vr_rank.h's bisection on the byte,
// eight rounds of "how many neighbours lie below the candidate".
//
// The tile is the morph's, 32 x 8 x 8; thread t owns the four x of dword t % 8
// at the two z of pair t / 8 % 4 in row t / 32.  The two z share 2H of their
// 2H + 2 slices, so a staged row is read once per round for both.  A tile with
// no texel inside leaves before any load.  Per painted channel:
//  1. tile and halo, coordinates clamped to the volume, from the plane to LDS,
//     as step 1 of k_morph_stage;
//  2. every lane with an inside texel runs the eight rounds.  Per round and
//     staged row of its windows it reads the NW dwords that hold the 4 + 2H
//     bytes of its four windows and splits them into pairs of even and of odd
//     bytes two apart in 16-bit halves (the morph's pe / po): pair n of one
//     parity is byte n of the windows of texels 0 and 2, or of 1 and 3.  The
//     candidates of those two texels sit in the halves of one register, and
//     (pair - candidates) has bit 15 of a half set exactly when that byte is
//     below that candidate (vr_rank.h below), so a packed subtract, a packed
//     shift and a packed add count two comparisons: 2 (2H + 1) triples per
//     row and quad.  A count is at most 343 and fits its half.  After the
//     last row vr_rank.h advance decides the round's bit per texel;
//  3. the SET blend and the store of step 4 of k_morph_stage.
// A lane none of whose eight texels is inside does no selection; a quad none
// of whose four is inside is skipped.  A texel outside that shares a quad with
// one inside rides along in the packed halves at no cost and is not stored.
// The 32 lanes of an LDS read group are 8 dwords x 4 z pairs of one row: the z
// pitch is padded until twice the pitch is 8 or 24 mod 32 dwords, which puts
// the four pairs on disjoint banks.
constexpr int rank_z_pitch(int dwords)
{
    while (dwords % 16 != 4 && dwords % 16 != 12) ++dwords;
    return dwords;
}

template <int H>
__global__ __launch_bounds__(kBlock) void k_rank_stage(PaintArgs a, unsigned rank, const uint8_t* __restrict__ src,
                                                       uint8_t* __restrict__ stage)
{
    constexpr int W = 2 * H + 1;
    constexpr int XH = kMorphTX + 2 * H, YH = kMorphTY + 2 * H, ZH = kMorphTZ + 2 * H;
    constexpr int XPW = (XH + 3) / 4;        // dwords of a staged row
    constexpr int NW = (H + 1) / 2 + 1;      // dwords that hold the 4 + 2H bytes of four adjacent windows
    constexpr int ZP = rank_z_pitch(YH * XPW);   // z pitch of the staged tile, in dwords
    static_assert(kMorphQ - 1 + NW <= XPW, "step 2 reads inside its row");
    static_assert(kMorphQ * (kMorphTZ / 2) * kMorphTY == kBlock, "a thread per dword and z pair of the tile");
    static_assert(W * W * W < 32768, "a count fits 15 bits of its half");
    __shared__ uint32_t raw32[ZH * ZP];

    const int tid = threadIdx.x, xq = tid % kMorphQ, zp = tid / kMorphQ % (kMorphTZ / 2), ly = tid / (kMorphQ * (kMorphTZ / 2));
    const Tile t0 = tile_origin(a, kMorphTX, kMorphTY, kMorphTZ);
    const int x = t0.x + 4 * xq, y = t0.y + ly, z = t0.z + 2 * zp;   // the first owned texel, in the box

    const QuadWeights qw = quad_weights(a, x, y, z);
    const unsigned (&wgt)[2][4] = qw.w;
    bool act[2];   // the quad at z + i has a texel inside
#pragma unroll
    for (int i = 0; i < 2; ++i) act[i] = (wgt[i][0] | wgt[i][1] | wgt[i][2] | wgt[i][3]) != 0u;
    if (!__syncthreads_or(act[0] || act[1] ? 1 : 0)) return;

    const long long plane = (long long)a.nx * a.ny * a.nz;
    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
    int k = 0;   // the channel's slab
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        if (a.strength[c] == 0u) continue;
        load_tile_halo<H, ZP>(a, src + c * plane, t0, raw32);
        __syncthreads();
        if (act[0] || act[1]) {
            // lo02[i], lo13[i]: the bits found so far of texels 0 and 2, and 1 and 3, of the quad at z + i, in halves
            uint32_t lo02[2] = {0u, 0u}, lo13[2] = {0u, 0u};
#pragma unroll 1
            for (unsigned bit = 128u; bit != 0u; bit >>= 1) {
                morph_u16x2 c02[2], c13[2], n02[2], n13[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    c02[i] = __builtin_bit_cast(morph_u16x2, lo02[i] | bit * 0x00010001u);
                    c13[i] = __builtin_bit_cast(morph_u16x2, lo13[i] | bit * 0x00010001u);
                    n02[i] = n13[i] = morph_u16x2{0, 0};
                }
#pragma unroll 1
                for (int zi = 0; zi < W + 1; ++zi) {
                    const bool use[2] = {act[0] && zi < W, act[1] && zi > 0};   // slice zi lies in the window of z + i
                    const uint32_t* rows = raw32 + (2 * zp + zi) * ZP + ly * XPW + xq;
#pragma unroll
                    for (int dy = 0; dy < W; ++dy) {
                        const uint32_t* w32 = rows + dy * XPW;
                        uint32_t ev[NW], od[NW];
#pragma unroll
                        for (int j = 0; j < NW; ++j) {
                            const uint32_t v = w32[j];
                            ev[j] = v & 0x00ff00ffu;
                            od[j] = (v >> 8) & 0x00ff00ffu;
                        }
                        // pe[n] = bytes (2n, 2n + 2), po[n] = bytes (2n + 1, 2n + 3) of the row from the dword's first byte on
                        morph_u16x2 pe[H + 1], po[H + 1];
#pragma unroll
                        for (int n = 0; n <= H; ++n) {
                            pe[n] = __builtin_bit_cast(morph_u16x2, n % 2 ? (ev[n / 2] >> 16) | (ev[n / 2 + 1] << 16) : ev[n / 2]);
                            po[n] = __builtin_bit_cast(morph_u16x2, n % 2 ? (od[n / 2] >> 16) | (od[n / 2 + 1] << 16) : od[n / 2]);
                        }
                        // texels 0 and 2 see bytes 0..2H and 2..2H + 2: pe[0..H] and po[0..H - 1]; texels 1 and 3: po[0..H], pe[1..H]
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            if (!use[i]) continue;
#pragma unroll
                            for (int n = 0; n <= H; ++n) {
                                n02[i] += (pe[n] - c02[i]) >> 15;
                                n13[i] += (po[n] - c13[i]) >> 15;
                            }
#pragma unroll
                            for (int n = 0; n < H; ++n) {
                                n02[i] += (po[n] - c02[i]) >> 15;
                                n13[i] += (pe[n + 1] - c13[i]) >> 15;
                            }
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const uint32_t m02 = __builtin_bit_cast(uint32_t, n02[i]), m13 = __builtin_bit_cast(uint32_t, n13[i]);
                    lo02[i] = rank::advance(lo02[i] & 0xffffu, bit, m02 & 0xffffu, rank) |
                              rank::advance(lo02[i] >> 16, bit, m02 >> 16, rank) << 16;
                    lo13[i] = rank::advance(lo13[i] & 0xffffu, bit, m13 & 0xffffu, rank) |
                              rank::advance(lo13[i] >> 16, bit, m13 >> 16, rank) << 16;
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (!act[i]) continue;
                const uint32_t* w32 = raw32 + (2 * zp + i + H) * ZP + (ly + H) * XPW + xq;
                const uint32_t old = (uint32_t)((((unsigned long long)w32[1] << 32) | w32[0]) >> (8 * H));
                const uint32_t m = lo02[i] | (lo13[i] << 8);
                uint32_t nw = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    nw |= brush::blend(VR_BRUSH_SET, (old >> (8 * j)) & 255u, (m >> (8 * j)) & 255u, wgt[i][j] * a.strength[c])
                          << (8 * j);
                uint8_t* __restrict__ o8 =
                    stage + (size_t)k * slab + ((size_t)(z + i) * (size_t)a.e[1] + (size_t)y) * (size_t)a.e[0] + (size_t)x;
                if (wgt[i][0] && wgt[i][1] && wgt[i][2] && wgt[i][3] && (reinterpret_cast<uintptr_t>(o8) & 3u) == 0u) {
                    *reinterpret_cast<uint32_t*>(o8) = nw;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (wgt[i][j]) o8[j] = (uint8_t)(nw >> (8 * j));
                }
            }
        }
        ++k;
        __syncthreads();   // the next channel rewrites the tile
    }
}

// vr_clone: k_paint_planar with the value of a texel
// read from the volume's own texel at the mapped, clamped position
// (vr_clone.h source).  Rows and lanes are k_paint_planar's.  The source row's
// y and z belong to the box row -- wave-uniform, computed once per row; x is
// per lane: consecutive lanes read consecutive bytes of ONE source row, rising
// or (mirrored) falling, until the clamp pins them to its first or last byte.
// A row or a texel outside the ellipsoid is left before any load.
//
// STAGE = false (k_clone_direct): `out` is the planes themselves.  The host has
// checked (vr_clone.h direct) that no texel of the box is read, so the bytes
// read are the bytes before the call whatever the order of the waves; a store
// goes only where the byte changed and the new bytes are folded into lo / hi.
// STAGE = true (k_clone_stage): the planes are read only and the new byte of
// every inside texel and painted channel goes to the staging slabs, exactly as
// k_blur_stage and k_morph_stage leave them; k_blur_commit follows.
template <bool STAGE>
__device__ __forceinline__ void clone_rows(const CloneArgs& g, const uint8_t* planes, uint8_t* out, unsigned (&lo)[4],
                                           unsigned (&hi)[4])
{
    const PaintArgs& a = g.p;
    const long long plane = (long long)a.nx * a.ny * a.nz;
    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
    struct Rows {
        long long drow, srow;   // the box row and its source row, in a plane
        size_t stage;           // the box row in a slab
    };
    walk_rows(
        a, wave_index(),
        [&](unsigned r, int y, int z) {
            const int sy = clone::source(a.o[1] + y, g.offset[1], g.mirror[1], a.ny);
            const int sz = clone::source(a.o[2] + z, g.offset[2], g.mirror[2], a.nz);
            return Rows{box_row(a, y, z), ((long long)sz * a.ny + sy) * a.nx, (size_t)r * (size_t)a.e[0]};
        },
        [&](const Rows& rw, int x, unsigned long long q) {
            const unsigned w = brush::weight(q, a.s, a.falloff);
            const int sx = clone::source(a.o[0] + x, g.offset[0], g.mirror[0], a.nx);
            int k = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                const uint8_t* pc = planes + c * plane;
                const unsigned old = pc[rw.drow + x];
                const unsigned nw = brush::blend(a.op, old, pc[rw.srow + sx], w * a.strength[c]);
                if constexpr (STAGE) {
                    out[(size_t)k * slab + rw.stage + (size_t)x] = (uint8_t)nw;
                    ++k;
                } else {
                    commit(out + c * plane + rw.drow + x, old, nw, lo[c], hi[c]);
                }
            }
        });
}

__global__ __launch_bounds__(kBlock) void k_clone_direct(CloneArgs g, uint8_t* planes, unsigned* __restrict__ mm)
{
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    clone_rows<false>(g, planes, planes, lo, hi);
    fold_minmax(lo, hi, mm);
}

__global__ __launch_bounds__(kBlock) void k_clone_stage(CloneArgs g, const uint8_t* __restrict__ src,
                                                        uint8_t* __restrict__ stage)
{
    unsigned lo[4], hi[4];   // not used
    clone_rows<true>(g, src, stage, lo, hi);
}

// vr_stamp: k_paint_planar over the EDITED box (the
// clipped box intersected with the placement) with the value of a texel read
// from the stamp texel that lies on it: one 4-byte load per inside lane,
// consecutive lanes on consecutive texels of one stamp row.
__global__ __launch_bounds__(kBlock) void k_paint_stamp(StampArgs g, const uint32_t* __restrict__ stamp,
                                                        uint8_t* __restrict__ dst, unsigned* __restrict__ mm)
{
    const PaintArgs& a = g.p;
    const long long plane = (long long)a.nx * a.ny * a.nz;
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    struct Rows {
        uint8_t* __restrict__ row;
        const uint32_t* __restrict__ srow;
    };
    walk_rows(
        a, wave_index(),
        [&](unsigned, int y, int z) {
            return Rows{dst + box_row(a, y, z),
                        stamp + (((size_t)g.so[2] + (size_t)z) * (size_t)g.sby + (size_t)g.so[1] + (size_t)y) * (size_t)g.sbx +
                            (size_t)g.so[0]};
        },
        [&](const Rows& rw, int x, unsigned long long q) {
            const unsigned w = brush::weight(q, a.s, a.falloff);
            const uint32_t v = rw.srow[x];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                uint8_t* p = rw.row + x + c * plane;
                const unsigned old = *p;
                commit(p, old, brush::blend(a.op, old, (v >> (8 * c)) & 255u, w * a.strength[c]), lo[c], hi[c]);
            }
        });
    fold_minmax(lo, hi, mm);
}

// vr_stamp_affine / vr_clone_affine: k_paint_planar
// with the value of a texel resampled from a source at the 16.16 position P
// that an affine map gives the texel (vr_affine.h).  Rows and lanes are
// k_paint_planar's: a wave takes a box row, consecutive lanes consecutive
// destination x.  The y, z and origin terms of P belong to the row --
// wave-uniform 64-bit values, computed once per row (affine_row); per lane each
// axis adds m[a][0] times the texel's x.  Consecutive lanes therefore read
// along ONE straight line through the source, m[.][0] apart: a row of the
// source for a translation or a scale, a diagonal for a rotation.  A row or a
// texel outside the ellipsoid, and (VR_BORDER_SKIP) a texel whose position is
// outside the source, is left before any load.
struct AffineRow {
    long long base[3];   // P of the row's texel x = 0 of the box
};
__device__ __forceinline__ AffineRow affine_row(const AffineArgs& g, int y, int z)
{
    const PaintArgs& a = g.p;
    AffineRow r;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
        r.base[ax] = affine::position(g.m[ax], g.origin[ax], g.pivot, a.o[0], a.o[1] + y, a.o[2] + z);
    return r;
}
// The clamped position of the row's texel x; false when VR_BORDER_SKIP leaves the texel alone.
__device__ __forceinline__ bool affine_position(const AffineArgs& g, const AffineRow& rw, int x, long long (&p)[3])
{
    bool out = false;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const long long v = rw.base[ax] + (long long)g.m[ax][0] * x;
        out = out || affine::outside(v, g.n[ax]);
        p[ax] = affine::clamp(v, g.n[ax]);
    }
    return !(out && g.border == VR_BORDER_SKIP);
}

// vr_stamp_affine: the source is the caller's box of dwords, one per texel with
// all four channels.  NEAREST: one dword load per inside lane.  LINEAR: eight,
// and the x stage of the trilinear sum runs on two channels at a time in the
// 0x00FF00FF halves of a register (a half holds at most 255 * 256); the y and z
// stages are vr_affine.h's per channel, so the bytes are the statement's.
template <bool LINEAR>
__global__ __launch_bounds__(kBlock) void k_stamp_affine(AffineArgs g, const uint32_t* __restrict__ stamp,
                                                         uint8_t* __restrict__ dst, unsigned* __restrict__ mm)
{
    const PaintArgs& a = g.p;
    const long long plane = (long long)a.nx * a.ny * a.nz;
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    struct Rows {
        uint8_t* __restrict__ row;
        AffineRow p;
    };
    const size_t sbx = (size_t)g.n[0], sby = (size_t)g.n[1];
    walk_rows(
        a, wave_index(), [&](unsigned, int y, int z) { return Rows{dst + box_row(a, y, z), affine_row(g, y, z)}; },
        [&](const Rows& rw, int x, unsigned long long q) {
            long long p[3];
            if (!affine_position(g, rw.p, x, p)) return;
            const unsigned w = brush::weight(q, a.s, a.falloff);
            unsigned v[4];
            if constexpr (LINEAR) {
                const affine::Axis ax = affine::linear_weights(p[0], g.n[0]), ay = affine::linear_weights(p[1], g.n[1]),
                                   az = affine::linear_weights(p[2], g.n[2]);
                const size_t r00 = ((size_t)az.i * sby + (size_t)ay.i) * sbx, r01 = ((size_t)az.i * sby + (size_t)ay.j) * sbx,
                             r10 = ((size_t)az.j * sby + (size_t)ay.i) * sbx, r11 = ((size_t)az.j * sby + (size_t)ay.j) * sbx;
                const uint32_t c[4][2] = {{stamp[r00 + ax.i], stamp[r00 + ax.j]}, {stamp[r01 + ax.i], stamp[r01 + ax.j]},
                                          {stamp[r10 + ax.i], stamp[r10 + ax.j]}, {stamp[r11 + ax.i], stamp[r11 + ax.j]}};
                uint32_t ev[4], od[4];   // the x sums of channels 0, 2 and of 1, 3, per (z, y) pair
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    ev[k] = (c[k][0] & 0x00ff00ffu) * (256u - ax.f) + (c[k][1] & 0x00ff00ffu) * ax.f;
                    od[k] = ((c[k][0] >> 8) & 0x00ff00ffu) * (256u - ax.f) + ((c[k][1] >> 8) & 0x00ff00ffu) * ax.f;
                }
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const int sh = 16 * (ch >> 1);
                    const uint32_t* xs = ch & 1 ? od : ev;
                    v[ch] = affine::linear_yz((xs[0] >> sh) & 0xffffu, (xs[1] >> sh) & 0xffffu, (xs[2] >> sh) & 0xffffu,
                                              (xs[3] >> sh) & 0xffffu, ay.f, az.f);
                }
            } else {
                const uint32_t t = stamp[((size_t)affine::nearest(p[2]) * sby + (size_t)affine::nearest(p[1])) * sbx +
                                         (size_t)affine::nearest(p[0])];
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) v[ch] = (t >> (8 * ch)) & 255u;
            }
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                if (a.strength[ch] == 0u) continue;
                uint8_t* d = rw.row + x + ch * plane;
                const unsigned old = *d;
                commit(d, old, brush::blend(a.op, old, v[ch], w * a.strength[ch]), lo[ch], hi[ch]);
            }
        });
    fold_minmax(lo, hi, mm);
}

// vr_clone_affine: the source is the planes themselves, byte gathers per painted
// channel (one for NEAREST, eight for LINEAR).  STAGE = false
// (k_clone_affine_direct): `out` is the planes; the host has checked
// (vr_affine.h direct) that no texel of the box is read.  STAGE = true
// (k_clone_affine_stage): the planes are read only and the new byte of every
// processed texel and painted channel goes to the staging slabs, as
// k_clone_stage leaves them; k_blur_commit follows.  A texel VR_BORDER_SKIP
// leaves alone stages its old bytes: the commit then stores nothing for it and
// folds a byte that the range holds already.
template <bool STAGE, bool LINEAR>
__device__ __forceinline__ void affine_rows(const AffineArgs& g, const uint8_t* planes, uint8_t* out, unsigned (&lo)[4],
                                            unsigned (&hi)[4])
{
    const PaintArgs& a = g.p;
    const long long plane = (long long)a.nx * a.ny * a.nz;
    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
    struct Rows {
        long long drow;   // the box row in a plane
        size_t stage;     // the box row in a slab
        AffineRow p;
    };
    walk_rows(
        a, wave_index(),
        [&](unsigned r, int y, int z) { return Rows{box_row(a, y, z), (size_t)r * (size_t)a.e[0], affine_row(g, y, z)}; },
        [&](const Rows& rw, int x, unsigned long long q) {
            long long p[3];
            const bool touched = affine_position(g, rw.p, x, p);
            if (!STAGE && !touched) return;
            const unsigned w = brush::weight(q, a.s, a.falloff);
            const affine::Axis ax = affine::linear_weights(p[0], a.nx), ay = affine::linear_weights(p[1], a.ny),
                               az = affine::linear_weights(p[2], a.nz);
            const long long r00 = ((long long)az.i * a.ny + ay.i) * a.nx, r01 = ((long long)az.i * a.ny + ay.j) * a.nx,
                            r10 = ((long long)az.j * a.ny + ay.i) * a.nx, r11 = ((long long)az.j * a.ny + ay.j) * a.nx;
            const long long near = ((long long)affine::nearest(p[2]) * a.ny + affine::nearest(p[1])) * a.nx + affine::nearest(p[0]);
            int k = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                const uint8_t* pc = planes + c * plane;
                const unsigned old = pc[rw.drow + x];
                unsigned nw = old;
                if (touched) {
                    unsigned v;
                    if constexpr (LINEAR) {
                        const unsigned gx = 256u - ax.f;
                        v = affine::linear_yz(pc[r00 + ax.i] * gx + pc[r00 + ax.j] * ax.f, pc[r01 + ax.i] * gx + pc[r01 + ax.j] * ax.f,
                                              pc[r10 + ax.i] * gx + pc[r10 + ax.j] * ax.f, pc[r11 + ax.i] * gx + pc[r11 + ax.j] * ax.f,
                                              ay.f, az.f);
                    } else {
                        v = pc[near];
                    }
                    nw = brush::blend(a.op, old, v, w * a.strength[c]);
                }
                if constexpr (STAGE) {
                    out[(size_t)k * slab + rw.stage + (size_t)x] = (uint8_t)nw;
                    ++k;
                } else {
                    commit(out + c * plane + rw.drow + x, old, nw, lo[c], hi[c]);
                }
            }
        });
}

template <bool LINEAR>
__global__ __launch_bounds__(kBlock) void k_clone_affine_direct(AffineArgs g, uint8_t* planes, unsigned* __restrict__ mm)
{
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    affine_rows<false, LINEAR>(g, planes, planes, lo, hi);
    fold_minmax(lo, hi, mm);
}

template <bool LINEAR>
__global__ __launch_bounds__(kBlock) void k_clone_affine_stage(AffineArgs g, const uint8_t* __restrict__ src,
                                                               uint8_t* __restrict__ stage)
{
    unsigned lo[4], hi[4];   // not used
    affine_rows<true, LINEAR>(g, src, stage, lo, hi);
}

// vr_warp, first launch: k_clone_affine_stage's
// contract -- the planes read only, the new byte of every inside texel and
// painted channel to the staging slabs, a texel VR_BORDER_SKIP leaves alone
// staged with its old byte, so k_blur_commit follows unchanged -- with the
// position of a texel blended with its own by the brush weight (vr_warp.h).
// The read footprint moves with the texel but stays near it, so a workgroup
// takes a kWarpT^3 tile of the clipped box, two texels per thread (z and z +
// kWarpT / 2 of one (x, y)), and
//  1. every thread forms its texels' weights and clamped positions and the
//     texels they read per axis (both of a LINEAR position, the nearest of a
//     NEAREST one); a wave reduce and one LDS atomic per wave and bound leave
//     the tile's footprint box in LDS;
//  2. after the barrier every thread reads the same box back.  At most
//     kWarpBudget texels (and option warp_lds): the box goes to LDS, per
//     painted channel, as aligned dwords of the plane wherever such a dword
//     lies inside the planes' allocation and as bytes elsewhere, rows dense;
//     the corners are then gathered from LDS.  Otherwise (extreme scales, a
//     collapse) they are gathered from the planes as affine_rows does;
//  3. either way the filter is vr_affine.h's and the blend the SET blend with
//     a = 256 * strength.
// Every thread reaches all three barriers: nothing returns, a tile without a
// touched texel has an empty footprint (lo > hi) and loads nothing, and every
// loop is bounded by the tile or by kWarpBudget.
constexpr int kWarpT = 8, kWarpBudget = 4096;
static_assert(kWarpT * kWarpT * (kWarpT / 2) == kBlock && kWarpT * kWarpT == 64, "two texels per thread, a wave per z pair");

template <bool LINEAR>
__global__ __launch_bounds__(kBlock) void k_warp_stage(AffineArgs g, int use_lds, const uint8_t* __restrict__ src,
                                                       uint8_t* __restrict__ stage)
{
    const PaintArgs& a = g.p;
    __shared__ int fp[6];                                  // the footprint box: first texel per axis, then last
    __shared__ uint32_t foot32[4 * kWarpBudget / 4];       // a painted channel's footprint, rows dense, per kWarpBudget bytes
    uint8_t* foot = reinterpret_cast<uint8_t*>(foot32);

    const int tid = threadIdx.x, lx = tid % kWarpT, ly = tid / kWarpT % kWarpT, lz = tid / (kWarpT * kWarpT);
    const Tile t0 = tile_origin(a, kWarpT, kWarpT, kWarpT);
    const int x = t0.x + lx, y = t0.y + ly;   // in the box
    if (tid < 6) fp[tid] = tid < 3 ? 0x7fffffff : -1;

    unsigned wgt[2] = {0u, 0u};     // 0 outside the ellipsoid or the box
    bool touched[2] = {false, false};
    long long p[2][3];
    int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {-1, -1, -1};
    const bool column = x < a.e[0] && y < a.e[1];
    const unsigned long long qxy =
        column ? brush::axis_term(a.d0[0] + x, a.k[0]) + brush::axis_term(a.d0[1] + y, a.k[1]) : 0ull;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int z = t0.z + lz + j * (kWarpT / 2);
        p[j][0] = p[j][1] = p[j][2] = 0;
        if (column && z < a.e[2]) {
            const unsigned long long q = qxy + brush::axis_term(a.d0[2] + z, a.k[2]);
            if (q <= a.s) wgt[j] = brush::weight(q, a.s, a.falloff);
        }
        if (wgt[j] == 0u) continue;
        const int t[3] = {a.o[0] + x, a.o[1] + y, a.o[2] + z};
        bool out = false;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const long long v =
                warp::position(t[ax], warp::displacement(g.m[ax], g.origin[ax], g.pivot, t[0], t[1], t[2], t[ax]), wgt[j]);
            out = out || affine::outside(v, g.n[ax]);
            p[j][ax] = affine::clamp(v, g.n[ax]);
        }
        touched[j] = !(out && g.border == VR_BORDER_SKIP);
        if (!touched[j]) continue;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            int first, last;
            if constexpr (LINEAR) {
                const affine::Axis w = affine::linear_weights(p[j][ax], g.n[ax]);
                first = w.i; last = w.j;
            } else {
                first = last = affine::nearest(p[j][ax]);
            }
            mn[ax] = min(mn[ax], first);
            mx[ax] = max(mx[ax], last);
        }
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            mn[ax] = min(mn[ax], __shfl_xor(mn[ax], d));
            mx[ax] = max(mx[ax], __shfl_xor(mx[ax], d));
        }
    __syncthreads();   // fp holds the empty box
    if ((tid & 63) == 0) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            atomicMin(&fp[ax], mn[ax]);
            atomicMax(&fp[3 + ax], mx[ax]);
        }
    }
    __syncthreads();
    const int f0[3] = {fp[0], fp[1], fp[2]};
    const int ex = fp[3] - f0[0] + 1, ey = fp[4] - f0[1] + 1, ez = fp[5] - f0[2] + 1;   // <= 0 on every axis: no touched texel
    const bool lds = use_lds != 0 && ex > 0 && (long long)ex * ey * ez <= kWarpBudget;   // workgroup-uniform

    const long long plane = (long long)a.nx * a.ny * a.nz;
    if (lds) {
        const int rows = ey * ez, nd = (ex + 6) / 4;   // the dwords a row of ex bytes can meet at any alignment
        const uint8_t* const end = src + 4 * plane;
        int k = 0;
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {
            if (a.strength[c] == 0u) continue;
            const uint8_t* __restrict__ pc = src + c * plane;
            uint8_t* __restrict__ fl = foot + k * kWarpBudget;
            for (int i = tid; i < rows * nd; i += kBlock) {   // rows * nd <= 7 * kWarpBudget / 4
                const int r = i / nd, d = i - r * nd, zi = r / ey, yi = r - zi * ey;
                const uint8_t* row = pc + ((long long)(f0[2] + zi) * a.ny + (f0[1] + yi)) * a.nx + f0[0];
                const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 3u), x0 = 4 * d - mis;   // the dword's first byte, in the row
                if (x0 >= ex) continue;
                const uint8_t* q = row + x0;   // 4-byte aligned
                uint8_t* o = fl + r * ex;
                if (q >= src && q + 4 <= end) {
                    const uint32_t v = *reinterpret_cast<const uint32_t*>(q);
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (x0 + b >= 0 && x0 + b < ex) o[x0 + b] = (uint8_t)(v >> (8 * b));
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (x0 + b >= 0 && x0 + b < ex) o[x0 + b] = row[x0 + b];
                }
            }
            ++k;
        }
    }
    __syncthreads();   // the footprint is staged

    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (wgt[j] == 0u) continue;
        const int z = t0.z + lz + j * (kWarpT / 2);
        const long long drow = box_row(a, y, z) + x;
        const size_t srow = ((size_t)z * (size_t)a.e[1] + (size_t)y) * (size_t)a.e[0] + (size_t)x;
        const affine::Axis wx = affine::linear_weights(p[j][0], a.nx), wy = affine::linear_weights(p[j][1], a.ny),
                           wz = affine::linear_weights(p[j][2], a.nz);
        const int sx = affine::nearest(p[j][0]), sy = affine::nearest(p[j][1]), sz = affine::nearest(p[j][2]);
        int k = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (a.strength[c] == 0u) continue;
            const uint8_t* __restrict__ pc = src + c * plane;
            const unsigned old = pc[drow];
            unsigned nw = old;
            if (touched[j]) {
                const uint8_t* fl = foot + k * kWarpBudget;
                const auto texel = [&](int tx, int ty, int tz) -> unsigned {
                    return lds ? fl[((tz - f0[2]) * ey + (ty - f0[1])) * ex + (tx - f0[0])]
                               : pc[((long long)tz * a.ny + ty) * a.nx + tx];
                };
                unsigned v;
                if constexpr (LINEAR) {
                    const unsigned gx = 256u - wx.f;
                    v = affine::linear_yz(texel(wx.i, wy.i, wz.i) * gx + texel(wx.j, wy.i, wz.i) * wx.f,
                                          texel(wx.i, wy.j, wz.i) * gx + texel(wx.j, wy.j, wz.i) * wx.f,
                                          texel(wx.i, wy.i, wz.j) * gx + texel(wx.j, wy.i, wz.j) * wx.f,
                                          texel(wx.i, wy.j, wz.j) * gx + texel(wx.j, wy.j, wz.j) * wx.f, wy.f, wz.f);
                } else {
                    v = texel(sx, sy, sz);
                }
                nw = brush::blend(VR_BRUSH_SET, old, v, 256u * a.strength[c]);
            }
            stage[(size_t)k * slab + srow] = (uint8_t)nw;
            ++k;
        }
    }
}

// vr_remap / vr_remap_device: k_paint_planar with the
// value of a texel read from a table at the texel's own old byte
// (vr_remap.h).  Rows and lanes are k_paint_planar's.  At workgroup start the
// tables of the painted channels go into 1 KiB of LDS as dwords: wave c stages
// channel c (64 lanes x one dword = its 256 bytes) when strength[c] != 0 -- a
// wave-uniform test, and a table that is not needed is never read.  The source
// is the kernel's own arguments (DEVICE_LUT = false: the 1024 bytes travel by
// value, so the host table is free again when the launch call returns) or the
// caller's device table read when the kernel runs (DEVICE_LUT = true; 4-byte
// aligned).  Every thread reaches the barrier after the stage and
// fold_minmax's: a wave without a row falls through its loop, nothing returns
// early.  The lookup is one LDS byte read per texel and channel; a store goes
// only where the byte changed and the new bytes are folded into mm.
template <bool DEVICE_LUT>
struct RemapLut {
    vr_lut t;
};
template <>
struct RemapLut<true> {
    const uint32_t* t;
};

template <bool DEVICE_LUT>
__global__ __launch_bounds__(kBlock) void k_remap(PaintArgs a, RemapLut<DEVICE_LUT> lut, uint8_t* __restrict__ dst,
                                                  unsigned* __restrict__ mm)
{
    constexpr unsigned kWaves = kBlock / 64;
    static_assert(kWaves == 4 && sizeof(vr_lut) == 4 * 64 * sizeof(uint32_t), "a wave stages one channel's table");
    __shared__ uint32_t table[4 * 64];
    const long long plane = (long long)a.nx * a.ny * a.nz;
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    const int lane = threadIdx.x & 63;
    const unsigned wave = wave_index();
    if (a.strength[wave] != 0u) {
        const uint32_t* src;
        if constexpr (DEVICE_LUT) src = lut.t;
        else src = reinterpret_cast<const uint32_t*>(&lut.t);
        table[wave * 64 + lane] = src[wave * 64 + lane];
    }
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(table);
    walk_rows(
        a, wave, [&](unsigned, int y, int z) -> uint8_t* { return dst + box_row(a, y, z); },
        [&](uint8_t* __restrict__ row, int x, unsigned long long q) {
            const unsigned w = brush::weight(q, a.s, a.falloff);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                uint8_t* p = row + x + c * plane;
                const unsigned old = *p;
                commit(p, old, brush::blend(a.op, old, bytes[c * 256 + (int)old], w * a.strength[c]), lo[c], hi[c]);
            }
        });
    fold_minmax(lo, hi, mm);
}

// vr_stats_lut_device: vr_stats_lut (vr_remap.h) in ONE
// workgroup of 256 threads; thread v owns bin v.  Per channel: the bin goes to
// LDS, an inclusive block scan (Hillis-Steele, 8 steps, 64-bit) leaves cum(v)
// there, and lo / hi -- the lowest and highest non-empty bin -- come from LDS
// min / max over the threads whose bin is not 0; n = cum(255), cmin = cum(lo).
// Every thread then stores its byte of the channel's table: 1024 byte stores
// in all, nothing else is written.  An unselected channel reads no bin.
__global__ __launch_bounds__(256) void k_stats_lut(const vr_volume_stats* __restrict__ stats, int kind, unsigned mask,
                                                   vr_lut* __restrict__ out)
{
    __shared__ unsigned long long cum[256];
    __shared__ int ends[2];
    const int v = threadIdx.x;
    for (int c = 0; c < 4; ++c) {
        const bool selected = (mask >> c & 1u) != 0u;   // workgroup-uniform
        if (!selected) {
            out->lut[c][v] = (uint8_t)v;
            continue;
        }
        const unsigned long long h = stats->hist[c][v];
        cum[v] = h;
        if (v == 0) { ends[0] = 256; ends[1] = -1; }
        __syncthreads();
        if (h != 0ull) { atomicMin(&ends[0], v); atomicMax(&ends[1], v); }
        for (int off = 1; off < 256; off <<= 1) {
            const unsigned long long below = v >= off ? cum[v - off] : 0ull;
            __syncthreads();
            cum[v] += below;
            __syncthreads();
        }
        remap::Range r{ends[0], ends[1], cum[255], 0ull};
        if (r.lo <= 255) r.cmin = cum[r.lo];
        const unsigned long long mine = cum[v];
        __syncthreads();   // the next channel overwrites cum and ends
        out->lut[c][v] = (uint8_t)(remap::mapped(kind, true, r) ? remap::stats_value(kind, v, mine, r) : (unsigned)v);
    }
}

// vr_brush_stats / vr_box_stats: the statistics of the
// texels of a box that lie inside the brush (or, ellipsoid == 0, of all of
// them) added to *out, which the caller has zeroed.  It reads the planes and
// writes *out, nothing else.  The arithmetic is vr_stats.h's, in integers:
// adds commute, so neither the order of the workgroups nor the grid matters.
//
// Rows and lanes are k_paint_planar's: a wave takes a box row (y, z) at a
// time, consecutive lanes on consecutive x; a row outside the ellipsoid is
// left before any load; byte loads, the plane rows start at any byte.  The x
// loop's trip count is the wave's, not the lane's, so the ballots below see
// every lane.
//  * histogram: 4 x 256 32-bit bins per workgroup in LDS, added to with LDS
//    atomics.  A workgroup sees fewer texels than a plane holds (< 2^31,
//    dims_ok), so a bin cannot overflow.  64 lanes on one bin serialise, and
//    that is the common case (a uniform channel, any smooth region): per
//    channel the wave takes its first inside lane's byte, ballots the inside
//    lanes that hold the same byte, and that first lane adds their number in
//    ONE atomic while only the lanes holding another byte add 1 each -- one
//    ds_add instruction either way, with a single active lane when the row
//    segment is constant.
//  * count, weight, wsum[c]: 64-bit per lane, reduced over the wave with
//    shuffles and over the workgroup through LDS.
// After one barrier the workgroup adds its non-zero bins and sums to *out
// with 64-bit global atomics: at most 1030 per workgroup.
constexpr int kStatsMaxGrid = 1024;   // workgroups: bounds the flush at 1024 x 1030 atomics (launch_stats)

__global__ __launch_bounds__(kBlock) void k_stats(StatsArgs a, const uint8_t* __restrict__ src,
                                                  vr_volume_stats* __restrict__ out)
{
    constexpr unsigned kWaves = kBlock / 64;
    __shared__ unsigned bins[4 * 256];
    __shared__ unsigned long long red[kWaves][6];
    for (int i = threadIdx.x; i < 4 * 256; i += kBlock) bins[i] = 0u;
    __syncthreads();

    const long long plane = (long long)a.nx * a.ny * a.nz;
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned rows = (unsigned)a.e[1] * (unsigned)a.e[2];   // < 2^31 (inside the volume)
    unsigned long long sum[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};   // count, weight, wsum[4]
    for (unsigned r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
        const int z = (int)(r / (unsigned)a.e[1]), y = (int)(r - (unsigned)z * (unsigned)a.e[1]);
        unsigned long long qyz = 0ull;
        if (a.ellipsoid) {
            qyz = brush::axis_term(a.d0[1] + y, a.k[1]) + brush::axis_term(a.d0[2] + z, a.k[2]);
            if (qyz > a.s) continue;
        }
        const uint8_t* __restrict__ row = src + ((long long)(a.o[2] + z) * a.ny + (a.o[1] + y)) * a.nx + a.o[0];
        for (int x0 = 0; x0 < a.e[0]; x0 += 64) {
            const int x = x0 + lane;
            unsigned w = 0u;   // 0 = this lane's texel does not count
            if (x < a.e[0])
                w = stats::texel_weight(a.ellipsoid, a.ellipsoid ? qyz + brush::axis_term(a.d0[0] + x, a.k[0]) : 0ull,
                                        a.s, a.falloff);
            const bool in = w != 0u;
            const unsigned long long act = __ballot(in);
            if (act == 0ull) continue;
            const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
            sum[0] += in ? 1ull : 0ull;
            sum[1] += w;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (!stats::selected(a.mask, c)) continue;
                unsigned v = 0u;
                if (in) v = row[x + c * plane];
                sum[2 + c] += stats::wsum_term(w, v);
                const unsigned head = (unsigned)__builtin_amdgcn_readlane((int)v, first);
                const unsigned long long same = __ballot(in && v == head);
                if (in && (lane == first || v != head))
                    atomicAdd(&bins[c * 256 + (int)v], lane == first ? (unsigned)__popcll(same) : 1u);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        for (int off = 32; off > 0; off >>= 1) sum[k] += __shfl_xor(sum[k], off);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) red[wave][k] = sum[k];
    }
    __syncthreads();
    // *out as its 1030 64-bit words: count, weight, wsum[4], hist[4][256]
    static_assert(sizeof(vr_volume_stats) == 8 * (6 + 4 * 256) && offsetof(vr_volume_stats, hist) == 48 &&
                      offsetof(vr_volume_stats, wsum) == 16 && sizeof(unsigned long long) == 8,
                  "vr_volume_stats is 1030 packed 64-bit words");
    unsigned long long* __restrict__ words = reinterpret_cast<unsigned long long*>(out);
    for (int i = threadIdx.x; i < 4 * 256; i += kBlock) {
        const unsigned n = bins[i];
        if (n != 0u) atomicAdd(&words[6 + i], (unsigned long long)n);
    }
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        unsigned long long v = red[0][k];
        for (unsigned wv = 1; wv < kWaves; ++wv) v += red[wv][k];
        if (v != 0ull) atomicAdd(&words[k], v);
    }
}

}  // namespace

// a wave per box row, a workgroup per kBlock / 64 rows, grid-stride past 4096 workgroups
hipError_t launch_paint_planar(const PaintArgs& a, uint8_t* d_planar, unsigned* mm, hipStream_t s)
{
    const long long rows = (long long)a.e[1] * a.e[2];
    hipLaunchKernelGGL(k_paint_planar, dim3(grid_for(rows * 64)), dim3(kBlock), 0, s, a, d_planar, mm);
    return hipGetLastError();
}

// a wave per row of a dab's box, as launch_paint_planar; the list must hold a dab, and every dab a row
hipError_t launch_paint_stroke(const StrokeArgs& a, uint8_t* d_planar, unsigned* mm, hipStream_t s)
{
    if (a.count < 1 || a.count > VR_MAX_DABS) return hipErrorInvalidValue;
    for (int i = 0; i < a.count; ++i)
        if (a.row_begin[i + 1] <= a.row_begin[i]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_paint_stroke, dim3(grid_for((long long)a.row_begin[a.count] * 64)), dim3(kBlock), 0, s, a,
                       d_planar, mm);
    return hipGetLastError();
}

size_t blur_stage_bytes(const PaintArgs& a)
{
    size_t channels = 0;
    for (int c = 0; c < 4; ++c) channels += a.strength[c] != 0u;
    return channels * (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
}

// a workgroup per tile of the clipped box: at most 16 x 64 x 64 of them (a box edge is at most 511 texels)
hipError_t launch_blur_stage(const PaintArgs& a, int half_width, const uint8_t* d_planar, uint8_t* d_stage, hipStream_t s)
{
    if (a.e[0] < 1 || a.e[1] < 1 || a.e[2] < 1 || !d_stage) return hipErrorInvalidValue;
    const long long tiles = stage_tiles(a, kBlurTX, kBlurTY, kBlurTZ);
    if (tiles > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 g((unsigned)tiles), b(kBlock);
    switch (half_width) {
    case 1: hipLaunchKernelGGL(k_blur_stage<1>, g, b, 0, s, a, d_planar, d_stage); break;
    case 2: hipLaunchKernelGGL(k_blur_stage<2>, g, b, 0, s, a, d_planar, d_stage); break;
    case 3: hipLaunchKernelGGL(k_blur_stage<3>, g, b, 0, s, a, d_planar, d_stage); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the blur's grid over the morph's tile, one instantiation per half width and extremum
hipError_t launch_morph_stage(const PaintArgs& a, int op, int half_width, const uint8_t* d_planar, uint8_t* d_stage, hipStream_t s)
{
    if (a.e[0] < 1 || a.e[1] < 1 || a.e[2] < 1 || !d_stage) return hipErrorInvalidValue;
    if (op != VR_MORPH_ERODE && op != VR_MORPH_DILATE) return hipErrorInvalidValue;
    const long long tiles = stage_tiles(a, kMorphTX, kMorphTY, kMorphTZ);
    if (tiles > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 g((unsigned)tiles), b(kBlock);
    switch (2 * half_width + (op == VR_MORPH_DILATE)) {
    case 2: hipLaunchKernelGGL((k_morph_stage<1, false>), g, b, 0, s, a, d_planar, d_stage); break;
    case 3: hipLaunchKernelGGL((k_morph_stage<1, true>), g, b, 0, s, a, d_planar, d_stage); break;
    case 4: hipLaunchKernelGGL((k_morph_stage<2, false>), g, b, 0, s, a, d_planar, d_stage); break;
    case 5: hipLaunchKernelGGL((k_morph_stage<2, true>), g, b, 0, s, a, d_planar, d_stage); break;
    case 6: hipLaunchKernelGGL((k_morph_stage<3, false>), g, b, 0, s, a, d_planar, d_stage); break;
    case 7: hipLaunchKernelGGL((k_morph_stage<3, true>), g, b, 0, s, a, d_planar, d_stage); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the morph's grid and tile, one instantiation per half width; rank is 0..(2 half_width + 1)^3 - 1 (vr_rank.h resolve)
hipError_t launch_rank_stage(const PaintArgs& a, int rank, int half_width, const uint8_t* d_planar, uint8_t* d_stage, hipStream_t s)
{
    if (a.e[0] < 1 || a.e[1] < 1 || a.e[2] < 1 || !d_stage) return hipErrorInvalidValue;
    if (half_width < 1 || half_width > VR_RANK_MAX_HALF || rank < 0 || rank > rank::window(half_width) - 1)
        return hipErrorInvalidValue;
    const long long tiles = stage_tiles(a, kMorphTX, kMorphTY, kMorphTZ);
    if (tiles > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 g((unsigned)tiles), b(kBlock);
    switch (half_width) {
    case 1: hipLaunchKernelGGL(k_rank_stage<1>, g, b, 0, s, a, (unsigned)rank, d_planar, d_stage); break;
    case 2: hipLaunchKernelGGL(k_rank_stage<2>, g, b, 0, s, a, (unsigned)rank, d_planar, d_stage); break;
    case 3: hipLaunchKernelGGL(k_rank_stage<3>, g, b, 0, s, a, (unsigned)rank, d_planar, d_stage); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// a wave per box row, as launch_paint_planar
hipError_t launch_blur_commit(const PaintArgs& a, const uint8_t* d_stage, uint8_t* d_planar, unsigned* mm, hipStream_t s)
{
    const long long rows = (long long)a.e[1] * a.e[2];
    hipLaunchKernelGGL(k_blur_commit, dim3(grid_for(rows * 64)), dim3(kBlock), 0, s, a, d_stage, d_planar, mm);
    return hipGetLastError();
}

// vr_clone and vr_stamp: a wave per box row, as launch_paint_planar
hipError_t launch_clone_direct(const CloneArgs& a, uint8_t* d_planar, unsigned* mm, hipStream_t s)
{
    if (a.p.e[0] < 1 || a.p.e[1] < 1 || a.p.e[2] < 1 || !d_planar) return hipErrorInvalidValue;
    const long long rows = (long long)a.p.e[1] * a.p.e[2];
    hipLaunchKernelGGL(k_clone_direct, dim3(grid_for(rows * 64)), dim3(kBlock), 0, s, a, d_planar, mm);
    return hipGetLastError();
}

hipError_t launch_clone_stage(const CloneArgs& a, const uint8_t* d_planar, uint8_t* d_stage, hipStream_t s)
{
    if (a.p.e[0] < 1 || a.p.e[1] < 1 || a.p.e[2] < 1 || !d_planar || !d_stage) return hipErrorInvalidValue;
    const long long rows = (long long)a.p.e[1] * a.p.e[2];
    hipLaunchKernelGGL(k_clone_stage, dim3(grid_for(rows * 64)), dim3(kBlock), 0, s, a, d_planar, d_stage);
    return hipGetLastError();
}

hipError_t launch_paint_stamp(const StampArgs& a, const uint8_t* d_stamp, uint8_t* d_planar, unsigned* mm, hipStream_t s)
{
    if (a.p.e[0] < 1 || a.p.e[1] < 1 || a.p.e[2] < 1 || !d_planar || !d_stamp) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(d_stamp) & 3u) != 0u || a.so[0] < 0 || a.so[1] < 0 || a.so[2] < 0) return hipErrorInvalidValue;
    if ((long long)a.so[0] + a.p.e[0] > a.sbx || (long long)a.so[1] + a.p.e[1] > a.sby) return hipErrorInvalidValue;
    const long long rows = (long long)a.p.e[1] * a.p.e[2];
    hipLaunchKernelGGL(k_paint_stamp, dim3(grid_for(rows * 64)), dim3(kBlock), 0, s, a,
                       reinterpret_cast<const uint32_t*>(d_stamp), d_planar, mm);
    return hipGetLastError();
}

// vr_stamp_affine and vr_clone_affine: a wave per box row, as launch_paint_planar; one instantiation per filter
static bool affine_args_ok(const AffineArgs& a)
{
    if (a.p.e[0] < 1 || a.p.e[1] < 1 || a.p.e[2] < 1 || a.n[0] < 1 || a.n[1] < 1 || a.n[2] < 1) return false;
    if (a.filter != VR_FILTER_NEAREST && a.filter != VR_FILTER_LINEAR) return false;
    return a.border == VR_BORDER_CLAMP || a.border == VR_BORDER_SKIP;
}

hipError_t launch_stamp_affine(const AffineArgs& a, const uint8_t* d_stamp, uint8_t* d_planar, unsigned* mm, hipStream_t s)
{
    if (!affine_args_ok(a) || !d_planar || !d_stamp || (reinterpret_cast<uintptr_t>(d_stamp) & 3u) != 0u) return hipErrorInvalidValue;
    if (a.n[0] > VR_AFFINE_MAX_EXTENT || a.n[1] > VR_AFFINE_MAX_EXTENT || a.n[2] > VR_AFFINE_MAX_EXTENT) return hipErrorInvalidValue;
    const dim3 g(grid_for((long long)a.p.e[1] * a.p.e[2] * 64)), b(kBlock);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(d_stamp);
    if (a.filter == VR_FILTER_LINEAR) hipLaunchKernelGGL(k_stamp_affine<true>, g, b, 0, s, a, src, d_planar, mm);
    else hipLaunchKernelGGL(k_stamp_affine<false>, g, b, 0, s, a, src, d_planar, mm);
    return hipGetLastError();
}

hipError_t launch_clone_affine_direct(const AffineArgs& a, uint8_t* d_planar, unsigned* mm, hipStream_t s)
{
    if (!affine_args_ok(a) || !d_planar || a.n[0] != a.p.nx || a.n[1] != a.p.ny || a.n[2] != a.p.nz) return hipErrorInvalidValue;
    const dim3 g(grid_for((long long)a.p.e[1] * a.p.e[2] * 64)), b(kBlock);
    if (a.filter == VR_FILTER_LINEAR) hipLaunchKernelGGL(k_clone_affine_direct<true>, g, b, 0, s, a, d_planar, mm);
    else hipLaunchKernelGGL(k_clone_affine_direct<false>, g, b, 0, s, a, d_planar, mm);
    return hipGetLastError();
}

hipError_t launch_clone_affine_stage(const AffineArgs& a, const uint8_t* d_planar, uint8_t* d_stage, hipStream_t s)
{
    if (!affine_args_ok(a) || !d_planar || !d_stage || a.n[0] != a.p.nx || a.n[1] != a.p.ny || a.n[2] != a.p.nz)
        return hipErrorInvalidValue;
    const dim3 g(grid_for((long long)a.p.e[1] * a.p.e[2] * 64)), b(kBlock);
    if (a.filter == VR_FILTER_LINEAR) hipLaunchKernelGGL(k_clone_affine_stage<true>, g, b, 0, s, a, d_planar, d_stage);
    else hipLaunchKernelGGL(k_clone_affine_stage<false>, g, b, 0, s, a, d_planar, d_stage);
    return hipGetLastError();
}

// vr_warp: a workgroup per kWarpT^3 tile of the clipped box (at most 64^3 of them), one instantiation per filter
hipError_t launch_warp_stage(const AffineArgs& a, bool use_lds, const uint8_t* d_planar, uint8_t* d_stage, hipStream_t s)
{
    if (!affine_args_ok(a) || !d_planar || !d_stage || a.n[0] != a.p.nx || a.n[1] != a.p.ny || a.n[2] != a.p.nz)
        return hipErrorInvalidValue;
    if (a.p.op != VR_BRUSH_SET || (reinterpret_cast<uintptr_t>(d_planar) & 3u) != 0u) return hipErrorInvalidValue;
    const long long tiles = stage_tiles(a.p, kWarpT, kWarpT, kWarpT);
    if (tiles > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 g((unsigned)tiles), b(kBlock);
    if (a.filter == VR_FILTER_LINEAR) hipLaunchKernelGGL(k_warp_stage<true>, g, b, 0, s, a, use_lds ? 1 : 0, d_planar, d_stage);
    else hipLaunchKernelGGL(k_warp_stage<false>, g, b, 0, s, a, use_lds ? 1 : 0, d_planar, d_stage);
    return hipGetLastError();
}

// vr_remap (host_lut: its 1024 bytes go into the kernel's arguments here, during the call) and vr_remap_device
// (host_lut null: d_lut is read when the kernel runs): a wave per box row, as launch_paint_planar
hipError_t launch_remap(const PaintArgs& a, const vr_lut* host_lut, const void* d_lut, uint8_t* d_planar, unsigned* mm,
                        hipStream_t s)
{
    if (a.e[0] < 1 || a.e[1] < 1 || a.e[2] < 1 || !d_planar) return hipErrorInvalidValue;
    const long long rows = (long long)a.e[1] * a.e[2];
    if (host_lut) {
        RemapLut<false> l;
        l.t = *host_lut;
        hipLaunchKernelGGL(k_remap<false>, dim3(grid_for(rows * 64)), dim3(kBlock), 0, s, a, l, d_planar, mm);
    } else {
        if (!d_lut || (reinterpret_cast<uintptr_t>(d_lut) & 3u) != 0u) return hipErrorInvalidValue;
        RemapLut<true> l;
        l.t = static_cast<const uint32_t*>(d_lut);
        hipLaunchKernelGGL(k_remap<true>, dim3(grid_for(rows * 64)), dim3(kBlock), 0, s, a, l, d_planar, mm);
    }
    return hipGetLastError();
}

hipError_t launch_stats_lut(const vr_volume_stats* d_stats, int kind, unsigned mask, vr_lut* d_lut, hipStream_t s)
{
    if (!d_stats || !d_lut || mask > 15u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stats_lut, dim3(1), dim3(256), 0, s, d_stats, kind, mask, d_lut);
    return hipGetLastError();
}

// a wave per box row, a workgroup per kBlock / 64 rows, grid-stride past kStatsMaxGrid workgroups: every workgroup
// ends in up to 1030 global atomics, which the cap bounds whatever the box
hipError_t launch_stats(const StatsArgs& a, const uint8_t* d_planar, vr_volume_stats* d_stats, hipStream_t s)
{
    if (a.e[0] < 1 || a.e[1] < 1 || a.e[2] < 1 || !d_planar || !d_stats) return hipErrorInvalidValue;
    const long long rows = (long long)a.e[1] * a.e[2];
    const long long g = std::min<long long>((rows + kBlock / 64 - 1) / (kBlock / 64), kStatsMaxGrid);
    hipLaunchKernelGGL(k_stats, dim3((unsigned)g), dim3(kBlock), 0, s, a, d_planar, d_stats);
    return hipGetLastError();
}

}  // namespace vr
