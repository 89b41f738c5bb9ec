// vr_volume.hip -- volume producer and layout kernels, plus band assembly.
//
//  * repack: RGBA8 interleaved (the Texture3D input, TestMain.cpp:69-87)
//    -> per-channel planes (planar and padded), the layouts vr_march reads.
//  * noise + min/max + pack: TestMain.cpp:43-92 on the GPU.
//  * assemble: gathered band sets of N ranks -> one frame (SURVEY.md e).
// All are HBM-bound streaming kernels: wide coalesced accesses, grid-stride.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>

#include "vr_blur.h"
#include "vr_brush.h"
#include "vr_clone.h"
#include "vr_internal.h"
#include "vr_morph.h"
#include "vr_noise.h"
#include "vr_rank.h"
#include "vr_remap.h"
#include "vr_stats.h"

namespace vr {
namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// One thread per texel: read 4 B, write 1 B to each of 4 planes.  The padded
// planes get their own pass over (nx+2)(ny+2)(nz+2) positions.
__global__ __launch_bounds__(kBlock) void k_repack_planar(const uchar4* __restrict__ src, long long total,
                                                          uint8_t* __restrict__ dst)
{
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < total;
         i += (long long)gridDim.x * kBlock) {
        const uchar4 v = src[i];
        dst[i] = v.x;
        dst[i + total] = v.y;
        dst[i + 2 * total] = v.z;
        dst[i + 3 * total] = v.w;
    }
}

// The fold of a workgroup's per-channel byte min / max (lo, hi: each thread's
// own, 255 / 0 where it saw nothing) into mm (k_plane_minmax's [min x 4,
// max x 4]) -- the tail of the kernels that write texels into the planes
// (k_update_planar, k_paint_planar).  Every thread of the workgroup calls it.
__device__ __forceinline__ void fold_minmax(unsigned (&lo)[4], unsigned (&hi)[4], unsigned* __restrict__ mm)
{
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) {
            lo[k] = min(lo[k], (unsigned)__shfl_xor((int)lo[k], off));
            hi[k] = max(hi[k], (unsigned)__shfl_xor((int)hi[k], off));
        }
    // waves -> workgroup through LDS, then at most one atomic per channel and
    // bound: only where the box widens the range.  (mm only moves outwards, so a
    // stale read of it can ask for a redundant atomic, never miss a needed one;
    // a time-varying volume whose channels span 0..255 issues none.)
    __shared__ unsigned red[kBlock / 64][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { red[wave][k] = lo[k]; red[wave][4 + k] = hi[k]; }
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int k = threadIdx.x;
        unsigned v = red[0][k];
        for (int w = 1; w < kBlock / 64; ++w) v = k < 4 ? min(v, red[w][k]) : max(v, red[w][k]);
        if (k < 4) {
            if (v < mm[k]) atomicMin(&mm[k], v);
        } else {
            if (v > mm[k]) atomicMax(&mm[k], v);
        }
    }
}

// vr_update_volume: scatter a tightly packed RGBA8 box (bx x by x bz texels at
// texel (x0, y0, z0), x fastest) into the four planes.  One thread per texel,
// consecutive lanes on consecutive x of a box row: a 4-B load, then one byte
// store per plane -- the plane rows start at any byte (x0 and nx are
// arbitrary), so nothing wider is assumed.  Each workgroup folds its texels'
// per-channel byte min / max into mm (fold_minmax):
// both only move outwards, so a channel can lose min == max but never gain it.
__global__ __launch_bounds__(kBlock) void k_update_planar(const uchar4* __restrict__ src, int nx, int ny, int nz,
                                                          int x0, int y0, int z0, int bx, int by, int bz,
                                                          uint8_t* __restrict__ dst, unsigned* __restrict__ mm)
{
    const unsigned total = (unsigned)bx * (unsigned)by * (unsigned)bz;   // < 2^31 (inside the volume)
    const long long plane = (long long)nx * ny * nz;
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
        const unsigned t = i / (unsigned)bx;
        const int x = (int)(i - t * (unsigned)bx), y = (int)(t % (unsigned)by), z = (int)(t / (unsigned)by);
        const uchar4 v = src[i];
        const long long d = ((long long)(z0 + z) * ny + (y0 + y)) * nx + (x0 + x);
        dst[d] = v.x;
        dst[d + plane] = v.y;
        dst[d + 2 * plane] = v.z;
        dst[d + 3 * plane] = v.w;
        const unsigned c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) { lo[k] = min(lo[k], c[k]); hi[k] = max(hi[k], c[k]); }
    }
    fold_minmax(lo, hi, mm);
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
    constexpr unsigned kWaves = kBlock / 64;
    const long long plane = (long long)a.nx * a.ny * a.nz;
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned rows = (unsigned)a.e[1] * (unsigned)a.e[2];   // <= 511^2
    for (unsigned r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
        const int z = (int)(r / (unsigned)a.e[1]), y = (int)(r - (unsigned)z * (unsigned)a.e[1]);
        const unsigned long long qyz = brush::axis_term(a.d0[1] + y, a.k[1]) + brush::axis_term(a.d0[2] + z, a.k[2]);
        if (qyz > a.s) continue;
        uint8_t* __restrict__ row = dst + ((long long)(a.o[2] + z) * a.ny + (a.o[1] + y)) * a.nx + a.o[0];
        for (int x = lane; x < a.e[0]; x += 64) {
            const unsigned long long q = qyz + brush::axis_term(a.d0[0] + x, a.k[0]);
            if (q > a.s) continue;
            const unsigned w = brush::weight(q, a.s, a.falloff);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                uint8_t* p = row + x + c * plane;
                const unsigned old = *p;
                const unsigned nw = brush::blend(a.op, old, a.value[c], w * a.strength[c]);
                if (nw != old) *p = (uint8_t)nw;
                lo[c] = min(lo[c], nw);
                hi[c] = max(hi[c], nw);
            }
        }
    }
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
    const int ntx = (a.e[0] + kBlurTX - 1) / kBlurTX, nty = (a.e[1] + kBlurTY - 1) / kBlurTY;
    const int bt = blockIdx.x;
    const int tx0 = (bt % ntx) * kBlurTX, ty0 = (bt / ntx % nty) * kBlurTY, tz0 = (bt / (ntx * nty)) * kBlurTZ;
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
    constexpr unsigned kWaves = kBlock / 64;
    const long long plane = (long long)a.nx * a.ny * a.nz;
    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned rows = (unsigned)a.e[1] * (unsigned)a.e[2];   // <= 511^2
    for (unsigned r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
        const int z = (int)(r / (unsigned)a.e[1]), y = (int)(r - (unsigned)z * (unsigned)a.e[1]);
        const unsigned long long qyz = brush::axis_term(a.d0[1] + y, a.k[1]) + brush::axis_term(a.d0[2] + z, a.k[2]);
        if (qyz > a.s) continue;
        uint8_t* __restrict__ row = dst + ((long long)(a.o[2] + z) * a.ny + (a.o[1] + y)) * a.nx + a.o[0];
        const uint8_t* __restrict__ srow = stage + (size_t)r * (size_t)a.e[0];
        for (int x = lane; x < a.e[0]; x += 64) {
            const unsigned long long q = qyz + brush::axis_term(a.d0[0] + x, a.k[0]);
            if (q > a.s) continue;
            int k = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                uint8_t* p = row + x + c * plane;
                const unsigned old = *p, nw = srow[(size_t)k * slab + (size_t)x];
                if (nw != old) *p = (uint8_t)nw;
                lo[c] = min(lo[c], nw);
                hi[c] = max(hi[c], nw);
                ++k;
            }
        }
    }
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
    const int ntx = (a.e[0] + kMorphTX - 1) / kMorphTX, nty = (a.e[1] + kMorphTY - 1) / kMorphTY;
    const int bt = blockIdx.x;
    const int tx0 = (bt % ntx) * kMorphTX, ty0 = (bt / ntx % nty) * kMorphTY, tz0 = (bt / (ntx * nty)) * kMorphTZ;
    const int x = tx0 + 4 * xq, y = ty0 + ly, z = tz0 + 2 * zp;   // the first owned texel, in the box

    // the weights of the owned texels: 0 outside the ellipsoid or the box (an inside texel's is at least 1)
    unsigned wgt[2][4];
    const unsigned long long qy = y < a.e[1] ? brush::axis_term(a.d0[1] + y, a.k[1]) : 0ull;
    bool any = false;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wgt[i][j] = 0u;
            if (y < a.e[1] && z + i < a.e[2] && x + j < a.e[0]) {
                const unsigned long long q =
                    qy + brush::axis_term(a.d0[0] + x + j, a.k[0]) + brush::axis_term(a.d0[2] + z + i, a.k[2]);
                if (q <= a.s) wgt[i][j] = brush::weight(q, a.s, a.falloff);
            }
            any = any || wgt[i][j] != 0u;
        }
    if (!__syncthreads_or(any ? 1 : 0)) return;

    const long long plane = (long long)a.nx * a.ny * a.nz;
    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
    int k = 0;   // the channel's slab
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        if (a.strength[c] == 0u) continue;
        const uint8_t* __restrict__ p = src + c * plane;
        for (int i = tid; i < RAW; i += kBlock) {
            const int xw = i % XPW, t = i / XPW, yi = t % YH, zi = t / YH;
            const int gy = clampi(a.o[1] + ty0 - H + yi, 0, a.ny - 1), gz = clampi(a.o[2] + tz0 - H + zi, 0, a.nz - 1);
            const uint8_t* __restrict__ row = p + ((long long)gz * a.ny + gy) * a.nx;
            const int gx = a.o[0] + tx0 - H + 4 * xw;
            uint32_t v = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) v |= (uint32_t)row[clampi(gx + j, 0, a.nx - 1)] << (8 * j);
            raw32[i] = v;
        }
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
    const int ntx = (a.e[0] + kMorphTX - 1) / kMorphTX, nty = (a.e[1] + kMorphTY - 1) / kMorphTY;
    const int bt = blockIdx.x;
    const int tx0 = (bt % ntx) * kMorphTX, ty0 = (bt / ntx % nty) * kMorphTY, tz0 = (bt / (ntx * nty)) * kMorphTZ;
    const int x = tx0 + 4 * xq, y = ty0 + ly, z = tz0 + 2 * zp;   // the first owned texel, in the box

    // the weights of the owned texels: 0 outside the ellipsoid or the box (an inside texel's is at least 1)
    unsigned wgt[2][4];
    const unsigned long long qy = y < a.e[1] ? brush::axis_term(a.d0[1] + y, a.k[1]) : 0ull;
    bool act[2];   // the quad at z + i has a texel inside
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        act[i] = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wgt[i][j] = 0u;
            if (y < a.e[1] && z + i < a.e[2] && x + j < a.e[0]) {
                const unsigned long long q =
                    qy + brush::axis_term(a.d0[0] + x + j, a.k[0]) + brush::axis_term(a.d0[2] + z + i, a.k[2]);
                if (q <= a.s) wgt[i][j] = brush::weight(q, a.s, a.falloff);
            }
            act[i] = act[i] || wgt[i][j] != 0u;
        }
    }
    if (!__syncthreads_or(act[0] || act[1] ? 1 : 0)) return;

    const long long plane = (long long)a.nx * a.ny * a.nz;
    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
    int k = 0;   // the channel's slab
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        if (a.strength[c] == 0u) continue;
        const uint8_t* __restrict__ p = src + c * plane;
        for (int i = tid; i < ZH * YH * XPW; i += kBlock) {
            const int xw = i % XPW, t = i / XPW, yi = t % YH, zi = t / YH;
            const int gy = clampi(a.o[1] + ty0 - H + yi, 0, a.ny - 1), gz = clampi(a.o[2] + tz0 - H + zi, 0, a.nz - 1);
            const uint8_t* __restrict__ row = p + ((long long)gz * a.ny + gy) * a.nx;
            const int gx = a.o[0] + tx0 - H + 4 * xw;
            uint32_t v = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) v |= (uint32_t)row[clampi(gx + j, 0, a.nx - 1)] << (8 * j);
            raw32[zi * ZP + yi * XPW + xw] = v;
        }
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
    constexpr unsigned kWaves = kBlock / 64;
    const PaintArgs& a = g.p;
    const long long plane = (long long)a.nx * a.ny * a.nz;
    const size_t slab = (size_t)a.e[0] * (size_t)a.e[1] * (size_t)a.e[2];
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned rows = (unsigned)a.e[1] * (unsigned)a.e[2];   // <= 511^2
    for (unsigned r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
        const int z = (int)(r / (unsigned)a.e[1]), y = (int)(r - (unsigned)z * (unsigned)a.e[1]);
        const unsigned long long qyz = brush::axis_term(a.d0[1] + y, a.k[1]) + brush::axis_term(a.d0[2] + z, a.k[2]);
        if (qyz > a.s) continue;
        const int sy = clone::source(a.o[1] + y, g.offset[1], g.mirror[1], a.ny);
        const int sz = clone::source(a.o[2] + z, g.offset[2], g.mirror[2], a.nz);
        const long long drow = ((long long)(a.o[2] + z) * a.ny + (a.o[1] + y)) * a.nx + a.o[0];
        const long long srow = ((long long)sz * a.ny + sy) * a.nx;
        for (int x = lane; x < a.e[0]; x += 64) {
            const unsigned long long q = qyz + brush::axis_term(a.d0[0] + x, a.k[0]);
            if (q > a.s) continue;
            const unsigned w = brush::weight(q, a.s, a.falloff);
            const int sx = clone::source(a.o[0] + x, g.offset[0], g.mirror[0], a.nx);
            int k = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                const uint8_t* pc = planes + c * plane;
                const unsigned old = pc[drow + x];
                const unsigned nw = brush::blend(a.op, old, pc[srow + sx], w * a.strength[c]);
                if constexpr (STAGE) {
                    out[(size_t)k * slab + (size_t)r * (size_t)a.e[0] + (size_t)x] = (uint8_t)nw;
                    ++k;
                } else {
                    if (nw != old) out[c * plane + drow + x] = (uint8_t)nw;
                    lo[c] = min(lo[c], nw);
                    hi[c] = max(hi[c], nw);
                }
            }
        }
    }
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
    constexpr unsigned kWaves = kBlock / 64;
    const PaintArgs& a = g.p;
    const long long plane = (long long)a.nx * a.ny * a.nz;
    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned rows = (unsigned)a.e[1] * (unsigned)a.e[2];   // <= 511^2
    for (unsigned r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
        const int z = (int)(r / (unsigned)a.e[1]), y = (int)(r - (unsigned)z * (unsigned)a.e[1]);
        const unsigned long long qyz = brush::axis_term(a.d0[1] + y, a.k[1]) + brush::axis_term(a.d0[2] + z, a.k[2]);
        if (qyz > a.s) continue;
        uint8_t* __restrict__ row = dst + ((long long)(a.o[2] + z) * a.ny + (a.o[1] + y)) * a.nx + a.o[0];
        const uint32_t* __restrict__ srow =
            stamp + (((size_t)g.so[2] + (size_t)z) * (size_t)g.sby + (size_t)g.so[1] + (size_t)y) * (size_t)g.sbx + (size_t)g.so[0];
        for (int x = lane; x < a.e[0]; x += 64) {
            const unsigned long long q = qyz + brush::axis_term(a.d0[0] + x, a.k[0]);
            if (q > a.s) continue;
            const unsigned w = brush::weight(q, a.s, a.falloff);
            const uint32_t v = srow[x];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                uint8_t* p = row + x + c * plane;
                const unsigned old = *p;
                const unsigned nw = brush::blend(a.op, old, (v >> (8 * c)) & 255u, w * a.strength[c]);
                if (nw != old) *p = (uint8_t)nw;
                lo[c] = min(lo[c], nw);
                hi[c] = max(hi[c], nw);
            }
        }
    }
    fold_minmax(lo, hi, mm);
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
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (a.strength[wave] != 0u) {
        const uint32_t* src;
        if constexpr (DEVICE_LUT) src = lut.t;
        else src = reinterpret_cast<const uint32_t*>(&lut.t);
        table[wave * 64 + lane] = src[wave * 64 + lane];
    }
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(table);
    const unsigned rows = (unsigned)a.e[1] * (unsigned)a.e[2];   // <= 511^2
    for (unsigned r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
        const int z = (int)(r / (unsigned)a.e[1]), y = (int)(r - (unsigned)z * (unsigned)a.e[1]);
        const unsigned long long qyz = brush::axis_term(a.d0[1] + y, a.k[1]) + brush::axis_term(a.d0[2] + z, a.k[2]);
        if (qyz > a.s) continue;
        uint8_t* __restrict__ row = dst + ((long long)(a.o[2] + z) * a.ny + (a.o[1] + y)) * a.nx + a.o[0];
        for (int x = lane; x < a.e[0]; x += 64) {
            const unsigned long long q = qyz + brush::axis_term(a.d0[0] + x, a.k[0]);
            if (q > a.s) continue;
            const unsigned w = brush::weight(q, a.s, a.falloff);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (a.strength[c] == 0u) continue;
                uint8_t* p = row + x + c * plane;
                const unsigned old = *p;
                const unsigned nw = brush::blend(a.op, old, bytes[c * 256 + (int)old], w * a.strength[c]);
                if (nw != old) *p = (uint8_t)nw;
                lo[c] = min(lo[c], nw);
                hi[c] = max(hi[c], nw);
            }
        }
    }
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

// vr_get_volume_box: the planes' texel box -> tightly packed RGBA8 (what
// k_update_planar reads).  One thread per texel, one 4-byte store each.
__global__ __launch_bounds__(kBlock) void k_unpack_box(const uint8_t* __restrict__ src, int nx, int ny, int nz,
                                                       int x0, int y0, int z0, int bx, int by, int bz,
                                                       uchar4* __restrict__ dst)
{
    const unsigned total = (unsigned)bx * (unsigned)by * (unsigned)bz;   // < 2^31 (inside the volume)
    const long long plane = (long long)nx * ny * nz;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
        const unsigned t = i / (unsigned)bx;
        const int x = (int)(i - t * (unsigned)bx), y = (int)(t % (unsigned)by), z = (int)(t / (unsigned)by);
        const long long s = ((long long)(z0 + z) * ny + (y0 + y)) * nx + (x0 + x);
        dst[i] = make_uchar4(src[s], src[s + plane], src[s + 2 * plane], src[s + 3 * plane]);
    }
}

// Fast layouts, built from the planar planes.  Every element stores
// clamp-to-edge texels of the padded base position (a, b, c), where texel
// index = padded index - 1 (vr_internal.h Layout).
struct PlaneSrc {
    const uint8_t* p;
    int nx, ny, nz;
    __device__ __forceinline__ unsigned int at(int a, int b, int c) const  // padded coordinates
    {
        const int x = clampi(a - 1, 0, nx - 1), y = clampi(b - 1, 0, ny - 1), z = clampi(c - 1, 0, nz - 1);
        return p[((long long)z * ny + y) * nx + x];
    }
};

// One thread per output element: a byte of an apron brick, or one 8-byte
// footprint word (CORNER8).  Brick order and in-brick order match
// axis_offset() in vr_internal.h, which the march kernel's LDS tables use.
// Builds the bricks [o, o + n) per axis (CORNERH: positions; its "brick" is
// one 16-B word): the full build is o = 0, n = (nbx, nby, nbz), a box update
// (launch_build_layout_box) the bricks that store a texel of the box.
struct BuildRange {
    int o[3], n[3];
};
template <int LAYOUT>
__global__ __launch_bounds__(kBlock) void k_build_layout(const uint8_t* __restrict__ planar, int nx, int ny,
                                                         int nz, LayoutGeom g, BuildRange r,
                                                         long long plane_bytes, uint8_t* __restrict__ out, int nch = 4)
{
    const long long total_planar = (long long)nx * ny * nz;
    // elements per brick
    const long long per = LAYOUT == LAYOUT_CORNER8 ? 64 : LAYOUT == LAYOUT_CORNERH ? 1
                        : LAYOUT == LAYOUT_ZPAIR ? 128 : (long long)g.brick;
    const long long range_elems = per * r.n[0] * r.n[1] * r.n[2];
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < nch * range_elems;
         i += (long long)gridDim.x * kBlock) {
        const int ch = (int)(i / range_elems);
        const long long l = i - ch * range_elems;
        const long long lb = l / per;   // brick of the range, x fastest
        const int in = (int)(l - lb * per);
        const int bx = r.o[0] + (int)(lb % r.n[0]);
        const long long t = lb / r.n[0];
        const int by = r.o[1] + (int)(t % r.n[1]), bz = r.o[2] + (int)(t / r.n[1]);
        const long long e = (((long long)bz * g.nby + by) * g.nbx + bx) * per + in;   // element of the plane
        const PlaneSrc src{planar + ch * total_planar, nx, ny, nz};
        uint8_t* dst = out + ch * plane_bytes;
        if constexpr (LAYOUT == LAYOUT_CORNER8) {
            const int pos = in;
            const int a = 4 * bx + (pos & 3), b = 4 * by + ((pos >> 2) & 3), c = 4 * bz + (pos >> 4);
            unsigned long long q = 0;
            for (int k = 0; k < 8; ++k)
                q |= (unsigned long long)src.at(a + (k & 1), b + ((k >> 1) & 1), c + (k >> 2)) << (8 * k);
            reinterpret_cast<unsigned long long*>(dst)[e] = q;
        } else if constexpr (LAYOUT == LAYOUT_CORNERH) {
            // position (a, b, c), x fastest; dword k = footprint row (y, z) =
            // (b + (k & 1), c + (k >> 1)): f16 a in the low half, f16 (b - a)
            // in the high half (both exact: |values| <= 255)
            const int a = bx, b = by, c = bz;
            unsigned w[4];
            for (int k = 0; k < 4; ++k) {
                const int y = b + (k & 1), z = c + (k >> 1);
                const int va = (int)src.at(a, y, z), vb = (int)src.at(a + 1, y, z);
                const _Float16 ha = (_Float16)(float)va, hd = (_Float16)(float)(vb - va);
                w[k] = (unsigned)__builtin_bit_cast(unsigned short, ha) |
                       ((unsigned)__builtin_bit_cast(unsigned short, hd) << 16);
            }
            reinterpret_cast<uint4*>(dst)[e] = make_uint4(w[0], w[1], w[2], w[3]);
        } else if constexpr (LAYOUT == LAYOUT_ZPAIR) {
            // byte = x + 4 * (z + 2 * y): 4-byte rows, z fastest
            const int byte = in;
            dst[e] = src.at(3 * bx + (byte & 3), 15 * by + (byte >> 3), bz + ((byte >> 2) & 1));
        } else {
            const int byte = in;
            unsigned int v = 0;
            if (byte < g.Rn[0] * g.Rn[1] * g.Rn[2]) {
                const int u = byte % g.Rn[0], vv = (byte / g.Rn[0]) % g.Rn[1], w = byte / (g.Rn[0] * g.Rn[1]);
                v = src.at(g.Ba[0] * bx + u, g.Ba[1] * by + vv, g.Ba[2] * bz + w);
            }
            dst[e] = (uint8_t)v;
        }
    }
}

// The apron-brick layouts (BRICK4 family, BRICK5/8/16), staged through LDS.
// A workgroup builds a run of `run` consecutive bricks along x at one
// (by, bz): it loads their source box -- Rn[1] x Rn[2] planar rows of
// Ba[0] (run - 1) + Rn[0] bytes, clamped to the edge -- with coalesced byte
// loads (consecutive lanes, consecutive x), then writes the run, which is
// contiguous in the layout, as 16-B stores gathered from LDS.  The per-byte
// kernel before it (a 1-B store and 8 scattered planar reads per thread,
// 64-bit decode) took 4.0 ms at 512^3.
constexpr int kBrickStageBytes = 16 * 1024;
//
// zseg > 0 (COL48, whose columns run through the whole z extent): a workgroup
// builds segment blockIdx.y -- slices [zseg * seg, zseg * (seg + 1)) -- of a
// run of columns; a column's segment is contiguous, the run's columns sit a
// column (g.brick bytes) apart.
//
// The grid covers the bricks r.o[0] + [0, r.n[0]) in runs along x, r.o[1] +
// [0, r.n[1]) along y and r.o[2] + [0, gridDim.y) along z (zseg > 0: segments):
// everything for the full build, the bricks a box update touches otherwise.
__global__ __launch_bounds__(kBlock) void k_build_bricks(const uint8_t* __restrict__ planar, int nx, int ny, int nz,
                                                         LayoutGeom g, BuildRange r, int run, long long plane_bytes,
                                                         int zseg, uint8_t* __restrict__ out)
{
    __shared__ uint8_t st[kBrickStageBytes];
    const int ch = blockIdx.z;
    const uint8_t* __restrict__ p = planar + (long long)ch * nx * ny * nz;
    const int runs_x = (r.n[0] + run - 1) / run;
    const int rx = (int)blockIdx.x % runs_x, by = r.o[1] + (int)blockIdx.x / runs_x, bz = r.o[2] + (int)blockIdx.y;
    const int bx0 = r.o[0] + rx * run, nb = min(run, r.o[0] + r.n[0] - bx0);
    const int rn0 = g.Rn[0], rn1 = g.Rn[1], rn2 = zseg > 0 ? min(zseg, g.Rn[2] - zseg * bz) : g.Rn[2];
    // slice w of a COL48 column holds padded z position w (texel w - 1)
    const int x0 = g.Ba[0] * bx0 - 1, y0 = g.Ba[1] * by - 1, z0 = zseg > 0 ? zseg * bz - 1 : g.Ba[2] * bz - 1;
    const int xe = x0 + g.Ba[0] * (nb - 1) + rn0;    // one past the last staged x
    const int rows = rn1 * rn2;
    // stage: rows (v, w) of the source box, x fastest over the whole workgroup.
    // Runs inside the volume along x with dword-aligned planar rows take
    // aligned dword loads (xa = x0 & ~3 .. xe rounded up); the edge runs
    // clamp byte by byte.
    const int xa = x0 & ~3, wx = ((xe + 3) & ~3) - xa;   // staged row: [xa, xa + wx)
    if (xa >= 0 && xa + wx <= nx && (nx & 3) == 0) {
        const int wd = wx >> 2, total = rows * wd;
        unsigned* st4 = reinterpret_cast<unsigned*>(st);
#pragma unroll 4
        for (int i = threadIdx.x; i < total; i += kBlock) {
            const int row = i / wd, xi = i - row * wd;
            const int w = row / rn1, v = row - w * rn1;
            const int y = clampi(y0 + v, 0, ny - 1), z = clampi(z0 + w, 0, nz - 1);
            st4[i] = *reinterpret_cast<const unsigned*>(
                p + ((unsigned)z * (unsigned)ny + (unsigned)y) * (unsigned)nx + (unsigned)(xa + 4 * xi));
        }
    } else {
        const int total = rows * wx;
        for (int i = threadIdx.x; i < total; i += kBlock) {
            const int row = i / wx, xi = i - row * wx;
            const int w = row / rn1, v = row - w * rn1;
            const int x = clampi(xa + xi, 0, nx - 1), y = clampi(y0 + v, 0, ny - 1), z = clampi(z0 + w, 0, nz - 1);
            st[i] = p[((unsigned)z * (unsigned)ny + (unsigned)y) * (unsigned)nx + (unsigned)x];
        }
    }
    __syncthreads();
    // write: the run's bricks are contiguous, brick by brick in-brick order x
    // fastest (COL48: each column's segment is contiguous, columns g.brick apart)
    const unsigned used = (unsigned)(rn0 * rn1 * rn2);
    const unsigned per_brick = zseg > 0 ? used / 16u : g.brick / 16u;   // COL48: 32 B per slice
    uint8_t* __restrict__ dst0 = out + (long long)ch * plane_bytes +
                                 (zseg > 0 ? ((long long)by * g.nbx + bx0) * g.brick + (long long)bz * rn0 * rn1 * zseg
                                           : ((long long)(bz * g.nby + by) * g.nbx + bx0) * g.brick);
    for (unsigned c = threadIdx.x; c < (unsigned)nb * per_brick; c += kBlock) {
        const unsigned j = c / per_brick, b0 = (c - j * per_brick) * 16u;
        uint4* __restrict__ dst = reinterpret_cast<uint4*>(dst0 + (long long)j * g.brick) - j * per_brick;
        unsigned u = b0 % (unsigned)rn0, v = (b0 / (unsigned)rn0) % (unsigned)rn1, w = b0 / (unsigned)(rn0 * rn1);
        const unsigned xb = j * (unsigned)g.Ba[0] + (unsigned)(x0 - xa);
        unsigned word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (b0 + (unsigned)k < used)
                word[k >> 2] |= (unsigned)st[(w * (unsigned)rn1 + v) * (unsigned)wx + xb + u] << (8 * (k & 3));
            if (++u == (unsigned)rn0) { u = 0; if (++v == (unsigned)rn1) { v = 0; ++w; } }
        }
        dst[c] = make_uint4(word[0], word[1], word[2], word[3]);
    }
}

__global__ __launch_bounds__(kBlock) void k_unpack_planar(const uint8_t* __restrict__ src, long long total,
                                                          uchar4* __restrict__ dst)
{
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < total;
         i += (long long)gridDim.x * kBlock)
        dst[i] = make_uchar4(src[i], src[i + total], src[i + 2 * total], src[i + 3 * total]);
}

// GenUniformGrid3D: pos = (start + idx) * freq, x fastest.  Each block also
// writes its {min, max}; k_minmax folds them (exact, order-independent).
// kind 0 cellular, 1 Perlin, 2 simplex.  cell_n > 0 (cellular only): the
// workgroup first puts the feature-point data of the cells [cell_lo,
// cell_lo + cell_n)^3 in LDS (noise::cellular_cell, the procedural march's
// table) and evaluates F1 with noise::cellular_table -- bit-identical to
// noise::cellular, 7 VALU ops per cell instead of the hash, sqrt and
// reciprocal.  The host sizes the cell range from the grid's coordinate range.
constexpr int kNoiseTableMaxN = 12;
__global__ __launch_bounds__(kBlock) void k_noise(int kind, float* __restrict__ out, int x0, int y0, int z0,
                                                  int nx, int ny, int nz, float freq, int32_t seed,
                                                  int cell_lo, int cell_n, float2* __restrict__ partials)
{
    extern __shared__ float4 cells[];   // cell_n^3 entries (dynamic: none for Perlin / simplex)
    if (cell_n > 0) {
        const int n = cell_n;
        for (int i = threadIdx.x; i < n * n * n; i += kBlock) {
            const int ix = i % n, iy = (i / n) % n, iz = i / (n * n);
            cells[i] = noise::cellular_cell(seed, cell_lo + ix, cell_lo + iy, cell_lo + iz);
        }
        __syncthreads();
    }
    const unsigned total = (unsigned)nx * (unsigned)ny * (unsigned)nz;   // < 2^32 (host check)
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
        const unsigned t = i / (unsigned)nx;
        const int x = (int)(i - t * (unsigned)nx);
        const int y = (int)(t % (unsigned)ny), z = (int)(t / (unsigned)ny);
        const float px = (float)(x0 + x) * freq, py = (float)(y0 + y) * freq, pz = (float)(z0 + z) * freq;
        float v;
        if (kind == 0) v = cell_n > 0 ? noise::cellular_table(cells, cell_lo, cell_n, cell_n * cell_n, px, py, pz)
                                      : noise::cellular(seed, px, py, pz);
        else if (kind == 1) v = noise::perlin(seed, px, py, pz);
        else v = noise::simplex(seed, px, py, pz);
        if (out) out[i] = v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    __shared__ float2 red[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = make_float2(mn, mx);
    __syncthreads();
    if (threadIdx.x == 0) {
        float2 r = red[0];
        for (int w = 1; w < kBlock / 64; ++w) { r.x = fminf(r.x, red[w].x); r.y = fmaxf(r.y, red[w].y); }
        partials[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(kBlock) void k_minmax(const float2* __restrict__ partials, int n, float* __restrict__ out)
{
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int i = threadIdx.x; i < n; i += kBlock) { mn = fminf(mn, partials[i].x); mx = fmaxf(mx, partials[i].y); }
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    __shared__ float2 red[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = make_float2(mn, mx);
    __syncthreads();
    if (threadIdx.x == 0) {
        float2 r = red[0];
        for (int w = 1; w < kBlock / 64; ++w) { r.x = fminf(r.x, red[w].x); r.y = fmaxf(r.y, red[w].y); }
        out[0] = r.x;
        out[1] = r.y;
    }
}

// static_cast<unsigned char>(float) as x86-64 compiles it (cvttss2si, keep
// the low byte): TestMain.cpp:84-87.
__device__ __forceinline__ unsigned int f2u8_trunc(float f)
{
    if (!(f > -2147483648.0f && f < 2147483648.0f)) return 0u;
    return (unsigned int)(int)f & 0xffu;
}

// TestMain.cpp:64-92.  g2 == nullptr means the zero-filled noiseOutput2 of
// the literal recipe.  minmax = {min1,max1, min2,max2, min3,max3, min4,max4}.
__global__ __launch_bounds__(kBlock) void k_pack_recipe(const float* __restrict__ g1, const float* __restrict__ g2,
                                                        const float* __restrict__ g3, const float* __restrict__ g4,
                                                        const float* __restrict__ mm, long long total,
                                                        uchar4* __restrict__ out)
{
    const float inv1 = 1.0f / (mm[1] - mm[0]), inv2 = 1.0f / (mm[3] - mm[2]);
    const float inv3 = 1.0f / (mm[5] - mm[4]), inv4 = 1.0f / (mm[7] - mm[6]);
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < total;
         i += (long long)gridDim.x * kBlock) {
        float s1 = 1.0f - (g1[i] - mm[0]) * inv1;
        const float s2 = 1.0f - ((g2 ? g2[i] : 0.0f) - mm[2]) * inv2;
        const float s3 = 1.0f - (g3[i] - mm[4]) * inv3;
        const float s4 = 1.0f - (g4[i] - mm[6]) * inv4;
        s1 = s1 * ((s1 * s1) * s1);
        out[i] = make_uchar4(f2u8_trunc(s1 * 255.0f), f2u8_trunc(s2 * 255.0f), f2u8_trunc(s3 * 255.0f),
                             f2u8_trunc(s4 * 255.0f));
    }
}

// frame row y lives in band b = y / band_rows, rendered by rank b % nranks as
// its (b / nranks)-th band.  16-byte chunks when rows allow it.  Rows of ranks
// below first_rank are left as they are (rendered in place into the frame,
// vr.h VR_TARGET_BANDS_IN_PLACE).
//
// Row q (from rank first_rank's slot on) of the gathered band sets -> its
// frame row y: rank r's slot holds its bands lb = 0, 1, ... packed, and band
// lb of rank r is frame band lb * nranks + r -- or, serpentine (vr_target
// band_flip nranks - 1 - 2r), lb * nranks + nranks - 1 - r for odd lb.  -1 for slot rows past the
// frame (a rank with fewer rows than the slot).  Block-uniform: the divisions
// are scalar, once per row.
__device__ __forceinline__ int assembled_row(int q, int rows_per_rank, int nranks, int band_rows, int first_rank,
                                             int serp, int height)
{
    const int r = first_rank + q / rows_per_rank, lr = q % rows_per_rank;
    const int lb = lr / band_rows, rr = lr - lb * band_rows;
    const int y = (lb * nranks + ((serp && (lb & 1)) ? nranks - 1 - r : r)) * band_rows + rr;
    return y < height ? y : -1;
}

// The assembly kernels (vr_assemble_frame): rows x elements.  Each lane moves
// up to kAsmBatch rows' elements with all the loads in flight before the
// first store (frames taller than the grid); the frame row comes from
// block-uniform scalar arithmetic, with no per-element division.
constexpr int kAsmBatch = 8;
template <typename S, typename D, typename F>
__device__ __forceinline__ void assemble_rows(const S* __restrict__ src, int rows_per_rank, int nranks, int row_elems,
                                              int height, int band_rows, int first_rank, int serp, D* __restrict__ dst,
                                              F expand)
{
    const int rows = (nranks - first_rank) * rows_per_rank;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= row_elems) return;
    const size_t base = (size_t)first_rank * rows_per_rank;
    for (int q0 = blockIdx.y; q0 < rows; q0 += gridDim.y * kAsmBatch) {
        S v[kAsmBatch];
        int y[kAsmBatch];
#pragma unroll
        for (int j = 0; j < kAsmBatch; ++j) {
            const int q = q0 + j * (int)gridDim.y;
            y[j] = q < rows ? assembled_row(q, rows_per_rank, nranks, band_rows, first_rank, serp, height) : -1;
            if (y[j] >= 0) v[j] = src[(base + q) * row_elems + e];
        }
#pragma unroll
        for (int j = 0; j < kAsmBatch; ++j)
            if (y[j] >= 0) dst[(size_t)y[j] * row_elems + e] = expand(v[j]);
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_assemble(const T* __restrict__ src, int rows_per_rank, int nranks,
                                                     int row_elems, int height, int band_rows, int first_rank,
                                                     int serp, T* __restrict__ dst)
{
    assemble_rows(src, rows_per_rank, nranks, row_elems, height, band_rows, first_rank, serp, dst,
                  [](T v) { return v; });
}

// Grey band sets -> RGBA frame (vr_assemble_frame): element e of frame row y
// comes from the same place k_assemble reads, expanded.  P pixels per element:
// u8 x 4 (uchar4 -> 4 RGBA8 words, rows of a multiple of 4 pixels), u8 x 1,
// or fp32 x 1 (-> float4).
template <typename S, typename D>
__device__ __forceinline__ D grey_expand(S v);
template <>
__device__ __forceinline__ uint4 grey_expand<unsigned int, uint4>(unsigned int v)
{
    uint4 o;
    unsigned q = v & 0xffu;
    o.x = q * 0x010101u | 0xff000000u;
    q = (v >> 8) & 0xffu;
    o.y = q * 0x010101u | 0xff000000u;
    q = (v >> 16) & 0xffu;
    o.z = q * 0x010101u | 0xff000000u;
    q = v >> 24;
    o.w = q * 0x010101u | 0xff000000u;
    return o;
}
template <>
__device__ __forceinline__ unsigned int grey_expand<unsigned char, unsigned int>(unsigned char v)
{
    return (unsigned)v * 0x010101u | 0xff000000u;
}
template <>
__device__ __forceinline__ float4 grey_expand<float, float4>(float v)
{
    return make_float4(v, v, v, 1.0f);
}
template <typename S, typename D>
__global__ __launch_bounds__(kBlock) void k_assemble_grey(const S* __restrict__ src, int rows_per_rank,
                                                          int nranks, int row_elems, int height, int band_rows,
                                                          int first_rank, int serp, D* __restrict__ dst)
{
    assemble_rows(src, rows_per_rank, nranks, row_elems, height, band_rows, first_rank, serp, dst,
                  [](S v) { return grey_expand<S, D>(v); });
}

// grid of the assembly kernels: ceil(elems / kBlock) workgroups across a row,
// rows over blockIdx.y -- about 2048 workgroups in all, so 7/8 of a 1080p
// frame is one row per workgroup row (more, smaller workgroups run faster
// beside the other stream's march: profiles/r05/assembly_grid.txt)
dim3 grid_rows(size_t rows_per_rank, int nranks, int first_rank, long long elems)
{
    const long long rows = (long long)(nranks - first_rank) * (long long)rows_per_rank;
    const long long gx = (elems + kBlock - 1) / kBlock;
    constexpr long long target = 2048;   // rank 0 at N = 8: 0.0212 ms/frame, 0.0215 at 1024, 0.0220 at 512, 0.0245 at 128
    const long long gy = std::max(1LL, std::min({rows, (target + gx - 1) / gx, 65535LL}));
    return dim3((unsigned)gx, (unsigned)gy);
}

int grid_for(long long n)
{
    long long g = (n + kBlock - 1) / kBlock;
    if (g > 256 * 16) g = 256 * 16;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

// Byte min / max of each plane (blockIdx.y = plane): grid-stride bytes, a
// wave reduction, one atomicMin / atomicMax per wave.
__global__ __launch_bounds__(kBlock) void k_plane_minmax(const uint8_t* __restrict__ planes, long long total,
                                                         unsigned* __restrict__ mm)
{
    const uint8_t* pl = planes + (size_t)blockIdx.y * (size_t)total;
    unsigned lo = 255u, hi = 0u;
    // the 4-byte-aligned body as words, the rest as bytes
    const long long mis = (long long)((4u - (unsigned)((uintptr_t)pl & 3u)) & 3u);
    const long long head = mis < total ? mis : total;
    const long long words = (total - head) / 4;
    const unsigned* w = reinterpret_cast<const unsigned*>(pl + head);
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < words; i += stride) {
        const unsigned v = w[i];
        const unsigned b0 = v & 0xffu, b1 = (v >> 8) & 0xffu, b2 = (v >> 16) & 0xffu, b3 = v >> 24;
        lo = min(lo, min(min(b0, b1), min(b2, b3)));
        hi = max(hi, max(max(b0, b1), max(b2, b3)));
    }
    const long long tail0 = head + words * 4;
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < head + (total - tail0); i += stride) {
        const unsigned b = i < head ? pl[i] : pl[tail0 + (i - head)];
        lo = min(lo, b);
        hi = max(hi, b);
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, off));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, off));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[blockIdx.y], lo);
        atomicMax(&mm[4 + blockIdx.y], hi);
    }
}

hipError_t launch_plane_minmax(const uint8_t* d_planar, long long total, unsigned* mm, hipStream_t s)
{
    long long g = (total / 4 + kBlock - 1) / kBlock;
    g = g < 1 ? 1 : g > 1024 ? 1024 : g;
    hipLaunchKernelGGL(k_plane_minmax, dim3((unsigned)g, 4), dim3(kBlock), 0, s, d_planar, total, mm);
    return hipGetLastError();
}

hipError_t launch_repack(const uint8_t* d_rgba, int nx, int ny, int nz, uint8_t* d_planar, hipStream_t s)
{
    const long long total = (long long)nx * ny * nz;
    hipLaunchKernelGGL(k_repack_planar, dim3(grid_for(total)), dim3(kBlock), 0, s,
                       reinterpret_cast<const uchar4*>(d_rgba), total, d_planar);
    return hipGetLastError();
}

namespace {
long long layout_elems(int layout, int nx, int ny, int nz)
{
    const LayoutGeom g = layout_geom(layout, nx, ny, nz);
    const long long nb = (long long)g.nbx * g.nby * g.nbz;
    return layout == LAYOUT_CORNER8 ? nb * 64 : layout == LAYOUT_CORNERH ? nb : nb * g.brick;
}
int elem_bytes(int layout) { return layout == LAYOUT_CORNER8 ? 8 : layout == LAYOUT_CORNERH ? 16 : 1; }
}  // namespace

size_t layout_plane_bytes(int layout, int nx, int ny, int nz)
{
    const size_t b = (size_t)layout_elems(layout, nx, ny, nz) * elem_bytes(layout);
    return (b + 255) & ~(size_t)255;
}

size_t layout_total_bytes(int layout, int nx, int ny, int nz)
{
    if (layout == LAYOUT_COL48Z)   // three COL48 planes, then channel 3's ZPAIR plane
        return 3 * layout_plane_bytes(LAYOUT_COL48, nx, ny, nz) + layout_plane_bytes(LAYOUT_ZPAIR, nx, ny, nz);
    return 4 * layout_plane_bytes(layout, nx, ny, nz);
}

namespace {
// Build the bricks of range r (k_build_layout's units; COL48 / COL48Z: columns
// in x and y, 32-slice segments in z) of a fast layout from the planar planes.
constexpr int kColSeg = 32;   // COL48 z segment: 1 KiB of a column, BRICK4832's stage
hipError_t launch_build_range(int layout, const uint8_t* d_planar, int nx, int ny, int nz, uint8_t* d_out,
                              const BuildRange& r, hipStream_t s)
{
    const LayoutGeom g = layout_geom(layout, nx, ny, nz);
    const long long pb = (long long)layout_plane_bytes(layout, nx, ny, nz);
    const dim3 b(kBlock);
    const long long rows = (long long)g.Rn[1] * g.Rn[2];
    if (layout == LAYOUT_COL48 || layout == LAYOUT_COL48Z) {
        const int nch = layout == LAYOUT_COL48Z ? 3 : 4;   // COL48Z: channel 3 is ZPAIR's, below
        const long long srows = (long long)g.Rn[1] * kColSeg;
        const int run = (int)std::min<long long>(r.n[0], (kBrickStageBytes / srows - g.Rn[0] - 7) / g.Ba[0] + 1);
        const int runs_x = (r.n[0] + run - 1) / run;
        const dim3 gb((unsigned)(runs_x * r.n[1]), (unsigned)r.n[2], nch);   // the column's last segment is partial
        hipLaunchKernelGGL(k_build_bricks, gb, b, 0, s, d_planar, nx, ny, nz, g, r, run, pb, kColSeg, d_out);
        if (layout == LAYOUT_COL48Z) {   // (full builds only: the ZPAIR plane is built whole)
            const LayoutGeom gz = layout_geom(LAYOUT_ZPAIR, nx, ny, nz);
            const long long ez = layout_elems(LAYOUT_ZPAIR, nx, ny, nz);
            const BuildRange rz{{0, 0, 0}, {gz.nbx, gz.nby, gz.nbz}};
            hipLaunchKernelGGL(k_build_layout<LAYOUT_ZPAIR>, dim3(grid_for(ez)), b, 0, s,
                               d_planar + 3 * (long long)nx * ny * nz, nx, ny, nz, gz, rz,
                               (long long)layout_plane_bytes(LAYOUT_ZPAIR, nx, ny, nz), d_out + 3 * pb, 1);
        }
        return hipGetLastError();
    }
    if (layout != LAYOUT_CORNER8 && layout != LAYOUT_CORNERH && layout != LAYOUT_ZPAIR && g.brick % 16u == 0 &&
        rows * (g.Ba[0] + g.Rn[0] + 8) <= kBrickStageBytes) {
        // bricks per workgroup: the longest run whose source box (+ up to 7
        // bytes of dword alignment per row) fits the stage
        const int run = (int)std::min<long long>(r.n[0], (kBrickStageBytes / rows - g.Rn[0] - 7) / g.Ba[0] + 1);
        const int runs_x = (r.n[0] + run - 1) / run;
        const dim3 gb((unsigned)(runs_x * r.n[1]), (unsigned)r.n[2], 4);
        hipLaunchKernelGGL(k_build_bricks, gb, b, 0, s, d_planar, nx, ny, nz, g, r, run, pb, 0, d_out);
        return hipGetLastError();
    }
    const long long per = layout == LAYOUT_CORNER8 ? 64 : layout == LAYOUT_CORNERH ? 1
                        : layout == LAYOUT_ZPAIR ? 128 : (long long)g.brick;
    const dim3 gr(grid_for(4 * per * r.n[0] * r.n[1] * r.n[2]));
    switch (layout) {
    case LAYOUT_BRICK4: hipLaunchKernelGGL(k_build_layout<LAYOUT_BRICK4>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_BRICK5: hipLaunchKernelGGL(k_build_layout<LAYOUT_BRICK5>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_BRICK8: hipLaunchKernelGGL(k_build_layout<LAYOUT_BRICK8>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_BRICK16: hipLaunchKernelGGL(k_build_layout<LAYOUT_BRICK16>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_BRICK448: hipLaunchKernelGGL(k_build_layout<LAYOUT_BRICK448>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_BRICK488: hipLaunchKernelGGL(k_build_layout<LAYOUT_BRICK488>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_BRICK4816: hipLaunchKernelGGL(k_build_layout<LAYOUT_BRICK4816>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_BRICK4864: hipLaunchKernelGGL(k_build_layout<LAYOUT_BRICK4864>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_BRICK4832: hipLaunchKernelGGL(k_build_layout<LAYOUT_BRICK4832>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_COL48: hipLaunchKernelGGL(k_build_layout<LAYOUT_COL48>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_BRICK41616: hipLaunchKernelGGL(k_build_layout<LAYOUT_BRICK41616>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_ZPAIR: hipLaunchKernelGGL(k_build_layout<LAYOUT_ZPAIR>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_CORNER8: hipLaunchKernelGGL(k_build_layout<LAYOUT_CORNER8>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    case LAYOUT_CORNERH: hipLaunchKernelGGL(k_build_layout<LAYOUT_CORNERH>, gr, b, 0, s, d_planar, nx, ny, nz, g, r, pb, d_out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
}  // namespace

// The full build: the range that holds every brick.
hipError_t launch_build_layout(int layout, const uint8_t* d_planar, int nx, int ny, int nz, uint8_t* d_out,
                               hipStream_t s)
{
    const LayoutGeom g = layout_geom(layout, nx, ny, nz);
    const bool col = layout == LAYOUT_COL48 || layout == LAYOUT_COL48Z;
    const BuildRange r{{0, 0, 0}, {g.nbx, g.nby, col ? (g.Rn[2] + kColSeg - 1) / kColSeg : g.nbz}};
    return launch_build_range(layout, d_planar, nx, ny, nz, d_out, r, s);
}

hipError_t launch_update_planar(const uint8_t* d_box, int nx, int ny, int nz, int x0, int y0, int z0, int bx, int by,
                                int bz, uint8_t* d_planar, unsigned* mm, hipStream_t s)
{
    hipLaunchKernelGGL(k_update_planar, dim3(grid_for((long long)bx * by * bz)), dim3(kBlock), 0, s,
                       reinterpret_cast<const uchar4*>(d_box), nx, ny, nz, x0, y0, z0, bx, by, bz, d_planar, mm);
    return hipGetLastError();
}

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
    const long long tiles = (long long)((a.e[0] + kBlurTX - 1) / kBlurTX) * ((a.e[1] + kBlurTY - 1) / kBlurTY) *
                            ((a.e[2] + kBlurTZ - 1) / kBlurTZ);
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
    const long long tiles = (long long)((a.e[0] + kMorphTX - 1) / kMorphTX) * ((a.e[1] + kMorphTY - 1) / kMorphTY) *
                            ((a.e[2] + kMorphTZ - 1) / kMorphTZ);
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
    const long long tiles = (long long)((a.e[0] + kMorphTX - 1) / kMorphTX) * ((a.e[1] + kMorphTY - 1) / kMorphTY) *
                            ((a.e[2] + kMorphTZ - 1) / kMorphTZ);
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

hipError_t launch_unpack_box(const uint8_t* d_planar, int nx, int ny, int nz, int x0, int y0, int z0, int bx, int by,
                             int bz, uint8_t* d_box, hipStream_t s)
{
    hipLaunchKernelGGL(k_unpack_box, dim3(grid_for((long long)bx * by * bz)), dim3(kBlock), 0, s, d_planar, nx, ny, nz,
                       x0, y0, z0, bx, by, bz, reinterpret_cast<uchar4*>(d_box));
    return hipGetLastError();
}

// the default build's layouts, which launch_build_layout_box rebuilds over a box
bool layout_rebuilds_box(int layout)
{
    return layout == LAYOUT_CORNERH || layout == LAYOUT_CORNER8 || layout == LAYOUT_BRICK4832 || layout == LAYOUT_COL48;
}

// A fast layout stores texel x (padded index x + 1) under the base positions
// x and x + 1, and the clamp-to-edge copies of texels 0 and N - 1 under the
// positions 0 and N: the box [x0, x0 + bx) changes the positions [x0, x0 + bx]
// per axis -- the box and a halo of one position.  The bricks that hold them
// are [lo / Ba, hi / Ba] per axis (layout_geom / axis_offset): the brick q
// stores the padded texels Ba q .. Ba q + Ba, so a texel on a brick boundary
// lies in both neighbours, and the last brick holds everything past N.
hipError_t launch_build_layout_box(int layout, const uint8_t* d_planar, int nx, int ny, int nz, uint8_t* d_out,
                                   int x0, int y0, int z0, int bx, int by, int bz, hipStream_t s)
{
    if (!layout_rebuilds_box(layout))
        return launch_build_layout(layout, d_planar, nx, ny, nz, d_out, s);   // VR_EXPERIMENTS layouts: all of it
    const LayoutGeom g = layout_geom(layout, nx, ny, nz);
    const int lo[3] = {x0, y0, z0}, hi[3] = {x0 + bx, y0 + by, z0 + bz};
    BuildRange r{};
    for (int ax = 0; ax < 3; ++ax) {
        // Ba: CORNER8's footprint words sit in 4^3 position bricks (the update rewrites
        // whole ones), CORNERH's are addressed one by one (Ba = 1: the position box itself)
        r.o[ax] = lo[ax] / g.Ba[ax];
        r.n[ax] = hi[ax] / g.Ba[ax] - r.o[ax] + 1;
    }
    if (layout == LAYOUT_COL48) {
        // one column through z: slice w holds padded z position w (texel w - 1), and
        // the slices past nz + 1 (the even count) repeat the last texel
        const int last = z0 + bz == nz ? g.Rn[2] - 1 : z0 + bz;
        r.o[2] = z0 / kColSeg;
        r.n[2] = last / kColSeg - r.o[2] + 1;
    }
    return launch_build_range(layout, d_planar, nx, ny, nz, d_out, r, s);
}

hipError_t launch_unpack(const uint8_t* d_planar, int nx, int ny, int nz, uint8_t* d_rgba, hipStream_t s)
{
    const long long total = (long long)nx * ny * nz;
    hipLaunchKernelGGL(k_unpack_planar, dim3(grid_for(total)), dim3(kBlock), 0, s, d_planar, total,
                       reinterpret_cast<uchar4*>(d_rgba));
    return hipGetLastError();
}

int noise_partials_needed(int nx, int ny, int nz) { return grid_for((long long)nx * ny * nz); }

hipError_t launch_noise(int kind, float* d_out, int x0, int y0, int z0, int nx, int ny, int nz, float freq,
                        int32_t seed, float* d_partials, int* num_partials, hipStream_t s)
{
    const int g = grid_for((long long)nx * ny * nz);
    *num_partials = g;
    // k_noise strides a 32-bit index by gridDim * kBlock (<= 4096 * kBlock): a
    // total within one stride of 2^32 would wrap it and loop forever
    if ((long long)nx * ny * nz > (1ll << 32) - 4096ll * kBlock) return hipErrorInvalidValue;
    // cellular: the cell range the grid's coordinates (start + i) * freq can
    // reach, +-1 neighbour and a cell of margin for rint (cellular_table)
    int lo = 0, n = 0;
    if (kind == 0) {
        double cmin = 0.0, cmax = 0.0;
        bool first = true;
        for (int ax = 0; ax < 3; ++ax) {
            const int o = ax == 0 ? x0 : ax == 1 ? y0 : z0, m = ax == 0 ? nx : ax == 1 ? ny : nz;
            for (const int e : {o, o + m - 1}) {
                const double c = (double)(float)((float)e * freq);
                cmin = first ? c : std::min(cmin, c);
                cmax = first ? c : std::max(cmax, c);
                first = false;
            }
        }
        if (std::isfinite(cmin) && std::isfinite(cmax) && cmax - cmin < 64.0) {
            lo = (int)std::floor(cmin) - 2;
            n = (int)std::ceil(cmax) + 2 - lo + 1;
            if (n > kNoiseTableMaxN) n = 0;
        }
    }
    const size_t lds = (size_t)n * n * n * sizeof(float4);
    hipLaunchKernelGGL(k_noise, dim3(g), dim3(kBlock), lds, s, kind, d_out, x0, y0, z0, nx, ny, nz, freq, seed, lo, n,
                       reinterpret_cast<float2*>(d_partials));
    return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void k_perlin_lattice(uint2* __restrict__ out, int seed, int lo, int n)
{
    const long long total = (long long)n * n * n;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int ix = (int)(i % n), iy = (int)((i / n) % n), iz = (int)(i / ((long long)n * n));
        out[i] = noise::perlin_lattice_entry(seed, lo + ix, lo + iy, lo + iz);
    }
}

hipError_t launch_perlin_lattice(uint2* d_out, int seed, int lo, int n, hipStream_t s)
{
    const long long total = (long long)n * n * n;
    const long long blocks = std::min<long long>((total + kBlock - 1) / kBlock, 8192);
    hipLaunchKernelGGL(k_perlin_lattice, dim3((unsigned)blocks), dim3(kBlock), 0, s, d_out, seed, lo, n);
    return hipGetLastError();
}

hipError_t launch_minmax_reduce(const float* d_partials, int num_partials, float* d_minmax, hipStream_t s)
{
    hipLaunchKernelGGL(k_minmax, dim3(1), dim3(kBlock), 0, s, reinterpret_cast<const float2*>(d_partials),
                       num_partials, d_minmax);
    return hipGetLastError();
}

hipError_t launch_pack_recipe(const float* d_g1, const float* d_g2, const float* d_g3, const float* d_g4,
                              const float* d_minmax, long long total, uint8_t* d_rgba, hipStream_t s)
{
    hipLaunchKernelGGL(k_pack_recipe, dim3(grid_for(total)), dim3(kBlock), 0, s, d_g1, d_g2, d_g3, d_g4,
                       d_minmax, total, reinterpret_cast<uchar4*>(d_rgba));
    return hipGetLastError();
}

// Streaming kernels for the measured HBM roofline (vr_measure_bandwidth):
// 16 B per lane, one pass over the buffer, the grid as large as the buffer
// (each workgroup owns PL x 256 x 16 B; a persistent 2,048-workgroup
// grid-stride loop read 4.6-4.7 TB/s).  PL independent loads per lane are
// issued before anything consumes them.
//  * copy: the float4 copy of MI355X_MICROARCH.md's measured HBM rate
//    (counted as 2 x bytes moved);
//  * read: loads only, folded into one register per lane (xor), which is
//    stored only if it equals a value the 0x5a fill never produces -- every
//    lane's loads stay live, nothing is written.  The ray march is 98 % reads
//    (profiles/traffic.json), so this is its roofline denominator.
template <int PL>
__global__ __launch_bounds__(256) void k_stream_copy(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                     long long n)
{
    const long long base = (long long)blockIdx.x * (256 * PL) + threadIdx.x;
    uint4 v[PL];
#pragma unroll
    for (int k = 0; k < PL; ++k)
        if (base + k * 256 < n) v[k] = src[base + k * 256];
#pragma unroll
    for (int k = 0; k < PL; ++k)
        if (base + k * 256 < n) dst[base + k * 256] = v[k];
}

constexpr unsigned kReadSinkMagic = 0x9e3779b9u;

template <int PL>
__global__ __launch_bounds__(256) void k_stream_read(const uint4* __restrict__ src, unsigned* __restrict__ sink,
                                                     long long n)
{
    const long long base = (long long)blockIdx.x * (256 * PL) + threadIdx.x;
    uint4 v[PL];
#pragma unroll
    for (int k = 0; k < PL; ++k) v[k] = base + k * 256 < n ? src[base + k * 256] : make_uint4(0u, 0u, 0u, 0u);
    unsigned x = 0u;
#pragma unroll
    for (int k = 0; k < PL; ++k) x ^= (v[k].x ^ v[k].y) ^ (v[k].z ^ v[k].w);
    if (x == kReadSinkMagic) sink[threadIdx.x] = x;   // never taken for the 0x5a fill
}

template <int PL>
static hipError_t launch_stream_pl(int kind, const void* src, void* dst, long long n, hipStream_t s)
{
    const long long blocks = (n + 256 * PL - 1) / (256 * PL);
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (kind == 0)
        hipLaunchKernelGGL(k_stream_copy<PL>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint4*>(src),
                           static_cast<uint4*>(dst), n);
    else
        hipLaunchKernelGGL(k_stream_read<PL>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint4*>(src),
                           static_cast<unsigned*>(dst), n);
    return hipGetLastError();
}

hipError_t launch_stream_bw(int kind, int loads_per_lane, const void* src, void* dst, size_t bytes, hipStream_t s)
{
    const long long n = (long long)(bytes / 16);
    switch (loads_per_lane) {
    case 4: return launch_stream_pl<4>(kind, src, dst, n, s);
    case 8: return launch_stream_pl<8>(kind, src, dst, n, s);
    case 16: return launch_stream_pl<16>(kind, src, dst, n, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_stream_copy(const void* src, void* dst, size_t bytes, hipStream_t s)
{
    return launch_stream_bw(0, 4, src, dst, bytes, s);
}

hipError_t launch_assemble(const uint8_t* d_gathered, size_t rows_per_rank, int nranks, int width, int height,
                           int band_rows, int bpp, int first_rank, uint8_t* d_frame, hipStream_t s, bool serp)
{
    const long long row_bytes = (long long)width * bpp;
    if (row_bytes % 16 == 0) {
        const int elems = (int)(row_bytes / 16);
        hipLaunchKernelGGL(k_assemble<uint4>, grid_rows(rows_per_rank, nranks, first_rank, elems), dim3(kBlock), 0, s,
                           reinterpret_cast<const uint4*>(d_gathered), (int)rows_per_rank, nranks, elems,
                           height, band_rows, first_rank, (int)serp, reinterpret_cast<uint4*>(d_frame));
    } else if (row_bytes % 4 == 0) {
        const int elems = (int)(row_bytes / 4);
        hipLaunchKernelGGL(k_assemble<unsigned int>, grid_rows(rows_per_rank, nranks, first_rank, elems), dim3(kBlock), 0,
                           s, reinterpret_cast<const unsigned int*>(d_gathered), (int)rows_per_rank, nranks,
                           elems, height, band_rows, first_rank, (int)serp, reinterpret_cast<unsigned int*>(d_frame));
    } else {   // 1-byte pixels, rows of any width
        const int elems = (int)row_bytes;
        hipLaunchKernelGGL(k_assemble<unsigned char>, grid_rows(rows_per_rank, nranks, first_rank, elems), dim3(kBlock), 0,
                           s, d_gathered, (int)rows_per_rank, nranks, elems, height, band_rows, first_rank, (int)serp,
                           d_frame);
    }
    return hipGetLastError();
}

hipError_t launch_assemble_grey(const uint8_t* d_gathered, size_t rows_per_rank, int nranks, int width, int height,
                                int band_rows, bool f32, int first_rank, uint8_t* d_frame, hipStream_t s, bool serp)
{
    const dim3 blk(kBlock);
    if (f32) {
        hipLaunchKernelGGL((k_assemble_grey<float, float4>), grid_rows(rows_per_rank, nranks, first_rank, width), blk, 0, s,
                           reinterpret_cast<const float*>(d_gathered), (int)rows_per_rank, nranks, width, height,
                           band_rows, first_rank, (int)serp, reinterpret_cast<float4*>(d_frame));
    } else if (width % 4 == 0) {
        const int elems = width / 4;
        hipLaunchKernelGGL((k_assemble_grey<unsigned int, uint4>), grid_rows(rows_per_rank, nranks, first_rank, elems), blk, 0,
                           s, reinterpret_cast<const unsigned int*>(d_gathered), (int)rows_per_rank, nranks,
                           elems, height, band_rows, first_rank, (int)serp, reinterpret_cast<uint4*>(d_frame));
    } else {
        hipLaunchKernelGGL((k_assemble_grey<unsigned char, unsigned int>), grid_rows(rows_per_rank, nranks, first_rank, width),
                           blk, 0, s, d_gathered, (int)rows_per_rank, nranks, width, height, band_rows, first_rank, (int)serp,
                           reinterpret_cast<unsigned int*>(d_frame));
    }
    return hipGetLastError();
}

// ---- self tests (vr_selftest) ----
namespace {
__global__ __launch_bounds__(256) void k_selftest_cell_inv(int variant, unsigned long long* __restrict__ bad)
{
    constexpr unsigned kMaxK = 3u * 1023u * 1023u;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    const unsigned K = 8u * i + 3u;
    unsigned miss = 0;
    if (K <= kMaxK) {
        const float d2 = (float)K * 0.25f;
        const float want = noise::cell_inv_ieee(d2);
        const float got = variant == 0 ? noise::cell_inv_a(d2) : variant == 1 ? noise::cell_inv_b(d2)
                        : variant == 2 ? noise::cell_inv_c(d2) : noise::cell_inv(d2);
        miss = __float_as_uint(got) != __float_as_uint(want);
    }
    unsigned long long c = miss;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(bad, c);
}
}  // namespace

// Worley pruning (noise::cellular_table9) against the unpruned cellular():
// bit-equal F1 on points drawn uniformly and at the edge cases of the bound
// -- coordinates a few ulps around half-integers (the rint switch) and
// integers (the floor switch), and points next to a feature point (F1 ~ 0)
// or between two (near ties).  The table is the march's, cells [0, 9)^3
// with z pitch 83; points keep rint +- 1 inside it.
constexpr int kWorleyTestBlocks = 2048, kWorleyTestPerThread = 16;
__global__ __launch_bounds__(256) void k_selftest_worley(int seed, unsigned long long* __restrict__ bad)
{
    __shared__ float4 tab[noise::kWorleyN * noise::kWorleyPz];
    for (int i = threadIdx.x; i < noise::kWorleyN * noise::kWorleyN * noise::kWorleyN; i += 256) {
        const int ix = i % noise::kWorleyN, iy = (i / noise::kWorleyN) % noise::kWorleyN, iz = i / (noise::kWorleyN * noise::kWorleyN);
        tab[iz * noise::kWorleyPz + iy * noise::kWorleyN + ix] = noise::cellular_cell(seed, ix, iy, iz);
    }
    __syncthreads();
    unsigned miss = 0;
    for (int j = 0; j < kWorleyTestPerThread; ++j) {
        const unsigned id = (blockIdx.x * 256u + threadIdx.x) * kWorleyTestPerThread + (unsigned)j;
        unsigned h = id * 0x9E3779B1u + 0x85EBCA77u;
        auto next = [&h]() { h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15; return h; };
        auto unit = [&]() { return (float)(next() >> 8) * (1.0f / 16777216.0f); };   // [0, 1)
        float c[3];
        const unsigned kind = id % 5u;
        for (int a = 0; a < 3; ++a) c[a] = 1.0f + 6.0f * unit();   // [1, 7)
        if (kind == 1 || kind == 2) {
            // a few ulps around k + 0.5 (rint) or k (floor) on a random subset of axes
            for (int a = 0; a < 3; ++a) {
                if (next() & 1u) continue;
                const float k = (float)(1 + (int)(next() % 6u)) + (kind == 1 ? 0.5f : 0.0f);
                const int ulps = (int)(next() % 7u) - 3;
                c[a] = __int_as_float(__float_as_int(k) + ulps);
            }
        } else if (kind == 3 || kind == 4) {
            // next to a feature point (3), or between two neighbouring ones (4)
            const int cx = 2 + (int)(next() % 5u), cy = 2 + (int)(next() % 5u), cz = 2 + (int)(next() % 5u);
            const float4 f = tab[cz * noise::kWorleyPz + cy * noise::kWorleyN + cx];
            float p[3] = {fmaf(f.x, f.w, (float)cx), fmaf(f.y, f.w, (float)cy), fmaf(f.z, f.w, (float)cz)};
            if (kind == 4) {
                const int a = (int)(next() % 3u);
                const int dx = a == 0, dy = a == 1, dz = a == 2;
                const float4 g = tab[(cz + dz) * noise::kWorleyPz + (cy + dy) * noise::kWorleyN + cx + dx];
                const float q[3] = {fmaf(g.x, g.w, (float)(cx + dx)), fmaf(g.y, g.w, (float)(cy + dy)), fmaf(g.z, g.w, (float)(cz + dz))};
                for (int b = 0; b < 3; ++b) p[b] = 0.5f * (p[b] + q[b]);
            }
            const float r = kind == 3 ? 1e-3f : 1e-5f;
            for (int b = 0; b < 3; ++b) c[b] = fminf(fmaxf(p[b] + r * (2.0f * unit() - 1.0f), 0.51f), 7.49f);
        }
        bool full;
        const float got = noise::cellular_table9(tab, noise::worley9_nc(0), c[0], c[1], c[2], full);
        const float want = noise::cellular(seed, c[0], c[1], c[2]);
        miss += __float_as_uint(got) != __float_as_uint(want);
    }
    unsigned long long cnt = miss;
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(bad, cnt);
}

hipError_t launch_selftest_worley(int seed, unsigned long long* d_bad, hipStream_t s)
{
    hipLaunchKernelGGL(k_selftest_worley, dim3(kWorleyTestBlocks), dim3(256), 0, s, seed, d_bad);
    return hipGetLastError();
}

hipError_t launch_selftest_cell_inv(int variant, unsigned long long* d_bad, hipStream_t s)
{
    constexpr unsigned kCount = (3u * 1023u * 1023u - 3u) / 8u + 1u;
    hipLaunchKernelGGL(k_selftest_cell_inv, dim3((kCount + 255) / 256), dim3(256), 0, s, variant, d_bad);
    return hipGetLastError();
}

}  // namespace vr
