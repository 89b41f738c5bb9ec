// vr_volume_kernels.h -- what the volume kernels (vr_volume.hip) and the brush
// kernels (vr_paint.hip) share: the workgroup size, the clamp, the fold of a
// workgroup's byte min / max into mm, and the grid of a streaming launch.
// Device code is per translation unit (no -fgpu-rdc): each includes its copy.
#pragma once

namespace vr {
namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

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

inline int grid_for(long long n)
{
    long long g = (n + kBlock - 1) / kBlock;
    if (g > 256 * 16) g = 256 * 16;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace
}  // namespace vr
