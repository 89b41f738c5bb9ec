// vr_fill.hip -- the kernels and launchers of vr_fill, the flood-fill brush
// (include/vr.h): connected-component labelling of the
// passable texels of the brush's clipped box, then vr_paint's blend on the
// component that holds the seed.  Three launches; whatever one workgroup
// tells another that is not an atomic crosses a kernel boundary:
//   k_fill_label   a workgroup per 8 x 8 x 8 tile: the passable test and the
//                  tile-local components, a union-find over LDS atomics
//   k_fill_merge   the unions across the tiles' faces, in global memory with
//                  agent-scope atomic loads and atomic mins only
//   k_fill_commit  vr_paint's rows over the box: blend where the texel's root
//                  is the seed's, fold the new bytes into mm, add up the report
// The rule, the passable test, find / union and the tile labelling are
// vr_fill.h's, which the host statement (vr_brush.cpp) and the stand-alone
// check (tools/fill_check.cpp) include too.  No kernel waits for another
// workgroup, and every find / union loop is capped by the number of labels.
#include <cstddef>

#include "vr_brush.h"
#include "vr_fill.h"
#include "vr_internal.h"
#include "vr_volume_kernels.h"

namespace vr {
namespace {

// tile-local labels in LDS: other threads of the workgroup lower them during tile_link, so every access that
// phase makes is an atomic of workgroup scope
struct LdsLabels {
    uint32_t* l;
    __device__ __forceinline__ uint32_t load(uint32_t i) { return __hip_atomic_load(&l[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ void store(uint32_t i, uint32_t v) { l[i] = v; }
    __device__ __forceinline__ uint32_t fetch_min(uint32_t i, uint32_t v)
    {
        return __hip_atomic_fetch_min(&l[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

// the box's labels while other workgroups lower them (k_fill_merge): the XCDs' L2s are not coherent and a CU's L1
// is never refreshed by another CU's stores, so every access is an agent-scope atomic
struct AgentLabels {
    uint32_t* l;
    __device__ __forceinline__ uint32_t load(uint32_t i) { return __hip_atomic_load(&l[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t fetch_min(uint32_t i, uint32_t v)
    {
        return __hip_atomic_fetch_min(&l[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// the box's labels once nothing writes them (k_fill_commit)
struct ConstLabels {
    const uint32_t* __restrict__ l;
    __device__ __forceinline__ uint32_t load(uint32_t i) { return l[i]; }
};

__device__ __forceinline__ uint32_t box_index(const PaintArgs& p, int x, int y, int z)
{
    return ((uint32_t)z * (uint32_t)p.e[1] + (uint32_t)y) * (uint32_t)p.e[0] + (uint32_t)x;
}

// Launch 1.  Workgroup blockIdx.x takes tile (bt % ntx, bt / ntx % nty, bt / (ntx nty)) of the clipped box, x
// fastest; thread tid owns the tile's texels tid and tid + kBlock (the same x and y, z four apart): consecutive
// lanes on consecutive x of a row, eight rows per wave.  It reads the seed's selected bytes (the same address in
// every lane) and its texels' selected bytes from the planes, and writes every label of the tile that lies in the
// box -- kNone included, the scratch holds whatever the last call left.
__global__ __launch_bounds__(kBlock) void k_fill_label(FillArgs a, const uint8_t* __restrict__ src,
                                                       uint32_t* __restrict__ labels, vr_fill_report* __restrict__ rep)
{
    static_assert(fill::kTileTexels == 2 * kBlock, "two texels of the tile per thread");
    __shared__ uint32_t lds[fill::kTileTexels];
    LdsLabels lab{lds};
    const PaintArgs& p = a.p;
    const long long plane = (long long)p.nx * p.ny * p.nz;
    const int ntx = (p.e[0] + fill::kTile - 1) / fill::kTile, nty = (p.e[1] + fill::kTile - 1) / fill::kTile;
    const int bt = blockIdx.x;
    const int tx0 = (bt % ntx) * fill::kTile, ty0 = (bt / ntx % nty) * fill::kTile, tz0 = (bt / (ntx * nty)) * fill::kTile;

    unsigned seed[4] = {0u, 0u, 0u, 0u};
    const long long seed_at = ((long long)a.rule.seed[2] * p.ny + a.rule.seed[1]) * p.nx + a.rule.seed[0];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (a.rule.select[c]) seed[c] = src[seed_at + c * plane];

    const unsigned tid = threadIdx.x;
    bool in_box[2];
    uint32_t at[2];   // the box-linear index of the thread's texels
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned t = tid + k * kBlock;
        const int x = tx0 + (int)(t % fill::kTile), y = ty0 + (int)(t / fill::kTile % fill::kTile),
                  z = tz0 + (int)(t / (fill::kTile * fill::kTile));
        in_box[k] = x < p.e[0] && y < p.e[1] && z < p.e[2];
        at[k] = in_box[k] ? box_index(p, x, y, z) : 0u;
        bool inside = false;
        long long texel = 0;
        if (in_box[k]) {
            const unsigned long long q = brush::axis_term(p.d0[0] + x, p.k[0]) + brush::axis_term(p.d0[1] + y, p.k[1]) +
                                         brush::axis_term(p.d0[2] + z, p.k[2]);
            inside = q <= p.s;
            texel = ((long long)(p.o[2] + z) * p.ny + (p.o[1] + y)) * p.nx + (p.o[0] + x);
        }
        fill::tile_init(lab, t, fill::passable(a.rule, seed, inside, [&](int c) -> unsigned { return src[texel + c * plane]; }));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) fill::tile_link(lab, tid + k * kBlock);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!in_box[k]) continue;
        const uint32_t r = fill::tile_root(lab, tid + k * kBlock);
        uint32_t out = fill::kNone;
        if (r != fill::kNone)   // the root is a passable texel of the tile: inside the box
            out = box_index(p, tx0 + (int)(r % fill::kTile), ty0 + (int)(r / fill::kTile % fill::kTile),
                            tz0 + (int)(r / (fill::kTile * fill::kTile)));
        labels[at[k]] = out;
    }
    if (rep && blockIdx.x == 0 && tid == 0) fill::empty_report(rep, p.nx, p.ny, p.nz);
}

// the empty report alone: a brush that misses the volume, a seed outside the clipped box
__global__ void k_fill_empty_report(int nx, int ny, int nz, vr_fill_report* __restrict__ rep)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) fill::empty_report(rep, nx, ny, nz);
}

// Launch 2.  A thread per texel of the box (grid-stride); the ones on a tile's low x, y or z face whose neighbour
// across the face is passable too unite the two labels (vr_fill.h merge_texel) -- a texel off every low face
// loads nothing.
__global__ __launch_bounds__(kBlock) void k_fill_merge(FillArgs a, uint32_t* labels)
{
    AgentLabels lab{labels};
    const PaintArgs& p = a.p;
    const unsigned ex = (unsigned)p.e[0], ey = (unsigned)p.e[1];
    const unsigned long long total = (unsigned long long)ex * ey * (unsigned)p.e[2];
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < total;
         i += (unsigned long long)gridDim.x * kBlock) {
        const unsigned row = (unsigned)(i / ex);
        const int x = (int)(i - (unsigned long long)row * ex), z = (int)(row / ey), y = (int)(row - (unsigned)z * ey);
        fill::merge_texel(lab, p.e, x, y, z);
    }
}

// Launch 3.  k_paint_planar's rows: a wave per box row (y, z), consecutive lanes on consecutive x.  The labels
// are read-only here, so plain loads do.  A texel inside the ellipsoid whose label is not kNone is passable; where
// its root is the seed's it is blended as vr_paint blends it and its new bytes go into lo / hi for mm.  The
// report: the wave counts its passable and its filled texels with a ballot per 64 texels and adds each sum with
// one 64-bit atomic at the end; the bounds by atomic min / max, once per wave.
__global__ __launch_bounds__(kBlock) void k_fill_commit(FillArgs a, const uint32_t* __restrict__ labels,
                                                        uint8_t* __restrict__ dst, unsigned* __restrict__ mm,
                                                        vr_fill_report* rep)
{
    constexpr unsigned kWaves = kBlock / 64;
    ConstLabels lab{labels};
    const PaintArgs& p = a.p;
    const long long plane = (long long)p.nx * p.ny * p.nz;
    const uint32_t cap = (uint32_t)p.e[0] * (uint32_t)p.e[1] * (uint32_t)p.e[2];
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // the seed lies in the box (the host checked); a seed that is not passable has no root and nothing equals kNone
    const uint32_t seed_at = box_index(p, a.rule.seed[0] - p.o[0], a.rule.seed[1] - p.o[1], a.rule.seed[2] - p.o[2]);
    const uint32_t seed_root = lab.load(seed_at) == fill::kNone ? fill::kNone : fill::find(lab, seed_at, cap);

    unsigned lo[4] = {255u, 255u, 255u, 255u}, hi[4] = {0u, 0u, 0u, 0u};
    unsigned long long n_pass = 0ull, n_fill = 0ull;   // the wave's, the same in every lane
    int bmin[3] = {p.nx, p.ny, p.nz}, bmax[3] = {-1, -1, -1};
    const unsigned rows = (unsigned)p.e[1] * (unsigned)p.e[2];
    for (unsigned r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
        const int z = (int)(r / (unsigned)p.e[1]), y = (int)(r - (unsigned)z * (unsigned)p.e[1]);
        const unsigned long long qyz = brush::axis_term(p.d0[1] + y, p.k[1]) + brush::axis_term(p.d0[2] + z, p.k[2]);
        if (qyz > p.s) continue;
        uint8_t* __restrict__ row = dst + ((long long)(p.o[2] + z) * p.ny + (p.o[1] + y)) * p.nx + p.o[0];
        const uint32_t row_at = r * (uint32_t)p.e[0];
        for (int x0 = 0; x0 < p.e[0]; x0 += 64) {   // wave-uniform: the ballots see every lane
            const int x = x0 + lane;
            unsigned long long q = 0ull;
            bool inside = x < p.e[0];
            if (inside) {
                q = qyz + brush::axis_term(p.d0[0] + x, p.k[0]);
                inside = q <= p.s;
            }
            const bool pass = inside && lab.load(row_at + (uint32_t)x) != fill::kNone;
            const bool filled = pass && fill::find(lab, row_at + (uint32_t)x, cap) == seed_root;
            if (rep) {
                n_pass += (unsigned long long)__popcll(__ballot(pass));
                n_fill += (unsigned long long)__popcll(__ballot(filled));
            }
            if (!filled) continue;
            bmin[0] = min(bmin[0], p.o[0] + x); bmax[0] = max(bmax[0], p.o[0] + x);
            bmin[1] = min(bmin[1], p.o[1] + y); bmax[1] = max(bmax[1], p.o[1] + y);
            bmin[2] = min(bmin[2], p.o[2] + z); bmax[2] = max(bmax[2], p.o[2] + z);
            const unsigned w = brush::weight(q, p.s, p.falloff);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (p.strength[c] == 0u) continue;
                uint8_t* ptr = row + x + c * plane;
                const unsigned old = *ptr;
                const unsigned nw = brush::blend(p.op, old, p.value[c], w * p.strength[c]);
                if (nw != old) *ptr = (uint8_t)nw;
                lo[c] = min(lo[c], nw);
                hi[c] = max(hi[c], nw);
            }
        }
    }
    if (rep) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (int off = 32; off > 0; off >>= 1) {
                bmin[k] = min(bmin[k], __shfl_xor(bmin[k], off));
                bmax[k] = max(bmax[k], __shfl_xor(bmax[k], off));
            }
        if (lane == 0) {
            if (n_pass != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(&rep->passable), n_pass);
            if (n_fill != 0ull) {
                atomicAdd(reinterpret_cast<unsigned long long*>(&rep->filled), n_fill);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    atomicMin(&rep->min[k], bmin[k]);
                    atomicMax(&rep->max[k], bmax[k]);
                }
            }
        }
    }
    fold_minmax(lo, hi, mm);
}

bool fill_args_ok(const FillArgs& a)
{
    const PaintArgs& p = a.p;
    if (p.e[0] < 1 || p.e[1] < 1 || p.e[2] < 1 || p.e[0] > 511 || p.e[1] > 511 || p.e[2] > 511) return false;
    for (int ax = 0; ax < 3; ++ax) {
        const int n = ax == 0 ? p.nx : ax == 1 ? p.ny : p.nz;
        if (p.o[ax] < 0 || p.e[ax] > n - p.o[ax]) return false;                                      // the box in the volume
        if (a.rule.seed[ax] < p.o[ax] || a.rule.seed[ax] >= p.o[ax] + p.e[ax]) return false;      // the seed in the box
    }
    return true;
}

}  // namespace

size_t fill_label_bytes(const PaintArgs& p)
{
    return sizeof(uint32_t) * (size_t)p.e[0] * (size_t)p.e[1] * (size_t)p.e[2];
}

hipError_t launch_fill_empty_report(int nx, int ny, int nz, vr_fill_report* d_report, hipStream_t s)
{
    if (!d_report) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fill_empty_report, dim3(1), dim3(64), 0, s, nx, ny, nz, d_report);
    return hipGetLastError();
}

// a workgroup per tile of the clipped box: at most 64^3 of them (a box edge is at most 511 texels)
hipError_t launch_fill_label(const FillArgs& a, const uint8_t* d_planar, uint32_t* d_labels, vr_fill_report* d_report,
                             hipStream_t s)
{
    if (!fill_args_ok(a) || !d_labels) return hipErrorInvalidValue;
    const long long tiles = (long long)((a.p.e[0] + fill::kTile - 1) / fill::kTile) * ((a.p.e[1] + fill::kTile - 1) / fill::kTile) *
                            ((a.p.e[2] + fill::kTile - 1) / fill::kTile);
    hipLaunchKernelGGL(k_fill_label, dim3((unsigned)tiles), dim3(kBlock), 0, s, a, d_planar, d_labels, d_report);
    return hipGetLastError();
}

// a thread per texel of the box, grid-stride past 4096 workgroups
hipError_t launch_fill_merge(const FillArgs& a, uint32_t* d_labels, hipStream_t s)
{
    if (!fill_args_ok(a) || !d_labels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fill_merge, dim3(grid_for((long long)a.p.e[0] * a.p.e[1] * a.p.e[2])), dim3(kBlock), 0, s, a, d_labels);
    return hipGetLastError();
}

// a wave per box row, as launch_paint_planar
hipError_t launch_fill_commit(const FillArgs& a, const uint32_t* d_labels, uint8_t* d_planar, unsigned* mm,
                              vr_fill_report* d_report, hipStream_t s)
{
    if (!fill_args_ok(a) || !d_labels) return hipErrorInvalidValue;
    const long long rows = (long long)a.p.e[1] * a.p.e[2];
    hipLaunchKernelGGL(k_fill_commit, dim3(grid_for(rows * 64)), dim3(kBlock), 0, s, a, d_labels, d_planar, mm, d_report);
    return hipGetLastError();
}

}  // namespace vr
