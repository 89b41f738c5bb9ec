// vr_proc_kernels.h -- device code of the procedural medium: the fBm x Worley
// density, the per-pixel march with its shadow rays, the cost sort, the
// deferred shadow passes and the kernels, with with_proc_variant for the tile
// kernels' launchers.  Included by the two translation units that launch
// these kernels, vr_march.hip and vr_march_rect.hip; the grid march is
// vr_march_kernels.h, and what both share is vr_march_common.h.  Everything is
// in an anonymous namespace, so each translation unit keeps its own copy.
#pragma once
#include "vr_march_common.h"
#include "vr_noise.h"

namespace vr {
namespace {

// Procedural medium (BASELINE configs 2/3, build-defined; spec in
// oracle/vr_oracle.h vro_procedural): fBm Perlin x (1 - Worley F1).
// TABLE: 0 = direct noise, 1 = LDS tables with runtime Worley geometry,
// 2 = LDS tables with the fixed 9-cell geometry (noise::cellular_table9),
// 3 = 2 + the global Perlin lattice table (noise::perlin_lat)
// `cells` accumulates the Worley cells this evaluation computed (8, or 35 when
// the pruned lane also ran the 27-cell block; 27 without the pruned table) --
// vr option "count" = 2, the algorithmic work of the roofline (bench.py)
// WC: the Worley cube comes from the lane's register cache *wc
// (noise::cellular_table9_cached; the deferred shadow pass)
// The loop-invariant operands of proc_density, pinned to VGPRs ONCE, before
// a kernel's step / sample loops: a VALU op reading an SGPR issues at half
// rate, and an in_vgpr() inside the density is re-done
// (v_mov from the SGPR) at every evaluation -- the round-4 shadow pass spent
// 7 of its ~44 per-sample instructions outside the octaves on those copies.
struct DensityK {
    float gs, lac, gain, f0, wf, scale;
    float lat_sy, lat_sz, lat_nc;   // TABLE 3: the lattice table's byte-offset fma constants (lat_nc = -lat_c)
    float wt_nc;                    // TABLE >= 2: noise::worley9_nc(wt_lo)
};
template <int TABLE>
__device__ __forceinline__ DensityK density_k(const ProcParams& p, float scale)
{
    DensityK k;
    k.gs = noise::in_vgpr(p.grid_scale);
    k.lac = noise::in_vgpr(p.lacunarity);
    k.gain = noise::in_vgpr(p.gain);
    k.f0 = noise::in_vgpr(p.freq0);
    k.wf = noise::in_vgpr(p.worley_freq);
    k.scale = noise::in_vgpr(scale);
    if constexpr (TABLE == 3) {
        k.lat_sy = noise::in_vgpr(p.lat_sy);
        k.lat_sz = noise::in_vgpr(p.lat_sz);
        k.lat_nc = noise::in_vgpr(-p.lat_c);
    } else {
        k.lat_sy = k.lat_sz = k.lat_nc = 0.0f;
    }
    // the negated constant terms make the offset fmas v_fmamk (literal 8 / 16)
    k.wt_nc = TABLE >= 2 ? noise::in_vgpr(noise::worley9_nc(p.wt_lo)) : 0.0f;
    return k;
}

// Byte offset of the lattice word of cell (xs, ys, zs) (TABLE 3): exact small
// integers in fp32, one conversion.
__device__ __forceinline__ unsigned lat_offset(const DensityK& k, float xs, float ys, float zs)
{
    return (unsigned)fmaf(zs, k.lat_sz, fmaf(ys, k.lat_sy, fmaf(xs, 8.0f, k.lat_nc)));
}

// The recipe's octave count (vr_procedural_defaults), for which the fBm is
// also built fully unrolled: no loop-carried register copies, no loop control.
// In the primary marches: config 2 -4 % at 4 waves per SIMD
// (profiles/r05/ab_proc_diet_*.txt).
constexpr int kFbmUnroll = 4;

// fBm over the lattice table (TABLE 3).  The same operations in the same
// order either way:
// OCT = 0: p.octaves octaves, a loop; each octave loads its own lattice word.
// Loading the next octave's word during this one (a loop-carried prefetch) ran
// config 3 0.7 % slower (profiles/r05/ab_nopf.txt; arm removed).
// OCT > 0: exactly OCT octaves, fully unrolled, the lattice word of octave
// o + 1 loaded while octave o computes.  A scheduling barrier after each
// octave, to keep later octaves' loads out of earlier ones, was a round-5
// build knob that stayed off.
template <int OCT>
__device__ __forceinline__ float fbm_lat(const ProcParams& p, const DensityK& k, const float4* gp, float qx, float qy,
                                         float qz)
{
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.lat, (short)0, (int)p.lat_bytes, 0x00020000);
    float f = k.f0, amp = 1.0f, fbm = 0.0f;
    if constexpr (OCT == 0) {
#pragma unroll 1
        for (int o = 0; o < p.octaves; ++o) {
            const float x = qx * f, y = qy * f, z = qz * f;
            const float xs = floorf(x), ys = floorf(y), zs = floorf(z);
            const auto w = __builtin_amdgcn_raw_buffer_load_b64(rsrc, lat_offset(k, xs, ys, zs), 0, 0);
            const float pn = noise::perlin_lat(gp, make_uint2(w[0], w[1]), x, y, z, xs, ys, zs);
            fbm = fmaf(amp, pn, fbm);
            f = f * k.lac;
            amp = amp * k.gain;
        }
    } else {
        float x = qx * f, y = qy * f, z = qz * f;
        float xs = floorf(x), ys = floorf(y), zs = floorf(z);
        auto word = __builtin_amdgcn_raw_buffer_load_b64(rsrc, lat_offset(k, xs, ys, zs), 0, 0);
#pragma unroll
        for (int o = 0; o < OCT; ++o) {
            const uint2 w = make_uint2(word[0], word[1]);
            const float cx = x, cy = y, cz = z, cxs = xs, cys = ys, czs = zs;
            f = f * k.lac;
            if (o + 1 < OCT) {
                x = qx * f; y = qy * f; z = qz * f;
                xs = floorf(x); ys = floorf(y); zs = floorf(z);
                word = __builtin_amdgcn_raw_buffer_load_b64(rsrc, lat_offset(k, xs, ys, zs), 0, 0);
            }
            const float pn = noise::perlin_lat(gp, w, cx, cy, cz, cxs, cys, czs);
            fbm = fmaf(amp, pn, fbm);
            amp = amp * k.gain;
        }
    }
    return fbm;
}

// The recipe's density (TABLE 3, OCT octaves unrolled) in three phases: the
// lattice words of every octave are loaded first, the Worley cube is computed
// while they are in flight (its LDS reads and ~100 VALU ops hide the global
// load latency that fbm_lat<OCT> waits out at its first octave), then the
// octaves.  The same operations on the same values as proc_density: the fBm
// and F1 are independent until the final combine.  Two scheduling barriers
// keep the phases apart.  Config 2 -2.8 %, config 3 -1.7 %
// (profiles/r05/ab_phases.txt).
template <int OCT>
__device__ __forceinline__ float proc_density_phased(const ProcParams& p, const DensityK& k, const float4* wt,
                                                     float px, float py, float pz, unsigned& cells)
{
    const float qx = px * k.gs, qy = py * k.gs, qz = pz * k.gs;
    const float4* gp = wt + noise::kWorleyN * noise::kWorleyPz;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.lat, (short)0, (int)p.lat_bytes, 0x00020000);
    float X[OCT], Y[OCT], Z[OCT], XS[OCT], YS[OCT], ZS[OCT];
    uint2 W[OCT];
    float f = k.f0;
#pragma unroll
    for (int o = 0; o < OCT; ++o) {
        if (o > 0) f = f * k.lac;
        X[o] = qx * f; Y[o] = qy * f; Z[o] = qz * f;
        XS[o] = floorf(X[o]); YS[o] = floorf(Y[o]); ZS[o] = floorf(Z[o]);
        const auto w = __builtin_amdgcn_raw_buffer_load_b64(rsrc, lat_offset(k, XS[o], YS[o], ZS[o]), 0, 0);
        W[o] = make_uint2(w[0], w[1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    const float wf = k.wf;
    bool full;
    const float f1 = noise::cellular_table9(wt, k.wt_nc, qx * wf, qy * wf, qz * wf, full) + 1.0f;
    if (p.count_evals == 2) cells += full ? 35u : 8u;
    __builtin_amdgcn_sched_barrier(0);
    float amp = 1.0f, fbm = 0.0f;
#pragma unroll
    for (int o = 0; o < OCT; ++o) {
        const float pn = noise::perlin_lat(gp, W[o], X[o], Y[o], Z[o], XS[o], YS[o], ZS[o]);
        fbm = fmaf(amp, pn, fbm);
        amp = amp * k.gain;
    }
    return fmaxf(fbm * (1.0f - f1), 0.0f) * k.scale;
}

// UNROLL (TABLE 3): a density of the recipe's kFbmUnroll octaves takes the
// unrolled forms -- proc_density_phased, or fbm_lat<kFbmUnroll> when the Worley
// cube is cached (WC) -- and any other octave count the loop.
template <int TABLE, bool WC = false, bool UNROLL = false>
__device__ __forceinline__ float proc_density(const ProcParams& p, const DensityK& k, const float4* wt, float px,
                                              float py, float pz, unsigned& cells, noise::WorleyCube* wc = nullptr)
{
    if constexpr (TABLE == 3 && UNROLL && !WC)
        if (p.octaves == kFbmUnroll) return proc_density_phased<kFbmUnroll>(p, k, wt, px, py, pz, cells);
    const float qx = px * k.gs, qy = py * k.gs, qz = pz * k.gs;
    float fbm = 0.0f;
    if constexpr (TABLE == 3) {
        const float4* gp = wt + noise::kWorleyN * noise::kWorleyPz;
        if constexpr (UNROLL)
            fbm = p.octaves == kFbmUnroll ? fbm_lat<kFbmUnroll>(p, k, gp, qx, qy, qz) : fbm_lat<0>(p, k, gp, qx, qy, qz);
        else
            fbm = fbm_lat<0>(p, k, gp, qx, qy, qz);
    } else {
        float f = k.f0, amp = 1.0f;
        for (int o = 0; o < p.octaves; ++o) {
            float pn;
            if constexpr (TABLE == 2) pn = noise::perlin_gp(wt + noise::kWorleyN * noise::kWorleyPz, p.seed_fbm, qx * f, qy * f, qz * f);
            else if constexpr (TABLE == 1) pn = noise::perlin_gp(wt + p.wt_n * p.wt_pz, p.seed_fbm, qx * f, qy * f, qz * f);
            else pn = noise::perlin(p.seed_fbm, qx * f, qy * f, qz * f);
            fbm = fmaf(amp, pn, fbm);
            f = f * k.lac;
            amp = amp * k.gain;
        }
    }
    const float wf = k.wf;
    float f1;
    if constexpr (TABLE >= 2) {
        bool full;
        if constexpr (WC) f1 = noise::cellular_table9_cached(wt, k.wt_nc, qx * wf, qy * wf, qz * wf, full, *wc) + 1.0f;
        else f1 = noise::cellular_table9(wt, k.wt_nc, qx * wf, qy * wf, qz * wf, full) + 1.0f;
        if (p.count_evals == 2) cells += full ? 35u : 8u;
    } else {
        if constexpr (TABLE == 1) f1 = noise::cellular_table(wt, p.wt_lo, p.wt_n, p.wt_pz, qx * wf, qy * wf, qz * wf) + 1.0f;
        else f1 = noise::cellular(p.seed_worley, qx * wf, qy * wf, qz * wf) + 1.0f;
        if (p.count_evals == 2) cells += 27u;
    }
    return fmaxf(fbm * (1.0f - f1), 0.0f) * k.scale;
}

// Pixel value of the procedural march: single scatter, or frag.glsl:76-80.
template <bool SHADOW>
__device__ __forceinline__ float proc_epilogue(const MarchArgs& a, float acc, float rad)
{
    if constexpr (SHADOW) {
        return rad;
    } else {
        return ray_grey(a, acc);
    }
}

template <bool SHADOW, bool EARLY, int TABLE>
__device__ __forceinline__ unsigned march_pixel_proc(const MarchArgs& a, const float4* wt, int x, int orow)
{
    const Ray r = setup_ray(a, x, orow);
    const ProcParams& p = a.proc;
    float P0 = r.pxy.x, P1 = r.pxy.y, P2 = r.pz;
    float acc = 0.0f, rad = 0.0f, tv = 1.0f;
    int i = 0;
    unsigned evals = 0;   // shadow density evaluations
    unsigned cells = 0;   // Worley cells computed (count mode 2)
    const DensityK dk = density_k<TABLE>(p, a.scale);
    for (; i < r.n; ++i) {
        const float rho = proc_density<TABLE, false, true>(p, dk, wt, P0, P1, P2, cells);
        if constexpr (SHADOW) {
            if (rho > 0.0f) {
                float q0 = P0, q1 = P1, q2 = P2, sl = 0.0f;
                for (int j = 0; j < p.shadow_steps; ++j) {
                    q0 = q0 + p.lstep[0]; q1 = q1 + p.lstep[1]; q2 = q2 + p.lstep[2];
                    if (q0 >= 0.0f && q0 <= 1.0f && q1 >= 0.0f && q1 <= 1.0f && q2 >= 0.0f && q2 <= 1.0f) {
                        sl = sl + proc_density<TABLE>(p, dk, wt, q0, q1, q2, cells);
                        ++evals;
                    }
                }
                const float tl = spec_expf(-(sl * p.od));
                rad = fmaf((tv * (rho * p.od)), tl, rad);
            }
        }
        acc = acc + rho;
        if constexpr (SHADOW) tv = spec_expf(-(acc * p.od));
        P0 = P0 + r.sxy.x; P1 = P1 + r.sxy.y; P2 = P2 + r.sz;
        if constexpr (EARLY) {
            if (acc > a.acc_limit) { ++i; break; }
        }
    }
    if (r.live) store_pixel(a, x, orow, r.n >= 0, proc_epilogue<SHADOW>(a, acc, rad));
    if (r.n <= 0) return 0u;
    if (p.count_evals == 2) return cells;
    return p.count_evals ? (unsigned)i + evals : (unsigned)i;
}

// Shadow-ray compaction (config 3).  In march_pixel_proc a wave runs all
// shadow_steps density evaluations whenever ANY lane has rho > 0, so most
// lanes idle.  Here a wave instead deals the (lane, shadow step) pairs of the
// lanes that need them over all 64 lanes: cnt lanes need cnt * S evaluations,
// done in ceil(cnt * S / 64) rounds.  The results go through LDS and each lane
// then sums its own S values in step order, so the arithmetic (and the
// repeated-addition shadow positions) is exactly march_pixel_proc's.
// Requires wave-uniform control flow: every lane of the wave calls it.
// The pairs are dealt owner-major (a lane's run of steps is contiguous).  A
// step-major deal -- all owners' step 0, then step 1, ..., so that a round's
// neighbouring lanes evaluate neighbouring rays at one shadow step and share
// lattice cells -- cut the bank conflicts from 2.6 to 2.2 cycles per LDS
// instruction (1.4 together with the 64x64-region enumeration, option
// "proc_enum") and the VALU count by 2-6 %, yet ran 2-5 % slower
// (profiles/r03/ab_config3_deal_enum.txt, pmc_config3_deal_enum.txt): the
// conflicts are not on config 3's critical path.  Removed after measuring.
constexpr int kMaxCompactShadow = 8;
// Distance from the box faces beyond which the shadow-run fast path needs no
// per-sample test: 8 sequential adds drift < 8 * 6e-8 from the exact segment.
constexpr float kShadowInMargin = 1.0e-6f;
// Dealt pair pid lives at slot pid + pid / 32: an owner lane writes (and later
// reads) its run at off_k + c, and the offsets of neighbouring lanes step by
// their run lengths (~8), which without the pad puts 32 lanes on 4 LDS banks.
__device__ __forceinline__ int shadow_slot(int pid) { return pid + (pid >> 5); }
constexpr int kShadowSlots = 64 * kMaxCompactShadow + 64 * kMaxCompactShadow / 32;
struct ShadowLds {
    float4 p[64];                        // primary positions of the lanes that need shadow rays, [lane]
                                         // (one 16-B LDS access each way)
    union {
        unsigned code[kShadowSlots];   // dealt (lane << 3 | step) pairs, inside the box only
        float d[kShadowSlots];         // then their densities, same slot
    };
};

template <bool EARLY, int TABLE>
__device__ __forceinline__ unsigned march_pixel_proc_compact(const MarchArgs& a, const float4* wt, int x, int orow,
                                                             bool valid,
                                                             ShadowLds* sh, unsigned* shadow_evals)
{
    Ray r{};
    r.n = -1;
    if (valid) r = setup_ray(a, x, orow);
    const ProcParams& p = a.proc;
    const int S = p.shadow_steps;
    const int lane = threadIdx.x & 63;
    // the sun step in VGPRs: an add reading an SGPR issues at half rate
    const float l0 = noise::in_vgpr(p.lstep[0]), l1 = noise::in_vgpr(p.lstep[1]), l2 = noise::in_vgpr(p.lstep[2]);
    float P0 = r.pxy.x, P1 = r.pxy.y, P2 = r.pz;
    float acc = 0.0f, rad = 0.0f, tv = 1.0f;
    int i = 0;
    bool act = r.n > 0;
    unsigned evals = 0;
    unsigned cells = 0;   // Worley cells this lane computed (count mode 2), primary and dealt
    const DensityK dk = density_k<TABLE>(p, a.scale);
    for (;;) {
        act = act && i < r.n;
        if (__ballot(act) == 0) break;
        float rho = 0.0f;
        if (act) rho = proc_density<TABLE, false, true>(p, dk, wt, P0, P1, P2, cells);
        const bool need = act && rho > 0.0f;
        const unsigned long long m = __ballot(need);
        if (m) {
            // The samples q_j = P + (j+1) lstep (sequential adds) that fall inside the box form
            // one run j in [lo, lo+cnt): each coordinate moves monotonically, so its inside set
            // along j is an interval, and so is their intersection.  Only those are dealt, so
            // no lane of a round idles on an outside sample (they contribute exactly +0).
            int lo = 0, cnt = 0;
            // Fast path: the shadow samples lie on the segment from P + L to
            // P + S L (convex), and the sequential adds drift from it by at most
            // S half-ulps (< 6e-8 each below 2).  When both ends are inside the
            // box by kShadowInMargin, every sample is: the run is j = 0..S-1.
            bool slow = false;
            if (need) {
                const float fs = (float)S;
                const float a0 = fmaf(fs, l0, P0), a1 = fmaf(fs, l1, P1), a2 = fmaf(fs, l2, P2);
                const float b0 = P0 + l0, b1 = P1 + l1, b2 = P2 + l2;
                const float lo3 = fminf(fminf(fminf(a0, a1), a2), fminf(fminf(b0, b1), b2));
                const float hi3 = fmaxf(fmaxf(fmaxf(a0, a1), a2), fmaxf(fmaxf(b0, b1), b2));
                slow = !(lo3 >= kShadowInMargin && hi3 <= 1.0f - kShadowInMargin);
                cnt = slow ? 0 : S;
                sh->p[lane] = make_float4(P0, P1, P2, 0.0f);
            }
            if (__ballot(slow)) {
                if (slow) {
                    float q0 = P0, q1 = P1, q2 = P2;
                    for (int j = 0; j < S; ++j) {
                        q0 = q0 + l0; q1 = q1 + l1; q2 = q2 + l2;
                        // the box test as min3 / max3 (q is never NaN): 4 ops, not 6 compares
                        const bool in = fminf(fminf(q0, q1), q2) >= 0.0f && fmaxf(fmaxf(q0, q1), q2) <= 1.0f;
                        if (in && cnt == 0) lo = j;
                        cnt += in ? 1 : 0;
                    }
                }
            }
            // Exclusive prefix of cnt (0..8, four bits) over the wave, by bit-plane ballots.
            int off = 0, total = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned long long bb = __ballot((cnt >> b) & 1);
                off += __popcll(bb & ((1ull << lane) - 1ull)) << b;
                total += __popcll(bb) << b;
            }
            for (int c = 0; c < cnt; ++c) sh->code[shadow_slot(off + c)] = ((unsigned)lane << 3) | (unsigned)(lo + c);
            __builtin_amdgcn_wave_barrier();
            for (int base = 0; base < total; base += 64) {
                const int pid = base + lane;
                if (pid < total) {
                    const unsigned code = sh->code[shadow_slot(pid)];
                    const int kk = (int)(code >> 3), j = (int)(code & 7u);
                    const float4 pk = sh->p[kk];
                    float q0 = pk.x, q1 = pk.y, q2 = pk.z;
                    for (int jj = 0; jj <= j; ++jj) { q0 = q0 + l0; q1 = q1 + l1; q2 = q2 + l2; }
                    sh->d[shadow_slot(pid)] = proc_density<TABLE>(p, dk, wt, q0, q1, q2, cells);
                    ++evals;
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (need) {
                float sl = 0.0f;
                for (int c = 0; c < cnt; ++c) sl = sl + sh->d[shadow_slot(off + c)];
                const float tl = spec_expf(-(sl * p.od));
                rad = fmaf((tv * (rho * p.od)), tl, rad);
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (act) {
            acc = acc + rho;
            tv = spec_expf(-(acc * p.od));
            P0 = P0 + r.sxy.x; P1 = P1 + r.sxy.y; P2 = P2 + r.sz;
            ++i;
            if constexpr (EARLY) {
                if (acc > a.acc_limit) act = false;
            }
        }
    }
    if (r.live) store_pixel(a, x, orow, r.n >= 0, rad);
    if (p.count_evals == 2) {   // every lane's cells, also those a lane computed for another's shadow ray
        *shadow_evals = 0;
        return cells;
    }
    *shadow_evals = evals;
    return r.n > 0 ? (unsigned)i : 0u;
}

// Procedural medium: one 8x8 tile per wave (compute-bound; no volume), in
// row order (cx < 0) or in rings around tile (cx, cy) (ring_tile).
// Noise tables for the workgroup (dynamic LDS): the Worley cell table
// (wt_n^3 float4) followed by the 256 Perlin gradient pairs (2 float4 each),
// built before any wave may leave.  Returns null when the tables are off
// (wt_n = 0).
template <int TABLE>
__device__ __forceinline__ const float4* worley_table(const ProcParams& p, float4* lds)
{
    // TABLE > 0 only when the host sized the tables (wt_n > 0): the returned
    // pointer is the LDS symbol itself, so table reads fold its address
    if constexpr (TABLE == 0) return nullptr;
    const int n = p.wt_n, cells = n * p.wt_pz;   // z pitch wt_pz >= n * n
    for (int i = threadIdx.x; i < n * n * n; i += kThreads) {
        const int ix = i % n, iy = (i / n) % n, iz = i / (n * n);
        lds[iz * p.wt_pz + iy * n + ix] = noise::cellular_cell(p.seed_worley, p.wt_lo + ix, p.wt_lo + iy, p.wt_lo + iz);
    }
    noise::grad_pair_entry(threadIdx.x, lds + cells);   // 256 pairs, one per thread
    __syncthreads();
    return lds;
}

template <bool SHADOW, bool EARLY, int TABLE>
__global__ __launch_bounds__(kThreads) void march_proc(const MarchArgs a, int cx, int cy)
{
    extern __shared__ float4 wt_lds[];
    const float4* wt = worley_table<TABLE>(a.proc, wt_lds);
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int tiles_x8 = (a.width + 7) >> 3, rows8 = (a.out_rows + 7) >> 3;
    unsigned long long steps = 0;
    int tx, ty;
    if (cx >= 0) {
        ring_tile(t, cx, cy, &tx, &ty);
    } else {
        ty = t / tiles_x8;
        tx = t - ty * tiles_x8;
    }
    if (tx >= 0 && tx < tiles_x8 && ty >= 0 && ty < rows8) {
        steps = march_pixel_proc<SHADOW, EARLY, TABLE>(a, wt, tx * 8 + lane_x(lane), ty * 8 + lane_y(lane));
    }
    if (a.step_counter) add_steps(a, steps);
}

// ---- procedural, cost-sorted schedule ----
// A ray's cost is its step count n (a3), known after the ray setup.  Pass 1
// writes every pixel with n <= 0 and builds a histogram of n; pass 2 turns it
// into descending-n offsets; pass 3 scatters the packed pixel ids (orow << 16
// | x) in that order; the march then gives wave w the sorted pixels
// [64w, 64w + 64).  Lanes of a wave share n (no loop divergence) and the
// longest rays start first (longest-processing-time order, no tail).
constexpr int kKeyBins = 1024;
// Pixels per thread of the sort passes: fewer blocks -> fewer global atomics
// on hot bins.  Measured 2/4/8/16: 16 is best (bin 21 us, scatter 11 us at
// 1080p).  Wave-aggregated LDS increments (one atomic per distinct key) were
// slower than the plain LDS atomics.
constexpr int kSortPixelsPerThread = 16;
__device__ __forceinline__ int cost_key(int n) { return n < kKeyBins - 1 ? n : kKeyBins - 1; }
// The sort passes enumerate pixels by 64x64 regions (one region per block of
// 256 threads x 16 pixels), regions in row-major order.  A key's pixels then
// come out region by region, so the 64 lanes of a sorted wave are one compact
// segment of the n-contour instead of pixels from both sides of the ring
// (row-major enumeration): neighbouring rays share Worley cells and Perlin
// corners, so their LDS table reads broadcast instead of conflicting (config
// 2: 9 % faster together with the fixed table geometry).  With shadow rays
// (config 3) row-major order is kept: there compact waves are all-or-nothing
// in shadow work, which the per-wave compaction balances worse (4 % slower).
constexpr int kSortRegion = 64;
__device__ __forceinline__ bool sort_pixel(const MarchArgs& a, unsigned idx, int* x, int* orow)
{
    if (a.proc.shadow_steps > 0 && !a.proc.enum_regions) {
        *orow = (int)(idx / (unsigned)a.width);
        *x = (int)(idx - (unsigned)*orow * (unsigned)a.width);
        return *orow < a.out_rows;
    }
    const unsigned rx = (unsigned)(a.width + kSortRegion - 1) / kSortRegion;
    const unsigned reg = idx / (kSortRegion * kSortRegion), loc = idx % (kSortRegion * kSortRegion);
    *x = (int)((reg % rx) * kSortRegion + loc % kSortRegion);
    *orow = (int)((reg / rx) * kSortRegion + loc / kSortRegion);
    return *x < a.width && *orow < a.out_rows;
}
// The pixel at sorted position idx: proc_scatter's packed id (orow << 16 | x).
__device__ __forceinline__ void sorted_pixel(const unsigned* __restrict__ order, unsigned idx, int* x, int* orow)
{
    const unsigned pk = order[idx];
    *x = (int)(pk & 0xffffu);
    *orow = (int)(pk >> 16);
}

template <bool SHADOW>
__global__ __launch_bounds__(256) void proc_bin(const MarchArgs a, unsigned* __restrict__ hist,
                                                unsigned short* __restrict__ keys)
{
    __shared__ unsigned h[kKeyBins];
    for (int i = threadIdx.x; i < kKeyBins; i += 256) h[i] = 0;
    __syncthreads();
    for (int it = 0; it < kSortPixelsPerThread; ++it) {
        const unsigned pix = (blockIdx.x * kSortPixelsPerThread + it) * 256u + threadIdx.x;   // < 2^31 (host check)
        int x, orow;
        if (!sort_pixel(a, pix, &x, &orow)) {
            keys[pix] = 0;
            continue;
        }
        const Ray r = setup_ray(a, x, orow);
        int key = 0;
        if (r.n > 0) {
            key = cost_key(r.n);
            atomicAdd(&h[key], 1u);
        } else if (r.live) {
            store_pixel(a, x, orow, r.n >= 0, proc_epilogue<SHADOW>(a, 0.0f, 0.0f));   // 0 steps
        }
        keys[pix] = (unsigned short)key;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kKeyBins; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// Background of a frame whose sorted order is reused (same geometry): the
// pixels with no steps (key 0 in the bin pass) get (0,0,0,1), which is both
// the clear colour and the epilogue of zero steps in every format, so this is
// exactly what proc_bin stores for them.
// Run by the trailing blocks of march_proc_sorted (one launch per reused frame).
__device__ __forceinline__ void proc_fill_background(const MarchArgs& a, const unsigned short* __restrict__ keys,
                                                     unsigned positions, unsigned block, unsigned blocks)
{
    for (unsigned i = block * kThreads + threadIdx.x; i < positions; i += blocks * kThreads) {
        int x, orow;
        if (!sort_pixel(a, i, &x, &orow) || keys[i] != 0) continue;
        const int bl = orow / a.band_rows;
        const int y = set_band(bl, a.band_first, a.band_stride, a.band_flip) * a.band_rows + (orow - bl * a.band_rows);
        if (y < a.height) store_pixel(a, x, orow, false, 0.0f);
    }
}

// hist[kKeyBins] -> cursor[kKeyBins] (start of each key, descending keys) and
// total at cursor[kKeyBins].  One workgroup of kKeyBins threads.
// It also zeroes the histogram for the next frame (the buffer is zeroed once
// when allocated), which saves a memset launch per frame.
// With shadow rays (config 3) it also lays out the deferred passes' scratch
// (ScanOut; went = null: not needed).  Sorted wave w covers the sorted
// positions [64w, 64w + 64), whose keys bound their step counts (key = n below
// kKeyBins - 1, the last key holds every n >= kKeyBins - 1, bounded by
// max_steps).  Its lanes append at most one entry per step, so its entries fit
// the sum of its lanes' bounds, and it marches at most its first (largest)
// key's bound of wave-steps.  went / wrec are the exclusive prefixes of those
// two bounds over the waves -- the thread of a key writes the waves whose
// first position falls in its key's range -- and need[] their totals, which the
// host sizes the scratch from (vr_api.cpp ensure_defer).
struct ScanOut {
    unsigned long long* went;        // [waves + 1]: first entry of sorted wave w
    unsigned* wrec;                  // [waves + 1]: first step record (saturated at 2^32 - 1)
    unsigned long long* need;        // [0] entries, [1] step records of the frame
    unsigned long long* need_host;   // the same, host-mapped (optional)
    int max_steps;
};
// ([[maybe_unused]] on the non-template kernels: vr_march_rect.hip includes
// this header for the tile kernels and launches none of the sort passes)
[[maybe_unused]] __global__ __launch_bounds__(kKeyBins) void proc_scan(unsigned* __restrict__ hist, unsigned* __restrict__ cursor, ScanOut so)
{
    __shared__ unsigned sc[kKeyBins];
    __shared__ unsigned long long ce[kKeyBins], cr[kKeyBins];
    const int t = threadIdx.x;
    const unsigned own = hist[kKeyBins - 1 - t];
    sc[t] = own;   // descending key order
    __syncthreads();
    for (int off = 1; off < kKeyBins; off <<= 1) {
        const unsigned v = t >= off ? sc[t - off] : 0u;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    const int key = kKeyBins - 1 - t;
    const unsigned start = sc[t] - own, end = sc[t];
    cursor[key] = start;   // exclusive
    if (t == kKeyBins - 1) cursor[kKeyBins] = end;
    hist[key] = 0u;              // each thread clears the bin it read
    if (!so.went) return;        // kernel-uniform
    const unsigned long long val = key < kKeyBins - 1 ? (unsigned long long)key
                                                      : (unsigned long long)max(so.max_steps, key);
    const unsigned ws0 = (start + 63u) / 64u, ws1 = (end + 63u) / 64u;   // waves whose first position has this key
    const unsigned long long e_own = (unsigned long long)own * val, r_own = (unsigned long long)(ws1 - ws0) * val;
    ce[t] = e_own;
    cr[t] = r_own;
    __syncthreads();
    for (int off = 1; off < kKeyBins; off <<= 1) {
        const unsigned long long ve = t >= off ? ce[t - off] : 0ull, vr = t >= off ? cr[t - off] : 0ull;
        __syncthreads();
        ce[t] += ve;
        cr[t] += vr;
        __syncthreads();
    }
    const unsigned long long e0 = ce[t] - e_own, r0 = cr[t] - r_own;
    for (unsigned w = ws0; w < ws1; ++w) {
        so.went[w] = e0 + (unsigned long long)(64u * w - start) * val;
        const unsigned long long rw = r0 + (unsigned long long)(w - ws0) * val;
        so.wrec[w] = rw < 0xffffffffull ? (unsigned)rw : 0xffffffffu;
    }
    if (t == kKeyBins - 1) {   // key 0 holds no pixel: its start is the frame's end
        so.went[ws1] = ce[t];
        so.wrec[ws1] = cr[t] < 0xffffffffull ? (unsigned)cr[t] : 0xffffffffu;
        so.need[0] = ce[t];
        so.need[1] = cr[t];
        if (so.need_host) {
            so.need_host[0] = ce[t];
            so.need_host[1] = cr[t];
        }
    }
}

[[maybe_unused]] __global__ __launch_bounds__(256) void proc_scatter(const MarchArgs a, const unsigned short* __restrict__ keys,
                                                    unsigned* __restrict__ cursor, unsigned* __restrict__ order)
{
    __shared__ unsigned h[kKeyBins];
    for (int i = threadIdx.x; i < kKeyBins; i += 256) h[i] = 0;
    __syncthreads();
    int key[kSortPixelsPerThread];
    unsigned rank[kSortPixelsPerThread], packed[kSortPixelsPerThread];
    for (int it = 0; it < kSortPixelsPerThread; ++it) {
        key[it] = -1;
        const unsigned pix = (blockIdx.x * kSortPixelsPerThread + it) * 256u + threadIdx.x;
        int x, orow;
        if (sort_pixel(a, pix, &x, &orow)) {
            const int k = keys[pix];
            if (k > 0) {
                key[it] = k;
                rank[it] = atomicAdd(&h[k], 1u);
                packed[it] = ((unsigned)orow << 16) | (unsigned)x;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kKeyBins; i += 256)
        if (h[i]) h[i] = atomicAdd(&cursor[i], h[i]);   // block's base in the sorted list
    __syncthreads();
    for (int it = 0; it < kSortPixelsPerThread; ++it)
        if (key[it] >= 0) order[h[key[it]] + rank[it]] = packed[it];
}

// The primary procedural marches (unrolled fBm) are held to 4 waves per SIMD
// (<= 128 VGPRs): config 2 -4 % (profiles/r05/ab_proc_diet_*.txt).
template <bool SHADOW, bool EARLY, int TABLE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void march_proc_sorted(
    const MarchArgs a, const unsigned* __restrict__ order, const unsigned* __restrict__ total_ptr,
    const unsigned short* __restrict__ keys, unsigned fill_positions, unsigned fill_first, int stale)
{
    extern __shared__ float4 wt_lds[];
    // A reused sort order (vr_render): blocks from fill_first on write the
    // pixels without steps instead of marching, so a frame is one launch.
    // A stale order (an older camera, same target): the pixels it left out
    // may have steps now, so those blocks march them (unsorted; a 1.6-degree
    // turn moves only the silhouette) -- every pixel is still written once.
    // (Written out here and in march_proc_defer: as one helper the kernels'
    // instruction text changed)
    if (blockIdx.x >= fill_first) {
        if (!stale) {
            proc_fill_background(a, keys, fill_positions, blockIdx.x - fill_first, gridDim.x - fill_first);
            return;
        }
        const float4* wt = worley_table<TABLE>(a.proc, wt_lds);
        unsigned long long steps = 0;
        const unsigned blocks = gridDim.x - fill_first;
        for (unsigned i = (blockIdx.x - fill_first) * kThreads + threadIdx.x; i < fill_positions; i += blocks * kThreads) {
            int x, orow;
            if (sort_pixel(a, i, &x, &orow) && keys[i] == 0) steps += march_pixel_proc<SHADOW, EARLY, TABLE>(a, wt, x, orow);
        }
        if (a.step_counter) add_steps(a, steps);
        return;
    }
    const float4* wt = worley_table<TABLE>(a.proc, wt_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned total = *total_ptr;
    const unsigned base = (blockIdx.x * (kThreads / 64) + wave) * 64u;
    if (base >= total) return;   // wave-uniform
    const unsigned idx = base + lane;
    const bool valid = idx < total;
    int x = 0, orow = 0;
    if (valid) sorted_pixel(order, idx, &x, &orow);
    unsigned long long steps;
    if constexpr (SHADOW) {
        __shared__ ShadowLds sh[kThreads / 64];
        if (a.proc.shadow_steps <= kMaxCompactShadow) {
            unsigned ev = 0;
            steps = march_pixel_proc_compact<EARLY, TABLE>(a, wt, x, orow, valid, &sh[wave], &ev);
            if (a.proc.count_evals) steps += ev;
        } else {
            steps = valid ? march_pixel_proc<true, EARLY, TABLE>(a, wt, x, orow) : 0u;
        }
    } else {
        steps = valid ? march_pixel_proc<false, EARLY, TABLE>(a, wt, x, orow) : 0u;
    }
    if (a.step_counter) add_steps(a, steps);
}

// ---- deferred shadow rays (config 3; vr option "shadow_defer") ----
// The compaction above deals a wave's shadow samples over its own lanes at
// every primary step, so each step ends in a partial round (lane use ~0.85)
// and pays the dealing (box scan, ballot prefix, LDS round trips).  Deferred,
// the frame runs in passes instead:
//  1. march_proc_defer: the primary march of the sorted waves (config 2's loop,
//     64x64-region enumeration).  At a step with rho > 0 a lane appends the
//     entry (P, tv * (rho * od)) -- its ray point and the coefficient the
//     single-scatter term multiplies by the sun transmittance -- to its wave's
//     own region (a running count, no atomics: one device-scope counter for
//     all waves saturates at ~88 adds/us, MI355X_MICROARCH.md, and ran the
//     frame at 3.7 ms), and the wave records {first entry, lane mask} per step.
//  2. proc_shadow_scan / proc_shadow_map: the waves' entries in chunks of 64,
//     numbered across the frame: chunk -> (wave, chunk of the wave, count).
//  3. proc_shadow_eval: one lane per entry walks the S sun samples
//     P + (j+1) L (sequential adds) and sums the in-box densities in step
//     order, tl = exp(-(sl * od)); it rewrites the entry as (coef, tl).  Lanes
//     are busy whatever the owner rays (one partial chunk per wave).
//  4. proc_shadow_resolve: the sorted waves again; a lane folds
//     rad = fma(coef, tl, rad) over its entries in step order and stores the
//     pixel.
// Every value is computed by the same ops in the same order as
// march_pixel_proc<true>, so the frame stays bit-exact.
// (struct ShadowDefer: vr_internal.h)
// The primary march keeps the unrolled fBm without march_proc_sorted's
// occupancy cap: 0.905 ms vs 0.937 capped at 4 waves and 0.910 for round 4's
// build (profiles/r05/ab_defer.txt).
template <bool EARLY, int TABLE>
__global__ __launch_bounds__(kThreads) void march_proc_defer(const MarchArgs a, const unsigned* __restrict__ order,
                                                             const unsigned* __restrict__ total_ptr,
                                                             const unsigned short* __restrict__ keys,
                                                             unsigned fill_positions, unsigned fill_first, int stale,
                                                             ShadowDefer d)
{
    extern __shared__ float4 wt_lds[];
    if (blockIdx.x >= fill_first) {   // as march_proc_sorted: background, or a stale order's leftovers
        if (!stale) {
            proc_fill_background(a, keys, fill_positions, blockIdx.x - fill_first, gridDim.x - fill_first);
            return;
        }
        const float4* wt = worley_table<TABLE>(a.proc, wt_lds);
        unsigned long long steps = 0;
        const unsigned blocks = gridDim.x - fill_first;
        for (unsigned i = (blockIdx.x - fill_first) * kThreads + threadIdx.x; i < fill_positions; i += blocks * kThreads) {
            int x, orow;
            if (sort_pixel(a, i, &x, &orow) && keys[i] == 0) steps += march_pixel_proc<true, EARLY, TABLE>(a, wt, x, orow);
        }
        if (a.step_counter) add_steps(a, steps);
        return;
    }
    const float4* wt = worley_table<TABLE>(a.proc, wt_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned total = *total_ptr;
    const unsigned wid = blockIdx.x * (kThreads / 64) + wave;
    const unsigned base = wid * 64u;
    if (base >= total) return;   // wave-uniform
    const unsigned idx = base + lane;
    // the wave's ranges of entries and step records (proc_scan); past the
    // scratch (a frame larger than the one it was sized for) the wave marches
    // its shadow rays in place, and the later passes skip it
    const unsigned long long eb = d.went[wid];
    const unsigned rb = d.wrec[wid];
    if (d.went[wid + 1] > d.ent_cap || d.wrec[wid + 1] > d.rec_cap) {   // wave-uniform
        unsigned steps = 0;
        if (idx < total) {
            int x, orow;
            sorted_pixel(order, idx, &x, &orow);
            steps = march_pixel_proc<true, EARLY, TABLE>(a, wt, x, orow);
        }
        if (lane == 0) {
            d.wsteps[wid] = kDeferInPlace;
            d.wcount[wid] = 0;
        }
        if (a.step_counter) add_steps(a, steps);
        return;
    }
    Ray r{};
    r.n = -1;
    if (idx < total) {
        int x, orow;
        sorted_pixel(order, idx, &x, &orow);
        r = setup_ray(a, x, orow);
    }
    const ProcParams& p = a.proc;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint4* rec = d.rec + rb;
    float4* ent = d.ent + eb;
    float P0 = r.pxy.x, P1 = r.pxy.y, P2 = r.pz;
    float acc = 0.0f, tv = 1.0f;
    int i = 0;
    bool act = r.n > 0;
    unsigned cells = 0, s = 0, b = 0;   // b: entries the wave appended so far (wave-uniform)
    const DensityK dk = density_k<TABLE>(p, a.scale);
    for (;;) {
        act = act && i < r.n;
        if (__ballot(act) == 0) break;
        float rho = 0.0f;
        if (act) rho = proc_density<TABLE, false, true>(p, dk, wt, P0, P1, P2, cells);
        const bool need = act && rho > 0.0f;
        const unsigned long long m = __ballot(need);
        if (need) ent[b + (unsigned)__popcll(m & lt)] = make_float4(P0, P1, P2, tv * (rho * p.od));
        if (lane == 0) rec[s] = make_uint4(b, (unsigned)m, (unsigned)(m >> 32), 0u);
        b += (unsigned)__popcll(m);
        ++s;
        if (act) {
            acc = acc + rho;
            tv = spec_expf(-(acc * p.od));
            P0 = P0 + r.sxy.x; P1 = P1 + r.sxy.y; P2 = P2 + r.sz;
            ++i;
            if constexpr (EARLY) {
                if (acc > a.acc_limit) act = false;
            }
        }
    }
    if (lane == 0) {
        d.wsteps[wid] = s;
        d.wcount[wid] = b;
    }
    if (a.step_counter) add_steps(a, p.count_evals == 2 ? cells : r.n > 0 ? (unsigned)i : 0u);
}

// Exclusive prefix of the waves' chunk counts (one workgroup; waves past the
// frame's sorted total count 0) and the frame's chunk total in count[0].
constexpr int kScanThreads = 1024;
[[maybe_unused]] __global__ __launch_bounds__(kScanThreads) void proc_shadow_scan(const unsigned* __restrict__ total_ptr, ShadowDefer d)
{
    __shared__ unsigned sc[kScanThreads];
    const int t = threadIdx.x;
    const unsigned nw = min((*total_ptr + 63u) / 64u, d.waves);
    const unsigned per = (nw + kScanThreads - 1) / kScanThreads;
    const unsigned w0 = min((unsigned)t * per, nw), w1 = min(w0 + per, nw);
    unsigned own = 0;
    for (unsigned w = w0; w < w1; ++w) own += (d.wcount[w] + 63u) / 64u;
    sc[t] = own;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const unsigned v = t >= off ? sc[t - off] : 0u;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    unsigned c = sc[t] - own;
    for (unsigned w = w0; w < w1; ++w) {
        d.wchunk[w] = c;
        c += (d.wcount[w] + 63u) / 64u;
    }
    if (t == kScanThreads - 1) d.count[0] = sc[t];
}

// chunk -> (wave, chunk of the wave, entries): one wave per sorted wave.
[[maybe_unused]] __global__ __launch_bounds__(kThreads) void proc_shadow_map(const unsigned* __restrict__ total_ptr, ShadowDefer d)
{
    const unsigned w = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    if (w >= min((*total_ptr + 63u) / 64u, d.waves)) return;
    const unsigned n = d.wcount[w], c0 = d.wchunk[w];
    const unsigned e0 = (unsigned)d.went[w];   // < ent_cap < 2^32 for a wave with entries
    for (unsigned k = lane; k * 64u < n; k += 64u) d.map[c0 + k] = make_uint4(e0 + k * 64u, 0u, min(64u, n - k * 64u), 0u);
}

// The shadow pass's density takes the unrolled forms (proc_density UNROLL),
// held to 5 waves per SIMD: config 3 -2.3 % (profiles/r05/ab_shadow_phased.txt;
// 4 waves, uncapped at 107 VGPRs: level).
template <int TABLE, bool WC>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(5))) void proc_shadow_eval(const MarchArgs a,
                                                                                                      ShadowDefer d)
{
    noise::WorleyCube wc;   // WC: the lane's Worley cube, kept across its samples (and entries)
    extern __shared__ float4 wt_lds[];
    const float4* wt = worley_table<TABLE>(a.proc, wt_lds);
    const ProcParams& p = a.proc;
    const unsigned chunks = *d.count;
    const int S = p.shadow_steps;
    const unsigned lane = threadIdx.x & 63;
    const float l0 = noise::in_vgpr(p.lstep[0]), l1 = noise::in_vgpr(p.lstep[1]), l2 = noise::in_vgpr(p.lstep[2]);
    unsigned evals = 0, cells = 0;
    for (unsigned c = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); c < chunks; c += gridDim.x * (kThreads / 64)) {
        const uint4 mc = d.map[c];   // wave-uniform
#if defined(VR_COUNT_SLOTS) && VR_COUNT_SLOTS == 2
        if (lane == 0) evals += 64u * (unsigned)S;   // lane-slots of the chunk (timing experiment)
#endif
        if (lane >= mc.z) continue;
#if defined(VR_COUNT_SLOTS) && VR_COUNT_SLOTS == 1
        evals += (unsigned)S;   // slots of the entry (timing experiment)
#endif
        float4* e = d.ent + mc.x + lane;
        const float4 en = *e;
        float q0 = en.x, q1 = en.y, q2 = en.z, sl = 0.0f;
        for (int j = 0; j < S; ++j) {
            q0 = q0 + l0; q1 = q1 + l1; q2 = q2 + l2;
            // march_pixel_proc's box test as min3 / max3 (q is never NaN)
            if (fminf(fminf(q0, q1), q2) >= 0.0f && fmaxf(fmaxf(q0, q1), q2) <= 1.0f) {
                // the operands pinned per sample, as before round 5: hoisted out
                // of the loops they take the pass from 75 to 86 VGPRs (6 -> 5
                // waves per SIMD) and it ran 0.4 % slower (profiles/r05)
                const DensityK dk = density_k<TABLE>(p, a.scale);
                sl = sl + proc_density<TABLE, WC, true>(p, dk, wt, q0, q1, q2, cells, &wc);
#ifndef VR_COUNT_SLOTS
                ++evals;
#endif
            }
        }
        const float tl = spec_expf(-(sl * p.od));
        *reinterpret_cast<float2*>(e) = make_float2(en.w, tl);
    }
    if (a.step_counter) add_steps(a, p.count_evals == 2 ? cells : p.count_evals ? evals : 0u);
}

// The shadow pass with 8 lanes per entry (option shadow_cache = 2): lane j of
// an entry's group of 8 evaluates the sun samples j, j + 8, ... of its ray
// (reached by the same sequential adds, P + (s+1) L), and the group sums them
// in sample order through __shfl, so sl is the per-lane loop's, bit for bit
// (an out-of-box sample adds +0, which leaves sl >= +0 unchanged).  The 8
// lanes of a group sample one sun ray a few texels apart, so their Worley
// cube and Perlin corners mostly coincide: their LDS table reads broadcast
// instead of spreading over 64 rays' cells (bank conflicts, verdict r03 #5).
template <int TABLE>
__global__ __launch_bounds__(kThreads) void proc_shadow_eval8(const MarchArgs a, ShadowDefer d)
{
    extern __shared__ float4 wt_lds[];
    const float4* wt = worley_table<TABLE>(a.proc, wt_lds);
    const ProcParams& p = a.proc;
    const unsigned units = *d.count * 8u;   // 8 entries per unit
    const int S = p.shadow_steps;
    const unsigned lane = threadIdx.x & 63, g = lane >> 3, j = lane & 7;
    const float l0 = noise::in_vgpr(p.lstep[0]), l1 = noise::in_vgpr(p.lstep[1]), l2 = noise::in_vgpr(p.lstep[2]);
    unsigned evals = 0, cells = 0;
    const DensityK dk = density_k<TABLE>(p, a.scale);
    for (unsigned u = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); u < units; u += gridDim.x * (kThreads / 64)) {
        const uint4 mc = d.map[u >> 3];   // wave-uniform
        const unsigned k = (u & 7u) * 8u + g;   // the group's entry within the chunk
        const bool has = k < mc.z;
        float4* e = d.ent + mc.x + k;
        float4 en = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (has) en = *e;
        float q0 = en.x, q1 = en.y, q2 = en.z, sl = 0.0f;
        for (unsigned t = 0; t <= j; ++t) { q0 = q0 + l0; q1 = q1 + l1; q2 = q2 + l2; }   // sample j
        for (int r = 0; r < S; r += 8) {
            float v = 0.0f;
            // march_pixel_proc's box test as min3 / max3 (q is never NaN)
            if (has && r + (int)j < S && fminf(fminf(q0, q1), q2) >= 0.0f && fmaxf(fmaxf(q0, q1), q2) <= 1.0f) {
                v = proc_density<TABLE>(p, dk, wt, q0, q1, q2, cells);
                ++evals;
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {   // the group's samples r .. r + 7, in order
                const float vt = __shfl(v, (int)(g * 8u) + t);
                if (r + t < S) sl = sl + vt;
            }
            for (int t = 0; t < 8; ++t) { q0 = q0 + l0; q1 = q1 + l1; q2 = q2 + l2; }   // sample j + r + 8
        }
        if (has && j == 0) *reinterpret_cast<float2*>(e) = make_float2(en.w, spec_expf(-(sl * p.od)));
    }
    if (a.step_counter) add_steps(a, p.count_evals == 2 ? cells : p.count_evals ? evals : 0u);
}

// Steps folded per batch in the resolve pass: lanes 0..31 load the batch's
// step records with one vector load, v_readlane hands each record to the
// wave, and every lane issues its entry loads back to back (the fold itself is
// a serial fma chain; the loads are independent): two round trips per batch.
constexpr int kResolveBatch = 32;
[[maybe_unused]] __global__ __launch_bounds__(kThreads) void proc_shadow_resolve(const MarchArgs a, const unsigned* __restrict__ order,
                                                                const unsigned* __restrict__ total_ptr, ShadowDefer d)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned total = *total_ptr;
    const unsigned wid = __builtin_amdgcn_readfirstlane(blockIdx.x * (kThreads / 64) + wave);
    const unsigned base = wid * 64u;
    if (base >= total) return;
    const unsigned ns = d.wsteps[wid];
    if (ns == kDeferInPlace) return;   // the primary pass stored this wave's pixels
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint4* rec = d.rec + d.wrec[wid];
    const float4* ent = d.ent + d.went[wid];
    float rad = 0.0f;
    for (unsigned s0 = 0; s0 < ns; s0 += kResolveBatch) {
        uint4 rc = make_uint4(0u, 0u, 0u, 0u);
        if (lane < kResolveBatch && s0 + lane < ns) rc = rec[s0 + lane];
        float2 v[kResolveBatch];
        bool h[kResolveBatch];
#pragma unroll
        for (int k = 0; k < kResolveBatch; ++k) {
            // (readlane returns int: widen the low word unsigned, not sign-extended)
            const unsigned bk = (unsigned)__builtin_amdgcn_readlane(rc.x, k);
            const unsigned long long m = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(rc.z, k) << 32) |
                                         (unsigned long long)(unsigned)__builtin_amdgcn_readlane(rc.y, k);
            h[k] = (m >> lane) & 1ull;
            v[k] = make_float2(0.0f, 0.0f);
            if (h[k]) v[k] = *reinterpret_cast<const float2*>(ent + bk + (unsigned)__popcll(m & lt));
        }
#pragma unroll
        for (int k = 0; k < kResolveBatch; ++k)
            if (h[k]) rad = fmaf(v[k].x, v[k].y, rad);
    }
    const unsigned idx = base + lane;
    if (idx < total) {
        int x, orow;
        sorted_pixel(order, idx, &x, &orow);
        const Ray r = setup_ray(a, x, orow);
        if (r.live) store_pixel(a, x, orow, r.n >= 0, rad);
    }
}

// Dynamic LDS of a procedural kernel: the Worley cell table (worley_table), if any
inline size_t worley_table_bytes(const ProcParams& p)
{
    return p.wt_n > 0 ? ((size_t)p.wt_n * p.wt_pz + 512) * sizeof(float4) : 0;
}
// The variant of a procedural tile kernel (march_proc, march_proc_rect, march_proc_rects):
// launch(SHADOW, EARLY, TABLE, LDS bytes), TABLE 1 = the Worley cells from LDS at runtime geometry
template <class F>
hipError_t with_proc_variant(const MarchArgs& a, bool early, F&& launch)
{
    const size_t wt_bytes = worley_table_bytes(a.proc);
    return with_bool(a.proc.shadow_steps > 0, [&](auto S) { return with_bool(early, [&](auto E) {
        return with_value<0, 1>(wt_bytes ? 1 : 0, [&](auto T) {
            launch(S, E, T, wt_bytes);
            return hipGetLastError();
        }, hipErrorInvalidValue);
    }); });
}

}  // namespace
}  // namespace vr
