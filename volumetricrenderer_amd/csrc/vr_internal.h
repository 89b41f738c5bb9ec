// vr_internal.h -- internal structures shared by the HIP kernels and the C ABI
// (not installed; the public interface is include/vr.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/vr.h"
#include "vr_dispatch.h"

namespace vr {

// Volume layouts in HBM.  Each keeps one array per
// channel, so a tap reads only the channel it needs (frag.glsl:66-69 read
// .x, .y, .z, .w at four different coordinates).
//
// LAYOUT_PLANAR is the canonical copy and the source of every other layout.
// It is u8 plane[z][y][x], takes any wrap mode, and does 8 byte loads per tap.
//
// The fast layouts are indexed by the *padded* base texel a = floor(g), with
// g = u*N + 0.5 and a in [0, N].  They store the clamp-to-edge values of the
// 2x2x2 trilinear footprint, so a tap needs no index wrapping.  They are
// exact wherever clamp-to-edge equals mirrored repeat.  The host checks that
// per frame; otherwise LAYOUT_PLANAR runs.  A tap's byte offset is
// TX[a] + TY[b] + TZ[c], from three per-axis tables the kernel keeps in LDS,
// so the brick geometry costs two adds per tap.
enum Layout : int {
    LAYOUT_PLANAR = 1,
    LAYOUT_BRICK5 = 2,    // B=4: 4^3 texels + 1-texel apron = 5^3 B in one 128-B
                          // line (2.0x bytes); a footprint never leaves its line
    LAYOUT_BRICK8 = 3,    // B=7: 8^3 = 512 B bricks (1.49x bytes)
    LAYOUT_BRICK16 = 4,   // B=15: 16^3 = 4 KiB bricks (1.21x bytes)
    LAYOUT_CORNER8 = 5,   // per base texel its 8 footprint bytes (u64) in 4^3
                          // position bricks of 512 B (8x bytes); 1 load per tap
    LAYOUT_BRICK4 = 6,    // B=3: 3^3 texels + apron = 4^3 = 64 B (2.37x bytes);
                          // a z-slice of a footprint is one dword-aligned 8-B load
    LAYOUT_ZPAIR = 7,     // 4x16x2 texels = 128 B (3x15x1 positions, 2.93x bytes),
                          // 4-byte rows ordered z-fastest: rows (y,z) (y,z+1)
                          // (y+1,z) (y+1,z+1) are 16 contiguous bytes, so a whole
                          // footprint is one dword-aligned 16-B load
    LAYOUT_BRICK448 = 8,  // 4x4x8 texels = 128 B (3x3x7 positions, 2.03x bytes);
                          // BRICK4's in-brick order, so the same two 8-B loads
    LAYOUT_BRICK488 = 9,  // 4x8x8 texels = 256 B (3x7x7 positions, 1.74x bytes);
                          // slices 32 B apart
    LAYOUT_BRICK4816 = 10,   // 4x8x16 texels = 512 B (3x7x15 positions, 1.60x bytes)
    LAYOUT_BRICK41616 = 11,  // 4x16x16 texels = 1 KiB (3x15x15 positions, 1.52x
                             // bytes); slices 64 B apart
    LAYOUT_BRICK4832 = 12,   // 4x8x32 texels = 1 KiB (3x7x31 positions, 1.53x bytes)
    LAYOUT_BRICK4864 = 13,   // 4x8x64 texels = 2 KiB (3x7x63 positions, 1.51x bytes)
    LAYOUT_CORNERH = 14,     // per base position 16 B: for each footprint row (y,z)
                             // the f16 pair {a, b - a} of its x-neighbours a, b, so
                             // each x-lerp is one v_fma_mix_f32; x fastest, no
                             // bricks: the index is computed in fp32 (16x bytes)
    LAYOUT_COL48 = 15,       // columns of 4x8 texels (3x7 positions) through the whole
                             // z extent, slices 32 B apart (1.52x bytes): BRICK4832
                             // without z bricks, so any run of slices of a column is
                             // contiguous -- the fill unit of the LDS slab march
                             // (vr_march_slab.hip); also a plain BRICK4-family layout
    LAYOUT_COL48Z = 16,      // channels 0-2 as COL48, channel 3 as ZPAIR (one 16-B load per
                             // tap): the reference's smallest-scale tap (A at 0.7,
                             // frag.glsl:69) trades 1.9x its bytes for half its loads
};
constexpr int kNumLayouts = 17;
// CORNERH's fp32 index a + (nx+1)(b + (ny+1)c) is exact below 2^24 positions
constexpr long long kCornerHMaxPositions = 1ll << 24;
// the layouts whose taps are BRICK4's two dword-aligned 8-B loads
__host__ __device__ constexpr bool is_b4_family(int l)
{
    return l == LAYOUT_BRICK4 || l == LAYOUT_BRICK448 || l == LAYOUT_BRICK488 || l == LAYOUT_BRICK4816 ||
           l == LAYOUT_BRICK41616 || l == LAYOUT_BRICK4832 ||
           l == LAYOUT_BRICK4864 || l == LAYOUT_COL48;
}

// Variants measured slower than the defaults and kept as the record of that
// (DESIGN.md sec. 4, 5.1-5.4): the layouts other than the auto ones, the
// queue / strided / XCD-row schedules, 8- and 16-wave workgroups, and the
// procedural sort_reuse / proc_enum options.  They are compiled only with
// VR_EXPERIMENTS=1 (make EXPERIMENTS=1); the default library refuses their
// options.  The LDS slab march (north star; option slab, off by default) is
// in every build so that its parity test runs in the default GPU suite.
#ifndef VR_EXPERIMENTS
#define VR_EXPERIMENTS 0
#endif
// The layouts each march translation unit instantiates; a launcher reaches a kernel only
// through with_layout over one of these (vr_dispatch.h), so a layout outside its unit's
// list is an error there, never another kernel.
#if VR_EXPERIMENTS
using ExperimentLayouts = value_list<LAYOUT_BRICK4, LAYOUT_BRICK448, LAYOUT_BRICK488, LAYOUT_BRICK4816, LAYOUT_BRICK4864,
                                     LAYOUT_BRICK41616, LAYOUT_COL48Z, LAYOUT_ZPAIR, LAYOUT_BRICK5, LAYOUT_BRICK8,
                                     LAYOUT_BRICK16>;
#else
using ExperimentLayouts = value_list<>;
#endif
using MarchLayouts = list_cat_t<value_list<LAYOUT_PLANAR, LAYOUT_COL48, LAYOUT_BRICK4832>, ExperimentLayouts>;   // vr_march.hip
using CornerLayouts = value_list<LAYOUT_CORNER8, LAYOUT_CORNERH>;   // vr_march_c8.hip, compiled in parallel with it
using BuiltLayouts = list_cat_t<MarchLayouts, CornerLayouts>;       // every layout of this build: vr_march_rect.hip
// the multi-frame kernels (march_regions_frames); CORNERH's are vr_march_c8.hip's
using FrameLayouts = value_list<LAYOUT_COL48, LAYOUT_BRICK4832, LAYOUT_CORNERH>;
constexpr bool layout_built(int l) { return list_has(BuiltLayouts{}, l); }

enum Wrap : int { WRAP_CLAMP = 0, WRAP_MIRROR = 1 };
// with_layout, and the wrap mode: f(layout tag, wrap tag).  Only PLANAR has WRAP_MIRROR;
// the fast layouts store clamp-to-edge footprints and run where the two agree.
template <class LayoutList, class F>
hipError_t with_layout_wrap(int layout, int wrap, F&& f)
{
    return with_layout<LayoutList>(layout, [&](auto L) {
        if constexpr (L == LAYOUT_PLANAR)
            if (wrap != WRAP_CLAMP) return f(L, std::integral_constant<int, WRAP_MIRROR>{});
        return f(L, std::integral_constant<int, WRAP_CLAMP>{});
    });
}

// Geometry of a fast layout for one channel (host and device).
struct LayoutGeom {
    int B;          // useful positions per brick edge (cubic layouts)
    int R;          // stored edge of an apron brick, R = B + 1
    int Ba[3];      // useful positions per brick along x, y, z
    int Rn[3];      // stored texels per brick along x, y, z (in-brick order x fastest)
    unsigned brick; // bytes per brick
    int nbx, nby, nbz;
};
__host__ __device__ inline LayoutGeom layout_geom(int layout, int nx, int ny, int nz)
{
    LayoutGeom g{};
    if (layout == LAYOUT_CORNER8) {
        g.B = 4; g.R = 4; g.brick = 512;
    } else if (layout == LAYOUT_CORNERH) {
        g.B = 1; g.R = 1; g.brick = 16;
    } else if (layout == LAYOUT_ZPAIR) {
        g.B = 3; g.R = 4; g.brick = 128;
    } else if (layout == LAYOUT_COL48 || layout == LAYOUT_COL48Z) {
        // slices c and c + 1 for every padded position c in [0, nz]: nz + 2
        // slices, rounded up to an even count (64-B chunks of two slices)
        g.B = 3; g.R = 4;
        g.brick = 32u * (unsigned)((nz + 3) & ~1);
    } else if (layout == LAYOUT_BRICK448 || layout == LAYOUT_BRICK488 || layout == LAYOUT_BRICK4816 ||
               layout == LAYOUT_BRICK41616 || layout == LAYOUT_BRICK4832 || layout == LAYOUT_BRICK4864) {
        g.B = 3; g.R = 4;
        g.brick = layout == LAYOUT_BRICK448 ? 128u : layout == LAYOUT_BRICK488 ? 256u
                : layout == LAYOUT_BRICK4816 ? 512u : layout == LAYOUT_BRICK4864 ? 2048u : 1024u;
    } else {
        g.B = layout == LAYOUT_BRICK4 ? 3 : layout == LAYOUT_BRICK5 ? 4 : layout == LAYOUT_BRICK8 ? 7 : 15;
        g.R = g.B + 1;
        const unsigned r3 = (unsigned)(g.R * g.R * g.R);
        // whole 128-B lines; BRICK4's 64-B bricks pair up in one line
        g.brick = layout == LAYOUT_BRICK4 ? 64u : (r3 + 127u) & ~127u;
    }
    g.Ba[0] = g.Ba[1] = g.Ba[2] = g.B;
    g.Rn[0] = g.Rn[1] = g.Rn[2] = g.R;
    if (layout == LAYOUT_ZPAIR) { g.Ba[1] = 15; g.Ba[2] = 1; }
    if (layout == LAYOUT_BRICK448) { g.Ba[2] = 7; g.Rn[2] = 8; }
    if (layout == LAYOUT_BRICK488) { g.Ba[1] = g.Ba[2] = 7; g.Rn[1] = g.Rn[2] = 8; }
    if (layout == LAYOUT_BRICK4816) { g.Ba[1] = 7; g.Rn[1] = 8; g.Ba[2] = 15; g.Rn[2] = 16; }
    if (layout == LAYOUT_BRICK4864) { g.Ba[1] = 7; g.Rn[1] = 8; g.Ba[2] = 63; g.Rn[2] = 64; }
    if (layout == LAYOUT_BRICK4832) { g.Ba[1] = 7; g.Rn[1] = 8; g.Ba[2] = 31; g.Rn[2] = 32; }
    if (layout == LAYOUT_BRICK41616) { g.Ba[1] = g.Ba[2] = 15; g.Rn[1] = g.Rn[2] = 16; }
    if (layout == LAYOUT_COL48 || layout == LAYOUT_COL48Z) { g.Ba[1] = 7; g.Rn[1] = 8; g.Ba[2] = nz + 1; g.Rn[2] = (nz + 3) & ~1; }
    // padded base positions a in [0, N] -> bricks a / B in [0, N / B]
    g.nbx = nx / g.Ba[0] + 1;
    g.nby = ny / g.Ba[1] + 1;
    g.nbz = nz / g.Ba[2] + 1;
    return g;
}
// byte offset of padded position a along axis 0/1/2 inside one channel plane
__host__ __device__ inline unsigned axis_offset(const LayoutGeom& g, int layout, int axis, int a)
{
    const unsigned q = (unsigned)(a / g.Ba[axis]), r = (unsigned)(a % g.Ba[axis]);
    const unsigned stride = axis == 0 ? g.brick : axis == 1 ? g.brick * (unsigned)g.nbx
                                                            : g.brick * (unsigned)g.nbx * (unsigned)g.nby;
    if (layout == LAYOUT_CORNER8) return q * stride + (r << (3 + 2 * axis));   // 8 B per position
    if (layout == LAYOUT_ZPAIR) return q * stride + (axis == 0 ? r : axis == 1 ? 8u * r : 0u);
    return q * stride + r * (axis == 0 ? 1u : axis == 1 ? (unsigned)g.Rn[0] : (unsigned)(g.Rn[0] * g.Rn[1]));
}

// Procedural medium parameters (vr_procedural; BASELINE configs 2/3).
struct ProcParams {
    float grid_scale;
    int octaves;
    float freq0, lacunarity, gain;
    int seed_fbm;
    float worley_freq;
    int seed_worley;
    int shadow_steps;
    float lstep[3];   // (step_size * sun_dir) / box_range
    float od;         // step_size * density
    int count_evals;  // step_counter counts: 0 ray-steps, 1 density evaluations (incl. shadow
                      // samples), 2 Worley cells computed (8 or 35 per evaluation when pruned, else 27)
    int wt_lo, wt_n;  // Worley cell table in LDS: cells [wt_lo, wt_lo + wt_n)^3; wt_n = 0: none
    int wt_pz;        // its z pitch in entries (>= wt_n^2, padded against LDS bank aliasing)
    int wt_fixed;     // 1: the fixed geometry wt_n = 9, wt_pz = 83 (noise::cellular_table9)
    int enum_regions; // sort passes: 1 = 64x64-region enumeration also with shadow rays
    // Perlin lattice table (global, noise::perlin_lattice_entry): cells
    // [lat_lo, lat_lo + lat_n)^3, entry (x, y, z) at byte offset
    // 8 x + lat_sy y + lat_sz z - lat_c, all exact in fp32.  Null: none.
    const uint2* lat;
    unsigned lat_bytes;
    float lat_c, lat_sy, lat_sz;
};

// Everything one launch of the march kernel needs.  Passed by value
// (kernarg segment), computed on the host per vr_render call.
struct MarchArgs {
    // ray basis in box-local space: dir(x,y) = o + (x+.5)*px + (y+.5)*py
    float org[3], o[3], px[3], py[3];
    float r2[4], r3[4];          // rows 2/3 of P*V*M (coverage clip test)
    int cam_mode;                // 1: org/o/px/py are the View eye's, the march starts at cam (RayBasis)
    float cam[3];
    float box_min[3], box_max[3], box_range[3];
    float step_size, density, scale, acc_limit;
    int max_steps;
    // tap t samples padded texel coordinate g = fma(P, tap_S, tap_T)
    // (= u*N + 0.5 with u = P*s_t + o_t, frag.glsl:66-69)
    float tap_S[4][3], tap_T[4][3];
    int zero_offsets;            // every tap_T is exactly 0.5 (no MediaScroll offsets)
    // uniform channels (vr_api.cpp install_volume: min == max over the plane):
    // bit t set = every texel of channel t is v_t, so tap t is exactly
    // uval[t] = v_t * (1/255) (the spec's lerps of equal values return them,
    // DESIGN.md sec. 3.2) and the march needs no load for it
    int umask;
    float uval[4];
    // COL48Z: channel 3's ZPAIR plane (geometry, bytes) after the three COL48 planes
    LayoutGeom geom3;
    unsigned plane3_bytes;
    // volume
    int nx, ny, nz;
    const uint8_t* vol;          // channel plane 0; plane c at vol + c*plane_stride
    unsigned plane_stride;       // bytes (< 2^31)
    LayoutGeom geom;             // fast layouts
    // target
    int width, height, band_rows, band_stride, band_first, out_rows;
    int band_flip;               // vr_target.band_flip: odd bands of the set shifted (set_band)
    int tiles_x, tiles_y, num_blocks;   // static schedule: 16x16 tiles
    void* out;
    long long pitch;
    int format;
    int empty_fill;              // regions lists: march each XCD's first hdr[kRegionWork + x] entries, fill the
                                 // rest (tiles no ray of which meets the box) with the uncovered value
    int bands_in_place;          // vr.h VR_TARGET_BANDS_IN_PLACE: packed row orow is stored at its frame row
    unsigned long long* step_counter;
    ProcParams proc;
    int slab_cap;                // LDS slab march (COL48): chunks per channel the slab holds
};

// Dynamic LDS of a march kernel: the per-axis offset tables of fast_prologue
// (vr_march_kernels.h; COL48Z keeps a second set for channel 3's ZPAIR plane);
// PLANAR and CORNERH compute their offsets
template <int L>
constexpr size_t march_lds_bytes(const MarchArgs& a)
{
    if (L == LAYOUT_PLANAR || L == LAYOUT_CORNERH) return 0;
    return (size_t)(a.nx + a.ny + a.nz + 3) * sizeof(unsigned) * (L == LAYOUT_COL48Z ? 2 : 1);
}

// The _u kernels (march_regions_u, march_regions_frames_u, march_regions_split's UM): a
// regions march that skips the loads of one uniform channel.  They are built for these
// layouts, without early-out, for zero tap offsets and for exactly one uniform channel;
// every other case runs the general kernel, which is exact too.  u_kernel_channel: the
// channel a _u kernel skips (the kernel's UM is 1 << channel = umask), or -1 for none.
constexpr bool has_u_kernels(int l)
{
    return l == LAYOUT_COL48 || l == LAYOUT_BRICK4832 || l == LAYOUT_CORNERH || l == LAYOUT_COL48Z;
}
constexpr int u_kernel_channel(bool early, bool zero_offsets, int umask)
{
    if (early || !zero_offsets) return -1;
    return umask == 1 ? 0 : umask == 2 ? 1 : umask == 4 ? 2 : umask == 8 ? 3 : -1;
}

// The kernels with a QUAD instance (four frames of one camera in the lanes of a quad,
// vr_march_kernels.h regions_frames_body): every multi-frame kernel but the general one of
// COL48 / BRICK4832 with zero offsets and no early-out, whose QUAD instance needs 97 VGPRs
// where the NF = 4 one needs 96 and so loses a wave per SIMD; its
// launches keep the NF = 4 kernel until the trade is measured.
constexpr bool quad_instance(int layout, bool early, bool zero_offsets, int umask)
{
    if (u_kernel_channel(early, zero_offsets, umask) >= 0) return true;   // the _u kernels
    return !(is_b4_family(layout) && !early && zero_offsets);
}

// How a four-frame launch uses the lanes of a quad (launch_march_frames; the multi-frame
// kernels' template parameter QM).  Each mode is the one before it and one thing more, so the
// order of the enum is the meaning and the predicates below are the only place that says so:
//   QUAD_NONE    wave = frame, a quad's lanes are four pixels
//   QUAD_FRAMES  the QUAD instance: a quad's lanes are the four frames of one pixel, one ray
//   QUAD_SPLIT   and the lanes split each tap's loads between them (option quad_split;
//                vr_march_kernels.h march_pixel_quad_split)
//   QUAD_STEPS   and each lane fetches and blends one step of four (option quad_steps;
//                march_pixel_quad_steps)
//   QUAD_PAIRS   and a round's loads are issued in slice pairs (option quad_pairs;
//                march_pixel_quad_steps<QUAD_PAIRS>, the lane maps below)
// The split fetch and all that builds on it exist for the layouts whose footprint slice packs
// into one dword, 32 bytes apart in z (quad_split_layout).
enum QuadMode : int { QUAD_NONE = 0, QUAD_FRAMES = 1, QUAD_SPLIT = 2, QUAD_STEPS = 3, QUAD_PAIRS = 4 };
constexpr int kGroupFrames = 4;   // the frames of a group launch (vr_render_group): the lanes of a quad
constexpr __host__ __device__ bool quad_is_quad(int mode) { return mode >= QUAD_FRAMES; }
constexpr __host__ __device__ bool quad_splits(int mode) { return mode >= QUAD_SPLIT; }
constexpr __host__ __device__ bool quad_rounds(int mode) { return mode >= QUAD_STEPS; }
constexpr __host__ __device__ bool quad_paired(int mode) { return mode >= QUAD_PAIRS; }
constexpr bool quad_split_layout(int layout) { return layout == LAYOUT_COL48 || layout == LAYOUT_BRICK4832; }
constexpr unsigned kSplitZ = 32;   // bytes between the z-slices of those layouts (vr_march_kernels.h tap_fetch's kZ)

// The mode a context's options ask for (vr_render.cpp render_frames): each option switches on
// the mode that builds on the one before it.  eligible: four frames of one camera, none counted.
constexpr int quad_requested(bool eligible, bool frame_quad, bool quad_split, bool quad_steps, bool quad_pairs)
{
    return !(eligible && frame_quad) ? QUAD_NONE : !quad_split ? QUAD_FRAMES : !quad_steps ? QUAD_SPLIT
         : !quad_pairs ? QUAD_STEPS : QUAD_PAIRS;
}
// The mode of the kernel that runs a launch of nf frames for a requested mode: the request cut
// down to what the kernel has.  render_frames launches this mode; launch_frames_l instantiates
// it for every (layout, nf, early, zero_offsets, umask, request) and refuses a request it cuts.
constexpr int quad_kernel_mode(int layout, int nf, bool early, bool zero_offsets, int umask, int requested)
{
    if (nf != kGroupFrames || !quad_instance(layout, early, zero_offsets, umask)) return QUAD_NONE;   // a quad is four frames
    if (!quad_split_layout(layout)) return requested < QUAD_FRAMES ? requested : QUAD_FRAMES;
    return requested;
}

// The occupancy floor (amdgpu_waves_per_eu) of a multi-frame kernel.  1 is the floor a kernel
// of 4-wave workgroups has without the attribute.
constexpr int quad_waves_floor(int mode, bool zero_offsets, bool early)
{
    if (!quad_splits(mode)) return 1;
    if (quad_rounds(mode) && !zero_offsets) return 1;
    if (quad_paired(mode) && early) return 1;
    return 5;
}
// (mode, zero_offsets, early) -> the floor
static_assert(quad_waves_floor(QUAD_NONE, false, false) == 1 && quad_waves_floor(QUAD_NONE, false, true) == 1 &&
              quad_waves_floor(QUAD_NONE, true, false) == 1 && quad_waves_floor(QUAD_NONE, true, true) == 1 &&
              quad_waves_floor(QUAD_FRAMES, false, false) == 1 && quad_waves_floor(QUAD_FRAMES, false, true) == 1 &&
              quad_waves_floor(QUAD_FRAMES, true, false) == 1 && quad_waves_floor(QUAD_FRAMES, true, true) == 1,
              "no split fetch: compiled as before it");
static_assert(quad_waves_floor(QUAD_SPLIT, false, false) == 5 && quad_waves_floor(QUAD_SPLIT, false, true) == 5 &&
              quad_waves_floor(QUAD_SPLIT, true, false) == 5 && quad_waves_floor(QUAD_SPLIT, true, true) == 5,
              "left alone the scheduler spreads a pair's six blends over 102 VGPRs (4 waves); with the floor 75, no scratch");
static_assert(quad_waves_floor(QUAD_STEPS, true, false) == 5 && quad_waves_floor(QUAD_STEPS, true, true) == 5,
              "zero tap offsets: 102 VGPRs without the floor, 96 or fewer and no scratch with it");
static_assert(quad_waves_floor(QUAD_STEPS, false, false) == 1 && quad_waves_floor(QUAD_STEPS, false, true) == 1,
              "tap offsets: the floor costs 8 bytes of scratch (124 VGPRs, 4 waves without it)");
static_assert(quad_waves_floor(QUAD_PAIRS, true, false) == 5 && quad_waves_floor(QUAD_PAIRS, false, false) == 1 &&
              quad_waves_floor(QUAD_PAIRS, false, true) == 1,
              "the paired fetch follows the step rounds");
static_assert(quad_waves_floor(QUAD_PAIRS, true, true) == 1, "but the early-out instance spills 40 bytes under the floor");

// The lane maps of the paired fetch.  A round of four steps loads a tap
// with two b64 instructions, I = 0 (A) and 1 (B).  In instruction I quad lane fl loads z-slice
// pair_load_slice(fl) of the round's step pair_load_step(I, fl), the step that quad lane of the
// same number owns: one instruction names both slices of two steps, the split fetch's address
// set.  The owner of step j then finds slice z of its step in the register of instruction
// pair_owner_instr(j) on quad lane pair_owner_lane(j, z).  quad_perm_ctrl is the DPP control
// with which lane k of a quad reads lane l[k].  tools/pair_check.cpp runs a quad through them.
constexpr __host__ __device__ int pair_load_step(int instr, int fl) { return 2 * instr + (fl >> 1); }
constexpr __host__ __device__ int pair_load_slice(int fl) { return fl & 1; }
constexpr __host__ __device__ int pair_owner_instr(int j) { return j >> 1; }
constexpr __host__ __device__ int pair_owner_lane(int j, int z) { return 2 * (j & 1) + z; }
constexpr __host__ __device__ int quad_perm_ctrl(int l0, int l1, int l2, int l3) { return l0 | l1 << 2 | l2 << 4 | l3 << 6; }
constexpr __host__ __device__ int quad_lane_ctrl(int j) { return quad_perm_ctrl(j, j, j, j); }   // every lane reads lane j
// the loaders' read of the owners' offsets for instruction I, and the owners' read of slice z
constexpr __host__ __device__ int pair_load_ctrl(int instr)
{
    return quad_perm_ctrl(pair_load_step(instr, 0), pair_load_step(instr, 1), pair_load_step(instr, 2), pair_load_step(instr, 3));
}
constexpr __host__ __device__ int pair_owner_ctrl(int z)
{
    return quad_perm_ctrl(pair_owner_lane(0, z), pair_owner_lane(1, z), pair_owner_lane(2, z), pair_owner_lane(3, z));
}
static_assert(pair_load_ctrl(0) == 0x50 && pair_load_ctrl(1) == 0xfa, "quad_perm [0,0,1,1] and [2,2,3,3]");
static_assert(pair_owner_ctrl(0) == 0x88 && pair_owner_ctrl(1) == 0xdd, "quad_perm [0,2,0,2] and [1,3,1,3]");

// One round of march_pixel_quad_steps' accumulation: t[j] is the term of step base + j (formed
// by quad lane j), n the ray's steps.  The terms are added in step order, each only where the
// ray has that step and no earlier sum passed acc_limit (EARLY), so acc takes the values of
// the sequential loop `acc = acc + term; if (EARLY && acc > acc_limit) break;` one after the
// other.  *stop: the early-out ended the march in this round.  tools/round_check.cpp compares
// the two on the host.
template <bool EARLY>
__host__ __device__ inline float quad_round_accumulate(float acc, float t0, float t1, float t2, float t3, int base, int n,
                                                       float acc_limit, bool* stop)
{
    bool st = false;
    const float t[4] = {t0, t1, t2, t3};
    for (int j = 0; j < 4; ++j) {
        acc = base + j < n && !st ? acc + t[j] : acc;
        if (EARLY) st = acc > acc_limit;
    }
    *stop = st;
    return acc;
}

// The part of MarchArgs that differs between the frames of one multi-frame launch
// (vr_render_pair, vr_render_group): the camera (ray basis, r2 / r3, cam, tap_T), the
// target buffer, the empty-tile fill and the step counter -- what vr_render.cpp's
// pair_compatible leaves out.  Everything else is the launch's common part.  A field
// that a later change makes per-frame moves here (and into frame_part / set_frame and out
// of pair_compatible): the two- and the four-frame kernels both read it from FramesArgs.
struct FrameArgs {
    float org[3], o[3], px[3], py[3];
    float r2[4], r3[4];
    int cam_mode;
    float cam[3];
    float tap_T[4][3];
    int empty_fill;
    void* out;
    unsigned long long* step_counter;
};
__host__ __device__ inline FrameArgs frame_part(const MarchArgs& a)
{
    FrameArgs f{};
    for (int i = 0; i < 3; ++i) { f.org[i] = a.org[i]; f.o[i] = a.o[i]; f.px[i] = a.px[i]; f.py[i] = a.py[i]; f.cam[i] = a.cam[i]; }
    for (int i = 0; i < 4; ++i) { f.r2[i] = a.r2[i]; f.r3[i] = a.r3[i]; }
    for (int t = 0; t < 4; ++t)
        for (int i = 0; i < 3; ++i) f.tap_T[t][i] = a.tap_T[t][i];
    f.cam_mode = a.cam_mode;
    f.empty_fill = a.empty_fill;
    f.out = a.out;
    f.step_counter = a.step_counter;
    return f;
}
__host__ __device__ inline void set_frame(MarchArgs* a, const FrameArgs& f)
{
    for (int i = 0; i < 3; ++i) { a->org[i] = f.org[i]; a->o[i] = f.o[i]; a->px[i] = f.px[i]; a->py[i] = f.py[i]; a->cam[i] = f.cam[i]; }
    for (int i = 0; i < 4; ++i) { a->r2[i] = f.r2[i]; a->r3[i] = f.r3[i]; }
    for (int t = 0; t < 4; ++t)
        for (int i = 0; i < 3; ++i) a->tap_T[t][i] = f.tap_T[t][i];
    a->cam_mode = f.cam_mode;
    a->empty_fill = f.empty_fill;
    a->out = f.out;
    a->step_counter = f.step_counter;
}
// A multi-frame launch's kernel argument: the common part (frame 0's MarchArgs) and the
// NF frames' own parts, NF = 2 (vr_render_pair) or kGroupFrames (vr_render_group)
template <int NF>
struct FramesArgs {
    MarchArgs c;
    FrameArgs fr[NF];
};
using GroupArgs = FramesArgs<kGroupFrames>;
// The frames of a four-frame launch share one camera: fr[1..3] equal fr[0] bit for bit in
// every field but the target buffer and the step counter, so one ray serves a pixel of all
// four (the QUAD kernels).  Every field is named in the bindings below: one added to
// FrameArgs does not compile here until it is classified as compared or per-frame.
inline bool frames_share_camera(const FrameArgs* fr, int n)
{
    if (n != kGroupFrames) return false;
    const auto& [org0, o0, px0, py0, r20, r30, cam_mode0, cam0, tap_T0, empty_fill0, out0, step_counter0] = fr[0];
    (void)out0; (void)step_counter0;   // per frame
    for (int k = 1; k < n; ++k) {
        const auto& [org, o, px, py, r2, r3, cam_mode, cam, tap_T, empty_fill, out, step_counter] = fr[k];
        (void)out; (void)step_counter;   // per frame
#define VR_SAME(A, B) (sizeof(A) == sizeof(B) && __builtin_memcmp(&(A), &(B), sizeof(A)) == 0)
        if (!(VR_SAME(org, org0) && VR_SAME(o, o0) && VR_SAME(px, px0) && VR_SAME(py, py0) && VR_SAME(r2, r20) &&
              VR_SAME(r3, r30) && VR_SAME(cam_mode, cam_mode0) && VR_SAME(cam, cam0) && VR_SAME(tap_T, tap_T0) &&
              VR_SAME(empty_fill, empty_fill0)))
            return false;
#undef VR_SAME
    }
    return true;
}
static_assert(sizeof(FramesArgs<2>) + 64 <= 4096 && sizeof(GroupArgs) + 64 <= 4096,
              "one MarchArgs, the FrameArgs and the lists' pointers travel in the 4-KiB kernarg segment");

// The frame band of a band set's k-th band (vr_target): band_first + k *
// band_stride, every odd one shifted by band_flip (the serpentine deal)
__host__ __device__ inline int set_band(int k, int first, int stride, int flip)
{
    return first + k * stride + ((k & 1) ? flip : 0);
}

// How the march kernel maps tiles to waves.
enum ScheduleKind : int {
    SCHED_STATIC = 0, SCHED_QUEUE = 1, SCHED_STRIDED = 2, SCHED_XCDROWS = 3, SCHED_RINGS = 4, SCHED_REGIONS = 5
};
// Regions schedule: XCD x (blockIdx % 8) renders the 8x8 tiles
// tiles[off[x] .. off[x+1]) (packed ty << 16 | tx), wave w of its nwx waves
// the tiles w, w + nwx, ...  Built on the host (vr_api.cpp build_regions).
struct TileMap {
    int off[9];
    int nwx;
};
// The regions schedule's lists in device memory: a header of kRegionHeader
// ints, then the list entries.  The header:
//   [0..8]   off[]: XCD x renders the entries [off[x], off[x+1])
//   [9]      tiles with estimated work    [10] the longest list
//   [11]     entries
//   [16..23] marched tiles of XCD x (kRegionWork): its list holds the tiles
//            with estimated work, then the other tiles some ray of which may
//            meet the box, then the empty ones (tile_is_empty) -- those last
//            are written with the uncovered value, not marched
// Built on the host (vr_api.cpp build_regions) or, for a moving camera, on
// the GPU (vr_regions.hip launch_region_build, the same dealing).
constexpr int kRegionHeader = 24;
constexpr int kRegionWork = 16;
struct RegionBuild {
    int tw, th, width, out_rows, band_rows, band_stride, band_first, max_steps;
    int height, band_flip;
    float step_size;
    float org[3], o[3], px[3], py[3], box_min[3], box_max[3];
    float r3[4];           // row 3 of P*V*M (clip w), for tile_is_empty
    double ccx, ccy;       // box-centre tile (fractional), S x S block of it
    int ctx, cty;
    int supertile, wedges;
    int order;             // option region_order: 0 inside-out, 1 longest tile first, 2 longest S x S block first
};
// True when no ray of tile (tx, ty) of the target can be covered (setup_ray,
// vr_march_common.h), so the march would write the uncovered value at every
// pixel of it.  Conservative, in double: the box lies wholly in front of the
// camera (clip w > 0 at its 8 corners: no line through the eye meets it
// behind), and one side plane of the tile's frustum -- through the eye and
// two corner rays of the tile's pixel-edge rectangle, half a pixel outside
// every pixel centre -- has all 8 box corners strictly outside.  The pixel
// centre rays then pass half a pixel or more from any point of the box; the
// fp32 ray setup cannot close that.  Tiles whose rows span two bands (band
// rows not a multiple of 8) are never empty.  Host and GPU list builds.
__host__ __device__ inline bool tile_is_empty(const float org[3], const float o[3], const float px[3], const float py[3],
                                              const float bmin[3], const float bmax[3], const float r3[4], int width,
                                              int out_rows, int height, int band_rows, int band_stride, int band_first,
                                              int band_flip, int tx, int ty)
{
    if (band_rows > 0 && band_rows % 8 != 0) return false;
    const int x0 = tx * 8, x1 = x0 + 8 < width ? x0 + 8 : width;
    const int r0 = ty * 8, rows = r0 + 8 < out_rows ? 8 : out_rows - r0;
    if (x1 <= x0 || rows <= 0) return true;   // no pixels
    int y0 = r0;
    if (band_rows > 0) {
        const int bl = r0 / band_rows;
        y0 = set_band(bl, band_first, band_stride, band_flip) * band_rows + (r0 - bl * band_rows);
    }
    if (y0 >= height) return true;   // rows past the frame: never stored
    double c[8][3];
    for (int k = 0; k < 8; ++k) {
        c[k][0] = (double)((k & 1) ? bmax[0] : bmin[0]) - (double)org[0];
        c[k][1] = (double)((k & 2) ? bmax[1] : bmin[1]) - (double)org[1];
        c[k][2] = (double)((k & 4) ? bmax[2] : bmin[2]) - (double)org[2];
        const double w = (double)r3[0] * (c[k][0] + (double)org[0]) + (double)r3[1] * (c[k][1] + (double)org[1]) +
                         (double)r3[2] * (c[k][2] + (double)org[2]) + (double)r3[3];
        if (!(w > 1e-6)) return false;   // some of the box at or behind the eye
    }
    const double fxs[4] = {(double)x0, (double)x1, (double)x1, (double)x0};
    const double fys[4] = {(double)y0, (double)y0, (double)(y0 + rows), (double)(y0 + rows)};
    double d[4][3], m[3];
    for (int j = 0; j < 3; ++j)
        m[j] = (double)o[j] + 0.5 * (x0 + x1) * (double)px[j] + (y0 + 0.5 * rows) * (double)py[j];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 3; ++j) d[i][j] = (double)o[j] + fxs[i] * (double)px[j] + fys[i] * (double)py[j];
    for (int i = 0; i < 4; ++i) {
        const double* a = d[i];
        const double* b = d[(i + 1) & 3];
        double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double sm = n[0] * m[0] + n[1] * m[1] + n[2] * m[2];
        if (sm == 0.0) continue;
        if (sm > 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }   // outward: away from the tile's centre ray
        const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        bool out = true;
        for (int k = 0; k < 8 && out; ++k) {
            const double cl = sqrt(c[k][0] * c[k][0] + c[k][1] * c[k][1] + c[k][2] * c[k][2]);
            out = n[0] * c[k][0] + n[1] * c[k][1] + n[2] * c[k][2] > 1e-9 * nn * cl;
        }
        if (out) return true;
    }
    return false;
}
size_t region_build_bytes(int ntiles);
hipError_t region_build_preload();   // load the build's code object (first host build, once)
// h_hdr (optional, host-mapped): a copy of the header, for sizing later launches
hipError_t launch_region_build(const RegionBuild& b, void* scratch, unsigned* d_list, int* d_hdr, int* h_hdr,
                               hipStream_t s);

struct Schedule {
    int kind;
    int center_x, center_y;   // rings: target pixel under the projected box centre
    int tiles_per_wave;    // strided: 8x8 tiles per wave
    int waves_per_simd;    // queue: persistent waves per SIMD (grid = 256 CUs x this)
    int* heads;            // queue: 8 device ints, zeroed before each launch
    const unsigned* tiles; // regions: device tile lists
    TileMap map;           // regions (nwx counts waves of split units)
    int split;             // regions: lanes per ray (1, 2, 4, 8; BRICK4 / CORNER8 only)
    int slab;              // regions + COL48: the LDS slab march (vr_march_slab.hip)
    int wg_waves;          // regions (one lane per ray): waves per workgroup, 4 (default), 8 or 16
    const int* hdr;        // regions: the lists' device header (kRegionHeader; off[x] per XCD)
};

// Cost-sort scratch of the procedural march (vr_march.hip launch_march_procedural),
// byte offsets for a target of width x out_rows: the key histogram, the bin
// cursors, the sorted order, the keys per enumerated position, and for the
// deferred shadow passes the per-sorted-wave first entry / first step record
// (proc_scan; waves + 1 entries each) and the frame's totals (need[0] entries,
// need[1] step records).
struct SortLayout {
    size_t hist, cursor, order, keys, went, wrec, need, bytes;
    unsigned waves;   // sorted waves a frame can have: ceil(pixels / 64)
};
SortLayout sort_layout(int width, int out_rows);

// Deferred shadow rays (vr_proc_kernels.h march_proc_defer): device scratch,
// sized from the frame (vr_api.cpp ensure_defer).  Sorted wave w appends at most
// went[w + 1] - went[w] entries (the sum of its lanes' step counts, bounded by
// their cost keys) and marches at most wrec[w + 1] - wrec[w] wave-steps (its
// first lane's key); proc_scan computes both prefixes from the cost histogram.
// A wave whose range lies beyond the capacities marches its shadow rays in
// place (march_pixel_proc) and is skipped by the later passes, so any capacity
// gives the exact frame.
struct ShadowDefer {
    unsigned* count;      // [0]: chunks of 64 entries this frame (written by proc_shadow_scan)
    unsigned* wsteps;     // per sorted wave: wave-steps marched; kDeferInPlace = its shadow rays were marched in place
    unsigned* wcount;     // per sorted wave: entries appended (dense from went[w])
    unsigned* wchunk;     // per sorted wave: its first chunk (exclusive prefix of ceil(wcount / 64))
    uint4* map;           // per chunk: {index of its first entry, 0, entries in it, 0}
    uint4* rec;           // step records {wave-local first entry, lane mask lo, hi, 0}, wave w's from wrec[w]
    float4* ent;          // entries (P, coef), wave w's from went[w]; pass 2 rewrites .xy as (coef, tl)
    const unsigned long long* went;   // sort buffer (SortLayout::went)
    const unsigned* wrec;             // sort buffer (SortLayout::wrec)
    unsigned long long ent_cap;       // entries the scratch holds (< 2^32)
    unsigned rec_cap;                 // step records it holds
    unsigned map_cap;                 // chunk map entries (ent_cap / 64 + waves)
    unsigned waves;                   // sorted waves the per-wave arrays hold
    unsigned eval_blocks;             // workgroups of the shadow pass (0 = kShadowEvalBlocks)
    int worley_cache;                 // shadow pass: keep each lane's Worley cube in registers (option shadow_cache)
};
constexpr unsigned kDeferInPlace = 0xffffffffu;

// launchers (vr_march.hip / vr_volume.hip / vr_paint.hip); return hipError_t
hipError_t launch_march(const MarchArgs& a, int layout, int wrap, bool early, const Schedule& sc, hipStream_t s);
// nf (2 or 4) frames in one regions launch (march_regions_frames; vr_render_pair,
// vr_render_group): the layouts with such a kernel, and the launch -- a is frame 0's
// arguments, fr[k] frame k's per-frame part (the frames differ in nothing else), sc is a
// regions schedule with one lane per ray (no split, no slab, 4-wave workgroups); deal
// (nf = 2 only) 0 = the frame in the wave's parity, 1 = in the workgroup's (vr_march_kernels.h)
constexpr bool pair_layout(int layout) { return list_has(FrameLayouts{}, layout); }
// quad (a QuadMode; other than QUAD_NONE for nf = 4, frames_share_camera(fr, nf) and no step
// counter only): the kernels' QUAD instance, the four frames in the lanes of a quad
// (vr_march_kernels.h regions_frames_body); QUAD_SPLIT, QUAD_STEPS and QUAD_PAIRS for a quad_split_layout only
hipError_t launch_march_frames(const MarchArgs& a, const FrameArgs* fr, int nf, int layout, bool early, const Schedule& sc,
                               int deal, int quad, hipStream_t s);
hipError_t launch_march_frames_cornerh(const MarchArgs& a, const FrameArgs* fr, int nf, bool early, const Schedule& sc,
                                       int deal, int quad, hipStream_t s);   // vr_march_c8.hip
// per-plane byte min (mm[0..3]) and max (mm[4..7]) of the planar volume; mm
// must hold 0xffffffff x 4 then 0 x 4 (atomicMin / atomicMax)
hipError_t launch_plane_minmax(const uint8_t* d_planar, long long total, unsigned* mm, hipStream_t s);
// bytes per pixel of a vr_format (include/vr.h), and the grey format of an RGBA one
__host__ __device__ constexpr int format_bytes(int f) { return f == 0 ? 16 : f <= 2 ? 4 : f <= 4 ? 1 : 4; }
__host__ __device__ constexpr int grey_of(int f) { return f == 0 ? 5 : f == 1 ? 3 : f == 2 ? 4 : -1; }
// grey band sets (1 B or fp32 per pixel) -> RGBA frame rows (vr_assemble_frame)
hipError_t launch_assemble_grey(const uint8_t* d_gathered, size_t rows_per_rank, int nranks, int width, int height,
                                int band_rows, bool f32, int first_rank, uint8_t* d_frame, hipStream_t s,
                                bool serp = false);
hipError_t launch_march_corner8(const MarchArgs& a, int layout, bool early, const Schedule& sc,
                                hipStream_t s);   // CORNER8 / CORNERH, vr_march_c8.hip
// vr_render_rect (vr_march_rect.hip): the frame pixels [x0, x1) x [y0, y1), one wave per 8x8 tile
// anchored at (x0 & ~7, y0 & ~7); tiles_x = the tile columns that spans.  `a` describes the
// whole frame (band_rows = height); the procedural launch needs a.proc.lat == nullptr.
struct RectArgs {
    int x0, y0, x1, y1, tiles_x;
};
RectArgs rect_args(int x, int y, int width, int height);
hipError_t launch_march_rect(const MarchArgs& a, int layout, int wrap, bool early, const RectArgs& rc, hipStream_t s);
hipError_t launch_march_proc_rect(const MarchArgs& a, bool early, const RectArgs& rc, hipStream_t s);
// vr_query_rect (vr_march_query.hip): what the query kernels need beyond MarchArgs and RectArgs, by
// value next to them.  The record of the rectangle's pixel (col, row) is the 64 bytes at
// rec + 4 * (row * pitch + col) (include/vr.h vr_ray_record; pitch in records, >= the rectangle's
// width; rec 16-byte aligned).  limit: the accumulator value the hit search compares with
// (acc_limit's expression, vr_ctx.h acc_limit_of; INFINITY = no search).  `a` as for launch_march_rect,
// with no pixel buffer and no step counter: neither is touched.
struct QueryArgs {
    float4* rec;
    long long pitch;
    float limit;
};
hipError_t launch_march_query(const MarchArgs& a, int layout, int wrap, bool early, const RectArgs& rc, const QueryArgs& q,
                              hipStream_t s);
hipError_t launch_march_proc_query(const MarchArgs& a, bool early, const RectArgs& rc, const QueryArgs& q, hipStream_t s);
// vr_render_rects (vr_march_rect.hip): a list of rectangles in one launch, by value in the
// kernarg segment next to MarchArgs.  Rectangle k is the pixels [e[k][0], e[k][2]) x
// [e[k][1], e[k][3]); its 8x8 tiles are anchored as RectArgs anchors them and numbered
// tile_begin[k] .. tile_begin[k + 1) in row order (tile_begin: the exclusive prefix sum of
// the tile counts, tile_begin[count] = all tiles).  A pixel belongs to the first rectangle
// of the list that holds it.  Every rectangle is non-empty and inside the frame.
constexpr int kMaxRects = 64;   // VR_MAX_RECTS (include/vr.h)
struct RectList {
    int count;
    int pad[3];                        // e[] on a 16-B boundary: one scalar x4 load per rectangle
    int e[kMaxRects][4];               // x0, y0, x1, y1
    unsigned tile_begin[kMaxRects + 1];
};
static_assert(sizeof(MarchArgs) + sizeof(RectList) + 16 <= 4096,
              "MarchArgs and RectList travel together in the 4-KiB kernarg segment");
// Appends a non-empty rectangle inside the frame; false when the list is full.
bool rect_list_add(RectList* rl, int x, int y, int width, int height);
hipError_t launch_march_rects(const MarchArgs& a, int layout, int wrap, bool early, const RectList& rl, hipStream_t s);
hipError_t launch_march_proc_rects(const MarchArgs& a, bool early, const RectList& rl, hipStream_t s);
hipError_t launch_march_slab(const MarchArgs& a, bool early, const Schedule& sc, hipStream_t s);   // vr_march_slab.hip
constexpr int kSlabMaxChunks = 32;   // per channel and wave (64 B each): 8 KiB of LDS per wave
// sort_buf (sort_layout) selects the cost-sorted schedule; null = 8x8
// tiles, in rings when sc.kind == SCHED_RINGS, else in row order
// reuse_sort (vr_api.cpp sort key): SORT_BUILD = sort this frame; SORT_REUSE =
// sort_buf holds the order of a frame with the same geometry (skip the sort
// passes, write the background only); SORT_STALE = the order of an older camera
// with the same target (skip the sort passes, march the pixels it left out too)
enum { SORT_BUILD = 0, SORT_REUSE = 1, SORT_STALE = 2 };
// need_host (optional, host-mapped, 2 entries): a frame that sorts with shadow rays
// writes there the deferred scratch it needs (entries, step records; ensure_defer)
hipError_t launch_march_procedural(const MarchArgs& a, bool early, void* sort_buf, int reuse_sort, const Schedule& sc,
                                   hipStream_t s, const ShadowDefer* defer = nullptr,
                                   unsigned long long* need_host = nullptr);
// blocks of the deferred shadow pass (proc_shadow_eval), at least: a grid-stride loop over
// the chunks (vr_api.cpp ensure_defer sizes the grid from the frame)
constexpr unsigned kShadowEvalBlocks = 256 * 6;
hipError_t launch_repack(const uint8_t* d_rgba, int nx, int ny, int nz, uint8_t* d_planar, hipStream_t s);
// Build a fast layout from the planar planes.
hipError_t launch_build_layout(int layout, const uint8_t* d_planar, int nx, int ny, int nz, uint8_t* d_out,
                               hipStream_t s);
// vr_update_volume: scatter the tightly packed RGBA8 box d_box (bx x by x bz texels at texel
// (x0, y0, z0), inside the volume) into the planar planes, and fold its per-channel byte
// min / max into mm (launch_plane_minmax's layout) with atomicMin / atomicMax
hipError_t launch_update_planar(const uint8_t* d_box, int nx, int ny, int nz, int x0, int y0, int z0, int bx, int by,
                                int bz, uint8_t* d_planar, unsigned* mm, hipStream_t s);
// Rebuild the elements of a fast layout that store a texel of that box, from the (updated)
// planar planes: work and bytes follow the box and its one-position halo.  The default
// build's layouts (CORNERH, CORNER8, BRICK4832, COL48); any other is rebuilt whole.
hipError_t launch_build_layout_box(int layout, const uint8_t* d_planar, int nx, int ny, int nz, uint8_t* d_out,
                                   int x0, int y0, int z0, int bx, int by, int bz, hipStream_t s);
size_t layout_plane_bytes(int layout, int nx, int ny, int nz);
// bytes of all four planes of a fast layout (COL48Z's planes differ in size)
size_t layout_total_bytes(int layout, int nx, int ny, int nz);
hipError_t launch_unpack(const uint8_t* d_planar, int nx, int ny, int nz, uint8_t* d_rgba,
                         hipStream_t s);
// vr_get_volume_box: the planes' texel box (inside the volume) -> tightly packed RGBA8, x fastest
hipError_t launch_unpack_box(const uint8_t* d_planar, int nx, int ny, int nz, int x0, int y0, int z0, int bx, int by,
                             int bz, uint8_t* d_box, hipStream_t s);
// vr_paint: a validated brush (vr.h vr_brush) and its bounding box clipped to the volume (vr_brush.h clip)
struct PaintArgs {
    int nx, ny, nz;
    int o[3], e[3];               // the clipped box: origin and extent (e > 0)
    int d0[3];                    // o - centre: the offset of the box's first texel from the centre, per axis
    int op, falloff;
    unsigned value[4], strength[4];
    unsigned long long s, k[3];   // vr_brush.h Terms of the radii
};
// Blend the brush into the planar planes in place and fold the new bytes' per-channel min / max into mm
hipError_t launch_paint_planar(const PaintArgs& a, uint8_t* d_planar, unsigned* mm, hipStream_t s);
// vr_paint_stroke: the validated dabs that reach the volume, in order, in the kernel arguments (no device
// buffer, no copy).  The work items are the rows (y, z) of the dabs' clipped boxes: the rows of dab i are
// [row_begin[i], row_begin[i + 1]), y fastest.
struct StrokeArgs {
    int nx, ny, nz;
    int count;                              // 1..VR_MAX_DABS
    unsigned row_begin[VR_MAX_DABS + 1];    // <= 64 * 511^2 rows in all
    vr_brush dab[VR_MAX_DABS];              // centres within radius of the volume: offsets fit an int
};
static_assert(sizeof(StrokeArgs) <= 4096, "StrokeArgs travels in the kernarg segment");
// Apply the dabs in order, every texel by one thread (k_paint_stroke), and fold the final bytes' min / max into mm
hipError_t launch_paint_stroke(const StrokeArgs& a, uint8_t* d_planar, unsigned* mm, hipStream_t s);
// vr_blur: `a` is the brush as for launch_paint_planar (op VR_BRUSH_SET; value is not read),
// half_width 1..VR_BLUR_MAX_HALF.  d_stage holds one slab of e[0] x e[1] x e[2] bytes (x fastest) per channel with
// strength != 0, in channel order (blur_stage_bytes).  The stage kernel reads the planes and writes the new byte of
// every inside texel to its slab; the commit kernel stores those bytes to the planes where they differ from the old
// ones and folds them into mm.  Two launches: no byte a mean reads has been written by this call.
size_t blur_stage_bytes(const PaintArgs& a);
hipError_t launch_blur_stage(const PaintArgs& a, int half_width, const uint8_t* d_planar, uint8_t* d_stage, hipStream_t s);
hipError_t launch_blur_commit(const PaintArgs& a, const uint8_t* d_stage, uint8_t* d_planar, unsigned* mm, hipStream_t s);
// vr_morph: launch_blur_stage's contract and slabs with the minimum (op VR_MORPH_ERODE) or
// maximum (VR_MORPH_DILATE) over the cube as the value; launch_blur_commit follows it.
hipError_t launch_morph_stage(const PaintArgs& a, int op, int half_width, const uint8_t* d_planar, uint8_t* d_stage,
                              hipStream_t s);
// vr_rank: launch_blur_stage's contract and slabs with the rank-th smallest byte of the cube
// as the value, rank already resolved to 0..(2 half_width + 1)^3 - 1; launch_blur_commit follows it.
hipError_t launch_rank_stage(const PaintArgs& a, int rank, int half_width, const uint8_t* d_planar, uint8_t* d_stage,
                             hipStream_t s);
// vr_fill (vr_fill.hip): the brush as for launch_paint_planar and the validated rule, whose
// seed lies in the clipped box.  d_labels holds fill_label_bytes(p) bytes, 4-byte aligned: one 32-bit label per texel
// of the box, x fastest.  Three launches in this order on one stream: launch_fill_label writes every label (the
// box-linear index of the smallest member of the texel's component within its 8 x 8 x 8 tile, 0xFFFFFFFF for a texel
// that is not passable) and, with d_report, the empty report; launch_fill_merge joins the components across the
// tiles' faces; launch_fill_commit blends the brush into the planes where a texel's root is the seed's, folds the
// new bytes into mm and, with d_report (a DEVICE vr_fill_report, 8-byte aligned, or null), adds up the report.
// launch_fill_empty_report writes the empty report and nothing else.
struct FillArgs {
    PaintArgs p;
    vr_fill_rule rule;
};
size_t fill_label_bytes(const PaintArgs& p);
hipError_t launch_fill_empty_report(int nx, int ny, int nz, vr_fill_report* d_report, hipStream_t s);
hipError_t launch_fill_label(const FillArgs& a, const uint8_t* d_planar, uint32_t* d_labels, vr_fill_report* d_report,
                             hipStream_t s);
hipError_t launch_fill_merge(const FillArgs& a, uint32_t* d_labels, hipStream_t s);
hipError_t launch_fill_commit(const FillArgs& a, const uint32_t* d_labels, uint8_t* d_planar, unsigned* mm,
                              vr_fill_report* d_report, hipStream_t s);
// vr_clone: the brush as for launch_paint_planar (value is not read) and the validated map.
// launch_clone_direct goes from the planes to the planes in one launch and folds the new bytes into mm: only for a
// map whose source range misses the clipped box on an axis (vr_clone.h direct).  launch_clone_stage has
// launch_blur_stage's contract and slabs; launch_blur_commit follows it.
struct CloneArgs {
    PaintArgs p;
    int offset[3], mirror[3];
};
hipError_t launch_clone_direct(const CloneArgs& a, uint8_t* d_planar, unsigned* mm, hipStream_t s);
hipError_t launch_clone_stage(const CloneArgs& a, const uint8_t* d_planar, uint8_t* d_stage, hipStream_t s);
// vr_stamp: p is the brush over the EDITED box (the clipped box intersected with the placement: o, e and d0 are that
// box's; value is not read); so is the position of the edited box's first texel in the stamp (>= 0), sbx and sby the
// stamp's row and slice pitch in texels.  d_stamp is 4-byte aligned.
struct StampArgs {
    PaintArgs p;
    int so[3];
    int sbx, sby;
};
hipError_t launch_paint_stamp(const StampArgs& a, const uint8_t* d_stamp, uint8_t* d_planar, unsigned* mm, hipStream_t s);
// vr_stamp_affine / vr_clone_affine: the brush as for launch_paint_planar (value is not
// read) and the validated map (vr_affine.h); n is the source's extent in texels -- the stamp's (d_stamp: tightly
// packed RGBA8, 4-byte aligned, each extent 1..32768) or the volume's own.  launch_stamp_affine and
// launch_clone_affine_direct are one launch into the planes and fold the new bytes into mm, the latter only for a
// map whose read range misses the clipped box on an axis (vr_affine.h direct); launch_clone_affine_stage has
// launch_blur_stage's contract and slabs, and launch_blur_commit follows it.
struct AffineArgs {
    PaintArgs p;
    int m[3][3], pivot[3], origin[3];
    int n[3];
    int filter, border;
};
hipError_t launch_stamp_affine(const AffineArgs& a, const uint8_t* d_stamp, uint8_t* d_planar, unsigned* mm, hipStream_t s);
hipError_t launch_clone_affine_direct(const AffineArgs& a, uint8_t* d_planar, unsigned* mm, hipStream_t s);
hipError_t launch_clone_affine_stage(const AffineArgs& a, const uint8_t* d_planar, uint8_t* d_stage, hipStream_t s);
// vr_warp: the brush (op VR_BRUSH_SET; value is not read) and the validated map (vr_warp.h),
// n the volume's own extent.  launch_blur_stage's contract and slabs, and launch_blur_commit follows it.  use_lds
// (option warp_lds): a tile whose read footprint fits the budget stages it in LDS; false = every tile gathers from
// the planes.  Both give the same bytes.
hipError_t launch_warp_stage(const AffineArgs& a, bool use_lds, const uint8_t* d_planar, uint8_t* d_stage, hipStream_t s);
// vr_remap / vr_remap_device: the brush as for launch_paint_planar (value is not read) with
// the value of a texel read from a table at the texel's old byte.  host_lut != null: the table is copied into the
// kernel's arguments during the call (d_lut is not used); host_lut == null: d_lut, a 4-byte aligned DEVICE vr_lut, is
// read when the kernel runs.  One launch, in place; the new bytes are folded into mm.
hipError_t launch_remap(const PaintArgs& a, const vr_lut* host_lut, const void* d_lut, uint8_t* d_planar, unsigned* mm,
                        hipStream_t s);
// vr_stats_lut_device: vr_stats_lut of the DEVICE *d_stats into the DEVICE *d_lut (k_stats_lut, one workgroup); it
// writes the table's 1024 bytes and nothing else
hipError_t launch_stats_lut(const vr_volume_stats* d_stats, int kind, unsigned mask, vr_lut* d_lut, hipStream_t s);
// vr_brush_stats / vr_box_stats: a texel box inside the volume and, for a brush
// (ellipsoid != 0), the ellipsoid as in PaintArgs; for a box d0, s and k are not read.
struct StatsArgs {
    int nx, ny, nz;
    int o[3], e[3];               // the box: origin and extent (e > 0)
    int d0[3];                    // o - centre, per axis
    int ellipsoid, falloff;
    unsigned mask;                // bit c set = channel c is selected
    unsigned long long s, k[3];   // vr_brush.h Terms of the radii
};
// Add the statistics of the box's inside texels to *d_stats (k_stats): the caller has zeroed it on `s`.  Reads the
// planes, writes nothing else.
hipError_t launch_stats(const StatsArgs& a, const uint8_t* d_planar, vr_volume_stats* d_stats, hipStream_t s);
// true for the layouts launch_build_layout_box rebuilds over the box; the others it rebuilds whole
bool layout_rebuilds_box(int layout);
// Perlin lattice table: entry (x, y, z) - lo of n^3 = noise::perlin_lattice_entry(seed, x, y, z)
hipError_t launch_perlin_lattice(uint2* d_out, int seed, int lo, int n, hipStream_t s);
hipError_t launch_noise(int kind, float* d_out, int x0, int y0, int z0, int nx, int ny, int nz,
                        float freq, int32_t seed, float* d_partials, int* num_partials,
                        hipStream_t s);
hipError_t launch_minmax_reduce(const float* d_partials, int num_partials, float* d_minmax,
                                hipStream_t s);
hipError_t launch_pack_recipe(const float* d_g1, const float* d_g2, const float* d_g3,
                              const float* d_g4, const float* d_minmax, long long total,
                              uint8_t* d_rgba, hipStream_t s);
hipError_t launch_assemble(const uint8_t* d_gathered, size_t rows_per_rank, int nranks,
                           int width, int height, int band_rows, int bpp, int first_rank, uint8_t* d_frame,
                           hipStream_t s, bool serp = false);   // serp: vr.h VR_ASSEMBLE_SERPENTINE
int noise_partials_needed(int nx, int ny, int nz);
// 16-B-per-lane grid-stride copy of `bytes` (a multiple of 16): the measured HBM roofline
hipError_t launch_stream_copy(const void* src, void* dst, size_t bytes, hipStream_t s);
// kind 0 = that copy, 1 = a read-only stream (loads folded into a register);
// loads_per_lane 4, 8 or 16 in flight per lane; dst of a read is a 1 KiB sink
hipError_t launch_stream_bw(int kind, int loads_per_lane, const void* src, void* dst, size_t bytes, hipStream_t s);
// variant 0..2 = noise::cell_inv_a..c, 3 = the sequence cellular() uses
hipError_t launch_selftest_cell_inv(int variant, unsigned long long* d_bad, hipStream_t s);
// noise::cellular_table9 (pruned) vs noise::cellular on 2^23 points per seed
hipError_t launch_selftest_worley(int seed, unsigned long long* d_bad, hipStream_t s);

// host camera math (vr_camera.cpp)
struct RayBasis {
    float org[3], o[3], px[3], py[3], r2[4], r3[4];
    // cam_mode 0: CameraPosition is the View eye (to float rounding): org is
    // the camera, o/px/py its pixel-ray directions.  cam_mode 1: org and
    // o/px/py are the View EYE's (they find the rasterised front-face point,
    // vert.glsl:20), cam the box-local CameraPosition the march starts from
    // (frag.glsl:36-38).  DESIGN.md sec. 3.1.
    int cam_mode;
    float cam[3];
};
bool invert4_d(const double* m, double* inv);
bool make_ray_basis(const float* obj48, const float* glob36, int width, int height, RayBasis* b);
void reference_shader_data(float aspect, float phi_deg, float theta_deg, float frame_time,
                           float* obj48, float* glob36);

}  // namespace vr
