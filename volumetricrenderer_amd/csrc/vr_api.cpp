// vr_api.cpp -- implementation of the C ABI declared in include/vr.h.
//
// Owns the device copy of the volume (replaces vkc::Texture3D,
// VulkanTexture.cpp:111-156) and the per-frame uniforms (replaces
// UniformBuffer<T>, VulkanUniformBuffer.h:37-61), and the helpers that turn
// them into the parts of a launch's MarchArgs (plan, ray basis, volume
// buffers).  The render entry points that launch the HIP march kernel -- they
// replace the EnqueueRenderPass + vkCmdDrawIndexed path of
// TestMain.cpp:194-217 -- are in vr_render.cpp.  No exception crosses the ABI;
// errors go through vr_last_error().
//
// The context type and the shared helpers are in vr_ctx.h; the options, the
// region lists / row partition and the procedural scratch live in
// vr_options.cpp, vr_regions_host.cpp and vr_proc_host.cpp; the scissored
// renders in vr_rect.cpp.
#include "vr_blur.h"
#include "vr_brush.h"
#include "vr_affine.h"
#include "vr_warp.h"
#include "vr_clone.h"
#include "vr_ctx.h"
#include "vr_morph.h"
#include "vr_fill.h"
#include "vr_rank.h"
#include "vr_remap.h"
#include "vr_stats.h"

namespace vrapi {

thread_local std::string g_err;

vr_status fail(vr_status st, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return st;
}

// Every extern "C" entry is a function-try-block ending in caught_exception:
// no C++ exception crosses the ABI (vr.h).  A host-side std::bad_alloc (the
// region-list build's vectors, a grown scratch) becomes VR_ERR_OOM, anything
// else VR_ERR_HIP, with the message in vr_last_error().  Called inside a
// catch handler: `throw;` rethrows the exception being handled.
vr_status caught_exception(const char* fn) noexcept
{
    try {
        throw;
    } catch (const std::bad_alloc&) {
        return fail(VR_ERR_OOM, "%s: host allocation failed (std::bad_alloc)", fn);
    } catch (const std::exception& e) {
        return fail(VR_ERR_HIP, "%s: unexpected exception: %s", fn, e.what());
    } catch (...) {
        return fail(VR_ERR_HIP, "%s: unexpected exception", fn);
    }
}


// Auto layout (measured): CORNERH (16 B per texel: one load
// and four v_fma_mix_f32 per tap, no byte conversions, arithmetic index) and
// CORNER8 (8 B per texel, one load per tap) win while the volume fits the
// 256 MiB Infinity Cache; CORNERH is 1.18x / 1.40x faster than CORNER8 at
// 128^3 (1080p x 128 / 4K x 256).  Past that they are HBM-bound, and BRICK4832 (1.53x bytes, 3x7x31
// positions per 4x8x32 brick, BRICK4's two dword-aligned 8-byte loads per tap)
// wins with the pipelined march: 2-5 % ahead of BRICK488 (1.74x) and 12-20 %
// ahead of BRICK4 (2.37x) at 384^3-512^3, level at 200^3-256^3.  Taller bricks
// in y (BRICK41616, slices 64 B apart) lose: a tap's z+1 slice leaves the line.
// COL48 (round 3) drops the z bricks altogether, and is the auto choice.
constexpr size_t kCorner8MaxBytes = 160ull << 20;
int auto_layout(int nx, int ny, int nz)
{
    if (4 * layout_plane_bytes(LAYOUT_CORNERH, nx, ny, nz) <= kCorner8MaxBytes &&
        (long long)(nx + 1) * (ny + 1) * (nz + 1) <= kCornerHMaxPositions)
        return LAYOUT_CORNERH;
    // COL48 = BRICK4832 without z bricks (columns of 3 x 7 positions through the
    // whole z extent): 2-4 % faster at 512^3 in round 3's same-box A/B
    // (profiles/r03/slab_ab_grid512.txt, 0.160-0.163 vs 0.164-0.170 ms).
    return 4 * layout_plane_bytes(LAYOUT_CORNER8, nx, ny, nz) <= kCorner8MaxBytes ? LAYOUT_CORNER8 : LAYOUT_COL48;
}

Ctx* as_ctx(void* p) { return static_cast<Ctx*>(p); }

void free_volume(Ctx* c)
{
    ++c->gen;
    if (c->mm_pending) (void)hipEventSynchronize(c->mm_ready);   // the scan still reads d_planar
    c->mm_pending = false;
    if (c->d_planar) (void)hipFree(c->d_planar);
    if (c->d_fast) (void)hipFree(c->d_fast);
    c->d_planar = c->d_fast = nullptr;
    c->uniform_mask = 0;
    c->fast_layout = 0;
    c->fast_plane_bytes = 0;
    c->nx = c->ny = c->nz = 0;
}

bool dims_ok(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0) return false;
    // widened before the + 2 (INT_MAX + 2 is no int), and one factor at a time: each padded axis is
    // at most 2^31 + 1, so the first product fits 64 bits, and once it is below 2^31 so does the second
    const long long limit = 1ll << 31;   // kernels index a plane with 32-bit ints
    const long long xy = ((long long)nx + 2) * ((long long)ny + 2);
    return xy < limit && xy * ((long long)nz + 2) < limit;
}

int wanted_fast_layout(const Ctx* c)
{
    int want = c->layout_pref == 0 ? auto_layout(c->nx, c->ny, c->nz) : c->layout_pref;
    if (want == LAYOUT_PLANAR) return 0;
    // CORNERH's fp32 index is exact only below 2^24 positions
    if (want == LAYOUT_CORNERH && (long long)(c->nx + 1) * (c->ny + 1) * (c->nz + 1) > kCornerHMaxPositions)
        want = LAYOUT_CORNER8;
    // 32-bit offsets inside the kernels: fall back to PAD16 if too large
    // and LDS offset tables of (nx+ny+nz+3) words: fall back to planar
    if (layout_plane_bytes(want, c->nx, c->ny, c->nz) >= (1ull << 31)) return 0;
    if (want == LAYOUT_COL48Z && layout_plane_bytes(LAYOUT_ZPAIR, c->nx, c->ny, c->nz) >= (1ull << 31)) return 0;
    if ((size_t)(c->nx + c->ny + c->nz + 3) * 4 > 48 * 1024) return 0;
    return want;
}

// (Re)build the fast layout the preference asks for, from the planar planes.
vr_status ensure_fast_layout(Ctx* c, hipStream_t s)
{
    const int want = c->d_planar ? wanted_fast_layout(c) : 0;
    if (want == c->fast_layout) return VR_OK;
    if (c->d_fast) (void)hipFree(c->d_fast);
    c->d_fast = nullptr;
    c->fast_layout = 0;
    c->fast_plane_bytes = 0;
    if (!want) return VR_OK;
    const size_t pb = layout_plane_bytes(want, c->nx, c->ny, c->nz);
    HIP_TRY(hipMalloc(&c->d_fast, layout_total_bytes(want, c->nx, c->ny, c->nz)));
    HIP_TRY(launch_build_layout(want, c->d_planar, c->nx, c->ny, c->nz, c->d_fast, s));
    c->fast_layout = want;
    c->fast_plane_bytes = pb;
    return VR_OK;
}

// Allocate the planes and repack from a device RGBA8 buffer.
vr_status install_volume(Ctx* c, const uint8_t* d_rgba, int nx, int ny, int nz, hipStream_t s)
{
    ++c->gen;
    free_volume(c);
    const size_t total = (size_t)nx * ny * nz;
    HIP_TRY(hipMalloc(&c->d_planar, 4 * total));
    HIP_TRY(launch_repack(d_rgba, nx, ny, nz, c->d_planar, s));
    c->nx = nx; c->ny = ny; c->nz = nz;
    // uniform channels: per-plane byte min / max, once per volume, on `s`;
    // read back into pinned memory and resolved at first use
    if (!c->d_mm) HIP_TRY(hipMalloc(&c->d_mm, 8 * sizeof(unsigned)));
    if (!c->h_mm) HIP_TRY(hipHostMalloc(&c->h_mm, 8 * sizeof(unsigned), hipHostMallocDefault));
    if (!c->mm_ready) HIP_TRY(hipEventCreateWithFlags(&c->mm_ready, hipEventDisableTiming));
    HIP_TRY(hipMemsetAsync(c->d_mm, 0xff, 4 * sizeof(unsigned), s));
    HIP_TRY(hipMemsetAsync(c->d_mm + 4, 0, 4 * sizeof(unsigned), s));
    HIP_TRY(launch_plane_minmax(c->d_planar, (long long)total, c->d_mm, s));
    HIP_TRY(hipMemcpyAsync(c->h_mm, c->d_mm, 8 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(c->mm_ready, s));
    c->mm_pending = true;
    return ensure_fast_layout(c, s);
}

// The uniform channels of the installed volume: waits (once per volume) for
// the install's scan.  vr_render, vr_kernel_variant and vr_get_option call it.
vr_status resolve_uniform(Ctx* c)
{
    if (!c->mm_pending) return VR_OK;
    HIP_TRY(hipEventSynchronize(c->mm_ready));
    c->mm_pending = false;
    ++c->gen;
    c->uniform_mask = 0;
    for (int ch = 0; ch < 4; ++ch)
        if (c->h_mm[ch] == c->h_mm[4 + ch]) {
            c->uniform_mask |= 1 << ch;
            c->uniform_val[ch] = (uint8_t)c->h_mm[ch];
        }
    return VR_OK;
}

// Tap constants of spec v2: tap t samples padded texel
// coordinate g = fma(P, S, T) with S = s_t*N and T = o_t*N + 0.5, where
// o_t = MediaScroll row t * weight_t (frag.glsl:66-69).
void tap_constants(const Ctx* c, float S[4][3], float T[4][3])
{
    const vr_march_params& m = c->march;
    const float* ms = c->glob + 20;  // MediaScroll, column-major; tap t reads row t
    const float dims[3] = {(float)c->nx, (float)c->ny, (float)c->nz};
    for (int t = 0; t < 4; ++t)
        for (int ax = 0; ax < 3; ++ax) {
            const float off = ms[ax * 4 + t] * m.tap_weight[t];
            S[t][ax] = m.tap_scale[t] * dims[ax];
            T[t][ax] = off * dims[ax] + 0.5f;
        }
}

// Is clamp-to-edge identical to mirrored repeat for every tap of every ray?
// Both agree while the base texel floor(g) - 1 stays in [-1, N-1], i.e.
// g in [0, N+1).  Ray points P lie in [0,1]^3 (box entry/exit normalised,
// frag.glsl:49-54) up to rounding drift bounded by `slack`.
bool clamp_is_exact(const Ctx* c, const float S[4][3], const float T[4][3])
{
    const vr_march_params& m = c->march;
    const double slack = (double)(m.max_steps + 16) * 1.2e-7;
    const int dims[3] = {c->nx, c->ny, c->nz};
    for (int t = 0; t < 4; ++t)
        for (int a = 0; a < 3; ++a) {
            const double s = S[t][a], o = T[t][a];
            const double margin = std::fabs(s) * slack + (dims[a] + 2.0) * 2.4e-7 + 1e-6;
            const double lo = std::fmin(o, s + o) - margin, hi = std::fmax(o, s + o) + margin;
            if (!(lo >= 0.0 && hi < dims[a] + 1.0)) return false;
        }
    return true;
}

int band_rows_packed(int height, int band_rows, int band_stride, int band_first, int band_flip)
{
    if (band_rows <= 0) return height;
    if (band_stride <= 0) band_stride = 1;
    const int nb = (height + band_rows - 1) / band_rows;
    if (band_first < 0 || band_first >= nb) return 0;
    int nsel = (nb - 1 - band_first) / band_stride + 1;
    // flipped: the set's bands still increase (|flip| < stride); drop a last
    // odd band the flip pushed past the frame, add one it pulled in
    if (band_flip != 0) {
        while (nsel > 0 && set_band(nsel - 1, band_first, band_stride, band_flip) >= nb) --nsel;
        while (set_band(nsel, band_first, band_stride, band_flip) < nb) ++nsel;
    }
    return nsel * band_rows;
}

vr_status make_plan(Ctx* c, MarchArgs* a, Plan* p)
{
    const vr_march_params& m = c->march;
    tap_constants(c, a->tap_S, a->tap_T);
    a->zero_offsets = 1;
    for (int t = 0; t < 4; ++t)
        for (int k = 0; k < 3; ++k) a->zero_offsets &= a->tap_T[t][k] == 0.5f;
    const bool exact = clamp_is_exact(c, a->tap_S, a->tap_T);
    if (!c->fast_layout) {
        p->layout = LAYOUT_PLANAR;
        p->wrap = exact ? WRAP_CLAMP : WRAP_MIRROR;
    } else if (exact) {
        p->layout = c->fast_layout;
        p->wrap = WRAP_CLAMP;
    } else {
        p->layout = LAYOUT_PLANAR;
        p->wrap = WRAP_MIRROR;
    }
    p->early = m.early_out > 0.0f;
    return VR_OK;
}

// The parts of a launch's MarchArgs that vr_render (vr_render.cpp) and the
// scissored renders (vr_rect.cpp) share; the target's part is target_geometry.
// frame_args: the ray basis of a width x height frame and the march constants;
// false when Projection*View is singular.
bool frame_args(const Ctx* c, int width, int height, MarchArgs* ap)
{
    MarchArgs& a = *ap;
    RayBasis b;
    if (!make_ray_basis(c->obj, c->glob, width, height, &b)) return false;
    std::memcpy(a.org, b.org, sizeof a.org); std::memcpy(a.o, b.o, sizeof a.o);
    std::memcpy(a.px, b.px, sizeof a.px); std::memcpy(a.py, b.py, sizeof a.py);
    std::memcpy(a.r2, b.r2, sizeof a.r2); std::memcpy(a.r3, b.r3, sizeof a.r3);
    a.cam_mode = b.cam_mode;
    std::memcpy(a.cam, b.cam, sizeof a.cam);
    const vr_march_params& m = c->march;
    a.step_size = (1.0f / (float)m.max_steps) * m.step_scale;   // frag.glsl:42
    for (int ax = 0; ax < 3; ++ax) {
        a.box_min[ax] = m.box_min[ax];
        a.box_max[ax] = m.box_max[ax];
        a.box_range[ax] = std::fabs(m.box_max[ax] - m.box_min[ax]);   // :51
    }
    a.density = m.density;
    a.scale = m.scale;
    a.max_steps = m.max_steps;
    a.acc_limit = acc_limit_of(m.early_out, m.density, a.step_size);
    return true;
}

// The procedural medium's parameters and LDS table geometry (after
// frame_args); the Perlin lattice table is the caller's (lat = nullptr here).
void proc_args(const Ctx* c, MarchArgs* ap)
{
    MarchArgs& a = *ap;
    const vr_march_params& m = c->march;
    ProcParams& q = a.proc;
    q.grid_scale = c->proc.grid_scale; q.octaves = c->proc.octaves; q.freq0 = c->proc.freq0;
    q.lacunarity = c->proc.lacunarity; q.gain = c->proc.gain; q.seed_fbm = c->proc.seed_fbm;
    q.worley_freq = c->proc.worley_freq; q.seed_worley = c->proc.seed_worley;
    q.shadow_steps = c->proc.shadow_steps;
    for (int ax = 0; ax < 3; ++ax) q.lstep[ax] = (a.step_size * c->proc.sun_dir[ax]) / a.box_range[ax];
    q.od = a.step_size * m.density;
    q.count_evals = c->count;
    // deferred shadow rays need the sorted schedule and the fixed-geometry tables (vr_render checks);
    // they march the waves in 64x64-region order, like config 2
    q.enum_regions = c->proc_enum || (c->shadow_defer && q.shadow_steps > 0);
    // Worley cell table (LDS): box points P in [0,1]^3 give cellular
    // coordinates in [0, G] per axis, G = grid_scale * worley_freq; the
    // 3x3x3 neighbourhood of rint() of those, with 2 cells of margin.
    const double G = (double)q.grid_scale * (double)q.worley_freq;
    const int lo = (int)std::floor(std::min(0.0, G)) - 2, hi = (int)std::ceil(std::max(0.0, G)) + 2;
    const bool small = std::fabs(G) < 64.0;
    int n = small ? hi - lo + 1 : 0;
    q.wt_fixed = small && n <= 9;   // kernels' fixed geometry (noise::kWorleyN / kWorleyPz)
    if (q.wt_fixed) n = 9;          // a superset of the cells needed
    q.wt_lo = lo;
    q.wt_pz = q.wt_fixed ? 83 : small ? worley_z_pitch(n) : 0;
    q.wt_n = (small && (long long)n * q.wt_pz * 16 <= kMaxWorleyTableBytes) ? n : 0;   // + 8 KiB pairs
    q.lat = nullptr;
}

// The volume buffers of the planned layout.
void volume_args(const Ctx* c, const Plan& pl, MarchArgs* ap)
{
    MarchArgs& a = *ap;
    if (pl.layout != LAYOUT_PLANAR) {
        a.vol = c->d_fast;
        a.plane_stride = (unsigned)c->fast_plane_bytes;
        a.geom = layout_geom(pl.layout, c->nx, c->ny, c->nz);
        if (pl.layout == LAYOUT_COL48Z) {
            a.geom3 = layout_geom(LAYOUT_ZPAIR, c->nx, c->ny, c->nz);
            a.plane3_bytes = (unsigned)layout_plane_bytes(LAYOUT_ZPAIR, c->nx, c->ny, c->nz);
        }
    } else {
        a.vol = c->d_planar;
        a.plane_stride = (unsigned)((size_t)c->nx * c->ny * c->nz);
    }
}

const char* variant_name(const Plan& p)
{
    static const char* names[kNumLayouts][2] = {
        {"none", "none"},
        {"grid_planar_clamp", "grid_planar_clamp_early"},
        {"grid_brick5_clamp", "grid_brick5_clamp_early"},
        {"grid_brick8_clamp", "grid_brick8_clamp_early"},
        {"grid_brick16_clamp", "grid_brick16_clamp_early"},
        {"grid_corner8_clamp", "grid_corner8_clamp_early"},
        {"grid_brick4_clamp", "grid_brick4_clamp_early"},
        {"grid_zpair_clamp", "grid_zpair_clamp_early"},
        {"grid_brick448_clamp", "grid_brick448_clamp_early"},
        {"grid_brick488_clamp", "grid_brick488_clamp_early"},
        {"grid_brick4816_clamp", "grid_brick4816_clamp_early"},
        {"grid_brick41616_clamp", "grid_brick41616_clamp_early"},
        {"grid_brick4832_clamp", "grid_brick4832_clamp_early"},
        {"grid_brick4864_clamp", "grid_brick4864_clamp_early"},
        {"grid_cornerh_clamp", "grid_cornerh_clamp_early"},
        {"grid_col48_clamp", "grid_col48_clamp_early"},
        {"grid_col48z_clamp", "grid_col48z_clamp_early"},
    };
    if (p.layout == LAYOUT_PLANAR && p.wrap == WRAP_MIRROR)
        return p.early ? "grid_planar_mirror_early" : "grid_planar_mirror";
    return names[p.layout][p.early ? 1 : 0];
}

}  // namespace vrapi

using namespace vrapi;

extern "C" {

const char* vr_last_error(void) { return g_err.c_str(); }
int vr_abi_version(void) { return VR_ABI_VERSION; }

vr_status vr_march_defaults(vr_march_params* m)
try {
    if (!m) return fail(VR_ERR_INVALID, "vr_march_defaults: null");
    std::memset(m, 0, sizeof *m);
    m->max_steps = 128;        // frag.glsl:30
    m->step_scale = 4.0f;      // :42
    m->density = 1.0f;         // :29
    m->scale = 0.2f;           // :63
    for (int a = 0; a < 3; ++a) { m->box_min[a] = -1.0f; m->box_max[a] = 1.0f; }  // :31-32
    const float ts[4] = {1.0f, 0.8f, 0.75f, 0.7f}, tw[4] = {0.0f, 0.2f, 0.25f, 0.3f};  // :66-69
    for (int t = 0; t < 4; ++t) { m->tap_scale[t] = ts[t]; m->tap_weight[t] = tw[t]; }
    m->early_out = 0.0f;
    return VR_OK;
} catch (...) {
    return caught_exception("vr_march_defaults");
}

vr_status vr_volume_recipe_defaults(vr_volume_recipe* r)
try {
    if (!r) return fail(VR_ERR_INVALID, "vr_volume_recipe_defaults: null");
    r->size = 128;  // TestMain.cpp:51
    const float f[4] = {0.01f, 0.03f, 0.19f, 0.15f};  // :59-62
    for (int k = 0; k < 4; ++k) { r->freq[k] = f[k]; r->seed[k] = k + 1; }
    r->literal_overwrite = 1;
    return VR_OK;
} catch (...) {
    return caught_exception("vr_volume_recipe_defaults");
}

vr_status vr_create(int device, void** out)
try {
    if (!out) return fail(VR_ERR_INVALID, "vr_create: out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(VR_ERR_NO_DEVICE, "vr_create: no HIP device");
    if (device < 0 || device >= n) return fail(VR_ERR_NO_DEVICE, "vr_create: device %d of %d", device, n);
    HIP_TRY(hipSetDevice(device));
    Ctx* c = new (std::nothrow) Ctx();
    if (!c) return fail(VR_ERR_OOM, "vr_create: host allocation failed");
    c->device = device;
    vr_march_defaults(&c->march);
    if (hipMalloc(&c->d_heads, 64) != hipSuccess) {
        delete c;
        return fail(VR_ERR_OOM, "vr_create: queue heads");
    }
    *out = c;
    return VR_OK;
} catch (...) {
    return caught_exception("vr_create");
}

vr_status vr_destroy(void* p)
try {
    if (!p) return VR_OK;
    Ctx* c = as_ctx(p);
    (void)hipSetDevice(c->device);
    free_volume(c);
    if (c->d_heads) (void)hipFree(c->d_heads);
    if (c->d_sort) (void)hipFree(c->d_sort);
    (void)hipDeviceSynchronize();   // queued renders may still read the region lists and the scratch
    if (c->d_blur) (void)hipFree(c->d_blur);
    for (const auto& ds : c->defer_sets)
        if (ds.d) (void)hipFree(ds.d);
    for (const auto& q : c->defer_retired) {
        (void)hipFree(q.p);
        if (q.ev) (void)hipEventDestroy(q.ev);
    }
    if (c->h_need) (void)hipHostFree(c->h_need);
    if (c->need_ev) (void)hipEventDestroy(c->need_ev);
    if (c->d_lat) (void)hipFree(c->d_lat);
    if (c->d_rg) (void)hipFree(c->d_rg);
    if (c->h_rghdr) (void)hipHostFree(c->h_rghdr);
    if (c->rg_ev) (void)hipEventDestroy(c->rg_ev);
    for (auto& u : c->proc_uses) (void)hipEventDestroy(u.ev);
    if (c->proc_wev) (void)hipEventDestroy(c->proc_wev);
    if (c->d_mm) (void)hipFree(c->d_mm);
    if (c->h_mm) (void)hipHostFree(c->h_mm);
    if (c->mm_ready) (void)hipEventDestroy(c->mm_ready);
    for (auto& b : c->region) {
        if (b.d) (void)hipFree(b.d);
        if (b.h) (void)hipHostFree(b.h);
        for (hipEvent_t e : b.used)
            if (e) (void)hipEventDestroy(e);
        if (b.uploaded) (void)hipEventDestroy(b.uploaded);
    }
    delete c;
    return VR_OK;
} catch (...) {
    return caught_exception("vr_destroy");
}

vr_status vr_set_volume(void* p, const uint8_t* rgba8, int nx, int ny, int nz)
try {
    if (!p || !rgba8) return fail(VR_ERR_INVALID, "vr_set_volume: null argument");  // VulkanTexture.cpp:121-124
    if (!dims_ok(nx, ny, nz)) return fail(VR_ERR_INVALID, "vr_set_volume: bad extent %dx%dx%d", nx, ny, nz);
    Ctx* c = as_ctx(p);
    ++c->gen;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)nx * ny * nz * 4;
    uint8_t* staging = nullptr;
    HIP_TRY(hipMalloc(&staging, bytes));
    hipError_t e = hipMemcpy(staging, rgba8, bytes, hipMemcpyHostToDevice);
    vr_status st = VR_OK;
    if (e == hipSuccess) st = install_volume(c, staging, nx, ny, nz, nullptr);
    if (e == hipSuccess && st == VR_OK) e = hipDeviceSynchronize();
    (void)hipFree(staging);
    if (st != VR_OK) return st;
    if (e != hipSuccess) return fail(VR_ERR_HIP, "vr_set_volume: %s", hipGetErrorString(e));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_set_volume");
}

vr_status vr_set_volume_device(void* p, const void* d_rgba8, int nx, int ny, int nz, void* stream)
try {
    if (!p || !d_rgba8) return fail(VR_ERR_INVALID, "vr_set_volume_device: null argument");
    if (!dims_ok(nx, ny, nz)) return fail(VR_ERR_INVALID, "vr_set_volume_device: bad extent %dx%dx%d", nx, ny, nz);
    Ctx* c = as_ctx(p);
    ++c->gen;
    HIP_TRY(hipSetDevice(c->device));
    return install_volume(c, static_cast<const uint8_t*>(d_rgba8), nx, ny, nz, static_cast<hipStream_t>(stream));
} catch (...) {
    return caught_exception("vr_set_volume_device");
}

}  // extern "C"

namespace vrapi {

// The argument checks of vr_update_volume / vr_update_volume_device: a refused
// call has touched nothing.
static vr_status check_update(const char* fn, void* p, const void* data, int x0, int y0, int z0, int bx, int by, int bz)
{
    if (!p || !data) return fail(VR_ERR_INVALID, "%s: null argument", fn);
    if (bx <= 0 || by <= 0 || bz <= 0) return fail(VR_ERR_INVALID, "%s: bad box extent %dx%dx%d", fn, bx, by, bz);
    const Ctx* c = as_ctx(p);
    if (!c->d_planar) return fail(VR_ERR_NO_VOLUME, "%s: no volume set", fn);
    if (x0 < 0 || y0 < 0 || z0 < 0 || bx > c->nx - x0 || by > c->ny - y0 || bz > c->nz - z0)
        return fail(VR_ERR_INVALID, "%s: box %dx%dx%d at (%d, %d, %d) leaves the %dx%dx%d volume", fn, bx, by, bz, x0,
                    y0, z0, c->nx, c->ny, c->nz);
    return VR_OK;
}

// What follows a kernel that has rewritten texels of the box in the planes and
// folded their byte range into d_mm (the update's scatter, the brush), on `s`:
// launches only, no allocation, no host wait.  The held fast layout is rebuilt
// over the box.  A uniform channel (uniform_mask, which the _uX kernels sample
// as a constant) can only be lost: while some channel is uniform, or the
// install's scan is still unresolved, the read-back is re-armed and the next
// render / vr_kernel_variant / vr_get_option resolves it as after an install.
// With no uniform channel left nothing can change: no read-back, no `gen`
// bump, and the cached launches stay valid (same buffers, same geometry).
//
// The two halves, for an edit of several boxes (vr_paint_stroke): the rebuild
// once per box, the re-armed read-back once after them.
static vr_status rebuild_box(Ctx* c, int x0, int y0, int z0, int bx, int by, int bz, hipStream_t s)
{
    if (c->fast_layout)
        HIP_TRY(launch_build_layout_box(c->fast_layout, c->d_planar, c->nx, c->ny, c->nz, c->d_fast, x0, y0, z0, bx,
                                        by, bz, s));
    return VR_OK;
}

static vr_status rearm_minmax(Ctx* c, hipStream_t s)
{
    if (c->mm_pending || c->uniform_mask != 0) {
        HIP_TRY(hipMemcpyAsync(c->h_mm, c->d_mm, 8 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(c->mm_ready, s));
        c->mm_pending = true;
    }
    return VR_OK;
}

static vr_status box_edited(Ctx* c, int x0, int y0, int z0, int bx, int by, int bz, hipStream_t s)
{
    if (vr_status st = rebuild_box(c, x0, y0, z0, bx, by, bz, s)) return st;
    return rearm_minmax(c, s);
}

// The layout rebuilds of a stroke: the dabs' clipped boxes coalesced to at most kStrokeRebuilds boxes
// (a diagonal stroke's bounding box is far larger than its dabs, and a rebuild per dab repeats the shared
// bricks).  The rebuild reads the planes, so boxes that overlap are correct.  A layout that is rebuilt
// whole whatever the box (VR_EXPERIMENTS) gets one box.
constexpr int kStrokeRebuilds = 8;
static vr_status stroke_edited(Ctx* c, const vr_box* boxes, int count, hipStream_t s)
{
    if (c->fast_layout) {
        vr_box merged[kStrokeRebuilds];
        int n = 0;
        if (vr_status st = vr_boxes_coalesce(boxes, count, layout_rebuilds_box(c->fast_layout) ? kStrokeRebuilds : 1,
                                             merged, &n))
            return st;
        for (int k = 0; k < n; ++k)
            if (vr_status st = rebuild_box(c, merged[k].x, merged[k].y, merged[k].z, merged[k].bx, merged[k].by,
                                           merged[k].bz, s))
                return st;
    }
    return rearm_minmax(c, s);
}

// Patch the planes (the scatter folds the box's byte range into d_mm) and the held fast layout on `s`.
static vr_status update_volume_device(Ctx* c, const uint8_t* d_box, int x0, int y0, int z0, int bx, int by, int bz,
                                      hipStream_t s)
{
    HIP_TRY(launch_update_planar(d_box, c->nx, c->ny, c->nz, x0, y0, z0, bx, by, bz, c->d_planar, c->d_mm, s));
    return box_edited(c, x0, y0, z0, bx, by, bz, s);
}

// vr_blur's staging scratch.  A queued blur may still use the held buffer, hence the device sync before it is freed.
vr_status release_blur(Ctx* c)
{
    if (!c->d_blur) return VR_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    (void)hipFree(c->d_blur);
    c->d_blur = nullptr;
    c->blur_bytes = 0;
    return VR_OK;
}

vr_status ensure_blur(Ctx* c, size_t need)
{
    if (need <= c->blur_bytes) return VR_OK;
    if (vr_status st = release_blur(c)) return st;
    HIP_TRY(hipSetDevice(c->device));
    const size_t mib = (size_t)1 << 20, bytes = (need + mib - 1) / mib * mib;
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VR_ERR_OOM, "vr_blur: %zu bytes of staging scratch", bytes);
    }
    c->d_blur = static_cast<uint8_t*>(d);
    c->blur_bytes = bytes;
    return VR_OK;
}

// What a brush or the statistics need of the context: an installed volume that the frames read.
static vr_status check_target(const char* fn, const Ctx* c)
{
    if (!c->d_planar) return fail(VR_ERR_NO_VOLUME, "%s: no volume set", fn);
    if (c->proc.enabled) return fail(VR_ERR_NO_VOLUME, "%s: a procedural medium is enabled (it reads no volume)", fn);
    return VR_OK;
}

// The ellipsoid of a validated vr_brush over the box a.o, a.e of the volume: the fields PaintArgs and StatsArgs share.
template <class Args>
static void brush_geometry(const Ctx* c, const vr_brush* b, Args& a)
{
    a.nx = c->nx; a.ny = c->ny; a.nz = c->nz;
    const vr::brush::Terms t = vr::brush::terms(b->radius);
    a.s = t.s;
    for (int ax = 0; ax < 3; ++ax) {
        a.d0[ax] = (int)((long long)a.o[ax] - b->centre[ax]);   // within the radius of 0
        a.k[ax] = t.k[ax];
    }
    a.falloff = b->falloff;
}

// The brush of a validated vr_brush over the box a.o, a.e of the volume; false when every strength is 0 -- nothing
// would be read or written.
static bool source_brush_args(const Ctx* c, const vr_brush* b, PaintArgs& a)
{
    brush_geometry(c, b, a);
    a.op = b->op;
    bool any = false;
    for (int ch = 0; ch < 4; ++ch) {
        a.value[ch] = b->value[ch];
        a.strength[ch] = b->strength[ch];
        any = any || b->strength[ch] != 0;
    }
    return any;
}

// The staged brushes (blur, morph, rank, and the clone whose source overlaps its box): the scratch (grown only when
// the call needs more than is held), the caller's stage launch from the planes to the scratch, k_blur_commit from
// the scratch to the planes, and what follows an edit of the clipped box.  Some strength of `a` is not 0.
// stage_name is the launcher stage() calls, for the text of a failed launch.
template <class Stage>
static vr_status staged_brush(Ctx* c, const PaintArgs& a, hipStream_t s, const char* stage_name, Stage stage)
{
    if (vr_status st = ensure_blur(c, blur_stage_bytes(a))) return st;
    HIP_TRY(hipSetDevice(c->device));
    if (const hipError_t e = stage())
        return fail(e == hipErrorOutOfMemory ? VR_ERR_OOM : VR_ERR_HIP, "%s: %s (%s:%d)", stage_name, hipGetErrorString(e),
                    __FILE__, __LINE__);
    HIP_TRY(launch_blur_commit(a, c->d_blur, c->d_planar, c->d_mm, s));
    return box_edited(c, a.o[0], a.o[1], a.o[2], a.e[0], a.e[1], a.e[2], s);
}

}  // namespace vrapi

extern "C" {

vr_status vr_update_volume(void* p, const uint8_t* rgba8, int x0, int y0, int z0, int bx, int by, int bz)
try {
    if (vr_status st = check_update("vr_update_volume", p, rgba8, x0, y0, z0, bx, by, bz)) return st;
    Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)bx * by * bz * 4;
    uint8_t* staging = nullptr;   // the box, not the volume
    HIP_TRY(hipMalloc(&staging, bytes));
    hipError_t e = hipMemcpy(staging, rgba8, bytes, hipMemcpyHostToDevice);
    vr_status st = VR_OK;
    if (e == hipSuccess) st = update_volume_device(c, staging, x0, y0, z0, bx, by, bz, nullptr);
    if (e == hipSuccess && st == VR_OK) e = hipDeviceSynchronize();
    (void)hipFree(staging);
    if (st != VR_OK) return st;
    if (e != hipSuccess) return fail(VR_ERR_HIP, "vr_update_volume: %s", hipGetErrorString(e));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_update_volume");
}

vr_status vr_update_volume_device(void* p, const void* d_rgba8, int x0, int y0, int z0, int bx, int by, int bz,
                                  void* stream)
try {
    if (vr_status st = check_update("vr_update_volume_device", p, d_rgba8, x0, y0, z0, bx, by, bz)) return st;
    Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    return update_volume_device(c, static_cast<const uint8_t*>(d_rgba8), x0, y0, z0, bx, by, bz,
                                static_cast<hipStream_t>(stream));
} catch (...) {
    return caught_exception("vr_update_volume_device");
}

int vr_volume_extent_ok(int nx, int ny, int nz) { return dims_ok(nx, ny, nz) ? 1 : 0; }

vr_status vr_volume_dims(void* p, int* nx, int* ny, int* nz)
try {
    if (!p || !nx || !ny || !nz) return fail(VR_ERR_INVALID, "vr_volume_dims: null argument");
    Ctx* c = as_ctx(p);
    *nx = c->nx; *ny = c->ny; *nz = c->nz;
    return VR_OK;
} catch (...) {
    return caught_exception("vr_volume_dims");
}

vr_status vr_get_volume(void* p, uint8_t* out)
try {
    if (!p || !out) return fail(VR_ERR_INVALID, "vr_get_volume: null argument");
    Ctx* c = as_ctx(p);
    if (!c->d_planar) return fail(VR_ERR_NO_VOLUME, "vr_get_volume: no volume set");
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->nx * c->ny * c->nz * 4;
    uint8_t* staging = nullptr;
    HIP_TRY(hipMalloc(&staging, bytes));
    hipError_t e = launch_unpack(c->d_planar, c->nx, c->ny, c->nz, staging, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, staging, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(staging);
    if (e != hipSuccess) return fail(VR_ERR_HIP, "vr_get_volume: %s", hipGetErrorString(e));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_get_volume");
}

vr_status vr_get_volume_box(void* p, int x0, int y0, int z0, int bx, int by, int bz, uint8_t* out)
try {
    if (vr_status st = check_update("vr_get_volume_box", p, out, x0, y0, z0, bx, by, bz)) return st;
    Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)bx * by * bz * 4;
    uint8_t* staging = nullptr;   // the box, not the volume
    HIP_TRY(hipMalloc(&staging, bytes));
    hipError_t e = launch_unpack_box(c->d_planar, c->nx, c->ny, c->nz, x0, y0, z0, bx, by, bz, staging, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, staging, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(staging);
    if (e != hipSuccess) return fail(VR_ERR_HIP, "vr_get_volume_box: %s", hipGetErrorString(e));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_get_volume_box");
}

vr_status vr_get_volume_box_device(void* p, int x0, int y0, int z0, int bx, int by, int bz, void* d_out, void* stream)
try {
    if (vr_status st = check_update("vr_get_volume_box_device", p, d_out, x0, y0, z0, bx, by, bz)) return st;
    Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_unpack_box(c->d_planar, c->nx, c->ny, c->nz, x0, y0, z0, bx, by, bz, static_cast<uint8_t*>(d_out),
                              static_cast<hipStream_t>(stream)));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_get_volume_box_device");
}

// The brush on the device: k_paint_planar over the clipped bounding box, then what follows an update of that box.
// A brush whose strengths are all 0 launches too: the kernel stores nothing, and the box counts as edited.
vr_status vr_paint(void* p, const vr_brush* b, void* stream)
try {
    if (!p || !b) return fail(VR_ERR_INVALID, "vr_paint: null argument");
    if (const char* why = vr::brush::invalid(b)) return fail(VR_ERR_INVALID, "vr_paint: %s", why);
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_paint", c)) return st;
    PaintArgs a{};
    if (!vr::brush::clip(b, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // the brush misses the volume
    (void)source_brush_args(c, b, a);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(launch_paint_planar(a, c->d_planar, c->d_mm, s));
    return box_edited(c, a.o[0], a.o[1], a.o[2], a.e[0], a.e[1], a.e[2], s);
} catch (...) {
    return caught_exception("vr_paint");
}

// A stroke on the device: every check first (a refused call has launched nothing), then k_paint_stroke over
// the dabs that reach the volume -- they travel in its arguments -- and what follows an edit of their boxes.
vr_status vr_paint_stroke(void* p, const vr_brush* dabs, int count, void* stream)
try {
    if (!p) return fail(VR_ERR_INVALID, "vr_paint_stroke: null ctx");
    if (count < 0 || count > VR_MAX_DABS)
        return fail(VR_ERR_INVALID, "vr_paint_stroke: count %d (0..%d)", count, VR_MAX_DABS);
    if (count == 0) return VR_OK;
    if (!dabs) return fail(VR_ERR_INVALID, "vr_paint_stroke: null dabs with count %d", count);
    for (int i = 0; i < count; ++i)
        if (const char* why = vr::brush::invalid(&dabs[i])) return fail(VR_ERR_INVALID, "vr_paint_stroke: dab %d: %s", i, why);
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_paint_stroke", c)) return st;
    StrokeArgs a{};
    vr_box boxes[VR_MAX_DABS];
    a.nx = c->nx; a.ny = c->ny; a.nz = c->nz;
    for (int i = 0; i < count; ++i) {
        int o[3], e[3];
        if (!vr::brush::clip(&dabs[i], c->nx, c->ny, c->nz, o, e)) continue;   // the dab misses the volume
        a.dab[a.count] = dabs[i];
        boxes[a.count] = vr_box{o[0], o[1], o[2], e[0], e[1], e[2]};
        a.row_begin[a.count + 1] = a.row_begin[a.count] + (unsigned)e[1] * (unsigned)e[2];
        ++a.count;
    }
    if (a.count == 0) return VR_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(launch_paint_stroke(a, c->d_planar, c->d_mm, s));
    return stroke_edited(c, boxes, a.count, s);
} catch (...) {
    return caught_exception("vr_paint_stroke");
}

// The smoothing brush on the device: every check first, then the staged sequence with k_blur_stage as its first
// launch.
vr_status vr_blur(void* p, const vr_brush* b, int half_width, void* stream)
try {
    if (!p || !b) return fail(VR_ERR_INVALID, "vr_blur: null argument");
    if (const char* why = vr::blur::invalid(b, half_width)) return fail(VR_ERR_INVALID, "vr_blur: %s", why);
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_blur", c)) return st;
    PaintArgs a{};
    if (!vr::brush::clip(b, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // the brush misses the volume
    if (!source_brush_args(c, b, a)) return VR_OK;                          // every strength is 0
    a.op = VR_BRUSH_SET;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return staged_brush(c, a, s, "launch_blur_stage", [&] { return launch_blur_stage(a, half_width, c->d_planar, c->d_blur, s); });
} catch (...) {
    return caught_exception("vr_blur");
}

// The erode / dilate brush on the device: vr_blur's sequence with k_morph_stage as the first launch.  The staging
// scratch is the blur's (same need, same growth rule, same option).
vr_status vr_morph(void* p, const vr_brush* b, int op, int half_width, void* stream)
try {
    if (!p || !b) return fail(VR_ERR_INVALID, "vr_morph: null argument");
    if (const char* why = vr::morph::invalid(b, op, half_width)) return fail(VR_ERR_INVALID, "vr_morph: %s", why);
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_morph", c)) return st;
    PaintArgs a{};
    if (!vr::brush::clip(b, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // the brush misses the volume
    if (!source_brush_args(c, b, a)) return VR_OK;                          // every strength is 0
    a.op = VR_BRUSH_SET;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return staged_brush(c, a, s, "launch_morph_stage", [&] { return launch_morph_stage(a, op, half_width, c->d_planar, c->d_blur, s); });
} catch (...) {
    return caught_exception("vr_morph");
}

// The median / rank-filter brush on the device: vr_morph's sequence with k_rank_stage as the first launch.  The
// staging scratch is the blur's (same need, same growth rule, same option).
vr_status vr_rank(void* p, const vr_brush* b, int rank, int half_width, void* stream)
try {
    if (!p || !b) return fail(VR_ERR_INVALID, "vr_rank: null argument");
    if (const char* why = vr::rank::invalid(b, rank, half_width)) return fail(VR_ERR_INVALID, "vr_rank: %s", why);
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_rank", c)) return st;
    PaintArgs a{};
    if (!vr::brush::clip(b, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // the brush misses the volume
    if (!source_brush_args(c, b, a)) return VR_OK;                          // every strength is 0
    hipStream_t s = static_cast<hipStream_t>(stream);
    return staged_brush(c, a, s, "launch_rank_stage", [&] {
        return launch_rank_stage(a, vr::rank::resolve(rank, half_width), half_width, c->d_planar, c->d_blur, s);
    });
} catch (...) {
    return caught_exception("vr_rank");
}

// The flood-fill brush on the device: every check first (a refused call has launched nothing), then the labels in
// the family's scratch (4 bytes per texel of the clipped box; same growth rule, same option), the three launches of
// vr_fill.hip and what follows an edit of the clipped box.  A brush that misses the volume and a seed outside the
// clipped box give the empty report and nothing else; with every strength 0 the call is a measurement: it runs for
// the report alone, and without one it launches nothing.
vr_status vr_fill(void* p, const vr_brush* b, const vr_fill_rule* rule, vr_fill_report* d_report, void* stream)
try {
    if (!p || !b || !rule) return fail(VR_ERR_INVALID, "vr_fill: null argument");
    if (const char* why = vr::fill::invalid(b, rule)) return fail(VR_ERR_INVALID, "vr_fill: %s", why);
    if ((reinterpret_cast<uintptr_t>(d_report) & 7u) != 0u) return fail(VR_ERR_INVALID, "vr_fill: d_report is not 8-byte aligned");
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_fill", c)) return st;
    if (const char* why = vr::fill::invalid_seed(rule, c->nx, c->ny, c->nz)) return fail(VR_ERR_INVALID, "vr_fill: %s", why);
    FillArgs a{};
    a.rule = *rule;
    hipStream_t s = static_cast<hipStream_t>(stream);
    bool reached = vr::brush::clip(b, c->nx, c->ny, c->nz, a.p.o, a.p.e);
    for (int ax = 0; ax < 3; ++ax) reached = reached && rule->seed[ax] >= a.p.o[ax] && rule->seed[ax] - a.p.o[ax] < a.p.e[ax];
    if (!reached) {   // the brush misses the volume, or the seed lies outside its clipped box: the region is empty
        if (!d_report) return VR_OK;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(launch_fill_empty_report(c->nx, c->ny, c->nz, d_report, s));
        return VR_OK;
    }
    const bool paints = source_brush_args(c, b, a.p);
    if (!paints && !d_report) return VR_OK;   // nothing to write and nobody to tell
    if (vr_status st = ensure_blur(c, fill_label_bytes(a.p))) return st;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t* labels = reinterpret_cast<uint32_t*>(c->d_blur);
    HIP_TRY(launch_fill_label(a, c->d_planar, labels, d_report, s));
    HIP_TRY(launch_fill_merge(a, labels, s));
    HIP_TRY(launch_fill_commit(a, labels, c->d_planar, c->d_mm, d_report, s));
    if (!paints) return VR_OK;                // a measurement: no byte was written
    return box_edited(c, a.p.o[0], a.p.o[1], a.p.o[2], a.p.e[0], a.p.e[1], a.p.e[2], s);
} catch (...) {
    return caught_exception("vr_fill");
}

// The clone brush on the device: every check first, then the host picks the path in integers (vr_clone.h direct).
// Direct: one launch from the planes to the planes, then what follows an edit of the box.  Staged: the staged
// sequence with k_clone_stage as its first launch.
vr_status vr_clone(void* p, const vr_brush* b, const vr_clone_map* m, void* stream)
try {
    if (!p || !b || !m) return fail(VR_ERR_INVALID, "vr_clone: null argument");
    if (const char* why = vr::clone::invalid(b, m)) return fail(VR_ERR_INVALID, "vr_clone: %s", why);
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_clone", c)) return st;
    CloneArgs g{};
    PaintArgs& a = g.p;
    if (!vr::brush::clip(b, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // the brush misses the volume
    if (!source_brush_args(c, b, a)) return VR_OK;                          // every strength is 0
    for (int ax = 0; ax < 3; ++ax) { g.offset[ax] = m->offset[ax]; g.mirror[ax] = m->mirror[ax]; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!vr::clone::direct(m, a.o, a.e, c->nx, c->ny, c->nz))
        return staged_brush(c, a, s, "launch_clone_stage", [&] { return launch_clone_stage(g, c->d_planar, c->d_blur, s); });
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_clone_direct(g, c->d_planar, c->d_mm, s));
    return box_edited(c, a.o[0], a.o[1], a.o[2], a.e[0], a.e[1], a.e[2], s);
} catch (...) {
    return caught_exception("vr_clone");
}

// The stamp brush on the device: every check first, then k_paint_stamp over the edited box (the clipped box
// intersected with the placement) and what follows an edit of that box.
vr_status vr_stamp(void* p, const vr_brush* b, const void* d_rgba8, const vr_box* placement, void* stream)
try {
    if (!p || !b || !d_rgba8 || !placement) return fail(VR_ERR_INVALID, "vr_stamp: null argument");
    if (const char* why = vr::stamp::invalid(b, placement)) return fail(VR_ERR_INVALID, "vr_stamp: %s", why);
    if ((reinterpret_cast<uintptr_t>(d_rgba8) & 3u) != 0u) return fail(VR_ERR_INVALID, "vr_stamp: d_rgba8 is not 4-byte aligned");
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_stamp", c)) return st;
    StampArgs g{};
    PaintArgs& a = g.p;
    if (!vr::stamp::clip(b, placement, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // nothing under brush and stamp
    if (!source_brush_args(c, b, a)) return VR_OK;                                     // every strength is 0
    const long long p0[3] = {placement->x, placement->y, placement->z};
    for (int ax = 0; ax < 3; ++ax) g.so[ax] = (int)((long long)a.o[ax] - p0[ax]);   // 0 <= so < the stamp's extent
    g.sbx = placement->bx;
    g.sby = placement->by;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(launch_paint_stamp(g, static_cast<const uint8_t*>(d_rgba8), c->d_planar, c->d_mm, s));
    return box_edited(c, a.o[0], a.o[1], a.o[2], a.e[0], a.e[1], a.e[2], s);
} catch (...) {
    return caught_exception("vr_stamp");
}

// The transform paste on the device (vr_affine.h): what both calls share of the validated map.
static void affine_args(const vr_affine* m, int snx, int sny, int snz, AffineArgs& g)
{
    for (int ax = 0; ax < 3; ++ax) {
        for (int k = 0; k < 3; ++k) g.m[ax][k] = m->m[ax][k];
        g.pivot[ax] = m->pivot[ax];
        g.origin[ax] = m->origin[ax];
    }
    g.n[0] = snx; g.n[1] = sny; g.n[2] = snz;
    g.filter = m->filter;
    g.border = m->border;
}

// vr_stamp_affine: every check first, then k_stamp_affine over the brush's clipped box and what follows an edit of
// that box.
vr_status vr_stamp_affine(void* p, const vr_brush* b, const void* d_rgba8, int sbx, int sby, int sbz, const vr_affine* m,
                          void* stream)
try {
    if (!p || !b || !d_rgba8 || !m) return fail(VR_ERR_INVALID, "vr_stamp_affine: null argument");
    if (const char* why = vr::affine::invalid(b, m)) return fail(VR_ERR_INVALID, "vr_stamp_affine: %s", why);
    if (const char* why = vr::affine::invalid_extent(sbx, sby, sbz)) return fail(VR_ERR_INVALID, "vr_stamp_affine: %s", why);
    if ((reinterpret_cast<uintptr_t>(d_rgba8) & 3u) != 0u) return fail(VR_ERR_INVALID, "vr_stamp_affine: d_rgba8 is not 4-byte aligned");
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_stamp_affine", c)) return st;
    AffineArgs g{};
    PaintArgs& a = g.p;
    if (!vr::brush::clip(b, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // the brush misses the volume
    if (!source_brush_args(c, b, a)) return VR_OK;                          // every strength is 0
    affine_args(m, sbx, sby, sbz, g);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(launch_stamp_affine(g, static_cast<const uint8_t*>(d_rgba8), c->d_planar, c->d_mm, s));
    return box_edited(c, a.o[0], a.o[1], a.o[2], a.e[0], a.e[1], a.e[2], s);
} catch (...) {
    return caught_exception("vr_stamp_affine");
}

// vr_clone_affine: every check first, then the host picks the path in integers (vr_affine.h direct), as vr_clone.
vr_status vr_clone_affine(void* p, const vr_brush* b, const vr_affine* m, void* stream)
try {
    if (!p || !b || !m) return fail(VR_ERR_INVALID, "vr_clone_affine: null argument");
    if (const char* why = vr::affine::invalid(b, m)) return fail(VR_ERR_INVALID, "vr_clone_affine: %s", why);
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_clone_affine", c)) return st;
    AffineArgs g{};
    PaintArgs& a = g.p;
    if (!vr::brush::clip(b, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // the brush misses the volume
    if (!source_brush_args(c, b, a)) return VR_OK;                          // every strength is 0
    affine_args(m, c->nx, c->ny, c->nz, g);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!vr::affine::direct(m, a.o, a.e, c->nx, c->ny, c->nz))
        return staged_brush(c, a, s, "launch_clone_affine_stage", [&] { return launch_clone_affine_stage(g, c->d_planar, c->d_blur, s); });
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_clone_affine_direct(g, c->d_planar, c->d_mm, s));
    return box_edited(c, a.o[0], a.o[1], a.o[2], a.e[0], a.e[1], a.e[2], s);
} catch (...) {
    return caught_exception("vr_clone_affine");
}

// The liquify brush on the device (vr_warp.h): every check first, then always the staged sequence -- a soft warp reads
// texels that it writes -- with k_warp_stage as its first launch.
vr_status vr_warp(void* p, const vr_brush* b, const vr_affine* m, void* stream)
try {
    if (!p || !b || !m) return fail(VR_ERR_INVALID, "vr_warp: null argument");
    if (const char* why = vr::warp::invalid(b, m)) return fail(VR_ERR_INVALID, "vr_warp: %s", why);
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target("vr_warp", c)) return st;
    AffineArgs g{};
    PaintArgs& a = g.p;
    if (!vr::brush::clip(b, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // the brush misses the volume
    if (!source_brush_args(c, b, a)) return VR_OK;                          // every strength is 0
    affine_args(m, c->nx, c->ny, c->nz, g);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return staged_brush(c, a, s, "launch_warp_stage", [&] { return launch_warp_stage(g, c->warp_lds != 0, c->d_planar, c->d_blur, s); });
} catch (...) {
    return caught_exception("vr_warp");
}

// The lookup-table brush on the device: every check first, then k_remap over the clipped box -- with the host table
// in the kernel's arguments (lut) or the caller's device table (d_lut) -- and what follows an edit of that box.
static vr_status remap_brush(const char* fn, void* p, const vr_brush* b, const vr_lut* lut, const void* d_lut, void* stream)
{
    if (!p || !b || (!lut && !d_lut)) return fail(VR_ERR_INVALID, "%s: null argument", fn);
    if (const char* why = vr::brush::invalid(b)) return fail(VR_ERR_INVALID, "%s: %s", fn, why);
    if (!lut && (reinterpret_cast<uintptr_t>(d_lut) & 3u) != 0u) return fail(VR_ERR_INVALID, "%s: d_lut is not 4-byte aligned", fn);
    Ctx* c = as_ctx(p);
    if (vr_status st = check_target(fn, c)) return st;
    PaintArgs a{};
    if (!vr::brush::clip(b, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // the brush misses the volume
    if (!source_brush_args(c, b, a)) return VR_OK;                          // every strength is 0
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(launch_remap(a, lut, d_lut, c->d_planar, c->d_mm, s));
    return box_edited(c, a.o[0], a.o[1], a.o[2], a.e[0], a.e[1], a.e[2], s);
}

vr_status vr_remap(void* p, const vr_brush* b, const vr_lut* lut, void* stream)
try {
    return remap_brush("vr_remap", p, b, lut, nullptr, stream);
} catch (...) {
    return caught_exception("vr_remap");
}

vr_status vr_remap_device(void* p, const vr_brush* b, const void* d_lut, void* stream)
try {
    return remap_brush("vr_remap_device", p, b, nullptr, d_lut, stream);
} catch (...) {
    return caught_exception("vr_remap_device");
}

// vr_stats_lut on the device: the context names the device and nothing else of it is used -- no volume is needed
// and a procedural medium may be enabled.
vr_status vr_stats_lut_device(void* p, const void* d_stats, int kind, int channel_mask, void* d_lut, void* stream)
try {
    if (!p || !d_stats || !d_lut) return fail(VR_ERR_INVALID, "vr_stats_lut_device: null argument");
    if (const char* why = vr::remap::invalid_kind(kind)) return fail(VR_ERR_INVALID, "vr_stats_lut_device: %s", why);
    if (const char* why = vr::remap::invalid_mask(channel_mask)) return fail(VR_ERR_INVALID, "vr_stats_lut_device: %s", why);
    if ((reinterpret_cast<uintptr_t>(d_stats) & 7u) != 0u) return fail(VR_ERR_INVALID, "vr_stats_lut_device: d_stats is not 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_lut) & 3u) != 0u) return fail(VR_ERR_INVALID, "vr_stats_lut_device: d_lut is not 4-byte aligned");
    const Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_stats_lut(static_cast<const vr_volume_stats*>(d_stats), kind, (unsigned)channel_mask,
                             static_cast<vr_lut*>(d_lut), static_cast<hipStream_t>(stream)));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_stats_lut_device");
}

// The statistics under a brush or in a box: every check first (a refused call writes nothing), then the buffer is
// zeroed on the stream and k_stats adds to it.  It reads c->d_planar and touches nothing else of the context.
static vr_status stats_target(const char* fn, const Ctx* c, const void* d_stats)
{
    if (((uintptr_t)d_stats & 7u) != 0) return fail(VR_ERR_INVALID, "%s: d_stats is not 8-byte aligned", fn);
    return check_target(fn, c);
}

vr_status vr_brush_stats(void* p, const vr_brush* b, void* d_stats, void* stream)
try {
    if (!p || !b || !d_stats) return fail(VR_ERR_INVALID, "vr_brush_stats: null argument");
    if (const char* why = vr::brush::invalid(b)) return fail(VR_ERR_INVALID, "vr_brush_stats: %s", why);
    Ctx* c = as_ctx(p);
    if (vr_status st = stats_target("vr_brush_stats", c, d_stats)) return st;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(vr_volume_stats), s));
    StatsArgs a{};
    if (!vr::brush::clip(b, c->nx, c->ny, c->nz, a.o, a.e)) return VR_OK;   // the brush misses the volume: all zero
    brush_geometry(c, b, a);
    a.ellipsoid = 1;
    a.mask = vr::stats::brush_mask(b->strength);
    HIP_TRY(launch_stats(a, c->d_planar, static_cast<vr_volume_stats*>(d_stats), s));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_brush_stats");
}

vr_status vr_box_stats(void* p, int x0, int y0, int z0, int bx, int by, int bz, int channel_mask, void* d_stats,
                       void* stream)
try {
    if (!p || !d_stats) return fail(VR_ERR_INVALID, "vr_box_stats: null argument");
    if (const char* why = vr::stats::invalid_mask(channel_mask)) return fail(VR_ERR_INVALID, "vr_box_stats: %s", why);
    Ctx* c = as_ctx(p);
    if (vr_status st = stats_target("vr_box_stats", c, d_stats)) return st;
    if (vr_status st = check_update("vr_box_stats", p, d_stats, x0, y0, z0, bx, by, bz)) return st;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(vr_volume_stats), s));
    StatsArgs a{};
    a.nx = c->nx; a.ny = c->ny; a.nz = c->nz;
    a.o[0] = x0; a.o[1] = y0; a.o[2] = z0;
    a.e[0] = bx; a.e[1] = by; a.e[2] = bz;
    a.mask = (unsigned)channel_mask;   // ellipsoid = 0: every texel of the box, weight 256
    HIP_TRY(launch_stats(a, c->d_planar, static_cast<vr_volume_stats*>(d_stats), s));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_box_stats");
}

vr_status vr_noise_grid(void* p, int kind, void* d_out, int x0, int y0, int z0, int nx, int ny, int nz,
                        float freq, int32_t seed, float* out_min, float* out_max, void* stream)
try {
    if (!p) return fail(VR_ERR_INVALID, "vr_noise_grid: null ctx");
    if (kind < 0 || kind > 2) return fail(VR_ERR_INVALID, "vr_noise_grid: kind %d", kind);
    if (nx <= 0 || ny <= 0 || nz <= 0) return fail(VR_ERR_INVALID, "vr_noise_grid: bad extent");
    Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int np = noise_partials_needed(nx, ny, nz);
    float* part = nullptr;
    float* mm = nullptr;
    HIP_TRY(hipMalloc(&part, (size_t)np * 2 * sizeof(float)));
    hipError_t e = hipMalloc(&mm, 2 * sizeof(float));
    int used = 0;
    if (e == hipSuccess) e = launch_noise(kind, static_cast<float*>(d_out), x0, y0, z0, nx, ny, nz, freq, seed, part, &used, s);
    if (e == hipSuccess) e = launch_minmax_reduce(part, used, mm, s);
    float h[2] = {0.f, 0.f};
    if (e == hipSuccess) e = hipMemcpyAsync(h, mm, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(part);
    if (mm) (void)hipFree(mm);
    if (e != hipSuccess) return fail(VR_ERR_HIP, "vr_noise_grid: %s", hipGetErrorString(e));
    if (out_min) *out_min = h[0];
    if (out_max) *out_max = h[1];
    return VR_OK;
} catch (...) {
    return caught_exception("vr_noise_grid");
}

vr_status vr_selftest(void* p, const char* name, long long* failures)
try {
    if (!p || !name || !failures) return fail(VR_ERR_INVALID, "vr_selftest: null argument");
    static const char* const kNames[] = {"cell_inv_a", "cell_inv_b", "cell_inv_c", "cell_inv", "worley_prune"};
    int variant = -1;
    for (int i = 0; i < 5; ++i)
        if (std::strcmp(name, kNames[i]) == 0) variant = i;
    if (variant < 0) return fail(VR_ERR_INVALID, "vr_selftest: unknown test '%s'", name);
    Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc(&d, sizeof *d));
    unsigned long long h = 0;
    hipError_t e = hipMemset(d, 0, sizeof *d);
    if (variant == 4) {   // three seeds, the recipe's Worley seed among them
        for (int seed : {2, 1337, -987654321})
            if (e == hipSuccess) e = launch_selftest_worley(seed, d, nullptr);
    } else if (e == hipSuccess) {
        e = launch_selftest_cell_inv(variant, d, nullptr);
    }
    if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(VR_ERR_HIP, "vr_selftest: %s", hipGetErrorString(e));
    *failures = (long long)h;
    return VR_OK;
} catch (...) {
    return caught_exception("vr_selftest");
}

vr_status vr_measure_bandwidth(void* p, int kind, int loads_per_lane, size_t bytes, int reps, void* stream,
                               double* gbs_best, double* gbs_median, int* loads_best)
try {
    if (!p || !gbs_best || reps <= 0 || bytes < 16 || (kind != VR_BW_COPY && kind != VR_BW_READ) ||
        (loads_per_lane != 0 && loads_per_lane != 4 && loads_per_lane != 8 && loads_per_lane != 16))
        return fail(VR_ERR_INVALID, "vr_measure_bandwidth: bad argument");
    Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    bytes &= ~(size_t)15;
    const std::vector<int> pls = loads_per_lane ? std::vector<int>{loads_per_lane} : std::vector<int>{4, 8, 16};
    const size_t dst_bytes = kind == VR_BW_COPY ? bytes : 1024;   // a read's 1 KiB sink is never written
    const size_t nev = 2 * (size_t)reps * pls.size();
    void *src = nullptr, *dst = nullptr;
    std::vector<hipEvent_t> ev(nev, nullptr);
    hipError_t e = hipMalloc(&src, bytes);
    if (e == hipSuccess) e = hipMalloc(&dst, dst_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(src, 0x5a, bytes, s);
    for (auto& v : ev)
        if (e == hipSuccess) e = hipEventCreate(&v);
    // warm-up (page mapping, clocks), then the timed reps, interleaved over the widths
    for (int pl : pls)
        if (e == hipSuccess) e = launch_stream_bw(kind, pl, src, dst, bytes, s);
    for (int i = 0; i < reps && e == hipSuccess; ++i)
        for (size_t j = 0; j < pls.size() && e == hipSuccess; ++j) {
            const size_t k = 2 * (i * pls.size() + j);
            e = hipEventRecord(ev[k], s);
            if (e == hipSuccess) e = launch_stream_bw(kind, pls[j], src, dst, bytes, s);
            if (e == hipSuccess) e = hipEventRecord(ev[k + 1], s);
        }
    std::vector<std::pair<double, int>> gbs;
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const double moved = (kind == VR_BW_COPY ? 2.0 : 1.0) * (double)bytes;
    for (int i = 0; i < reps && e == hipSuccess; ++i)
        for (size_t j = 0; j < pls.size() && e == hipSuccess; ++j) {
            const size_t k = 2 * (i * pls.size() + j);
            float ms = 0.0f;
            e = hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
            if (e == hipSuccess && ms > 0.0f) gbs.push_back({moved / (ms * 1e-3) / 1e9, pls[j]});
        }
    for (auto& v : ev)
        if (v) (void)hipEventDestroy(v);
    if (src) (void)hipFree(src);
    if (dst) (void)hipFree(dst);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? VR_ERR_OOM : VR_ERR_HIP, "vr_measure_bandwidth: %s",
                                     hipGetErrorString(e));
    if (gbs.empty()) return fail(VR_ERR_HIP, "vr_measure_bandwidth: no timing");
    std::sort(gbs.begin(), gbs.end());
    *gbs_best = gbs.back().first;
    if (loads_best) *loads_best = gbs.back().second;
    if (gbs_median) {   // the median rep of the best width
        std::vector<double> w;
        for (const auto& g : gbs)
            if (g.second == gbs.back().second) w.push_back(g.first);
        *gbs_median = w[w.size() / 2];
    }
    return VR_OK;
} catch (...) {
    return caught_exception("vr_measure_bandwidth");
}

vr_status vr_measure_copy_bandwidth(void* p, size_t bytes, int reps, void* stream, double* gbs_best, double* gbs_median)
try {
    return vr_measure_bandwidth(p, VR_BW_COPY, 4, bytes, reps, stream, gbs_best, gbs_median, nullptr);
} catch (...) {
    return caught_exception("vr_measure_copy_bandwidth");
}

vr_status vr_generate_volume(void* p, const vr_volume_recipe* r, void* stream)
try {
    if (!p || !r) return fail(VR_ERR_INVALID, "vr_generate_volume: null argument");
    const int N = r->size;
    if (!dims_ok(N, N, N)) return fail(VR_ERR_INVALID, "vr_generate_volume: bad size %d", N);
    Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t total = (size_t)N * N * N;
    const int np = noise_partials_needed(N, N, N);
    float *g1 = nullptr, *g2 = nullptr, *g3 = nullptr, *g4 = nullptr, *part = nullptr, *mm = nullptr;
    uint8_t* rgba = nullptr;
    hipError_t e = hipSuccess;
    auto alloc = [&](void** ptr, size_t bytes) { if (e == hipSuccess) e = hipMalloc(ptr, bytes); };
    alloc((void**)&g1, total * sizeof(float));
    if (!r->literal_overwrite) alloc((void**)&g2, total * sizeof(float));
    alloc((void**)&g3, total * sizeof(float));
    alloc((void**)&g4, total * sizeof(float));
    alloc((void**)&part, (size_t)np * 2 * sizeof(float));
    alloc((void**)&mm, 8 * sizeof(float));
    alloc((void**)&rgba, total * 4);
    int used = 0;
    // TestMain.cpp:59-62.  Literal recipe: run 1's values are overwritten by
    // run 2 (both target noiseOutput1), so run 1 only yields its min/max.
    float* outs[4] = {r->literal_overwrite ? nullptr : g1, r->literal_overwrite ? g1 : g2, g3, g4};
    const int kinds[4] = {0, 0, 1, 2};
    for (int k = 0; k < 4 && e == hipSuccess; ++k) {
        e = launch_noise(kinds[k], outs[k], 0, 0, 0, N, N, N, r->freq[k], r->seed[k], part, &used, s);
        if (e == hipSuccess) e = launch_minmax_reduce(part, used, mm + 2 * k, s);
    }
    if (e == hipSuccess) e = launch_pack_recipe(g1, g2, g3, g4, mm, (long long)total, rgba, s);
    vr_status st = VR_OK;
    if (e == hipSuccess) st = install_volume(c, rgba, N, N, N, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    for (void* q : {(void*)g1, (void*)g2, (void*)g3, (void*)g4, (void*)part, (void*)mm, (void*)rgba})
        if (q) (void)hipFree(q);
    if (st != VR_OK) return st;
    if (e != hipSuccess) {
        free_volume(c);
        return fail(e == hipErrorOutOfMemory ? VR_ERR_OOM : VR_ERR_HIP, "vr_generate_volume: %s", hipGetErrorString(e));
    }
    return VR_OK;
} catch (...) {
    return caught_exception("vr_generate_volume");
}

vr_status vr_set_shader_data(void* p, const vr_object_shader_data* osd, const vr_global_shader_data* gsd)
try {
    if (!p || !osd || !gsd) return fail(VR_ERR_INVALID, "vr_set_shader_data: null argument");
    Ctx* c = as_ctx(p);
    ++c->gen;
    std::memcpy(c->obj, osd, sizeof(float) * 48);
    std::memcpy(c->glob, gsd, sizeof(float) * 36);
    RayBasis b;
    if (!make_ray_basis(c->obj, c->glob, 16, 16, &b)) {
        c->has_camera = false;
        return fail(VR_ERR_INVALID, "vr_set_shader_data: Projection*View is singular");
    }
    c->has_camera = true;
    return VR_OK;
} catch (...) {
    return caught_exception("vr_set_shader_data");
}

vr_status vr_reference_shader_data(float aspect, float phi_deg, float theta_deg, float frame_time,
                                   vr_object_shader_data* osd, vr_global_shader_data* gsd)
try {
    if (!osd || !gsd) return fail(VR_ERR_INVALID, "vr_reference_shader_data: null argument");
    if (!(aspect > 0.0f)) return fail(VR_ERR_INVALID, "vr_reference_shader_data: aspect must be > 0");
    reference_shader_data(aspect, phi_deg, theta_deg, frame_time, reinterpret_cast<float*>(osd),
                          reinterpret_cast<float*>(gsd));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_reference_shader_data");
}

vr_status vr_set_march(void* p, const vr_march_params* m)
try {
    if (!p || !m) return fail(VR_ERR_INVALID, "vr_set_march: null argument");
    if (m->max_steps <= 0) return fail(VR_ERR_INVALID, "vr_set_march: max_steps must be > 0");
    if (!(m->step_scale > 0.0f) || !std::isfinite(m->step_scale))
        return fail(VR_ERR_INVALID, "vr_set_march: step_scale must be finite and > 0");
    if (!(m->early_out >= 0.0f && m->early_out < 1.0f)) return fail(VR_ERR_INVALID, "vr_set_march: early_out in [0,1)");
    if (m->early_out > 0.0f && !(m->density > 0.0f))
        return fail(VR_ERR_INVALID, "vr_set_march: early_out needs density > 0");
    for (int a = 0; a < 3; ++a)
        if (!(m->box_max[a] != m->box_min[a])) return fail(VR_ERR_INVALID, "vr_set_march: empty box on axis %d", a);
    if (m->reserved[0] || m->reserved[1] || m->reserved[2]) return fail(VR_ERR_INVALID, "vr_set_march: reserved must be 0");
    as_ctx(p)->march = *m;
    ++as_ctx(p)->gen;
    return VR_OK;
} catch (...) {
    return caught_exception("vr_set_march");
}

int vr_band_rows_packed(int height, int band_rows, int band_stride, int band_first, int band_flip)
try {
    if (band_flip != 0 && (band_rows <= 0 || band_stride < 2 || std::abs(band_flip) >= band_stride)) return -1;
    return band_rows_packed(height, band_rows, band_stride, band_first, band_flip);
} catch (...) {
    (void)caught_exception("vr_band_rows_packed");
    return -1;
}


vr_status vr_assemble_frame(void* p, const void* d_gathered, int gathered_format, size_t rows_per_rank, int nranks,
                            int width, int height, int band_rows, int frame_format, void* d_frame, void* stream)
try {
    return vr_assemble_frame_ranks(p, d_gathered, gathered_format, rows_per_rank, nranks, 0, width, height, band_rows,
                                   frame_format, d_frame, stream);
} catch (...) {
    return caught_exception("vr_assemble_frame");
}

vr_status vr_assemble_frame_ranks(void* p, const void* d_gathered, int gathered_format, size_t rows_per_rank,
                                  int nranks, int first_rank, int width, int height, int band_rows, int frame_format,
                                  void* d_frame, void* stream)
try {
    if (!p || !d_gathered || !d_frame) return fail(VR_ERR_INVALID, "vr_assemble_frame: null argument");
    if (first_rank < 0 || first_rank > nranks) return fail(VR_ERR_INVALID, "vr_assemble_frame: first_rank %d", first_rank);
    if (first_rank == nranks) return VR_OK;   // every rank's rows are in place
    if (nranks > 0 && rows_per_rank > (size_t)(INT_MAX / nranks))   // the kernels index rows in 32 bits
        return fail(VR_ERR_INVALID, "vr_assemble_frame: rows_per_rank %zu x %d ranks", rows_per_rank, nranks);
    const bool serp = (frame_format & VR_ASSEMBLE_SERPENTINE) != 0;
    frame_format &= ~VR_ASSEMBLE_SERPENTINE;
    if (gathered_format < 0 || gathered_format > 5 || frame_format < 0 || frame_format > 5)
        return fail(VR_ERR_INVALID, "vr_assemble_frame: bad format %d -> %d", gathered_format, frame_format);
    if (gathered_format != frame_format && grey_of(frame_format) != gathered_format)
        return fail(VR_ERR_INVALID, "vr_assemble_frame: format %d does not expand into %d", gathered_format,
                    frame_format);
    if (nranks <= 0 || width <= 0 || height <= 0 || band_rows <= 0)
        return fail(VR_ERR_INVALID, "vr_assemble_frame: bad geometry");
    for (int r = first_rank; r < nranks; ++r)
        if ((size_t)band_rows_packed(height, band_rows, nranks, r, serp ? nranks - 1 - 2 * r : 0) > rows_per_rank)
            return fail(VR_ERR_INVALID, "vr_assemble_frame: rows_per_rank %zu too small for rank %d", rows_per_rank, r);
    Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    if (gathered_format == frame_format) {
        HIP_TRY(launch_assemble(static_cast<const uint8_t*>(d_gathered), rows_per_rank, nranks, width, height,
                                band_rows, format_bytes(frame_format), first_rank, static_cast<uint8_t*>(d_frame),
                                static_cast<hipStream_t>(stream), serp));
        return VR_OK;
    }
    HIP_TRY(launch_assemble_grey(static_cast<const uint8_t*>(d_gathered), rows_per_rank, nranks, width, height,
                                 band_rows, frame_format == VR_FMT_RGBA32F, first_rank, static_cast<uint8_t*>(d_frame),
                                 static_cast<hipStream_t>(stream), serp));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_assemble_frame_ranks");
}

vr_status vr_assemble_bands(void* p, const void* d_gathered, size_t rows_per_rank, int nranks, int width,
                            int height, int band_rows, int bytes_per_pixel, void* d_frame, void* stream)
try {
    if (!p || !d_gathered || !d_frame) return fail(VR_ERR_INVALID, "vr_assemble_bands: null argument");
    if (nranks <= 0 || width <= 0 || height <= 0 || band_rows <= 0 ||
        (bytes_per_pixel != 1 && bytes_per_pixel != 4 && bytes_per_pixel != 16))
        return fail(VR_ERR_INVALID, "vr_assemble_bands: bad geometry");
    for (int r = 0; r < nranks; ++r)
        if ((size_t)band_rows_packed(height, band_rows, nranks, r) > rows_per_rank)
            return fail(VR_ERR_INVALID, "vr_assemble_bands: rows_per_rank %zu too small for rank %d", rows_per_rank, r);
    Ctx* c = as_ctx(p);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_assemble(static_cast<const uint8_t*>(d_gathered), rows_per_rank, nranks, width, height,
                            band_rows, bytes_per_pixel, 0, static_cast<uint8_t*>(d_frame),
                            static_cast<hipStream_t>(stream)));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_assemble_bands");
}

}  // extern "C"
