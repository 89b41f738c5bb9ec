// vr_render.cpp -- the whole-frame render entry points of the C ABI: vr_render,
// vr_render_sequence, vr_render_pair and vr_render_group (include/vr.h).
//
// A grid frame goes from a vr_target to a launch in named steps, which
// vr_render and render_frames (vr_render_pair, vr_render_group) call:
//   check_target -> honour_inject_throw -> cache_hit, or else
//   grid_frame_args -> attach_regions (regions schedule) -> launch_frame,
// where launch_frame remembers a planned frame in the launch cache.  A
// procedural frame gets its arguments here and is run by render_procedural
// (vr_proc_host.cpp).  The target checks and geometry are shared with the
// scissored renders of vr_rect.cpp.
#include "vr_ctx.h"

namespace vrapi {

vr_status check_frame_state(const char* fn, const Ctx* c, const vr_target* t)
{
    if (!c->d_planar && !c->proc.enabled)
        return fail(VR_ERR_NO_VOLUME, "%s: no volume (vr_set_volume / vr_generate_volume)", fn);
    if (!c->has_camera) return fail(VR_ERR_NO_CAMERA, "%s: no shader data (vr_set_shader_data)", fn);
    if (t->width <= 0 || t->height <= 0) return fail(VR_ERR_INVALID, "%s: bad size %dx%d", fn, t->width, t->height);
    return VR_OK;
}

vr_status check_pixels(const char* fn, const vr_target* t, int format, size_t* pitch)
{
    if (!t->pixels) return fail(VR_ERR_INVALID, "%s: pixels is null", fn);
    const int bpp = format_bytes(format);
    *pitch = t->row_pitch ? t->row_pitch : (size_t)t->width * bpp;
    if (*pitch < (size_t)t->width * bpp || *pitch % bpp != 0 || ((uintptr_t)t->pixels % bpp) != 0)
        return fail(VR_ERR_INVALID, "%s: pitch/alignment (pitch %zu, bpp %d)", fn, *pitch, bpp);
    return VR_OK;
}

vr_status check_target(const char* fn, const Ctx* c, const vr_target* t, TargetInfo* ti)
{
    if (const vr_status st = check_frame_state(fn, c, t)) return st;
    ti->format = t->format & ~(VR_TARGET_BANDS_IN_PLACE | VR_TARGET_ROW_RANGE);
    ti->in_place = (t->format & VR_TARGET_BANDS_IN_PLACE) != 0;
    ti->row_range = (t->format & VR_TARGET_ROW_RANGE) != 0;
    if (ti->format < 0 || ti->format > 5) return fail(VR_ERR_INVALID, "%s: bad format %d", fn, t->format);
    if (const vr_status st = check_pixels(fn, t, ti->format, &ti->pitch)) return st;
    if (t->band_rows < 0 || (t->band_rows > 0 && (t->band_stride <= 0 || t->band_first < 0)))
        return fail(VR_ERR_INVALID, "%s: bad band selection", fn);
    if (ti->row_range && (t->band_rows <= 0 || t->band_stride != 1 || t->band_first % 8 != 0))
        return fail(VR_ERR_INVALID, "%s: bad row range (rows %d, stride %d, first row %d: need rows > 0, "
                    "stride 1, first a multiple of 8)", fn, t->band_rows, t->band_stride, t->band_first);
    if (t->band_flip != 0 &&
        (ti->row_range || t->band_rows <= 0 || t->band_stride < 2 || std::abs(t->band_flip) >= t->band_stride))
        return fail(VR_ERR_INVALID, "%s: band_flip %d needs a band set with |flip| < stride (%d)", fn, t->band_flip,
                    t->band_stride);
    if (t->reserved != 0) return fail(VR_ERR_INVALID, "%s: vr_target.reserved must be 0", fn);
    return VR_OK;
}

void target_geometry(const vr_target* t, const TargetInfo& ti, MarchArgs* ap)
{
    MarchArgs& a = *ap;
    a.width = t->width;
    a.height = t->height;
    if (ti.row_range) {
        // rows [first, first + n) = the 8-row bands from first / 8 on, cut at n
        // rows: the kernels' band-row mapping as it is
        a.band_rows = 8; a.band_stride = 1; a.band_first = t->band_first / 8;
    } else if (t->band_rows > 0) {
        a.band_rows = t->band_rows; a.band_stride = t->band_stride; a.band_first = t->band_first;
        a.band_flip = t->band_flip;
    } else {
        a.band_rows = t->height; a.band_stride = 1; a.band_first = 0;
    }
    a.out_rows = band_rows_packed(t->height, a.band_rows, a.band_stride, a.band_first, a.band_flip);
    if (ti.row_range) a.out_rows = std::min(a.out_rows, t->band_rows);
    a.tiles_x = (t->width + 15) / 16;
    a.tiles_y = (a.out_rows + 15) / 16;
    a.num_blocks = 8 * ((a.tiles_y + 7) / 8) * a.tiles_x;
    a.out = t->pixels;
    a.pitch = (long long)ti.pitch;
    a.format = ti.format;
    a.bands_in_place = ti.in_place && (t->band_rows > 0 || ti.row_range) ? 1 : 0;
    a.step_counter = reinterpret_cast<unsigned long long*>(t->step_counter);
}

void honour_inject_throw(Ctx* c)
{
    if (!c->inject_throw) return;
    const int k = c->inject_throw;
    c->inject_throw = 0;
    if (k == 2) throw std::bad_alloc();
    throw std::runtime_error("injected by vr option inject_throw");
}

vr_status frame_march_args(const char* fn, Ctx* c, const vr_target* t, const TargetInfo& ti, MarchArgs* a, Plan* pl)
{
    if (!frame_args(c, t->width, t->height, a)) return fail(VR_ERR_INVALID, "%s: Projection*View is singular", fn);
    *pl = Plan{LAYOUT_PLANAR, WRAP_CLAMP, c->march.early_out > 0.0f};
    if (c->proc.enabled) proc_args(c, a);   // no lattice table: the fBm hashes every corner
    else make_plan(c, a, pl);
    a->nx = c->nx; a->ny = c->ny; a->nz = c->nz;
    volume_args(c, *pl, a);
    target_geometry(t, ti, a);
    return VR_OK;
}

}  // namespace vrapi

using namespace vrapi;

namespace {

// ---- the launch cache (Ctx::lc)

const Ctx::Cached* cached_frame(const Ctx* c, const vr_target* t, hipStream_t hs, unsigned long long gen)
{
    for (const Ctx::Cached& e : c->lc)
        if (e.valid && e.gen == gen && e.stream == hs && std::memcmp(&e.t, t, sizeof *t) == 0) return &e;
    return nullptr;
}

// `gen`: the context's when the frame was planned
void remember_frame(Ctx* c, const vr_target* t, hipStream_t hs, unsigned long long gen, const GridFrame& f)
{
    if (!c->launch_cache) return;
    Ctx::Cached& e = c->lc[c->lc_next];
    c->lc_next = (c->lc_next + 1) % (int)(sizeof c->lc / sizeof c->lc[0]);
    e.valid = true;
    e.gen = gen;
    e.t = *t;
    e.stream = hs;
    e.f = f;
}

// An unchanged grid frame on this stream and target: *hit = the cached frame,
// counted as a render with the current region lists; null = plan the frame.
vr_status cache_hit(Ctx* c, const vr_target* t, hipStream_t hs, const GridFrame** hit)
{
    *hit = nullptr;
    if (!c->launch_cache || c->mm_pending || c->rg_pending) return VR_OK;
    const Ctx::Cached* e = cached_frame(c, t, hs, c->gen);
    if (!e) return VR_OK;
    HIP_TRY(hipSetDevice(c->device));
    ++c->renders_since_build;
    ++c->lc_hits;
    if (e->f.kind == SCHED_REGIONS) c->region_slot = e->f.slot;
    *hit = &e->f;
    return VR_OK;
}

// ---- planning a grid frame

// The frame's arguments, plan and schedule without the region lists:
// frame_march_args, the uniform channels, schedule kind and tiles per wave.
// The render is not counted and the lists are not touched (a pair's second
// frame stops here: the lists are the first's).  *f: a fresh GridFrame.
vr_status grid_frame_args(Ctx* c, const vr_target* t, const TargetInfo& ti, GridFrame* f)
{
    MarchArgs& a = f->a;
    if (const vr_status st = frame_march_args("vr_render", c, t, ti, &a, &f->pl)) return st;
    if (c->uniform_skip) {
        const vr_status us = resolve_uniform(c);
        if (us != VR_OK) return us;
        a.umask = c->uniform_mask;
        for (int ch = 0; ch < 4; ++ch) a.uval[ch] = (float)c->uniform_val[ch] * (1.0f / 255.0f);   // blend()'s scale
    }
    HIP_TRY(hipSetDevice(c->device));
    // auto schedule (measured): regions -- per-XCD angular
    // wedges of the frame, each walked inside-out (longest rays first)
    const int kind = c->schedule >= 0 ? c->schedule : SCHED_REGIONS;
    // tiles per wave, auto: rings 2; regions 3 for COL48 (the streamed 512^3
    // layout: 0.1216 -> 0.1176 ms with 8 wedges, profiles/r04/r04_tpw_c5.txt)
    // and 2 for the others (config 4 level); strided 1
    const int tpw = c->tiles_per_wave > 0 ? c->tiles_per_wave
                    : kind == SCHED_REGIONS ? (f->pl.layout == LAYOUT_COL48 ? 3 : 2)
                    : kind == SCHED_RINGS ? 2 : 1;
    Schedule& sc = f->sc;
    sc = Schedule{kind, 0, 0, tpw, c->waves_per_simd, c->d_heads, nullptr, {}, 1, 0, c->wg_waves, nullptr};
    sc.slab = f->pl.layout == LAYOUT_COL48 && c->slab;
    a.slab_cap = c->slab_cap;
    if (kind == SCHED_RINGS || kind == SCHED_REGIONS) box_centre_pixel(c, a, &sc.center_x, &sc.center_y);
    f->kind = kind;
    return VR_OK;
}

// The region lists of a regions frame (build_regions counts the render and
// reuses, or rebuilds, the lists), the empty-tile fill, the wave count and the
// step split.
vr_status attach_regions(Ctx* c, hipStream_t hs, GridFrame* f)
{
    MarchArgs& a = f->a;
    const Plan& pl = f->pl;
    Schedule& sc = f->sc;
    const int tpw = sc.tiles_per_wave;
    const bool splittable = is_b4_family(pl.layout) || pl.layout == LAYOUT_ZPAIR || pl.layout == LAYOUT_CORNER8 ||
                            pl.layout == LAYOUT_CORNERH || pl.layout == LAYOUT_COL48Z;
    const vr_status st = build_regions(c, a, tpw, sc.center_x, sc.center_y, hs);
    if (st != VR_OK) return st;
    const Ctx::RegionBuf& rb = c->region[c->region_cur];
    sc.tiles = rb.d + kRegionHeader;
    sc.hdr = reinterpret_cast<const int*>(rb.d);
    sc.map = rb.map;
    // the default kernels march the lists' first hdr[kRegionWork + x] entries
    // and fill the rest (tile_is_empty); the slab march marches all
    const bool fill = c->empty_fill && c->region_exact && !sc.slab;
    a.empty_fill = fill ? 1 : 0;
    // Waves: as many as before (the list over tiles_per_wave), but no more
    // than marched entries -- the waves that held only empty tiles go;
    // each marched tile keeps a wave of its own where it had one
    if (fill && rb.most_marched > 0) sc.map.nwx = std::max(1, std::min(sc.map.nwx, rb.most_marched));
    if (splittable) {
        // step-split rays: K lanes per ray when the frame
        // share is too small to fill the GPU with one-lane-per-ray waves
        int K = c->split;
        if (sc.slab) K = K == 0 ? 1 : K;   // the slab march has one lane per ray; split > 1 uses the plain march
        if (K == 0) K = auto_split(c, rb.nwork);
        if (K > 1) {
            sc.split = K;
            sc.map.nwx = std::max(1, (rb.most * K + tpw - 1) / tpw);
            if (a.empty_fill && rb.most_marched > 0)   // (as above, in split units)
                sc.map.nwx = std::max(1, std::min(sc.map.nwx, rb.most_marched * K));
        }
    }
    f->slot = c->region_slot;
    return VR_OK;
}

// Launch a frame alone.  remember: the target to cache it under (null for a
// frame that came from the cache), with the context's `gen` of its planning.
vr_status launch_frame(Ctx* c, const GridFrame& f, const vr_target* remember, unsigned long long gen, hipStream_t hs)
{
    HIP_TRY(launch_march(f.a, f.pl.layout, f.pl.wrap, f.pl.early, f.sc, hs));
    if (remember) remember_frame(c, remember, hs, gen, f);
    if (f.kind == SCHED_REGIONS) return note_region_render(c, hs);
    return VR_OK;
}

// A procedural frame (BASELINE configs 2/3): its arguments and the Perlin
// lattice table; the scratch and stream bookkeeping and the launch are
// render_procedural's.
vr_status render_procedural_frame(Ctx* c, const vr_target* t, const TargetInfo& ti, hipStream_t hs)
{
    MarchArgs a{};
    Plan pl;
    if (const vr_status st = frame_march_args("vr_render", c, t, ti, &a, &pl)) return st;
    ProcParams& q = a.proc;
    if (q.wt_fixed && q.wt_n > 0 && c->lattice && c->schedule != SCHED_STATIC && c->schedule != SCHED_RINGS) {
        const vr_status st = ensure_lattice(c, &q, hs);
        if (st != VR_OK) return st;
    }
    HIP_TRY(hipSetDevice(c->device));
    return render_procedural(c, a, pl.early, hs);
}

// render_frames' first frame, planned as vr_render plans it (the checks,
// inject_throw, the cached frame or a planned one with its lists) but not
// launched.  Its errors are vr_render's, a caught exception included.
vr_status plan_first_frame(Ctx* c, const vr_target* t, hipStream_t hs, TargetInfo* ti, GridFrame* f)
try {
    if (const vr_status st = check_target("vr_render", c, t, ti)) return st;
    honour_inject_throw(c);
    const GridFrame* hit = nullptr;
    if (const vr_status st = cache_hit(c, t, hs, &hit)) return st;
    if (hit) {
        *f = *hit;
        return VR_OK;
    }
    if (const vr_status st = grid_frame_args(c, t, *ti, f)) return st;
    return f->kind == SCHED_REGIONS ? attach_regions(c, hs, f) : VR_OK;
} catch (...) {
    return caught_exception("vr_render");
}

// The second frame's arguments may differ from the first's only in what the paired kernel
// reads per frame: the camera (ray basis, r2 / r3, cam, tap_T), the target buffer, the
// empty-tile fill and the step counter.
bool pair_compatible(const GridFrame& f0, const GridFrame& f1)
{
    if (f0.pl.layout != f1.pl.layout || f0.pl.wrap != f1.pl.wrap || f0.pl.early != f1.pl.early) return false;
    const MarchArgs &a = f0.a, &b = f1.a;
    // the shared part, field by field (the structs' padding is not compared)
#define VR_SAME(F) (std::memcmp(&a.F, &b.F, sizeof a.F) == 0)
    return VR_SAME(box_min) && VR_SAME(box_max) && VR_SAME(box_range) && VR_SAME(step_size) && VR_SAME(density) &&
           VR_SAME(scale) && VR_SAME(acc_limit) && VR_SAME(max_steps) && VR_SAME(tap_S) && VR_SAME(zero_offsets) &&
           VR_SAME(umask) && VR_SAME(uval) && VR_SAME(nx) && VR_SAME(ny) && VR_SAME(nz) && VR_SAME(vol) &&
           VR_SAME(plane_stride) && VR_SAME(geom.B) && VR_SAME(geom.R) && VR_SAME(geom.Ba) && VR_SAME(geom.Rn) &&
           VR_SAME(geom.brick) && VR_SAME(geom.nbx) && VR_SAME(geom.nby) && VR_SAME(geom.nbz) && VR_SAME(width) &&
           VR_SAME(height) && VR_SAME(band_rows) && VR_SAME(band_stride) && VR_SAME(band_first) && VR_SAME(out_rows) &&
           VR_SAME(band_flip) && VR_SAME(pitch) && VR_SAME(format) && VR_SAME(bands_in_place) && VR_SAME(slab_cap);
#undef VR_SAME
}

// The region lists' empty tiles (built for frame 0's camera) are frame 1's too: the part
// of build_regions' key that the camera sets is the same
bool same_region_camera(const GridFrame& f0, const GridFrame& f1)
{
    const MarchArgs &a = f0.a, &b = f1.a;
    return f0.sc.center_x == f1.sc.center_x && f0.sc.center_y == f1.sc.center_y &&
           std::memcmp(a.org, b.org, sizeof a.org) == 0 && std::memcmp(a.o, b.o, sizeof a.o) == 0 &&
           std::memcmp(a.px, b.px, sizeof a.px) == 0 && std::memcmp(a.py, b.py, sizeof a.py) == 0 &&
           std::memcmp(a.r3, b.r3, sizeof a.r3) == 0;
}

// vr_render_pair's and vr_render_group's targets: one geometry, format, band selection and
// step counter, n buffers (t[0] itself is checked by frame 0's plan)
vr_status check_targets_agree(const char* fn, const vr_target* t, int n)
{
    for (int k = 1; k < n; ++k) {
        // field by field: the structs' padding is the caller's
        const vr_target &a = t[0], &b = t[k];
        if (a.width != b.width || a.height != b.height || a.format != b.format || a.band_rows != b.band_rows ||
            a.band_stride != b.band_stride || a.band_first != b.band_first || a.row_pitch != b.row_pitch ||
            a.step_counter != b.step_counter || a.band_flip != b.band_flip || a.reserved != b.reserved)
            return fail(VR_ERR_INVALID, "%s: the targets must agree in everything but pixels", fn);
        const int f = a.format & ~(VR_TARGET_BANDS_IN_PLACE | VR_TARGET_ROW_RANGE);
        if (!b.pixels || (f >= 0 && f <= 5 && (uintptr_t)b.pixels % format_bytes(f) != 0))
            return fail(VR_ERR_INVALID, "%s: target %d's pixels are null or misaligned", fn, k);
    }
    return VR_OK;
}

// Frames i..n-1 as ordinary renders, in order, each with its own shader data
vr_status render_plain(void* p, const vr_target* t, int i, int n, const vr_object_shader_data* osd,
                       const vr_global_shader_data* gsd, void* stream)
{
    vr_status st = VR_OK;
    for (; i < n && st == VR_OK; ++i) {
        if (osd) st = vr_set_shader_data(p, &osd[i], &gsd[i]);
        if (st == VR_OK) st = vr_render(p, &t[i], stream);
    }
    return st;
}

// n = 2 or 4 queued frames in one launch (vr_render_pair, vr_render_group), or as ordinary
// renders where there is no such launch for them.  The targets agree (check_targets_agree).
vr_status render_frames(void* p, const vr_target* t, int n, const vr_object_shader_data* osd,
                        const vr_global_shader_data* gsd, void* stream)
{
    Ctx* c = as_ctx(p);
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    if (c->proc.enabled) return render_plain(p, t, 0, n, osd, gsd, stream);   // a procedural medium
    if (osd) {
        const vr_status st = vr_set_shader_data(p, &osd[0], &gsd[0]);
        if (st != VR_OK) return st;
    }
    // frame 0: vr_render's whole path (checks, plan, region lists) up to the launch
    TargetInfo ti;
    GridFrame f[VR_MAX_GROUP];
    vr_status st = plan_first_frame(c, &t[0], hs, &ti, &f[0]);
    if (st != VR_OK) return st;
    const unsigned long long gen0 = c->gen;
    // launched alone it is remembered under gen0, unless it came from the cache: no second entry for it
    const auto frame0_alone = [&] {
        return launch_frame(c, f[0], cached_frame(c, &t[0], hs, gen0) ? nullptr : &t[0], gen0, hs);
    };
    const bool groupable = f[0].kind == SCHED_REGIONS && f[0].sc.split <= 1 && !f[0].sc.slab && f[0].sc.wg_waves == 4 &&
                           pair_layout(f[0].pl.layout) && f[0].pl.wrap == WRAP_CLAMP;
    bool grouped = groupable;
    for (int k = 1; k < n && groupable; ++k) {
        // frame k: its arguments and plan only (the lists are frame 0's); t[k] passed t[0]'s checks
        if (osd) st = vr_set_shader_data(p, &osd[k], &gsd[k]);
        if (st == VR_OK) st = grid_frame_args(c, &t[k], ti, &f[k]);
        if (st != VR_OK) {   // frames 0..k-1 still render (frame 0 is planned and counted)
            const std::string msg = g_err;
            vr_status rs = frame0_alone();
            if (rs == VR_OK) rs = render_plain(p, t, 1, k, osd, gsd, stream);
            if (osd) (void)vr_set_shader_data(p, &osd[k], &gsd[k]);   // the ctx holds what the failed frame set
            g_err = msg;
            return st;
        }
        grouped = grouped && f[k].kind == f[0].kind && pair_compatible(f[0], f[k]);
    }
    if (!grouped) {
        // no multi-frame kernel for this plan (split rays, the slab, an experiment schedule, a
        // layout without an instance), or frames whose plans differ: the ordinary renders
        st = frame0_alone();
        return st == VR_OK ? render_plain(p, t, 1, n, osd, gsd, stream) : st;
    }
    // frame k fills the lists' empty tiles only where they are its own (attach_regions'
    // region_exact rule); a launch one frame of which marches every entry keeps the
    // unreduced wave count
    const Ctx::RegionBuf& rb = c->region[c->region_cur];
    FrameArgs fr[VR_MAX_GROUP];
    bool every = f[0].a.empty_fill != 0;
    for (int k = 0; k < n; ++k) {
        if (k > 0) f[k].a.empty_fill = f[0].a.empty_fill && same_region_camera(f[0], f[k]) ? 1 : 0;
        every = every && f[k].a.empty_fill;
        fr[k] = frame_part(f[k].a);
    }
    Schedule sc = f[0].sc;
    if (f[0].a.empty_fill && !every) sc.map.nwx = std::max(1, rb.map.nwx);
    // four frames of one camera (the static-camera frame loop): the QUAD instance, one ray per
    // pixel for all four; every other group launches the kernel it always did.  The QUAD
    // instance counts no steps (the per-lane sum's registers would cost it a wave per SIMD),
    // so a counted launch is one of those others
    bool eligible = frames_share_camera(fr, n);
    for (int k = 0; k < n; ++k) eligible = eligible && !fr[k].step_counter;
    // what the options ask for (each builds on the one before: quad_split splits each tap's loads
    // between the lanes, quad_steps gives each lane one step of four, quad_pairs issues a round's
    // loads in slice pairs), cut down to what this plan's kernel has
    const int mode = quad_kernel_mode(f[0].pl.layout, n, f[0].pl.early, f[0].a.zero_offsets != 0, f[0].a.umask,
                                      quad_requested(eligible, c->frame_quad, c->quad_split, c->quad_steps, c->quad_pairs));
    HIP_TRY(launch_march_frames(f[0].a, fr, n, f[0].pl.layout, f[0].pl.early, sc, c->pair_deal, mode, hs));
    c->quad_launches += quad_is_quad(mode);
    c->quad_split_launches += quad_splits(mode);
    c->quad_steps_launches += quad_rounds(mode);
    c->quad_pairs_launches += quad_paired(mode);
    c->group_launches += n == VR_MAX_GROUP;
    c->pair_launches += n / 2;   // (pairs of frames that shared a launch)
    c->renders_since_build += n - 1;   // the later renders with these lists (build_regions counted the first)
    c->region_slot = f[0].slot;
    return note_region_render(c, hs);
}

}  // namespace

extern "C" {

vr_status vr_render(void* p, const vr_target* t, void* stream)
try {
    if (!p || !t) return fail(VR_ERR_INVALID, "vr_render: null argument");
    Ctx* c = as_ctx(p);
    TargetInfo ti;
    if (const vr_status st = check_target("vr_render", c, t, &ti)) return st;
    honour_inject_throw(c);
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    if (c->proc.enabled) return render_procedural_frame(c, t, ti, hs);
    // an unchanged grid frame on this stream and target: launch the cached arguments
    const GridFrame* hit = nullptr;
    if (const vr_status st = cache_hit(c, t, hs, &hit)) return st;
    if (hit) return launch_frame(c, *hit, nullptr, 0, hs);
    GridFrame f;
    if (const vr_status st = grid_frame_args(c, t, ti, &f)) return st;
    if (f.kind == SCHED_REGIONS)
        if (const vr_status st = attach_regions(c, hs, &f)) return st;
    return launch_frame(c, f, t, c->gen, hs);
} catch (...) {
    return caught_exception("vr_render");
}

vr_status vr_render_sequence(void* p, const vr_target* t, int frames, const vr_object_shader_data* osd,
                             const vr_global_shader_data* gsd, void* stream)
try {
    if (!p || !t || frames < 0 || (frames > 0 && (!osd || !gsd)))
        return fail(VR_ERR_INVALID, "vr_render_sequence: bad argument");
    for (int i = 0; i < frames; ++i) {
        vr_status st = vr_set_shader_data(p, &osd[i], &gsd[i]);
        if (st == VR_OK) st = vr_render(p, t, stream);
        if (st != VR_OK) return st;
    }
    return VR_OK;
} catch (...) {
    return caught_exception("vr_render_sequence");
}

vr_status vr_render_pair(void* p, const vr_target* t0, const vr_target* t1, const vr_object_shader_data* osd,
                         const vr_global_shader_data* gsd, void* stream)
try {
    if (!p || !t0 || !t1 || (!osd) != (!gsd)) return fail(VR_ERR_INVALID, "vr_render_pair: bad argument");
    const vr_target t[2] = {*t0, *t1};
    if (const vr_status st = check_targets_agree("vr_render_pair", t, 2)) return st;
    return render_frames(p, t, 2, osd, gsd, stream);
} catch (...) {
    return caught_exception("vr_render_pair");
}

vr_status vr_render_group(void* p, const vr_target* t, int n, const vr_object_shader_data* osd,
                          const vr_global_shader_data* gsd, void* stream)
try {
    if (!p || !t || n < 1 || n > VR_MAX_GROUP || (!osd) != (!gsd)) return fail(VR_ERR_INVALID, "vr_render_group: bad argument");
    if (const vr_status st = check_targets_agree("vr_render_group", t, n)) return st;
    int launches[3];
    const int nl = vr_group_split(n, launches);
    if (launches[0] == VR_MAX_GROUP) return render_frames(p, t, n, osd, gsd, stream);
    // n < 4: a pair and / or a plain render, vr_render_pair's and vr_render's paths
    int i = 0;
    for (int l = 0; l < nl; ++l) {
        const vr_status st = launches[l] == 2 ? vr_render_pair(p, &t[i], &t[i + 1], osd ? &osd[i] : nullptr,
                                                               gsd ? &gsd[i] : nullptr, stream)
                                              : render_plain(p, t, i, n, osd, gsd, stream);
        if (st != VR_OK) return st;
        i += launches[l];
    }
    return VR_OK;
} catch (...) {
    return caught_exception("vr_render_group");
}

int vr_group_split(int n, int launches[3])
{
    if (!launches || n < 1 || n > VR_MAX_GROUP) return 0;
    int k = 0;
    if (n == VR_MAX_GROUP) launches[k++] = VR_MAX_GROUP;
    else {
        if (n >= 2) launches[k++] = 2;
        if (n & 1) launches[k++] = 1;
    }
    for (int i = k; i < 3; ++i) launches[i] = 0;
    return k;
}

}   // extern "C"
