// vr_rect.cpp -- vr_render_rect, the scissored render, and vr_update_footprint
// (include/vr.h).
//
// vr_render_rect builds the whole frame's MarchArgs with the helpers it shares
// with vr_render (frame_args, proc_args, make_plan, volume_args) and launches
// the rectangle kernels of vr_march_rect.hip.  It reads the context and
// changes nothing in it: no cached launch, region list, sort or deferred-shadow
// scratch, no `gen` bump, and the pending uniform-channel read-back
// (mm_pending) stays pending for the next vr_render -- the rectangle kernels
// load every channel (umask 0), which is exact whatever the read-back will say.
#include "vr_ctx.h"

using namespace vrapi;

extern "C" {

vr_status vr_render_rect(void* p, const vr_target* t, const vr_rect* r, void* stream)
try {
    if (!p || !t || !r) return fail(VR_ERR_INVALID, "vr_render_rect: null argument");
    Ctx* c = as_ctx(p);
    if (!c->d_planar && !c->proc.enabled)
        return fail(VR_ERR_NO_VOLUME, "vr_render_rect: no volume (vr_set_volume / vr_generate_volume)");
    if (!c->has_camera) return fail(VR_ERR_NO_CAMERA, "vr_render_rect: no shader data (vr_set_shader_data)");
    if (t->width <= 0 || t->height <= 0)
        return fail(VR_ERR_INVALID, "vr_render_rect: bad size %dx%d", t->width, t->height);
    if (t->format < 0 || t->format > 5)
        return fail(VR_ERR_INVALID, "vr_render_rect: bad format %d (a whole-frame target: no VR_TARGET_* flag)", t->format);
    if (t->band_rows != 0 || t->band_flip != 0)
        return fail(VR_ERR_INVALID, "vr_render_rect: a whole-frame target is needed (band_rows %d, band_flip %d)",
                    t->band_rows, t->band_flip);
    if (t->reserved != 0) return fail(VR_ERR_INVALID, "vr_render_rect: vr_target.reserved must be 0");
    if (!t->pixels) return fail(VR_ERR_INVALID, "vr_render_rect: pixels is null");
    const int bpp = format_bytes(t->format);
    const size_t pitch = t->row_pitch ? t->row_pitch : (size_t)t->width * bpp;
    if (pitch < (size_t)t->width * bpp || pitch % bpp != 0 || ((uintptr_t)t->pixels % bpp) != 0)
        return fail(VR_ERR_INVALID, "vr_render_rect: pitch/alignment (pitch %zu, bpp %d)", pitch, bpp);
    if (r->x < 0 || r->y < 0 || r->width < 0 || r->height < 0 || r->width > t->width - r->x ||
        r->height > t->height - r->y)
        return fail(VR_ERR_INVALID, "vr_render_rect: rectangle %dx%d at (%d, %d) leaves the %dx%d frame", r->width,
                    r->height, r->x, r->y, t->width, t->height);
    if (c->inject_throw) {
        const int k = c->inject_throw;
        c->inject_throw = 0;
        if (k == 2) throw std::bad_alloc();
        throw std::runtime_error("injected by vr option inject_throw");
    }
    if (r->width == 0 || r->height == 0) return VR_OK;

    MarchArgs a{};
    if (!frame_args(c, t->width, t->height, &a))
        return fail(VR_ERR_INVALID, "vr_render_rect: Projection*View is singular");
    Plan pl{LAYOUT_PLANAR, WRAP_CLAMP, c->march.early_out > 0.0f};
    if (c->proc.enabled) proc_args(c, &a);   // no lattice table: the fBm hashes every corner
    else make_plan(c, &a, &pl);
    a.nx = c->nx; a.ny = c->ny; a.nz = c->nz;
    volume_args(c, pl, &a);
    // the whole frame, as vr_render describes it with band_rows = 0
    a.width = t->width;
    a.height = t->height;
    a.band_rows = t->height; a.band_stride = 1; a.band_first = 0;
    a.out_rows = t->height;
    a.tiles_x = (t->width + 15) / 16;
    a.tiles_y = (t->height + 15) / 16;
    a.num_blocks = 8 * ((a.tiles_y + 7) / 8) * a.tiles_x;
    a.out = t->pixels;
    a.pitch = (long long)pitch;
    a.format = t->format;
    a.step_counter = reinterpret_cast<unsigned long long*>(t->step_counter);
    const RectArgs rc = rect_args(r->x, r->y, r->width, r->height);
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (c->proc.enabled) HIP_TRY(launch_march_proc_rect(a, pl.early, rc, hs));
    else HIP_TRY(launch_march_rect(a, pl.layout, pl.wrap, pl.early, rc, hs));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_render_rect");
}

vr_status vr_update_footprint(void* p, int width, int height, int x0, int y0, int z0, int bx, int by, int bz,
                              vr_rect* out)
try {
    if (!p || !out) return fail(VR_ERR_INVALID, "vr_update_footprint: null argument");
    const Ctx* c = as_ctx(p);
    if (!c->d_planar) return fail(VR_ERR_NO_VOLUME, "vr_update_footprint: no volume set");
    if (!c->has_camera) return fail(VR_ERR_NO_CAMERA, "vr_update_footprint: no shader data (vr_set_shader_data)");
    static_assert(sizeof(vr_object_shader_data) == sizeof c->obj && sizeof(vr_global_shader_data) == sizeof c->glob,
                  "the context keeps the shader data in the ABI's layout");
    vr_object_shader_data osd;
    vr_global_shader_data gsd;
    std::memcpy(&osd, c->obj, sizeof osd);
    std::memcpy(&gsd, c->glob, sizeof gsd);
    return vr_volume_box_footprint(&osd, &gsd, &c->march, c->nx, c->ny, c->nz, width, height, x0, y0, z0, bx, by, bz,
                                   out);
} catch (...) {
    return caught_exception("vr_update_footprint");
}

}  // extern "C"
