// vr_rect.cpp -- vr_render_rect and vr_render_rects, the scissored renders, and
// vr_update_footprint (include/vr.h).
//
// Both renders build the whole frame's MarchArgs as vr_render does
// (frame_march_args, vr_render.cpp: band_rows = 0, every channel loaded) and launch
// the rectangle kernels of vr_march_rect.hip.  They read the context and
// change nothing in it: no cached launch, region list, sort or deferred-shadow
// scratch, no `gen` bump, and the pending uniform-channel read-back
// (mm_pending) stays pending for the next vr_render -- the rectangle kernels
// load every channel (umask 0), which is exact whatever the read-back will say.
#include "vr_ctx.h"

namespace vrapi {

bool rect_in_frame(int width, int height, const vr_rect* r)
{
    return r->x >= 0 && r->y >= 0 && r->width >= 0 && r->height >= 0 && r->width <= width - r->x &&
           r->height <= height - r->y;
}

}  // namespace vrapi

using namespace vrapi;

namespace {

// What vr_render_rect and vr_render_rects check before they look at a
// rectangle: the context, the volume, the camera and a plain whole-frame target
// (vr_render's checks, in these entry points' own order).
vr_status check_frame_target(const char* fn, const Ctx* c, const vr_target* t, TargetInfo* ti)
{
    if (const vr_status st = check_frame_state(fn, c, t)) return st;
    if (t->format < 0 || t->format > 5)
        return fail(VR_ERR_INVALID, "%s: bad format %d (a whole-frame target: no VR_TARGET_* flag)", fn, t->format);
    if (t->band_rows != 0 || t->band_flip != 0)
        return fail(VR_ERR_INVALID, "%s: a whole-frame target is needed (band_rows %d, band_flip %d)", fn,
                    t->band_rows, t->band_flip);
    if (t->reserved != 0) return fail(VR_ERR_INVALID, "%s: vr_target.reserved must be 0", fn);
    *ti = TargetInfo{t->format, 0, false, false};
    return check_pixels(fn, t, t->format, &ti->pitch);
}

bool holds(const vr_rect& a, const vr_rect& b)   // a contains b, both non-empty
{
    return a.x <= b.x && a.y <= b.y && b.x + b.width <= a.x + a.width && b.y + b.height <= a.y + a.height;
}

}  // namespace

extern "C" {

vr_status vr_render_rect(void* p, const vr_target* t, const vr_rect* r, void* stream)
try {
    if (!p || !t || !r) return fail(VR_ERR_INVALID, "vr_render_rect: null argument");
    Ctx* c = as_ctx(p);
    TargetInfo ti;
    if (const vr_status st = check_frame_target("vr_render_rect", c, t, &ti)) return st;
    if (!rect_in_frame(t->width, t->height, r))
        return fail(VR_ERR_INVALID, "vr_render_rect: rectangle %dx%d at (%d, %d) leaves the %dx%d frame", r->width,
                    r->height, r->x, r->y, t->width, t->height);
    honour_inject_throw(c);
    if (r->width == 0 || r->height == 0) return VR_OK;

    MarchArgs a{};
    Plan pl{};
    if (const vr_status st = frame_march_args("vr_render_rect", c, t, ti, &a, &pl)) return st;
    const RectArgs rc = rect_args(r->x, r->y, r->width, r->height);
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (c->proc.enabled) HIP_TRY(launch_march_proc_rect(a, pl.early, rc, hs));
    else HIP_TRY(launch_march_rect(a, pl.layout, pl.wrap, pl.early, rc, hs));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_render_rect");
}

vr_status vr_render_rects(void* p, const vr_target* t, const vr_rect* rects, int count, void* stream)
try {
    if (!p || !t) return fail(VR_ERR_INVALID, "vr_render_rects: null argument");
    if (count < 0 || count > VR_MAX_RECTS)
        return fail(VR_ERR_INVALID, "vr_render_rects: count %d (0 .. %d; vr_rects_coalesce shortens a list)", count,
                    VR_MAX_RECTS);
    if (count > 0 && !rects) return fail(VR_ERR_INVALID, "vr_render_rects: rects is null with count %d", count);
    Ctx* c = as_ctx(p);
    TargetInfo ti;
    if (const vr_status st = check_frame_target("vr_render_rects", c, t, &ti)) return st;
    for (int i = 0; i < count; ++i)
        if (!rect_in_frame(t->width, t->height, &rects[i]))
            return fail(VR_ERR_INVALID, "vr_render_rects: rectangle %d, %dx%d at (%d, %d), leaves the %dx%d frame", i,
                        rects[i].width, rects[i].height, rects[i].x, rects[i].y, t->width, t->height);
    honour_inject_throw(c);
    // The kernel's list: no empty rectangle, and none that another one of the list holds (of
    // identical ones the first stays) -- the union, and with it what is written and counted,
    // is the same, and no wave is launched for a tile that owns no pixel.
    RectList rl{};
    for (int i = 0; i < count; ++i) {
        const vr_rect& r = rects[i];
        if (r.width == 0 || r.height == 0) continue;
        bool held = false;
        for (int j = 0; j < count && !held; ++j) {
            const vr_rect& q = rects[j];
            if (j == i || q.width == 0 || q.height == 0 || !holds(q, r)) continue;
            held = !holds(r, q) || j < i;
        }
        if (!held) rect_list_add(&rl, r.x, r.y, r.width, r.height);
    }
    if (rl.count == 0) return VR_OK;

    MarchArgs a{};
    Plan pl{};
    if (const vr_status st = frame_march_args("vr_render_rects", c, t, ti, &a, &pl)) return st;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (c->proc.enabled) HIP_TRY(launch_march_proc_rects(a, pl.early, rl, hs));
    else HIP_TRY(launch_march_rects(a, pl.layout, pl.wrap, pl.early, rl, hs));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_render_rects");
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
