// vr_query.cpp -- vr_query_rect, the per-pixel ray records of a rectangle of the
// frame (include/vr.h).
//
// The call builds the whole frame's MarchArgs as vr_render_rect does
// (frame_march_args, vr_render.cpp: band_rows = 0, every channel loaded) for a
// width x height frame with no pixel buffer and no step counter, and launches
// the query kernels of vr_march_query.hip, which write records and nothing else.
// It reads the context and changes nothing in it: no cached launch, region
// list, sort or deferred-shadow scratch, no `gen` bump, and the pending
// uniform-channel read-back (mm_pending) stays pending for the next vr_render.
#include "vr_ctx.h"

using namespace vrapi;

static_assert(sizeof(vr_ray_record) == 64 && offsetof(vr_ray_record, entry) == 16 && offsetof(vr_ray_record, step) == 32 &&
                  offsetof(vr_ray_record, hit) == 48,
              "a record is the four 16-byte stores of vr_march_query.hip store_record");

extern "C" {

vr_status vr_query_rect(void* p, int width, int height, const vr_rect* r, float threshold, void* d_records,
                        size_t row_pitch_records, void* stream)
try {
    if (!p || !r || !d_records) return fail(VR_ERR_INVALID, "vr_query_rect: null argument");
    Ctx* c = as_ctx(p);
    vr_target t{};   // the frame the rays belong to: no pixels, no counter
    t.width = width;
    t.height = height;
    t.format = VR_FMT_R32F;
    if (const vr_status st = check_frame_state("vr_query_rect", c, &t)) return st;
    if (!rect_in_frame(width, height, r))
        return fail(VR_ERR_INVALID, "vr_query_rect: rectangle %dx%d at (%d, %d) leaves the %dx%d frame", r->width,
                    r->height, r->x, r->y, width, height);
    const size_t pitch = row_pitch_records ? row_pitch_records : (size_t)r->width;
    if (pitch < (size_t)r->width || pitch > ((size_t)1 << 28))   // 2^28 records: row * pitch stays far inside 64 bits
        return fail(VR_ERR_INVALID, "vr_query_rect: row pitch %zu records (the rectangle's width %d .. 2^28)", pitch,
                    r->width);
    if ((uintptr_t)d_records % 16 != 0)
        return fail(VR_ERR_INVALID, "vr_query_rect: d_records must be 16-byte aligned");
    if (!(threshold >= 0.0f && threshold < 1.0f)) return fail(VR_ERR_INVALID, "vr_query_rect: threshold in [0,1)");
    if (threshold > 0.0f && !(c->march.density > 0.0f))
        return fail(VR_ERR_INVALID, "vr_query_rect: a threshold needs density > 0");
    honour_inject_throw(c);
    if (r->width == 0 || r->height == 0) return VR_OK;

    MarchArgs a{};
    Plan pl{};
    const TargetInfo ti{VR_FMT_R32F, (size_t)width * sizeof(float), false, false};
    if (const vr_status st = frame_march_args("vr_query_rect", c, &t, ti, &a, &pl)) return st;
    const RectArgs rc = rect_args(r->x, r->y, r->width, r->height);
    // the limit by acc_limit's own expression: a query at threshold T finds the step a context with early_out T stops after
    const QueryArgs q{static_cast<float4*>(d_records), (long long)pitch, acc_limit_of(threshold, a.density, a.step_size)};
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (c->proc.enabled) HIP_TRY(launch_march_proc_query(a, pl.early, rc, q, hs));
    else HIP_TRY(launch_march_query(a, pl.layout, pl.wrap, pl.early, rc, q, hs));
    return VR_OK;
} catch (...) {
    return caught_exception("vr_query_rect");
}

}  // extern "C"
