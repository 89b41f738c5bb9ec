// vr_renderer.hpp -- C++ host interface over the C ABI of vr.h.
//
// A thin RAII layer that gives C++ callers the shape of the reference's own
// host API for this path:
//
//   reference (file:line)                                  here
//   vkc::Renderer::Init / Shutdown (VulkanRenderer.h:68-72) Renderer ctor / dtor
//   vkc::Texture3D(data, extent) (VulkanTexture.h:55-60)    Renderer::SetVolume
//   noise -> pixelData start-up (TestMain.cpp:43-92)        Renderer::GenerateVolume
//   UniformBuffer<ObjectShaderData>::Update (TestMain:248)  Renderer::UpdateObjectData
//   UniformBuffer<GlobalShaderData>::Update (TestMain:249)  Renderer::UpdateGlobalData
//   EnqueueRenderPass("BasePass", rect, ...) + draw
//     (VulkanRenderer.h:84-87, TestMain.cpp:194-217)       Renderer::EnqueueRenderPass
//
// Errors are thrown as vr::Error on the C++ side, as the reference throws from
// Error() (Utils.h:22-29).  They become status codes at the C ABI.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "vr.h"

namespace vr {

using ObjectShaderData = vr_object_shader_data;   // TestMain.cpp:27-32
using GlobalShaderData = vr_global_shader_data;   // TestMain.cpp:34-39

class Error : public std::runtime_error {
public:
    Error(vr_status s, const std::string& what) : std::runtime_error(what), status(s) {}
    vr_status status;
};

inline void Check(vr_status s, const char* where)
{
    if (s != VR_OK) throw Error(s, std::string(where) + ": " + vr_last_error());
}

struct Rect2D {  // VkRect2D analogue: the rows/columns of the frame to draw
    int width = 0, height = 0;
};

// At most max_out rectangles whose union contains the union of `rects`
// (vr_rects_coalesce): for a caller of Renderer::RenderRects with more than
// VR_MAX_RECTS edits, or many tiny ones.  Host code only.
inline std::vector<vr_rect> CoalesceRects(const std::vector<vr_rect>& rects, int max_out = VR_MAX_RECTS)
{
    std::vector<vr_rect> out(rects.size());
    int n = 0;
    Check(vr_rects_coalesce(rects.data(), (int)rects.size(), max_out, out.data(), &n), "vr_rects_coalesce");
    out.resize((size_t)n);
    return out;
}

// The brush's bounding box clipped to an nx x ny x nz volume (vr_brush_box):
// what Renderer::Paint rewrites and what Renderer::UpdateFootprint takes;
// false (and a zero extent) when the brush misses the volume.  Host code only.
inline bool BrushBox(const vr_brush& brush, int nx, int ny, int nz, int origin[3], int extent[3])
{
    Check(vr_brush_box(&brush, nx, ny, nz, origin, extent), "vr_brush_box");
    return extent[0] > 0;
}

// The smoothing brush on a host RGBA8 volume (vr_brush_blur_apply): the CPU
// statement of Renderer::Blur.  Host code only.
inline void BrushBlurApply(const vr_brush& brush, int half_width, uint8_t* rgba, int nx, int ny, int nz)
{
    Check(vr_brush_blur_apply(&brush, half_width, rgba, nx, ny, nz), "vr_brush_blur_apply");
}

// The erode / dilate brush on a host RGBA8 volume (vr_brush_morph_apply): the
// CPU statement of Renderer::Morph.  Host code only.
inline void BrushMorphApply(const vr_brush& brush, int op, int half_width, uint8_t* rgba, int nx, int ny, int nz)
{
    Check(vr_brush_morph_apply(&brush, op, half_width, rgba, nx, ny, nz), "vr_brush_morph_apply");
}

// The median / rank-filter brush on a host RGBA8 volume (vr_brush_rank_apply):
// the CPU statement of Renderer::Rank.  Host code only.
inline void BrushRankApply(const vr_brush& brush, int rank, int half_width, uint8_t* rgba, int nx, int ny, int nz)
{
    Check(vr_brush_rank_apply(&brush, rank, half_width, rgba, nx, ny, nz), "vr_brush_rank_apply");
}

// The flood-fill brush on a host RGBA8 volume (vr_brush_fill_apply): the CPU
// statement of Renderer::Fill; *report (optional) receives what it found.
// Host code only.
inline void BrushFillApply(const vr_brush& brush, const vr_fill_rule& rule, uint8_t* rgba, int nx, int ny, int nz,
                           vr_fill_report* report = nullptr)
{
    Check(vr_brush_fill_apply(&brush, &rule, rgba, nx, ny, nz, report), "vr_brush_fill_apply");
}

// The clone brush on a host RGBA8 volume (vr_brush_clone_apply): the CPU
// statement of Renderer::Clone.  Host code only.
inline void BrushCloneApply(const vr_brush& brush, const vr_clone_map& map, uint8_t* rgba, int nx, int ny, int nz)
{
    Check(vr_brush_clone_apply(&brush, &map, rgba, nx, ny, nz), "vr_brush_clone_apply");
}

// The stamp brush on a host RGBA8 volume with a host stamp
// (vr_brush_stamp_apply): the CPU statement of Renderer::Stamp.  Host code only.
inline void BrushStampApply(const vr_brush& brush, const uint8_t* stamp_rgba, const vr_box& placement, uint8_t* rgba,
                            int nx, int ny, int nz)
{
    Check(vr_brush_stamp_apply(&brush, stamp_rgba, &placement, rgba, nx, ny, nz), "vr_brush_stamp_apply");
}

// The transform paste on host arrays (vr_brush_stamp_affine_apply,
// vr_brush_clone_affine_apply): the CPU statements of Renderer::StampAffine and
// Renderer::CloneAffine.  Host code only.
inline void BrushStampAffineApply(const vr_brush& brush, const uint8_t* stamp_rgba, int sbx, int sby, int sbz,
                                  const vr_affine& map, uint8_t* rgba, int nx, int ny, int nz)
{
    Check(vr_brush_stamp_affine_apply(&brush, stamp_rgba, sbx, sby, sbz, &map, rgba, nx, ny, nz), "vr_brush_stamp_affine_apply");
}
inline void BrushCloneAffineApply(const vr_brush& brush, const vr_affine& map, uint8_t* rgba, int nx, int ny, int nz)
{
    Check(vr_brush_clone_affine_apply(&brush, &map, rgba, nx, ny, nz), "vr_brush_clone_affine_apply");
}

// The map that pastes the source turned / scaled by the row-major 3 x 3
// `forward` with source position src_centre on destination texel dst_centre
// (vr_affine_place).  Host code only; throws for a singular matrix.
inline vr_affine AffinePlace(const double forward[9], const double src_centre[3], const int32_t dst_centre[3],
                             int filter = VR_FILTER_LINEAR, int border = VR_BORDER_CLAMP)
{
    vr_affine a{};
    Check(vr_affine_place(forward, src_centre, dst_centre, filter, border, &a), "vr_affine_place");
    return a;
}

// The liquify brush on a host array (vr_brush_warp_apply): the CPU statement of
// Renderer::Warp; and the map of a push by d16 (16.16 texels per axis) under a
// brush at `centre` (vr_warp_push).  Host code only.
inline void BrushWarpApply(const vr_brush& brush, const vr_affine& map, uint8_t* rgba, int nx, int ny, int nz)
{
    Check(vr_brush_warp_apply(&brush, &map, rgba, nx, ny, nz), "vr_brush_warp_apply");
}
inline vr_affine WarpPush(const int32_t centre[3], const int32_t d16[3], int filter = VR_FILTER_LINEAR,
                          int border = VR_BORDER_CLAMP)
{
    vr_affine a{};
    Check(vr_warp_push(centre, d16, filter, border, &a), "vr_warp_push");
    return a;
}

// What a stamp edits in an nx x ny x nz volume (vr_stamp_box): the brush's
// clipped box intersected with the placement, what Renderer::UpdateFootprint
// takes after Renderer::Stamp; false (and a zero extent) when it is empty.
// Host code only.
inline bool StampBox(const vr_brush& brush, const vr_box& placement, int nx, int ny, int nz, int origin[3], int extent[3])
{
    Check(vr_stamp_box(&brush, &placement, nx, ny, nz, origin, extent), "vr_stamp_box");
    return extent[0] > 0;
}

// The lookup-table brush on a host RGBA8 volume (vr_brush_remap_apply): the CPU
// statement of Renderer::Remap.  vr_lut_identity, vr_lut_levels, vr_lut_compose
// and vr_stats_lut build the table.  Host code only.
inline void BrushRemapApply(const vr_brush& brush, const vr_lut& lut, uint8_t* rgba, int nx, int ny, int nz)
{
    Check(vr_brush_remap_apply(&brush, &lut, rgba, nx, ny, nz), "vr_brush_remap_apply");
}

// The dabs of a drag from brush.centre to the texel `to`, at most `spacing`
// texels apart (vr_brush_line): what Renderer::PaintStroke takes.  skip_first
// omits the dab on the brush's own centre, the joint of two segments.  Host
// code only.
inline std::vector<vr_brush> BrushLine(const vr_brush& brush, const int32_t to[3], int spacing, bool skip_first = false)
{
    int n = 0;
    const vr_status st = vr_brush_line(&brush, to, spacing, skip_first ? 1 : 0, nullptr, 0, &n);   // the number alone
    if (n <= 0) Check(st, "vr_brush_line");
    std::vector<vr_brush> out((size_t)n);
    Check(vr_brush_line(&brush, to, spacing, skip_first ? 1 : 0, out.data(), n, &n), "vr_brush_line");
    return out;
}

class Renderer {
public:
    explicit Renderer(int device = 0) { Check(vr_create(device, &ctx_), "vr_create"); }
    ~Renderer() { vr_destroy(ctx_); }
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    void SetVolume(const uint8_t* rgba, int nx, int ny, int nz)
    {
        Check(vr_set_volume(ctx_, rgba, nx, ny, nz), "vr_set_volume");
    }
    // The copy region with a non-zero imageOffset: overwrite the texel box
    // (bx, by, bz) at (x0, y0, z0) of the installed volume (vr_update_volume).
    void UpdateVolume(const uint8_t* rgba, int x0, int y0, int z0, int bx, int by, int bz)
    {
        Check(vr_update_volume(ctx_, rgba, x0, y0, z0, bx, by, bz), "vr_update_volume");
    }
    // the same from device memory, asynchronous on `stream` (vr_update_volume_device)
    void UpdateVolumeDevice(const void* d_rgba, int x0, int y0, int z0, int bx, int by, int bz, void* stream = nullptr)
    {
        Check(vr_update_volume_device(ctx_, d_rgba, x0, y0, z0, bx, by, bz, stream), "vr_update_volume_device");
    }
    // Blend a brush into the installed volume on the device, asynchronous on
    // `stream` (vr_paint): pick (QueryRect), Paint, UpdateFootprint of
    // BrushBox, RenderRect queue on one stream with no host round trip.
    void Paint(const vr_brush& brush, void* stream = nullptr) { Check(vr_paint(ctx_, &brush, stream), "vr_paint"); }
    // A stroke: at most VR_MAX_DABS dabs applied in order in one paint launch
    // (vr_paint_stroke), bit for bit what Paint of each in turn leaves.
    void PaintStroke(const vr_brush* dabs, int count, void* stream = nullptr)
    {
        Check(vr_paint_stroke(ctx_, dabs, count, stream), "vr_paint_stroke");
    }
    void PaintStroke(const std::vector<vr_brush>& dabs, void* stream = nullptr)
    {
        PaintStroke(dabs.data(), (int)dabs.size(), stream);
    }
    // Soften the installed volume under the brush (vr_blur): a SET brush whose
    // value is the mean of each texel's (2 half_width + 1)^3 neighbourhood as
    // it was before the call; brush.op must be VR_BRUSH_SET.  Queued on
    // `stream` as Paint is; BrushBox names the box it rewrites.
    void Blur(const vr_brush& brush, int half_width = 1, void* stream = nullptr)
    {
        Check(vr_blur(ctx_, &brush, half_width, stream), "vr_blur");
    }
    // Grow or shrink the installed volume under the brush (vr_morph): a SET
    // brush whose value is the minimum (VR_MORPH_ERODE) or maximum
    // (VR_MORPH_DILATE) of each texel's (2 half_width + 1)^3 cube as it was
    // before the call; brush.op must be VR_BRUSH_SET.  Queued on `stream` as
    // Blur is, through the same staging scratch.
    void Morph(const vr_brush& brush, int op, int half_width = 1, void* stream = nullptr)
    {
        Check(vr_morph(ctx_, &brush, op, half_width, stream), "vr_morph");
    }
    // Remove speckle under the brush and keep edges where they are (vr_rank):
    // a SET brush whose value is the rank-th smallest byte (VR_RANK_MEDIAN:
    // the median) of each texel's (2 half_width + 1)^3 cube as it was before
    // the call; brush.op must be VR_BRUSH_SET.  Queued on `stream` as Blur is,
    // through the same staging scratch.
    void Rank(const vr_brush& brush, int rank = VR_RANK_MEDIAN, int half_width = 1, void* stream = nullptr)
    {
        Check(vr_rank(ctx_, &brush, rank, half_width, stream), "vr_rank");
    }
    // Bucket fill / magic wand (vr_fill): the brush blended, as Paint blends
    // it, into the texels under it that pass `rule` and are connected to
    // rule.seed by axis steps over such texels inside the ellipsoid.
    // d_report (optional): a DEVICE vr_fill_report, 8-byte aligned, that
    // receives the region's size and bounds; with every strength 0 the call
    // only measures.  Queued on `stream` as Blur is; the labels (4 bytes per
    // texel of the clipped box) live in the same scratch.
    void Fill(const vr_brush& brush, const vr_fill_rule& rule, vr_fill_report* d_report = nullptr, void* stream = nullptr)
    {
        Check(vr_fill(ctx_, &brush, &rule, d_report, stream), "vr_fill");
    }
    // Paint under the brush with the volume's own texels from elsewhere
    // (vr_clone): the value of texel t is the texel at t + map.offset (per
    // axis map.offset - t where map.mirror is 1), clamped to the volume, as it
    // was before the call -- clone stamp, push, mirror.  Queued on `stream` as
    // Paint is; a source that meets the brush's box goes through Blur's
    // staging scratch.
    void Clone(const vr_brush& brush, const vr_clone_map& map, void* stream = nullptr)
    {
        Check(vr_clone(ctx_, &brush, &map, stream), "vr_clone");
    }
    // Paint under the brush with the texels of a device RGBA8 box laid on the
    // volume at `placement` (vr_stamp): GetVolumeBoxDevice's format, 4-byte
    // aligned, alive until the launch has run.  One launch on `stream`;
    // StampBox names the box it edits.
    void Stamp(const vr_brush& brush, const void* d_rgba, const vr_box& placement, void* stream = nullptr)
    {
        Check(vr_stamp(ctx_, &brush, d_rgba, &placement, stream), "vr_stamp");
    }
    // Paste a device RGBA8 box of sbx x sby x sbz texels through an affine map
    // and a filter (vr_stamp_affine): rotated, scaled, sheared or shifted by a
    // fraction of a texel.  One launch on `stream`; vr_brush_box names the box
    // it edits.
    void StampAffine(const vr_brush& brush, const void* d_rgba, int sbx, int sby, int sbz, const vr_affine& map,
                     void* stream = nullptr)
    {
        Check(vr_stamp_affine(ctx_, &brush, d_rgba, sbx, sby, sbz, &map, stream), "vr_stamp_affine");
    }
    // The same with the volume itself, as it was before the call, as the
    // source (vr_clone_affine): one launch when the read range misses the box,
    // else vr_blur's staging scratch and commit.
    void CloneAffine(const vr_brush& brush, const vr_affine& map, void* stream = nullptr)
    {
        Check(vr_clone_affine(ctx_, &brush, &map, stream), "vr_clone_affine");
    }
    // Liquify (vr_warp): what is under the brush (op VR_BRUSH_SET) moves along
    // `map` -- WarpPush for a push, AffinePlace about the brush centre for a
    // pinch, a bloat or a twirl -- by an amount that fades out towards the rim.
    // vr_blur's staging scratch and commit; vr_brush_box names the edited box.
    void Warp(const vr_brush& brush, const vr_affine& map, void* stream = nullptr)
    {
        Check(vr_warp(ctx_, &brush, &map, stream), "vr_warp");
    }
    // Paint under the brush with a function of each texel's own byte
    // (vr_remap): the value of channel c is lut.lut[c][old byte] -- levels,
    // invert, threshold, equalise.  The host table is copied during the call.
    // Queued on `stream` as Paint is: one launch, no scratch.
    void Remap(const vr_brush& brush, const vr_lut& lut, void* stream = nullptr)
    {
        Check(vr_remap(ctx_, &brush, &lut, stream), "vr_remap");
    }
    // The same with a DEVICE vr_lut (vr_remap_device; 4-byte aligned), read when
    // the kernel runs: a table written earlier on `stream` is the one applied.
    void RemapDevice(const vr_brush& brush, const void* d_lut, void* stream = nullptr)
    {
        Check(vr_remap_device(ctx_, &brush, d_lut, stream), "vr_remap_device");
    }
    // A device table from a device vr_volume_stats (vr_stats_lut_device): what
    // BrushStats / BoxStats wrote -> what RemapDevice takes, on one stream.
    void StatsLutDevice(const void* d_stats, int kind, int channel_mask, void* d_lut, void* stream = nullptr) const
    {
        Check(vr_stats_lut_device(ctx_, d_stats, kind, channel_mask, d_lut, stream), "vr_stats_lut_device");
    }
    // The read-back counterpart of UpdateVolume (vr_get_volume_box): save a
    // box, Paint, UpdateVolume the saved box -- undo.
    void GetVolumeBox(int x0, int y0, int z0, int bx, int by, int bz, uint8_t* rgba_out) const
    {
        Check(vr_get_volume_box(ctx_, x0, y0, z0, bx, by, bz, rgba_out), "vr_get_volume_box");
    }
    void GetVolumeBoxDevice(int x0, int y0, int z0, int bx, int by, int bz, void* d_rgba_out,
                            void* stream = nullptr) const
    {
        Check(vr_get_volume_box_device(ctx_, x0, y0, z0, bx, by, bz, d_rgba_out, stream), "vr_get_volume_box_device");
    }
    // What is in the installed volume under the brush, or in a texel box
    // (vr_brush_stats, vr_box_stats): count, weight, weighted sums and
    // histograms of the selected channels into a DEVICE vr_volume_stats, which
    // the call overwrites.  Queued on `stream`; nothing of the renderer changes.
    // vr_stats_summary reads min / max / mean / median and the eyedropper's
    // value off a copy on the host.
    void BrushStats(const vr_brush& brush, void* d_stats, void* stream = nullptr) const
    {
        Check(vr_brush_stats(ctx_, &brush, d_stats, stream), "vr_brush_stats");
    }
    void BoxStats(int x0, int y0, int z0, int bx, int by, int bz, int channel_mask, void* d_stats,
                  void* stream = nullptr) const
    {
        Check(vr_box_stats(ctx_, x0, y0, z0, bx, by, bz, channel_mask, d_stats, stream), "vr_box_stats");
    }
    void GenerateVolume(const vr_volume_recipe& r, void* stream = nullptr)
    {
        Check(vr_generate_volume(ctx_, &r, stream), "vr_generate_volume");
    }
    void UpdateObjectData(const ObjectShaderData& o)
    {
        osd_ = o;
        has_osd_ = true;
        Flush();
    }
    void UpdateGlobalData(const GlobalShaderData& g)
    {
        gsd_ = g;
        has_gsd_ = true;
        Flush();
    }
    void SetMarch(const vr_march_params& m) { Check(vr_set_march(ctx_, &m), "vr_set_march"); }
    // BASELINE configs 2/3: the procedural medium replaces the volume (enabled = 0 restores it)
    void SetProcedural(const vr_procedural& p) { Check(vr_set_procedural(ctx_, &p), "vr_set_procedural"); }
    void SetOption(const char* name, int value) { Check(vr_set_option(ctx_, name, value), "vr_set_option"); }

    // Render the whole frame (or a band set) into a device buffer.
    void EnqueueRenderPass(const Rect2D& rect, vr_format fmt, void* d_pixels, void* stream = nullptr,
                           uint64_t* d_step_counter = nullptr, int band_rows = 0, int band_stride = 1,
                           int band_first = 0, int band_flip = 0)
    {
        vr_target t{};
        t.width = rect.width;
        t.height = rect.height;
        t.format = fmt;
        t.band_rows = band_rows;
        t.band_stride = band_stride;
        t.band_first = band_first;
        t.band_flip = band_flip;   // vr.h: odd bands of the set shifted (the serpentine deal)
        t.pixels = d_pixels;
        t.row_pitch = 0;
        t.step_counter = d_step_counter;
        Check(vr_render(ctx_, &t, stream), "vr_render");
    }
    // Two queued frames in one launch (vr_render_pair): frame i into d_pixels[i]
    // with (osd[i], gsd[i]); osd = gsd = nullptr renders both with the current
    // shader data.  The same bytes as two EnqueueRenderPass calls.
    void EnqueueRenderPassPair(const Rect2D& rect, vr_format fmt, void* const d_pixels[2],
                               const vr_object_shader_data* osd = nullptr, const vr_global_shader_data* gsd = nullptr,
                               void* stream = nullptr, uint64_t* d_step_counter = nullptr, int band_rows = 0,
                               int band_stride = 1, int band_first = 0, int band_flip = 0)
    {
        vr_target t[2] = {};
        for (int i = 0; i < 2; ++i) {
            t[i].width = rect.width;
            t[i].height = rect.height;
            t[i].format = fmt;
            t[i].band_rows = band_rows;
            t[i].band_stride = band_stride;
            t[i].band_first = band_first;
            t[i].band_flip = band_flip;
            t[i].pixels = d_pixels[i];
            t[i].step_counter = d_step_counter;
        }
        Check(vr_render_pair(ctx_, &t[0], &t[1], osd, gsd, stream), "vr_render_pair");
    }
    // vkCmdSetScissor + the draw: render only the pixels `scissor` of the whole
    // frame `frame` in d_pixels (vr_render_rect); the rest of it is untouched.
    void RenderRect(const Rect2D& frame, const vr_rect& scissor, vr_format fmt, void* d_pixels, void* stream = nullptr,
                    uint64_t* d_step_counter = nullptr, size_t row_pitch = 0)
    {
        vr_target t{};
        t.width = frame.width;
        t.height = frame.height;
        t.format = fmt;
        t.pixels = d_pixels;
        t.row_pitch = row_pitch;
        t.step_counter = d_step_counter;
        Check(vr_render_rect(ctx_, &t, &scissor, stream), "vr_render_rect");
    }
    // The scissor for a list: the union of scissors[0..count) in ONE launch, a
    // pixel that several of them cover marched, stored and counted once
    // (vr_render_rects; at most VR_MAX_RECTS -- CoalesceRects shortens a list).
    // The K-edit loop: UpdateVolume K boxes, UpdateFootprint each, RenderRects.
    void RenderRects(const Rect2D& frame, const vr_rect* scissors, int count, vr_format fmt, void* d_pixels,
                     void* stream = nullptr, uint64_t* d_step_counter = nullptr, size_t row_pitch = 0)
    {
        vr_target t{};
        t.width = frame.width;
        t.height = frame.height;
        t.format = fmt;
        t.pixels = d_pixels;
        t.row_pitch = row_pitch;
        t.step_counter = d_step_counter;
        Check(vr_render_rects(ctx_, &t, scissors, count, stream), "vr_render_rects");
    }
    void RenderRects(const Rect2D& frame, const std::vector<vr_rect>& scissors, vr_format fmt, void* d_pixels,
                     void* stream = nullptr, uint64_t* d_step_counter = nullptr, size_t row_pitch = 0)
    {
        RenderRects(frame, scissors.data(), (int)scissors.size(), fmt, d_pixels, stream, d_step_counter, row_pitch);
    }
    // The pixels of `frame` that an UpdateVolume of this texel box can change
    // (vr_update_footprint): UpdateVolume, then RenderRect of it, gives the
    // patched volume's whole frame.
    vr_rect UpdateFootprint(const Rect2D& frame, int x0, int y0, int z0, int bx, int by, int bz) const
    {
        vr_rect r{};
        Check(vr_update_footprint(ctx_, frame.width, frame.height, x0, y0, z0, bx, by, bz, &r), "vr_update_footprint");
        return r;
    }
    // The opposite question: which part of the volume does a pixel see?  One
    // vr_ray_record per pixel of `scissor` into the device buffer d_records
    // (scissor.height rows of row_pitch_records records, 0 = scissor.width):
    // steps, depth, the render's R32F value and, with a transmittance
    // `threshold`, the first step and point that pass it (vr_query_rect).
    void QueryRect(const Rect2D& frame, const vr_rect& scissor, float threshold, vr_ray_record* d_records,
                   size_t row_pitch_records = 0, void* stream = nullptr)
    {
        Check(vr_query_rect(ctx_, frame.width, frame.height, &scissor, threshold, d_records, row_pitch_records, stream),
              "vr_query_rect");
    }
    const char* KernelVariant() const { return vr_kernel_variant(ctx_); }
    void* Handle() const { return ctx_; }

    static void ReferenceShaderData(float aspect, float phi_deg, float theta_deg, float frame_time,
                                    ObjectShaderData* o, GlobalShaderData* g)
    {
        Check(vr_reference_shader_data(aspect, phi_deg, theta_deg, frame_time, o, g),
              "vr_reference_shader_data");
    }

private:
    void Flush()
    {
        if (has_osd_ && has_gsd_) Check(vr_set_shader_data(ctx_, &osd_, &gsd_), "vr_set_shader_data");
    }
    void* ctx_ = nullptr;
    ObjectShaderData osd_{};
    GlobalShaderData gsd_{};
    bool has_osd_ = false, has_gsd_ = false;
};

}  // namespace vr
