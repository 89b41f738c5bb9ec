// vr_march.hip -- the hot path: per-pixel volumetric ray march for gfx950.
//
// Replaces shaders/frag.glsl:34-81 (and the coverage that vert.glsl:17-22
// plus rasterisation provide).  Each lane traces one ray and a wave64 owns an
// 8x8 pixel tile.  The work is gather + fp32 VALU; there is no dense
// contraction, so nothing here uses MFMA.
//
// The op sequence is the fp32 spec of DESIGN.md sec. 3.  The oracle
// (oracle/vr_oracle.c) restates the same spec, and results agree bit for bit.
// Packed fp32 ops (v_pk_fma_f32 / v_pk_add_f32) compute two independent IEEE
// lerps per instruction.  Built with -ffp-contract=off: the only fused ops
// are the explicit fma calls.
#include "vr_march_kernels.h"
#include "vr_proc_kernels.h"

namespace vr {

SortLayout sort_layout(int width, int out_rows)
{
    // hist, cursor (+ total), order (u32 per pixel), keys (u16 per enumerated
    // position: whole 64x64 regions, kSortRegion), then the deferred shadow
    // passes' per-wave prefixes (proc_scan) and the frame's totals
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    SortLayout L{};
    const size_t pixels = (size_t)width * (size_t)out_rows;
    const size_t regions = (size_t)((width + kSortRegion - 1) / kSortRegion) * ((out_rows + kSortRegion - 1) / kSortRegion);
    L.waves = (unsigned)((pixels + 63) / 64);
    L.hist = 0;
    L.cursor = kKeyBins * sizeof(unsigned);
    L.order = (size_t)(2 * kKeyBins + 64) * sizeof(unsigned);
    L.keys = L.order + pixels * 4u;
    L.went = up(L.keys + regions * kSortRegion * kSortRegion * 2u);
    L.wrec = up(L.went + ((size_t)L.waves + 1) * sizeof(unsigned long long));
    L.need = up(L.wrec + ((size_t)L.waves + 1) * sizeof(unsigned));
    L.bytes = L.need + 2 * sizeof(unsigned long long);
    return L;
}

hipError_t launch_march_procedural(const MarchArgs& a, bool early, void* sort_buf, int reuse_sort, const Schedule& sc,
                                   hipStream_t s, const ShadowDefer* defer, unsigned long long* need_host)
{
    if (a.width <= 0 || a.out_rows <= 0) return hipSuccess;
    const bool shadow = a.proc.shadow_steps > 0;
    const size_t wt_bytes = worley_table_bytes(a.proc);
    if (sort_buf) {
        const SortLayout L = sort_layout(a.width, a.out_rows);
        char* sb = static_cast<char*>(sort_buf);
        unsigned* hist = reinterpret_cast<unsigned*>(sb + L.hist);
        unsigned* cursor = reinterpret_cast<unsigned*>(sb + L.cursor);   // kKeyBins + 1 entries
        unsigned* order = reinterpret_cast<unsigned*>(sb + L.order);
        unsigned short* keys = reinterpret_cast<unsigned short*>(sb + L.keys);
        // hist is all zero here: zeroed when the buffer was allocated, and by
        // the previous frame's proc_scan after it read it
        const long long pixels = (long long)a.width * a.out_rows;
        static_assert(kSortRegion * kSortRegion == 256 * kSortPixelsPerThread, "one 64x64 region per sort block");
        const dim3 g1((unsigned)(((a.width + kSortRegion - 1) / kSortRegion) * ((a.out_rows + kSortRegion - 1) / kSortRegion)));
        // same geometry as the frame that built keys / order / total: only the
        // pixels without steps need writing, by trailing blocks of the march
        const unsigned positions = reuse_sort != SORT_BUILD ? g1.x * 256u * kSortPixelsPerThread : 0u;
        if (reuse_sort == SORT_BUILD) {
            if (shadow) hipLaunchKernelGGL((proc_bin<true>), g1, dim3(256), 0, s, a, hist, keys);
            else hipLaunchKernelGGL((proc_bin<false>), g1, dim3(256), 0, s, a, hist, keys);
            // with shadow rays proc_scan also lays out the deferred passes' per-wave ranges
            ScanOut so{};
            if (shadow) {
                so.went = reinterpret_cast<unsigned long long*>(sb + L.went);
                so.wrec = reinterpret_cast<unsigned*>(sb + L.wrec);
                so.need = reinterpret_cast<unsigned long long*>(sb + L.need);
                so.need_host = need_host;
                so.max_steps = a.max_steps;
            }
            hipLaunchKernelGGL(proc_scan, dim3(1), dim3(kKeyBins), 0, s, hist, cursor, so);
            hipLaunchKernelGGL(proc_scatter, g1, dim3(256), 0, s, a, keys, cursor, order);
        }
        // the scatter advanced cursor[k] to the end of key k; total stays at cursor[kKeyBins]
        const unsigned march_blocks = (unsigned)((pixels + kThreads - 1) / kThreads);
        const dim3 g4(march_blocks + (positions + kThreads * 16 - 1) / (kThreads * 16));
        const unsigned* total = cursor + kKeyBins;
        // tables: 2 = the fixed 9-cell Worley geometry (compile-time offsets), 1 = runtime geometry,
        // 3 = 2 + the Perlin lattice table
        const int tm = wt_bytes ? (a.proc.wt_fixed ? (a.proc.lat ? 3 : 2) : 1) : 0;
        const bool stale = reuse_sort == SORT_STALE;
        if (shadow && defer && tm >= 2) {   // deferred shadow rays: three passes (vr_proc_kernels.h)
            const ShadowDefer d = *defer;
            const dim3 eval_grid(d.eval_blocks ? d.eval_blocks : kShadowEvalBlocks);
            return with_value<2, 3>(tm, [&](auto T) {
                with_bool(early, [&](auto E) {
                    hipLaunchKernelGGL((march_proc_defer<E, T>), g4, dim3(kThreads), wt_bytes, s, a, order, total, keys,
                                       positions, march_blocks, stale, d);
                });
                hipLaunchKernelGGL(proc_shadow_scan, dim3(1), dim3(kScanThreads), 0, s, total, d);
                hipLaunchKernelGGL(proc_shadow_map, dim3((d.waves + 3) / 4), dim3(kThreads), 0, s, total, d);
                if (d.worley_cache == 2)
                    hipLaunchKernelGGL((proc_shadow_eval8<T>), eval_grid, dim3(kThreads), wt_bytes, s, a, d);
                else
                    with_bool(d.worley_cache != 0, [&](auto C) {
                        hipLaunchKernelGGL((proc_shadow_eval<T, C>), eval_grid, dim3(kThreads), wt_bytes, s, a, d);
                    });
                hipLaunchKernelGGL(proc_shadow_resolve, dim3(march_blocks), dim3(kThreads), 0, s, a, order, total, d);
                return hipGetLastError();
            }, hipErrorInvalidValue);
        }
        return with_bool(shadow, [&](auto S) { return with_bool(early, [&](auto E) {
            return with_value<0, 1, 2, 3>(tm, [&](auto T) {
                hipLaunchKernelGGL((march_proc_sorted<S, E, T>), g4, dim3(kThreads), wt_bytes, s, a, order, total, keys,
                                   positions, march_blocks, stale);
                return hipGetLastError();
            }, hipErrorInvalidValue);
        }); });
    }
    const int tiles_x8 = (a.width + 7) >> 3, rows8 = (a.out_rows + 7) >> 3;
    long long waves = (long long)tiles_x8 * rows8;
    int cx = -1, cy = -1;
    if (sc.kind == SCHED_RINGS) {
        cx = min(max(sc.center_x >> 3, 0), tiles_x8 - 1);
        cy = min(max(sc.center_y >> 3, 0), rows8 - 1);
        const int R = max(max(cx, tiles_x8 - 1 - cx), max(cy, rows8 - 1 - cy));
        waves = (2ll * R + 1) * (2ll * R + 1);
    }
    const dim3 grid((unsigned)((waves + 3) / 4)), block(kThreads);
    // the fixed geometry is also a valid runtime geometry (n = 9, pz = 83)
    return with_proc_variant(a, early, [&](auto S, auto E, auto T, size_t wt) {
        hipLaunchKernelGGL((march_proc<S, E, T>), grid, block, wt, s, a, cx, cy);
    });
}

hipError_t launch_march(const MarchArgs& a, int layout, int wrap, bool early, const Schedule& sc, hipStream_t s)
{
    if (a.width <= 0 || a.out_rows <= 0) return hipSuccess;
    if (list_has(CornerLayouts{}, layout)) return launch_march_corner8(a, layout, early, sc, s);   // vr_march_c8.hip
    return with_layout_wrap<MarchLayouts>(layout, wrap, [&](auto L, auto W) {
        if constexpr (L == LAYOUT_COL48)
            if (sc.kind == SCHED_REGIONS && sc.slab && sc.split <= 1) return launch_march_slab(a, early, sc, s);
        return launch_lw<L, W>(a, early, sc, s);
    });
}

hipError_t launch_march_frames(const MarchArgs& a, const FrameArgs* fr, int nf, int layout, bool early, const Schedule& sc,
                               int deal, int quad, hipStream_t s)
{
    if (a.width <= 0 || a.out_rows <= 0) return hipSuccess;
    // a layout without a multi-frame kernel is an error: the caller renders the frames one by one
    return with_layout<FrameLayouts>(layout, [&](auto L) {
        if constexpr (list_has(CornerLayouts{}, L)) return launch_march_frames_cornerh(a, fr, nf, early, sc, deal, quad, s);   // vr_march_c8.hip
        else return launch_frames_l<L, WRAP_CLAMP>(a, fr, nf, early, sc, deal, quad, s);
    });
}

}  // namespace vr

#ifdef VR_TIMELINE
// timing experiments only (make timeline): copy / clear the per-wave records
// of the regions kernels compiled in this translation unit
extern "C" int vr_timeline_fetch(unsigned long long* host, int waves)
{
    waves = waves < vr::kTimelineWaves ? waves : vr::kTimelineWaves;
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(vr::g_timeline), (size_t)waves * 3 * sizeof(unsigned long long));
}
extern "C" int vr_timeline_clear()
{
    static unsigned long long zero[vr::kTimelineWaves][3];
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(vr::g_timeline), zero, sizeof(zero));
}
#endif
