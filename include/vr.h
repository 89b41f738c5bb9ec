/*
 * vr.h -- C-ABI of the MI355X-native volumetric ray-march integrator
 *         (libvr.so, built from volumetricrenderer_amd/csrc/).
 *
 * The reference runs its hot path, shaders/frag.glsl, behind the Vulkan
 * render-pass / descriptor API.  Each entry point below
 * replaces one piece of that API; the reference interface it replaces is cited
 * in the comment above it.  Plain C types only: device buffers are passed as
 * void*, streams as void* (hipStream_t), no torch and no C++ types.
 *
 * Errors: every call returns a vr_status.  0 is success.  On failure,
 * vr_last_error() holds a message for the calling thread.  Exceptions never
 * cross the ABI.  (The reference instead throws from Error(), Utils.h:22-29.)
 *
 * Threading: one vr_ctx per device and host thread.  Calls on one vr_ctx are
 * not reentrant.  vr_render is asynchronous on the given stream.  It does not
 * allocate or synchronise, so a caller may capture it in a hipGraph -- except
 * that the first vr_render after a volume install waits (host) for that
 * install's uniform-channel scan (a few microseconds of GPU work queued with
 * the install), and the first procedural render of a
 * larger target allocates the context's cost-sort scratch (with shadow rays
 * also the deferred-shadow scratch, option "shadow_defer") after a device
 * synchronisation.  That scratch belongs to the context.  vr_render orders
 * procedural renders of one vr_ctx across streams itself: a frame that
 * writes the scratch (a new cost order, deferred shadow rays) waits for every
 * earlier procedural render, and a frame that only reads it (the same camera's
 * order) waits for the last writer, so readers overlap on alternating streams.
 */
#ifndef VR_H
#define VR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_ABI_VERSION 2

typedef enum {
    VR_OK = 0,
    VR_ERR_INVALID = 1,     /* bad argument (null pointer, bad size or enum) */
    VR_ERR_HIP = 2,         /* HIP runtime error (see vr_last_error)       */
    VR_ERR_NO_VOLUME = 3,   /* vr_render before vr_set_volume/generate     */
    VR_ERR_NO_CAMERA = 4,   /* vr_render before vr_set_shader_data         */
    VR_ERR_OOM = 5,         /* device allocation failed                    */
    VR_ERR_NO_DEVICE = 6,   /* no HIP device / bad device index            */
    VR_ERR_TIMEOUT = 7,     /* a collective (vr_shard.h) missed its deadline; communicator aborted */
    VR_ERR_COMM = 8         /* communicator error (RCCL, vr_shard.h); communicator aborted */
} vr_status;

typedef enum {
    VR_FMT_RGBA32F = 0,      /* 16 B/pixel, linear                          */
    VR_FMT_RGBA8_UNORM = 1,  /* 4 B/pixel, linear, round-to-nearest-even    */
    VR_FMT_RGBA8_SRGB = 2,   /* 4 B/pixel, sRGB-encoded on store, as the
                                reference's swapchain format
                                (VulkanSwapchain.cpp:181-191)               */
    /* Grey targets: frag.glsl:79-80 writes vec4(vec3(c), 1.0), so one channel
     * holds the whole pixel.  The value is the RGBA format's R (bit for bit);
     * G = B = R and A = 1 (255) are implied.  The multi-GPU band sets travel
     * in these (vr_shard.h), and vr_assemble_frame expands them.           */
    VR_FMT_R8_UNORM = 3,     /* 1 B/pixel: VR_FMT_RGBA8_UNORM's R           */
    VR_FMT_R8_SRGB = 4,      /* 1 B/pixel: VR_FMT_RGBA8_SRGB's R            */
    VR_FMT_R32F = 5          /* 4 B/pixel: VR_FMT_RGBA32F's R               */
} vr_format;

/* Replaces the binding-0 UBO `ObjectShaderData` (TestMain.cpp:27-32,
 * vert.glsl:4-9).  Column-major mat4, as in GLM.  192 bytes.              */
typedef struct {
    float model[16];
    float view[16];
    float projection[16];
} vr_object_shader_data;

/* Replaces the binding-1 UBO `GlobalShaderData` (TestMain.cpp:34-39,
 * frag.glsl:9-14).  The std140 layout is made explicit: the vec3 is padded
 * to 16 bytes, so media_scroll sits at byte 80.  The reference's C++ struct
 * put it at byte 76.  144 bytes.                     */
typedef struct {
    float world_to_local[16];
    float camera_position[3];
    float _pad0;
    float media_scroll[16];
} vr_global_shader_data;

/* Constants that the reference hard-codes in frag.glsl.  Fill it with
 * vr_march_defaults() to get the reference values.                        */
typedef struct {
    int32_t max_steps;      /* frag.glsl:30  maxSteps = 128                 */
    float   step_scale;     /* frag.glsl:42  stepSize = (1/maxSteps) * 4    */
    float   density;        /* frag.glsl:29  density = 1                    */
    float   scale;          /* frag.glsl:63  scale = 0.2                    */
    float   box_min[3];     /* frag.glsl:31  (-1,-1,-1)                     */
    float   box_max[3];     /* frag.glsl:32  ( 1, 1, 1)                     */
    float   tap_scale[4];   /* frag.glsl:66-69  Pin * {1, .8, .75, .7}      */
    float   tap_weight[4];  /* frag.glsl:66-69  MediaScroll * {0,.2,.25,.3} */
    float   early_out;      /* stop a ray once its transmittance is below this
                               value.  0 = off, which is the reference.      */
    int32_t reserved[3];    /* must be 0                                    */
} vr_march_params;

/* The volume recipe of TestMain.cpp:43-92: four FastNoise2-style grids
 * (Cellular f=.01 s1, Cellular f=.03 s2, Perlin f=.19 s3, Simplex f=.15 s4),
 * normalised, inverted, R raised to the 4th power, packed to RGBA8.       */
typedef struct {
    int32_t size;               /* N, for an N^3 volume (TestMain.cpp:51: 128) */
    float   freq[4];            /* TestMain.cpp:59-62                        */
    int32_t seed[4];
    int32_t literal_overwrite;  /* 1: replicate TestMain.cpp:60, where the
                                   f=.03 grid is written into noiseOutput1   */
} vr_volume_recipe;

/* Procedural medium: BASELINE configs 2/3, build-defined extensions with no
 * reference counterpart.  When enabled, vr_render
 * marches a density evaluated in-kernel instead of the volume:
 *   q = P * grid_scale              (P: box point in [0,1]^3)
 *   fbm = sum_o gain^o * perlin(seed_fbm, q * freq0 * lacunarity^o)
 *   F1  = cellular(seed_worley, q * worley_freq) + 1
 *   rho = max(fbm * (1 - F1), 0) * march.scale
 * With shadow_steps = 0, the output is Beer-Lambert 1 - exp(-density*sum(rho)*ds).
 * With shadow_steps > 0, each step adds single scatter lit from sun_dir
 * (box-local): Tview * rho*ds*density * exp(-density*ds*sum rho_sun), with
 * shadow_steps sun samples at P + k*ds*sun_dir, inside the box only.       */
typedef struct {
    int32_t enabled;
    float   grid_scale;     /* 128 */
    int32_t octaves;        /* 4 */
    float   freq0;          /* 0.19 */
    float   lacunarity;     /* 2 */
    float   gain;           /* 0.5 */
    int32_t seed_fbm;       /* 3 */
    float   worley_freq;    /* 0.03 */
    int32_t seed_worley;    /* 2 */
    int32_t shadow_steps;   /* 0 (config 2) or 8 (config 3) */
    float   sun_dir[3];     /* normalize(1,1,2); normalised by the library */
    int32_t reserved;       /* must be 0 */
} vr_procedural;

/* A render target.  `pixels` is a DEVICE pointer that the caller owns.
 * With band_rows > 0 only bands b = band_first, band_first + band_stride, ...
 * are rendered.  Band b covers frame rows [b*band_rows, (b+1)*band_rows).
 * band_flip (ABI 2) shifts every second band of the set: its k-th band is
 * band_first + k*band_stride + (k odd ? band_flip : 0), |band_flip| <
 * band_stride.  A world of S renderers with flips S-1-2i (renderer i) deals
 * the bands serpentine: forwards in even periods of S bands, backwards in odd
 * ones, so a cost that drifts down the frame does not load one renderer
 * more in every period (vr_shard.h vr_shard_set_serpentine).
 * The bands are written packed and in order, from row 0 of `pixels`; the
 * rows of a last, partial band that lie past `height` are left untouched.
 * This is how the frame is split across GPUs.  band_rows = 0 renders the whole
 * frame.  step_counter (device u64, may be NULL) has the executed ray-steps
 * added to it (the sum of n, frag.glsl:46).                                */
/* OR'ed into vr_target.format with band_rows > 0: each band is written at its
 * own frame rows of `pixels` (a whole-frame buffer, `height` rows) instead of
 * packed from row 0 -- rank 0 of the multi-GPU loop renders its bands straight
 * into the frame (vr_shard.h), and the assembly skips them
 * (vr_assemble_frame_ranks).                                               */
#define VR_TARGET_BANDS_IN_PLACE 0x100
/* OR'ed into vr_target.format: the target is one contiguous range of frame
 * rows, [band_first, band_first + band_rows), instead of a band set.
 * band_first must be a multiple of 8 and band_stride must be 1; rows past
 * `height` are not written.  The rows are packed from row 0 of `pixels`, or
 * stored at their frame rows with VR_TARGET_BANDS_IN_PLACE.  The multi-GPU
 * loop's balanced row ranges (vr_shard.h vr_shard_balance_rows).            */
#define VR_TARGET_ROW_RANGE 0x200

typedef struct {
    int32_t   width, height;
    int32_t   format;        /* vr_format, optionally | VR_TARGET_BANDS_IN_PLACE
                              * and/or VR_TARGET_ROW_RANGE                   */
    int32_t   band_rows, band_stride, band_first;
    void*     pixels;
    size_t    row_pitch;     /* bytes; 0 = tightly packed                  */
    uint64_t* step_counter;
    int32_t   band_flip;     /* 0 = plain band set; see above              */
    int32_t   reserved;      /* must be 0                                  */
} vr_target;

/* ---- context (replaces Renderer::Init/Shutdown, VulkanRenderer.h:68-72) */
vr_status   vr_create(int device, void** out_ctx);
vr_status   vr_destroy(void* ctx);
const char* vr_last_error(void);
int         vr_abi_version(void);
/* Hash of the sources this library was built from (tools/build_id.py; a
 * "-exp" suffix for the VR_EXPERIMENTS build): the tests and smoke() check
 * that the prebuilt library matches the checked-out code.  Static string.  */
const char* vr_build_id(void);

/* ---- volume: replaces vkc::Texture3D(unsigned char*, VkExtent3D)
 *      (VulkanTexture.h:55-60, VulkanTexture.cpp:111-156).  RGBA8 UNORM,
 *      x fastest (the TestMain.cpp:69-73 pack order).  The library copies the
 *      data into its own device layout.  The host call is synchronous.     */
vr_status vr_set_volume(void* ctx, const uint8_t* rgba8, int nx, int ny, int nz);
vr_status vr_set_volume_device(void* ctx, const void* d_rgba8, int nx, int ny, int nz, void* stream);
/* Partial update: the buffer-to-image copy region with a non-zero
 * imageOffset, which the reference never needs (it uploads once, offset 0,
 * full extent).  Overwrite the texel box [x0,x0+bx) x [y0,y0+by) x [z0,z0+bz)
 * of the installed volume with `rgba8` (bx*by*bz RGBA8 texels, tightly
 * packed, x fastest -- the order of vr_set_volume).  Afterwards the ctx
 * renders, and vr_get_volume reads, bit for bit what a vr_set_volume of the
 * whole patched volume would give.  The work follows the box (plus a halo of
 * one texel position in the device layouts), not the volume.
 *
 * VR_ERR_INVALID: a null pointer, a non-positive extent or a box that leaves
 * the volume; VR_ERR_NO_VOLUME before an install.  A refused call leaves the
 * volume untouched.  Dimensions, layout preference and buffers do not change.
 *
 * vr_update_volume is synchronous, like vr_set_volume.  The device variant is
 * asynchronous on `stream`: it allocates nothing and never waits on the host,
 * so `update, render, update, render ...` queues on one stream like the rest
 * of the frame loop.  Renders of the same ctx queued on OTHER streams are the
 * caller's to order against the update (an event, as for any shared buffer);
 * `d_rgba8` must stay valid until the update has run.
 *
 * Uniform channels (option "uniform_mask": every texel of a channel equal,
 * sampled as a constant): an update that breaks one clears its bit before
 * the next render; while a channel is uniform that next render waits on the
 * host once for the check, exactly as after an install.  A channel an update
 * makes uniform AGAIN stays "not uniform" until the next full install -- the
 * output is exact either way, only the loads are not skipped.             */
vr_status vr_update_volume(void* ctx, const uint8_t* rgba8, int x0, int y0, int z0, int bx, int by, int bz);
vr_status vr_update_volume_device(void* ctx, const void* d_rgba8, int x0, int y0, int z0, int bx, int by, int bz, void* stream);
/* read the volume back as RGBA8 (host); for tests and tools             */
vr_status vr_get_volume(void* ctx, uint8_t* rgba8_out);
vr_status vr_volume_dims(void* ctx, int* nx, int* ny, int* nz);
/* The read-back counterpart of vr_update_volume: the texel box [x0,x0+bx) x
 * [y0,y0+by) x [z0,z0+bz) of the installed volume as bx*by*bz RGBA8 texels,
 * tightly packed, x fastest -- what vr_update_volume takes, so saving a box,
 * editing it and handing the saved bytes back restores it (undo).  The box is
 * validated as vr_update_volume validates it and the cost follows the box.
 * The host call is synchronous; the device variant writes to DEVICE memory
 * and is asynchronous on `stream` (no allocation, no host wait).            */
vr_status vr_get_volume_box(void* ctx, int x0, int y0, int z0, int bx, int by, int bz, uint8_t* rgba8_out);
vr_status vr_get_volume_box_device(void* ctx, int x0, int y0, int z0, int bx, int by, int bz, void* d_rgba8_out,
                                   void* stream);

/* ---- the brush: a read-modify-write of the installed volume on the device.
 *      No reference counterpart (the reference uploads its texture once).
 *      vr_update_volume overwrites a box with bytes the caller has finished;
 *      a brush blends into what is there, so an editor needs no read-back:
 *      vr_query_rect (pick) -> vr_paint -> vr_update_footprint ->
 *      vr_render_rect queue on one stream with no host round trip.
 *
 * Everything is defined in integers.  For the texel at
 * offset (dx, dy, dz) from `centre`, with D_a = 2 radius[a] + 1, in unsigned
 * 64-bit arithmetic:
 *   S = Dx^2 Dy^2 Dz^2
 *   Q = (2dx)^2 Dy^2 Dz^2 + (2dy)^2 Dx^2 Dz^2 + (2dz)^2 Dx^2 Dy^2
 * The texel is inside iff |d_a| <= radius[a] on every axis and Q <= S; radius
 * (0, 0, 0) is exactly one texel.  Weight w = 256 for a hard edge (falloff 0);
 * for a smooth one (falloff 1) w = 256 - (256 Q) / (S + 1), integer division:
 * 256 at the centre, 1 on the rim.  Per channel c, a = w * strength[c]
 * (0..65280) and d = (value[c] a + 32640) / 65280:
 *   VR_BRUSH_SET  new = (old (65280 - a) + value[c] a + 32640) / 65280
 *   VR_BRUSH_ADD  new = min(255, old + d)
 *   VR_BRUSH_SUB  new = max(0, old - d)
 * Texels outside the ellipsoid, and texels of it outside the volume, are not
 * touched; a channel with strength 0 is neither read nor written.           */
typedef enum { VR_BRUSH_SET = 0, VR_BRUSH_ADD = 1, VR_BRUSH_SUB = 2 } vr_brush_op;
#define VR_BRUSH_MAX_RADIUS 255
typedef struct {              /* 48 bytes */
    int32_t centre[3];        /* texel (x, y, z); may lie outside the volume */
    int32_t radius[3];        /* semi-axes in texels, 0..VR_BRUSH_MAX_RADIUS; per axis,
                                 because a non-cubic volume fills the same [0,1]^3 box */
    int32_t op;               /* vr_brush_op */
    int32_t falloff;          /* 0 = hard edge, 1 = smooth (linear in squared distance) */
    uint8_t value[4];         /* per channel R, G, B, A */
    uint8_t strength[4];      /* per channel, 0..255; 0 leaves the channel as it is */
    int32_t reserved[2];      /* must be 0 */
} vr_brush;
/* Apply the brush to the installed volume, in place.  Afterwards the ctx
 * renders, and vr_get_volume reads, bit for bit what a vr_set_volume of the
 * painted volume would give.  The contract is vr_update_volume_device's:
 * asynchronous on `stream`, nothing allocated, no host wait; the device
 * layouts are rebuilt over the brush's clipped bounding box (plus the halo);
 * cached launches, region lists and the uniform-channel read-back are treated
 * exactly as the update treats them -- the new bytes are folded into the
 * channels' byte ranges, so a uniform channel the brush changes loses its bit
 * before the next render, and one it leaves alone (strength 0, or a result
 * equal to what was there) keeps it.  A brush that misses the volume is VR_OK
 * and launches nothing.
 * VR_ERR_INVALID: a null pointer, a bad op or falloff, a radius outside
 * 0..VR_BRUSH_MAX_RADIUS, non-zero reserved; VR_ERR_NO_VOLUME before an
 * install and while a procedural medium is enabled.  A refused call leaves
 * the volume untouched.                                                     */
vr_status vr_paint(void* ctx, const vr_brush* brush, void* stream);
/* The brush's bounding box [centre - radius, centre + radius] clipped to an
 * nx x ny x nz volume: what vr_paint (and vr_blur, below) rewrites, and what
 * to hand to vr_update_footprint.  extent = (0, 0, 0) (and origin 0) when the brush
 * misses the volume.  Pure host code: no context, no device.  The brush is
 * validated as by vr_paint; VR_ERR_INVALID also for a non-positive dimension. */
vr_status vr_brush_box(const vr_brush* brush, int nx, int ny, int nz, int origin[3], int extent[3]);
/* The same brush applied to a HOST RGBA8 volume (x fastest, the order of
 * vr_set_volume), for callers without a device: the CPU statement of the
 * arithmetic above, which vr_paint reproduces bit for bit.  Pure host code.  */
vr_status vr_brush_apply(const vr_brush* brush, uint8_t* rgba8, int nx, int ny, int nz);

/* A brush stroke: dabs[0..count) applied in ONE paint launch.  Afterwards the
 * ctx renders, and vr_get_volume reads, bit for bit what
 *   for (i = 0; i < count; ++i) vr_paint(ctx, &dabs[i], stream);
 * would leave -- the order of the list included (SET then ADD is not ADD then
 * SET) -- but every texel is loaded and stored once, however many dabs cover
 * it, and the device layouts are rebuilt over at most 8 boxes that cover the
 * dabs' clipped bounding boxes (vr_boxes_coalesce), not dab by dab.
 * Everything else is vr_paint's contract: asynchronous on `stream`, nothing
 * allocated, no host wait, region lists untouched, cached launches and the
 * uniform-channel read-back treated as after an update.
 *
 * Uniform channels: only the FINAL byte of each texel the stroke touched is
 * folded into the channels' byte ranges, not the intermediate ones.  A channel
 * whose texels all end equal to its uniform value keeps its bit (strength 0;
 * an ADD undone by a later SUB); one with a changed final byte loses it before
 * the next render.  The stroke may thus keep a bit that count separate
 * vr_paint calls would have dropped; the output is exact either way (see
 * vr_update_volume), only the loads are skipped.
 *
 * count == 0 is VR_OK and launches nothing (dabs may then be NULL).  Dabs that
 * miss the volume are dropped; if all miss, VR_OK and no launch.
 * VR_ERR_INVALID: a null ctx, count < 0, count > VR_MAX_DABS, dabs NULL with
 * count > 0, ANY dab vr_paint would refuse (the message names its index);
 * VR_ERR_NO_VOLUME as for vr_paint.  A refused call has launched nothing, not
 * even the valid dabs before the bad one.  More than VR_MAX_DABS dabs: split
 * the list.                                                                 */
#define VR_MAX_DABS 64
vr_status vr_paint_stroke(void* ctx, const vr_brush* dabs, int count, void* stream);
/* The dabs of a drag from brush->centre to the texel `to`.  With d = to -
 * centre per axis (64 bits) and n = max(1, ceil(max_a |d_a| / spacing)), dab
 * i = 0..n is a copy of `brush` whose centre is moved by
 * floor((2 i d_a + n) / (2 n)) on axis a (floor division, also for negative
 * numerators: the nearest texel of the segment, halves upwards); dab 0 is the
 * brush itself and dab n is centred on `to`.  skip_first = 1 omits dab 0, so
 * that the joint of two segments is not dabbed twice.  *out_count is the
 * number of dabs required, n + 1 - skip_first; they are written to `out`
 * (room for max_out).  Pure host code: no context, no device.
 * VR_ERR_INVALID: a null brush, to or out_count, a brush vr_paint would
 * refuse, spacing < 1, skip_first not 0 or 1, n above 2^20, max_out < 0, out
 * NULL with max_out > 0, and more dabs than max_out -- nothing is then written
 * to `out` and *out_count is still the number required (max_out = 0 asks for
 * the number alone); for every other refusal *out_count, when given, is 0.  */
vr_status vr_brush_line(const vr_brush* brush, const int32_t to[3], int spacing, int skip_first, vr_brush* out,
                        int max_out, int* out_count);
/* A texel box [x, x + bx) x [y, y + by) x [z, z + bz) */
typedef struct { int32_t x, y, z, bx, by, bz; } vr_box;
/* vr_rects_coalesce in three dimensions, with volumes in place of areas:
 * writes at most max_out (>= 1) boxes to `out` (room for min(count, max_out))
 * and their number to *out_count.  Their union contains the union of the
 * input, and each lies inside the bounding box of the non-empty inputs.  Empty
 * inputs are dropped, and so are inputs contained in another input (of
 * identical ones the first is kept); what remains keeps its order.  While more
 * than max_out remain, the pair whose bounding box adds the least volume
 * beyond the two boxes' own volumes is merged into that bounding box, at the
 * place of the pair's first (ties: the lowest pair of indices), and whatever
 * the new box contains is dropped.  Deterministic; edges and sums in 64 bits,
 * volumes (up to 2^93) in 128.  Pure host code: no context, no device; lists
 * of up to VR_MAX_DABS boxes allocate nothing.  vr_paint_stroke uses it for
 * its layout rebuilds.
 * VR_ERR_INVALID: count < 0, max_out < 1, a null pointer with count > 0, a
 * negative coordinate or extent, x + bx, y + by or z + bz above INT32_MAX.
 * count == 0 is VR_OK; *out_count, when given, is then 0.                  */
vr_status vr_boxes_coalesce(const vr_box* in, int count, int max_out, vr_box* out, int* out_count);

/* The smoothing brush: a box filter under the brush.
 * vr_blur is a VR_BRUSH_SET brush whose value, per texel and channel, is the
 * mean of that channel over the texel's neighbourhood AS IT WAS BEFORE THE
 * CALL.  In integers, with h = half_width in 1..VR_BLUR_MAX_HALF and
 * N = (2h + 1)^3 (27, 125, 343): for a texel t inside the ellipsoid and the
 * volume (the inside test and the weight w are the brush's, above) and a
 * channel c with strength[c] != 0,
 *   sum = the sum of channel c over the N texels at offsets -h..h per axis
 *         from t, coordinates clamped to the volume (clamp-to-edge);
 *         neighbours outside the brush's box are read like any other
 *   m   = (sum + N / 2) / N                  (integer division, 0..255)
 *   new = (old (65280 - a) + m a + 32640) / 65280,  a = w * strength[c]
 * -- the SET blend, unchanged.  brush->op must be VR_BRUSH_SET; brush->value
 * is not read.  Every mean is taken over the bytes before the call, whatever
 * the order in which texels are processed (a Jacobi step, not an in-place
 * sweep), so the result is deterministic and the host statement and the device
 * agree bit for bit.  A channel whose texels are all equal has m = old
 * everywhere: a blur never breaks a uniform channel.
 *
 * Device path: two launches on `stream` -- the new bytes of the clipped box
 * are staged in a scratch buffer that belongs to the context, then committed
 * to the planes -- followed by what follows vr_paint: the layout rebuild over
 * the clipped box (vr_brush_box names it; hand it to vr_update_footprint) and
 * the uniform-channel re-arm.  The scratch holds one byte per texel of the
 * clipped box and painted channel (at most 4 x the volume).  A call that needs
 * more than the context holds synchronises the device, frees the old buffer
 * and allocates the need rounded up to 1 MiB -- the rule of the cost-sort
 * scratch (top of this file); VR_ERR_OOM if that fails: nothing is then held
 * and the volume is untouched.  Every other call allocates nothing and never
 * waits on the host, so pick -> vr_blur -> vr_update_footprint ->
 * vr_render_rect queue on one stream.  vr_set_option("blur_scratch_kib", k)
 * reserves at least k KiB now, after a device synchronisation (0 frees it);
 * vr_get_option returns the KiB held.  The scratch is kept across volume
 * installs and freed by vr_destroy.  Two vr_blur calls of one ctx on DIFFERENT
 * streams share it: they are the caller's to order, as renders against
 * updates are.
 * VR_ERR_INVALID: a null pointer, anything vr_paint refuses, op other than
 * VR_BRUSH_SET, half_width outside 1..VR_BLUR_MAX_HALF; VR_ERR_NO_VOLUME
 * before an install and while a procedural medium is enabled.  A brush that
 * misses the volume is VR_OK and launches nothing.  A refused call has
 * launched nothing and leaves the volume untouched.                         */
#define VR_BLUR_MAX_HALF 3
vr_status vr_blur(void* ctx, const vr_brush* brush, int half_width, void* stream);
/* The same on a HOST RGBA8 volume (x fastest), as vr_brush_apply is for
 * vr_paint: the CPU statement, which vr_blur reproduces bit for bit.  It works
 * from a copy of the clipped box and its halo, never in place.  Pure host
 * code.  VR_ERR_INVALID as above, and for a non-positive dimension.         */
vr_status vr_brush_blur_apply(const vr_brush* brush, int half_width, uint8_t* rgba8, int nx, int ny, int nz);

/* The grow / shrink brush: erode and dilate under the brush (DESIGN.md sec.
 * 5.2.9).  vr_morph is a VR_BRUSH_SET brush whose value, per texel and
 * channel, is the MINIMUM (VR_MORPH_ERODE) or the MAXIMUM (VR_MORPH_DILATE) of
 * that channel over the texel's neighbourhood AS IT WAS BEFORE THE CALL.  In
 * integers, with h = half_width in 1..VR_MORPH_MAX_HALF: for a texel t inside
 * the ellipsoid and the volume (the inside test and the weight w are the
 * brush's, above) and a channel c with strength[c] != 0,
 *   m   = the minimum / maximum of channel c over the (2h + 1)^3 texels at
 *         offsets -h..h per axis from t, coordinates clamped to the volume
 *         (clamp-to-edge); neighbours outside the brush's box are read like
 *         any other
 *   new = (old (65280 - a) + m a + 32640) / 65280,  a = w * strength[c]
 * -- the SET blend, unchanged.  brush->op must be VR_BRUSH_SET; brush->value
 * is not read.  The structuring element is the CUBE, not a ball, because the
 * extremum over a cube is separable: the extremum over z of the extremum over
 * y of the extremum over x, all of them bytes.  Every extremum is taken over
 * the bytes before the call, whatever the order in which texels are processed
 * (a Jacobi step, not an in-place sweep), so the result is deterministic and
 * the host statement and the device agree bit for bit.  A channel whose texels
 * are all equal has m = old everywhere: a morph never breaks a uniform
 * channel.
 *
 * Device path: vr_blur's -- a stage launch from the planes to the context's
 * staging scratch, vr_blur's commit launch, the layout rebuild over the
 * clipped box (vr_brush_box names it) and the uniform-channel re-arm.
 * vr_morph and vr_blur SHARE the scratch: the need is the same (one byte per
 * texel of the clipped box and painted channel), so are the growth rule
 * (device synchronisation, whole MiB, VR_ERR_OOM holds nothing and leaves the
 * volume untouched) and option "blur_scratch_kib", which reserves, frees and
 * reports it for both.  Every call within what is held allocates nothing and
 * never waits on the host, so pick -> vr_morph -> vr_update_footprint ->
 * vr_render_rect queue on one stream.  Two vr_morph / vr_blur calls of one ctx
 * on DIFFERENT streams share the scratch: they are the caller's to order.
 * VR_ERR_INVALID: a null pointer, anything vr_paint refuses, brush->op other
 * than VR_BRUSH_SET, op outside vr_morph_op, half_width outside
 * 1..VR_MORPH_MAX_HALF; VR_ERR_NO_VOLUME before an install and while a
 * procedural medium is enabled.  A brush that misses the volume, or whose
 * strengths are all 0, is VR_OK and launches nothing.  A refused call has
 * launched nothing and leaves the volume untouched.                         */
typedef enum { VR_MORPH_ERODE = 0, VR_MORPH_DILATE = 1 } vr_morph_op;
#define VR_MORPH_MAX_HALF 3
vr_status vr_morph(void* ctx, const vr_brush* brush, int op, int half_width, void* stream);
/* The same on a HOST RGBA8 volume (x fastest): the CPU statement, which
 * vr_morph reproduces bit for bit.  It works from a copy of the clipped box
 * and its halo, never in place.  Pure host code.  VR_ERR_INVALID as above, and
 * for a non-positive dimension; a refused call leaves the array as it was.  */
vr_status vr_brush_morph_apply(const vr_brush* brush, int op, int half_width,
                               uint8_t* rgba8, int nx, int ny, int nz);

/* The median / rank-filter brush: it removes speckle
 * under the brush and leaves edges where they are.  vr_rank is a VR_BRUSH_SET
 * brush whose value, per texel and channel, is the RANK-TH SMALLEST byte of
 * that channel over the texel's neighbourhood AS IT WAS BEFORE THE CALL.  In
 * integers, with h = half_width in 1..VR_RANK_MAX_HALF and N = (2h + 1)^3 (27,
 * 125, 343): for a texel t inside the ellipsoid and the volume (the inside
 * test and the weight w are the brush's, above) and a channel c with
 * strength[c] != 0,
 *   m   = the rank-th smallest (0-based) of the N bytes of channel c at
 *         offsets -h..h per axis from t, coordinates clamped to the volume
 *         (clamp-to-edge), so a clamped texel counts once for every offset
 *         that lands on it; neighbours outside the brush's box are read like
 *         any other.  Equivalently m is the largest byte v with
 *         #{neighbours < v} <= rank, which is how it is computed (bisection
 *         on the byte from bit 7 down, csrc/vr_rank.h): ties need no rule
 *   new = (old (65280 - a) + m a + 32640) / 65280,  a = w * strength[c]
 * -- the SET blend, unchanged.  rank is 0..N - 1, or VR_RANK_MEDIAN for
 * (N - 1) / 2 = 13, 62, 171.  brush->op must be VR_BRUSH_SET; brush->value is
 * not read; a channel with strength 0 is neither read nor written.  Every m is
 * taken from the bytes before the call, whatever the order in which texels are
 * processed (a Jacobi step), so the host statement and the device agree bit
 * for bit.  Rank 0 is vr_morph's VR_MORPH_ERODE and rank N - 1 its
 * VR_MORPH_DILATE, bit for bit.  A channel whose texels are all equal has
 * m = old everywhere: vr_rank never breaks a uniform channel.
 *
 * Device path: vr_blur's and vr_morph's -- a stage launch from the planes to
 * the context's staging scratch (a rank is not separable, so this stage
 * selects over the whole cube), vr_blur's commit launch, the layout rebuild
 * over the clipped box (vr_brush_box names it) and the uniform-channel re-arm.
 * The scratch is the one vr_blur and vr_morph share: same need, same growth
 * rule (device synchronisation, whole MiB, VR_ERR_OOM holds nothing and leaves
 * the volume untouched), same option "blur_scratch_kib".  Every call within
 * what is held allocates nothing and never waits on the host, so pick ->
 * vr_rank -> vr_update_footprint -> vr_render_rect queue on one stream.  Calls
 * of one ctx on DIFFERENT streams share the scratch: they are the caller's to
 * order.
 * VR_ERR_INVALID: a null pointer, anything vr_paint refuses, brush->op other
 * than VR_BRUSH_SET, half_width outside 1..VR_RANK_MAX_HALF, rank outside
 * 0..N - 1 and not VR_RANK_MEDIAN; VR_ERR_NO_VOLUME before an install and
 * while a procedural medium is enabled.  A brush that misses the volume, or
 * whose strengths are all 0, is VR_OK and launches nothing.  A refused call
 * has launched nothing and leaves the volume untouched.                     */
#define VR_RANK_MAX_HALF 3
#define VR_RANK_MEDIAN (-1)
vr_status vr_rank(void* ctx, const vr_brush* brush, int rank, int half_width, void* stream);
/* The same on a HOST RGBA8 volume (x fastest): the CPU statement, which
 * vr_rank reproduces bit for bit.  It works from a copy of the clipped box and
 * its halo, never in place.  Pure host code.  VR_ERR_INVALID as above, and for
 * a non-positive dimension; a refused call leaves the array as it was.      */
vr_status vr_brush_rank_apply(const vr_brush* brush, int rank, int half_width,
                              uint8_t* rgba8, int nx, int ny, int nz);

/* Brushes whose value is read from texels: the clone
 * stamp, push / smudge, mirror (vr_clone) and the paste of a block with a soft
 * edge (vr_stamp).  A SOURCE BRUSH is a vr_brush used as vr_paint uses it: the
 * inside test, the clipped box (vr_brush_box), the weight w, a = w *
 * strength[c] and all three ops with their blends are the same; only value[c]
 * is replaced by a per-texel byte v_c(t).  brush->value is validated like the
 * rest of the brush and never read.  A channel with strength 0 is neither read
 * nor written.
 *
 * vr_clone: v_c(t) is channel c of the installed volume's own texel s, AS IT
 * WAS BEFORE THE CALL, where per axis a, in 64-bit arithmetic,
 *   s_a = mirror[a] ? offset[a] - t_a : t_a + offset[a]
 * clamped to [0, n_a - 1] (clamp-to-edge, as vr_blur and vr_morph read).  A
 * Jacobi step, whatever the order texels are processed in, so the host
 * statement and the device agree bit for bit.  Every int32 offset is legal.
 * The identity map with VR_BRUSH_SET leaves every byte as it was ((old 65280 +
 * 32640) / 65280 == old), so a SET clone never breaks a uniform channel; ADD
 * and SUB can, and fold their new bytes into the byte ranges as vr_paint does.
 * A mirror about the plane through a brush centred at cx is mirror[0] = 1,
 * offset[0] = 2 cx; a push by one texel is offset -1 or +1 on an axis.
 *
 * Device path, chosen on the host in integers; both give the same bytes.
 *   direct: when the clamped source range of the clipped box, [min s_a, max
 *     s_a], misses the box on at least one axis, no texel that is read is
 *     written: ONE launch from the planes to the planes -- no scratch, nothing
 *     allocated, no host wait.  The clone stamp whose offset is larger than
 *     the brush.
 *   staged: otherwise (push, mirror in place, short offsets) a stage launch
 *     from the planes to the context's staging scratch and vr_blur's commit
 *     launch.  The scratch is vr_blur's and vr_morph's: the same need (one
 *     byte per texel of the clipped box and painted channel), growth rule
 *     (device synchronisation, whole MiB, VR_ERR_OOM holds nothing and leaves
 *     the volume untouched) and option "blur_scratch_kib".
 * Both end with the layout rebuild over the clipped box (vr_brush_box names
 * it) and treat cached launches, region lists and the uniform-channel
 * read-back exactly as vr_paint does.
 * VR_ERR_INVALID: a null pointer, anything vr_paint refuses, a mirror other
 * than 0 or 1, non-zero reserved; VR_ERR_NO_VOLUME before an install and while
 * a procedural medium is enabled.  A brush that misses the volume, or whose
 * strengths are all 0, is VR_OK and launches nothing.  A refused call has
 * launched nothing and leaves the volume untouched.                          */
typedef struct {              /* 32 bytes */
    int32_t offset[3];
    int32_t mirror[3];        /* 0 or 1 per axis */
    int32_t reserved[2];      /* must be 0 */
} vr_clone_map;
vr_status vr_clone(void* ctx, const vr_brush* brush, const vr_clone_map* map, void* stream);
/* The same on a HOST RGBA8 volume (x fastest): the CPU statement, which
 * vr_clone reproduces bit for bit.  It works from a copy of what it reads,
 * never in place.  Pure host code.  VR_ERR_INVALID as above, and for a
 * non-positive dimension; a refused call leaves the array as it was.        */
vr_status vr_brush_clone_apply(const vr_brush* brush, const vr_clone_map* map,
                               uint8_t* rgba8, int nx, int ny, int nz);

/* vr_stamp: v_c(t) is channel c of a texel of the caller's DEVICE box: bx * by
 * * bz RGBA8 texels, tightly packed, x fastest -- what vr_update_volume takes
 * and vr_get_volume_box_device writes.  Stamp texel (i, j, k) lies on volume
 * texel (placement.x + i, .y + j, .z + k); x, y, z may be any int32 (the stamp
 * may hang over a face or miss the volume; x + bx and the like are formed in
 * 64 bits), the extents must be positive.  A texel is touched if and only if
 * it is inside the ellipsoid, inside the volume and inside the placement:
 * a bitmap brush with the ellipsoid as its mask.  The edited box is the
 * brush's clipped box intersected with the placement: vr_stamp_box names it,
 * and it is what to hand to vr_update_footprint.  When it is empty, or every
 * strength is 0, the call is VR_OK and launches nothing.
 * One launch and the layout rebuild over the edited box: asynchronous on
 * `stream`, nothing allocated, no host wait, no scratch; everything else as
 * after vr_paint.  d_rgba8 must be 4-byte aligned and stay valid until the
 * launch has run.  vr_get_volume_box_device(a box) followed by vr_stamp
 * elsewhere on one stream is a copy and paste with a soft edge; stamping a
 * saved box back through a soft brush is a feathered undo.
 * VR_ERR_INVALID: a null pointer, anything vr_paint refuses, a non-positive
 * stamp extent, a misaligned d_rgba8; VR_ERR_NO_VOLUME as for vr_paint.  A
 * refused call has launched nothing and leaves the volume untouched.        */
vr_status vr_stamp(void* ctx, const vr_brush* brush, const void* d_rgba8, const vr_box* placement, void* stream);
/* The same on a HOST RGBA8 volume with a HOST stamp: the CPU statement, which
 * vr_stamp reproduces bit for bit.  Pure host code; the stamp is copied first,
 * so it may lie inside rgba8.  VR_ERR_INVALID as above (no alignment is
 * asked), and for a non-positive dimension; a refused call leaves the array as
 * it was.                                                                    */
vr_status vr_brush_stamp_apply(const vr_brush* brush, const uint8_t* stamp_rgba8, const vr_box* placement,
                               uint8_t* rgba8, int nx, int ny, int nz);
/* The edited box of a stamp in an nx x ny x nz volume; extent = (0, 0, 0) (and
 * origin 0) when it is empty.  Pure host code, validated as above.          */
vr_status vr_stamp_box(const vr_brush* brush, const vr_box* placement, int nx, int ny, int nz,
                       int origin[3], int extent[3]);

/* Transform paste: vr_stamp and vr_clone with an
 * affine map from destination texels to source POSITIONS and a resampling
 * filter -- a copy pasted rotated, scaled, sheared or shifted by a fraction of
 * a texel.  Both are SOURCE BRUSHES as above; only v_c(t) differs.  All of it
 * is integer arithmetic, so host and device agree bit for bit.
 *
 * The map.  For a destination texel t (volume coordinates), a source of n_x *
 * n_y * n_z texels and each axis a, in signed 64 bits,
 *   P_a = origin[a] + sum_b m[a][b] * (t_b - pivot[b])
 * a 16.16 position in source texel coordinates (|m| <= 2^24 and |t - pivot| <
 * 2^32 keep it below 2^59).  The texel is OUTSIDE the source iff on some axis
 * P_a < 0 or P_a > (n_a - 1) << 16.  VR_BORDER_SKIP: an outside texel is not
 * touched -- nothing is read, written or folded for it.  VR_BORDER_CLAMP:
 * every P_a is clamped to [0, (n_a - 1) << 16] (clamp-to-edge, as vr_clone)
 * and the texel is processed.  Then i_a = P_a >> 16, and
 *   VR_FILTER_NEAREST  v_c = channel c of source texel i_a + ((P_a & 0xFFFF) >=
 *     0x8000) -- never past n_a - 1;
 *   VR_FILTER_LINEAR   f_a = (P_a >> 8) & 255, j_a = min(i_a + 1, n_a - 1), and
 *     v_c = (sum over the 8 corners of wx wy wz byte(corner) + 2^23) >> 24 with
 *     weight 256 - f_a for i_a and f_a for j_a: exact in unsigned 32 bits
 *     (the weights sum to 2^24), nothing rounded in between.  Equal corner
 *     bytes give that byte back, so an affine SET over a uniform channel never
 *     breaks it.
 *
 * vr_stamp_affine: the source is the caller's DEVICE RGBA8 box of sbx * sby *
 * sbz texels (each 1..32768), tightly packed, x fastest, 4-byte aligned: what
 * vr_get_volume_box_device writes.  A texel is touched iff it is inside the
 * ellipsoid, inside the volume and (VR_BORDER_SKIP) not outside the source.
 * ONE launch, asynchronous on `stream`, nothing allocated, no host wait, no
 * scratch, then the layout rebuild over the brush's clipped box (vr_brush_box
 * names it: what to hand to vr_update_footprint); everything else as vr_stamp.
 *
 * vr_clone_affine: the source is the installed volume AS IT WAS BEFORE THE
 * CALL (a Jacobi step); n is the volume's size.  The device path is chosen on
 * the host in integers: the 8 corners of the clipped box are mapped to P, per
 * axis lo = min P and hi = max P, the read range is [lo >> 16, (hi >> 16) + 1]
 * (LINEAR) or [(lo + 0x8000) >> 16, (hi + 0x8000) >> 16] (NEAREST), clamped
 * to [0, n_a - 1]; when it misses the clipped box on at least one axis the
 * path is DIRECT (one launch from the planes to the planes, no scratch), else
 * STAGED (a stage launch into vr_blur's scratch and its commit launch: the
 * same need, growth rule, VR_ERR_OOM rule and "blur_scratch_kib").  Both give
 * the same bytes.  vr_affine_direct tells which.
 *
 * VR_ERR_INVALID: a null pointer, anything vr_paint refuses, a filter or
 * border outside its enum, non-zero reserved, |m[a][b]| above
 * VR_AFFINE_MAX_COEFF, a source extent outside 1..32768, a misaligned
 * d_rgba8; VR_ERR_NO_VOLUME as for vr_paint.  A brush that misses the volume,
 * or whose strengths are all 0, is VR_OK and launches nothing.  A refused
 * call has launched nothing and leaves the volume untouched.                */
typedef enum { VR_FILTER_NEAREST = 0, VR_FILTER_LINEAR = 1 } vr_filter;
typedef enum { VR_BORDER_CLAMP = 0, VR_BORDER_SKIP = 1 } vr_border;
#define VR_AFFINE_ONE       65536          /* 16.16 fixed point */
#define VR_AFFINE_MAX_COEFF (256 * 65536)  /* |m[a][b]| <= 2^24 */
#define VR_AFFINE_MAX_EXTENT 32768         /* of a vr_stamp_affine source, per axis */
typedef struct {            /* 72 bytes */
    int32_t m[3][3];        /* 16.16: source texels per destination texel */
    int32_t pivot[3];       /* destination texel (volume coords, any int32) that lands on `origin` */
    int32_t origin[3];      /* 16.16 position in SOURCE texel coordinates */
    int32_t filter;         /* vr_filter */
    int32_t border;         /* vr_border */
    int32_t reserved;       /* must be 0 */
} vr_affine;
vr_status vr_stamp_affine(void* ctx, const vr_brush* brush, const void* d_rgba8, int sbx, int sby, int sbz,
                          const vr_affine* map, void* stream);
vr_status vr_clone_affine(void* ctx, const vr_brush* brush, const vr_affine* map, void* stream);
/* The same on HOST arrays: the CPU statements, which the device calls
 * reproduce bit for bit.  Pure host code; each works from a copy of what it
 * reads (the stamp may lie inside rgba8).  VR_ERR_INVALID as above (no
 * alignment is asked), and for a non-positive dimension; a refused call leaves
 * the array as it was.                                                      */
vr_status vr_brush_stamp_affine_apply(const vr_brush* brush, const uint8_t* stamp_rgba8, int sbx, int sby, int sbz,
                                      const vr_affine* map, uint8_t* rgba8, int nx, int ny, int nz);
vr_status vr_brush_clone_affine_apply(const vr_brush* brush, const vr_affine* map, uint8_t* rgba8, int nx, int ny, int nz);
/* *direct = 1 when vr_clone_affine of this brush and map in an nx x ny x nz
 * volume takes the direct path, 0 for the staged one (and for a brush that
 * misses the volume).  Pure host code, validated as above.                  */
vr_status vr_affine_direct(const vr_brush* brush, const vr_affine* map, int nx, int ny, int nz, int* direct);
/* Builders, pure host code.  vr_affine_identity: m = the identity, pivot =
 * origin = 0, NEAREST, CLAMP.  vr_affine_place: "rotate / scale the copy by
 * `forward` (row-major, destination offset = forward * source offset) and put
 * the source position src_centre (texels) on destination texel dst_centre":
 * m = rint(inverse(forward) * 65536), pivot = dst_centre, origin =
 * rint(src_centre * 65536).  VR_ERR_INVALID for a null pointer, a bad filter
 * or border, a non-finite entry, a singular `forward` (|det| < 1e-12 times the
 * cube of its largest absolute entry), a coefficient above
 * VR_AFFINE_MAX_COEFF or an origin outside int32; *out is written only on
 * success.                                                                  */
vr_status vr_affine_identity(vr_affine* out);
vr_status vr_affine_place(const double forward[9], const double src_centre[3], const int32_t dst_centre[3],
                          int filter, int border, vr_affine* out);

/* The liquify brush: push, pinch, bloat, twirl.  What
 * is under the brush MOVES, by an amount that fades out towards the rim:
 * vr_clone_affine's resampling with the brush weight blending the POSITION
 * with the identity, not the moved copy with the original.  Integers only.
 *
 * vr_warp is a source brush that reads the installed volume AS IT WAS BEFORE
 * THE CALL (a Jacobi step).  For a texel t inside the ellipsoid and inside the
 * volume, with w vr_paint's weight (256 for falloff 0; 256 at the centre down
 * to 1 on the rim for falloff 1) and per axis a, in signed 64 bits,
 *   I_a = t_a << 16
 *   A_a = map->origin[a] + sum_b map->m[a][b] * (t_b - map->pivot[b])
 *   D_a = A_a - I_a
 *   P_a = I_a + ((w * D_a) >> 8)          (>> arithmetic: floor)
 * so w = 256 gives P = A exactly and a small w leaves P next to the texel
 * itself.  The outside test, the clamp, VR_BORDER_SKIP / VR_BORDER_CLAMP,
 * VR_FILTER_NEAREST and VR_FILTER_LINEAR are vr_clone_affine's, applied to P,
 * with n the volume's size.  The blend is the SET blend with a = 256 *
 * strength[c]: falloff shapes the displacement, not the mix -- no ghost image,
 * and the motion fades to nothing at the rim.  brush->op must be
 * VR_BRUSH_SET; brush->value is not read; a channel with strength 0 is
 * neither read nor written.  The identity map leaves every byte as it was;
 * with falloff 0 the result is vr_clone_affine's with the same map, SET and
 * falloff 0; a warp never breaks a uniform channel.
 *
 * The maps.  A push is vr_warp_push: m = the identity, pivot = centre,
 * origin[a] = (centre[a] << 16) - d16[a], so the content under the brush moves
 * by +d16 / 65536 texels; a drag is a sequence of pushes.  The others need no
 * builder: they are vr_affine_place(forward, centre, centre, ...) with the
 * brush centre as both centres, e.g.
 *   pinch  forward = diag(0.8, 0.8, 0.8)   (bloat: diag(1.25, 1.25, 1.25))
 *   twirl  forward = the rotation by 20 degrees about z,
 *          {c, -s, 0,  s, c, 0,  0, 0, 1} with c = cos 20, s = sin 20.
 *
 * Device path: always staged (a soft warp reads texels that it writes).  The
 * scratch is vr_blur's -- one byte per texel of the clipped box and painted
 * channel, the same growth rule, VR_ERR_OOM rule and "blur_scratch_kib" --
 * then a stage launch (a workgroup per 8 x 8 x 8 tile of the clipped box; a
 * tile whose source footprint is at most 4096 texels reads it through LDS,
 * option "warp_lds", default 1; 0 = every tile gathers from memory), vr_blur's
 * commit launch, the layout rebuild over the clipped box (vr_brush_box) and
 * the uniform-channel re-arm.  Within the scratch held it allocates nothing
 * and never waits on the host, so pick -> vr_warp -> vr_update_footprint ->
 * vr_render_rect queue on one stream.
 *
 * VR_ERR_INVALID: everything vr_clone_affine refuses, an op other than
 * VR_BRUSH_SET, and a map whose |D_a| passes VR_WARP_MAX_DISP << 16 at one of
 * the 8 corners of the UNCLIPPED box [centre - radius, centre + radius] (D is
 * affine in t, so the corners bound it under the whole brush; the limit keeps
 * w * D below 2^40).  vr_warp_reach tells the largest |D_a| per axis.
 * VR_ERR_NO_VOLUME as for vr_paint.  A brush that misses the volume, or whose
 * strengths are all 0, is VR_OK and launches nothing.  A refused call has
 * launched nothing and leaves the volume untouched.                         */
#define VR_WARP_MAX_DISP 32768             /* texels: |D_a| <= 2^31 in 16.16 */
vr_status vr_warp(void* ctx, const vr_brush* brush, const vr_affine* map, void* stream);
/* The same on a HOST RGBA8 volume (x fastest): the CPU statement, which
 * vr_warp reproduces bit for bit.  Pure host code; it works from a copy of
 * what it reads.  VR_ERR_INVALID as above, and for a null rgba8 or a
 * non-positive dimension; a refused call leaves the array as it was.        */
vr_status vr_brush_warp_apply(const vr_brush* brush, const vr_affine* map, uint8_t* rgba8, int nx, int ny, int nz);
/* reach16[a] = max |D_a| over the 8 corners of the unclipped box, in 16.16,
 * saturated at INT32_MAX (the limit itself, 2^31, and anything above it read
 * INT32_MAX).  Pure host code; VR_ERR_INVALID for a null pointer and for what
 * vr_clone_affine refuses of the brush and the map -- not for the op or the
 * reach, so that a caller can see why vr_warp refused a map.                */
vr_status vr_warp_reach(const vr_brush* brush, const vr_affine* map, int32_t reach16[3]);
/* The map of a push by d16 (16.16 texels per axis), integer-exact.  Pure host
 * code; VR_ERR_INVALID for a null pointer, a bad filter or border, or an
 * origin outside int32; *out is written only on success.                    */
vr_status vr_warp_push(const int32_t centre[3], const int32_t d16[3], int filter, int border, vr_affine* out);

/* The flood-fill brush: the bucket fill / magic wand.
 * Every other brush selects an ellipsoid of texels; vr_fill selects, inside
 * that ellipsoid, the texels CONNECTED to a seed whose bytes resemble it, and
 * applies vr_paint's brush to those only.  Integers throughout.
 *
 * PASSABLE.  With s_c the seed texel's byte of channel c, a texel t is
 * passable iff, on the bytes AS THEY WERE BEFORE THE CALL,
 *   - t is inside the brush (vr_paint's inside test, clipped to the volume),
 *   - and for every channel c with select[c] != 0 its byte b satisfies
 *       relative == 0:  lo[c] <= b <= hi[c]
 *       relative == 1:  max(0, s_c - lo[c]) <= b <= min(255, s_c + hi[c]).
 * REGION.  The passable texels reachable from the seed by steps of +-1 on one
 * axis (6-connectivity), every texel of the path passable.  A path may not
 * leave the ellipsoid: two parts of one blob joined only outside the brush
 * are two regions.  If the seed itself is not passable (outside the
 * ellipsoid, or out of range with relative == 0) the region is empty.
 * EFFECT.  vr_paint's brush on the texels of the region only: the same weight
 * w, a = w * strength[c], the same SET / ADD / SUB blends with brush->value.
 * A channel with strength 0 is neither read nor written unless it is a select
 * channel, which is read; the selected and the painted channels are
 * independent of each other.  The region is a fixed point that does not
 * depend on the order of processing, so the host statement and the device
 * agree bit for bit, in the volume and in the report.
 *
 * REPORT (optional).  filled = the texels of the region; passable = the
 * passable texels, connected to the seed or not; min / max = the region's
 * inclusive bounds in volume coordinates.  The EMPTY report is filled =
 * passable = 0, min = {nx, ny, nz}, max = {-1, -1, -1}; a region that is
 * empty because the seed is not passable still counts `passable`, with the
 * empty bounds.  d_report is a DEVICE vr_fill_report, 8-byte aligned, which
 * the call overwrites on `stream`.
 *
 * With every strength 0 and a report the call runs and writes nothing but the
 * report (the magic wand as a measurement); with every strength 0 and no
 * report it launches nothing.  A brush that misses the volume, or a seed
 * outside the brush's clipped box (vr_brush_box), is VR_OK: the report, if
 * given, is set to the empty one and nothing else is launched.
 *
 * Device path: three launches and what follows an edit of the clipped box --
 * (1) a workgroup per 8 x 8 x 8 tile of the box evaluates `passable` and
 * labels the tile's passable texels by tile-local connected component in LDS
 * (a union-find), writing per texel the box-linear index of its component's
 * smallest member; (2) a thread per texel on a tile's low face whose
 * neighbour across the face is passable too unites the two labels in global
 * memory (agent-scope atomic loads and atomicMin only); (3) vr_paint's rows
 * over the box: a texel whose root is the seed's root is blended, the new
 * bytes are folded into the channels' byte ranges, the report is accumulated.
 * No kernel waits for another workgroup and every loop is bounded by the
 * box's texel count.  The labels (4 bytes per texel of the clipped box) live
 * in the scratch vr_blur, vr_morph and vr_rank share: same growth rule (device
 * synchronisation, whole MiB, VR_ERR_OOM holds nothing and leaves the volume
 * untouched), same option "blur_scratch_kib".  Within what is held the call
 * allocates nothing and never waits on the host, so pick -> vr_fill ->
 * vr_update_footprint -> vr_render_rect queue on one stream.  The edited box
 * is the brush's clipped box; a caller who reads the report back may use its
 * tighter bounds.
 * VR_ERR_INVALID: a null ctx, brush or rule, anything vr_paint refuses, a seed
 * outside the volume, relative not 0 or 1, no selected channel, relative == 0
 * with lo[c] > hi[c] on a selected channel, non-zero reserved, d_report not
 * 8-byte aligned; VR_ERR_NO_VOLUME as for vr_paint.  A refused call has
 * launched nothing.                                                         */
typedef struct {              /* 32 bytes */
    int32_t seed[3];          /* texel (x, y, z); must lie inside the volume */
    int32_t relative;         /* 0: lo / hi are bytes; 1: distances below / above the seed's byte */
    uint8_t lo[4], hi[4];     /* per channel R, G, B, A */
    uint8_t select[4];        /* non-zero: the channel takes part in the test; at least one */
    int32_t reserved;         /* must be 0 */
} vr_fill_rule;
typedef struct {              /* 40 bytes */
    uint64_t filled;          /* texels of the region */
    uint64_t passable;        /* texels of the brush that pass the test, connected to the seed or not */
    int32_t  min[3], max[3];  /* inclusive bounds of the region; {nx, ny, nz} / {-1, -1, -1} when filled == 0 */
} vr_fill_report;
vr_status vr_fill(void* ctx, const vr_brush* brush, const vr_fill_rule* rule,
                  vr_fill_report* d_report /* DEVICE, may be NULL */, void* stream);
/* The same on a HOST RGBA8 volume (x fastest): the CPU statement, which
 * vr_fill reproduces bit for bit -- a breadth-first search with a queue over
 * the passable mask of the clipped box, taken before any byte is written.
 * Pure host code.  VR_ERR_INVALID as above (no alignment is asked), and for a
 * null rgba8 or a non-positive dimension; a refused call leaves the array and
 * *report as they were.                                                     */
vr_status vr_brush_fill_apply(const vr_brush* brush, const vr_fill_rule* rule, uint8_t* rgba8,
                              int nx, int ny, int nz, vr_fill_report* report /* HOST, may be NULL */);

/* The read side of the brush: what is in the volume under it (DESIGN.md sec.
 * 5.2.8) -- the eyedropper, a histogram panel, and the answer to "has this
 * channel become constant again?".  Everything is an integer sum, so the
 * result does not depend on the order in which texels are visited and the
 * host statement and the device agree in every bit.
 *
 * A texel is INSIDE exactly as for vr_paint: |d_a| <= radius[a] on every axis,
 * Q <= S, and inside the volume; its weight w is the brush's (256 for a hard
 * edge, 256 at the centre down to 1 on the rim for a smooth one).  Channel c
 * is SELECTED iff strength[c] != 0 -- vr_paint's rule; an unselected channel
 * is not read.  op and value are validated and then ignored.  Over a texel
 * box (vr_box_stats) every texel of the box is inside with w = 256, and bit c
 * of channel_mask selects channel c.
 *   count     the inside texels
 *   weight    the sum of w over them (256 * count for a hard edge and a box)
 *   wsum[c]   selected c: the sum of w * byte over them; else 0
 *   hist[c][v] selected c: the inside texels whose channel c holds v; else 0
 * so the bins of a selected channel add up to count.  All fields are 64 bits
 * wide: nothing in the struct can overflow (w * byte <= 65280 per texel and a
 * volume has fewer than 2^31 texels).                                       */
typedef struct {              /* 8240 bytes; all-zero is the empty result */
    uint64_t count;           /* inside texels                                   */
    uint64_t weight;          /* sum of w over them (256 * count for a hard edge) */
    uint64_t wsum[4];         /* per selected channel: sum of w * byte; else 0   */
    uint64_t hist[4][256];    /* per selected channel: inside texels holding byte v; else 0 */
} vr_volume_stats;
/* The statistics of the installed volume under the brush, into `d_stats`: a
 * DEVICE vr_volume_stats, 8-byte aligned, which the call OVERWRITES (a
 * hipMemsetAsync to zero on `stream`, then one kernel launch).  Asynchronous
 * on `stream`, nothing allocated, no host wait.  It reads the planes as
 * vr_get_volume_box_device does -- after a vr_paint on the same stream it sees
 * the painted bytes -- and writes only `d_stats`: cached launches, region
 * lists, scratches, the pending uniform-channel read-back and the channels'
 * byte ranges are neither used nor disturbed, so the next render is what it
 * would have been without the call.  A brush that misses the volume still
 * zeroes the buffer and launches no kernel; with every strength 0, count and
 * weight are still produced and the channels are empty.
 * VR_ERR_INVALID: a null pointer, a brush vr_paint would refuse, d_stats not
 * 8-byte aligned; VR_ERR_NO_VOLUME before an install and while a procedural
 * medium is enabled.  A refused call writes nothing.                        */
vr_status vr_brush_stats(void* ctx, const vr_brush* brush, void* d_stats, void* stream);
/* The same over the texel box [x0,x0+bx) x [y0,y0+by) x [z0,z0+bz): the same
 * kernel with the ellipsoid test switched off.  The box is validated as
 * vr_update_volume validates it (the whole volume is a valid box);
 * channel_mask outside 0..15 is VR_ERR_INVALID.  min == max of a channel (see
 * vr_stats_summary) over the whole volume says the channel is constant again:
 * a re-install would re-arm its uniform bit.                                */
vr_status vr_box_stats(void* ctx, int x0, int y0, int z0, int bx, int by, int bz, int channel_mask, void* d_stats,
                       void* stream);
/* The same two on a HOST RGBA8 volume (x fastest): the CPU statements, which
 * the device reproduces bit for bit, as vr_brush_apply is for vr_paint.  *out
 * is overwritten.  Pure host code.  VR_ERR_INVALID as above, and for a
 * non-positive dimension; a refused call leaves *out as it was.             */
vr_status vr_brush_stats_host(const vr_brush* brush, const uint8_t* rgba8, int nx, int ny, int nz, vr_volume_stats* out);
vr_status vr_box_stats_host(const uint8_t* rgba8, int nx, int ny, int nz, int x0, int y0, int z0, int bx, int by, int bz,
                            int channel_mask, vr_volume_stats* out);
/* What a caller reads off a vr_volume_stats, per channel c, with
 * n = sum_v hist[c][v] (integer division throughout):
 *   n[c]
 *   min[c], max[c]   the lowest and the highest non-empty bin
 *   mean[c]          (sum_v v hist[c][v] + n / 2) / n
 *   wmean[c]         (wsum[c] + weight / 2) / weight -- the eyedropper's value:
 *                    value[c] = wmean[c] for the next vr_paint
 *   median[c]        the smallest v with 2 cum(v) >= n, cum(v) = sum_{u<=v} hist[c][u]
 * and all five are 0 where n = 0 (an unselected channel, an empty result).
 * Pure host code.  VR_ERR_INVALID: a null pointer.                          */
typedef struct {              /* 112 bytes */
    uint64_t n[4];
    int32_t  min[4], max[4], mean[4], wmean[4], median[4];
} vr_volume_summary;
vr_status vr_stats_summary(const vr_volume_stats* stats, vr_volume_summary* out);

/* The lookup-table brush: the tone family of an editor
 * -- levels, contrast, invert, threshold, posterise, equalise.  vr_remap is a
 * SOURCE BRUSH in the sense of vr_clone above: the inside test, the clipped box
 * (vr_brush_box), the weight w, a = w * strength[c], all three ops and their
 * blends are vr_paint's; only value[c] is replaced, by a function of the
 * texel's OWN byte,
 *   v_c(t) = lut[c][ old_c(t) ]      new = blend(op, old, lut[c][old], a)
 * brush->value is validated like the rest of the brush and never read.  A
 * channel with strength 0 is neither read nor written, and its table is never
 * read.  A texel's new byte depends on that texel's old byte alone: there is
 * no Jacobi question, no scratch and no choice of path -- one launch, in
 * place.  The identity table with VR_BRUSH_SET leaves every byte as it was (so
 * it never breaks a uniform channel); ADD and SUB do not.
 *
 * Everything is in integers, so the host and the device agree bit for bit.  */
typedef struct { uint8_t lut[4][256]; } vr_lut;      /* 1024 bytes; lut[c][v] = the value for byte v of channel c */
typedef enum { VR_LUT_EQUALIZE = 0, VR_LUT_STRETCH = 1 } vr_lut_kind;
/* Table builders: pure host code, no context, no device.  Each writes *out
 * only on success; VR_ERR_INVALID for a null pointer, a bad kind, a mask
 * outside 0..15 or a bad range.
 *   vr_lut_identity  out[c][v] = v.
 *   vr_lut_levels    for the channels of channel_mask (bit c = channel c; the
 *     others keep what *out ALREADY holds, so calls stack per channel), with
 *     0 <= in_lo < in_hi <= 255 and out_lo, out_hi in 0..255 in either order:
 *     v <= in_lo gives out_lo, v >= in_hi gives out_hi, and between them
 *       out_lo + floor((2 (v - in_lo)(out_hi - out_lo) + (in_hi - in_lo))
 *                      / (2 (in_hi - in_lo)))
 *     (floor also of a negative numerator, as in vr_brush_line).  Invert is
 *     (0, 255, 255, 0); a threshold at T >= 1 is (T - 1, T, 0, 255).
 *   vr_lut_compose   out[c][v] = then[c][ first[c][v] ]; out may alias either.
 *   vr_stats_lut     a table from the histograms of a vr_volume_stats (only
 *     hist is read); it overwrites all four channels.  A channel outside the
 *     mask is the identity, and so is one whose bins sum to n = 0 or that has
 *     a single non-empty bin.  For the others, with lo and hi the lowest and
 *     highest non-empty bin, cum(v) = sum_{u<=v} hist[c][u] in 64 bits and
 *     cmin = cum(lo) (integer division):
 *       VR_LUT_STRETCH   v <= lo: 0;  v >= hi: 255;  else
 *                        ((v - lo) 255 + (hi - lo) / 2) / (hi - lo)
 *       VR_LUT_EQUALIZE  v < lo: 0;  else
 *                        ((cum(v) - cmin) 255 + (n - cmin) / 2) / (n - cmin)
 *     (bins are meant to be those of vr_brush_stats / vr_box_stats, below
 *     2^47 in sum; sums wrap at 64 bits, a wrapped n - cmin of 0 gives the
 *     identity, and the entry is the low byte of the quotient).              */
vr_status vr_lut_identity(vr_lut* out);
vr_status vr_lut_levels(vr_lut* out, int channel_mask, int in_lo, int in_hi, int out_lo, int out_hi);
vr_status vr_lut_compose(const vr_lut* first, const vr_lut* then, vr_lut* out);
vr_status vr_stats_lut(const vr_volume_stats* stats, int kind, int channel_mask, vr_lut* out);
/* vr_remap: the brush on the installed volume with a HOST table.  The table is
 * read DURING the call (its 1024 bytes travel by value in the kernel's
 * arguments): the caller may overwrite it as soon as the call returns, queued
 * calls never share a buffer, and the call can be captured in a graph.
 * vr_remap_device: the table is a DEVICE vr_lut, 4-byte aligned, read WHEN THE
 * KERNEL RUNS: a table written earlier on the same stream -- by
 * vr_stats_lut_device or by a copy -- is the one applied; d_lut must stay
 * valid until then.  Both follow vr_paint's contract: asynchronous on
 * `stream`, nothing allocated, no host wait; afterwards the context renders,
 * and vr_get_volume reads, bit for bit what vr_set_volume of the remapped
 * volume would give.  One launch (the tables of the painted channels are
 * staged into 1 KiB of LDS per workgroup, the lookup is an LDS byte read, a
 * byte is stored only where it changed, the new bytes are folded into the
 * channels' byte ranges), then the layout rebuild over the clipped box
 * (vr_brush_box names it: what to hand to vr_update_footprint); cached
 * launches, region lists and the uniform-channel read-back are treated exactly
 * as after vr_paint.
 * VR_ERR_INVALID: a null pointer, anything vr_paint refuses, a misaligned
 * d_lut; VR_ERR_NO_VOLUME before an install and while a procedural medium is
 * enabled.  A brush that misses the volume, or whose strengths are all 0, is
 * VR_OK and launches nothing.  A refused call has launched nothing and leaves
 * the volume untouched.                                                      */
vr_status vr_remap(void* ctx, const vr_brush* brush, const vr_lut* lut /* HOST */, void* stream);
vr_status vr_remap_device(void* ctx, const vr_brush* brush, const void* d_lut /* DEVICE vr_lut, 4-byte aligned */, void* stream);
/* vr_stats_lut on the device: d_stats is a DEVICE vr_volume_stats (8-byte
 * aligned) as vr_brush_stats / vr_box_stats leave it, d_lut a DEVICE vr_lut
 * (4-byte aligned).  One launch on `stream` that writes all 1024 bytes of
 * d_lut -- bit for bit vr_stats_lut's -- and nothing else, so
 *   vr_brush_stats -> vr_stats_lut_device -> vr_remap_device
 *     -> vr_update_footprint -> vr_render_rect
 * queues on one stream with no host round trip.  It needs a context only for
 * its device: no volume is needed, a procedural medium may be enabled, and
 * nothing of the context is used or disturbed.
 * VR_ERR_INVALID: a null pointer, a misaligned d_stats or d_lut, a bad kind or
 * mask; a refused call has launched nothing and leaves d_lut untouched.      */
vr_status vr_stats_lut_device(void* ctx, const void* d_stats /* DEVICE vr_volume_stats, 8-byte aligned */,
                              int kind, int channel_mask, void* d_lut /* DEVICE vr_lut, 4-byte aligned */, void* stream);
/* vr_remap on a HOST RGBA8 volume (x fastest): the CPU statement, which the
 * device reproduces bit for bit.  In place -- safe, since a texel depends on
 * itself only.  Pure host code.  VR_ERR_INVALID as above (no alignment is
 * asked), and for a non-positive dimension; a refused call leaves the array as
 * it was.                                                                    */
vr_status vr_brush_remap_apply(const vr_brush* brush, const vr_lut* lut, uint8_t* rgba8, int nx, int ny, int nz);
/* 1 if vr_set_volume / vr_set_volume_device accept an nx x ny x nz extent
 * (the device layouts index a plane with 32-bit offsets), else 0: every
 * axis positive and (nx + 2)(ny + 2)(nz + 2) < 2^31, for any int arguments */
int       vr_volume_extent_ok(int nx, int ny, int nz);

/* ---- volume generation on the GPU: replaces the host start-up loops of
 *      TestMain.cpp:43-92.  Synchronous.             */
vr_status vr_volume_recipe_defaults(vr_volume_recipe* r);
vr_status vr_generate_volume(void* ctx, const vr_volume_recipe* r, void* stream);
/* one noise grid, for parity tests: kind 0 cellular, 1 perlin, 2 simplex.
 * d_out: device float[nx*ny*nz] (may be NULL); min/max to host.           */
vr_status vr_noise_grid(void* ctx, int kind, void* d_out, int x0, int y0, int z0,
                        int nx, int ny, int nz, float freq, int32_t seed,
                        float* out_min, float* out_max, void* stream);
/* Exhaustive device self-test of an arithmetic shortcut against its IEEE
 * definition; *failures = number of mismatching inputs (synchronous).
 * "cell_inv" (the cellular cell-point magnitude that the noise kernels use)
 * and the candidates "cell_inv_a", "cell_inv_b", "cell_inv_c";
 * "worley_prune": the procedural march's pruned Worley F1 against the full
 * 27-cell one on 2^23 points per seed (uniform, and at the bound's edge
 * cases: rint and floor switches, feature points, near ties).            */
vr_status vr_selftest(void* ctx, const char* name, long long* failures);

/* ---- uniforms: replaces UniformBuffer<T>::Update x2 (TestMain.cpp:248-249,
 *      VulkanUniformBuffer.h:58-61).  The data is copied.                  */
vr_status vr_set_shader_data(void* ctx, const vr_object_shader_data* osd,
                             const vr_global_shader_data* gsd);
/* host camera producer of TestMain.cpp:219-245: Model = rotZ(phi)*rotY(theta),
 * lookAt((3,3,3), 0, +Z), perspective(45deg, aspect, .1, 10) with y flipped,
 * W2L = inverse(Model), MediaScroll[0][0] = -frame_time.                   */
vr_status vr_reference_shader_data(float aspect, float phi_deg, float theta_deg,
                                   float frame_time, vr_object_shader_data* osd,
                                   vr_global_shader_data* gsd);

/* ---- procedural medium (configs 2/3) ----------------------------------- */
vr_status vr_procedural_defaults(vr_procedural* p);   /* enabled = 0 */
vr_status vr_set_procedural(void* ctx, const vr_procedural* p);

/* ---- march constants (frag.glsl:29-32, 42, 63-69) ---------------------- */
vr_status vr_march_defaults(vr_march_params* m);
vr_status vr_set_march(void* ctx, const vr_march_params* m);

/* ---- the hot path: replaces EnqueueRenderPass("BasePass") + the draw of
 *      TestMain.cpp:194-217 + vert.glsl/frag.glsl (VulkanRenderer.h:84-87).
 *      A procedural medium, when enabled, needs no volume.

 *      stream = hipStream_t (NULL = default stream).                       */
vr_status vr_render(void* ctx, const vr_target* target, void* stream);
/* The frame loop of TestMain.cpp:173-256 with a moving camera: `frames`
 * renders into `target`, frame i with shader data (osd[i], gsd[i]) -- the
 * per-frame UBO updates of :219-249 -- all queued on `stream` without a host
 * wait.  The ctx keeps the last frame's shader data.                       */
vr_status vr_render_sequence(void* ctx, const vr_target* target, int frames, const vr_object_shader_data* osd,
                             const vr_global_shader_data* gsd, void* stream);
/* Two queued frames in one launch: frame 0 into `t0` with shader data (osd[0],
 * gsd[0]), frame 1 into `t1` with (osd[1], gsd[1]); osd and gsd both NULL =
 * both frames with the ctx's current shader data.  The bytes in both targets
 * and the sum added to step_counter are those of
 *   vr_set_shader_data(0); vr_render(t0); vr_set_shader_data(1); vr_render(t1)
 * and the ctx ends holding shader data 1.  The targets must agree in every
 * field but `pixels` (VR_ERR_INVALID otherwise, nothing written).  A grid
 * medium on the default regions schedule (one lane per ray; the COL48,
 * BRICK4832 and CORNERH layouts) marches both frames in one kernel over one
 * set of region lists -- frame 0's -- so the two frames read each brick of the
 * volume at the same moment.  Anything else (a
 * procedural medium, split rays, option slab, another schedule or layout,
 * frames whose MediaScroll offsets select different kernels) is issued as the
 * two ordinary renders.  Asynchronous on `stream`; steady state neither
 * allocates nor waits on the host.                                          */
vr_status vr_render_pair(void* ctx, const vr_target* t0, const vr_target* t1, const vr_object_shader_data osd[2],
                         const vr_global_shader_data gsd[2], void* stream);
/* n = 1..4 queued frames: frame i into `targets[i]` with shader data (osd[i],
 * gsd[i]); osd and gsd both NULL = every frame with the ctx's current shader
 * data.  The bytes in every target and the sum added to step_counter are
 * those of vr_set_shader_data(i); vr_render(targets[i]) for i = 0..n-1 in
 * order, and the ctx ends holding shader data n-1.  The targets must agree in
 * every field but `pixels` (VR_ERR_INVALID otherwise, nothing written).
 * Four frames that vr_render_pair would pair (a grid medium, the regions
 * schedule with one lane per ray, the COL48, BRICK4832 and CORNERH layouts,
 * frames that select one kernel) are marched by ONE kernel over frame 0's
 * region lists: a workgroup is one list entry x four frames, so the four
 * readers of a brick share one L1.  n = 3 is a pair
 * (vr_render_pair's path) and a plain render, n = 2 vr_render_pair's path,
 * n = 1 vr_render's.  Fallbacks: whatever vr_render_pair issues as ordinary
 * renders -- a procedural medium, split rays, option slab, another schedule
 * or layout, the planar layout with mirrored repeat, frames whose MediaScroll
 * offsets select different kernels -- is issued here as n ordinary renders, in
 * order: four frames that do not all share one plan do not degrade to pairs,
 * even where two of them would pair with each other.  Frame 0 is planned as vr_render plans it and its errors read as
 * vr_render's; a frame k that fails to plan leaves frames 0..k-1 rendered and
 * returns its error.  Asynchronous on `stream`; steady state neither
 * allocates nor waits on the host.                                          */
#define VR_MAX_GROUP 4
vr_status vr_render_group(void* ctx, const vr_target* targets, int n, const vr_object_shader_data* osd,
                          const vr_global_shader_data* gsd, void* stream);
/* How vr_render_group (and the native frame loop, vr_shard.h) issues n = 1..4
 * frames: the frames per launch, in order, into launches[0..] (the rest 0) --
 * 4 -> {4}, 3 -> {2, 1}, 2 -> {2}, 1 -> {1}.  Returns the number of launches,
 * 0 for any other n.  Host arithmetic only.                                 */
int vr_group_split(int n, int launches[3]);

/* ---- the scissor: replaces vkCmdSetScissor with a VkRect2D, a dynamic state
 *      of the reference's pipeline (TestMain.cpp:192, 204-205, where it is
 *      always the whole swapchain extent).  Pixels: x along a row, y the
 *      frame row.                                                            */
typedef struct { int32_t x, y, width, height; } vr_rect;
/* Render the pixels [x, x+width) x [y, y+height) of a whole-frame target:
 * each of them gets, bit for bit, what vr_render of the same target writes
 * there; no other byte of `pixels` is touched.  `target` must be a plain
 * whole-frame target (band_rows 0, band_flip 0, no VR_TARGET_* flag), in any
 * format and with any valid row_pitch.  step_counter, when given, has the
 * ray-steps of those pixels added (option "count" as for vr_render).
 *
 * An empty rectangle (width or height 0) is VR_OK and does nothing.
 * VR_ERR_INVALID: a null pointer, a rectangle that is negative or leaves the
 * frame, a band / row-range / in-place target; VR_ERR_NO_VOLUME and
 * VR_ERR_NO_CAMERA as for vr_render.  A refused call writes nothing.
 *
 * Asynchronous on `stream`; allocates nothing and NEVER waits on the host.
 * One wave marches one 8x8 tile of the rectangle and the grid is sized from
 * the rectangle, so the cost follows it (down to the floor its longest ray
 * sets).  The call uses none of the context's cached launches, region lists,
 * cost-sort or deferred-shadow scratch and leaves them as they are: a
 * vr_render before or after it behaves as without it, and a procedural
 * rectangle needs none of vr_render's ordering across streams (its shadow
 * rays are marched in place, its fBm hashes every corner).
 * Uniform channels: the call marches every channel with loads (exact either
 * way), so after a vr_update_volume it neither waits for the pending
 * uniform-channel read-back nor resolves it -- the next vr_render does.
 * Option "inject_throw" is honoured as by vr_render.                       */
vr_status vr_render_rect(void* ctx, const vr_target* target, const vr_rect* rect, void* stream);

/* The scissor for a set of rectangles: render the union of rects[0..count)
 * into a whole-frame target in ONE kernel launch, whatever count is (none
 * when the union is empty).  Apart from what follows the contract is
 * vr_render_rect's: the same targets and formats, every pixel of the union
 * gets bit for bit what vr_render writes there and no other byte of `pixels`
 * is touched, asynchronous on `stream`, nothing allocated, no host wait, the
 * context read and left as it is (cached launches, region lists, sort and
 * deferred-shadow scratch, the pending uniform-channel read-back), every
 * channel loaded, options "inject_throw" and "count" honoured.
 *
 * The rectangles may overlap, repeat, contain one another and be empty, in
 * any order.  A pixel that several of them cover is marched and stored ONCE,
 * so step_counter receives exactly the sum over the union's pixels -- K calls
 * of vr_render_rect would count the overlaps K times -- and the launch pays
 * the floor of its longest ray once, not K times.
 *
 * count == 0 is VR_OK and does nothing (rects may then be NULL).
 * VR_ERR_INVALID: count < 0, count > VR_MAX_RECTS, rects NULL with count > 0,
 * ANY rectangle of the list that is negative or leaves the frame, and
 * everything vr_render_rect refuses.  A refused call writes nothing, not even
 * the valid rectangles before the bad one.  More than VR_MAX_RECTS
 * rectangles, or many tiny ones: vr_rects_coalesce first.                  */
#define VR_MAX_RECTS 64
vr_status vr_render_rects(void* ctx, const vr_target* target, const vr_rect* rects, int count, void* stream);

/* Shorten a rectangle list: writes at most max_out (>= 1) rectangles to `out`
 * (room for min(count, max_out)) and their number to *out_count.  Their union
 * contains the union of the input, and each lies inside the bounding
 * rectangle of the non-empty inputs.  Empty inputs are dropped, and so are
 * inputs contained in another input (of identical ones the first is kept);
 * what remains keeps its order.  While more than max_out remain, the pair
 * whose bounding rectangle adds the least area beyond the two rectangles
 * themselves is merged into that bounding rectangle, at the place of the
 * pair's first (ties: the lowest pair of indices), and whatever the new
 * rectangle contains is dropped.  Deterministic; areas and sums in 64 bits.
 * Pure host code: no context, no device.
 * VR_ERR_INVALID: count < 0, max_out < 1, a null pointer with count > 0, a
 * negative coordinate or extent, x + width or y + height above INT32_MAX (no
 * vr_rect could hold a bounding rectangle).  count == 0 is VR_OK; *out_count,
 * when given, is then 0.                                                   */
vr_status vr_rects_coalesce(const vr_rect* in, int count, int max_out, vr_rect* out, int* out_count);

/* Which pixels can an edit change?  *out = one rectangle inside the
 * width x height frame that contains every pixel whose value, for ANY volume
 * contents, can depend on a texel of the box [x0,x0+bx) x [y0,y0+by) x
 * [z0,z0+bz) of an nx x ny x nz volume, rendered with this shader data and
 * these march constants.  So: render the frame whole, vr_update_volume the
 * box, vr_render_rect the footprint into the same buffer -- the buffer is
 * then bit for bit the whole frame of the patched volume.  The rectangle may
 * be empty (width = height = 0: no ray reads the box, or it projects off the
 * frame) and it may be the whole frame: always when a corner of the box's
 * image lies at or behind the eye, when the eye is inside the volume's box,
 * when Projection*View or WorldToLocal is singular, and when CameraPosition
 * is not the View eye (the rays then do not leave the projection centre).
 * Pure host code in double precision: no context, no device.  All four taps,
 * their scales, the MediaScroll offsets and mirrored repeat are followed
 * (DESIGN.md sec. 5.2.2).  The procedural medium reads no volume.
 * VR_ERR_INVALID: a null pointer, a non-positive extent, volume or frame
 * size, a box that leaves the volume.                                      */
vr_status vr_volume_box_footprint(const vr_object_shader_data* osd, const vr_global_shader_data* gsd,
                                  const vr_march_params* march, int nx, int ny, int nz,
                                  int width, int height,
                                  int x0, int y0, int z0, int bx, int by, int bz, vr_rect* out);
/* The same with the context's current shader data, march constants and
 * volume dimensions; VR_ERR_NO_VOLUME / VR_ERR_NO_CAMERA before they are set. */
vr_status vr_update_footprint(void* ctx, int width, int height,
                              int x0, int y0, int z0, int bx, int by, int bz, vr_rect* out);

/* ---- the ray query: which part of the volume does a pixel see?  The
 *      opposite question to vr_update_footprint, and no reference counterpart:
 *      the reference's fragment keeps only outColor (frag.glsl:80).  One
 *      record is one ray as vr_render marches it.  64 bytes.               */
typedef struct {
    int32_t steps;          /* executed ray-steps (frag.glsl:46 actualSteps, fewer
                               where early_out stops the ray): exactly what this
                               pixel adds to step_counter under option "count" 0;
                               -1 = the pixel is not covered (vr_render writes
                               the background there)                         */
    int32_t hit_step;       /* first step that passes `threshold`, see below;
                               -1 = none                                     */
    float   value;          /* the pixel's VR_FMT_R32F value, bit for bit
                               (frag.glsl:79-80)                             */
    float   optical_depth;  /* acc * step_size of the view ray (frag.glsl:76), fp32 */
    float   entry[3];       /* Pin in [0,1]^3 after frag.glsl:49-53          */
    float   reserved0;      /* 0                                             */
    float   step[3];        /* stepVec after frag.glsl:54                    */
    float   reserved1;      /* 0                                             */
    float   hit[3];         /* sample point of step hit_step (Pin at that
                               iteration of frag.glsl:64-75); zeros if none  */
    float   reserved2;      /* 0                                             */
} vr_ray_record;
/* Write the records of the pixels [x, x+width) x [y, y+height) of the
 * width x height frame to `d_records`, a DEVICE buffer of rect->height rows of
 * row_pitch_records records (0 = tightly packed, rect->width), 16-byte
 * aligned: the rectangle's pixel (x + i, y + j) is record j * pitch + i.
 * Pixels outside the rectangle have no record and nothing else of the buffer
 * is written.  No pixel buffer is involved.
 *
 * value is what vr_render of the same context stores at that pixel in
 * VR_FMT_R32F, bit for bit: the query's march repeats the render's fp32
 * operations in the render's order.  entry, step and steps are the ray setup
 * of frag.glsl:36-55; optical_depth the accumulated `accumulatedTransmission *
 * stepSize` of :76.  A pixel the box does not cover has steps = hit_step = -1,
 * value = the background (0) and zeros elsewhere; a covered ray too short for
 * one step has steps = 0.
 *
 * `threshold` has the meaning and the validation of
 * vr_march_params.early_out: a transmittance in [0,1), 0 = off, and it needs
 * density > 0.  Its accumulator limit L is computed by the expression that
 * turns early_out into the march's own limit; hit_step is the smallest step
 * index i such that the fp32 accumulator AFTER step i exceeds L, and hit the
 * fp32 sample point of that step as marched (entry with step added hit_step
 * times, in that order).  So a query with threshold T on a context without
 * early_out names the step after which a context with early_out = T stops
 * the ray: that context executes hit_step + 1 steps.  The search covers
 * executed steps only; the context's own early_out, if set, ends it.
 *
 * Procedural medium (with and without shadow rays): value is the rendered
 * radiance; optical_depth, hit_step and hit refer to the VIEW ray's
 * accumulator; steps counts ray-steps whatever option "count" says.
 *
 * An empty rectangle is VR_OK and does nothing.  VR_ERR_INVALID: a null
 * pointer, a non-positive frame size, a rectangle that is negative or leaves
 * the frame, a pitch below the rectangle's width, a misaligned buffer, a bad
 * threshold; VR_ERR_NO_VOLUME and VR_ERR_NO_CAMERA as for vr_render.  A
 * refused call writes nothing.
 *
 * Otherwise the contract is vr_render_rect's: asynchronous on `stream`;
 * allocates nothing and NEVER waits on the host; one wave per 8x8 tile of the
 * rectangle; uses and disturbs none of the context's cached launches, region
 * lists, cost-sort or deferred-shadow scratch, nor the pending
 * uniform-channel read-back; every channel marched with loads; option
 * "inject_throw" honoured.                                                 */
vr_status vr_query_rect(void* ctx, int width, int height, const vr_rect* rect,
                        float threshold, void* d_records, size_t row_pitch_records,
                        void* stream);

/* ---- multi-GPU frame assembly.  The band sets of `nranks` ranks are
 *      gathered into one device buffer, d_gathered = [rank][packed rows].
 *      Each rank's set holds `rows_per_rank` rows.  This call scatters them
 *      into the full frame.  Rank r rendered with band_stride = nranks and
 *      band_first = r.  The layout matches vr_render's packed output.
 *      bytes_per_pixel: 1, 4 or 16 (the target format's pixel size).      */
vr_status vr_assemble_bands(void* ctx, const void* d_gathered, size_t rows_per_rank,
                            int nranks, int width, int height, int band_rows,
                            int bytes_per_pixel, void* d_frame, void* stream);
/* The same scatter between formats: band sets gathered in `gathered_format`
 * into a frame in `frame_format`.  Equal formats copy (vr_assemble_bands);
 * a grey set expands into its RGBA format: R8_UNORM -> RGBA8_UNORM,
 * R8_SRGB -> RGBA8_SRGB, R32F -> RGBA32F (G = B = R, A = 255 / 1.0), so the
 * gather moves a quarter of the bytes.  Other pairs are VR_ERR_INVALID.   */
vr_status vr_assemble_frame(void* ctx, const void* d_gathered, int gathered_format, size_t rows_per_rank,
                            int nranks, int width, int height, int band_rows, int frame_format,
                            void* d_frame, void* stream);
/* vr_assemble_frame for the ranks first_rank .. nranks-1 only: the rows of
 * ranks below first_rank are left untouched (rendered in place, with
 * VR_TARGET_BANDS_IN_PLACE); their gather slots are not read.
 * frame_format | VR_ASSEMBLE_SERPENTINE: rank r rendered its set with
 * band_flip nranks-1-2r (the serpentine deal, vr_target).                 */
#define VR_ASSEMBLE_SERPENTINE 0x400
vr_status vr_assemble_frame_ranks(void* ctx, const void* d_gathered, int gathered_format, size_t rows_per_rank,
                                  int nranks, int first_rank, int width, int height, int band_rows,
                                  int frame_format, void* d_frame, void* stream);
/* rows that vr_render writes for a band set (for sizing buffers): whole
 * bands, the set's last partial one included                             */
int vr_band_rows_packed(int height, int band_rows, int band_stride, int band_first, int band_flip);
/* Split the frame's rows into `parts` contiguous ranges of equal estimated
 * march work for the ctx's current camera and march constants (host, double;
 * the same inputs give the same split on every rank).  row_begin[parts + 1]:
 * range k is [row_begin[k], row_begin[k + 1]); row_begin[0] = 0,
 * row_begin[parts] = height, the others multiples of 8 or height
 * (VR_TARGET_ROW_RANGE).  The estimate per ray that meets the box is
 * n^(row_pow / 100) + row_setup, n its a3 step count (frag.glsl:46), sampled
 * every 8th pixel of every 8th row (vr_set_option "row_pow", default 130,
 * and "row_setup", default 40: long rays cost more than their steps, the
 * longest waves bound a small share's launch); range 0 takes
 * "row_first_pct" (default 100) % of a mean share.                        */
vr_status vr_row_partition(void* ctx, int width, int height, int parts, int* row_begin);
/* vr_row_partition corrected by measurement: range k of the previous split
 * prev_begin[parts + 1] took prev_ms[k] (any unit, >= 0; 0 = not measured);
 * each of its strips' estimated work is scaled by prev_ms[k] / (the model's
 * work of range k), and the frame is split again (vr_shard_rebalance_rows). */
vr_status vr_row_partition_measured(void* ctx, int width, int height, int parts, const int* prev_begin,
                                    const double* prev_ms, int* row_begin);

/* The estimate vr_row_partition splits: the march work of every 8-row strip
 * of a width x height frame for the ctx's current camera and march constants
 * (strip_work[nstrips], nstrips = ceil(height / 8); host, double; the same
 * inputs give the same values on every rank).  vr_shard_balance_lead sizes
 * rank 0's lead rows from it.  New (no reference counterpart).            */
vr_status vr_row_work(void* ctx, int width, int height, double* strip_work, int nstrips);

/* ---- introspection: the kernel variant vr_render will launch ----------- */
/* returns a static string, e.g. "grid_pad16_clamp"                        */
const char* vr_kernel_variant(void* ctx);
/* Choose the device volume layout: 0 = auto (default),
 * 1 = planar only, 2 = 4^3 apron bricks in 128-B lines ("brick5"),
 * 3 = 7^3 apron bricks of 512 B ("brick8"), 4 = 15^3 apron bricks of 4 KiB
 * ("brick16"), 5 = 8-corner footprint words ("corner8"), 6 = 3^3 apron
 * bricks of 64 B ("brick4"), 7 = 4x16x2-texel bricks of 128 B whose
 * rows run z-fastest, one 16-B load per tap ("zpair"), 8 = 4x4x8-texel
 * bricks of 128 B ("brick448"), 9 = 4x8x8-texel bricks of 256 B
 * ("brick488"), 10 = 4x8x16-texel bricks of 512 B ("brick4816"),
 * 11 = 4x16x16-texel bricks of 1 KiB ("brick41616"), 12 = 4x8x32-texel
 * bricks of 1 KiB ("brick4832"), 13 = 4x8x64-texel bricks of 2 KiB
 * ("brick4864"), 14 = per position the f16 pairs {a, b - a} of the four
 * footprint rows, one 16-B load and four v_fma_mix_f32 per tap ("cornerh";
 * volumes below 2^24 positions), 15 = columns of 4x8 texels through the
 * whole z extent, slices 32 B apart ("col48"; auto above 160 MiB), 16 = col48
 * for channels 0-2 and zpair for channel 3 ("col48z").  Layouts 2-16 are
 * used only where clamp-to-edge equals mirrored repeat.  Otherwise the
 * planar, mirrored-repeat kernel runs.  Rebuilds the layout (synchronous). */
vr_status vr_set_layout_preference(void* ctx, int pref);
/* Tuning knobs.
 *   "layout"          as vr_set_layout_preference.
 *   "schedule"        -1 = auto (the default); 0 = one static 16x16 tile per
 *                     workgroup, tile rows dealt to XCDs; 1 = persistent waves
 *                     pulling 8x8 tiles from per-XCD queues; 2 = each wave
 *                     renders "tiles_per_wave" strided 8x8 tiles; 3 = 8-px
 *                     tile rows dealt to XCDs; 4 = rings of 8x8 tiles around
 *                     the projected box centre, longest rays first; 5 =
 *                     regions: each XCD renders "wedges" contiguous angular
 *                     wedges of tiles around the box centre with equal
 *                     estimated work, inside-out (auto for the volume; the
 *                     lists are rebuilt on the host when the geometry
 *                     changes, at most every 32 renders for a moving camera).
 *                     Procedural medium: auto = cost-sorted pixels, 0 = 8x8
 *                     tiles in row order, 4 = rings.
 *   "waves_per_simd"  1-8, queue schedule.
 *   "tiles_per_wave"  1-64, strided, ring and region schedules; 0 = auto,
 *                     the default: 2 for rings, 3 for regions on the col48
 *                     layout and 2 on the others, 1 for strided.
 *   "wedges"          1-64, regions schedule: wedges per XCD; 0 = auto (the
 *                     default): 4 while frames_overlap is set (frames in
 *                     flight on several streams), else 8.  vr_get_option
 *                     returns the count in force.
 *   "supertile"       1, 2, 4, regions schedule: the tile lists are ordered by
 *                     S x S blocks of 8x8 tiles (default 2), so a workgroup's
 *                     waves render one block.
 *   "region_order"    regions schedule, each XCD's list: 2 (default) = S x S
 *                     blocks by their longest estimated tile, longest first;
 *                     1 = tiles by estimate, longest first; 0 = inside-out
 *                     (ring around the projected box centre, then angle).
 *   "wg_waves"        4 (default), 8, 16: waves per workgroup of the regions
 *                     march (col48, brick4832, cornerh).
 *   "slab"            0/1, col48 + regions: the per-wave LDS slab march
 *                     (the north star's "per-tile density slabs staged in
 *                     LDS", bit-exact; measured slower, so 0 is the
 *                     default); "slab_cap" 0-32 chunks per channel.
 *   "split"           regions schedule, brick4/448/488/zpair/corner8: lanes per ray
 *                     (1, 2, 4, 8; each lane marches every K-th step and the
 *                     terms are summed in step order, bit-exact); 0 = auto,
 *                     the default: 2 or 4 when the target has too few rays
 *                     to fill the GPU (a 1/N share of a frame).
 *   "count"           0 = vr_target.step_counter sums executed ray-steps (the
 *                     default); 1 = it sums density evaluations, i.e.
 *                     ray-steps plus the procedural shadow samples -- the unit
 *                     of the procedural roofline; 2 = the Worley cells those
 *                     evaluations computed.
 *   "uniform_skip"    1 (default) = a channel whose texels all hold one byte value
 *                     (found when the volume is installed; the reference recipe's
 *                     G, TestMain.cpp:60) is sampled as the exact constant v/255
 *                     with no loads; 0 = every channel is loaded.
 *   "uniform_mask"    read-only (vr_get_option): bit c set = channel c uniform.
 *   "blur_scratch_kib" vr_blur's staging scratch: set k > 0 = hold at least k
 *                     KiB from now on (a device synchronisation, then the
 *                     allocation, in whole MiB; never shrinks), 0 = free it;
 *                     vr_get_option returns the KiB held now.
 *   "region_work_tiles" read-only: 8x8 tiles with estimated work in the current
 *                     region lists (what the auto split K is chosen from).
 *   "sort_reuse"      0-64, procedural sorted schedule: renders that may march
 *                     the cost order of an older camera (default 0).
 *   "proc_enum"       0/1, procedural sort with shadow rays: enumerate
 *                     64x64 regions (default 0, row-major; the deferred
 *                     shadow passes always enumerate regions).
 *   "shadow_defer"    procedural medium with shadow rays, sorted schedule:
 *                     1 (default) = the primary march appends its
 *                     shadow-ray origins, one pass evaluates them all and a
 *                     resolve pass folds them per ray in step order;
 *                     0 = each wave deals its own shadow samples at every
 *                     step (at most 8 shadow steps).  Results are identical.
 *                     The deferred passes keep a device scratch sized from
 *                     the frame: ~16 B per executed ray-step x 5/4 (0.35 GB at
 *                     1080p x 128, ~2.7 GB at 3840 x 2160 x 256), grown when a
 *                     frame needs more (a wave past it marches its shadow rays
 *                     in place, exactly); setting "shadow_defer" 0 or
 *                     "shadow_defer_mib" 0 frees it (after a device sync).
 *                     "shadow_blocks" 0-65536: workgroups of the deferred
 *                     shadow pass (0 = auto, 3/8 of the sorted waves).
 *                     "shadow_defer_mib": the largest scratch the deferred
 *                     passes may allocate (default 4096); "shadow_defer_entries"
 *                     a fixed entry capacity (tests; 0 = from the frame).
 *                     Read-only: "shadow_defer_kib" the scratch held now,
 *                     "shadow_defer_last" 1 if the last procedural render ran
 *                     the deferred passes.
 *   "lattice"         procedural medium, sorted schedule: 1 = the fBm reads its
 *                     per-cell gradient-pair offsets from a lattice table in
 *                     global memory (the default; built when the seed or the
 *                     lattice range changes, at most 2^24 cells, 128 MiB);
 *                     0 = it hashes every corner.  Results are identical.
 *   "quad_pairs"      0/1, vr_render_group of four frames of one camera on
 *                     col48 / brick4832, where "frame_quad", "quad_split" and
 *                     "quad_steps" (each 0/1, default 1) select the march by
 *                     rounds of four steps: 1 (default) = the four lanes of a
 *                     ray load each round's texels in pairs of z-slices, so
 *                     one load instruction names fewer cache lines; 0 = every
 *                     lane loads its own step.  Results are identical.
 *                     Read-only: "quad_pairs_launches", such launches so far
 *                     (they also count in "quad_steps_launches",
 *                     "quad_split_launches" and "quad_launches").
 * vr_get_option returns -1 for an unknown name.                           */
vr_status vr_set_option(void* ctx, const char* name, int value);
int       vr_get_option(void* ctx, const char* name);

/* ---- measurement: the device's streaming bandwidth, the measured HBM
 *      roofline the bench reports next to the 8 TB/s spec.
 *      vr_measure_bandwidth: one pass of 16 B per lane over `bytes`, the grid
 *      as large as the buffer, `loads_per_lane` (4, 8 or 16) independent loads
 *      in flight per lane, 0 = each of 4, 8, 16 (the best is reported), `reps`
 *      times on `stream`, each timed with HIP events.
 *        kind VR_BW_COPY: float4 copy between two fresh buffers; bytes moved
 *                         = read + written (2 x bytes);
 *        kind VR_BW_READ: loads only, folded into a register, nothing stored;
 *                         bytes moved = bytes (the ray march is ~98 % reads).
 *      *gbs_best and *gbs_median in GB/s; *loads_best (may be NULL) = the
 *      loads per lane of the best rep.  Synchronous.
 *      vr_measure_copy_bandwidth = kind VR_BW_COPY at 4 loads per lane.     */
#define VR_BW_COPY 0
#define VR_BW_READ 1
vr_status vr_measure_bandwidth(void* ctx, int kind, int loads_per_lane, size_t bytes, int reps, void* stream,
                               double* gbs_best, double* gbs_median, int* loads_best);
vr_status vr_measure_copy_bandwidth(void* ctx, size_t bytes, int reps, void* stream, double* gbs_best,
                                    double* gbs_median);

#ifdef __cplusplus
}
#endif
#endif /* VR_H */
