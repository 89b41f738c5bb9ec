// vr_footprint.cpp -- vr_volume_box_footprint: the pixel rectangle whose rays
// can read a texel box of the volume (include/vr.h).
//
// Pure host code in double precision: no context, no device, no HIP header.
// tools/footprint_check.cpp compiles this file alone (-DVR_FOOTPRINT_STANDALONE,
// which only drops the vr_last_error text) under the address and
// undefined-behaviour sanitizers.
//
// Geometry.  A pixel's ray is the line from the View eye through the pixel
// centre, carried to box-local space by WorldToLocal (vr_camera.cpp
// make_ray_basis), so a box-local point Q that the ray samples projects, by
// Projection * View * inverse(WorldToLocal), onto that pixel centre.  Tap t
// samples u = P * s_t + o_t per axis (P = the box point in [0,1]^3) and its
// trilinear fetch at u*N - 0.5 reads texels floor and floor + 1 under
// mirrored repeat, so texel i is read for fold(u*N) in (i - 0.5, i + 1.5).
// Per tap and axis the pre-images of the box's interval in P are enumerated
// (every reflection that meets the tap's range), widened by the march's
// rounding drift, multiplied out to boxes in P, transformed and projected; the
// answer is the bounding rectangle of all projected corners, rounded
// outwards, plus one pixel, clipped to the frame.  Anything the projection
// cannot bound (a corner at or behind the eye, a singular matrix, rays that do
// not leave the projection centre, a non-finite number) gives the whole frame.
#include <cmath>
#include <cstdint>
#include <utility>

#include "../../include/vr.h"

#ifdef VR_FOOTPRINT_STANDALONE
namespace {
vr_status fail(vr_status st, const char*, ...) { return st; }
}
#else
#include "vr_ctx.h"
using vrapi::fail;
#endif

namespace {

// 4x4 inverse, Gauss-Jordan with partial pivoting (column-major in and out)
bool invert4(const double* m, double* inv)
{
    double a[4][8];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            a[r][c] = m[c * 4 + r];
            a[r][4 + c] = r == c ? 1.0 : 0.0;
        }
    for (int k = 0; k < 4; ++k) {
        int piv = k;
        for (int r = k + 1; r < 4; ++r)
            if (std::fabs(a[r][k]) > std::fabs(a[piv][k])) piv = r;
        if (!(std::fabs(a[piv][k]) > 0.0) || !std::isfinite(a[piv][k])) return false;
        for (int c = 0; c < 8; ++c) std::swap(a[k][c], a[piv][c]);
        const double d = 1.0 / a[k][k];
        for (int c = 0; c < 8; ++c) a[k][c] *= d;
        for (int r = 0; r < 4; ++r) {
            if (r == k) continue;
            const double f = a[r][k];
            if (f != 0.0)
                for (int c = 0; c < 8; ++c) a[r][c] -= f * a[k][c];
        }
    }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            if (!std::isfinite(a[r][4 + c])) return false;
            inv[c * 4 + r] = a[r][4 + c];
        }
    return true;
}

void mul4(const double* a, const double* b, double* o)   // o = a * b, column-major
{
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[k * 4 + r] * b[c * 4 + k];
            o[c * 4 + r] = s;
        }
}

struct Interval {
    double lo, hi;
};
// Pre-image intervals of one tap and axis, at most kMaxIntervals: a tap range
// that spans more reflections than that keeps their hull (conservative).
constexpr int kMaxIntervals = 8;
struct IntervalSet {
    int n = 0;
    Interval v[kMaxIntervals];
    void add(double lo, double hi)
    {
        if (n < kMaxIntervals) {
            v[n++] = Interval{lo, hi};
            return;
        }
        double l = lo, h = hi;
        for (int i = 0; i < n; ++i) {
            l = std::fmin(l, v[i].lo);
            h = std::fmax(h, v[i].hi);
        }
        v[0] = Interval{l, h};
        n = 1;
    }
};

// P in [0,1] (widened by `slack`) for which tap coordinate v = (P*s + o)*N
// lies within `margin` of an image of (x0 - 0.5, x0 + b + 0.5) under the
// reflections v -> 2Nk + v and v -> 2Nk - v.  False: not finite.
bool axis_preimages(double s, double o, int N, int x0, int b, double slack, double margin, IntervalSet* out)
{
    const double n = (double)N, lo = (double)x0 - 0.5 - margin, hi = (double)(x0 + b) + 0.5 + margin;
    const double plo = -slack, phi = 1.0 + slack;
    const double va = (plo * s + o) * n, vb = (phi * s + o) * n;
    const double vmin = std::fmin(va, vb), vmax = std::fmax(va, vb);
    if (!std::isfinite(vmin) || !std::isfinite(vmax)) return false;
    const double period = 2.0 * n;
    const double k0 = std::floor((vmin - hi) / period) - 1.0, k1 = std::ceil((vmax + hi) / period) + 1.0;
    if (k1 - k0 > 4.0 * kMaxIntervals || s == 0.0) {
        // too many reflections to list, or a constant tap: all of P (a constant
        // tap that misses every image reads nothing of the box)
        if (s == 0.0) {
            bool hit = false;
            for (double k = k0; k <= k1 && !hit; k += 1.0)
                hit = (vmin >= lo + period * k && vmin <= hi + period * k) ||
                      (vmin >= period * k - hi && vmin <= period * k - lo);
            if (!hit) return true;
        }
        out->add(plo, phi);
        return true;
    }
    for (double k = k0; k <= k1; k += 1.0)
        for (int refl = 0; refl < 2; ++refl) {
            const double a = refl ? period * k - hi : period * k + lo;
            const double c = refl ? period * k - lo : period * k + hi;
            if (c < vmin || a > vmax) continue;
            const double pa = (std::fmax(a, vmin) / n - o) / s, pc = (std::fmin(c, vmax) / n - o) / s;
            out->add(std::fmax(std::fmin(pa, pc) - slack, plo), std::fmin(std::fmax(pa, pc) + slack, phi));
        }
    return true;
}

}  // namespace

extern "C" vr_status vr_volume_box_footprint(const vr_object_shader_data* osd, const vr_global_shader_data* gsd,
                                             const vr_march_params* march, int nx, int ny, int nz, int width,
                                             int height, int x0, int y0, int z0, int bx, int by, int bz, vr_rect* out)
{
    if (!osd || !gsd || !march || !out) return fail(VR_ERR_INVALID, "vr_volume_box_footprint: null argument");
    if (width <= 0 || height <= 0)
        return fail(VR_ERR_INVALID, "vr_volume_box_footprint: bad frame size %dx%d", width, height);
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return fail(VR_ERR_INVALID, "vr_volume_box_footprint: bad volume size %dx%dx%d", nx, ny, nz);
    if (bx <= 0 || by <= 0 || bz <= 0)
        return fail(VR_ERR_INVALID, "vr_volume_box_footprint: bad box extent %dx%dx%d", bx, by, bz);
    if (x0 < 0 || y0 < 0 || z0 < 0 || bx > nx - x0 || by > ny - y0 || bz > nz - z0)
        return fail(VR_ERR_INVALID, "vr_volume_box_footprint: box %dx%dx%d at (%d, %d, %d) leaves the %dx%dx%d volume",
                    bx, by, bz, x0, y0, z0, nx, ny, nz);
    const vr_rect whole{0, 0, width, height};
    *out = whole;

    double V[16], P[16], L[16], PV[16], Li[16], Vi[16], T[16];
    for (int i = 0; i < 16; ++i) {
        V[i] = osd->view[i];
        P[i] = osd->projection[i];
        L[i] = gsd->world_to_local[i];
    }
    mul4(P, V, PV);
    double tmp[16];
    if (!invert4(PV, tmp)) return VR_OK;               // vr_render refuses this camera
    if (!invert4(V, Vi) || !(std::fabs(Vi[15]) > 0.0)) return VR_OK;
    if (!invert4(L, Li)) return VR_OK;
    // cam_mode 1 of make_ray_basis: the march starts at CameraPosition, not at
    // the projection centre, so a sample does not project onto its own pixel
    double err = 0.0, mag = 1.0, eye[3];
    for (int i = 0; i < 3; ++i) {
        eye[i] = Vi[12 + i] / Vi[15];
        err = std::fmax(err, std::fabs(eye[i] - (double)gsd->camera_position[i]));
        mag = std::fmax(mag, std::fabs(eye[i]));
    }
    if (!(err <= 1e-6 * mag)) return VR_OK;
    mul4(PV, Li, T);   // box-local -> clip

    double bmin[3], range[3];
    bool eye_inside = true;
    for (int a = 0; a < 3; ++a) {
        bmin[a] = march->box_min[a];
        range[a] = std::fabs((double)march->box_max[a] - (double)march->box_min[a]);
        if (!std::isfinite(bmin[a]) || !std::isfinite(range[a]) || !(range[a] > 0.0)) return VR_OK;
        const double e = L[0 * 4 + a] * eye[0] + L[1 * 4 + a] * eye[1] + L[2 * 4 + a] * eye[2] + L[3 * 4 + a];
        const double lo = std::fmin(march->box_min[a], march->box_max[a]), hi = std::fmax(march->box_min[a], march->box_max[a]);
        eye_inside = eye_inside && e >= lo && e <= hi;
    }
    if (eye_inside) return VR_OK;   // the eye inside the volume's box

    // the drift of the fp32 ray point over the march, in P (vr_api.cpp
    // clamp_is_exact), and the rounding of the tap coordinate, in texels
    const double slack = ((double)(march->max_steps > 0 ? march->max_steps : 0) + 16.0) * 1.2e-7;
    const int dims[3] = {nx, ny, nz}, b0[3] = {x0, y0, z0}, bn[3] = {bx, by, bz};
    double sx0 = INFINITY, sy0 = INFINITY, sx1 = -INFINITY, sy1 = -INFINITY;
    for (int t = 0; t < 4; ++t) {
        IntervalSet iv[3];
        for (int a = 0; a < 3; ++a) {
            const double s = march->tap_scale[t];
            const double o = (double)gsd->media_scroll[a * 4 + t] * (double)march->tap_weight[t];
            const double margin = (dims[a] + 2.0) * 2.4e-7 + 1e-6 + std::fabs(s * dims[a]) * 2.4e-7;
            if (!axis_preimages(s, o, dims[a], b0[a], bn[a], slack, margin, &iv[a])) return VR_OK;
        }
        for (int i = 0; i < iv[0].n; ++i)
            for (int j = 0; j < iv[1].n; ++j)
                for (int k = 0; k < iv[2].n; ++k)
                    for (int c = 0; c < 8; ++c) {
                        const double p[3] = {(c & 1) ? iv[0].v[i].hi : iv[0].v[i].lo,
                                             (c & 2) ? iv[1].v[j].hi : iv[1].v[j].lo,
                                             (c & 4) ? iv[2].v[k].hi : iv[2].v[k].lo};
                        double q[3];
                        for (int a = 0; a < 3; ++a) q[a] = bmin[a] + p[a] * range[a];
                        double clip[4];
                        for (int r = 0; r < 4; ++r)
                            clip[r] = T[0 * 4 + r] * q[0] + T[1 * 4 + r] * q[1] + T[2 * 4 + r] * q[2] + T[3 * 4 + r];
                        if (!(clip[3] > 1e-9) || !std::isfinite(clip[0]) || !std::isfinite(clip[1]) ||
                            !std::isfinite(clip[3]))
                            return VR_OK;   // at or behind the eye
                        // pixel (x, y)'s centre is at NDC ((x + .5) * 2 / W - 1, (y + .5) * 2 / H - 1)
                        const double sx = (clip[0] / clip[3] + 1.0) * 0.5 * width;
                        const double sy = (clip[1] / clip[3] + 1.0) * 0.5 * height;
                        sx0 = std::fmin(sx0, sx); sx1 = std::fmax(sx1, sx);
                        sy0 = std::fmin(sy0, sy); sy1 = std::fmax(sy1, sy);
                    }
    }
    const vr_rect empty{0, 0, 0, 0};
    if (!(sx0 <= sx1)) {   // no tap reads the box
        *out = empty;
        return VR_OK;
    }
    if (!std::isfinite(sx0) || !std::isfinite(sx1) || !std::isfinite(sy0) || !std::isfinite(sy1)) return VR_OK;
    // pixels whose centre lies in [s0, s1]: rounded outwards, one pixel of margin
    const double w = width, h = height;
    const double fx0 = std::fmax(std::floor(sx0) - 1.0, 0.0), fx1 = std::fmin(std::ceil(sx1) + 1.0, w);
    const double fy0 = std::fmax(std::floor(sy0) - 1.0, 0.0), fy1 = std::fmin(std::ceil(sy1) + 1.0, h);
    if (!(fx0 < fx1 && fy0 < fy1)) {
        *out = empty;
        return VR_OK;
    }
    out->x = (int32_t)fx0;
    out->y = (int32_t)fy0;
    out->width = (int32_t)(fx1 - fx0);
    out->height = (int32_t)(fy1 - fy0);
    return VR_OK;
}
