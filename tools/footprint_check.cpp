// footprint_check -- stand-alone host check of vr_volume_box_footprint
// (volumetricrenderer_amd/csrc/vr_footprint.cpp), built with
// -fsanitize=address,undefined and run on the CPU (`make check-footprint`
// builds and runs it).  It links the footprint's translation unit only: no
// libvr.so, no HIP, no device.
//
// A few thousand seeded random cameras (orbiting, inside the box, degenerate),
// MediaScroll offsets, tap scales (negative, zero, > 1, huge), march boxes,
// volumes, texel boxes and frame sizes: every VR_OK result must lie inside the
// frame, every bad argument must be refused, and nothing may trip a sanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "vr.h"

namespace {

void look_at(const double eye[3], const double ctr[3], float* m)
{
    double f[3] = {ctr[0] - eye[0], ctr[1] - eye[1], ctr[2] - eye[2]};
    const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (double& v : f) v /= fl > 0 ? fl : 1.0;
    const double up[3] = {0, 0, 1};
    double s[3] = {f[1] * up[2] - up[1] * f[2], f[2] * up[0] - up[2] * f[0], f[0] * up[1] - up[0] * f[1]};
    const double sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (double& v : s) v /= sl > 0 ? sl : 1.0;
    const double u[3] = {s[1] * f[2] - f[1] * s[2], s[2] * f[0] - f[2] * s[0], s[0] * f[1] - f[0] * s[1]};
    for (int i = 0; i < 16; ++i) m[i] = 0.0f;
    for (int i = 0; i < 3; ++i) {
        m[i * 4 + 0] = (float)s[i];
        m[i * 4 + 1] = (float)u[i];
        m[i * 4 + 2] = (float)-f[i];
    }
    m[12] = (float)-(s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2]);
    m[13] = (float)-(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]);
    m[14] = (float)(f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2]);
    m[15] = 1.0f;
}

// vr_march_defaults (libvr.so, not linked here): the frag.glsl constants
void march_defaults(vr_march_params* m)
{
    *m = vr_march_params{};
    m->max_steps = 128; m->step_scale = 4.0f; m->density = 1.0f; m->scale = 0.2f;
    const float ts[4] = {1.0f, 0.8f, 0.75f, 0.7f}, tw[4] = {0.0f, 0.2f, 0.25f, 0.3f};
    for (int i = 0; i < 3; ++i) { m->box_min[i] = -1.0f; m->box_max[i] = 1.0f; }
    for (int i = 0; i < 4; ++i) { m->tap_scale[i] = ts[i]; m->tap_weight[i] = tw[i]; }
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20240611);
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    auto pick = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
    long ok = 0, whole = 0, empty = 0, refused = 0, failures = 0;
    for (int it = 0; it < 6000; ++it) {
        vr_object_shader_data osd{};
        vr_global_shader_data gsd{};
        vr_march_params m{};
        // camera: an orbit around the box, sometimes inside it, sometimes degenerate
        const int kind = pick(0, 9);
        const double dist = kind == 0 ? uni(0.0, 1.5) : uni(1.8, 12.0);
        const double th = uni(0.0, 6.283), ph = uni(-1.5, 1.5);
        double eye[3] = {dist * std::cos(th) * std::cos(ph), dist * std::sin(th) * std::cos(ph), dist * std::sin(ph)};
        const double ctr[3] = {uni(-0.5, 0.5), uni(-0.5, 0.5), uni(-0.5, 0.5)};
        look_at(eye, ctr, osd.view);
        const double fov = uni(0.02, 2.6), aspect = uni(0.3, 3.0), zn = 0.1, zf = 10.0;
        const double t = std::tan(fov / 2);
        osd.projection[0] = (float)(1.0 / (aspect * t));
        osd.projection[5] = (float)(-1.0 / t);
        osd.projection[10] = (float)(zf / (zn - zf));
        osd.projection[11] = -1.0f;
        osd.projection[14] = (float)(-(zf * zn) / (zf - zn));
        if (kind == 1) osd.projection[pick(0, 15)] = 0.0f;                 // maybe singular
        if (kind == 2) osd.view[pick(0, 15)] = (float)uni(-2.0, 2.0);      // not a rigid view
        // WorldToLocal: a rotation about z with a scale, sometimes singular
        const double a = uni(0.0, 6.283), sc = kind == 3 ? 0.0 : uni(0.5, 2.0);
        gsd.world_to_local[0] = (float)(sc * std::cos(a)); gsd.world_to_local[1] = (float)(sc * std::sin(a));
        gsd.world_to_local[4] = (float)(-sc * std::sin(a)); gsd.world_to_local[5] = (float)(sc * std::cos(a));
        gsd.world_to_local[10] = (float)sc; gsd.world_to_local[15] = 1.0f;
        for (int i = 0; i < 3; ++i) {
            osd.model[i * 5] = 1.0f;
            gsd.camera_position[i] = (float)eye[i] + (kind == 4 ? (float)uni(-1.0, 1.0) : 0.0f);
        }
        osd.model[15] = 1.0f;
        for (int i = 0; i < 16; ++i) gsd.media_scroll[i] = pick(0, 2) ? (float)uni(-6.0, 6.0) : 0.0f;
        if (kind == 5) gsd.media_scroll[pick(0, 15)] = NAN;
        if (kind == 6) gsd.media_scroll[pick(0, 15)] = INFINITY;
        march_defaults(&m);
        m.max_steps = pick(-2, 512);
        for (int k = 0; k < 4; ++k) {
            const int sk = pick(0, 7);
            m.tap_scale[k] = sk == 0 ? 0.0f : sk == 1 ? (float)uni(-3.0, 0.0) : sk == 2 ? (float)uni(1.0, 40.0)
                            : sk == 3 ? 1e9f : (float)uni(0.05, 1.0);
            m.tap_weight[k] = (float)uni(-1.0, 1.0);
        }
        for (int i = 0; i < 3; ++i) {
            m.box_min[i] = (float)uni(-2.0, 0.0);
            m.box_max[i] = kind == 7 ? m.box_min[i] : (float)uni(0.0, 2.0);
        }
        const int nx = pick(1, 600), ny = pick(1, 600), nz = pick(1, 600);
        const int W = pick(1, 4096), H = pick(1, 2200);
        int x0 = pick(0, nx - 1), y0 = pick(0, ny - 1), z0 = pick(0, nz - 1);
        int bx = pick(1, nx - x0), by = pick(1, ny - y0), bz = pick(1, nz - z0);
        const int bad = pick(0, 11);   // a bad argument now and then
        if (bad == 0) bx = nx - x0 + 1;
        if (bad == 1) by = 0;
        if (bad == 2) z0 = -1;
        vr_rect r{-7, -7, -7, -7};
        const vr_status st = vr_volume_box_footprint(&osd, &gsd, &m, nx, ny, nz, bad == 3 ? 0 : W, H, x0, y0, z0, bx, by,
                                                     bz, bad == 4 ? nullptr : &r);
        if (bad <= 4) {
            if (st != VR_ERR_INVALID || r.x != -7) {
                std::printf("case %d: bad argument %d accepted (status %d)\n", it, bad, (int)st);
                ++failures;
            }
            ++refused;
            continue;
        }
        if (st != VR_OK) {
            std::printf("case %d: status %d\n", it, (int)st);
            ++failures;
            continue;
        }
        const bool is_empty = r.width == 0 && r.height == 0;
        const bool inside = r.x >= 0 && r.y >= 0 && r.width >= 0 && r.height >= 0 && r.width <= W - r.x &&
                            r.height <= H - r.y && ((r.width > 0) == (r.height > 0));
        if (!inside) {
            std::printf("case %d: rectangle (%d, %d, %d, %d) outside the %dx%d frame\n", it, r.x, r.y, r.width, r.height,
                        W, H);
            ++failures;
        }
        ++ok;
        whole += r.x == 0 && r.y == 0 && r.width == W && r.height == H;
        empty += is_empty;
    }
    // null pointers one by one
    vr_object_shader_data osd{};
    vr_global_shader_data gsd{};
    vr_march_params m{};
    vr_rect r{};
    march_defaults(&m);
    failures += vr_volume_box_footprint(nullptr, &gsd, &m, 4, 4, 4, 8, 8, 0, 0, 0, 1, 1, 1, &r) != VR_ERR_INVALID;
    failures += vr_volume_box_footprint(&osd, nullptr, &m, 4, 4, 4, 8, 8, 0, 0, 0, 1, 1, 1, &r) != VR_ERR_INVALID;
    failures += vr_volume_box_footprint(&osd, &gsd, nullptr, 4, 4, 4, 8, 8, 0, 0, 0, 1, 1, 1, &r) != VR_ERR_INVALID;
    std::printf("footprint_check: %ld ok (%ld whole frame, %ld empty), %ld refused, %ld failures\n", ok, whole, empty,
                refused, failures);
    return failures ? 1 : 0;
}
