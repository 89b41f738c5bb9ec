// warp_check -- stand-alone host check of vr_brush_warp_apply, vr_warp_reach and
// vr_warp_push (volumetricrenderer_amd/csrc/vr_brush.cpp, vr_warp.h), built with
// -fsanitize=address,undefined and run on the CPU (`make check-warp` builds and
// runs it).  It links the brush's translation unit only: no libvr.so, no HIP, no
// device.
//
// Every volume is allocated exactly, so a read or write outside one trips the
// address sanitizer, and an overflow in a position trips the undefined-behaviour
// sanitizer.  Random volumes, brushes and maps -- pushes, turns, scales up to the
// displacement limit, both filters and borders, both falloffs.  Each result is
// compared with a naive restatement of vr.h: a full copy of the volume before
// the call, plain loops over every texel, the ellipsoid in unsigned __int128,
// positions in __int128 with a floor division by 256 and the trilinear value as
// one sum over eight corners.  Then the three identities (the identity map, a
// hard warp against vr_brush_clone_affine_apply, a constant channel), the
// corner bound of vr_warp_reach by brute force over every texel of small boxes,
// the limit itself, and the push builder.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "check_common.hpp"

namespace {

// the shared failure counter, with the failed condition and its line on stdout
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++failures <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                   \
    } while (0)

i128 floor_div(i128 a, i128 b)   // b > 0
{
    const i128 q = a / b;
    return a % b < 0 ? q - 1 : q;
}

i128 affine_position(const vr_affine& m, int a, const long long t[3])
{
    i128 p = m.origin[a];
    for (int b = 0; b < 3; ++b) p += (i128)m.m[a][b] * ((i128)t[b] - m.pivot[b]);
    return p;
}

// vr.h, literally: the new volume from a copy of the old one
std::vector<uint8_t> naive(const vr_brush& b, const vr_affine& m, const std::vector<uint8_t>& vol, int nx, int ny, int nz)
{
    std::vector<uint8_t> out = vol;
    const int n[3] = {nx, ny, nz};
    const auto at = [&](long long x, long long y, long long z, int c) -> unsigned long long {
        return vol.at(((size_t)(z * ny + y) * (size_t)nx + (size_t)x) * 4 + (size_t)c);
    };
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const unsigned w = weight(b, x, y, z);
                if (!w) continue;
                const long long t[3] = {x, y, z};
                i128 P[3];
                bool outside = false;
                for (int a = 0; a < 3; ++a) {
                    const i128 I = (i128)t[a] * 65536, D = affine_position(m, a, t) - I;
                    P[a] = I + floor_div((i128)w * D, 256);
                    const i128 last = (i128)(n[a] - 1) * 65536;
                    if (P[a] < 0 || P[a] > last) outside = true;
                    P[a] = P[a] < 0 ? 0 : P[a] > last ? last : P[a];
                }
                if (outside && m.border == VR_BORDER_SKIP) continue;
                long long i[3], f16[3];
                for (int a = 0; a < 3; ++a) { i[a] = (long long)(P[a] / 65536); f16[a] = (long long)(P[a] % 65536); }
                for (int c = 0; c < 4; ++c) {
                    if (!b.strength[c]) continue;
                    unsigned long long v;
                    if (m.filter == VR_FILTER_NEAREST) {
                        v = at(i[0] + (f16[0] >= 0x8000), i[1] + (f16[1] >= 0x8000), i[2] + (f16[2] >= 0x8000), c);
                    } else {
                        unsigned long long sum = 0, total = 0;
                        for (int k = 0; k < 8; ++k) {
                            unsigned long long wk = 1;
                            long long s[3];
                            for (int a = 0; a < 3; ++a) {
                                const long long f = f16[a] / 256;
                                const bool second = (k >> a & 1) != 0;
                                s[a] = second ? (i[a] + 1 > n[a] - 1 ? n[a] - 1 : i[a] + 1) : i[a];
                                wk *= (unsigned long long)(second ? f : 256 - f);
                            }
                            total += wk;
                            if (wk) sum += wk * at(s[0], s[1], s[2], c);
                        }
                        EXPECT(total == 1ull << 24);
                        v = (sum + (1ull << 23)) >> 24;
                    }
                    const unsigned long long old = at(x, y, z, c), a = 256ull * b.strength[c];
                    out[((size_t)(z * ny + y) * (size_t)nx + (size_t)x) * 4 + (size_t)c] =
                        (uint8_t)((old * (65280 - a) + v * a + 32640) / 65280);
                }
            }
    return out;
}

vr_brush make_brush(std::mt19937& rng, int nx, int ny, int nz, int falloff)
{
    vr_brush b{};
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        b.centre[a] = (int)(rng() % (unsigned)(n[a] + 6)) - 3;
        b.radius[a] = (int)(rng() % 12u);
    }
    b.op = VR_BRUSH_SET;
    b.falloff = falloff;
    for (int c = 0; c < 4; ++c) {
        b.value[c] = (uint8_t)rng();
        b.strength[c] = rng() % 4u == 0u ? 0 : (uint8_t)rng();
    }
    return b;
}

vr_affine make_map(std::mt19937& rng, const vr_brush& b, int kind)
{
    vr_affine m{};
    for (int a = 0; a < 3; ++a) {
        m.m[a][a] = VR_AFFINE_ONE;
        m.pivot[a] = b.centre[a];
        m.origin[a] = (int32_t)(uint32_t)((int64_t)b.centre[a] * 65536);   // wraps for a centre past +-32767: any origin will do
    }
    if (kind == 1)   // a push by up to +-4 texels
        for (int a = 0; a < 3; ++a) m.origin[a] += (int)(rng() % (8u << 16)) - (4 << 16);
    if (kind == 2)   // any small matrix: turns, shears, scales, flips
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) m.m[a][c] = (int)(rng() % (6u << 16)) - (3 << 16);
    if (kind == 3) {  // the largest coefficients, and a far origin
        for (int a = 0; a < 3; ++a) m.m[a][(a + 1) % 3] = rng() & 1u ? VR_AFFINE_MAX_COEFF : -VR_AFFINE_MAX_COEFF;
        m.origin[0] += (int)(rng() % (1u << 30));
    }
    m.filter = (int)(rng() & 1u);
    m.border = (int)(rng() & 1u);
    return m;
}

void check_apply()
{
    std::mt19937 rng(20240611);
    int applied = 0, changed = 0;
    for (int it = 0; it < 400; ++it) {
        const int nx = 1 + (int)(rng() % 13u), ny = 1 + (int)(rng() % 11u), nz = 1 + (int)(rng() % 9u);
        std::vector<uint8_t> vol((size_t)nx * ny * nz * 4);
        for (auto& v : vol) v = (uint8_t)rng();
        const vr_brush b = make_brush(rng, nx, ny, nz, it & 1);
        const vr_affine m = make_map(rng, b, it % 4);
        std::vector<uint8_t> got = vol;
        const vr_status st = vr_brush_warp_apply(&b, &m, got.data(), nx, ny, nz);
        int32_t reach[3];
        EXPECT(vr_warp_reach(&b, &m, reach) == VR_OK);
        if (st != VR_OK) {   // only the reach can refuse these
            EXPECT(reach[0] == INT_MAX || reach[1] == INT_MAX || reach[2] == INT_MAX);
            EXPECT(got == vol);
            continue;
        }
        ++applied;
        const std::vector<uint8_t> want = naive(b, m, vol, nx, ny, nz);
        EXPECT(got == want);
        changed += want != vol;
        // a hard warp is the transform paste
        if (!b.falloff) {
            std::vector<uint8_t> paste = vol;
            EXPECT(vr_brush_clone_affine_apply(&b, &m, paste.data(), nx, ny, nz) == VR_OK);
            EXPECT(paste == got);
        }
        // the identity map changes nothing, whatever the filter, border and falloff
        vr_affine id = make_map(rng, b, 0);
        std::vector<uint8_t> same = vol;
        EXPECT(vr_brush_warp_apply(&b, &id, same.data(), nx, ny, nz) == VR_OK);
        EXPECT(same == vol);
        // a constant channel stays constant
        std::vector<uint8_t> flat = vol;
        for (size_t i = 1; i < flat.size(); i += 4) flat[i] = 77;
        EXPECT(vr_brush_warp_apply(&b, &m, flat.data(), nx, ny, nz) == VR_OK);
        bool constant = true;
        for (size_t i = 1; i < flat.size(); i += 4) constant = constant && flat[i] == 77;
        EXPECT(constant);
    }
    EXPECT(applied > 250 && changed > 100);
    std::printf("apply: %d maps applied, %d changed the volume\n", applied, changed);
}

// max |D_a| over EVERY texel of the unclipped box equals the value at the corners
void check_reach()
{
    std::mt19937 rng(7);
    for (int it = 0; it < 300; ++it) {
        vr_brush b{};
        for (int a = 0; a < 3; ++a) {
            b.centre[a] = (int)(rng() % 2001u) - 1000;
            b.radius[a] = (int)(rng() % 6u);
        }
        if (it == 0) { b.centre[0] = INT_MAX; b.centre[1] = INT_MIN; }
        vr_affine m = make_map(rng, b, 1 + it % 3);
        if (it % 5 == 0)
            for (int a = 0; a < 3; ++a) { m.pivot[a] = (int)rng(); m.origin[a] = (int)rng(); }
        int32_t got[3];
        EXPECT(vr_warp_reach(&b, &m, got) == VR_OK);
        i128 want[3] = {0, 0, 0};
        for (long long z = (long long)b.centre[2] - b.radius[2]; z <= (long long)b.centre[2] + b.radius[2]; ++z)
            for (long long y = (long long)b.centre[1] - b.radius[1]; y <= (long long)b.centre[1] + b.radius[1]; ++y)
                for (long long x = (long long)b.centre[0] - b.radius[0]; x <= (long long)b.centre[0] + b.radius[0]; ++x) {
                    const long long t[3] = {x, y, z};
                    for (int a = 0; a < 3; ++a) {
                        i128 d = affine_position(m, a, t) - (i128)t[a] * 65536;
                        if (d < 0) d = -d;
                        if (d > want[a]) want[a] = d;
                    }
                }
        for (int a = 0; a < 3; ++a) EXPECT((i128)got[a] == (want[a] > INT_MAX ? (i128)INT_MAX : want[a]));
    }
    // the limit: exactly VR_WARP_MAX_DISP texels is accepted, one unit of 1 / 65536 more is refused
    vr_brush b{};
    b.centre[0] = 3; b.centre[1] = 2; b.centre[2] = 1;
    b.radius[0] = b.radius[1] = b.radius[2] = 2;
    b.falloff = 1;
    b.strength[0] = b.strength[2] = 255;
    std::vector<uint8_t> vol(7 * 5 * 4 * 4), got;
    std::mt19937 rng2(3);
    for (auto& v : vol) v = (uint8_t)rng2();
    for (int over = 0; over < 2; ++over) {
        vr_affine m{};
        for (int a = 0; a < 3; ++a) { m.m[a][a] = VR_AFFINE_ONE; m.pivot[a] = b.centre[a]; m.origin[a] = b.centre[a] * 65536; }
        m.origin[0] = (int)(3ll * 65536 - ((long long)VR_WARP_MAX_DISP << 16) - over);
        m.filter = VR_FILTER_LINEAR;
        got = vol;
        EXPECT(vr_brush_warp_apply(&b, &m, got.data(), 7, 5, 4) == (over ? VR_ERR_INVALID : VR_OK));
        EXPECT(over ? got == vol : got == naive(b, m, vol, 7, 5, 4));
    }
    vr_brush add = b;
    add.op = VR_BRUSH_ADD;
    vr_affine id{};
    EXPECT(vr_affine_identity(&id) == VR_OK);
    got = vol;
    EXPECT(vr_brush_warp_apply(&add, &id, got.data(), 7, 5, 4) == VR_ERR_INVALID && got == vol);
    std::printf("reach: ok\n");
}

void check_push()
{
    const int32_t c[3] = {17, -4, 32767}, d[3] = {0x18000, -0x8000, INT_MAX};
    vr_affine a{};
    EXPECT(vr_warp_push(c, d, VR_FILTER_LINEAR, VR_BORDER_SKIP, &a) == VR_OK);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) EXPECT(a.m[i][j] == (i == j ? VR_AFFINE_ONE : 0));
        EXPECT(a.pivot[i] == c[i] && (long long)a.origin[i] == (long long)c[i] * 65536 - d[i]);
    }
    EXPECT(a.filter == VR_FILTER_LINEAR && a.border == VR_BORDER_SKIP && a.reserved == 0);
    vr_affine keep;
    std::memset(&keep, 0x5a, sizeof keep);
    const vr_affine before = keep;
    const int32_t far[3] = {32767, 0, 0}, back[3] = {-65536, 0, 0};
    EXPECT(vr_warp_push(far, back, 0, 0, &keep) == VR_ERR_INVALID);   // origin 2^31
    EXPECT(vr_warp_push(c, d, 2, 0, &keep) == VR_ERR_INVALID && vr_warp_push(c, d, 0, 2, &keep) == VR_ERR_INVALID);
    EXPECT(vr_warp_push(nullptr, d, 0, 0, &keep) == VR_ERR_INVALID && vr_warp_push(c, d, 0, 0, nullptr) == VR_ERR_INVALID);
    EXPECT(std::memcmp(&keep, &before, sizeof keep) == 0);
    std::printf("push: ok\n");
}

}  // namespace

int main()
{
    check_apply();
    check_reach();
    check_push();
    if (failures) {
        std::printf("warp_check: %ld FAILURES\n", failures);
        return 1;
    }
    std::printf("warp_check: ok\n");
    return 0;
}
