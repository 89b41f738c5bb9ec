// clone_check -- stand-alone host check of vr_brush_clone_apply,
// vr_brush_stamp_apply and vr_stamp_box
// (volumetricrenderer_amd/csrc/vr_brush.cpp), built with
// -fsanitize=address,undefined and run on the CPU (`make check-clone` builds
// and runs it).  It links the brush's translation unit only: no libvr.so, no
// HIP, no device.
//
// Every volume and every stamp is allocated exactly, so a read or write
// outside one trips the address sanitizer, and a 32-bit sum of a coordinate
// and an offset (or of a placement's origin and extent) trips the undefined-
// behaviour sanitizer.  First the brushes and maps of the test suite
// (tests/paint_spec.py BRUSHES, tests/clone_spec.py MAPS) on the 37 x 22 x 45
// volume, every op and falloff; then random volumes, brushes, maps and
// placements, with offsets, centres and origins at the ends of int32.  Each
// result is compared with a naive restatement of vr.h: a full copy of the
// volume before the call, plain loops over every texel, the ellipsoid in
// unsigned __int128 and every coordinate in long long.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "check_common.hpp"

namespace {

long long clampll(long long s, int n) { return s < 0 ? 0 : s > n - 1 ? n - 1 : s; }

void restate_clone(const vr_brush& b, const vr_clone_map& m, std::vector<uint8_t>& v, int nx, int ny, int nz)
{
    const std::vector<uint8_t> before = v;
    const int n[3] = {nx, ny, nz};
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const unsigned w = weight(b, x, y, z);
                if (!w) continue;
                const int t[3] = {x, y, z};
                long long s[3];
                for (int a = 0; a < 3; ++a)
                    s[a] = clampll(m.mirror[a] ? (long long)m.offset[a] - t[a] : (long long)t[a] + m.offset[a], n[a]);
                uint8_t* p = &v[(((size_t)z * ny + y) * nx + x) * 4];
                const uint8_t* q = &before[(((size_t)s[2] * ny + (size_t)s[1]) * nx + (size_t)s[0]) * 4];
                for (int c = 0; c < 4; ++c)
                    if (b.strength[c]) p[c] = blend(b.op, p[c], q[c], (long long)w * b.strength[c]);
            }
}

// also the edited box: lo > hi on an axis when nothing was touched
void restate_stamp(const vr_brush& b, const std::vector<uint8_t>& stamp, const vr_box& pl, std::vector<uint8_t>& v, int nx,
                   int ny, int nz, int lo[3], int hi[3])
{
    for (int a = 0; a < 3; ++a) { lo[a] = INT_MAX; hi[a] = INT_MIN; }
    const long long p0[3] = {pl.x, pl.y, pl.z}, pe[3] = {pl.bx, pl.by, pl.bz};
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int t[3] = {x, y, z};
                long long i[3];
                bool covered = true;
                for (int a = 0; a < 3; ++a) {
                    i[a] = (long long)t[a] - p0[a];
                    covered = covered && i[a] >= 0 && i[a] < pe[a];
                }
                if (!covered) continue;
                // the clipped brush BOX, not the ellipsoid, bounds the edited box
                bool in_box = true;
                for (int a = 0; a < 3; ++a) {
                    const long long d = (long long)t[a] - b.centre[a];
                    in_box = in_box && d >= -(long long)b.radius[a] && d <= (long long)b.radius[a];
                }
                if (in_box)
                    for (int a = 0; a < 3; ++a) { lo[a] = t[a] < lo[a] ? t[a] : lo[a]; hi[a] = t[a] > hi[a] ? t[a] : hi[a]; }
                const unsigned w = weight(b, x, y, z);
                if (!w) continue;
                uint8_t* p = &v[(((size_t)z * ny + y) * nx + x) * 4];
                const uint8_t* q = &stamp[(((size_t)i[2] * (size_t)pe[1] + (size_t)i[1]) * (size_t)pe[0] + (size_t)i[0]) * 4];
                for (int c = 0; c < 4; ++c)
                    if (b.strength[c]) p[c] = blend(b.op, p[c], q[c], (long long)w * b.strength[c]);
            }
}

std::mt19937_64 rng(20240903);
int pick(int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); }

long cloned = 0, stamped = 0, refused = 0, changed = 0, empty_boxes = 0;

void check_clone(const vr_brush& b, const vr_clone_map& m, const std::vector<uint8_t>& base, int nx, int ny, int nz, int it)
{
    std::vector<uint8_t> vol = base, want = base;
    restate_clone(b, m, want, nx, ny, nz);
    expect(vr_brush_clone_apply(&b, &m, vol.data(), nx, ny, nz) == VR_OK, "vr_brush_clone_apply refused a valid call", it);
    expect(vol == want, "vr_brush_clone_apply differs from the restatement", it);
    const bool identity = !m.offset[0] && !m.offset[1] && !m.offset[2] && !m.mirror[0] && !m.mirror[1] && !m.mirror[2];
    if (identity && b.op == VR_BRUSH_SET) expect(vol == base, "the identity SET clone changed a byte", it);
    ++cloned;
    changed += vol != base;
}

void check_stamp(const vr_brush& b, const vr_box& pl, const std::vector<uint8_t>& base, int nx, int ny, int nz, int it)
{
    const std::vector<uint8_t> stamp = random_bytes(rng, (size_t)pl.bx * pl.by * pl.bz * 4);
    std::vector<uint8_t> vol = base, want = base;
    int lo[3], hi[3], o[3], e[3];
    restate_stamp(b, stamp, pl, want, nx, ny, nz, lo, hi);
    expect(vr_brush_stamp_apply(&b, stamp.data(), &pl, vol.data(), nx, ny, nz) == VR_OK, "vr_brush_stamp_apply refused a valid call", it);
    expect(vol == want, "vr_brush_stamp_apply differs from the restatement", it);
    expect(vr_stamp_box(&b, &pl, nx, ny, nz, o, e) == VR_OK, "vr_stamp_box refused a valid call", it);
    if (lo[0] > hi[0]) {
        expect(e[0] == 0 && e[1] == 0 && e[2] == 0 && o[0] == 0 && o[1] == 0 && o[2] == 0, "vr_stamp_box of nothing is not empty", it);
        expect(vol == base, "a stamp that edits nothing changed a byte", it);
        ++empty_boxes;
    } else {
        for (int a = 0; a < 3; ++a) expect(o[a] == lo[a] && e[a] == hi[a] - lo[a] + 1, "vr_stamp_box differs from the restatement", it);
    }
    ++stamped;
    changed += vol != base;
}

}  // namespace

int main()
{
    // ---- the suite's brushes and maps on its volume's dimensions
    {
        const int nx = 37, ny = 22, nz = 45;
        const std::vector<uint8_t> base = random_bytes(rng, (size_t)nx * ny * nz * 4);
        const int brushes[][6] = {{17, 11, 23, 3, 2, 4},   {17, 11, 23, 0, 0, 0},  {0, 0, 0, 5, 5, 5},       {36, 21, 44, 5, 3, 6},
                                  {-2, 10, 47, 4, 4, 4},   {19, 10, 31, 16, 4, 2}, {18, 11, 22, 40, 40, 40}, {18, 11, 22, 255, 255, 255},
                                  {-10, -10, -10, 4, 4, 4}};
        const int maps[][6] = {{12, 0, 0, 0, 0, 0}, {7, 0, 0, 0, 0, 0},  {6, 0, 0, 0, 0, 0},  {1, 0, 0, 0, 0, 0},     {-1, 0, 0, 0, 0, 0},
                               {0, 1, 0, 0, 0, 0},  {0, -1, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0},  {0, 0, -1, 0, 0, 0},    {34, 0, 0, 1, 0, 0},
                               {0, 0, 0, 1, 1, 1} /* offset = 2 centre, below */, {-30, 40, -60, 0, 0, 0}, {INT32_MAX, INT32_MIN, 0, 0, 0, 0},
                               {0, 0, 0, 0, 0, 0}, {INT32_MIN, INT32_MAX, INT32_MIN, 1, 1, 1}};
        int it = 0;
        for (const auto& br : brushes)
            for (const auto& mp : maps)
                for (int op = 0; op < 3; ++op)
                    for (int falloff = 0; falloff < 2; ++falloff) {
                        vr_brush b{};
                        vr_clone_map m{};
                        for (int a = 0; a < 3; ++a) {
                            b.centre[a] = br[a];
                            b.radius[a] = br[3 + a];
                            m.offset[a] = mp[0] == 0 && mp[3] && mp[4] && mp[5] ? 2 * br[a] : mp[a];
                            m.mirror[a] = mp[3 + a];
                        }
                        b.op = op;
                        b.falloff = falloff;
                        const uint8_t strength[4] = {255, 128, 1, 0};
                        for (int c = 0; c < 4; ++c) { b.value[c] = (uint8_t)(50 * c + 3); b.strength[c] = strength[c]; }
                        check_clone(b, m, base, nx, ny, nz, it++);
                    }
        // the stamp cases of the suite
        const int stamps[][9] = {{17, 11, 23, 3, 2, 4, 9, 7, 11}, {0, 0, 0, 5, 5, 5, 8, 9, 6}, {36, 21, 44, 5, 3, 6, 7, 5, 9},
                                 {19, 10, 31, 16, 4, 2, 5, 3, 2}, {17, 11, 23, 3, 2, 4, 3, 3, 3}, {18, 11, 22, 40, 40, 40, 4, 4, 4},
                                 {17, 11, 23, 3, 2, 4, 1, 1, 1}, {18, 11, 22, 255, 255, 255, 37, 22, 45}};
        const int origins[][3] = {{13, 8, 18}, {-3, -4, 1}, {33, 19, 40}, {18, 9, 30}, {25, 11, 23}, {INT32_MAX - 3, INT32_MIN, 40},
                                  {17, 11, 23}, {0, 0, 0}};
        for (int k = 0; k < 8; ++k)
            for (int op = 0; op < 3; ++op)
                for (int falloff = 0; falloff < 2; ++falloff) {
                    vr_brush b{};
                    for (int a = 0; a < 3; ++a) { b.centre[a] = stamps[k][a]; b.radius[a] = stamps[k][3 + a]; }
                    b.op = op;
                    b.falloff = falloff;
                    for (int c = 0; c < 4; ++c) b.strength[c] = (uint8_t)(c == 3 ? 0 : 255 >> c);
                    const vr_box pl{origins[k][0], origins[k][1], origins[k][2], stamps[k][6], stamps[k][7], stamps[k][8]};
                    check_stamp(b, pl, base, nx, ny, nz, it++);
                }
    }
    // ---- random volumes, brushes, maps and placements
    const int far[] = {INT32_MAX, INT32_MIN, INT32_MAX - 255, INT32_MIN + 255, 1 << 30, -(1 << 30)};
    for (int it = 10000; it < 12400; ++it) {
        const int kind = it % 6;
        int nx = pick(1, 14), ny = pick(1, 14), nz = pick(1, 14);
        if (kind == 1) nx = ny = nz = 1;
        if (kind == 2) { nx = 2; ny = 3; nz = 1; }
        const int n[3] = {nx, ny, nz};
        vr_brush b{};
        for (int a = 0; a < 3; ++a) {
            b.centre[a] = pick(-3, n[a] + 2);
            b.radius[a] = pick(0, 6);
        }
        if (kind == 3)
            for (int a = 0; a < 3; ++a) { b.radius[a] = VR_BRUSH_MAX_RADIUS; b.centre[a] = pick(-260, 270); }
        if (kind == 4)
            for (int a = 0; a < 3; ++a)
                if (a == it / 6 % 3 || pick(0, 2) == 0) { b.centre[a] = far[pick(0, 5)]; b.radius[a] = pick(0, 1) ? 255 : 0; }
        b.op = it / 6 % 3;
        b.falloff = it / 18 % 2;
        for (int c = 0; c < 4; ++c) { b.value[c] = (uint8_t)pick(0, 255); b.strength[c] = (uint8_t)(pick(0, 3) ? pick(0, 255) : pick(0, 1) * 255); }
        vr_clone_map m{};
        for (int a = 0; a < 3; ++a) {
            m.mirror[a] = pick(0, 1);
            m.offset[a] = pick(0, 4) == 0 ? far[pick(0, 5)] : m.mirror[a] ? pick(-2, 2 * n[a] + 1) : pick(-n[a] - 1, n[a] + 1);
        }
        const std::vector<uint8_t> base = random_bytes(rng, (size_t)nx * ny * nz * 4);
        check_clone(b, m, base, nx, ny, nz, it);
        vr_box pl{};
        pl.bx = pick(1, 9); pl.by = pick(1, 9); pl.bz = pick(1, 9);
        pl.x = pick(-pl.bx - 1, nx + 1); pl.y = pick(-pl.by - 1, ny + 1); pl.z = pick(-pl.bz - 1, nz + 1);
        if (kind != 4 && pick(0, 2)) {   // so that many stamps edit something
            int32_t* org[3] = {&pl.x, &pl.y, &pl.z};
            const int32_t ext[3] = {pl.bx, pl.by, pl.bz};
            for (int a = 0; a < 3; ++a) *org[a] = (int)clampll(b.centre[a], n[a]) - pick(0, ext[a] - 1);   // over the texel nearest the centre
        }
        if (kind == 5) {   // an origin at the ends of int32: x + bx does not fit 32 bits
            int32_t* org[3] = {&pl.x, &pl.y, &pl.z};
            *org[it / 6 % 3] = pick(0, 1) ? INT32_MAX - pick(0, 3) : INT32_MIN + pick(0, 3);
        }
        check_stamp(b, pl, base, nx, ny, nz, it);

        // refusals: nothing written
        std::vector<uint8_t> vol = base;
        const std::vector<uint8_t> stamp = random_bytes(rng, (size_t)pl.bx * pl.by * pl.bz * 4);
        vr_brush bad = b;
        vr_clone_map badm = m;
        vr_box badp = pl;
        switch (it % 8) {
        case 0: bad.op = 3; break;
        case 1: bad.falloff = 2; break;
        case 2: bad.radius[it % 3] = 256; break;
        case 3: bad.radius[it % 3] = -1; break;
        case 4: bad.reserved[it % 2] = 1; break;
        case 5: badm.mirror[it % 3] = it % 2 ? 2 : -1; badp.bx = 0; break;
        case 6: badm.reserved[it % 2] = 1; badp.by = -1; break;
        default: badm.mirror[it % 3] = INT32_MAX; badp.bz = INT32_MIN; break;
        }
        int o[3] = {7, 7, 7}, e[3] = {7, 7, 7};
        expect(vr_brush_clone_apply(&bad, &badm, vol.data(), nx, ny, nz) == VR_ERR_INVALID && vol == base, "a bad clone was applied", it);
        expect(vr_brush_stamp_apply(&bad, stamp.data(), &badp, vol.data(), nx, ny, nz) == VR_ERR_INVALID && vol == base, "a bad stamp was applied", it);
        expect(vr_stamp_box(&bad, &badp, nx, ny, nz, o, e) == VR_ERR_INVALID, "a bad stamp box was accepted", it);
        expect(vr_brush_clone_apply(&b, &m, vol.data(), it % 2 ? 0 : nx, ny, it % 2 ? nz : -1) == VR_ERR_INVALID &&
                   vr_brush_stamp_apply(&b, stamp.data(), &pl, vol.data(), nx, it % 2 ? 0 : -1, nz) == VR_ERR_INVALID &&
                   vr_stamp_box(&b, &pl, nx, ny, it % 2 ? INT32_MIN : 0, o, e) == VR_ERR_INVALID && vol == base,
               "bad dimensions were accepted", it);
        expect(vr_brush_clone_apply(nullptr, &m, vol.data(), nx, ny, nz) == VR_ERR_INVALID &&
                   vr_brush_clone_apply(&b, nullptr, vol.data(), nx, ny, nz) == VR_ERR_INVALID &&
                   vr_brush_clone_apply(&b, &m, nullptr, nx, ny, nz) == VR_ERR_INVALID &&
                   vr_brush_stamp_apply(&b, nullptr, &pl, vol.data(), nx, ny, nz) == VR_ERR_INVALID &&
                   vr_brush_stamp_apply(&b, stamp.data(), nullptr, vol.data(), nx, ny, nz) == VR_ERR_INVALID &&
                   vr_stamp_box(&b, &pl, nx, ny, nz, nullptr, e) == VR_ERR_INVALID && vol == base,
               "a null pointer was accepted", it);
        refused += 12;
    }
    expect(changed > 1500, "too few cases changed a byte", (int)changed);
    expect(empty_boxes > 100 && empty_boxes < stamped - 500, "the placements do not cover both an empty and a full edited box", (int)empty_boxes);
    std::printf("clone_check: %ld cloned, %ld stamped (%ld empty boxes; %ld cases changed bytes), %ld refused, ", cloned,
                stamped, empty_boxes, changed, refused);
    return finish("clone_check");
}
