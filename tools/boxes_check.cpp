// boxes_check -- stand-alone host check of vr_boxes_coalesce
// (volumetricrenderer_amd/csrc/vr_boxes_coalesce.cpp), built with
// -fsanitize=address,undefined and run on the CPU (`make check-boxes` builds
// and runs it).  It links the coalescer's translation unit only: no libvr.so,
// no HIP, no device, no Python.
//
// A few thousand seeded random lists -- small volumes, and coordinates and
// extents up to INT32_MAX, where a volume needs 93 bits -- with empty, repeated
// and nested boxes, below and above the VR_MAX_DABS boxes that the coalescer
// works on without allocating.  Every VR_OK result must cover the input's union
// (on the grid of all edges), lie inside the input's bounding box, hold at most
// max_out boxes, none empty and none inside another, and come out the same a
// second time; `out` is allocated at exactly min(count, max_out) so that a write
// past it trips the sanitizer; every bad argument must be refused.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "vr.h"

namespace {

struct Box {
    int64_t lo[3], hi[3];
};
Box box_of(const vr_box& r)
{
    return Box{{r.x, r.y, r.z}, {(int64_t)r.x + r.bx, (int64_t)r.y + r.by, (int64_t)r.z + r.bz}};
}
bool holds(const Box& a, const Box& b)
{
    for (int k = 0; k < 3; ++k)
        if (b.lo[k] < a.lo[k] || b.hi[k] > a.hi[k]) return false;
    return true;
}
bool same(const vr_box& a, const vr_box& b)
{
    return a.x == b.x && a.y == b.y && a.z == b.z && a.bx == b.bx && a.by == b.by && a.bz == b.bz;
}

// every cell of the grid of all edges that an input covers is covered by an output
bool covers(const std::vector<Box>& in, const std::vector<Box>& out)
{
    std::vector<int64_t> e[3];
    for (const auto* v : {&in, &out})
        for (const Box& b : *v)
            for (int k = 0; k < 3; ++k) { e[k].push_back(b.lo[k]); e[k].push_back(b.hi[k]); }
    for (int k = 0; k < 3; ++k) {
        std::sort(e[k].begin(), e[k].end());
        e[k].erase(std::unique(e[k].begin(), e[k].end()), e[k].end());
    }
    for (size_t i = 0; i + 1 < e[0].size(); ++i)
        for (size_t j = 0; j + 1 < e[1].size(); ++j)
            for (size_t l = 0; l + 1 < e[2].size(); ++l) {
                const Box cell{{e[0][i], e[1][j], e[2][l]}, {e[0][i + 1], e[1][j + 1], e[2][l + 1]}};
                bool a = false, b = false;
                for (const Box& k : in) a = a || holds(k, cell);
                if (!a) continue;
                for (const Box& k : out) b = b || holds(k, cell);
                if (!b) return false;
            }
    return true;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20240627);
    auto pick = [&](int64_t a, int64_t b) { return std::uniform_int_distribution<int64_t>(a, b)(rng); };
    long ok = 0, merged = 0, huge = 0, longlists = 0, refused = 0, failures = 0;
    for (int it = 0; it < 2000; ++it) {
        const bool longlist = it % 50 == 7, big = !longlist && it % 3 == 0;
        const int64_t dim = longlist ? pick(1, 12) : big ? INT32_MAX : pick(1, 120);   // (the cover check is cubic in the edges)
        const int count = longlist ? (int)pick(VR_MAX_DABS + 1, VR_MAX_DABS + 30) : (int)pick(0, 9);
        std::vector<vr_box> in((size_t)count);
        for (vr_box& r : in) {
            const int kind = (int)pick(0, 9);
            int64_t e[3];
            // extents: tiny, anything, or the whole volume; now and then empty
            for (int k = 0; k < 3; ++k)
                e[k] = kind < 4 ? pick(1, std::min<int64_t>(dim, 16)) : kind < 9 ? pick(0, dim) : dim;
            if (kind == 8) e[pick(0, 2)] = 0;
            r = vr_box{(int32_t)pick(0, dim - e[0]), (int32_t)pick(0, dim - e[1]), (int32_t)pick(0, dim - e[2]),
                       (int32_t)e[0], (int32_t)e[1], (int32_t)e[2]};
        }
        for (int k = 0; k < count / 6; ++k) in[(size_t)pick(0, count - 1)] = in[(size_t)pick(0, count - 1)];
        int max_out = (int)pick(1, 8) == 1 ? 1 : (int)pick(1, std::max(1, count + 2));
        const int bad = (int)pick(0, 19);   // a bad argument now and then
        if (count > 0) {
            vr_box& v = in[(size_t)pick(0, count - 1)];
            if (bad == 0) v.x = -1;
            if (bad == 1) v.bz = -5;
            if (bad == 2) { v.z = INT32_MAX; v.bz = 1; }
            if (bad == 3) { v.y = 7; v.by = INT32_MAX - 6; }
        }
        if (bad == 4) max_out = (int)pick(-3, 0);
        const size_t room = (size_t)std::min(count, std::max(max_out, 0));
        std::vector<vr_box> out(room), again(room);   // exactly the room the contract asks for
        int n = -7, n2 = -7;
        const vr_status st = vr_boxes_coalesce(in.data(), bad == 5 ? -1 - count : count, max_out, out.data(), &n);
        if ((bad <= 3 && count > 0) || bad == 4 || bad == 5) {
            if (st != VR_ERR_INVALID || n != -7) {
                std::printf("case %d: bad argument %d accepted (status %d)\n", it, bad, (int)st);
                ++failures;
            }
            ++refused;
            continue;
        }
        if (st != VR_OK || vr_boxes_coalesce(in.data(), count, max_out, again.data(), &n2) != VR_OK) {
            std::printf("case %d: status %d\n", it, (int)st);
            ++failures;
            continue;
        }
        std::vector<Box> live, res;
        for (const vr_box& r : in)
            if (r.bx > 0 && r.by > 0 && r.bz > 0) live.push_back(box_of(r));
        bool good = n == n2 && n >= 0 && n <= max_out && n <= count && (n > 0) == !live.empty();
        for (int k = 0; good && k < n; ++k) {
            good = same(out[k], again[k]) && out[k].x >= 0 && out[k].y >= 0 && out[k].z >= 0 && out[k].bx > 0 &&
                   out[k].by > 0 && out[k].bz > 0;
            res.push_back(box_of(out[k]));
        }
        if (good && !live.empty()) {
            Box bb = live[0];
            for (const Box& b : live)
                for (int k = 0; k < 3; ++k) { bb.lo[k] = std::min(bb.lo[k], b.lo[k]); bb.hi[k] = std::max(bb.hi[k], b.hi[k]); }
            for (size_t a = 0; good && a < res.size(); ++a) {
                good = holds(bb, res[a]);
                for (size_t b = 0; good && b < res.size(); ++b) good = a == b || !holds(res[b], res[a]);
            }
            if (good && max_out == 1) good = holds(res[0], bb);   // one box: the bounding box itself
            good = good && covers(live, res);
        }
        if (!good) {
            std::printf("case %d: count %d, max_out %d, %d out: a property fails\n", it, count, max_out, n);
            ++failures;
        }
        ++ok;
        merged += (size_t)max_out < live.size() && n == max_out;
        huge += big;
        longlists += longlist;
    }
    // a diagonal run of overlapping cubes, the stroke's case: 8 boxes hold far less than the bounding box
    {
        std::vector<vr_box> in;
        for (int i = 0; i < 64; ++i) in.push_back(vr_box{4 * i, 4 * i, 4 * i, 17, 17, 17});
        vr_box out[8];
        int n = 0;
        bool good = vr_boxes_coalesce(in.data(), 64, 8, out, &n) == VR_OK && n == 8;
        double vol = 0;
        std::vector<Box> live, res;
        for (const vr_box& r : in) live.push_back(box_of(r));
        for (int k = 0; good && k < n; ++k) { vol += (double)out[k].bx * out[k].by * out[k].bz; res.push_back(box_of(out[k])); }
        good = good && covers(live, res) && vol < 269.0 * 269.0 * 269.0 / 8.0;
        if (!good) { std::printf("diagonal run: %d boxes, volume %.0f\n", n, vol); ++failures; }
    }
    // null pointers one by one, and count 0 with every pointer null
    vr_box r{0, 0, 0, 1, 1, 1}, o{};
    int n = 0;
    failures += vr_boxes_coalesce(nullptr, 1, 1, &o, &n) != VR_ERR_INVALID;
    failures += vr_boxes_coalesce(&r, 1, 1, nullptr, &n) != VR_ERR_INVALID;
    failures += vr_boxes_coalesce(&r, 1, 1, &o, nullptr) != VR_ERR_INVALID;
    failures += vr_boxes_coalesce(nullptr, 0, 1, nullptr, nullptr) != VR_OK;
    failures += vr_boxes_coalesce(nullptr, 0, 0, nullptr, nullptr) != VR_ERR_INVALID;
    std::printf("boxes_check: %ld ok (%ld at the merge limit, %ld with huge coordinates, %ld longer than VR_MAX_DABS), "
                "%ld refused, %ld failures\n", ok, merged, huge, longlists, refused, failures);
    return failures ? 1 : 0;
}
