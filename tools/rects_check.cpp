// rects_check -- stand-alone host check of vr_rects_coalesce
// (volumetricrenderer_amd/csrc/vr_rects_coalesce.cpp), built with
// -fsanitize=address,undefined and run on the CPU (`make check-rects` builds
// and runs it).  It links the coalescer's translation unit only: no libvr.so,
// no HIP, no device, no Python.
//
// A few thousand seeded random lists -- small frames, and coordinates and
// extents up to INT32_MAX, where an area needs 62 bits -- with empty, repeated
// and nested rectangles.  Every VR_OK result must cover the input's union (on
// the grid of all edges), lie inside the input's bounding rectangle, hold at
// most max_out rectangles, none empty and none inside another, and come out the
// same a second time; `out` is allocated at exactly min(count, max_out) so that
// a write past it trips the sanitizer; every bad argument must be refused.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "vr.h"

namespace {

struct Box {
    int64_t x0, y0, x1, y1;
};
Box box_of(const vr_rect& r) { return Box{r.x, r.y, (int64_t)r.x + r.width, (int64_t)r.y + r.height}; }
bool holds(const Box& a, const Box& b) { return a.x0 <= b.x0 && a.y0 <= b.y0 && b.x1 <= a.x1 && b.y1 <= a.y1; }

// every cell of the grid of all edges that an input covers is covered by an output
bool covers(const std::vector<Box>& in, const std::vector<Box>& out)
{
    std::vector<int64_t> xs, ys;
    for (const auto* v : {&in, &out})
        for (const Box& b : *v) {
            xs.push_back(b.x0); xs.push_back(b.x1);
            ys.push_back(b.y0); ys.push_back(b.y1);
        }
    std::sort(xs.begin(), xs.end()); xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    std::sort(ys.begin(), ys.end()); ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
    for (size_t i = 0; i + 1 < xs.size(); ++i)
        for (size_t j = 0; j + 1 < ys.size(); ++j) {
            const Box cell{xs[i], ys[j], xs[i + 1], ys[j + 1]};
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
    std::mt19937_64 rng(20240620);
    auto pick = [&](int64_t a, int64_t b) { return std::uniform_int_distribution<int64_t>(a, b)(rng); };
    long ok = 0, merged = 0, huge = 0, refused = 0, failures = 0;
    for (int it = 0; it < 4000; ++it) {
        const bool big = it % 3 == 0;
        const int64_t frame = big ? INT32_MAX : pick(1, 300);
        const int count = (int)pick(0, big ? 24 : 48);
        std::vector<vr_rect> in((size_t)count);
        for (vr_rect& r : in) {
            const int kind = (int)pick(0, 9);
            // extents: tiny, anything, or the whole frame; now and then empty
            int64_t w = kind < 4 ? pick(1, std::min<int64_t>(frame, 16)) : kind < 9 ? pick(0, frame) : frame;
            int64_t h = kind < 4 ? pick(1, std::min<int64_t>(frame, 16)) : kind < 9 ? pick(0, frame) : frame;
            if (kind == 8) (pick(0, 1) ? w : h) = 0;
            r = vr_rect{(int32_t)pick(0, frame - w), (int32_t)pick(0, frame - h), (int32_t)w, (int32_t)h};
        }
        for (int k = 0; k < count / 6; ++k) in[(size_t)pick(0, count - 1)] = in[(size_t)pick(0, count - 1)];
        int max_out = (int)pick(1, 8) == 1 ? 1 : (int)pick(1, std::max(1, count + 2));
        const int bad = (int)pick(0, 15);   // a bad argument now and then
        if (count > 0) {
            vr_rect& v = in[(size_t)pick(0, count - 1)];
            if (bad == 0) v.x = -1;
            if (bad == 1) v.height = -5;
            if (bad == 2) { v.x = INT32_MAX; v.width = 1; }
            if (bad == 3) { v.y = 7; v.height = INT32_MAX - 6; }
        }
        if (bad == 4) max_out = (int)pick(-3, 0);
        const size_t room = (size_t)std::min(count, std::max(max_out, 0));
        std::vector<vr_rect> out(room), again(room);   // exactly the room the contract asks for
        int n = -7, n2 = -7;
        const vr_status st = vr_rects_coalesce(in.data(), bad == 5 ? -1 - count : count, max_out, out.data(), &n);
        if ((bad <= 3 && count > 0) || bad == 4 || bad == 5) {
            if (st != VR_ERR_INVALID || n != -7) {
                std::printf("case %d: bad argument %d accepted (status %d)\n", it, bad, (int)st);
                ++failures;
            }
            ++refused;
            continue;
        }
        if (st != VR_OK || vr_rects_coalesce(in.data(), count, max_out, again.data(), &n2) != VR_OK) {
            std::printf("case %d: status %d\n", it, (int)st);
            ++failures;
            continue;
        }
        std::vector<Box> live, res;
        for (const vr_rect& r : in)
            if (r.width > 0 && r.height > 0) live.push_back(box_of(r));
        bool good = n == n2 && n >= 0 && n <= max_out && n <= count && (n > 0) == !live.empty();
        for (int k = 0; good && k < n; ++k) {
            good = out[k].x == again[k].x && out[k].y == again[k].y && out[k].width == again[k].width &&
                   out[k].height == again[k].height && out[k].x >= 0 && out[k].y >= 0 && out[k].width > 0 &&
                   out[k].height > 0;
            res.push_back(box_of(out[k]));
        }
        if (good && !live.empty()) {
            Box bb = live[0];
            for (const Box& b : live)
                bb = Box{std::min(bb.x0, b.x0), std::min(bb.y0, b.y0), std::max(bb.x1, b.x1), std::max(bb.y1, b.y1)};
            for (size_t a = 0; good && a < res.size(); ++a) {
                good = holds(bb, res[a]);
                for (size_t b = 0; good && b < res.size(); ++b) good = a == b || !holds(res[b], res[a]);
            }
            good = good && covers(live, res);
        }
        if (!good) {
            std::printf("case %d: count %d, max_out %d, %d out: a property fails\n", it, count, max_out, n);
            ++failures;
        }
        ++ok;
        merged += (size_t)max_out < live.size() && n == max_out;
        huge += big;
    }
    // null pointers one by one, and count 0 with every pointer null
    vr_rect r{0, 0, 1, 1}, o{};
    int n = 0;
    failures += vr_rects_coalesce(nullptr, 1, 1, &o, &n) != VR_ERR_INVALID;
    failures += vr_rects_coalesce(&r, 1, 1, nullptr, &n) != VR_ERR_INVALID;
    failures += vr_rects_coalesce(&r, 1, 1, &o, nullptr) != VR_ERR_INVALID;
    failures += vr_rects_coalesce(nullptr, 0, 1, nullptr, nullptr) != VR_OK;
    failures += vr_rects_coalesce(nullptr, 0, 0, nullptr, nullptr) != VR_ERR_INVALID;
    std::printf("rects_check: %ld ok (%ld at the merge limit, %ld with huge coordinates), %ld refused, %ld failures\n", ok,
                merged, huge, refused, failures);
    return failures ? 1 : 0;
}
