// dispatch_check -- stand-alone host check of the march launchers' compile-time
// dispatcher (volumetricrenderer_amd/csrc/vr_dispatch.h) and of the lists and
// rules the launchers feed it (vr_internal.h): no libvr.so, no HIP runtime call,
// no device.  `make check-dispatch` builds it with -fsanitize=address,undefined
// for the default and the EXPERIMENTS=1 lists and runs both.
//
// For every runtime value in and just outside each list: the callable runs
// exactly once with the matching tag, or not at all and the fallback comes back;
// nested with_bool / with_value hand their tags on in argument order (a swapped
// template argument in a launcher is the bug this guards against); the layout
// lists partition the build's layouts as the translation units expect; the _u
// rule and march_lds_bytes give the values the launchers had written out; the mode a
// multi-frame launch runs in (quad_kernel_mode) is the request cut down to what the kernel has.
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "vr_internal.h"

using namespace vr;

namespace {

int g_fail = 0;
#define CHECK(...)                                                              \
    do {                                                                        \
        if (!(__VA_ARGS__)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__);  \
            ++g_fail;                                                           \
        }                                                                       \
    } while (0)

constexpr int kMiss = -12345;

// with_value<Vs...> over [lo, hi]: one call with tag == v for a listed v, else none and the fallback
template <int... Vs>
void check_values(int lo, int hi)
{
    const int listed[] = {Vs...};
    for (int v = lo; v <= hi; ++v) {
        int calls = 0, tag = kMiss;
        const int r = with_value<Vs...>(v, [&](auto V) {
            static_assert(std::is_same_v<decltype(V), std::integral_constant<int, decltype(V)::value>>, "an int tag");
            ++calls;
            tag = V;
            return 1000 + V;
        }, kMiss);
        bool in = false;
        for (int l : listed) in = in || l == v;
        CHECK(calls == (in ? 1 : 0));
        CHECK(r == (in ? 1000 + v : kMiss));
        CHECK(tag == (in ? v : kMiss));
    }
}

template <int... Ls>
void check_layouts(value_list<Ls...> list, std::initializer_list<int> want)
{
    CHECK(sizeof...(Ls) == want.size());
    for (int l = -2; l <= kNumLayouts + 2; ++l) {
        int calls = 0, tag = kMiss;
        const hipError_t e = with_layout<value_list<Ls...>>(l, [&](auto L) {
            ++calls;
            tag = L;
            return hipSuccess;
        });
        bool in = false;
        for (int w : want) in = in || w == l;
        CHECK(list_has(list, l) == in);
        CHECK(calls == (in ? 1 : 0));
        CHECK(tag == (in ? l : kMiss));
        CHECK(e == (in ? hipSuccess : hipErrorInvalidValue));
    }
}

template <class List>
void check_wrap()
{
    for (int l = -2; l <= kNumLayouts + 2; ++l)
        for (int wrap = -1; wrap <= 2; ++wrap) {
            int calls = 0, tl = kMiss, tw = kMiss;
            const hipError_t e = with_layout_wrap<List>(l, wrap, [&](auto L, auto W) {
                ++calls;
                tl = L;
                tw = W;
                return hipSuccess;
            });
            const bool in = list_has(List{}, l);
            CHECK(calls == (in ? 1 : 0) && e == (in ? hipSuccess : hipErrorInvalidValue));
            if (in) CHECK(tl == l && tw == (l == LAYOUT_PLANAR && wrap != WRAP_CLAMP ? WRAP_MIRROR : WRAP_CLAMP));
        }
}

template <int L>
void check_lds()
{
    MarchArgs a{};
    a.nx = 16; a.ny = 33; a.nz = 7;
    const size_t written_out = L == LAYOUT_PLANAR || L == LAYOUT_CORNERH ? 0
                             : (size_t)(a.nx + a.ny + a.nz + 3) * sizeof(unsigned) * (L == LAYOUT_COL48Z ? 2 : 1);
    CHECK(march_lds_bytes<L>(a) == written_out);
    // the multi-frame launcher's copy had no COL48Z factor: the same for its layouts
    if (pair_layout(L)) CHECK(march_lds_bytes<L>(a) == (L == LAYOUT_CORNERH ? 0 : (size_t)(a.nx + a.ny + a.nz + 3) * sizeof(unsigned)));
}
template <int... Ls>
void check_lds_all(std::integer_sequence<int, Ls...>)
{
    (check_lds<Ls + 1>(), ...);
}

// quad_kernel_mode over every multi-frame launch, and quad_waves_floor over every instance
template <int... Ls>
void check_quad_modes(value_list<Ls...>)
{
    for (int l : {Ls...})
        for (int nf : {2, kGroupFrames})
            for (int early = 0; early < 2; ++early)
                for (int zo = 0; zo < 2; ++zo)
                    for (int um = 0; um <= 15; ++um)
                        for (int req = QUAD_NONE; req <= QUAD_PAIRS; ++req) {
                            const int m = quad_kernel_mode(l, nf, early != 0, zo != 0, um, req);
                            CHECK(m >= QUAD_NONE && m <= req);
                            if (nf == 2 || !quad_instance(l, early != 0, zo != 0, um)) CHECK(m == QUAD_NONE);
                            else if (!quad_split_layout(l)) CHECK(m == (req < QUAD_FRAMES ? req : QUAD_FRAMES));
                            else CHECK(m == req);
                            // the launcher's general kernel is instantiated for umask 0: the same mode
                            if (u_kernel_channel(early != 0, zo != 0, um) < 0)
                                CHECK(m == quad_kernel_mode(l, nf, early != 0, zo != 0, 0, req));
                            const int w = quad_waves_floor(m, zo != 0, early != 0);
                            CHECK(w == 1 || w == 5);
                            if (w == 5) CHECK(quad_splits(m));
                        }
    // the predicates are the chain: each mode is the one before it and one thing more
    for (int m = QUAD_NONE; m <= QUAD_PAIRS; ++m) {
        CHECK(quad_is_quad(m) == (m != QUAD_NONE));
        CHECK(quad_splits(m) == (m == QUAD_SPLIT || m == QUAD_STEPS || m == QUAD_PAIRS));
        CHECK(quad_rounds(m) == (m == QUAD_STEPS || m == QUAD_PAIRS));
        CHECK(quad_paired(m) == (m == QUAD_PAIRS));
    }
    // the options' ladder: an option counts only where the one before it is on
    for (int b = 0; b < 32; ++b) {
        const bool el = b & 1, fq = b & 2, sp = b & 4, st = b & 8, pr = b & 16;
        const int want = !(el && fq) ? QUAD_NONE : !sp ? QUAD_FRAMES : !st ? QUAD_SPLIT : !pr ? QUAD_STEPS : QUAD_PAIRS;
        CHECK(quad_requested(el, fq, sp, st, pr) == want);
    }
}

}  // namespace

int main()
{
    // with_bool: one call, the matching tag, the callable's value
    for (int b = 0; b < 2; ++b) {
        int calls = 0;
        const int r = with_bool(b != 0, [&](auto B) {
            static_assert(std::is_same_v<decltype(B), std::true_type> || std::is_same_v<decltype(B), std::false_type>, "a bool tag");
            ++calls;
            return B ? 7 : 3;
        });
        CHECK(calls == 1 && r == (b ? 7 : 3));
        with_bool(b != 0, [&](auto B) { CHECK(bool(B) == (b != 0)); });   // a callable that returns nothing
    }

    // every value list a launcher uses, one outside each end and the gaps between
    check_values<2, 4, 8>(0, 9);                 // split K
    check_values<1, 2, 4, 8>(-1, 16);            // the _u kernels' UM (umask 10: VR_UM_EXPERIMENT's own arm)
    check_values<8, 16>(3, 17);                  // wide workgroups
    check_values<2, kGroupFrames>(0, 5);         // NF
    check_values<2, 3>(0, 4);                    // deferred shadow passes' TABLE
    check_values<0, 1, 2, 3>(-1, 4);             // march_proc_sorted's TABLE
    check_values<0, 1>(-1, 2);                   // march_proc's TABLE
    check_values<>(-1, 1);                       // an empty list never calls
    {   // a repeated value calls once
        int calls = 0;
        CHECK(with_value<3, 3>(3, [&](auto) { return ++calls; }, kMiss) == 1 && calls == 1);
    }

    // the layout lists
#if VR_EXPERIMENTS
    check_layouts(ExperimentLayouts{}, {LAYOUT_BRICK4, LAYOUT_BRICK448, LAYOUT_BRICK488, LAYOUT_BRICK4816, LAYOUT_BRICK4864,
                                        LAYOUT_BRICK41616, LAYOUT_COL48Z, LAYOUT_ZPAIR, LAYOUT_BRICK5, LAYOUT_BRICK8,
                                        LAYOUT_BRICK16});
    check_layouts(MarchLayouts{}, {LAYOUT_PLANAR, LAYOUT_COL48, LAYOUT_BRICK4832, LAYOUT_BRICK4, LAYOUT_BRICK448,
                                   LAYOUT_BRICK488, LAYOUT_BRICK4816, LAYOUT_BRICK4864, LAYOUT_BRICK41616, LAYOUT_COL48Z,
                                   LAYOUT_ZPAIR, LAYOUT_BRICK5, LAYOUT_BRICK8, LAYOUT_BRICK16});
    check_layouts(BuiltLayouts{}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16});
#else
    check_layouts(ExperimentLayouts{}, {});
    check_layouts(MarchLayouts{}, {LAYOUT_PLANAR, LAYOUT_COL48, LAYOUT_BRICK4832});
    check_layouts(BuiltLayouts{}, {LAYOUT_PLANAR, LAYOUT_COL48, LAYOUT_BRICK4832, LAYOUT_CORNER8, LAYOUT_CORNERH});
#endif
    check_layouts(CornerLayouts{}, {LAYOUT_CORNER8, LAYOUT_CORNERH});
    check_layouts(FrameLayouts{}, {LAYOUT_COL48, LAYOUT_BRICK4832, LAYOUT_CORNERH});
    for (int l = -2; l <= kNumLayouts + 2; ++l) {
        // vr_march.hip and vr_march_c8.hip split the build's layouts between them
        CHECK(list_has(BuiltLayouts{}, l) == (list_has(MarchLayouts{}, l) != list_has(CornerLayouts{}, l)));
        CHECK(!(list_has(MarchLayouts{}, l) && list_has(CornerLayouts{}, l)));
        CHECK(layout_built(l) == list_has(BuiltLayouts{}, l));
        CHECK(pair_layout(l) == (l == LAYOUT_COL48 || l == LAYOUT_BRICK4832 || l == LAYOUT_CORNERH));
        if (pair_layout(l)) CHECK(layout_built(l) && has_u_kernels(l));
        CHECK(has_u_kernels(l) == (l == LAYOUT_COL48 || l == LAYOUT_BRICK4832 || l == LAYOUT_CORNERH || l == LAYOUT_COL48Z));
    }
    check_wrap<MarchLayouts>();
    check_wrap<CornerLayouts>();
    check_wrap<BuiltLayouts>();

    // nesting hands the tags on in argument order
    for (int e = 0; e < 2; ++e)
        for (int z = 0; z < 2; ++z)
            for (int k = 0; k <= 9; ++k)
                for (int u = 0; u <= 9; ++u) {
                    int calls = 0;
                    const int r = with_bool(e != 0, [&](auto E) { return with_bool(z != 0, [&](auto Z) {
                        return with_value<2, 4, 8>(k, [&](auto K) { return with_value<1, 2, 4, 8>(u, [&](auto U) {
                            ++calls;
                            constexpr int packed = (E ? 1000 : 0) + (Z ? 100 : 0) + K * 10 + U;   // tags are constants here
                            return packed;
                        }, kMiss); }, kMiss);
                    }); });
                    const bool in = (k == 2 || k == 4 || k == 8) && (u == 1 || u == 2 || u == 4 || u == 8);
                    CHECK(calls == (in ? 1 : 0));
                    CHECK(r == (in ? e * 1000 + z * 100 + k * 10 + u : kMiss));
                }

    // the _u rule
    for (int early = 0; early < 2; ++early)
        for (int zo = 0; zo < 2; ++zo)
            for (int um = -1; um <= 17; ++um) {
                const bool one = um == 1 || um == 2 || um == 4 || um == 8;
                const int want = !early && zo && one ? (um == 1 ? 0 : um == 2 ? 1 : um == 4 ? 2 : 3) : -1;
                const int ch = u_kernel_channel(early != 0, zo != 0, um);
                CHECK(ch == want);
                if (ch >= 0) CHECK((1 << ch) == um);   // the kernels' UM is the mask
            }

    check_lds_all(std::make_integer_sequence<int, kNumLayouts - 1>{});
    check_quad_modes(FrameLayouts{});

    std::printf("dispatch_check: %s (VR_EXPERIMENTS=%d)\n", g_fail ? "FAILED" : "ok", VR_EXPERIMENTS);
    return g_fail ? 1 : 0;
}
