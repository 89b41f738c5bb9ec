// round_check -- stand-alone host check of quad_round_accumulate
// (volumetricrenderer_amd/csrc/vr_internal.h), the accumulation of one round of four steps
// in march_pixel_quad_steps: no libvr.so, no HIP runtime call, no device.
// `make check-round` builds it with -fsanitize=address,undefined and runs it.
//
// The march by rounds (four terms per call, base = 0, 4, ... until the function stops or
// base >= n) must leave acc and the executed steps' sum equal, bit for bit, to the plain loop
//     for (i = 0; i < n; ++i) { acc = acc + term[i]; if (EARLY && acc > acc_limit) break; }
// for n = 0..9, with and without EARLY, for random terms and for terms that make acc pass
// acc_limit exactly at every position of a round (and of the second and third round).  The
// terms past the ray's last step are poison (NaN, infinities, huge values): a lane beyond
// the end forms a term from another point, and it must not reach acc.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "vr_internal.h"

using namespace vr;

namespace {

int g_fail = 0;
long long g_cases = 0;

uint32_t bits(float v)
{
    uint32_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
float rnd()   // [0, 1)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (float)(g_rng >> 40) * (1.0f / 16777216.0f);
}

constexpr int kMax = 12;   // terms handed to a march: n <= 9, rounded up to whole rounds

// the sequential loop: acc, and *steps = the steps executed
template <bool EARLY>
float plain(const float* term, int n, float acc_limit, int* steps)
{
    float acc = 0.0f;
    int i = 0;
    for (; i < n; ++i) {
        acc = acc + term[i];
        if (EARLY && acc > acc_limit) { ++i; break; }
    }
    *steps = i;
    return acc;
}

// the march by rounds, as march_pixel_quad_steps runs it; *rounds = the rounds executed
template <bool EARLY>
float rounds(const float* term, int n, float acc_limit, int* nrounds, bool* stopped)
{
    float acc = 0.0f;
    *nrounds = 0;
    *stopped = false;
    if (n > 0)
        for (int base = 0;;) {
            bool stop = true;   // the function sets it either way
            acc = quad_round_accumulate<EARLY>(acc, term[base], term[base + 1], term[base + 2], term[base + 3], base, n,
                                               acc_limit, &stop);
            ++*nrounds;
            base += 4;
            *stopped = stop;
            if (stop || base >= n) break;
        }
    return acc;
}

template <bool EARLY>
void check(const float* term, int n, float acc_limit, const char* what)
{
    int steps, nr;
    bool stopped;
    const float want = plain<EARLY>(term, n, acc_limit, &steps);
    const float got = rounds<EARLY>(term, n, acc_limit, &nr, &stopped);
    ++g_cases;
    // the rounds executed are those of the steps executed; it stops early exactly where the loop does
    const bool ended = EARLY && steps > 0 && want > acc_limit;
    const int want_rounds = n > 0 ? (steps + 3) / 4 : 0;
    if (bits(got) != bits(want) || nr != want_rounds || stopped != ended) {
        if (g_fail < 20)
            std::printf("FAIL %s: EARLY %d n %d limit %a: acc %a (want %a), %d rounds (want %d), stop %d (want %d)\n", what,
                        (int)EARLY, n, acc_limit, got, want, nr, want_rounds, (int)stopped, (int)ended);
        ++g_fail;
    }
}

void poison(float* term, int n, int kind)
{
    const float p[4] = {NAN, INFINITY, -INFINITY, 3.0e38f};
    for (int i = n; i < kMax; ++i) term[i] = p[(kind + i) & 3];
}

}  // namespace

int main()
{
    float term[kMax];
    for (int n = 0; n <= 9; ++n) {
        for (int rep = 0; rep < 2000; ++rep) {
            // random terms of a march: non-negative, of mixed magnitude, some exactly zero
            for (int i = 0; i < n; ++i) {
                const float m = rnd();
                term[i] = m < 0.1f ? 0.0f : rnd() * (m < 0.5f ? 1.0f : m < 0.8f ? 1.0e-3f : 37.0f);
            }
            poison(term, n, rep);
            // no limit reached, a random limit, and a limit below every sum
            check<false>(term, n, 0.0f, "no early-out");
            check<true>(term, n, INFINITY, "limit never passed");
            check<true>(term, n, rnd() * 8.0f, "random limit");
            check<true>(term, n, -1.0f, "limit passed at once");
            // acc passes the limit exactly at step k (every position of every round): the limit is the
            // sum just before the one that must pass it, or that sum itself (">" is strict: acc ==
            // acc_limit goes on)
            float sum[kMax + 1];
            sum[0] = 0.0f;
            for (int i = 0; i < n; ++i) sum[i + 1] = sum[i] + term[i];
            for (int k = 0; k < n; ++k) {
                check<true>(term, n, sum[k + 1], "limit equal to the sum after step k");
                check<true>(term, n, std::nextafterf(sum[k + 1], -INFINITY), "limit one ulp below the sum after step k");
                check<true>(term, n, sum[k], "limit equal to the sum before step k");
            }
        }
        // a NaN sum never passes the limit, in either form
        for (int k = 0; k < n; ++k) {
            for (int i = 0; i < n; ++i) term[i] = 0.25f;
            term[k] = NAN;
            poison(term, n, k);
            check<true>(term, n, 0.5f, "NaN term");
            check<false>(term, n, 0.5f, "NaN term");
        }
    }
    std::printf("round_check: %lld cases, %s\n", g_cases, g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
}
