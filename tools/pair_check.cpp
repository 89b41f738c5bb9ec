// pair_check -- stand-alone host check of the paired fetch's lane maps
// (volumetricrenderer_amd/csrc/vr_internal.h: pair_load_step, pair_load_slice, pair_owner_instr,
// pair_owner_lane and the quad_perm controls made from them), the fetch of the step rounds under
// option quad_pairs: no libvr.so, no HIP runtime call, no device.
// `make check-pair` builds it with -fsanitize=address,undefined and runs it.
//
// One quad is emulated on the host over a synthetic channel plane.  Each of the four lanes owns
// one step of a round and holds that step's byte offset.  The paired fetch -- two b64
// instructions A and B, each lane loading one z-slice of another lane's step at that lane's
// offset, the loader's shift and pack, the owner's read of its two slices -- runs through the
// maps, a DPP quad_perm read written as an array index and v_alignbyte_b32 / v_perm_b32 as plain
// C++.  For every owner the two packed dwords must equal, byte for byte, the four footprint
// bytes per slice that the step rounds' own fetch (step_fetch + step_tap in vr_march_kernels.h:
// two b64 loads at the lane's own offset, four v_alignbyte_b32) gives for that lane's offset.
// Every piece an instruction names must be consumed by exactly one owner, and the pieces of a
// round must be the eight that step_fetch loads.
//
// Offsets: off & 3 in 0..3 for each lane independently; slice pairs inside one 128-byte line and
// across a line boundary; equal offsets in several lanes (lanes past the ray's end take the
// round's first point); the first and the last valid offset of the plane.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "vr_internal.h"

using namespace vr;

namespace {

int g_fail = 0;
long long g_cases = 0;

// the plane: neighbouring bytes differ, and so do bytes 4, 8, 32 and 128 apart; behind it a guard
// of zeros, what a load past the end reads through the kernels' range-checked descriptor
constexpr unsigned kPlane = 4096;
constexpr unsigned kGuard = 64;
std::vector<uint8_t> g_plane;

void fill_plane()
{
    g_plane.assign(kPlane + kGuard, 0);
    for (unsigned i = 0; i < kPlane; ++i) g_plane[i] = (uint8_t)(1u + i * 167u + (i >> 8) * 29u);
}

struct B64 {
    uint32_t d[2];
};
B64 load_b64(unsigned addr)
{
    B64 r{};
    if (addr + 8 > kPlane) {   // no load of a valid offset leaves the plane, by either fetch
        ++g_fail;
        std::printf("FAIL load of bytes %u..%u, outside the plane\n", addr, addr + 7);
        if (addr + 8 > kPlane + kGuard) return r;
    }
    std::memcpy(r.d, &g_plane[addr], 8);
    return r;
}
// v_alignbyte_b32: ({hi, lo} >> 8 * (shift & 3)), the low dword
uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t shift)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (shift & 3u)));
}
// v_perm_b32 with selectors 0..7 only: byte s of {hi, lo}
uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; ++k) r |= (uint32_t)((v >> (8 * ((sel >> (8 * k)) & 7u))) & 0xffu) << (8 * k);
    return r;
}
// vr_march_kernels.h split_pack: bytes 0, 1 = row y at x, x + 1, bytes 2, 3 = row y + 1
uint32_t split_pack(const B64& s, uint32_t shift)
{
    const uint32_t q0 = alignbyte(s.d[1], s.d[0], shift), q1 = alignbyte(s.d[1], s.d[1], shift);
    return perm(q1, q0, 0x05040100u);
}
// a DPP quad_perm read: lane fl takes v of the lane the control names for it
uint32_t quad_read(int ctrl, const uint32_t v[4], int fl) { return v[(ctrl >> (2 * fl)) & 3]; }

// the step rounds' own fetch of the lane's step (step_fetch + step_tap), as the packed slices
void own_fetch(unsigned off, uint32_t want[2])
{
    for (int z = 0; z < 2; ++z) {
        const B64 s = load_b64((off & ~3u) + (unsigned)z * kSplitZ);
        const uint32_t q0 = alignbyte(s.d[1], s.d[0], off), q1 = alignbyte(s.d[1], s.d[1], off);
        want[z] = (q0 & 0xffffu) | (q1 << 16);   // tap_blend reads bytes 0, 1 of each
    }
}

void check_quad(const unsigned off[4], const char* what)
{
    ++g_cases;
    // owner side: the aligned offset and the full one
    uint32_t al[4], full[4];
    for (int fl = 0; fl < 4; ++fl) { al[fl] = off[fl] & ~3u; full[fl] = off[fl]; }
    // loader side: instructions A and B
    B64 ld[2][4];
    uint32_t sh[4];
    std::multiset<std::pair<int, int>> named;   // (step of the round, z-slice)
    for (int fl = 0; fl < 4; ++fl) {
        const unsigned zoff = (unsigned)pair_load_slice(fl) * kSplitZ;
        for (int I = 0; I < 2; ++I) {
            ld[I][fl] = load_b64(quad_read(pair_load_ctrl(I), al, fl) + zoff);
            named.insert({pair_load_step(I, fl), pair_load_slice(fl)});
            // the control reads the lane that owns the map's step
            if (((pair_load_ctrl(I) >> (2 * fl)) & 3) != pair_load_step(I, fl)) { ++g_fail; std::printf("FAIL control of instruction %d\n", I); }
        }
        sh[fl] = (quad_read(pair_load_ctrl(0), full, fl) & 3u) | (quad_read(pair_load_ctrl(1), full, fl) << 2);
    }
    // the consuming round: pack on the loader, read on the owner
    uint32_t pk[2][4];
    for (int fl = 0; fl < 4; ++fl) {
        pk[0][fl] = split_pack(ld[0][fl], sh[fl]);
        pk[1][fl] = split_pack(ld[1][fl], sh[fl] >> 2);
    }
    std::multiset<std::pair<int, int>> used;   // (instruction, lane) an owner read
    for (int j = 0; j < 4; ++j) {
        uint32_t want[2];
        own_fetch(off[j], want);
        for (int z = 0; z < 2; ++z) {
            const uint32_t a = quad_read(pair_owner_ctrl(z), pk[0], j), b = quad_read(pair_owner_ctrl(z), pk[1], j);
            const uint32_t got = pair_owner_instr(j) ? b : a;
            const int src = (pair_owner_ctrl(z) >> (2 * j)) & 3;
            if (src != pair_owner_lane(j, z)) { ++g_fail; std::printf("FAIL control of slice %d\n", z); }
            used.insert({pair_owner_instr(j), src});
            // the piece read is the owner's own
            if (pair_load_step(pair_owner_instr(j), src) != j || pair_load_slice(src) != z) {
                ++g_fail;
                std::printf("FAIL %s: owner %d slice %d reads step %d slice %d\n", what, j, z, pair_load_step(pair_owner_instr(j), src),
                            pair_load_slice(src));
            }
            if (got != want[z]) {
                if (g_fail < 20)
                    std::printf("FAIL %s: offsets %u %u %u %u, owner %d slice %d: %08x, want %08x\n", what, off[0], off[1], off[2],
                                off[3], j, z, got, want[z]);
                ++g_fail;
            }
        }
    }
    // coverage: the eight pieces of the step rounds, each named once and each read once
    bool cover = named.size() == 8 && used.size() == 8;
    for (int j = 0; j < 4; ++j)
        for (int z = 0; z < 2; ++z) cover = cover && named.count({j, z}) == 1;
    for (int I = 0; I < 2; ++I)
        for (int fl = 0; fl < 4; ++fl) cover = cover && used.count({I, fl}) == 1;
    if (!cover) { ++g_fail; std::printf("FAIL %s: coverage\n", what); }
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
unsigned rnd(unsigned n)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)((g_rng >> 33) % n);
}

}  // namespace

int main()
{
    fill_plane();
    // the last valid offset: its second slice's 8 bytes end at the plane's end
    const unsigned last = kPlane - kSplitZ - 8 + 3;
    // aligned bases: the first position; both slices in one 128-byte line; the second slice in the next
    // line; a slice that itself straddles a line (bytes 124..131); the last position
    const unsigned bases[] = {0, 64, 88, 96, 124, 128 + 92, 1024 - 32, 2048 + 60, last & ~3u};
    const int nb = (int)(sizeof bases / sizeof bases[0]);
    // every lane's off & 3 independently, for every base of lane 0 and a few of the others
    for (int b0 = 0; b0 < nb; ++b0)
        for (int pick = 0; pick < 12; ++pick) {
            unsigned base[4] = {bases[b0], bases[rnd(nb)], bases[rnd(nb)], bases[rnd(nb)]};
            if (pick == 0) base[1] = base[2] = base[3] = base[0];   // one brick row for the whole round
            for (int low = 0; low < 256; ++low) {
                unsigned off[4];
                for (int fl = 0; fl < 4; ++fl) off[fl] = base[fl] + ((low >> (2 * fl)) & 3);
                check_quad(off, "low bits");
            }
        }
    // equal offsets in several lanes: the lanes past the ray's end (n = 1, 2, 3 of a round) take lane 0's
    for (int n = 1; n <= 3; ++n)
        for (int rep = 0; rep < 2000; ++rep) {
            unsigned off[4];
            for (int fl = 0; fl < 4; ++fl) off[fl] = rnd(last + 1);
            for (int fl = n; fl < 4; ++fl) off[fl] = off[0];
            check_quad(off, "lanes past the end");
        }
    // the first and the last valid offset in every lane pattern
    for (int m = 0; m < 16; ++m)
        for (int other = 0; other < 2; ++other) {
            unsigned off[4];
            for (int fl = 0; fl < 4; ++fl) off[fl] = (m >> fl) & 1 ? last : other ? 0 : rnd(last + 1);
            check_quad(off, "first and last offset");
        }
    // random offsets
    for (int rep = 0; rep < 20000; ++rep) {
        unsigned off[4];
        for (int fl = 0; fl < 4; ++fl) off[fl] = rnd(last + 1);
        check_quad(off, "random");
    }
    std::printf("pair_check: %lld cases, %s\n", g_cases, g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
}
