// Host emulation of the claimed walk of ols_tile_kernel (csrc/ols_walk.hpp): the workgroups of a launch as state machines over the header's
// own functions, their atomic operations -- the only thing they share -- interleaved at random.
//
// What a workgroup does, in the order its thread 0 does it in the kernel: draw from the counter draw_from(w) and take() the value, until
// walk_over(w); then add one to the completion count, and put all counters back if that completed it.  (The kernel issues a draw a tile
// ahead of its use; that moves a workgroup's draws in TIME, which is what the random interleaving covers, not in their order.)
//
// Cases: ntiles in {1, 7, 8, 9, grid - 1, grid, grid + 1, 2 grid + 3, 9363} x grid in {8, 63, 504, 512}; 1000 random interleavings each, one
// launch behind the other on ONE counter block (so every launch but the first starts from what its predecessor's reset left), plus one
// schedule in which workgroup 0 runs alone until it stops (the kMaxSteps bound).  Per launch:
//   * every walk index is taken exactly once;
//   * a workgroup draws past the end of a range at most once per range, in the fixed order own, own + 1, ... (mod 8), and exits on the
//     eighth such draw (its one exit draw) or with kMaxSteps tiles -- never with tiles left that nobody will take;
//   * the last index of the last range -- tile 0 of a sharded launch -- is the last index taken from that range;
//   * no counter exceeds len + grid, and all are zero behind the launch.
// A launch that walk_takes() refuses (9363 tiles on 8 workgroups) must be one that the bound could indeed leave unfinished.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include <random>
#include <algorithm>
#include "ols_walk.hpp"

using namespace skdsp::olswalk;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Wg {
    Walker w;
    int past[kRanges];   // draws past the end, per range
    int npast;
};

// one launch; ahead >= 0: that workgroup runs alone first
static void launch(std::vector<unsigned> &ctr, int64_t ntiles, int grid, std::mt19937_64 &rng, int ahead)
{
    std::vector<Wg> wg((size_t)grid);
    std::vector<int> live((size_t)grid);
    for (int b = 0; b < grid; ++b) {
        wg[b].w = walker(b);
        std::fill(wg[b].past, wg[b].past + kRanges, 0);
        wg[b].npast = 0;
        live[b] = b;
    }
    std::vector<int> taken((size_t)ntiles, 0);
    const int64_t last_start = range_start(ntiles, kRanges - 1);
    bool tile0_seen = false;
    int resets = 0;
    while (!live.empty()) {
        size_t pick = (size_t)(rng() % live.size());
        if (ahead >= 0) {
            auto it = std::find(live.begin(), live.end(), ahead);
            if (it != live.end()) pick = (size_t)(it - live.begin()); else ahead = -1;
        }
        Wg &g = wg[live[pick]];
        if (walk_over(g.w)) {   // the completion count, and the reset by whoever completes it
            const unsigned d = ctr[kDone * kCtrStride]++;
            CHECK(d < (unsigned)grid, "completion count %u of %d", d, grid);
            if (d == (unsigned)grid - 1) {
                for (int r = 0; r <= kRanges; ++r) ctr[r * kCtrStride] = 0;
                ++resets;
                CHECK(live.size() == 1, "reset with %zu workgroups still drawing", live.size() - 1);
            }
            CHECK(g.w.k == kRanges || g.w.steps == kMaxSteps, "exit with k = %d, steps = %d", g.w.k, g.w.steps);
            CHECK(g.npast <= kRanges, "%d draws past an end", g.npast);
            live[pick] = live.back();
            live.pop_back();
            continue;
        }
        const int r = range_of(g.w.xcd, g.w.k), k_before = g.w.k;
        CHECK(draw_from(g.w) == r * kCtrStride, "draw_from");
        const unsigned drawn = ctr[r * kCtrStride]++;
        const int64_t len = range_start(ntiles, r + 1) - range_start(ntiles, r);
        CHECK((int64_t)drawn < len + grid, "counter %d at %u, len %lld, grid %d", r, drawn, (long long)len, grid);
        const int64_t idx = take(g.w, ntiles, drawn);
        if (idx >= 0) {
            CHECK(idx >= range_start(ntiles, r) && idx < range_start(ntiles, r + 1), "index %lld outside range %d", (long long)idx, r);
            CHECK(g.w.k == k_before, "a tile moved the workgroup on");
            if (idx < ntiles) ++taken[(size_t)idx];
            if (idx >= last_start) {
                CHECK(!tile0_seen, "index %lld of the last range behind its last index", (long long)idx);
                if (idx == ntiles - 1) tile0_seen = true;
            }
        } else {
            CHECK(g.w.k == k_before + 1, "an empty range must move the workgroup on by one");
            CHECK(++g.past[r] == 1, "range %d found empty twice by one workgroup", r);
            ++g.npast;
        }
    }
    CHECK(resets == 1, "%d resets", resets);
    for (int64_t i = 0; i < ntiles; ++i)
        if (taken[(size_t)i] != 1) { CHECK(false, "ntiles %lld grid %d: index %lld taken %d times", (long long)ntiles, grid, (long long)i, taken[(size_t)i]); break; }
    for (int r = 0; r <= kRanges; ++r) CHECK(ctr[r * kCtrStride] == 0, "counter %d = %u behind the launch", r, ctr[r * kCtrStride]);
}

int main()
{
    // the ranges: contiguous, in order, covering [0, ntiles)
    for (int64_t nt : {(int64_t)1, (int64_t)7, (int64_t)8, (int64_t)9, (int64_t)9363, ((int64_t)1 << 31) - 1}) {
        CHECK(range_start(nt, 0) == 0 && range_start(nt, kRanges) == nt, "ranges of %lld", (long long)nt);
        for (int r = 0; r < kRanges; ++r) CHECK(range_start(nt, r) <= range_start(nt, r + 1), "range %d of %lld", r, (long long)nt);
    }
    std::mt19937_64 rng(18);
    long launches = 0;
    for (int grid : {8, 63, 504, 512}) {
        const int64_t cases[] = {1, 7, 8, 9, grid - 1, grid, grid + 1, 2 * (int64_t)grid + 3, 9363};
        for (int64_t ntiles : cases) {
            if (!walk_takes(ntiles, grid)) {   // such a launch stays dealt; the bound must be the reason
                CHECK(ntiles > (int64_t)grid * kMaxSteps, "walk_takes refuses %lld tiles on %d workgroups", (long long)ntiles, grid);
                printf("ntiles %lld grid %d: not claimed (more than %d steps per workgroup possible)\n", (long long)ntiles, grid, kMaxSteps);
                continue;
            }
            std::vector<unsigned> ctr((size_t)kCtrWords, 0u);
            for (int rep = 0; rep < 1000; ++rep, ++launches) launch(ctr, ntiles, grid, rng, -1);
            launch(ctr, ntiles, grid, rng, 0);   // workgroup 0 runs alone until it stops
            launch(ctr, ntiles, grid, rng, grid - 1);
            launches += 2;
        }
    }
    printf("%ld launches emulated\n", launches);
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
