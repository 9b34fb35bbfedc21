// ols_walk.hpp -- the index algebra of the CLAIMED walk of the overlap-save tile kernel (fir_ols.hip: ols_tile_kernel<..., CLAIM = true>,
// option ols_walk: 1 for the plain filter, 2 for every form, 0 never).  Standard headers only: the kernel and tests/host/ols_walk_emul.cpp
// run the same functions.  What the walk was built against and what it gained: profiles/r18/README.md (workgroups of one launch run at
// persistently different speeds, 8.1 to 11.6 us per tile; dealt equal shares, the fast ones stood idle for 17 % of the launch).
//
// The dealt walk hands workgroup b the tiles first(b), first(b) + grid, ...: every workgroup's share is fixed before the launch, and the
// launch ends with its slowest workgroup.  Here a workgroup DRAWS its next tile when it needs one:
//   * The walk indices 0 .. ntiles - 1 are cut into kRanges = 8 contiguous ranges, one per XCD (workgroup b runs on XCD b % 8), each with a
//     counter in device memory.  A workgroup draws from its own XCD's range -- one atomicAdd(counter, 1) by one lane -- so neighbouring
//     tiles are still walked by one XCD at about one time and their overlap still comes out of that XCD's L2.
//   * A value past the end of the range says that the range is empty; the workgroup goes on to the next range (own + 1, own + 2, ... mod 8)
//     and never comes back to one it found empty.  Behind the eighth empty range it exits.  Nothing ever waits on another workgroup.
//   * Every workgroup therefore draws past the end of each range AT MOST ONCE (exactly once unless it stops at kMaxSteps), which bounds
//     the counters: counter r never exceeds len(r) + grid < 2^32.
//   * A workgroup keeps the walk index of each of its steps in LDS (the poisoned-tile replay of careful.hpp goes by step), kMaxSteps of
//     them.  One that has taken kMaxSteps tiles draws no more; the tiles still get walked as long as ntiles <= grid * kMaxSteps (if
//     tiles are left, some workgroup is below its bound and keeps drawing until every range is empty), which walk_takes() asks of the
//     launch -- longer walks stay dealt.
//   * Sharded launches walk tile 0 last: walk index w stands for tile w + 1 and the last index for tile 0 (the kernel's phys()), so tile 0
//     is the LAST INDEX OF THE LAST RANGE: no other tile of that range is drawn behind it.
//
// Clean counters for every launch, without a stream operation of their own: the counters start at zero (zeroed once, when their block is
// allocated) and THE KERNEL puts them back.  Every workgroup, behind its last draw, adds one to a completion count; the workgroup that
// brings it to gridDim.x knows that no draw of this launch is still to come and stores zero into the eight counters and the count.
// The alternative -- counters that only grow, the launch told their value before it -- needs the host to know how far each launch moves
// each counter; it does (len(r) + grid, above) only as long as no workgroup stops at kMaxSteps, and a launch replayed with the arguments
// of an earlier one would read a stale base.  The kernel-side reset has neither condition.  What it does need is that two launches never
// draw from one block at one time: a block belongs to ONE STREAM (fir_ols.hip keeps one per plan and stream, made on first use under the
// handle's lock), and the launches of a stream run one behind the other.  Launches of one handle on several streams, and the slots of the
// host pipeline (clones of the handle, each with its own plans), draw from different blocks.  A launch that a fault cuts short leaves its block
// dirty -- with the context it ran in.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SK_WALK_HD __host__ __device__ __forceinline__
#else
#define SK_WALK_HD inline
#endif

namespace skdsp {
namespace olswalk {

constexpr int kRanges = 8;        // one per XCD
constexpr int kMaxSteps = 896;    // walk indices a workgroup keeps in LDS (3.5 KiB of the 4 KiB two resident workgroups leave each other)
constexpr int kCtrStride = 32;    // counters lie 128 bytes apart: draws of different XCDs do not meet in one line
constexpr int kDone = kRanges;    // the completion count behind the eight counters
constexpr int kCtrWords = (kRanges + 1) * kCtrStride;

// range r = [range_start(r), range_start(r + 1)); ntiles < 2^31
SK_WALK_HD int64_t range_start(int64_t ntiles, int r) { return ntiles * r / kRanges; }
// the k-th range a workgroup of XCD xcd draws from
SK_WALK_HD int range_of(int xcd, int k) { return (xcd + k) % kRanges; }
// may a launch of `grid` workgroups over ntiles walk indices be claimed? (see kMaxSteps above)
SK_WALK_HD bool walk_takes(int64_t ntiles, int64_t grid) { return grid > 0 && ntiles <= grid * (int64_t)kMaxSteps; }

// One workgroup's side of the walk (uniform over the workgroup)
struct Walker {
    int xcd;     // blockIdx.x % 8
    int k;       // ranges found empty so far
    int steps;   // tiles taken so far
};
SK_WALK_HD Walker walker(int block) { return Walker{block % kRanges, 0, 0}; }
// no further draw: every range is empty, or the workgroup's list of steps is full
SK_WALK_HD bool walk_over(const Walker &w) { return w.k >= kRanges || w.steps >= kMaxSteps; }
// the counter the next draw goes to (index into the block, in words)
SK_WALK_HD int draw_from(const Walker &w) { return range_of(w.xcd, w.k) * kCtrStride; }
// what a drawn value means: the walk index of the workgroup's next tile, or -1: that range is empty (w moves on to the next one)
SK_WALK_HD int64_t take(Walker &w, int64_t ntiles, unsigned drawn)
{
    const int r = range_of(w.xcd, w.k);
    const int64_t s = range_start(ntiles, r), len = range_start(ntiles, r + 1) - s;
    if ((int64_t)drawn < len) {
        ++w.steps;
        return s + (int64_t)drawn;
    }
    ++w.k;
    return -1;
}

}  // namespace olswalk
}  // namespace skdsp
