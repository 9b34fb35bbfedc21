// Host run of csrc/stage_plan.hpp: the layout arithmetic behind every host-pointer entry point, on declared piece sizes alone (no device, no HIP).
// For every combination of sizes: each offset is a multiple of 256, no two pieces share a byte, a zero-byte piece still gets an offset of its own inside
// the slot, the primary input sits kStageHeadroom into workspace 0, and each slot's total covers its last piece plus a 256-byte tail.  Declaring more
// pieces than the plan holds is reported and writes nothing past the array.  The device form hands the caller's pointers through.
#include "stage_plan.hpp"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

using namespace skdsp;

static int g_checks = 0;
#define REQUIRE(cond)                                                      \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            printf("FAILED line %d: %s\n", __LINE__, #cond);               \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static const size_t kSizes[] = {0, 1, 255, 256, 257, 65536, ((size_t)1 << 32) + 7};
static const int kNumSizes = (int)(sizeof(kSizes) / sizeof(kSizes[0]));

static void check_layout(const StagePlan &p, const size_t *bytes, int n)
{
    REQUIRE(p.npiece == n);
    for (int i = 0; i < n; ++i) {
        const StagePlan::Piece &a = p.piece[i];
        REQUIRE(a.bytes == bytes[i]);
        REQUIRE(a.off % 256 == 0);
        REQUIRE(a.off + a.bytes + 256 <= p.total1());   // inside the slot, the tail behind it
        for (int j = 0; j < i; ++j) {
            const StagePlan::Piece &b = p.piece[j];
            REQUIRE(a.off != b.off);                                           // (also for zero-byte pieces)
            REQUIRE(a.off >= b.off + b.bytes || b.off >= a.off + a.bytes);     // no shared byte
        }
    }
    if (n) REQUIRE(p.total1() >= p.piece[n - 1].off + p.piece[n - 1].bytes + 256);
}

int main()
{
    static_assert(sizeof(size_t) == 8, "the sizes above 2^32 need a 64-bit size_t");
    REQUIRE(kStageAlign == 256 && kStageHeadroom == 65536 && kStageHeadroom % kStageAlign == 0);
    REQUIRE(stage_round(0) == 0 && stage_round(1) == 256 && stage_round(255) == 256 && stage_round(256) == 256 && stage_round(257) == 512);
    REQUIRE(stage_round(((size_t)1 << 32) + 7) == ((size_t)1 << 32) + 256);

    // the primary input: kStageHeadroom into workspace 0, the slot covers it and a 256-byte tail
    char fake0[1], fake1[1];   // stand-ins for the slots' bases: only addresses are formed, nothing is dereferenced
    for (int s = 0; s < kNumSizes; ++s) {
        StagePlan p;
        p.input(nullptr, kSizes[s]);
        REQUIRE(p.total0() >= kStageHeadroom + kSizes[s] + 256 && p.total0() % 256 == 0);
        REQUIRE(p.npiece == 0 && p.total1() == 256);
        p.base0 = fake0;
        REQUIRE((uintptr_t)p.in_dev() - (uintptr_t)fake0 == kStageHeadroom);
    }

    // every triple of sizes, and every size as each of the kMaxPieces pieces among 257-byte neighbours
    for (int a = 0; a < kNumSizes; ++a)
        for (int b = 0; b < kNumSizes; ++b)
            for (int c = 0; c < kNumSizes; ++c) {
                const size_t bytes[3] = {kSizes[a], kSizes[b], kSizes[c]};
                StagePlan p;
                REQUIRE(p.add_in(&bytes, bytes[0]) == 0 && p.add_out(fake1, bytes[1]) == 1 && p.add(nullptr, nullptr, bytes[2]) == 2);
                check_layout(p, bytes, 3);
                p.base1 = fake1;
                for (int i = 0; i < 3; ++i) REQUIRE((uintptr_t)p.dev(i) - (uintptr_t)fake1 == p.piece[i].off);
            }
    for (int s = 0; s < kNumSizes; ++s)
        for (int at = 0; at < StagePlan::kMaxPieces; ++at) {
            size_t bytes[StagePlan::kMaxPieces];
            StagePlan p;
            for (int i = 0; i < StagePlan::kMaxPieces; ++i) REQUIRE(p.add_out(fake1, bytes[i] = i == at ? kSizes[s] : 257) == i);
            check_layout(p, bytes, StagePlan::kMaxPieces);
        }

    // all pieces empty: distinct offsets all the same
    {
        const size_t bytes[StagePlan::kMaxPieces] = {0, 0, 0, 0, 0, 0};
        StagePlan p;
        for (int i = 0; i < StagePlan::kMaxPieces; ++i) p.add_in(nullptr, 0);
        check_layout(p, bytes, StagePlan::kMaxPieces);
    }

    // one piece too many: reported, not stored (an index past the array would stop the run: -fsanitize=bounds), the layout as it was
    {
        REQUIRE(StagePlan::kMaxPieces >= 6);   // two inputs, three outputs and one to spare
        size_t bytes[StagePlan::kMaxPieces];
        StagePlan p;
        for (int i = 0; i < StagePlan::kMaxPieces; ++i) REQUIRE(p.add_out(fake1, bytes[i] = 100 + i) == i);
        const size_t total = p.total1();
        REQUIRE(!p.overflow);
        REQUIRE(p.add_out(fake1, 1000) == -1 && p.add_in(fake1, 1) == -1);
        REQUIRE(p.overflow && p.total1() == total);
        check_layout(p, bytes, StagePlan::kMaxPieces);
        REQUIRE(p.dev(-1) == nullptr && p.dev(StagePlan::kMaxPieces) == nullptr);
    }

    // the device form: the caller's pointers pass through, whatever the sizes say
    {
        char x[1], a[1], y[1];
        StagePlan p(false);
        p.input(x, 12345);
        const int ia = p.add_in(a, 77), iy = p.add_out(y, 0), in = p.add_out(nullptr, 8);
        REQUIRE(p.in_dev() == x && p.dev(ia) == a && p.dev(iy) == y && p.dev(in) == nullptr);
    }

    printf("%d checks\nOK\n", g_checks);
    return 0;
}
