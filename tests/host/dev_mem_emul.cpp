// Host run of csrc/dev_mem.hpp: the four dev_* functions the header reaches the device through are defined HERE, as a fake that counts live
// blocks, records the order of its calls and fails the k-th one on request.  Checked: DevTable (upload, move, re-upload, destruction, a failing
// copy), DevBuffer (no call when the capacity suffices, sync before free, fresh, a failed grow and the one after it) and tile_plan (every
// failure point of a three-table plan, stable addresses, distinct packed keys).  Built with -fsanitize=address,undefined by the suite.
#include "dev_mem.hpp"
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

using namespace skdsp;

namespace {
std::set<void *> g_live;
std::string g_log;      // a: alloc, f: free, c: copy, s: sync -- in call order
int g_calls = 0;        // calls that can fail (alloc, copy, sync)
int g_fail_at = 0;      // > 0: that call fails
int g_checks = 0, g_bad = 0;

bool failing()
{
    ++g_calls;
    return g_fail_at > 0 && g_calls == g_fail_at;
}
void arm(int k)
{
    g_calls = 0;
    g_fail_at = k;
    g_log.clear();
}
#define CHECK(c)                                                    \
    do {                                                            \
        ++g_checks;                                                 \
        if (!(c)) {                                                 \
            ++g_bad;                                                \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);      \
        }                                                           \
    } while (0)
}  // namespace

namespace skdsp {
int dev_alloc(void **out, size_t bytes)
{
    g_log += 'a';
    if (failing()) return -3;
    *out = std::malloc(bytes ? bytes : 1);
    g_live.insert(*out);
    return 0;
}
void dev_free(void *p)
{
    g_log += 'f';
    if (!g_live.erase(p)) {   // a double free, or a pointer the fake never handed out
        ++g_bad;
        std::printf("FAILED: free of a block that is not live\n");
        return;
    }
    std::free(p);
}
int dev_copy_in(void *dst, const void *src, size_t bytes)
{
    g_log += 'c';
    if (failing()) return -5;
    if (!g_live.count(dst)) {
        ++g_bad;
        std::printf("FAILED: copy into a block that is not live\n");
        return -5;
    }
    std::memcpy(dst, src, bytes);
    return 0;
}
int dev_sync(void *)
{
    g_log += 's';
    return failing() ? -5 : 0;
}
}  // namespace skdsp

struct Plan3 : TilePlan {
    DevTable<float> a;
    DevTable<double> b;
    DevTable<int> c;
    int tag = 0;
};

static int fill3(Plan3 &p, int tag)
{
    const std::vector<float> a(7, 1.0f);
    const std::vector<double> b(5, 2.0);
    const std::vector<int> c(3, tag);
    int rc;
    if ((rc = p.a.upload(a)) || (rc = p.b.upload(b)) || (rc = p.c.upload(c))) return rc;
    p.tag = tag;
    return 0;
}

int main()
{
    // ---- DevTable
    arm(0);
    {
        const std::vector<int> v{1, 2, 3, 4};
        DevTable<int> t;
        CHECK(t.dev == nullptr && g_live.empty());
        CHECK(t.upload(v) == 0 && t.dev && g_live.size() == 1 && t.dev[2] == 3);
        DevTable<int> u(std::move(t));                       // move construction: one block, the source empty
        CHECK(t.dev == nullptr && u.dev && g_live.size() == 1);
        DevTable<int> w;
        CHECK(w.upload(v) == 0 && g_live.size() == 2);
        w = std::move(u);                                    // move assignment frees what the target held
        CHECK(u.dev == nullptr && w.dev && g_live.size() == 1 && w.dev[3] == 4);
        const std::vector<int> v2{9, 8};
        CHECK(w.upload(v2) == 0 && g_live.size() == 1 && w.dev[0] == 9);   // a second upload on a live table frees the first block
        DevTable<int> &self = w;
        w = std::move(self);                                 // (self-assignment keeps the block)
        CHECK(w.dev && g_live.size() == 1);
        arm(2);                                              // alloc succeeds, the copy fails: the table is empty again
        CHECK(w.upload(v) == -5 && w.dev == nullptr && g_live.empty());
        arm(1);                                              // the alloc fails
        CHECK(w.upload(v) == -3 && w.dev == nullptr && g_live.empty());
        arm(0);
        CHECK(w.upload(v) == 0 && g_live.size() == 1);       // and the next attempt succeeds
        CHECK(t.alloc(16) == 0 && t.dev && g_live.size() == 2);
    }
    CHECK(g_live.empty());                                   // destruction frees

    // ---- DevBuffer
    {
        DevBuffer b;
        int stream_tag = 0;
        bool fresh = false;
        arm(0);
        CHECK(b.reserve(0, &stream_tag, &fresh) == 0 && !fresh && b.dev == nullptr && g_log.empty());   // nothing asked, nothing done
        CHECK(b.reserve(100, &stream_tag, &fresh) == 0 && fresh && b.cap == 100 && g_live.size() == 1 && g_log == "a");   // (no old block: no sync)
        arm(0);
        CHECK(b.reserve(100, &stream_tag, &fresh) == 0 && !fresh && g_log.empty());   // the capacity suffices: no call at all
        CHECK(b.reserve(40, &stream_tag, &fresh) == 0 && !fresh && g_log.empty() && b.cap == 100);
        CHECK(b.reserve(100, &stream_tag) == 0 && g_log.empty());                     // (fresh is optional)
        CHECK(b.reserve(101, &stream_tag, &fresh) == 0 && fresh && b.cap == 101 && g_live.size() == 1 && g_live.count(b.dev) == 1);
        CHECK(g_log == "sfa");                               // growing: the sync strictly before the free, then the new block
        arm(2);                                              // sync passes, the alloc fails: empty, nothing live
        CHECK(b.reserve(500, &stream_tag, &fresh) == -3 && !fresh && b.dev == nullptr && b.cap == 0 && g_live.empty());
        arm(0);
        CHECK(b.reserve(50, &stream_tag, &fresh) == 0 && fresh && b.cap == 50 && g_live.size() == 1);   // the next reserve succeeds
        arm(1);                                              // the sync itself fails: still empty, nothing live, an error
        CHECK(b.reserve(60, &stream_tag, &fresh) == -5 && !fresh && b.dev == nullptr && b.cap == 0 && g_live.empty() && g_log == "sf");
        arm(0);
        CHECK(b.reserve(60, &stream_tag, &fresh) == 0 && fresh && b.as<char>() == b.dev && g_live.size() == 1);
    }
    CHECK(g_live.empty());

    // ---- tile_plan: a plan of three tables makes six backend calls (alloc, copy) x 3; fail each in turn
    {
        TilePlans plans;
        Plan3 *first = nullptr;
        arm(0);
        CHECK(tile_plan(plans, plan_key(3, 5, 1), &first, [&](Plan3 &p) { return fill3(p, 11); }) == 0 && first && plans.size() == 1 && g_live.size() == 3);
        const uint64_t key = plan_key(4, 5, 2);
        for (int k = 1; k <= 6; ++k) {
            Plan3 *p = nullptr;
            arm(k);
            const int rc = tile_plan(plans, key, &p, [&](Plan3 &q) { return fill3(q, 22); });
            CHECK(rc != 0 && p == nullptr && plans.size() == 1 && g_live.size() == 3);   // an error, no entry, nothing left behind
        }
        Plan3 *second = nullptr;
        arm(0);
        CHECK(tile_plan(plans, key, &second, [&](Plan3 &q) { return fill3(q, 22); }) == 0 && second && second->tag == 22 && plans.size() == 2 && g_live.size() == 6);
        for (int i = 0; i < 64; ++i) {                       // 64 further insertions under other keys
            Plan3 *p = nullptr;
            CHECK(tile_plan(plans, plan_key(100 + i, 7), &p, [&](Plan3 &q) { return fill3(q, 1000 + i); }) == 0 && p && p->tag == 1000 + i);
        }
        CHECK(plans.size() == 66 && g_live.size() == 3 * 66);
        Plan3 *again = nullptr;
        int fills = 0;
        CHECK(tile_plan(plans, key, &again, [&](Plan3 &q) { ++fills; return fill3(q, 33); }) == 0 && again == second && fills == 0 && again->c.dev[0] == 22);
        CHECK(tile_plan(plans, plan_key(3, 5, 1), &again, [&](Plan3 &q) { ++fills; return fill3(q, 33); }) == 0 && again == first && fills == 0 && again->tag == 11);
    }
    CHECK(g_live.empty());

    // ---- packed keys: (L, M, R), (L, M) and (kind, L) over the ranges the engines use, distinct within each cache
    {
        auto distinct = [](std::vector<uint64_t> &k) {
            std::sort(k.begin(), k.end());
            return std::adjacent_find(k.begin(), k.end()) == k.end();
        };
        std::vector<uint64_t> lmr, lm, kl;
        for (int L = 1; L <= 256; ++L)
            for (int M = 1; M <= 4096; ++M) {
                lm.push_back(plan_key(L, M));
                for (int R : {1, 2, 4}) lmr.push_back(plan_key(L, M, R));
            }
        for (int kind = 0; kind <= 3; ++kind)
            for (int L = 1; L <= 256; ++L) kl.push_back(plan_key(kind, L));
        CHECK(lm.size() == (size_t)256 * 4096 && distinct(lm));
        CHECK(lmr.size() == (size_t)3 * 256 * 4096 && distinct(lmr));
        CHECK(kl.size() == (size_t)4 * 256 && distinct(kl));
        CHECK(plan_key(1, 2) != plan_key(2, 1) && plan_key(0, 1) != plan_key(1, 0) && plan_key(1, 2, 4) != plan_key(1, 2));
    }

    if (g_bad) {
        std::printf("%d of %d checks FAILED\n", g_bad, g_checks);
        return 1;
    }
    std::printf("%d checks OK\n", g_checks);
    return 0;
}
