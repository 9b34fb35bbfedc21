// Ownership of device memory: the one rule is that device memory a handle owns is a DevTable or a DevBuffer, alone or inside a plan
// of a TilePlans cache.  Standard headers only: the device is reached through the four dev_* functions below (runtime.hip defines them
// with the HIP calls; tests/host/dev_mem_emul.cpp links a fake), so every path of this header runs in a host program.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <memory>
#include <utility>
#include <vector>

namespace skdsp {

// The seam.  0 on success, otherwise the library's error code with the message set (runtime.hip: hip_fail).
int dev_alloc(void **out, size_t bytes);
void dev_free(void *p);
int dev_copy_in(void *dst, const void *src, size_t bytes);   // host to device, synchronous
int dev_sync(void *stream);                                  // the hipStream_t, opaque here

// One device allocation, freed with its owner.  Non-empty only once its contents are what the owner put there: an upload whose
// copy fails leaves the table empty.
template <class T> struct DevTable {
    T *dev = nullptr;
    DevTable() = default;
    DevTable(const DevTable &) = delete;
    DevTable &operator=(const DevTable &) = delete;
    DevTable(DevTable &&o) noexcept : dev(o.dev) { o.dev = nullptr; }
    DevTable &operator=(DevTable &&o) noexcept
    {
        if (this != &o) { reset(); dev = o.dev; o.dev = nullptr; }
        return *this;
    }
    ~DevTable() { reset(); }
    void reset()
    {
        if (dev) dev_free(dev);
        dev = nullptr;
    }
    // count elements, contents undefined: for a table the owner fills on the device or by a copy of its own
    int alloc(size_t count)
    {
        reset();
        const int rc = dev_alloc((void **)&dev, count * sizeof(T));
        if (rc) dev = nullptr;
        return rc;
    }
    int upload(const T *src, size_t count)
    {
        int rc = alloc(count);
        if (!rc && (rc = dev_copy_in(dev, src, count * sizeof(T)))) reset();
        return rc;
    }
    int upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
};

// A grow-only device block.  Growing discards the contents: `fresh` tells the caller to zero or refill.
struct DevBuffer {
    void *dev = nullptr;
    size_t cap = 0;
    DevBuffer() = default;
    DevBuffer(const DevBuffer &) = delete;
    DevBuffer &operator=(const DevBuffer &) = delete;
    ~DevBuffer()
    {
        if (dev) dev_free(dev);
    }
    int reserve(size_t bytes, void *stream, bool *fresh = nullptr)
    {
        if (fresh) *fresh = false;
        if (bytes <= cap) return 0;
        if (dev) {
            const int rc = dev_sync(stream);   // what ran on the stream may still read the old block
            dev_free(dev);
            dev = nullptr; cap = 0;
            if (rc) return rc;
        }
        const int rc = dev_alloc(&dev, bytes);
        if (rc) { dev = nullptr; return rc; }
        cap = bytes;
        if (fresh) *fresh = true;
        return 0;
    }
    template <class T> T *as() const { return static_cast<T *>(dev); }
};

// What a handle keeps per key (a rate-change factor, a shape, an engine's kind): the engine's file derives its plan from this.
struct TilePlan {
    uint64_t key = 0;
    virtual ~TilePlan() {}
};
typedef std::vector<std::unique_ptr<TilePlan>> TilePlans;
// The key of up to three small non-negative integers: (L), (L, M), (L, M, R), (kind, L)
inline uint64_t plan_key(int a, int b = 0, int c = 0) { return ((uint64_t)(uint32_t)a << 40) | ((uint64_t)(uint32_t)b << 16) | (uint64_t)(uint16_t)c; }
// The plan of `key`, built by fill(P &) on first use (under the handle's lock, like every other table); a plan whose fill fails is
// released with everything it had uploaded.  The plan's address holds for the life of the cache.
template <class P, class Fill> int tile_plan(TilePlans &plans, uint64_t key, P **out, Fill fill)
{
    for (auto &q : plans)
        if (q->key == key) { *out = static_cast<P *>(q.get()); return 0; }
    std::unique_ptr<P> p(new P());
    p->key = key;
    const int rc = fill(*p);
    if (rc) return rc;
    *out = p.get();
    plans.push_back(std::move(p));
    return 0;
}

}  // namespace skdsp
