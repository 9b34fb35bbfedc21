// stage_plan.hpp -- where the pieces of a host-pointer call live on the device.  Standard headers only: tests/host/stage_plan_emul.cpp
// checks this arithmetic without a device.  The part that touches HIP is stage_begin / stage_finish (host_pipe.hip).
//
// A host form DECLARES its pieces, calls stage_begin once, launches on the pointers the plan hands back, and calls stage_finish once:
//   input(x, bytes)        the primary input: workspace 0, kStageHeadroom bytes into the slot (kernels may be handed history in front of it)
//   add(src, dst, bytes)   a further input (src: host pointer copied in by stage_begin), an output (dst: host pointer copied back by
//                          stage_finish) or device-only room (both null): workspace 1, in the order declared
//   scratch_bytes          workspace 3, reserved as given
// The rules that make this correct, kept here and nowhere else:
//   1. every piece starts on a kStageAlign (256-byte) boundary, zero-byte pieces included, and no two pieces share a byte;
//   2. a workspace slot is reserved ONCE per call, with its summed size, before any pointer into it exists -- a workspace that grows is freed
//      and allocated anew, so a pointer taken before a second reserve of the same slot would dangle;
//   3. a call syncs its stream once, in stage_finish, with or without bytes to copy back;
//   4. argument errors return before stage_begin: nothing here is reached without a device.
// A plan made with host = false is the DEVICE form of the same call: the caller's pointers pass through dev() / in_dev(), only the scratch is
// reserved and stage_finish does nothing, so a pair of entry points shares one body.
#pragma once
#include <stddef.h>

namespace skdsp {

constexpr size_t kStageAlign = 256, kStageHeadroom = 65536;
inline size_t stage_round(size_t v) { return (v + kStageAlign - 1) / kStageAlign * kStageAlign; }

struct StagePlan {
    static constexpr int kMaxPieces = 6;   // the largest user declares two inputs and three outputs
    struct Piece {
        const void *src;
        void *dst;
        size_t bytes, off;
    };
    bool host, overflow = false;
    const void *in = nullptr;
    size_t in_bytes = 0, next = 0, scratch_bytes = 0;   // next: where the next piece of workspace 1 starts
    Piece piece[kMaxPieces];
    int npiece = 0;
    void *base0 = nullptr, *base1 = nullptr, *scratch = nullptr;   // set by stage_begin

    explicit StagePlan(bool host_form = true) : host(host_form) {}
    void input(const void *x, size_t bytes) { in = x, in_bytes = bytes; }
    int add(const void *src, void *dst, size_t bytes)   // the piece's index for dev(); -1 (and stage_begin fails) past the capacity
    {
        if (npiece == kMaxPieces) return overflow = true, -1;
        piece[npiece] = Piece{src, dst, bytes, next};
        next += stage_round(bytes ? bytes : 1);
        return npiece++;
    }
    int add_in(const void *src, size_t bytes) { return add(src, nullptr, bytes); }
    int add_out(void *dst, size_t bytes) { return add(nullptr, dst, bytes); }
    size_t total0() const { return kStageHeadroom + stage_round(in_bytes) + kStageAlign; }
    size_t total1() const { return next + kStageAlign; }
    void *in_dev() const { return host ? (char *)base0 + kStageHeadroom : const_cast<void *>(in); }
    void *dev(int i) const
    {
        if (i < 0 || i >= npiece) return nullptr;
        if (host) return (char *)base1 + piece[i].off;
        return piece[i].dst ? piece[i].dst : const_cast<void *>(piece[i].src);
    }
};

}  // namespace skdsp
