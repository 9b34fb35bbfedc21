// blockcode_core.hpp -- the plan, the run staging and the per-block functions of the block-code kernels behind fec_block.FECHamming /
// FECCyclic (fec_block.py:61-423 of the reference).  Plain C++ for host and device: blockcode.hip builds its kernels from it and
// tests/host/blockcode_emul.cpp walks the same functions thread by thread without a GPU.
//
// The code arrives as three tables of j-bit words (j = n - k parity bits, row 0 of H / register cell S[1] the most significant bit):
//     encode:  p = XOR over { i < k : x[i] = 1 } of enc[i]      code word = x[0..k) followed by bits j-1 ... 0 of p
//     decode:  s = XOR over { i < n : c[i] = 1 } of syn[i]      out[i] = c[i] ^ (s == trap[i]),  i < k
// Both are one syndrome_word() over the block's input bytes and one emit() per output byte.  Bits travel one byte (0 / 1) each.
//
// A block is n = 2^j - 1 bytes, an ODD length: no block after the first starts on a 4- or 16-byte boundary.  So a workgroup never moves
// blocks, it moves its RUN: the contiguous bytes of its blocks_per_wg blocks.  The run is staged into an LDS image whose byte t holds
// the byte at (run start rounded down to 16) + t: every 16-byte chunk that lies inside the run moves as one aligned 16-byte access, the
// (at most two) partial chunks at its ends byte by byte, and nothing outside [run start, run end) is touched (stage_in / stage_out).
// The results are assembled in a second image laid out by the OUTPUT run's alignment and leave the same way.
//
// Three forms, by n (plan_make):
//     kLane  (j <= 6,  n <= 63):     256 blocks per workgroup, one lane walks one block of the image byte by byte
//     kWave  (j <= 12, n <= 4095):   one wave per block, lanes take aligned dwords of the image; tables in LDS (syn / enc dealt into
//                                    four planes by index mod 4, so that the 64 lanes' reads of one byte position hit consecutive words)
//     kGroup (j <= 16, n <= 65535):  one workgroup per block, waves combine through LDS; tables read through L2
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef SK_HD
#define SK_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef SK_HD
#define SK_HD inline
#endif
#endif

namespace skdsp {
namespace blk {

constexpr int kMinJ = 3, kMaxJ = 16;
constexpr int kLanes = 64;
constexpr int kLaneMaxJ = 6, kWaveMaxJ = 12;
enum Form { kLane = 0, kWave = 1, kGroup = 2 };
enum Mode { kEncode = 0, kDecode = 1 };

// an LDS image that takes a run of up to `len` bytes at any alignment: up to 15 bytes of lead, rounded up to whole chunks
constexpr int image_bytes(int len) { return (len + 15 + 15) / 16 * 16; }

struct Plan {
    int n = 0, k = 0, j = 0;
    int form = 0;
    int threads = 0;         // per workgroup
    int blocks_per_wg = 0;   // blocks in a workgroup's run
    int plane = 0;           // kWave: words per plane of the dealt syn / enc table
    // LDS layout (byte offsets, multiples of 16): input image, output image, syn / enc table, trap table, one word per wave
    int off_in = 0, off_out = 0, off_tab = 0, off_trap = 0, off_red = 0, lds_bytes = 0;
};

// 0, or the complaint (a static string)
inline const char *plan_make(int n, int k, Plan *p)
{
    const int j = n - k;
    if (j < kMinJ || j > kMaxJ) return "n - k (the parity bits) must be 3 ... 16";
    if (n != (1 << j) - 1) return "n must be 2^(n - k) - 1";
    p->n = n;
    p->k = k;
    p->j = j;
    p->form = j <= kLaneMaxJ ? kLane : j <= kWaveMaxJ ? kWave : kGroup;
    int tab_words = 0, trap_words = 0;
    if (p->form == kLane) {
        p->threads = 256;
        p->blocks_per_wg = 256;
        tab_words = n;
        trap_words = k;
    } else if (p->form == kWave) {
        p->threads = 256;
        int b = 16384 / n;                       // a run of about 16 KiB, a whole number of rounds of the four waves
        b = b < 4 ? 4 : b > 128 ? 128 : b / 4 * 4;
        p->blocks_per_wg = b;
        p->plane = (n + 3) / 4 + 1;
        tab_words = 4 * p->plane;
        trap_words = k;
    } else {
        p->threads = 1024;
        p->blocks_per_wg = 1;
    }
    const int img = image_bytes(p->blocks_per_wg * n);
    p->off_in = 0;
    p->off_out = img;
    p->off_tab = 2 * img;
    p->off_trap = p->off_tab + (tab_words * 4 + 15) / 16 * 16;
    p->off_red = p->off_trap + (trap_words * 4 + 15) / 16 * 16;
    p->lds_bytes = p->off_red + (p->threads / kLanes) * 4;
    p->lds_bytes = (p->lds_bytes + 15) / 16 * 16;
    return nullptr;
}

SK_HD int bytes_in(const Plan &p, int mode) { return mode == kEncode ? p.k : p.n; }
SK_HD int bytes_out(const Plan &p, int mode) { return mode == kEncode ? p.n : p.k; }
// where word i of the syn / enc table lives: kWave deals it into planes by i mod 4 (lanes take dwords of the block, so for one byte
// position of the dword the lanes' indices are 4 apart: consecutive words of one plane); the other forms keep the natural order
SK_HD int tab_index(const Plan &p, int i) { return p.form == kWave ? (i & 3) * p.plane + (i >> 2) : i; }

// ---- a run <-> its image.  Thread t of T; g: the run's first byte in global memory, len: its bytes.  Mem does the global accesses:
// ld8 / st8 one byte, in16 / out16 one 16-byte chunk (global address a multiple of 16; the image address always is).
SK_HD int lead_of(const void *g) { return (int)((uintptr_t)g & 15); }
template <class Mem> SK_HD void stage_in(const Mem &m, const uint8_t *g, int len, uint8_t *img, int t, int T)
{
    const int lead = lead_of(g), nch = (lead + len + 15) >> 4;
    for (int c = t; c < nch; c += T) {
        const int lo = 16 * c - lead;   // the chunk's first byte as an offset into the run
        if (lo >= 0 && lo + 16 <= len) {
            m.in16(img + 16 * c, g + lo);
        } else {
            for (int b = 0; b < 16; ++b) {
                const int o = lo + b;
                img[16 * c + b] = (o >= 0 && o < len) ? m.ld8(g + o) : (uint8_t)0;
            }
        }
    }
}
template <class Mem> SK_HD void stage_out(const Mem &m, uint8_t *g, int len, const uint8_t *img, int t, int T)
{
    const int lead = lead_of(g), nch = (lead + len + 15) >> 4;
    for (int c = t; c < nch; c += T) {
        const int lo = 16 * c - lead;
        if (lo >= 0 && lo + 16 <= len) {
            m.out16(g + lo, img + 16 * c);
        } else {
            for (int b = 0; b < 16; ++b) {
                const int o = lo + b;
                if (o >= 0 && o < len) m.st8(g + o, img[16 * c + b]);
            }
        }
    }
}

SK_HD uint32_t image_dword(const uint8_t *img, int d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return reinterpret_cast<const uint32_t *>(img)[d];
#else
    uint32_t v;
    memcpy(&v, img + 4 * (size_t)d, 4);
    return v;
#endif
}

// ---- the block's word.  The block is image bytes [s, s + count); tab is the syn / enc table as tab_index() lays it out.
// Member m of M (kLane: 0 of 1, kWave: the lane of 64, kGroup: the thread of the workgroup) returns the XOR over ITS share; the XOR of all
// members' words is the block's word.  kLane walks bytes; the others walk the aligned dwords [s / 4, (s + count - 1) / 4] of the image
// (bytes of a dword outside the block are skipped: they are a neighbour's, or the zeros stage_in wrote).
SK_HD uint32_t syndrome_word(const Plan &p, const uint8_t *img, int s, int count, const uint32_t *tab, int m, int M)
{
    uint32_t w = 0;
    if (p.form == kLane) {
        for (int i = 0; i < count; ++i) w ^= img[s + i] ? tab[i] : 0u;
        return w;
    }
    const int d0 = s >> 2, d1 = (s + count - 1) >> 2;
    for (int d = d0 + m; d <= d1; d += M) {
        const uint32_t v = image_dword(img, d);
        const int i0 = 4 * d - s;   // the block index of the dword's byte 0
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + b;
            if (i >= 0 && i < count && ((v >> (8 * b)) & 0xffu)) w ^= tab[tab_index(p, i)];
        }
    }
    return w;
}

// ---- output byte i of a block whose word is w; in_byte: the block's input byte i (read only for i < k); trap_i: trap[i] (decode only)
SK_HD uint8_t emit(const Plan &p, int mode, int i, uint8_t in_byte, uint32_t w, uint32_t trap_i)
{
    if (mode == kDecode) return (uint8_t)(in_byte ^ (w == trap_i ? 1u : 0u));
    return i < p.k ? in_byte : (uint8_t)((w >> (p.n - 1 - i)) & 1u);
}

// the workgroups of a call and the blocks of workgroup g
inline int64_t grid_of(const Plan &p, int64_t nblocks) { return (nblocks + p.blocks_per_wg - 1) / p.blocks_per_wg; }
SK_HD int blocks_of(const Plan &p, int64_t nblocks, int64_t g)
{
    const int64_t left = nblocks - g * p.blocks_per_wg;
    return left < p.blocks_per_wg ? (int)left : p.blocks_per_wg;
}

// table words must fit the j bits
inline bool tables_fit(const Plan &p, const uint32_t *enc, const uint32_t *syn, const uint32_t *trap)
{
    const uint32_t top = p.j >= 32 ? 0xffffffffu : ((1u << p.j) - 1u);
    for (int i = 0; i < p.k; ++i)
        if (enc[i] > top || trap[i] > top) return false;
    for (int i = 0; i < p.n; ++i)
        if (syn[i] > top) return false;
    return true;
}

}  // namespace blk
}  // namespace skdsp
