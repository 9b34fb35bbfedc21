// psd_core.hpp -- the in-LDS forward FFT and the |X|^2 accumulation of the Welch primitive (psd.hip):
//     S[k] = sum_i | sum_{n < ns} w[n] x[i step + n] exp(-2 pi j k n / N) |^2,   N = 2^LOG2N, 64 <= N <= 4096.
// Same code for the device (hipcc, gfx950) and the host (g++: tests/host/psd_emul.cpp).
//
// The transform is a decimation-in-frequency FFT IN PLACE: radix-4 passes over sub-blocks of M = N, N/4, N/16, ... points
// and, for an odd log2 N, one radix-2 pass at the end.  A butterfly reads and writes the same four points, so a pass needs
// no second buffer and only one barrier separates two passes.  Nothing is ever sorted back: the bin of position p is
//     p = k1 N/4 + k2 N/16 + ...   ->   f = k1 + 4 k2 + 16 k3 + ...        (bin_of)
// and |X|^2 is accumulated per POSITION in registers; the one permutation happens when a workgroup writes its partial row.
//
// Geometry for 256 threads: a butterfly per thread and pass while N <= 1024 (TS = N/4 threads per segment, NB = 256/TS
// segments side by side), R = N/1024 butterflies per thread beyond.  Butterfly u of the pass over sub-blocks of M points:
//     q = M/4, block = u / q, j = u % q, points block M + j + m q (m < 4), results times W_M^(j k) = tw[j k N/M] to point k
// (tw: exp(-2 pi j i / N), i < N, from the host in float64).
// The first pass takes its points from a loader (the staged input times the window), the last one stores nothing: it adds
// |X|^2 of its four points, formed and summed in float64, to acc[4 i + m] <-> position 4 (t + TS i) + m.
//
// LDS image: N complex points in natural order per segment.  Lanes run over j in the wide passes (consecutive 8-byte units:
// conflict-free); the passes with q < 32 (the last two or three) stride by M points and are bank-conflicted: 2 of 5 passes
// at N = 1024, and with the 16-byte points of a float64 image the conflict cycles measured exceed the LDS instruction
// cycles (the kernel is bound on chip, not by HBM; a padded or transposed image is open work).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef SK_HD
#define SK_HD __host__ __device__ __forceinline__
#endif
#ifndef SK_UNROLL
#define SK_UNROLL _Pragma("unroll")
#endif
#else
#ifndef SK_HD
#define SK_HD inline
#endif
#ifndef SK_UNROLL
#define SK_UNROLL
#endif
#endif

namespace skdsp {
namespace psd {

constexpr int kThreads = 256;
constexpr int kMinLog2 = 6, kMaxLog2 = 12;

template <typename T> struct cx { T x, y; };

template <typename T> SK_HD cx<T> cadd(cx<T> a, cx<T> b) { return cx<T>{a.x + b.x, a.y + b.y}; }
template <typename T> SK_HD cx<T> csub(cx<T> a, cx<T> b) { return cx<T>{a.x - b.x, a.y - b.y}; }

template <typename T> SK_HD cx<T> cmul(cx<T> a, cx<T> b) { return cx<T>{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <typename TO, typename TI> SK_HD cx<TO> cvt(cx<TI> a) { return cx<TO>{(TO)a.x, (TO)a.y}; }

// forward DFT4 in place: v[k] = sum_m v[m] (-j)^(m k)
template <typename T> SK_HD void dft4(cx<T> *v)
{
    const cx<T> s02 = cadd(v[0], v[2]), d02 = csub(v[0], v[2]), s13 = cadd(v[1], v[3]), d13 = csub(v[1], v[3]);
    v[0] = cadd(s02, s13);
    v[2] = csub(s02, s13);
    v[1] = cx<T>{d02.x + d13.y, d02.y - d13.x};
    v[3] = cx<T>{d02.x - d13.y, d02.y + d13.x};
}

// T: the scalar type of the LDS image; TC: the one the butterflies, the window product and the twiddles are computed in.
// The float32 image is computed in float64 (T = float, TC = double): a pass then rounds each point once, at its store,
// where float32 arithmetic rounds it four or five times, and the twiddles and the window carry no float32 rounding of their
// own -- a table entry's error is the same in every segment, so unlike the roundings of the arithmetic it does not average
// out over segments (plain float32 twiddles left every bin of a noise spectrum 5e-8 low, however many segments were summed).
template <typename T, typename TC, int LOG2N> struct Core {
    static_assert(LOG2N >= kMinLog2 && LOG2N <= kMaxLog2, "n_fft out of range");
    static constexpr int N = 1 << LOG2N;
    static constexpr int TS = N / 4 < kThreads ? N / 4 : kThreads;   // threads per segment
    static constexpr int NB = kThreads / TS;                         // segments side by side
    static constexpr int R = N / (4 * TS);                           // butterflies per thread and pass
    static constexpr int ODD = LOG2N & 1;
    static constexpr int NP4 = LOG2N / 2;                            // radix-4 passes (the last pass is one of them unless ODD)
    static constexpr int NSTORE = ODD ? NP4 : NP4 - 1;               // passes that store: first() and mid(1 .. NSTORE-1)
    static constexpr int NACC = 4 * R;

    // bin of position p
    static SK_HD int bin_of(int p)
    {
        int f = 0, w = 1, q = N;
        SK_UNROLL
        for (int s = 0; s < NP4; ++s) {
            q >>= 2;
            f += ((p / q) & 3) * w;
            w <<= 2;
        }
        if (ODD) f += (p & 1) * w;
        return f;
    }

    // one radix-4 butterfly of the pass over sub-blocks of M = N >> (2 s) points, results to img
    static SK_HD void bfly_store(int s, int u, cx<TC> *v, const cx<TC> *tw, cx<T> *img)
    {
        const int lq = LOG2N - 2 * s - 2;   // log2 q
        const int q = 1 << lq, j = u & (q - 1), base = ((u >> lq) << (lq + 2)) + j;
        dft4(v);
        const int ts = j << (2 * s);   // j N/M
        img[base] = cvt<T>(v[0]);
        img[base + q] = cvt<T>(cmul(v[1], tw[ts]));
        img[base + 2 * q] = cvt<T>(cmul(v[2], tw[2 * ts]));
        img[base + 3 * q] = cvt<T>(cmul(v[3], tw[3 * ts]));
    }

    // pass 0: thread t (0 <= t < TS) of a segment; ld(n) is the windowed sample n of the segment in TC (zero for n >= ns)
    template <class Load> static SK_HD void first(int t, Load ld, const cx<TC> *tw, cx<T> *img)
    {
        SK_UNROLL
        for (int i = 0; i < R; ++i) {
            const int u = t + TS * i;
            cx<TC> v[4];
            SK_UNROLL
            for (int m = 0; m < 4; ++m) v[m] = ld(u + m * (N / 4));
            bfly_store(0, u, v, tw, img);
        }
    }

    // pass s, 1 <= s < NSTORE
    static SK_HD void mid(int s, int t, const cx<TC> *tw, cx<T> *img)
    {
        const int lq = LOG2N - 2 * s - 2, q = 1 << lq;
        SK_UNROLL
        for (int i = 0; i < R; ++i) {
            const int u = t + TS * i;
            const int base = ((u >> lq) << (lq + 2)) + (u & (q - 1));
            cx<TC> v[4];
            SK_UNROLL
            for (int m = 0; m < 4; ++m) v[m] = cvt<TC>(img[base + m * q]);
            bfly_store(s, u, v, tw, img);
        }
    }

    // the last pass: acc[4 i + m] += |X|^2 at position 4 (t + TS i) + m, in float64
    static SK_HD void last(int t, const cx<T> *img, double *acc)
    {
        SK_UNROLL
        for (int i = 0; i < R; ++i) {
            const int base = 4 * (t + TS * i);
            cx<TC> v[4];
            SK_UNROLL
            for (int m = 0; m < 4; ++m) v[m] = cvt<TC>(img[base + m]);
            if (ODD) {
                const cx<TC> a = v[0], b = v[1], c = v[2], d = v[3];
                v[0] = cadd(a, b);
                v[1] = csub(a, b);
                v[2] = cadd(c, d);
                v[3] = csub(c, d);
            } else {
                dft4(v);
            }
            SK_UNROLL
            for (int m = 0; m < 4; ++m) {
                const double re = (double)v[m].x, im = (double)v[m].y;
                acc[4 * i + m] += re * re + im * im;
            }
        }
    }
};

}  // namespace psd
}  // namespace skdsp
