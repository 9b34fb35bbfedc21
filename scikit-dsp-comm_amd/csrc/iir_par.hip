// iir_par.hip -- single-pass exact IIR scan in PARALLEL FORM for gfx950 (MI355X): one launch, the signal read once and
// written once, every wavefront an independent segment.
// Serves scipy.signal.sosfilt(sos, x) (multirate_helper.py:173, :181, :190) / lfilter(b, a, x) (:74, :81) for decaying
// cascades of up to 8 biquads with simple poles when no state crosses the call (zi / zf callers keep the cascade kernels
// of iir_fused.hip / iir_scan.hip, whose state coordinates are scipy's).
//
// Why a second formulation.  The cascade runs 5 (4 in unit-tail form) DEPENDENT FP64 instructions per biquad and sample --
// 40 per sample for 8 biquads, one chain -- and its one-chunk transition is a dense block-triangular 16 x 16 matrix, so
// every level of the chunk scan is a 16 x 16 matrix-vector product per chunk.  The same transfer function expanded in
// partial fractions,
//     H(z) = c0 + sum_k (r0_k + r1_k z^-1) / (1 + a1_k z^-1 + a2_k z^-2),
// is 8 INDEPENDENT two-state recurrences (2 FMA each) plus a 17-term output sum that depends on the previous states only:
// 33 FP64 instructions per sample with no chain longer than two, and a block-DIAGONAL transition -- a scan level is 8
// 2 x 2 products (32 FMA) instead of 144-256.  The expansion is done on the host in long double by arithmetic modulo each
// section's denominator (no root finding, so a section may hold a complex pair, two real poles or a double pole); it is
// accepted only when the impulse response of the expansion, with its coefficients rounded to double, reproduces the cascade's to
// 1e-12 and its branches do not cancel (sum of the branch l1 norms <= 1e3 x the l1 norm of h): every design scipy makes for
// rate_change / IIR_bpf / IIR_lpf passes with a factor of 2-20, i.e. a roundoff of ~1e-14 of the output.
//
// Structure (real signals).  A WAVE owns one segment of 64 chunks x T samples (T = 128 float32 / 64 float64: 8192 / 4096
// samples) and keeps it on chip -- each lane its own chunk in registers:
//   A  the segment streams in through a wave-private [64 rows x 32 samples] LDS image (full-line 16-byte loads, next piece in
//      flight); each lane copies its row into registers and the same image feeds the FP64 matrix pipe with the B operands
//      of V = G x, the from-rest end states (w[T-1], w[T-2]) of all 8 sections of the wave's 64 chunks
//      (v_mfma_f64_16x16x4_f64, 16 state rows = one tile height exactly)
//   S  from-rest Hillis-Steele scan of the wave's 64 chunk states: per level 8 ds_read_b128 + 32 FMA per lane, matrices
//      through the scalar cache; only levels whose power of the chunk transition is not negligible
//   L  decoupled look-back: the wave publishes its from-rest end state (32 eight-byte {half, epoch} granules, relaxed
//      agent-scope atomics: the data is its own flag) and reads those of its K predecessors.  K = the number of segments the
//      filter remembers (config 4: 1); the state at the start of the segment is c = sum_j Psi^j P_(s-1-j), exact to the
//      negligibility threshold, from FROM-REST values only -- no wave waits for a chain.  Segments are handed out by a
//      ticket counter, so a predecessor is a wave that already runs; the poll is bounded and reports through a host-mapped
//      word instead of hanging
//   C  z_j = p_(j-1) + Phi^j c by binary powers
//   B  the recurrence over the register-resident samples; outputs leave through the LDS image as full lines
// Nothing in A..B meets another wave: no workgroup barrier after the table load, so the 8 waves of a CU drift through
// their memory / matrix / LDS / VALU phases independently.  N-D inputs are rows of the same launch (row = ticket / nseg).
#include "iir_common.hpp"
#include "iir_par_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

namespace skdsp {

constexpr int kParMaxK = 8;   // look-back depth served (segments the filter may remember): 8 for float64 signals, 4 for float32 ones
// (half the samples per segment and a 1e-30 instead of a 1e-18 threshold make a float64 segment "shorter" for the same filter; the look-back
// words of K segments live behind the scan exchange inside the wave's stage image, which is twice as large for float64)
constexpr int par_max_k(bool dbl) { return dbl ? 8 : 4; }
constexpr int kParTickets = 16;   // segment dispensers per launch
constexpr int SK_PAR_T32 = 128;   // samples per lane (float32 signals); float64 signals: half
constexpr int SK_PAR_PRIO = 3;      // wave priority in front of the recurrence (float32 signals, 6 - 8 biquads: DESIGN.md)
constexpr int SK_PAR_PRIO_ST = 1;   // ... and on a piece's way out through the image
constexpr int SK_PAR_OCC = 2;     // waves per SIMD the register budget is set for
constexpr int kParStageM2 = 13312;  // bytes of a wave's stage image in the DECM = 3 kernels (3072 + 3072 / 32 + 2 slots of 4 bytes, rounded up)
// (measured and not kept, round 6: three waves per SIMD for the lean decimating kernel with float32 from-rest states -- 168 VGPRs, 148 bytes of scratch per
// lane: 0.135 against 0.133 ms at two; the recurrence alone holds 96 sample + 32 state + 32 tap registers)
constexpr int SK_PAR_OCC_UPL = 4;   // ... of the lean .up kernels (UPJ, up to 4 biquads: no input image, no table in LDS)

template <int NSEC> struct ParCoef {
    double na1[NSEC], na2[NSEC];   // -a1, -a2
    double al[NSEC], be[NSEC];     // output taps on (w[n-1], w[n-2])
    double gamma;                  // direct term
};

struct ParArgs {
    const void *x;
    void *y;
    int64_t n;                   // samples per row
    int64_t x_stride, y_stride;  // elements between rows
    int nseg;                    // segments per row
    int total;                   // rows x nseg
    unsigned long long *lb;      // [total][32] look-back granules
    unsigned long long *ticket;  // [kParTickets] segment dispensers (monotonic; ticket_base = their common value before this launch)
    unsigned long long ticket_base;
    unsigned epoch;
    int n_lv;                    // scan levels inside a wave that matter (0..6)
    int K;                       // look-back depth (1..kParMaxK)
    unsigned *err;               // host-mapped: a look-back poll gave up
    int aligned;                 // rows start 16-byte aligned (vector loads / stores)
    int dec;                     // > 1: only y[k * dec] is stored (at y[k])
    int dec_dq, dec_dr;          // (rows between a lane's staged segments x T) div / mod dec
    int64_t n_keep;              // (n / dec) * dec
    // dec_compact: the kept outputs of a whole segment are gathered in the wave's (idle) stage image and leave as one contiguous run of
    // y (dec >= the samples of a 16-byte unit, and n_seg / dec of them fit the image); else the image-and-pick path below
    int dec_compact;
    // dec_rounds > 1 (float32 / complex64 with dec = 2, 3: a segment keeps more than the image holds, and a 16-byte unit up to two samples):
    // the gathering happens behind the recurrence, dec_rounds ranges of chunks one after the other, each range a run of its own
    int dec_rounds;
    unsigned dec_magic;          // ceil(2^32 / dec)
    // up > 1 (one row): x holds n_in = n / up samples and the kernel filters up * upsample(x, up) -- the zero-stuffed
    // signal exists only in the wave's staging image (multirate_IIR.up / rate_change.up: multirate_helper.py:69-75, 177-184)
    int up;
    unsigned up_magic;           // ceil(2^32 / up): (v * up_magic) >> 32 = v / up for the v < 2^15 met here
    int64_t n_in;
};

// v += P * left, P = the level's 2 x 2 block of every section (row-major), through the scalar cache
template <int NSEC>
__device__ __forceinline__ void blocks_acc(const double *__restrict__ P, const double (&in)[2 * NSEC], double (&out)[2 * NSEC])
{
#pragma unroll
    for (int k = 0; k < NSEC; ++k) {
        out[2 * k] = fma(P[4 * k + 1], in[2 * k + 1], fma(P[4 * k], in[2 * k], out[2 * k]));
        out[2 * k + 1] = fma(P[4 * k + 3], in[2 * k + 1], fma(P[4 * k + 2], in[2 * k], out[2 * k + 1]));
    }
}

typedef double v2d_t __attribute__((ext_vector_type(2)));

// DECM: 0 every output is stored; 1 .dn (the kept outputs gathered per piece, or picked out of the image); 2 .dn with dec = 2, 3 on 4-sample
// units (gathered behind the recurrence in ranges of chunks) -- an instantiation of its own: inside the others its 64 predicated LDS
// writes cost the 8-biquad kernels 450 spilled SGPRs and 2 % on every other M
// TT: samples per chunk (0: SK_PAR_T32 / its half for float64).  The decimating kernels of float32 / complex64 signals run on chunks of 96 where M divides 96
// (M = 2, 3, 4, 6, 8, 12, 16, 24, ...): every chunk of every segment then starts on a kept sample, all lanes of a wave walk the SAME phase, and the 2 NSEC + 1
// term output sum is formed for one sample in M -- with 128, M = 3 put the lanes on three phases and every sum was formed (M = 12: three in twelve).
// UPJ (.up by 8 or more, with TT = 96 and L a divisor of 96): between two input samples the filter runs on stuffed zeros, so the recurrence does not step
// through them -- every output is a 2 NSEC term product of the state right behind the last input sample with a row of c A^j (a table, wave-uniform
// because all chunks start on an input sample), and the state jumps by A^L per INPUT sample: 2 NSEC + 5 NSEC / L multiply-adds per output instead of
// 4 NSEC + 1 (order-8 Butterworth, L = 12: 9.7 instead of 17).  float64 / complex128 signals too (they never hold the chunk in registers).
// UPS (.up by 2, 3, 4 -- the factors of sigsys.interp24's stages): the stuffed zeros are compile-time facts; staged at the input rate (UP2 in the kernel).
// The rate forms are LEAN: the bookkeeping of the general kernel (zero-stuffing unit by unit, per-lane phase tests, the pick of kept samples) was two
// thirds of their instructions -- see UPL / DNL / UP2 at the top of the kernel and LABNOTES R5.8.
// V32 (float32 / complex64 signals, 7 - 8 biquads, where the plan's probe accepts it: par_v32_probe): V = G x on v_mfma_f32_16x16x4_f32 -- half the issue cycles
// of the FP64 form (32 against 64; both share the vector datapath: tools/ubench_mixed_pipes.hip), G rounded to float32 once, the samples exact, a float32
// fmaf chain over the chunk, oldest sample first.  The from-rest end states then carry ~1e-7 of error, which the output sum amplifies by the cancellation
// between the branches -- so the form is EARNED per filter: the host runs the same chain bit for bit on probe inputs and admits the filter below 5e-7.
template <int NSEC, typename IO, int DECM, bool CPLX, int TT = 0, bool UPJ = false, int UPS = 0, bool V32 = false>
__global__ __launch_bounds__(kIirThreads, (UPJ && NSEC <= 4 && sizeof(IO) == 4) ? SK_PAR_OCC_UPL : SK_PAR_OCC) void iir_par_kernel(ParArgs a, ParCoef<NSEC> cf, const double *__restrict__ gtab,
                                                                 const double *__restrict__ lvl, const double *__restrict__ psi,
                                                                 unsigned long long,   // (keeps upj out of the register tuple the three pointers above arrive in: that tuple was spilled as a whole, upj with it, and restored -- eight registers -- in front of every pair of row loads)
                                                                 const double *__restrict__ upj = nullptr)   // UPJ: [up][2 nsec] rows c A^j (up to 4 biquads: row 0 once more), then [nsec][4] the blocks of A^up
{
    constexpr bool DEC = DECM != 0;
    constexpr int D = 2 * NSEC;
    // UPL, the lean form UPJ kernels take: a chunk of 96 outputs holds 96 / up <= 12 input samples and starts on one, so the zero-stuffed chunk
    // never exists, not even in the wave's image: a lane loads ITS inputs (adjacent lanes adjacent runs: whole lines per wave), forms its from-rest end
    // state from the 96 / up columns of G those meet (wave-uniform columns: scalar loads, no table in LDS) and hands the recurrence the next input as a
    // register.  The zero-stuffing through the image (two magic divisions, a dozen selects and an LDS round trip per 16-byte unit of OUTPUT-rate
    // samples) was two thirds of the kernel's 3000 vector instructions per segment (profiles/r05/pmc_rcup12.json: SQ_INSTS_VALU) -- the FP64 work is 1000.
    constexpr bool UP2 = UPS != 0;   // (named after the first of its factors)
    constexpr int UL = UPS ? UPS : 1;
    constexpr bool UPL = UPJ;   // (every UPJ kernel is lean; what differs by the number of biquads is how the rows of c A^j are requested)
    // UP2 (.up by 2 -- the smallest factor: one sample in two carries input and the state jump would cost more than it saves): every chunk starts on an input sample and every second sample is a stuffed zero -- known when
    // the kernel is compiled.  The segment is staged at the INPUT rate (the plain filter's loads over chunks of T / 2 samples: whole lines, no division, no
    // select), V = G x runs over the even columns of G, and the recurrence reads input k / 2 at even k and a literal zero at odd k.  Building the
    // zero-stuffed image unit by unit (two magic divisions, two loads, a dozen selects per 16 bytes of OUTPUT) was 2600 of the 7200 vector instructions per
    // segment of multirate_IIR(8 biquads).up(x, 2) -- the arithmetic is 4500 (SQ_INSTS_VALU, LABNOTES R5.8).
    // The same for 3 (chunks of 96) and 4 (float32 / complex64: a float64 chunk of 64 holds 16 inputs, half a staging piece).
    static_assert(!UP2 || (DECM == 0 && !UPJ && (UPS == 3 ? TT == 96 : TT == 0) && (UPS == 2 || UPS == 3 || UPS == 4)), "UPS: the plain store; by 3 on chunks of 96");
    // DNL, the lean form of the compact decimating store (TT = 96, M a divisor of 96 from 3 on: a segment's kept outputs fit the image): every chunk of every segment starts on a kept sample,
    // so WHICH samples are kept is wave-uniform -- a scalar counter and a scalar branch instead of the per-lane phase arithmetic (a compare and an exec
    // mask per sample, the unit bookkeeping per 16 bytes, the pick out of the unit at the gathering: 2000 of the 3700 vector instructions per segment of
    // rate_change(12).dn, profiles/r05/pmc_rcdn12.json).  A kept output goes straight from the sum into its slot of the wave's idle image.
    constexpr bool DNL = (DECM == 1 || DECM == 3) && TT == 96;   // (3: M = 2, whose 3072 kept outputs per segment need a larger image -- see kWaveStage)
    constexpr bool UNI = DEC && TT == 96;   // (M = 2 on 96-sample chunks keeps its gathering in ranges but tests for kept samples the same way)
    constexpr bool G4 = D <= 12;   // V = G x by 4 x 4 x 4 products over the row groups in use (see phase A)
    static_assert(!V32 || (sizeof(IO) == 4 && !G4 && !UPJ), "V32: float32 signals, more than 6 biquads, a kernel that runs V = G x on the matrix instruction");
    constexpr int T = TT ? TT : SK_PAR_T32 * 4 / (int)sizeof(IO);
    constexpr int NP = T / kPiece;
    constexpr int TI = T / UL;   // samples per chunk at the rate the signal is READ at
    constexpr int NPI = TI / kPiece;
    static_assert(TI % kPiece == 0, "UP2: whole pieces at the input rate");
    static_assert(T % kPiece == 0 && ((T / 4) * 64) % kIirThreads == 0, "chunk length: whole pieces, a table the workgroup loads evenly");
    using St = Stage<IO>;
    constexpr int kRowBytes = St::pitch * (int)sizeof(IO);
    // 9216 (float) / 17408 (double) bytes: also holds the 8 KiB scan exchange.  DECM = 3 (the lean compact store at M = 2, float32 / complex64, more than 4
    // biquads -- kernels that run two workgroups per CU anyway): room for the 3072 kept outputs of a segment and their padding
    constexpr int kWaveStage = DECM == 3 ? kParStageM2 : 64 * kRowBytes;
    constexpr int KMAX = par_max_k(sizeof(IO) == 8);
    static_assert(kWaveStage >= 64 * 16 * 8 + KMAX * 64 * 4, "scan exchange + look-back words must fit the wave's stage image");
    __shared__ __attribute__((aligned(16))) char lds_raw[4 * kWaveStage];
    __shared__ double gl[UPL ? 64 : (T / 4) * 64];
    __shared__ int base_sh;
    float *glf = reinterpret_cast<float *>(gl);   // V32: the table as float32 (the first half of the same array)
    // CPLX: an interleaved complex signal.  Lane L owns component L & 1 (re / im) of complex chunk L >> 1: T complex samples
    // per chunk, 32 chunks per wave segment.  The two components are independent real signals through the same real
    // filter, so everything between the staging image and the recurrence is the real kernel with "the chunk to my left"
    // two lanes away; only the staging (de-interleave on the way in, re-interleave on the way out) and the look-back
    // (two end states per segment) differ.
    constexpr int LS = CPLX ? 2 : 1;            // lanes per chunk
    constexpr int CH = 64 / LS;                 // chunks per wave segment
    constexpr int GR = 32 * LS;                 // look-back granules per segment

    // (the wave index through readfirstlane: segment, row and every base address are then wave-uniform SGPR values)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Everything in front of the recurrence runs at raised priority -- where the recurrence is what the launch waits for.  The
    // recurrence of the wave that shares this SIMD is a dense v_fma_f64 stream and, being the older wave, wins every issue
    // arbitration: a younger wave's G x products (the same FP64 datapath), its scan and its correction then crawl
    // (tools/par_trace.py: 29 k clocks for 128 MFMAs that take 8 k) and are still unfinished when the older wave's recurrence ends --
    // the pipe idles until they are.  With priority the preparation is over early and the next recurrence starts the moment the
    // pipe is free.  Config 4: 0.161 -> 0.150 ms float32, 0.322 -> 0.303 ms complex64 (same box, alternating); float64 signals and
    // cascades of fewer than 6 biquads are bound by their memory walk and LOSE 2-6 % with it (the stores of the older wave then
    // wait behind the younger wave's loads), so the switch follows the FP64 work per byte.
    constexpr bool PRIO = SK_PAR_PRIO != 0 && sizeof(IO) == 4 && NSEC >= 6;
    if (PRIO) __builtin_amdgcn_s_setprio(SK_PAR_PRIO);
    // kParTickets dispensers, one per workgroup residue (a single word serialises the 2048 draws of a 2^26-sample launch in
    // the L2 atomic unit: 22 us of an otherwise empty launch): workgroup b draws q from dispenser b mod kParTickets and serves
    // wave segments 4 (kParTickets q + b mod kParTickets) ...; every dispenser hands out exactly the numbers of its residue
    // class, so the launch covers every segment once, and the smallest segment not yet drawn is drawn by the next workgroup
    // of its class that starts -- which needs only that running workgroups finish, and those wait for smaller segments only
    // (the table is requested first and the ticket behind it, so that the two round trips overlap: thread 0 used to wait for its ticket
    // before it asked for its share of the table, and the barrier for thread 0)
    constexpr int kTabPer = (T / 4) * 64 / kIirThreads;
    double tab[kTabPer];
    if constexpr (!UPL) {
#pragma unroll
        for (int i = 0; i < kTabPer; ++i) tab[i] = gtab[tid + i * kIirThreads];
    }
    // UPL: the blocks of A^up in vector registers (used once in `up` samples: not worth 32 scalar registers).  Vector loads of one address -- a lane offset
    // the compiler cannot see through: as scalar loads they were 4 NSEC round trips one after the other, each waited for before its value could move over
    double AuV[UPL ? 4 * NSEC : 1];
    if constexpr (UPL) {
        int vz = 0;
        asm volatile("" : "+v"(vz));
        const double *Ap = upj + (size_t)(a.up + (NSEC <= 4 ? 1 : 0)) * D + vz;   // (up to 4 biquads the table repeats row 0 behind row up - 1)
#pragma unroll
        for (int i = 0; i < 4 * NSEC; ++i) AuV[i] = Ap[i];
    }
    unsigned long long drawn = 0;
    if (tid == 0) drawn = atomicAdd(a.ticket + blockIdx.x % kParTickets, 1ull);
    if constexpr (!UPL) {
#pragma unroll
        for (int i = 0; i < kTabPer; ++i) {
            if constexpr (V32) glf[tid + i * kIirThreads] = (float)tab[i];
            else gl[tid + i * kIirThreads] = tab[i];
        }
    }
    if (tid == 0) base_sh = 4 * (int)((unsigned)(drawn - a.ticket_base) * kParTickets + blockIdx.x % kParTickets);
    __syncthreads();   // the only workgroup barrier
    // (UPL, measured and not kept: PERSISTENT waves that draw their own tickets and ask for the next one before they start on a segment -- 0.072 -> 0.135 ms:
    // a ticket held early is a segment whose from-rest state appears a segment's time late, and its successor, drawn by another wave a moment later,
    // waits for it in the look-back.  The draw itself is 8 % of rate_change(12).up (ticket replaced by blockIdx: 0.0755 -> 0.0695 ms), which needs the
    // dispatch order the hardware happens to follow and promises nowhere.)
    // (Round 6, measured once more for the plain filter and in the form that draws ON TIME: every wave persistent, drawing segment 16 q + class from its class's
    // dispenser when it is free for it.  Config 4 0.143 -> 0.200 ms, .dn(x, 3) 0.135 -> 0.190: the classes drift apart, and a wave whose predecessor's class is a
    // round behind polls for it instead of working -- the four waves of a workgroup that start four CONSECUTIVE segments together are what keeps the look-back short.)
    const int tk = __builtin_amdgcn_readfirstlane(base_sh) + wave;
    if (tk >= a.total) return;
    const int row = a.nseg == a.total ? 0 : __builtin_amdgcn_readfirstlane(tk / a.nseg), seg = tk - row * a.nseg;
    const IO *x = reinterpret_cast<const IO *>(a.x) + (size_t)row * a.x_stride;
    IO *y = reinterpret_cast<IO *>(a.y) + (size_t)row * a.y_stride;
    IO *stage = reinterpret_cast<IO *>(lds_raw + wave * kWaveStage);
    double *E = reinterpret_cast<double *>(lds_raw + wave * kWaveStage);   // scan exchange [section][lane][2] (aliases the image)
    const int64_t row0 = (int64_t)seg * CH;   // first chunk of the segment
    const bool interior = a.aligned && (row0 + CH) * T <= a.n;   // (a.n: samples per row -- complex samples for CPLX)

    typedef float pre_t __attribute__((ext_vector_type(4)));
    pre_t pre[NP][St::per_thread];
    // (uniform segment base + one 32-bit lane offset + constants: hipcc then addresses every access of the segment as
    // SGPR base + VGPR offset + immediate instead of keeping a 64-bit address pair per access alive)
    const IO *xseg = x + row0 * TI * LS;         // (IO scalars: an interleaved complex sample is two)
    IO *yseg = y + row0 * T * LS;
    // a 16-byte unit of a chunk's piece: St::segs units per real chunk piece, 2 x St::segs per complex one (re/im interleaved)
    constexpr int USEG = St::segs * LS;
    const unsigned loff = (unsigned)((lane / USEG) * T * LS + (lane % USEG) * St::elems);
    constexpr unsigned kRowStep = (64 / USEG) * T * LS;   // IO scalars between a lane's consecutive staged units
    const unsigned loff_in = UP2 ? (unsigned)((lane / USEG) * TI * LS + (lane % USEG) * St::elems) : loff;   // (the same on the way in, at the rate read at)
    constexpr unsigned kRowStepIn = (64 / USEG) * TI * LS;
    auto load_piece = [&](int p) {  // interior segments only
#pragma unroll
        for (int i = 0; i < St::per_thread; ++i)
            pre[p][i] = __builtin_nontemporal_load(reinterpret_cast<const pre_t *>(xseg + (loff_in + i * kRowStepIn + p * kPiece * LS)));
    };
    // image position of staged unit (i, lane): real: 16 bytes of row idx / segs; complex: the unit holds elems / 2 complex
    // samples of chunk idx / USEG -- their re parts go to row 2 chunk, their im parts to row 2 chunk + 1
    auto image_put = [&](int i, const pre_t &val) __attribute__((always_inline)) {
        const int idx = i * 64 + lane;
        if constexpr (!CPLX) {
            const int r = idx / St::segs, sg = idx % St::segs;
            *reinterpret_cast<pre_t *>(stage + r * St::pitch + sg * St::elems) = val;
        } else {
            const int ch = idx / USEG, u = idx % USEG;
            const IO *e = reinterpret_cast<const IO *>(&val);
            IO *re = stage + (2 * ch) * St::pitch + u * (St::elems / 2), *im = re + St::pitch;
#pragma unroll
            for (int k = 0; k < St::elems / 2; ++k) {
                re[k] = e[2 * k];
                im[k] = e[2 * k + 1];
            }
        }
    };
    auto image_get = [&](int i) __attribute__((always_inline)) -> pre_t {
        const int idx = i * 64 + lane;
        if constexpr (!CPLX) {
            const int r = idx / St::segs, sg = idx % St::segs;
            return *reinterpret_cast<const pre_t *>(stage + r * St::pitch + sg * St::elems);
        } else {
            const int ch = idx / USEG, u = idx % USEG;
            const IO *re = stage + (2 * ch) * St::pitch + u * (St::elems / 2), *im = re + St::pitch;
            pre_t val;
            IO *e = reinterpret_cast<IO *>(&val);
#pragma unroll
            for (int k = 0; k < St::elems / 2; ++k) {
                e[2 * k] = re[k];
                e[2 * k + 1] = im[k];
            }
            return val;
        }
    };
    auto stage_slow = [&](int p) {  // zero beyond the signal
#pragma unroll 1
        for (int i = 0; i < St::per_thread; ++i) {
            const int idx = i * 64 + lane;
            const int r = idx / USEG, sg = idx % USEG;
            // g: index of the unit's first sample (a complex sample for CPLX) in the row
            const int64_t g = (row0 + r) * TI + (int64_t)p * kPiece + (int64_t)sg * (St::elems / LS);
            const int64_t nlim = UP2 ? a.n_in : a.n;
            pre_t val;
            IO *e4 = reinterpret_cast<IO *>(&val);
#pragma unroll
            for (int e = 0; e < St::elems; ++e) e4[e] = (g + e / LS < nlim) ? x[g * LS + e] : IO(0);
            image_put(i, val);
        }
    };

    // .up: output-rate unit (i, lane) of piece p from the input-rate signal: sample m of the row is up * x[m / up] where up divides m
    const int64_t m0 = row0 * T;                                 // output-rate index of the segment's first sample (wave-uniform)
    const int64_t up_q0 = a.up > 1 ? m0 / a.up : 0;
    const unsigned up_r0 = a.up > 1 ? (unsigned)(m0 - up_q0 * a.up) : 0u;
    // A unit holds EL = elems / LS consecutive output-rate samples v .. v + EL - 1; the ones that carry input are the multiples of up: the
    // first at e0 = (up - v mod up) mod up, a second at e0 + up only where that is still inside the unit (EL = 4 with up = 2, 3).  One
    // or two loads and EL selects per unit.  (Before: every element of every unit tested on its own -- three comparisons, a product, a
    // predicated load each: .up cost a third more than the plain filter of the same number of output samples.)
    const IO *xup = x + up_q0 * LS;   // (uniform base + 32-bit lane offsets: the input samples this segment needs start here)
    const int64_t in_left = a.n_in - up_q0;
    const unsigned in_lim = in_left > 0x7fffffff ? 0x7fffffffu : (in_left > 0 ? (unsigned)in_left : 0u);
    // up_request(p): the one or two input samples of every unit of piece p, all requested before any is used (as load_piece does for the plain
    // filter; until round 4 a unit's loads were issued and waited for unit by unit -- 8 dependent round trips per piece, 32 per segment,
    // which is what held rate_change(12).up at 0.13 ms per 2^26 outputs); up_put(p): the units, zero-stuffed, into the image.
    // (they land in pre[][] -- the registers the plain filter's pieces land in: a unit of more than two samples, float32 only, can hold two
    // inputs, anything else one, so a unit's inputs are 16 bytes at most)
    static_assert((St::elems / LS > 2 ? 2 : 1) * LS * sizeof(IO) <= sizeof(pre_t), "a unit's inputs fit its landing register");
    auto up_unit = [&](int p, int i, unsigned &e0, unsigned &qa) __attribute__((always_inline)) {
        constexpr int EL = St::elems / LS;
        const int idx = i * 64 + lane;
        const int r = idx / USEG, sg = idx % USEG;
        // v: the unit's first sample (a complex sample for CPLX) counted from the last multiple of up in front of the segment
        const unsigned v = up_r0 + (unsigned)(r * T + p * kPiece + sg * EL);   // < up + 64 T
        const unsigned q = (unsigned)(((unsigned long long)v * a.up_magic) >> 32);
        const unsigned rem = v - q * (unsigned)a.up;
        e0 = rem ? (unsigned)a.up - rem : 0u;
        qa = q + (rem ? 1u : 0u);
    };
    auto up_request = [&](int p) __attribute__((always_inline)) {
        const unsigned last = in_lim ? in_lim - 1u : 0u;
#pragma unroll
        for (int i = 0; i < St::per_thread; ++i) {
            unsigned e0, qa;
            up_unit(p, i, e0, qa);
            const unsigned q0 = qa < last ? qa : last, q1 = qa + 1u < last ? qa + 1u : last;   // (clamped: the put decides what is used)
            pre_t val = {0.f, 0.f, 0.f, 0.f};
            IO *e4 = reinterpret_cast<IO *>(&val);
#pragma unroll
            for (int c = 0; c < LS; ++c) {
                e4[c] = xup[q0 * LS + c];
                if (St::elems / LS > 2) e4[LS + c] = xup[q1 * LS + c];
            }
            pre[p][i] = val;
        }
    };
    auto up_put = [&](int p) __attribute__((always_inline)) {
        constexpr int EL = St::elems / LS;
        const IO gain = (IO)a.up;
#pragma unroll
        for (int i = 0; i < St::per_thread; ++i) {
            unsigned e0, qa;
            up_unit(p, i, e0, qa);
            const unsigned e1 = e0 + (unsigned)a.up;
            const bool okA = e0 < (unsigned)EL && qa < in_lim, okB = EL > 2 && e1 < (unsigned)EL && qa + 1u < in_lim;
            const pre_t got = pre[p][i];
            const IO *in = reinterpret_cast<const IO *>(&got);
            pre_t val;
            IO *e4 = reinterpret_cast<IO *>(&val);
#pragma unroll
            for (int e = 0; e < St::elems; ++e) {
                const unsigned es = (unsigned)(e / LS);
                const IO va = gain * in[e % LS], vb = EL > 2 ? gain * in[LS + e % LS] : IO(0);
                e4[e] = (okA && es == e0) ? va : ((okB && es == e1) ? vb : IO(0));
            }
            image_put(i, val);
        }
    };
    const bool ld_fast = interior && (a.up == 1 || UP2);
    // .up by 8 or more (from 4 on the unrolled column loop costs more than the zeros: rate_change(4).up 0.130 -> 0.140 ms): at most T / 8 + 1 samples of a chunk are not stuffed zeros, so V = G x is a handful of columns of G per chunk -- formed
    // per lane on the vector ALU from the INPUT samples instead of multiplying the zeros on the matrix pipe (rate_change(12).up: 11 of 128 columns;
    // the chunks of a wave start at different phases of the stuffing, so the columns differ from lane to lane and the matrix form cannot drop them)
    const bool sparse = !DEC && !V32 && a.up >= 8;                         // (.up never comes with a decimating store: none of this in those kernels)
    const int ust = !DEC && (a.up == 2 || a.up == 4) ? a.up : 1;   // .up by 2 / 4: the column step of V = G x (see phase A)

    // ---- A: stream the segment in; chunk rows to registers; V = G x on the matrix pipe --------------------------------
    // (the chunk as 16-byte vectors: as a scalar array hipcc's SROA left half of it in scratch memory)
    typedef IO xv_t __attribute__((ext_vector_type(St::elems)));
    xv_t xq[T / St::elems];
    v4d_t acc[4];
    typedef float v4f_t __attribute__((ext_vector_type(4)));
    v4f_t accf[4];   // V32
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        acc[g] = v4d_t{0.0, 0.0, 0.0, 0.0};
        accf[g] = v4f_t{0.f, 0.f, 0.f, 0.f};
    }
    const int c = lane & 15, j = lane >> 4;
    IO *myrow = stage + lane * St::pitch;
    constexpr int NIN = UPL ? T / 8 : 1;   // UPL: input samples a chunk can hold
    IO xs[NIN];                            // ... this lane's, times the gain, rounded in the signal's type as the staging rounds them
    const int nin = UPL ? T / a.up : 0;    // ... and how many there are
    if constexpr (UPL) {
        const unsigned qa = (unsigned)((lane / LS) * nin);   // the chunk's first input sample, counted from the segment's
        const unsigned last = in_lim ? in_lim - 1u : 0u;
        const IO gain = (IO)a.up;
#pragma unroll
        for (int jj = 0; jj < NIN; ++jj) {
            IO val = IO(0);
            if (jj < nin && in_lim) {
                const unsigned qi = qa + (unsigned)jj;
                const IO got = xup[(qi < last ? qi : last) * LS + lane % LS];
                val = qi < in_lim ? gain * got : IO(0);
            }
            xs[jj] = val;
        }
    }
    xv_t xin[UP2 ? TI / St::elems : 1];   // UP2: the chunk's input samples
    if constexpr (UP2) {
        if (ld_fast) {
#pragma unroll
            for (int p = 0; p < NPI; ++p) load_piece(p);
        }
#pragma unroll
        for (int p = 0; p < NPI; ++p) {
            if (ld_fast) {
#pragma unroll
                for (int i = 0; i < St::per_thread; ++i) image_put(i, pre[p][i]);
            } else {
                stage_slow(p);
            }
            wave_lds_sync();
#pragma unroll
            for (int sgi = 0; sgi < St::segs; ++sgi) xin[p * St::segs + sgi] = *reinterpret_cast<const xv_t *>(myrow + sgi * St::elems);
            // V = G x over every UL-th column of G: input 4 s + j of the piece meets column UL (4 (8 p + s) + j) -- read with a per-lane address, as the
            // zero-stuffed image's .up by 2 / 4 below reads it
            const IO *xu = stage + c * St::pitch + j;
#pragma unroll
            for (int s = 0; s < kPiece / 4; ++s) {
                const int kcol = UL * (4 * (p * (kPiece / 4) + s) + j);
                const double *ga_p = gl + ((kcol >> 2) << 6) + ((kcol & 3) << 4);
                if constexpr (G4) {
                    constexpr int NG = (D + 3) / 4;
                    double ga[NG];
#pragma unroll
                    for (int r = 0; r < NG; ++r) ga[r] = ga_p[4 * r + (lane & 3)];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const double b = (double)xu[g * 16 * St::pitch + 4 * s];
#pragma unroll
                        for (int r = 0; r < NG; ++r) acc[g][r] = __builtin_amdgcn_mfma_f64_4x4x4f64(ga[r], b, acc[g][r], 0, 0, 0);
                    }
                } else if constexpr (V32) {
                    const float gaf = glf[((kcol >> 2) << 6) + ((kcol & 3) << 4) + (lane & 15)];
#pragma unroll
                    for (int g = 0; g < 4; ++g) accf[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(gaf, (float)xu[g * 16 * St::pitch + 4 * s], accf[g], 0, 0, 0);
                } else {
                    const double ga = ga_p[lane & 15];
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga, (double)xu[g * 16 * St::pitch + 4 * s], acc[g], 0, 0, 0);
                }
            }
            wave_lds_sync();
        }
    } else if constexpr (!UPL) {
    // (every piece of the segment is requested up front: the landing registers are the ones the chunk will occupy anyway)
    if (ld_fast) {
#pragma unroll
        for (int p = 0; p < NP; ++p) load_piece(p);
    } else if (a.up > 1) {
        if (in_lim) {
#pragma unroll
            for (int p = 0; p < NP; ++p) up_request(p);
        } else {   // (nothing of the input reaches this segment: up_put selects zeros)
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int i = 0; i < St::per_thread; ++i) pre[p][i] = pre_t{0.f, 0.f, 0.f, 0.f};
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (ld_fast) {
#pragma unroll
            for (int i = 0; i < St::per_thread; ++i) image_put(i, pre[p][i]);
        } else if (a.up > 1) {
            up_put(p);
        } else {
            stage_slow(p);
        }
        wave_lds_sync();
#pragma unroll
        for (int sgi = 0; sgi < St::segs; ++sgi) xq[p * St::segs + sgi] = *reinterpret_cast<const xv_t *>(myrow + sgi * St::elems);
        const IO *xs = stage + c * St::pitch + j;
        if (ust > 1) {
            // .up by 2 or 4: every chunk starts on a multiple of the factor, so the stuffed zeros are the same columns of G in every chunk --
            // the product runs over the other columns only (column ust (4 st + k) of the table for step st, read with a per-lane address)
            const IO *xu = stage + c * St::pitch + j * ust;
            const int nst = (kPiece / 4) / ust;
#pragma unroll
            for (int s = 0; s < kPiece / 8; ++s) {
                if (s < nst) {
                    const int kcol = ust * (4 * (p * nst + s) + j);
                    const double *ga_p = gl + ((kcol >> 2) << 6) + ((kcol & 3) << 4);
                    if constexpr (G4) {
                        constexpr int NG = (D + 3) / 4;
                        double ga[NG];
#pragma unroll
                        for (int r = 0; r < NG; ++r) ga[r] = ga_p[4 * r + (lane & 3)];
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const double b = (double)xu[g * 16 * St::pitch + 4 * ust * s];
#pragma unroll
                            for (int r = 0; r < NG; ++r) acc[g][r] = __builtin_amdgcn_mfma_f64_4x4x4f64(ga[r], b, acc[g][r], 0, 0, 0);
                        }
                    } else if constexpr (V32) {
                        const float gaf = glf[((kcol >> 2) << 6) + ((kcol & 3) << 4) + (lane & 15)];
#pragma unroll
                        for (int g = 0; g < 4; ++g) accf[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(gaf, (float)xu[g * 16 * St::pitch + 4 * ust * s], accf[g], 0, 0, 0);
                    } else {
                        const double ga = ga_p[lane & 15];
#pragma unroll
                        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga, (double)xu[g * 16 * St::pitch + 4 * ust * s], acc[g], 0, 0, 0);
                    }
                }
            }
        } else if (!sparse)
#pragma unroll
        for (int s = 0; s < kPiece / 4; ++s) {
            if constexpr (G4) {
                // v_mfma_f64_4x4x4_4b: four independent 4 x 4 x 4 products -- here the SAME four state rows against four groups of four chunks.
                // Its B operand (lane = 16 k + chunk) and its result (lane = 16 (row mod 4) + chunk) lie exactly where the 16 x 16 x 4
                // instruction has them, and register r of the accumulator is row group r; its A operand is G[4 r + (lane & 3)][k = lane >> 4]
                // in every group of four lanes -- read from the same table.  16 cycles against 64 (tools/ubench_mfma_f64_4x4.hip: 7.3 / 35 ns),
                // and only the row groups that hold states are multiplied: 4 biquads pay 2 x 16 cycles per step and column tile, not 64.
                constexpr int NG = (D + 3) / 4;   // row groups that hold states (rows >= D of the table are zero)
                double ga[NG];
#pragma unroll
                for (int r = 0; r < NG; ++r) ga[r] = gl[(p * (kPiece / 4) + s) * 64 + (lane & 48) + 4 * r + (lane & 3)];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const double b = (double)xs[g * 16 * St::pitch + 4 * s];
#pragma unroll
                    for (int r = 0; r < NG; ++r) acc[g][r] = __builtin_amdgcn_mfma_f64_4x4x4f64(ga[r], b, acc[g][r], 0, 0, 0);
                }
            } else if constexpr (V32) {
                const float gaf = glf[(p * (kPiece / 4) + s) * 64 + lane];
#pragma unroll
                for (int g = 0; g < 4; ++g) accf[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(gaf, (float)xs[g * 16 * St::pitch + 4 * s], accf[g], 0, 0, 0);
            } else {
                const double ga = gl[(p * (kPiece / 4) + s) * 64 + lane];
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga, (double)xs[g * 16 * St::pitch + 4 * s], acc[g], 0, 0, 0);
            }
        }
        wave_lds_sync();
    }
    }

    // chunk end states from the accumulator layout (column = lane & 15, state row = (lane >> 4) + 4 reg) to one lane per chunk
    double v[D];
    if constexpr (UPL) {
#pragma unroll
        for (int d = 0; d < D; ++d) v[d] = 0.0;
#pragma unroll
        for (int jj = 0; jj < NIN; ++jj) {
            if (jj < nin) {
                const int kk = jj * a.up;                                      // column of G: the same for every chunk
                const double *gp = gtab + (kk >> 2) * 64 + 16 * (kk & 3);     // (its D state rows are consecutive in the operand order of the table)
                const double xv = (double)xs[jj];
#pragma unroll
                for (int d = 0; d < D; ++d) v[d] = fma(gp[d], xv, v[d]);
            }
        }
#pragma unroll
        for (int k = 0; k < NSEC; ++k) *reinterpret_cast<v2d_t *>(E + (k * 64 + lane) * 2) = v2d_t{v[2 * k], v[2 * k + 1]};
        wave_lds_sync();
    } else if (sparse) {
        constexpr int JMAX = T / 8 + 1;
        const unsigned v0 = up_r0 + (unsigned)((lane / LS) * T);          // this lane's chunk start, counted from the last multiple of up in front of the segment
        const unsigned q = (unsigned)(((unsigned long long)v0 * a.up_magic) >> 32);
        const unsigned rem = v0 - q * (unsigned)a.up;
        const unsigned qa = q + (rem ? 1u : 0u), k0 = rem ? (unsigned)a.up - rem : 0u;   // first input sample of the chunk and its place in it
        const unsigned last = in_lim ? in_lim - 1u : 0u;
        const IO gain = (IO)a.up;
        IO xin[JMAX];
#pragma unroll
        for (int jj = 0; jj < JMAX; ++jj) {
            const unsigned qi = qa + (unsigned)jj;
            xin[jj] = in_lim ? xup[(qi < last ? qi : last) * LS + lane % LS] : IO(0);
        }
#pragma unroll
        for (int d = 0; d < D; ++d) v[d] = 0.0;
#pragma unroll
        for (int jj = 0; jj < JMAX; ++jj) {
            const unsigned k = k0 + (unsigned)jj * (unsigned)a.up;
            const bool ok = k < (unsigned)T && qa + (unsigned)jj < in_lim;
            const double xv = ok ? (double)(gain * xin[jj]) : 0.0;             // (the value the staging put into the chunk: rounded in the signal's type)
            const unsigned kk = k < (unsigned)T ? k : (unsigned)(T - 1);
            const double *gp = gl + (kk >> 2) * 64 + 16 * (kk & 3);             // column kk of G: its D state rows are consecutive
#pragma unroll
            for (int d = 0; d < D; d += 2) {
                const v2d_t g2 = *reinterpret_cast<const v2d_t *>(gp + d);
                v[d] = fma(g2[0], xv, v[d]);
                v[d + 1] = fma(g2[1], xv, v[d + 1]);
            }
        }
#pragma unroll
        for (int k = 0; k < NSEC; ++k) *reinterpret_cast<v2d_t *>(E + (k * 64 + lane) * 2) = v2d_t{v[2 * k], v[2 * k + 1]};
        wave_lds_sync();
    } else {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // state row: section d >> 1, component d & 1.  The FP64 instruction leaves row (lane >> 4) + 4 reg in register reg, the float32 one row 4 (lane >> 4) + reg
            const int d = V32 ? 4 * j + r : j + 4 * r;
            if (V32 || 4 * r < D) {
                const double av = V32 ? (double)accf[g][r] : acc[g][r];
                if (d < D) E[(((d >> 1) * 64) + 16 * g + c) * 2 + (d & 1)] = UP2 ? (double)UL * av : av;   // (UP2: the gain the zero-stuffed image would have carried)
            }
        }
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < NSEC; ++k) {
        const v2d_t t = *reinterpret_cast<const v2d_t *>(E + (k * 64 + lane) * 2);
        v[2 * k] = t[0];
        v[2 * k + 1] = t[1];
    }
    }

    // ---- S: from-rest inclusive scan of the wave's 64 chunk states ------------------------------------------------------
#pragma unroll 1
    for (int l = 0; l < a.n_lv; ++l) {
        const int s = LS << l;
        const int src = lane >= s ? lane - s : lane;
        double left[D];
#pragma unroll
        for (int k = 0; k < NSEC; ++k) {
            const v2d_t t = *reinterpret_cast<const v2d_t *>(E + (k * 64 + src) * 2);
            left[2 * k] = t[0];
            left[2 * k + 1] = t[1];
        }
        wave_lds_sync();
        if (lane >= s) blocks_acc<NSEC>(lvl + (size_t)l * NSEC * 4, left, v);
#pragma unroll
        for (int k = 0; k < NSEC; ++k) *reinterpret_cast<v2d_t *>(E + (k * 64 + lane) * 2) = v2d_t{v[2 * k], v[2 * k + 1]};
        wave_lds_sync();
    }
    double z[D];
#pragma unroll
    for (int k = 0; k < NSEC; ++k) {
        const v2d_t t = *reinterpret_cast<const v2d_t *>(E + (k * 64 + (lane >= LS ? lane - LS : 0)) * 2);
        z[2 * k] = lane >= LS ? t[0] : 0.0;
        z[2 * k + 1] = lane >= LS ? t[1] : 0.0;
    }

    // ---- L: publish the segment's end state(s) from rest, fetch the K predecessors' ------------------------------------
    // (CPLX: two states per segment -- lanes 62 / 63 hold the re / im stream's; granule g belongs to stream g >> 5)
    unsigned *cw = reinterpret_cast<unsigned *>(lds_raw + wave * kWaveStage + 64 * 16 * 8);   // behind the scan exchange, inside the (idle) image
    if (lane < GR && (lane & 31) < 2 * D) {
        const int d = (lane & 31) >> 1, src_lane = CPLX ? 62 + (lane >> 5) : 63;
        const unsigned half = reinterpret_cast<const unsigned *>(E)[((((d >> 1) * 64) + src_lane) * 2 + (d & 1)) * 2 + (lane & 1)];
        __hip_atomic_store(a.lb + (size_t)tk * GR + lane, ((unsigned long long)a.epoch << 32) | half, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    if (seg > 0) {
#pragma unroll 1
        for (int k0 = 0; k0 < a.K; k0 += 64 / GR) {
            const int back = k0 + (CPLX ? 0 : (lane >> 5)) + 1;   // this lane's predecessor distance
            const int gi = CPLX ? lane : (lane & 31);            // its granule
            unsigned got = 0;
            if (back <= a.K && back <= seg && (gi & 31) < 2 * D) {
                const unsigned long long *srcp = a.lb + (size_t)(tk - back) * GR + gi;
                unsigned long long g = 0;
                int spins = 0;
                for (;;) {
                    g = __hip_atomic_load(srcp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((unsigned)(g >> 32) == a.epoch) break;
                    if (++spins > (1 << 22)) {  // ~ seconds: never in a healthy run; fail loudly instead of hanging the GPU
                        *a.err = 1u;
                        g = 0;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(8);
                }
                got = (unsigned)g;
            }
            if (back <= KMAX) cw[(back - 1) * GR + gi] = got;
        }
        wave_lds_sync();

        // ---- C: z_j += Phi^j c,  c = sum_m Psi^m P_(s-1-m) ---------------------------------------------------------------
        double u[D];
        const double *cwd = reinterpret_cast<const double *>(cw) + (CPLX ? (lane & 1) * 16 : 0);   // (this lane's stream)
        const int cj = lane / LS;   // chunk index inside the segment
#pragma unroll
        for (int k = 0; k < NSEC; ++k) {
            const v2d_t t = *reinterpret_cast<const v2d_t *>(cwd + 2 * k);
            u[2 * k] = t[0];
            u[2 * k + 1] = t[1];
        }
#pragma unroll 1
        for (int m = 1; m < a.K; ++m) {
            double pm[D];
#pragma unroll
            for (int k = 0; k < NSEC; ++k) {
                const v2d_t t = *reinterpret_cast<const v2d_t *>(cwd + m * (GR / 2) + 2 * k);
                pm[2 * k] = t[0];
                pm[2 * k + 1] = t[1];
            }
            blocks_acc<NSEC>(psi + (size_t)(m - 1) * NSEC * 4, pm, u);
        }
        // (Phi^j by the binary digits of j: up to six rounds of 2 x 2 products, every lane through every level some lane needs -- ~480 vector instructions per
        // segment for the 32 multiply-adds a lane wants.  Round 6 tried the lane's own row of a [64][NSEC][4] table of Phi^j instead, requested in front of the
        // look-back's poll: 64 more live registers next to the chunk, 180 bytes of scratch per lane in the plain 8-biquad kernel; not kept.)
#pragma unroll 1
        for (int l = 0; l < a.n_lv; ++l) {
            if ((cj >> l) & 1) {
                double t2[D];
#pragma unroll
                for (int d = 0; d < D; ++d) t2[d] = 0.0;
                blocks_acc<NSEC>(lvl + (size_t)l * NSEC * 4, u, t2);
#pragma unroll
                for (int d = 0; d < D; ++d) u[d] = t2[d];
            }
        }
        if ((cj >> a.n_lv) == 0) {   // (Phi^j c is negligible for j >= 2^n_lv)
#pragma unroll
            for (int d = 0; d < D; ++d) z[d] += u[d];
        }
    }
    wave_lds_sync();  // the image is free again
    if (PRIO) __builtin_amdgcn_s_setprio(0);

    // ---- B: the recurrence over the register-resident chunk; outputs leave through the LDS image ------------------------
    // (the output taps live in VGPRs: 33 double coefficients next to the addresses do not fit a wave's 102 SGPRs, and
    // hipcc then shuffles them through v_readlane / re-reads them from the kernel arguments inside the body)
    double al[NSEC], be[NSEC], gam = cf.gamma;
    if constexpr (!UPL) {   // (UPL: the taps are row 0 of its table, and that arrives by scalar loads)
#pragma unroll
        for (int s = 0; s < NSEC; ++s) {
            al[s] = cf.al[s];
            be[s] = cf.be[s];
            asm volatile("" : "+v"(be[s]));
        }
    }
    // .dn, compact form: this lane's sample stream (T samples of chunk cj, component lane % LS) walks the positions
    // v = R0 + cj T + c of the segment, R0 = (first sample of the segment) mod dec; sample v is kept iff dec divides v, as
    // output Q0 + v / dec of the row.  (dq, dt) = (v / dec, v mod dec) of the next 16-byte unit, advanced by its size per unit.
    const bool compact = DEC && a.dec_compact;
    constexpr bool rounds = DECM == 2;
    int64_t dec_q0 = 0;
    unsigned dec_r0 = 0, dq = 0, dt = 0;
    if (DEC) {
        dec_q0 = m0 / a.dec;
        dec_r0 = (unsigned)(m0 - dec_q0 * a.dec);
        const unsigned v0 = dec_r0 + (unsigned)((lane / LS) * T);
        dq = (unsigned)(((unsigned long long)v0 * a.dec_magic) >> 32);
        dt = v0 - dq * (unsigned)a.dec;
    }
    const unsigned dec_ob = dec_r0 != 0 ? 1u : 0u;     // first output of the segment, relative to dec_q0
    const int64_t n_out = a.n_keep / a.dec;
    const int64_t olim64 = n_out - dec_q0;
    const unsigned olim = olim64 <= 0 ? 0u : (olim64 > 0x7fffffff ? 0x7fffffffu : (unsigned)olim64);   // outputs of this row from dec_q0 on
    // .dn, compact form: an output is a 2 NSEC + 1 term sum over the states, and only every dec-th one is kept -- the sum is formed for the
    // kept samples only (e0r: the kept element of the current 16-byte unit, if any, as the gathering below finds it).  The lanes of a wave
    // walk different phases unless dec divides the chunk length, so a sample's sum is skipped only where NO lane keeps it: at dec = 12 the
    // 64 chunks of a segment start at three different phases (128 mod 12 = 8) and three of twelve samples pay for the sum instead of all.
    unsigned dtr = dt, e0r = 0;
    int upj_cnt = 0;   // UPJ: (samples since the last input sample) - 1
    constexpr bool UPJ_PRE = UPJ && NSEC <= 4;
    // UPJ, up to 4 biquads: the rows c A^cnt arrive by scalar loads, wave-uniform, in PAIRS (rows cnt, cnt + 1 are adjacent in the table, row `up` repeats
    // row 0), requested a pair ahead.  Scalar loads return in no order, so a wave can only wait for ALL of them: with one row requested per sample the wait
    // for this sample's row was also the wait for the next one's, one sample old -- 200 clocks of scalar-cache latency against 40 of arithmetic, and four
    // waves per SIMD do not cover that (SQ_WAIT_ANY: half of every wave's life).  Pairs halve the waits and double the distance.
    double cjn[UPJ_PRE ? 2 * D : 1];   // the pair requested last: rows of the next two samples once the current pair is used up
    double cjc[UPJ_PRE ? 2 * D : 1];   // the pair in use
    int upj_c2 = 2;                    // first row of the pair to request next
    // more than 4 biquads: a row is 2 NSEC doubles = up to 32 scalar registers, a pair in use and a pair in flight would be all there are: one row, a sample ahead
    double cj1[(UPJ && !UPJ_PRE) ? D : 1];
    if constexpr (UPJ && !UPJ_PRE) {
#pragma unroll
        for (int d = 0; d < D; ++d) cj1[d] = upj[d];
    }
    if constexpr (UPJ_PRE) {
#pragma unroll
        for (int d = 0; d < 2 * D; ++d) cjn[d] = upj[d];
#pragma unroll
        for (int d = 0; d < 2 * D; ++d) cjc[d] = 0.0;
    }
    if constexpr (UPL) {
        // (the blocks of A^up, requested at the top of the kernel, have arrived: said HERE, so that no wait for them -- which would also be a wait for the
        // wave's own stores -- appears at the input samples inside the loop)
#pragma unroll
        for (int i = 0; i < 4 * NSEC; ++i) asm volatile("" : "+v"(AuV[i]));
    }
    int dnl_cnt = 0;                                  // DNL: samples since the last kept one
    unsigned dnl_o = (unsigned)(lane / LS) * (unsigned)(T / (DNL ? a.dec : 1));   // DNL: this lane's next output, counted from the segment's first
    int upl_ji = 1;                                   // UPL: the next input sample of the chunk
    double upl_next = UPL ? (double)xs[NIN > 1 ? 1 : 0] : 0.0;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if constexpr (UPL || UP2) wave_lds_sync();   // (the wave's rows are free: UPL / UP2 hand every 16-byte unit to the image as it completes)
        xv_t ou = xv_t(0);   // UP2: the unit being completed
#pragma unroll
        for (int k = 0; k < kPiece; ++k) {
            constexpr int kE = St::elems;
            const int e = (p * kPiece + k) % kE;
            if (DEC && !UNI && e == 0) {
                e0r = dtr == 0 ? 0u : (unsigned)a.dec - dtr;
                dtr += kE;
                dtr = dtr >= (unsigned)a.dec ? dtr - (unsigned)a.dec : dtr;
                dtr = dtr >= (unsigned)a.dec ? dtr - (unsigned)a.dec : dtr;   // (M = 2, 3: a 4-sample unit spans more than one period)
            }
            double xd;
            const bool zero_in = UP2 && ((p * kPiece + k) % UL) != 0;   // UP2: a stuffed zero (known here, not tested)
            if constexpr (UPL) xd = p * kPiece + k == 0 ? (double)xs[0] : upl_next;   // (read at input samples only)
            else if constexpr (UP2) xd = zero_in ? 0.0 : (double)UL * (double)xin[((p * kPiece + k) / UL) / kE][((p * kPiece + k) / UL) % kE];
            else xd = (double)xq[(p * kPiece + k) / kE][e];
            if constexpr (UPJ) {
                if (p * kPiece + k > 0) {   // (the chunk's first sample is an input sample met with the state from the scan: the plain step below)
                    // (up to 4 biquads the row c A^cnt of THIS sample was requested a sample ago -- scalar loads, wave-uniform -- and the next one goes
                    // out first; longer rows would not leave the scalar registers for two of them)
                    double cj[D];
                    const bool is_input = upj_cnt == a.up - 1;
                    if constexpr (UPJ_PRE) {
                        const int half = (p * kPiece + k - 1) & 1;   // samples 1, 2 are the first pair
                        if (half == 0) {
#pragma unroll
                            for (int d = 0; d < 2 * D; ++d) cjc[d] = cjn[d];
                            asm volatile("" : "+s"(upj_c2));   // (one address at a time: hipcc otherwise works out the addresses of many pairs ahead and spills them)
                            const double *nr = upj + (size_t)upj_c2 * D;
#pragma unroll
                            for (int d = 0; d < 2 * D; ++d) cjn[d] = nr[d];
                            upj_c2 += 2;                                   // (rows c2, c2 + 1; the pair behind row up - 1 or up starts over)
                            upj_c2 = upj_c2 >= a.up ? upj_c2 - a.up : upj_c2;
                        }
#pragma unroll
                        for (int d = 0; d < D; ++d) cj[d] = cjc[half * D + d];
                        upj_cnt = is_input ? 0 : upj_cnt + 1;
                    } else {
#pragma unroll
                        for (int d = 0; d < D; ++d) cj[d] = cj1[d];
                        upj_cnt = is_input ? 0 : upj_cnt + 1;
                        const double *nr = upj + (size_t)upj_cnt * D;
#pragma unroll
                        for (int d = 0; d < D; ++d) cj1[d] = nr[d];
                    }
                    double yv = cj[0] * z[0];
                    yv = fma(cj[1], z[1], yv);
#pragma unroll
                    for (int s = 1; s < NSEC; ++s) {
                        yv = fma(cj[2 * s], z[2 * s], yv);
                        yv = fma(cj[2 * s + 1], z[2 * s + 1], yv);
                    }
                    if (is_input) {   // an input sample: its direct term, and the state jumps to right behind it (the blocks of A^up: one sample in `up`)
                        yv = fma(gam, xd, yv);
                        const double *Au = AuV;
#pragma unroll
                        for (int s = 0; s < NSEC; ++s) {
                            const double n0 = fma(Au[4 * s + 1], z[2 * s + 1], fma(Au[4 * s], z[2 * s], xd));
                            const double n1 = fma(Au[4 * s + 3], z[2 * s + 1], Au[4 * s + 2] * z[2 * s]);
                            z[2 * s] = n0;
                            z[2 * s + 1] = n1;
                        }
                        if constexpr (UPL) {
                            upl_ji = upl_ji + 1 < NIN ? upl_ji + 1 : NIN - 1;
                            upl_next = (double)xs[upl_ji];   // (a wave-uniform index into registers)
                        }
                    }
                    xq[(p * kPiece + k) / kE][e] = (IO)yv;
                    if constexpr (UPL) {
                        if (e == kE - 1) *reinterpret_cast<xv_t *>(myrow + (k / kE) * kE) = xq[(p * kPiece + k) / kE];
                    }
                    continue;
                }
                if constexpr (UPL) {   // the chunk's first sample: an input sample met with the state from the scan -- the taps are row 0, the step the plain one
                    double yv = gam * xd;
#pragma unroll
                    for (int d = 0; d < D; ++d) yv = fma(UPJ_PRE ? cjn[d] : cj1[d], z[d], yv);   // (the first pair / row, requested above, is or starts with row 0)
                    xq[0][0] = (IO)yv;
#pragma unroll
                    for (int s = 0; s < NSEC; ++s) {
                        const double w0 = fma(cf.na2[s], z[2 * s + 1], fma(cf.na1[s], z[2 * s], xd));
                        z[2 * s + 1] = z[2 * s];
                        z[2 * s] = w0;
                    }
                    continue;
                }
            }
            bool keep;
            if constexpr (UNI) keep = dnl_cnt == 0;
            else keep = !DEC || e0r == (unsigned)e || e0r + (unsigned)a.dec == (unsigned)e;   // (the unit's kept samples: e0r and, with M below the samples of a unit, e0r + M)
            if constexpr (UNI) dnl_cnt = dnl_cnt + 1 == a.dec ? 0 : dnl_cnt + 1;
            if constexpr (DNL) {
                if (keep) {
                    double yv = gam * xd;
#pragma unroll
                    for (int s = 0; s < NSEC; ++s) {
                        yv = fma(al[s], z[2 * s], yv);
                        yv = fma(be[s], z[2 * s + 1], yv);
                    }
                    if (dnl_o < olim) {
                        const unsigned slot = dnl_o * LS + (unsigned)(lane % LS);
                        stage[slot + (slot >> 5)] = (IO)yv;
                    }
                    ++dnl_o;
                }
            } else if (keep) {
                // (one chain of 2 NSEC + 1 dependent operations per output.  Measured and not kept, round 6: two chains -- even and odd sections -- and one add:
                // config 4 0.1435 -> 0.1455 ms, .dn(x, 3) 0.136 -> 0.140; the recurrences of the same sample already fill the chain's gaps)
                double yv = zero_in ? al[0] * z[0] : fma(al[0], z[0], gam * xd);
                yv = fma(be[0], z[1], yv);
#pragma unroll
                for (int s = 1; s < NSEC; ++s) {
                    yv = fma(al[s], z[2 * s], yv);
                    yv = fma(be[s], z[2 * s + 1], yv);
                }
                if constexpr (UP2) {
                    ou[e] = (IO)yv;
                    if (e == kE - 1) *reinterpret_cast<xv_t *>(myrow + (k / kE) * kE) = ou;
                } else {
                    xq[(p * kPiece + k) / kE][e] = (IO)yv;
                }
            }
#pragma unroll
            for (int s = 0; s < NSEC; ++s) {
                const double w0 = fma(cf.na2[s], z[2 * s + 1], zero_in ? cf.na1[s] * z[2 * s] : fma(cf.na1[s], z[2 * s], xd));
                z[2 * s + 1] = z[2 * s];
                z[2 * s] = w0;
            }
        }
        if constexpr (DNL) continue;   // (the kept outputs are in the image already)
        if (compact) {
#pragma unroll
            for (int sgi = 0; sgi < St::segs; ++sgi) {
                const xv_t u = xq[p * St::segs + sgi];
                const unsigned e0 = dt == 0 ? 0u : (unsigned)a.dec - dt;    // the unit's kept sample, if < elems (dec >= elems: at most one)
                IO pick = u[0];
#pragma unroll
                for (int e = 1; e < St::elems; ++e) pick = (e0 == (unsigned)e) ? u[e] : pick;
                const unsigned oq = dq + (dt != 0);                          // its output, relative to dec_q0
                if (e0 < (unsigned)St::elems && oq < olim) {
                    const unsigned slot = (oq - dec_ob) * LS + (unsigned)(lane % LS);
                    stage[slot + (slot >> 5)] = pick;                        // (one pad per 32: the lanes' runs start T / dec slots apart)
                }
                dt += St::elems;
                if (dt >= (unsigned)a.dec) { dt -= (unsigned)a.dec; dq += 1; }
            }
            continue;
        }
        if (rounds) continue;   // (the outputs stay in the registers of the chunk until the gathering below)
        if (PRIO && SK_PAR_PRIO_ST) __builtin_amdgcn_s_setprio(SK_PAR_PRIO);   // (the piece's way out through the image: -2.7 %)
        if constexpr (!UPL && !UP2) {
            wave_lds_sync();  // the wave's rows are free (its previous piece's stores have read them)
#pragma unroll
            for (int sgi = 0; sgi < St::segs; ++sgi) *reinterpret_cast<xv_t *>(myrow + sgi * St::elems) = xq[p * St::segs + sgi];
        }
        wave_lds_sync();
        if (!DEC && interior) {
            {
                // (all reads of the image first, into the registers the piece has just left: issued one behind the other they cost
                // one LDS round trip; hipcc otherwise cycles two staging vectors through four read -> wait -> store rounds)
                pre_t outq[St::per_thread];
#pragma unroll
                for (int i = 0; i < St::per_thread; ++i) outq[i] = image_get(i);
#pragma unroll
                for (int i = 0; i < St::per_thread; ++i) asm volatile("" : "+v"(outq[i]));
#pragma unroll
                for (int i = 0; i < St::per_thread; ++i)
                    __builtin_nontemporal_store(outq[i], reinterpret_cast<pre_t *>(yseg + (loff + i * kRowStep + p * kPiece * LS)));
            }
            if (PRIO && SK_PAR_PRIO_ST) __builtin_amdgcn_s_setprio(0);
            continue;
        }
        int64_t dq_run = 0;
        int dr_run = 0;
#pragma unroll 1
        for (int i = 0; i < St::per_thread; ++i) {
            const int idx = i * 64 + lane;
            const int r = idx / USEG, sg = idx % USEG;
            const int64_t g = (row0 + r) * T + (int64_t)p * kPiece + (int64_t)sg * (St::elems / LS);   // first sample of the unit
            const pre_t val = image_get(i);
            const IO *tmp = reinterpret_cast<const IO *>(&val);
            if (DEC && !CPLX) {
                // decimating store (as in iir_fused_kernel): segment i of this lane starts a fixed number of samples after
                // segment i - 1, so its (quotient, remainder) by dec follow from the first by adding (dec_dq, dec_dr)
                if (i == 0) {
                    dq_run = g / a.dec;
                    dr_run = (int)(g - dq_run * a.dec);
                }
                if (a.dec >= St::elems) {  // at most one kept sample per 16-byte segment
                    const int e0 = dr_run == 0 ? 0 : a.dec - dr_run;
                    if (e0 < St::elems && g + e0 < a.n_keep) {
                        IO pick = tmp[0];
#pragma unroll
                        for (int e = 1; e < St::elems; ++e) pick = (e0 == e) ? tmp[e] : pick;
                        y[dq_run + (dr_run != 0)] = pick;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < St::elems; ++e) {
                        const int t = dr_run + e;  // < dec + elems
                        const int m = (t >= a.dec) + (t >= 2 * a.dec) + (t >= 3 * a.dec) + (t >= 4 * a.dec);
                        if (t == m * a.dec && g + e < a.n_keep) y[dq_run + m] = tmp[e];
                    }
                }
                dq_run += a.dec_dq;
                dr_run += a.dec_dr;
                if (dr_run >= a.dec) { dr_run -= a.dec; ++dq_run; }
            } else if (g < a.n) {
#pragma unroll
                for (int e = 0; e < St::elems; ++e)
                    if (g + e / LS < a.n) y[g * LS + e] = tmp[e];
            }
        }
    }
    if constexpr (rounds) {
        // dec = 2, 3 on 4-sample units: the chunks of the segment in a.dec_rounds ranges; a range's kept outputs are a run of the row
        const unsigned M = (unsigned)a.dec;
        const int per = CH / a.dec_rounds;                              // chunks per range
        const int cj = lane / LS;
        const unsigned v0 = dec_r0 + (unsigned)(cj * T);
        const unsigned dq0 = (unsigned)(((unsigned long long)v0 * a.dec_magic) >> 32), dt0 = v0 - dq0 * M;
#pragma unroll 1
        for (int rd = 0; rd < a.dec_rounds; ++rd) {
            const unsigned vb = dec_r0 + (unsigned)(rd * per * T);       // the range's first sample
            const unsigned ob_r = (vb + M - 1) / M;                        // its first output, relative to dec_q0
            if (cj / per == rd) {
                unsigned q = dq0, t = dt0;
#pragma unroll
                for (int ui = 0; ui < T / St::elems; ++ui) {
                    const xv_t u = xq[ui];
                    // the unit's kept samples: e0 = (-t) mod M and, if it still lies inside the unit, e0 + M
                    const unsigned e0 = t == 0 ? 0u : M - t, e1 = e0 + M;
                    IO p0 = u[0], p1 = u[St::elems - 1];
#pragma unroll
                    for (int e = 1; e < St::elems; ++e) {
                        p0 = (e0 == (unsigned)e) ? u[e] : p0;
                        p1 = (e1 == (unsigned)e) ? u[e] : p1;
                    }
                    const unsigned o0 = q + (t != 0);                      // output of the sample at e0, relative to dec_q0
                    const unsigned slot = (o0 - ob_r) * LS + (unsigned)(lane % LS);
                    if (e0 < (unsigned)St::elems && o0 < olim) stage[slot + (slot >> 5)] = p0;
                    if (e1 < (unsigned)St::elems && o0 + 1 < olim) stage[slot + LS + ((slot + LS) >> 5)] = p1;
                    t += St::elems;
                    const unsigned kk = (t >= M) + (t >= 2 * M);
                    t -= kk * M;
                    q += kk;
                }
            }
            wave_lds_sync();
            const unsigned ve = dec_r0 + (unsigned)((rd + 1) * per * T);
            unsigned oe_r = (ve + M - 1) / M;
            if (oe_r > olim) oe_r = olim;
            const int cnt = oe_r > ob_r ? (int)(oe_r - ob_r) * LS : 0;
            IO *yo = y + (dec_q0 + ob_r) * LS;
#pragma unroll 1
            for (int i = lane; i < cnt; i += 64) __builtin_nontemporal_store(stage[i + (i >> 5)], yo + i);
            wave_lds_sync();
        }
    }
    if (compact) {
        // the segment's kept outputs: one contiguous run of the row, y[dec_q0 + dec_ob ...)
        wave_lds_sync();
        const int64_t ob = dec_q0 + dec_ob;
        int64_t oe = dec_q0 + (int64_t)((dec_r0 + (unsigned)(CH * T) + (unsigned)a.dec - 1) / (unsigned)a.dec);
        if (oe > n_out) oe = n_out;
        const int cnt = oe > ob ? (int)(oe - ob) * LS : 0;
        IO *yo = y + ob * LS;
#pragma unroll 1
        for (int i = lane; i < cnt; i += 64) __builtin_nontemporal_store(stage[i + (i >> 5)], yo + i);
    }
}

// ------------------------------------------------------------------------------------------------------- host side
// The numerics (par_expand, par_v32_probe, the table values) and the dispatch decision (par_choose) are iir_par_plan.hpp: standard headers only,
// run on the host by tests/host/iir_par_plan_emul.cpp.  Here: the device copies of the tables, the launch arguments and the one launch.
static_assert(kParPlanMaxK == kParMaxK && kParPlanT32 == SK_PAR_T32 && kParPlanStageM2 == kParStageM2, "iir_par_plan.hpp mirrors these constants");
static_assert(par_stage_image_bytes(4) == (int64_t)64 * Stage<float>::pitch * (int64_t)sizeof(float) &&
              par_stage_image_bytes(8) == (int64_t)64 * Stage<double>::pitch * (int64_t)sizeof(double), "par_stage_image_bytes is 64 rows of Stage<IO>");

struct ParTables {
    int T = 0;                   // 0: not made yet (published, with n_lv and K, once the three tables below are on the device)
    int n_lv = 0, K = 0;         // K = 0: the filter remembers more than par_max_k segments of this length (not served)
    DevTable<double> gt, lvl, psi;   // ParTableValues::gt, lvl, psi on the device
    int v32 = 0;                 // V = G x in float32 for chunks of this length (par_v32_probe): 0 not probed, 1 admitted, -1 refused
    double v32_err = 0.0;        // ... the worst probe error it showed (a refusal: the first one above the limit)
};

struct ParPlan : TilePlan {      // (owned by its handle through the base: IirHandle::par)
    int state = 0;               // 0 untested, 1 expansion accepted, -1 not applicable
    ParExpansion e;
    ParTables tab[8];            // by slot (iir_par_plan.hpp: par_slot_T and its neighbours)
    struct UpJump : TilePlan { DevTable<double> dev; };
    TilePlans upj;               // per L (the key): par_upj_values on the device (UPJ kernels)
    DevBuffer lbg_dev;           // look-back granules
    DevTable<unsigned long long> ticket_dev;   // kParTickets dispensers (allocated and zeroed by the first launch)
    unsigned long long ticket_count = 0;
    unsigned epoch = 0;
};
static ParPlan *par_plan_of(const IirHandle *h) { return static_cast<ParPlan *>(h->par.get()); }

// host-only: the expansion of a handle's cascade (tests; no GPU needed).  out = [c0, (a1, a2, r0, r1) x nsec, kappa, ir_err, v32_err at 128, at 96]:
// 5 + 4 nsec doubles
int iir_par_expand_host(const double *coef, int nsec, double *out, int *accepted)
{
    ParExpansion P;
    const bool ok = nsec >= 1 && nsec <= 8 && par_expand(coef, nsec, P);
    if (accepted) *accepted = ok ? 1 : 0;
    if (out) {
        out[0] = (double)P.c0;
        for (int k = 0; k < nsec && k < 8; ++k) {
            out[1 + 4 * k] = (double)P.a1[k];
            out[2 + 4 * k] = (double)P.a2[k];
            out[3 + 4 * k] = (double)P.r0[k];
            out[4 + 4 * k] = (double)P.r1[k];
        }
        out[1 + 4 * nsec] = P.kappa;
        out[2 + 4 * nsec] = P.ir_err;
        // the float32 from-rest states of 128- and 96-sample chunks (V32): the worst probe error, admitted below kParV32Limit
        out[3 + 4 * nsec] = ok ? par_v32_probe(P, SK_PAR_T32) : 1.0;
        out[4 + 4 * nsec] = ok ? par_v32_probe(P, 96) : 1.0;
    }
    return SKDSP_OK;
}

// a table's allocation and the copy of its values, enqueued: the caller syncs once behind its group of tables (v outlives that sync)
static int par_upload(const std::vector<double> &v, DevTable<double> &t, hipStream_t s)
{
    const int rc = t.alloc(v.size());
    if (rc) return rc;
    SK_HIP(hipMemcpyAsync(t.dev, v.data(), v.size() * 8, hipMemcpyHostToDevice, s));
    return SKDSP_OK;
}

// par_choose's K query: the tables of a slot, made on first use.  Returns K (0: not served at this chunk length) or a negative error
static int par_slot_K(ParPlan &P, int slot, hipStream_t s)
{
    ParTables &tb = P.tab[slot];
    if (tb.T != 0) return tb.K;
    const ParTableValues v = par_table_values(P.e, par_slot_T(slot), par_slot_chunks(slot), par_slot_negl(slot), par_max_k(par_slot_dbl(slot)));
    if (!v.failed) {   // a failed attempt leaves the slot unmade (the next call tries again; a second alloc frees the first)
        int rc = par_upload(v.gt, tb.gt, s);
        if (!rc) rc = par_upload(v.lvl, tb.lvl, s);
        if (!rc) rc = par_upload(v.psi, tb.psi, s);
        if (rc) {
            (void)hipStreamSynchronize(s);   // (copies already enqueued read v, a local)
            return rc;
        }
        SK_HIP(hipStreamSynchronize(s));
    }
    tb.n_lv = v.n_lv;
    tb.K = v.failed ? 0 : v.K;
    tb.T = par_slot_T(slot);
    return tb.K;
}

// UPJ table of a plan for the factor L, made on first use
static int par_upj_table(ParPlan &P, int L, hipStream_t s, const double **out)
{
    ParPlan::UpJump *u = nullptr;
    const int rc = tile_plan(P.upj, plan_key(L), &u, [&](ParPlan::UpJump &t) -> int {
        const std::vector<double> tab = par_upj_values(P.e, L);
        const int rc2 = par_upload(tab, t.dev, s);
        if (rc2) return rc2;
        SK_HIP(hipStreamSynchronize(s));
        return SKDSP_OK;
    });
    if (!rc) *out = u->dev.dev;
    return rc;
}

// Which <N, IO, DECM, CPLX, TT, UPJ, UPS, V32> exist: the families <IO, TT, UPJ, UPS> par_choose names, and inside them the variants the kernel was
// written for.  Nothing else is instantiated (this file is the long pole of the build), and par_launch_kernel refuses everything else.
template <int N, typename IO, int DECM, bool CPLX, int TT, bool UPJ, int UPS, bool V32> constexpr bool par_kernel_exists()
{
#ifdef SK_PAR_DEV_NSEC   // (developer builds: one cascade length only)
    if (N != SK_PAR_DEV_NSEC) return false;
#endif
#ifdef SK_PAR_DEV_F32REAL   // (developer builds: float32 real signals only -- a third of the instantiations)
    if (sizeof(IO) == 8 || CPLX) return false;
#endif
    constexpr bool io4 = sizeof(IO) == 4;
    // UPJ: chunks of 96, every dtype.  Other chunks of 96 (.dn, .up by 3): 4-byte types.  Default chunks: plain / .dn and .up by 2 for every dtype, .up by 4 for 4-byte types
    constexpr bool family = UPJ ? (TT == 96 && UPS == 0) : TT == 96 ? (io4 && (UPS == 0 || UPS == 3)) : (TT == 0 && (UPS == 0 || UPS == 2 || (UPS == 4 && io4)));
    constexpr bool variant = DECM == 2 ? (io4 && !UPJ && UPS == 0)                              // (the .up families never decimate)
                             : DECM == 3 ? (io4 && !UPJ && UPS == 0 && TT == 96 && N > 4)
                             : DECM == 1 ? (!UPJ && UPS == 0)
                                         : (UPJ || UPS != 0 || TT == 0);
    constexpr bool v32 = !V32 || (N >= 7 && io4 && DECM == 0 && !UPJ);   // (.dn keeps the float64 from-rest states: par_choose)
    return family && variant && v32;
}

struct ParLaunch {   // a launch, but for the kernel's template parameters
    ParArgs a;
    const ParExpansion *e;
    const ParTables *tb;
    const double *upj;   // UPJ: the jump table; else null
    unsigned grid;
    hipStream_t s;
};

static int par_no_kernel(int N, int elem_bytes, int DECM, bool CPLX, int TT, bool UPJ, int UPS, bool V32)
{
    set_error("iir: no parallel-form kernel for %d biquads, %d-byte %s samples, DECM %d, TT %d, UPJ %d, UPS %d, V32 %d", N, elem_bytes,
              CPLX ? "complex" : "real", DECM, TT, (int)UPJ, UPS, (int)V32);
    return SKDSP_ERR_UNSUPPORTED;
}

template <int N, typename IO, int DECM, bool CPLX, int TT, bool UPJ, int UPS, bool V32> static int par_launch_kernel(const ParLaunch &L)
{
    if constexpr (par_kernel_exists<N, IO, DECM, CPLX, TT, UPJ, UPS, V32>()) {
        ParCoef<N> cf;
        for (int k = 0; k < N; ++k) { cf.na1[k] = L.e->na1[k]; cf.na2[k] = L.e->na2[k]; cf.al[k] = L.e->al[k]; cf.be[k] = L.e->be[k]; }
        cf.gamma = L.e->gamma;
        if constexpr (V32) note_path("iir_par_v32");   // (tests assert which arithmetic ran by this record)
        hipLaunchKernelGGL((iir_par_kernel<N, IO, DECM, CPLX, TT, UPJ, UPS, V32>), dim3(L.grid), dim3(kIirThreads), 0, L.s, L.a, cf,
                           L.tb->gt.dev, L.tb->lvl.dev, L.tb->psi.dev, 0ull, L.upj);
        return SKDSP_OK;
    } else
        return par_no_kernel(N, (int)sizeof(IO), DECM, CPLX, TT, UPJ, UPS, V32);
}

// run time -> template parameters: the variant (DECM, V32), the cascade length, the sample type
template <int N, typename IO, bool CPLX, int TT, bool UPJ, int UPS> static int par_launch_variant(int decm, bool v32, const ParLaunch &L)
{
    switch (2 * decm + (v32 ? 1 : 0)) {
        case 0: return par_launch_kernel<N, IO, 0, CPLX, TT, UPJ, UPS, false>(L);
        case 1: return par_launch_kernel<N, IO, 0, CPLX, TT, UPJ, UPS, true>(L);
        case 2: return par_launch_kernel<N, IO, 1, CPLX, TT, UPJ, UPS, false>(L);
        case 3: return par_launch_kernel<N, IO, 1, CPLX, TT, UPJ, UPS, true>(L);
        case 4: return par_launch_kernel<N, IO, 2, CPLX, TT, UPJ, UPS, false>(L);
        case 6: return par_launch_kernel<N, IO, 3, CPLX, TT, UPJ, UPS, false>(L);
        default: return par_no_kernel(N, (int)sizeof(IO), decm, CPLX, TT, UPJ, UPS, v32);
    }
}

template <typename IO, bool CPLX, int TT, bool UPJ, int UPS> static int par_launch_nsec(int nsec, int decm, bool v32, const ParLaunch &L)
{
    switch (nsec) {
        case 1: return par_launch_variant<1, IO, CPLX, TT, UPJ, UPS>(decm, v32, L);
        case 2: return par_launch_variant<2, IO, CPLX, TT, UPJ, UPS>(decm, v32, L);
        case 3: return par_launch_variant<3, IO, CPLX, TT, UPJ, UPS>(decm, v32, L);
        case 4: return par_launch_variant<4, IO, CPLX, TT, UPJ, UPS>(decm, v32, L);
        case 5: return par_launch_variant<5, IO, CPLX, TT, UPJ, UPS>(decm, v32, L);
        case 6: return par_launch_variant<6, IO, CPLX, TT, UPJ, UPS>(decm, v32, L);
        case 7: return par_launch_variant<7, IO, CPLX, TT, UPJ, UPS>(decm, v32, L);
        case 8: return par_launch_variant<8, IO, CPLX, TT, UPJ, UPS>(decm, v32, L);
        default: break;
    }
    set_error("iir: parallel-form scan takes 1..8 biquads");
    return SKDSP_ERR_UNSUPPORTED;
}

template <int TT, bool UPJ, int UPS> static int par_launch_dtype(bool dbl, bool interleaved, int nsec, int decm, bool v32, const ParLaunch &L)
{
    switch ((dbl ? 1 : 0) + (interleaved ? 2 : 0)) {
        case 0: return par_launch_nsec<float, false, TT, UPJ, UPS>(nsec, decm, v32, L);
        case 1: return par_launch_nsec<double, false, TT, UPJ, UPS>(nsec, decm, v32, L);
        case 2: return par_launch_nsec<float, true, TT, UPJ, UPS>(nsec, decm, v32, L);
        default: return par_launch_nsec<double, true, TT, UPJ, UPS>(nsec, decm, v32, L);
    }
}

// the call par_choose decided on: the launch arguments, the scratch a launch needs, the kernel
static int launch_par(IirHandle *h, ParPlan *p, const ParChoice &c, bool dbl, bool interleaved, const void *x, int64_t n, int nrow, int64_t x_stride,
                      int64_t y_stride, void *y, hipStream_t s, int dec, int up)
{
    note_path("iir_par");
    ParTables &tb = p->tab[c.slot];
    const int T = tb.T;
    const size_t elem = dbl ? 8 : 4;
    // V32 (see the kernel), once the probe has admitted this filter at this chunk length
    bool v32 = false;
    if (c.v32_wanted) {
        if (tb.v32 == 0) {
            tb.v32_err = par_v32_probe(p->e, T, kParV32Limit);
            tb.v32 = tb.v32_err <= kParV32Limit ? 1 : -1;
        }
        v32 = tb.v32 == 1 || opt().iir_par_v32 >= 2;
    }
    const int64_t S = (int64_t)(interleaved ? 32 : 64) * T;   // samples per wave segment
    const int64_t nseg = (n + S - 1) / S;
    SK_CHECK(nseg * nrow < (1 << 30), SKDSP_ERR_BADARG, "iir: too many segments");
    const int total = (int)(nseg * nrow);
    int rc;
    if (!p->ticket_dev.dev) {
        if ((rc = p->ticket_dev.alloc(kParTickets))) return rc;
        if (hipError_t e = hipMemsetAsync(p->ticket_dev.dev, 0, 8 * kParTickets, s)) {
            p->ticket_dev.reset();   // (dispensers that were never zeroed must not be found by the next call)
            return hip_fail(e, "hipMemsetAsync(tickets)", __FILE__, __LINE__);
        }
        p->ticket_count = 0;
    }
    const size_t need = (size_t)total * (interleaved ? 64 : 32) * 8;
    bool fresh;
    if ((rc = p->lbg_dev.reserve(need, s, &fresh))) return rc;
    if (fresh) SK_HIP(hipMemsetAsync(p->lbg_dev.dev, 0, need, s));  // epoch 0 is never used as a tag
    ParLaunch L;
    ParArgs &a = L.a;
    a.x = x; a.y = y; a.n = n; a.x_stride = x_stride; a.y_stride = y_stride;
    a.nseg = (int)nseg; a.total = total;
    a.lb = p->lbg_dev.as<unsigned long long>(); a.ticket = p->ticket_dev.dev; a.ticket_base = p->ticket_count;
    a.epoch = ++p->epoch;
    if (a.epoch == 0) a.epoch = ++p->epoch;
    a.n_lv = tb.n_lv; a.K = tb.K;
    a.err = async_err_dev(kAsyncErrIirLookback);
    SK_CHECK(a.err, SKDSP_ERR_HIP, "iir: no host-mapped error word");
    a.aligned = ((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0 && (nrow == 1 || ((x_stride * elem) % 16 == 0 && (y_stride * elem) % 16 == 0))) ? 1 : 0;
    a.dec = dec > 1 ? dec : 1;
    a.dec_magic = a.dec > 1 ? (unsigned)((((unsigned long long)1 << 32) + a.dec - 1) / a.dec) : 0u;
    a.dec_compact = c.dec_compact ? 1 : 0;
    a.dec_rounds = c.dec_rounds;
    a.up = up > 1 ? up : 1;
    a.up_magic = a.up > 1 ? (unsigned)((((unsigned long long)1 << 32) + a.up - 1) / a.up) : 0u;
    a.n_in = a.up > 1 ? n / a.up : n;
    a.n_keep = (n / a.dec) * a.dec;
    L.upj = nullptr;
    if (c.UPJ) {
        if ((rc = par_upj_table(*p, a.up, s, &L.upj))) return rc;
    }
    {
        const int64_t step = (int64_t)(64 / (dbl ? Stage<double>::segs : Stage<float>::segs)) * T;   // samples between a lane's staged segments
        a.dec_dq = (int)(step / a.dec);
        a.dec_dr = (int)(step % a.dec);
    }
    // (whole rounds of kParTickets workgroups, so that every dispenser advances by the same amount: the surplus workgroups
    // draw segments beyond the last and leave)
    L.grid = (unsigned)(((total + 3) / 4 + kParTickets - 1) / kParTickets * kParTickets);
    L.e = &p->e; L.tb = &tb; L.s = s;
    if (c.UPJ) rc = par_launch_dtype<96, true, 0>(dbl, interleaved, h->nsec, c.DECM, v32, L);
    else if (c.TT == 96) rc = c.UPS == 3 ? par_launch_dtype<96, false, 3>(dbl, interleaved, h->nsec, c.DECM, v32, L)
                                         : par_launch_dtype<96, false, 0>(dbl, interleaved, h->nsec, c.DECM, v32, L);
    else if (c.UPS == 2) rc = par_launch_dtype<0, false, 2>(dbl, interleaved, h->nsec, c.DECM, v32, L);
    else if (c.UPS == 4) rc = par_launch_dtype<0, false, 4>(dbl, interleaved, h->nsec, c.DECM, v32, L);
    else rc = par_launch_dtype<0, false, 0>(dbl, interleaved, h->nsec, c.DECM, v32, L);
    if (rc) return rc;   // (nothing was launched: the dispensers stay where they are)
    p->ticket_count += (unsigned long long)(L.grid / kParTickets);
    SK_HIP(hipGetLastError());
    return SKDSP_OK;
}

// Does the parallel form take this call, and how (status 0; otherwise the call goes to the cascade kernels): the plan on first use, then par_choose.
ParChoice iir_par_takes(IirHandle *h, int64_t n, int nrow, int dec, int interleaved, int up, hipStream_t s)
{
    ParChoice no;
    if (h->order != 2 || !par_call_shape_ok(h->nsec, interleaved != 0, nrow, dec, up, n)) return no;
    const bool dbl = dtype_double(h->dtype);
#ifdef SK_PAR_DEV_F32REAL   // (developer builds have the float32 real kernels only: every other signal takes the cascade kernels)
    if (dbl || interleaved) return no;
#endif
    if (!h->par) {
        std::unique_ptr<ParPlan> made(new ParPlan());
        made->state = par_expand(h->coef.data(), h->nsec, made->e) ? 1 : -1;
        h->par = std::move(made);
    }
    ParPlan *p = par_plan_of(h);
    if (p->state != 1) return no;   // (poles shared between sections, slow decay, ...)
    const ParOptions o{opt().iir_dn_t96, opt().iir_up_jump, opt().iir_up_lean, opt().iir_dn_compact, opt().iir_par_v32};
    return par_choose(h->nsec, dbl, interleaved != 0, nrow, dec, up, n, o, [&](int slot) { return par_slot_K(*p, slot, s); });
}

// the launch of a choice iir_par_takes made for this handle and this call
int iir_par_launch(IirHandle *h, const ParChoice &c, const void *x, int64_t n, int nrow, int64_t x_stride, int64_t y_stride, void *y, hipStream_t s, int dec,
                   int interleaved, int up)
{
    ParPlan *p = par_plan_of(h);
    SK_CHECK(c.status == 0 && p && p->state == 1 && p->tab[c.slot].T != 0, SKDSP_ERR_UNSUPPORTED,
             "iir_par: the parallel form does not take this call");
    const bool dbl = dtype_double(h->dtype);
    if (interleaved) return launch_par(h, p, c, dbl, true, x, n, 1, 0, 0, y, s, dec, up);
    return launch_par(h, p, c, dbl, false, x, n, nrow, x_stride, y_stride, y, s, dec, up);
}

}  // namespace skdsp
