// Internal declarations shared by the HIP translation units of libskdsp_hip.so.
// gfx950 (MI355X / CDNA4) only -- no portability layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <memory>
#include <mutex>
#include "../../include/skdsp.h"
#include "careful.hpp"
#include "dev_mem.hpp"

namespace skdsp {

// ------------------------------------------------------------------ errors
void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define SK_HIP(call)                                                        \
    do {                                                                    \
        hipError_t _e = (call);                                             \
        if (_e != hipSuccess) return skdsp::hip_fail(_e, #call, __FILE__, __LINE__); \
    } while (0)

#define SK_CHECK(cond, code, ...)            \
    do {                                     \
        if (!(cond)) {                       \
            skdsp::set_error(__VA_ARGS__);   \
            return (code);                   \
        }                                    \
    } while (0)

// Which engines the calling thread's last API calls launched (tests assert that a shape reaches the engine they mean to exercise):
// every *_launch appends its name once; skdsp_debug_path() reads and clears.  A few bytes of thread-local state, no device work.
void note_path(const char *engine);

// ------------------------------------------------------------------ options
// Run-time switches.  Read from the environment ONCE (first use: SKDSP_<NAME>), changed afterwards only through
// skdsp_set_option(): no getenv() on any launch path.  Most are developer A/B switches of measured alternatives.
struct Options {
    int device = -1;          // SKDSP_DEVICE: GPU to bind when skdsp_init() was not called explicitly
    int fir_algo = 0;         // SKDSP_FIR_ALGO = auto|direct|ols (0|1|2): override of every handle's choice
    int dn_no_ols = 0;        // .dn never through the overlap-save decimating store
    int fir_mm = 1;           // 0: no matrix-pipe FIR kernels at all (register sliding-window kernels instead)
    int fir_bx = 1;           // 0: no bf16x3 matrix-pipe kernel (FP32 matrix pipe instead)
    int fir_bx_t16 = 1;       // the float32 plain filter on the matrix pipe stores its 256-output tiles as runs (a 4 x 4 transpose between registers and lane groups); 0: four 64-byte runs per store (A/B switch)
    int ols_keep_overlap = 1; // overlap-save tiles: the blocks a tile shares with its neighbours are loaded with ordinary (L2-resident) loads, the rest nontemporal; 0: all nontemporal, 2: all ordinary -- what every value executed before the policy was compiled per block (A/B switch; complex64 tiles of fir_ols.hip)
    int ols_reserve = 8;      // workgroup slots a persistent overlap-save launch leaves free
    int ols_walk = 1;         // the walk of ols_tile_kernel: 0 dealt (workgroup b takes tiles first(b), + grid, ...), 1 claimed for the plain filter (ols_walk.hpp: workgroups draw tiles from per-XCD ranges), 2 claimed for every form of the kernel; the same bytes whichever (A/B switch; measured in profiles/r18)
    int iir_planar = 0;       // complex IIR through two real planes (tests compare it with the interleaved kernels)
    int iir_dn_full = 0;      // .dn as full-rate scan + downsample kernel
    int iir_no_mfma = 0;      // recurrence K1 instead of the matrix-pipe K1
    int iir_two_pass = 0;     // 1: K1 + carries + K3 even where the single-pass scan applies; -1: single pass wherever it applies
    int iir_par = 1;          // 0: never the parallel-form scan (iir_par.hip); the cascade kernels everywhere
    int iir_par_v32 = 1;      // the parallel form's from-rest end states of float32 / complex64 signals, 7 - 8 biquads, on the float32 matrix instruction: 1 where the
                              // plan's probe admits the filter (iir_par_plan.hpp: par_v32_probe), 2 always (tests, A/B), 0 never
    int iir_up_jump = 1;      // the parallel-form .up of float32 / complex64 signals by L >= 8, a divisor of 96: lean kernels whose state jumps from input sample to input sample; 0 never (A/B switch)
    int iir_seq = 1;          // cascades of more than 8 sections whose float64 spread the scans would lift past the contract run the reference's recursion (iir_seq.hip): 1 probed, 2 always, 0 never
    int iir_up_lean = 1;      // multirate_IIR.up by 2 staged at the input rate with the stuffed zeros known at compile time (A/B switch; 0: the zero-stuffed image)
    int iir_dn_t96 = 1;       // the parallel-form .dn of float32 / complex64 signals on 96-sample chunks: 1 where measured to pay (see par_choose in iir_par_plan.hpp), 2 wherever M divides 96, 3 as 1 but M = 2 keeps its gathering in ranges for every cascade, 0 never (A/B switch)
    int iir_dn_compact = 1;   // 0: the parallel-form .dn keeps the image-and-pick store for every M (A/B switch)
    int fir_up_ols_min = 64;  // multirate_FIR.up: phases of at least this many taps MAY go through the overlap-save walk (the cost model
                              // of fir_up_model in fir_route.hpp decides); 0: never; -k: always from k taps per phase on (A/B switch)
    int fir_up_rows_min = -1; // multirate_FIR.up through the overlap-save walk: from this L on the phases leave as rows and a second kernel weaves them
                              // (-1: the measured crossover per dtype, fir_up_rows in fir_route.hpp; 0: never)
    int fir_up_pair = 1;      // 0: float32 .up through the overlap-save walk never pairs its phases (A/B switch)
    int fir_up4k = 1;         // 0: multirate_FIR.up never through the one-workgroup-per-input-tile interpolator (fir_up4k.hip); the older engines instead (A/B switch)
    int fir_up2k = 1;         // the 2048-point tile with all phases per thread (fir_up2k.hip): 1 from five passes on (complex64: L >= 5, float32: L >= 9), 2 always, 0 never (A/B switch)
    int fir_up_rep = 1;       // multirate_FIR.up, even L, through the replicated spectrum of the zero-stuffed tile (ols_rep_kernel): 1 where the cost model prefers it, 2 wherever it applies, 0 never (A/B switch)
    int fir_dn_fold = 1;      // multirate_FIR.dn through overlap-save, M = 2, 4, 8, 16: the folded spectrum's inverse transform (ols_fold_kernel); 0: the decimating store (A/B switch)
    int fir_dn4k = 1;         // multirate_FIR.dn through the frequency-domain decimator (fir_dn4k.hip): 1 where the cost model prefers it, 2 wherever it applies, 0 never (A/B switch)
    int fir_up4k_group = 4;   // phases (float32: pairs of phases) whose results a thread of that kernel holds before it stores: 4 (32 bytes per lane) or 2 (A/B switch)
    int fir_up4k_staged = 1;  // 0: four-pass groups of that kernel store each lane's own 32 bytes (A/B switch)
    int fir_bank_per = 0;     // FIR bank (fir_bank.hip): bands per group; 0: the cost rule of bank_bands_per_group, k > 0: k per group (A/B switch; k >= the bands: one group)
    int fir_updn_fused = 1;   // 0: L / M through the overlap-save walk writes all n L outputs to scratch and copies every M-th (A/B switch)
    int iir_up_fused = 1;     // 0: multirate_IIR.up / rate_change.up write the zero-stuffed signal first (A/B switch)
    int shard_two_launches = 0; // sharded FIR: tile 0 as its own launch behind the halo event (instead of the in-kernel flag wait)
    int shard_probe = 1;        // 1: a process's FIRST sharded step runs the two-launch form, its second the overlapped form on probation (short
                                // poll, tile 0 repeated behind the halo event, one sync) and only a passed probation makes the overlapped form
                                // the steady state (dist.hip); 0: overlapped from the first step; 2 (test hook): the probation step's flag is
                                // never published, i.e. the probation fails
    int shard_halo_state = 0;   // read-only mirror of that state machine: 0 no sharded step yet, 1 first step done (probation next), 2 overlapped form
                                // proven, 3 probation failed (two-launch form for good)
    int shard_self_halo = 0;    // test hook: a 1-rank communicator sends its tail to ITSELF (exercises the whole halo path on one GPU)
    int dist_force_comm = 0;  // build an RCCL communicator for a 1-rank job too (exercises the plumbing on one GPU)
    int host_chunk_log2 = 22; // host-pointer entry points: samples per pipelined chunk (pinned double buffers)
    int host_pipeline = 1;    // 0: single staged copy in / kernel / copy out
    int psd_f32_image = 0;    // the Welch primitive (psd.hip) on float32 / complex64 signals: 1 keeps the transform's LDS image in float32 (each pass
                              // still computed in float64 and rounded once at its store): the 1e-6 contract only, not the per-bin one
    int host_multi_slot = 1;  // 0: host-pointer FIR calls stay on the caller's slot even when several are bound
    int pulse_mf_variant = 0; // the matched filter over rows (pulse.hip), A/B switch for timing only: 1 stages its window in its natural order (the naive
                              // layout: lanes read `step` apart), 2 contracts each product and sum into one fused multiply-add (NOT the host form's bits)
};
Options &opt();

// ------------------------------------------------------------------ context
// One Context per SLOT: a (device, stream, workspaces) binding.  Slot 0 is what every caller thread uses (skdsp_init);
// skdsp_init_devices binds further slots -- one per GPU of the node, or several on one GPU -- which the host-pointer
// entry points use from their own worker threads to spread a long host vector over all of them.  Each slot has its own
// lock: calls that run on different slots do not serialise each other.
constexpr int kMaxSlots = 16;
struct HostPipe;  // host_pipe.hip: pinned-free chunk pipeline state (streams, events, double buffers)
struct Context {
    bool ready = false;
    int slot = 0;
    int device = -1;
    HostPipe *pipe = nullptr;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    // grow-only device workspaces used by the host-pointer entry points
    hipStream_t comm_stream = nullptr;   // halo traffic of a sharded FIR, overlapped with the interior tiles
    hipEvent_t ev_in = nullptr, ev_halo = nullptr;
    unsigned *halo_flag = nullptr;       // device word the halo stream bumps when a shard's history has landed
    unsigned *async_err = nullptr;       // host-mapped [kAsyncErrWords]: kernels of this slot report here (async_err_check)
    unsigned halo_seq = 0;
    double last_timer_ms = -1.0;         // skdsp_last_kernel_ms
    int halo_state = 0;                  // the probation state machine of the sharded FIR step (Options::shard_halo_state mirrors it)
    void *ws[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t ws_bytes[4] = {0, 0, 0, 0};
    std::mutex mu;
};
// Failures a kernel can only report after the fact (a bounded device-side wait that gave up) land in host-mapped words of
// the slot; every entry point that synchronises the slot's stream tests them right after the sync, so the error is
// returned by the call that makes the affected results visible (and the word is cleared: later calls are not poisoned).
enum { kAsyncErrHalo = 0, kAsyncErrIirLookback = 1, kAsyncErrWords = 4 };
unsigned *async_err_dev(int which);   // device alias of the calling slot's word (allocated on first use); null on failure
int async_err_check(Context &c);      // call after a stream sync of slot c
Context &ctx();               // the calling thread's current slot (slot 0 unless a library worker selected another)
Context &ctx_of(int slot);
int slot_count();             // bound slots (0 before the first init)
int select_slot(int slot);    // thread-local: subsequent ctx() / launches of this thread use that slot (and its device)
int ensure_init();
int ws_reserve(int slot, size_t bytes, void **out);  // grow-only workspace slot 0..3

inline size_t dtype_size(int dt) { return dt == SKDSP_F32 ? 4 : dt == SKDSP_C64 ? 8 : dt == SKDSP_F64 ? 8 : 16; }
inline bool dtype_complex(int dt) { return dt == SKDSP_C64 || dt == SKDSP_C128; }
inline bool dtype_double(int dt) { return dt == SKDSP_F64 || dt == SKDSP_C128; }
inline bool dtype_valid(int dt) { return dt >= 0 && dt <= 3; }

// headroom (in samples) the host-pointer paths keep in front of the staged input
// so that kernels may be handed n_hist > 0; also keeps x 256-byte aligned.
constexpr int64_t kHeadroomBytes = 65536;

// ------------------------------------------------------------------ handles
enum HandleKind { H_FIR = 1, H_IIR = 2, H_FIRBANK = 3, H_VITERBI = 4, H_BLOCKCODE = 5, H_CONVCODE = 6, H_PULSE = 7 };

struct HandleBase {
    int kind;
    int dtype;
    int slot = 0;           // slot whose device holds this handle's tables
    std::vector<HandleBase *> clones;  // same filter on the other slots, made on demand by the multi-slot host path (owned)
    bool wide_out = false;  // host-pointer entry points deliver float64/complex128 (skdsp_set_wide_output)
    std::mutex mu;
    virtual ~HandleBase()
    {
        for (HandleBase *c : clones) delete c;
    }
};

// The one rule of the handles below: DEVICE MEMORY A HANDLE OWNS IS A DevTable OR A DevBuffer (dev_mem.hpp), alone or inside a plan of a TilePlans
// cache.  No handle declares a raw device pointer, no destructor enumerates allocations, a table is non-empty only once its upload succeeded,
// and a lookup hands out the plan's address, which holds for the life of the handle.  (Context-owned memory -- workspaces, the host pipeline,
// the sharding state -- has an explicit shutdown order instead: runtime.hip.)

// ---- the launch arithmetic of the tile engines (fir_up4k.hip, fir_up2k.hip, fir_dn4k.hip, fir_bank.hip) -------
// The launch arithmetic of a persistent walk over tiles (their overlap: tile_overlap in ols_tables.hpp).
// 2 workgroups per CU, less the slots option ols_reserve leaves free (where the grid is at least 4 x that), at most one per tile
inline int64_t persistent_grid(int64_t ntiles)
{
    int64_t grid = 2 * (int64_t)ctx().num_cus;
    const int reserve_wgs = opt().ols_reserve;
    if (reserve_wgs > 0 && grid >= 4 * (int64_t)reserve_wgs) grid -= reserve_wgs;
    return grid > ntiles ? ntiles : grid;
}
inline bool elem_aligned(const void *x, const void *y, int esz) { return ((((uintptr_t)x) | ((uintptr_t)y)) & (uintptr_t)(esz - 1)) == 0; }

// ---- FIR -----------------------------------------------------------------
struct FirHandle : HandleBase {
    int ntaps = 0;
    bool taps_complex = false;
    int algo = SKDSP_FIR_AUTO;
    std::vector<double> taps_host;  // ntaps (real) or 2*ntaps (complex, interleaved)
    DevTable<double> taps64;        // the same on the device, natural order (careful.hpp: the rare exact path of a poisoned tile); lazy
    // Per-shape tables and plans, made on first use; each engine's file derives its plan type and packs the key (plan_key):
    TilePlans poly;      // polyphase tap banks, keyed by L: bank[phase][t] = b[phase + L*t], T = ceil(P/L) (fir_direct.hip)
    TilePlans sw;        // sliding-window tap tables, keyed by (L, M, R) (fir_direct.hip)
    TilePlans mm;        // Toeplitz-product (matrix pipe) A-operand tables, keyed by (L, M) (fir_mm.hip)
    TilePlans bx;        // bf16x3 Toeplitz-product A-operand tables, keyed by (L, M) (fir_bx.hip)
    TilePlans ols;       // overlap-save plans, keyed by (kind, L): the plain filter and the walks of multirate_FIR.up (fir_ols.hip)
    TilePlans up4k;      // plans of the frequency-domain interpolator, keyed by L (fir_up4k.hip)
    TilePlans up2k;      // ... of its many-phase form (fir_up2k.hip)
    TilePlans dn4k;      // plans of the frequency-domain decimator, keyed by M (fir_dn4k.hip)
    TilePlans ols64;     // float64 overlap-save plans, keyed by (paired, L) (fir_ols64.hip)
    // Filters longer than one kernel launch takes (fir_part_len in fir_route.hpp) run as partial FIRs over consecutive tap segments,
    // each applied to the correspondingly delayed input and summed (fir_api.hip): parts[s] holds taps [s seg, (s+1) seg).
    std::vector<FirHandle *> parts;
    int part_seg = 0;
    // Calls FROM REST over fewer samples than taps only ever reach the first n taps: they run on a copy of the filter cut to the next power of
    // two >= n (fir_api.hip, fir_head) -- exact, and the float32 rounding then scales with the taps that matter, not with the whole filter
    std::vector<FirHandle *> heads;
    ~FirHandle();
};

// the taps as the careful path reads them (uploaded on first use, under the handle's lock like every other table)
int fir_careful(FirHandle *h, CarefulFir *out);

// Which engine a call runs, and whether an engine applies to a shape: fir_route.hpp (standard headers only; the FIR units include it).
// direct-form / polyphase launcher (fir_direct.hip): the tier fir_direct_tier (fir_route.hpp) names -- fir_bx_launch, fir_mm_launch, or its own kernels.
//   y[m] = L * sum_t b[phi + L t] * x[i - t],  j = m*M, phi = j mod L, i = j div L,  m in [0, n_out)
int fir_direct_launch(FirHandle *h, int tier, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, int64_t n_out,
                      void *y_dev, hipStream_t s);
// Toeplitz product on the FP32 matrix pipe (fir_mm.hip): float32 / complex64 signals, real taps
int fir_mm_launch(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, int64_t n_out, void *y_dev,
                  hipStream_t s);
// Toeplitz product on the BF16 matrix pipe in float32 precision (3-way bf16 split, fir_bx.hip): same coverage, tried first
int fir_bx_launch(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, int64_t n_out, void *y_dev,
                  hipStream_t s);
// FFT overlap-save (fir_ols.hip): c64 (and packed f32) .filter
int fir_ols_tile_outputs(FirHandle *h, int *V);  // outputs per overlap-save tile (builds the plan if needed)
int fir_algo_for(const FirHandle *h, int64_t n);  // SKDSP_FIR_OLS / SKDSP_FIR_DIRECT as skdsp_fir_filter_dev would pick
int fir_ols_launch(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev, hipStream_t s,
                   int dec = 1,           // dec > 1: decimating store, y holds n / dec samples
                   int reserve_wgs = -1,  // persistent grid smaller by this many workgroups (multiple of 8; -1: default 8)
                   // sharded launches: tile 0 is walked last and waits until *halo_flag >= halo_seq (the history in front
                   // of x is being received on another stream); halo_err (host-mapped) is set if that wait gives up
                   const unsigned *halo_flag = nullptr, unsigned halo_seq = 0, unsigned *halo_err = nullptr,
                   int halo_spins = 0);   // polls of ~1 us before that wait gives up (0: the steady-state bound, seconds)
int fir_ols_publish_halo(unsigned *flag, unsigned seq, hipStream_t s);  // one-thread kernel: *flag = seq (agent-scope release)
// multirate_FIR.up as an overlap-save walk over (tile, phase) pairs: complex64, float32 with real taps; 2..4097 taps per phase
int fir_ols_up_launch(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, void *y_dev, hipStream_t s, int dec = 1,
                      int64_t rows_pitch = 0, int paired = 0);  // dec = M: L / M, floor(n L / M) outputs; rows_pitch > 0: y[phase * rows_pitch + i] instead of
                                                                 // y[i L + phase]; paired: see fir_ols_up_pairs in fir_route.hpp (rows then hold 8-byte pairs, L / 2 of them)
// multirate_FIR.up, even L, tiles of the OUTPUT: the zero-stuffed tile's forward transform from its non-zero columns (fir_ols.hip: ols_rep_kernel)
int fir_ols_rep_launch(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, void *y_dev, hipStream_t s);
// multirate_FIR.up, one workgroup per input tile, all L phases from one forward transform (fir_up4k.hip): complex64, float32 with real
// taps; at most 2049 taps per phase
int fir_up4k_launch(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, void *y_dev, hipStream_t s);
// the same with a 2048-point tile and ALL phases of a sample in one thread (fir_up2k.hip): at most 1025 taps per phase
int fir_up2k_launch(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, void *y_dev, hipStream_t s);
// multirate_FIR.dn, one workgroup per OUTPUT tile: M forward transforms accumulated in the frequency domain, one inverse (fir_dn4k.hip)
int fir_dn4k_launch(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int M, void *y_dev, hipStream_t s);
// FFT overlap-save in float64 (fir_ols64.hip): complex128, and float64 with real taps; 2..2049 taps
int fir_ols64_launch(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev, hipStream_t s, int dec = 1);
int fir_ols64_up_launch(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, void *y_dev, hipStream_t s, int dec = 1, int64_t rows_pitch = 0, int paired = 0);

// ---- FIR bank (fir_bank.hip): B frequency-shifted copies of one FIR over ONE input, sigsys.fft_caf (sigsys.py:2696-2781) --------------
// band j = taps[n] exp(2 pi i ((shifts[j] n) mod period) / period); float32 / complex64 signals, complex64 rows; at most 2049 taps.
// The handle (a HandleBase of kind H_FIRBANK) owns its tables; skdsp_destroy frees it.
int fir_bank_create(const void *taps, int ntaps, int taps_complex, const int64_t *shifts, int nbands, int period, int dtype, HandleBase **out);
int fir_bank_launch(HandleBase *h, const void *x_dev, int64_t n, void *y_dev, int64_t row_stride, hipStream_t s);   // row j at y + j row_stride, n outputs each, from rest

// ---- IIR -----------------------------------------------------------------
struct IirPlan;  // iir_common.hpp
struct IirHandle : HandleBase {
    int nsec = 0;   // number of cascaded sections
    int order = 0;  // order of each section (2 for SOS, K-1 for a transfer function)
    std::vector<double> coef;  // per section: b[0..order], a[1..order]  (a0-normalised)
    // Biquad cascades whose sections all have b2 == b0 (zeros on the unit circle: every Butterworth / Chebyshev /
    // elliptic design of scipy.signal, all band types) are re-factored at creation -- the same transfer function with
    // all gain in section 0 and b0 = b2 = 1 in the others -- so that K3 needs 3 coefficients and 4 flops per such
    // section (iir_scan.hip).  state_scale[d] converts a DF2T state of the caller's factorisation into the internal
    // one (z_int = scale * z); empty = identity.
    bool unit_tail = false;
    std::vector<double> state_scale;
    // made on first use, owned through the base like the plans of a cache (the types are their units'): iir_plan_of() / par_plan_of() read them
    std::unique_ptr<TilePlan> plan;   // IirPlan (iir_common.hpp): the tables and buffers of the cascade scans
    std::unique_ptr<TilePlan> par;    // ParPlan (iir_par.hip): the partial-fraction form of the same transfer function
    // Cascades of more than 8 biquads run as consecutive groups of at most 8 (the kernels' register budgets; 8 is what the parallel form
    // takes): group g filters the output of group g - 1 in place, each with its own plans; the caller's per-section states are sliced.
    // scipy.signal.sosfilt takes any number of sections, and so does this.
    std::vector<IirHandle *> groups;
    // float32 handles whose sections cannot be grouped in float32 (the rounding of the signal between two groups, amplified by the rest
    // of the cascade, would break the float32 contract: iir_api.hip) and are too many for one launch sequence: the same cascade as a float64
    // handle; the signal is widened, filtered and narrowed on the device
    IirHandle *twin64 = nullptr;
    DevBuffer twin_in, twin_out;
    // Cascades whose float64 result is itself uncertain beyond what the scans may add to it (iir_api.hip: the probe at creation) run the reference's
    // own recursion (iir_seq.hip): the caller's sections [nsec][5], the relative float64 spread the probe measured
    bool seq = false;
    double seq_spread = 0.0;
    std::vector<double> seq_coef;
    DevTable<double> seq_coef_dev;
    int group_first = 0;             // (a group: its first section in the parent's numbering)
    DevBuffer group_tmp;             // full-rate intermediate of a decimating call
    ~IirHandle();
};
// Which engines a call runs is ONE decision (iir_route.hpp, standard headers only), made before the call's first kernel and executed by
// iir_api.hip (iir_run), which also owns the plans, the workspaces and the state transfer.  The units below only launch: an engine that is
// asked for a call it does not take returns SKDSP_ERR_UNSUPPORTED.  x / y: real rows or planes in the handle's precision (complex through
// two planes: nrow = 2), or interleaved complex where an engine says so.  In-place (y == x) is allowed.
// the reference's recursion, one wave per row (iir_seq.hip): handles with h->seq set
int iir_seq_launch(IirHandle *h, const void *x_dev, int64_t n, int nrow, int64_t x_stride, int64_t y_stride, void *y_dev, hipStream_t s,
                   const double *zi_host = nullptr, double *zf_host = nullptr, int dec = 1);
// Parallel-form single-pass scan (iir_par.hip): real signals, <= 8 biquads with simple poles, zero initial state, no state
// output; nrow rows x_stride / y_stride elements apart in one launch.  iir_par_takes: does it take this call (ParChoice::status == 0), and how
// (the plan and its tables on first use); iir_par_launch: the launch of such a choice.
struct ParChoice;   // iir_par_plan.hpp
ParChoice iir_par_takes(IirHandle *h, int64_t n, int nrow, int dec, int interleaved, int up, hipStream_t s);
int iir_par_launch(IirHandle *h, const ParChoice &c, const void *x_dev, int64_t n, int nrow, int64_t x_stride, int64_t y_stride, void *y_dev, hipStream_t s,
                   int dec = 1, int interleaved = 0,    // interleaved = 1: x / y interleaved complex, n complex samples, one row
                   int up = 1);                         // up > 1: x holds n / up samples, the launch filters up * upsample(x, up) (n outputs)
int iir_par_expand_host(const double *coef, int nsec, double *out, int *accepted);   // host-only (tests): [c0, (a1,a2,r0,r1) x nsec, kappa, ir_err, v32_err at 128, at 96]: 5 + 4 nsec doubles

// ---- resamplers (resample.hip) ---------------------------------------------
int upsample_launch(const void *x_dev, int64_t n, int L, int dtype, double scale, void *y_dev, hipStream_t s);
int upsample_planes_launch(const void *x_dev, int64_t n, int L, int dtype_complex_in, double scale, void *re_dev, void *im_dev,
                           hipStream_t s);  // complex zero-stuffing straight into two real planes
int downsample_launch(const void *x_dev, int64_t n, int M, int p, int dtype, void *y_dev, hipStream_t s);
int interleave_launch(const void *src_dev, int64_t n, int L, int64_t pitch, int dtype, void *y_dev, hipStream_t s);   // y[i L + p] = src[p pitch + i]
int deinterleave_launch(const void *x_dev, int64_t n, int dtype_complex_in, void *re_dev, void *im_dev, hipStream_t s);
int interleave_launch(const void *re_dev, const void *im_dev, int64_t n, int dtype_complex_out, void *y_dev, hipStream_t s);
int widen_launch(const void *src_dev, int64_t nscalars, void *dst_dev, hipStream_t s);  // float32 -> float64
int convert_launch(const void *src_dev, void *dst_dev, int64_t nscalars, bool to_double, hipStream_t s);   // element-wise float32 <-> float64, any alignment
int accumulate_launch(void *y_dev, const void *t_dev, int64_t nscalars, bool dbl, hipStream_t s);  // y += t
int fill_noise_launch(void *x_dev, int64_t n, int dtype, uint64_t seed, int64_t first, hipStream_t s);

// ---- Farrow resampler (farrow.hip) -----------------------------------------
int farrow_len(int64_t n, double ts_old, double ts_new, int64_t *n_out);   // host-only
int farrow_launch(const void *x_dev, int64_t n, int dtype, double ts_old, double ts_new, int i_ord, double alpha, int64_t n0,
                  int64_t count, int flags, void *y_dev, hipStream_t s);   // outputs [n0, n0 + count) into y_dev

// ---- Welch primitive (psd.hip) ----------------------------------------------
// S_dev[k] = sum_{i < nseg} |FFT_{n_fft}(window * x[i step .. i step + ns))[k]|^2, float64; window is a host array of ns doubles
int psd_check(int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg);   // host-only: the argument rules
int psd_launch(const void *x_dev, int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg,
               double *S_dev, hipStream_t s);

// ---- Viterbi decoder (viterbi.hip): fec_conv.FECConv.viterbi_decoder (fec_conv.py:252-499); the plan and the step are viterbi_core.hpp ----
// The handle (a HandleBase of kind H_VITERBI) owns the decoder state its stateful calls carry; skdsp_destroy frees it.
int viterbi_create(const char *const *polys, int npoly, int depth, HandleBase **out);
int viterbi_out_len(HandleBase *h, int64_t nval, int64_t *n_out);   // host-only
int viterbi_reset(HandleBase *h, hipStream_t s);
int viterbi_check(HandleBase *h, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, int stateful);   // host-only: the argument rules
int viterbi_launch(HandleBase *h, const void *x_dev, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, uint8_t *y_dev, int stateful,
                   hipStream_t s);

// ---- block codes (blockcode.hip): fec_block.FECHamming / FECCyclic (fec_block.py:61-423); the plan and the per-block functions are blockcode_core.hpp ----
// The handle (a HandleBase of kind H_BLOCKCODE) owns the code's three device tables; skdsp_destroy frees it.
int blockcode_create(int n, int k, const uint32_t *enc, const uint32_t *syn, const uint32_t *trap, HandleBase **out);
void blockcode_sizes(HandleBase *h, int *n, int *k);   // host-only
int blockcode_check(HandleBase *h, int64_t nblocks);   // host-only: the argument rules
int blockcode_launch(HandleBase *h, int mode, const uint8_t *in_dev, int64_t nblocks, uint8_t *out_dev, hipStream_t s);   // mode 0 encode, 1 decode

// ---- the FEC chain around the decoder (convcode.hip): conv_encoder / puncture / depuncture over rows and the count of digitalcom.bit_errors; the plans are convcode_core.hpp ----
// The handle (a HandleBase of kind H_CONVCODE) holds the encoder's masks only (no device memory); skdsp_destroy frees it.
int convcode_create(const char *const *polys, int npoly, HandleBase **out);   // host-only
void convcode_sizes(HandleBase *h, int *K, int *R);                           // host-only
int convcode_check(HandleBase *h, int64_t n, int64_t nrow, int64_t nstates_in);   // host-only: the argument rules
int convcode_launch(HandleBase *h, const uint8_t *bits_dev, int64_t n, int64_t nrow, const uint8_t *states_in_dev, int64_t nstates_in, uint8_t *code_dev,
                    uint8_t *states_out_dev, hipStream_t s);
int gather_check(int depuncture, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, int64_t *n_out);   // host-only; n_out: elements per output row
int gather_launch(int depuncture, const void *x_dev, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase_host,
                  void *y_dev, hipStream_t s);
int bitcount_check(int64_t tx_stride, int64_t rx_stride, int64_t n, int64_t nrow);   // host-only
int bitcount_launch(const uint8_t *tx_dev, int64_t tx_stride, const uint8_t *rx_dev, int64_t rx_stride, int64_t n, int64_t nrow, int invert, int64_t *counts_dev,
                    hipStream_t s);

// ---- Gray symbol mapping (symmap.hip): the symbol sequences of qam_gray_encode_bb / mpsk_gray_encode_bb and qam_gray_decode / mpsk_gray_decode over rows; the plans are symmap_core.hpp ----
// kind 0 QAM, 1 MPSK; symbols are complex64 / complex128, symbol k of a row is element start + k step; bits are bytes 0 / 1 at any alignment.  No handle: the tables travel as arguments.
int sym_bits_per_symbol(int kind, int mod);   // host-only: 0 for an order the family does not have
int symmap_check(int kind, int mod, int64_t n, int64_t nrow, int dtype, int64_t bits_stride, int64_t y_stride);   // host-only
int symmap_launch(const uint8_t *bits_dev, int64_t bits_stride, int64_t n, int64_t nrow, int kind, int mod, const double *tab_re_host, const double *tab_im_host, int ntab,
                  int dtype, void *y_dev, int64_t y_stride, hipStream_t s);
int symscale_check(int mod, int64_t n, int64_t nrow, int dtype, int64_t x_stride, int64_t start, int64_t step);   // host-only
size_t symscale_scratch_bytes(int64_t n, int64_t nrow);                                                            // host-only: the partial moments of a launch
int symscale_launch(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double c, void *scratch_dev,
                    double *r_dev, hipStream_t s);
int symdemap_check(int kind, int mod, int64_t n, int64_t nrow, int dtype, int64_t x_stride, int64_t start, int64_t step, int64_t bits_stride);   // host-only
int symdemap_launch(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int kind, int mod, const double *r_dev,
                    double rot_re, double rot_im, uint8_t *bits_dev, int64_t bits_stride, hipStream_t s);
// var_dev[row] = np.var of the row (M2 / n of the same merge of partial moments), rows of any of the four dtypes; scratch_dev as for symscale_launch
int symvar_launch(const void *x_dev, int64_t x_stride, int64_t n, int64_t nrow, int dtype, void *scratch_dev, double *var_dev, hipStream_t s);

// ---- the AWGN channel and the bit sources (channel.hip): cpx_awgn / cpx_awgn2 / awgn_channel, random data bits, pn_gen over rows; the draw and the plans are channel_core.hpp ----
// The value of element i of row r depends on (seed, first_row + r, first + i) only.  Strides in elements (bytes for bits); no handle: the plans travel as arguments.
int awgn_check(int x_dtype, int y_dtype, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, int64_t first, int64_t first_row);   // host-only
int awgn_launch(const void *x_dev, int64_t x_stride, int x_dtype, void *y_dev, int64_t y_stride, int y_dtype, int64_t n, int64_t nrow, const double *g_dev,
                const double *sigma_dev, double g, double sigma, uint64_t seed, int64_t first, int64_t first_row, hipStream_t s);
int chanbits_check(const char *name, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, int64_t first, int64_t first_row);          // host-only
int chanbits_launch(const uint8_t *x_dev, int64_t x_stride, uint8_t *y_dev, int64_t y_stride, int64_t n, int64_t nrow, const double *sigma_dev, double sigma, uint64_t seed,
                    int64_t first, int64_t first_row, int random, hipStream_t s);
int pn_check(int Q, int64_t n, int64_t nrow, int64_t y_stride, int64_t first);                                                                // host-only
int pn_launch(const uint8_t *period_dev, int Q, const int64_t *phases_dev, uint8_t *y_dev, int64_t y_stride, int64_t n, int64_t nrow, int64_t first, hipStream_t s);
int awgn_sigma_launch(int mode, double ns, double p, double var_w, int64_t nrow, double *g_dev, double *sigma_dev, hipStream_t s);

// ---- OFDM (ofdm.hip): digitalcom.ofdm_tx / ofdm_rx / chan_est_equalize over rows; the argument rules, the plans and the per-thread phases are ofdm_core.hpp ----
// complex64 / complex128 rows, strides in elements.  nsym: the data symbols of a row (tx), its received symbols (rx), the rows of its z (equalize).
// hht_host: the known channel on the nf filled carriers (complex128 on the HOST) or null; scratch_dev: ofdm_scratch_bytes, 256-byte aligned.
int ofdm_tx_check(int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, int64_t x_stride, int64_t y_stride);   // host-only
int ofdm_tx_launch(const void *x_dev, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, void *y_dev, int64_t y_stride,
                   hipStream_t s);
int ofdm_rx_check(int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, int has_table, int64_t x_stride, int64_t z_stride);   // host-only
size_t ofdm_scratch_bytes(int64_t nsym, int64_t nrow, int nf);                                                                                          // host-only
int ofdm_rx_launch(const void *x_dev, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, double alpha,
                   const double *hht_host, void *scratch_dev, void *z_dev, int64_t z_stride, void *h_dev, hipStream_t s);
int ofdm_equalize_check(int64_t nsym, int64_t nrow, int dtype, int nf, int npb, int64_t z_stride, int64_t out_stride);   // host-only
int ofdm_equalize_launch(const void *z_dev, int64_t z_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int npb, double alpha, const double *hht_host,
                         void *scratch_dev, void *out_dev, int64_t out_stride, void *h_dev, hipStream_t s);

// ---- symbol-error tools (symerr.hip): digitalcom.xcorr / qam_sep / qpsk_bep / bpsk_bep; the plans and the per-element decisions are symerr_core.hpp ----
// R[l] = sum_n a[(n + l) mod K] conj(b[n]) over the reference's lag window, float64, with E1 = sum |a|^2 and E2 = sum |b|^2; quant_levels M > 0 passes a through
// qam_sep's quantiser at the load.  The count: tx symbol i = tx[t0 + i], rx symbol i = x[start + (r0 + i) step] of its row, strides in elements.
int lagcorr_check(int64_t len, int64_t n_lags, int a_dtype, int b_dtype, int quant_levels, int64_t *n_out, int64_t *first_lag);   // host-only
size_t lagcorr_scratch_bytes(int64_t len, int64_t n_lags);                                                                        // host-only
int lagcorr_launch(const void *a_dev, int a_dtype, const void *b_dev, int b_dtype, int64_t len, int64_t n_lags, int quant_levels, void *scratch_dev, void *r_dev,
                   double *e_dev, hipStream_t s);
int symcount_check(int tx_dtype, int64_t tx_stride, int64_t t0, int x_dtype, int64_t x_stride, int64_t start, int64_t step, int64_t r0, int64_t n, int64_t nrow, int mode,
                   int levels, int kphase);   // host-only
int symcount_launch(const void *tx_dev, int tx_dtype, int64_t tx_stride, int64_t t0, const void *x_dev, int x_dtype, int64_t x_stride, int64_t start, int64_t step,
                    int64_t r0, int64_t n, int64_t nrow, int mode, int levels, int kphase, int64_t *counts_dev, hipStream_t s);

// ---- pulse shaping and matched filtering over rows (pulse.hip): lfilter(b, 1, upsample(s, ns)) and lfilter(b, 1, x)[start::step] per row, from rest; the plans and
// the per-thread functions are pulse_core.hpp ----
// The handle (a HandleBase of kind H_PULSE) owns the real float64 taps (uploaded on first use); skdsp_destroy frees it.  Strides in elements; x and y must not overlap.
int pulse_create(const double *b, int ntaps, int dtype, HandleBase **out);                                                              // host-only
int pulse_mf_out_len(int64_t n, int64_t start, int64_t step, int64_t *n_out);                                                            // host-only
int pulse_shape_check(HandleBase *h, int64_t n, int64_t nrow, int64_t ns, int64_t x_stride, int64_t y_stride);                           // host-only
int pulse_shape_launch(HandleBase *h, const void *x_dev, int64_t n, int64_t nrow, int64_t ns, int64_t x_stride, int64_t y_stride, int has_scale, double scale,
                       void *y_dev, hipStream_t s);
int pulse_mf_check(HandleBase *h, int64_t n, int64_t nrow, int64_t start, int64_t step, int64_t x_stride, int64_t y_stride);             // host-only
int pulse_mf_launch(HandleBase *h, const void *x_dev, int64_t n, int64_t nrow, int64_t start, int64_t step, int64_t x_stride, int64_t y_stride, void *y_dev,
                    hipStream_t s);

// ---- carrier phase tracking and its impairment helpers over rows (carrier.hip): synchronization.DD_carrier_sync / phase_step / time_step; the step, the plans and
// the per-thread functions are carrier_core.hpp ----
// family 0 QAM, 1 MPSK; symbol k of a row is element start + k step; outputs: bit 0 z_prime, 1 a_hat, 2 e_phi, 3 theta_h (an output that is not selected is not
// touched and may be null); y_stride serves the four outputs.  gains_dev: null (k1, k2 serve every row) or [nrow][2]; r_dev: the rows' 1 / scale (QAM; symscale_launch).
// inv_sqrt2, tab_re_host, tab_im_host: the host's 1 / np.sqrt(2) and exp(1j 2 pi a / M), read for MPSK 4 and MPSK above 4.  No handle.
int carrier_check(int family, int mod, int type, int dtype, int outputs, int64_t n, int64_t nrow, int64_t start, int64_t step, int64_t x_stride, int64_t y_stride);   // host-only
int carrier_launch(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, int dtype, int family, int mod, int type, int open_loop,
                   double k1, double k2, const double *gains_dev, const double *r_dev, double inv_sqrt2, const double *tab_re_host, const double *tab_im_host, int outputs,
                   void *z_dev, void *a_dev, double *e_dev, double *t_dev, int64_t y_stride, hipStream_t s);
// mode 0 time_step (shift / shifts_dev: t_step, one or [nrow] int64), mode 1 phase_step ((c, d) / factors_dev: exp(1j p_step), one or [nrow][2])
int impair_check(int mode, int dtype, int64_t n, int64_t n_out, int64_t nrow, int64_t ns, int64_t n_step, int64_t x_stride, int64_t y_stride);   // host-only
int impair_launch(int mode, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int dtype, int64_t ns, int64_t n_step, int64_t shift, const int64_t *shifts_dev,
                  double c, double d, const double *factors_dev, void *y_dev, int64_t n_out, int64_t y_stride, hipStream_t s);

// ---- symbol timing recovery over rows (timing.hip): synchronization.NDA_symb_sync; the recipe, the plans and the per-thread functions are timing_core.hpp ----
// n: the samples of a row's frame, x[row, start ... start + n - 1]; outputs: bit 0 zz, 1 e_tau (an output that is not selected is not touched and may be null); cap: the
// elements a row's outputs may take (y_stride >= cap apart); counts_dev[row]: the reference's output length, also where it exceeds cap.  Nothing behind
// min(counts[row], cap) elements of a row is written.  gains_dev: null (k1, k2 serve every row) or [nrow][2].  rot_host: Ns real parts, then Ns imaginary parts, of
// the host's np.exp(-1j 2 pi / Ns kk); inv_ns, inv_len, k_eps: the host's 1 / float(Ns), 1.0 / (2L + 1), -1 / (2 np.pi).  normalize: zz /= np.std(zz) per row, by a second
// kernel; for complex64 samples that one reads the raw symbols from scratch_dev (nda_scratch_bytes, 16-byte aligned), in float64.  No handle.
int nda_check(int ns, int L, int iord, int dtype, int outputs, int64_t n, int64_t nrow, int64_t start, int64_t x_stride, int64_t y_stride, int64_t cap);   // host-only
size_t nda_scratch_bytes(int dtype, int outputs, int normalize, int64_t nrow, int64_t cap);                                                               // host-only
int nda_launch(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int dtype, int ns, int L, int iord, double k1, double k2, const double *gains_dev,
               const double *rot_host, double inv_ns, double inv_len, double k_eps, int outputs, int normalize, int64_t cap, void *scratch_dev, void *z_dev, double *e_dev,
               int64_t *counts_dev, int64_t y_stride, hipStream_t s);

}  // namespace skdsp
