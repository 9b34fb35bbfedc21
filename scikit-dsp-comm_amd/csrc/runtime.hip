// runtime.hip -- what every entry point of libskdsp_hip.so stands on (see include/skdsp.h): error text, the slots (one
// Context per bound GPU / stream), failures reported after the fact, the options table, init / shutdown, the grow-only
// workspaces, the engine record of skdsp_debug_path, and the plain memory / sync / timer calls.
#include "api_internal.hpp"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace skdsp {

static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char *what, const char *file, int line)
{
    set_error("HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return SKDSP_ERR_NOMEM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return SKDSP_ERR_NODEVICE;
    return SKDSP_ERR_HIP;
}

// the device behind dev_mem.hpp
int dev_alloc(void **out, size_t bytes)
{
    SK_HIP(hipMalloc(out, bytes));
    return SKDSP_OK;
}
void dev_free(void *p) { (void)hipFree(p); }
int dev_copy_in(void *dst, const void *src, size_t bytes)
{
    SK_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return SKDSP_OK;
}
int dev_sync(void *stream)
{
    SK_HIP(hipStreamSynchronize((hipStream_t)stream));
    return SKDSP_OK;
}

static Context g_slots[kMaxSlots];
static int g_nslots = 0;            // bound slots; slot 0 is bound by the first call that needs a device
static std::mutex g_slots_mu;
static thread_local int t_slot = 0;

Context &ctx() { return g_slots[t_slot]; }
Context &ctx_of(int slot) { return g_slots[slot]; }
int slot_count() { return g_nslots; }
int select_slot(int slot)
{
    SK_CHECK(slot >= 0 && slot < kMaxSlots && g_slots[slot].ready, SKDSP_ERR_BADARG, "select_slot: slot %d is not bound", slot);
    t_slot = slot;
    SK_HIP(hipSetDevice(g_slots[slot].device));
    return SKDSP_OK;
}

// ---- failures reported after the fact (bounded device-side waits) ------------------------------
unsigned *async_err_dev(int which)
{
    Context &c = ctx();
    if (!c.async_err) {
        if (hipHostMalloc((void **)&c.async_err, kAsyncErrWords * sizeof(unsigned), hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            c.async_err = nullptr;
            return nullptr;
        }
        for (int i = 0; i < kAsyncErrWords; ++i) c.async_err[i] = 0;
    }
    unsigned *dev = nullptr;
    if (hipHostGetDevicePointer((void **)&dev, c.async_err, 0) != hipSuccess) return nullptr;
    return dev + which;
}

int async_err_check(Context &c)
{
    if (!c.async_err) return SKDSP_OK;
    volatile unsigned *w = c.async_err;
    if (w[kAsyncErrHalo]) {
        // The persistent launch of a sharded FIR step polled for seconds and gave up: the RCCL receive did not run beside
        // it on this system.  Tile 0 of that step was not written from a valid halo.  The two-launch form is used from now
        // on; the caller repeats the step -- COLLECTIVELY, on every rank (each step is one send/recv pair).
        w[kAsyncErrHalo] = 0;
        opt().shard_two_launches = 1;
        set_error("fir_filter_shard: a sharded step since the last synchronisation gave up waiting for its halo inside the filter "
                  "launch (the first tile of that step is invalid); switched to the two-launch form (option shard_two_launches) -- "
                  "repeat the step on every rank");
        return SKDSP_ERR_RCCL;
    }
    if (w[kAsyncErrIirLookback]) {
        w[kAsyncErrIirLookback] = 0;
        set_error("iir: a look-back poll of a single-pass scan launched since the last synchronisation timed out (the results of "
                  "that call are invalid; option iir_two_pass = 1 selects the two-pass scan)");
        return SKDSP_ERR_HIP;
    }
    return SKDSP_OK;
}

// stream sync of the calling slot + the deferred failures of what ran on it
int sync_checked()
{
    SK_HIP(hipStreamSynchronize(ctx().stream));
    return async_err_check(ctx());
}

// ---- options: environment read once, skdsp_set_option afterwards ----------------------------
namespace {
struct OptEntry { const char *name; int Options::*field; };
const OptEntry kOptTable[] = {
    {"device", &Options::device}, {"fir_algo", &Options::fir_algo}, {"dn_no_ols", &Options::dn_no_ols},
    {"fir_mm", &Options::fir_mm}, {"fir_bx", &Options::fir_bx}, 
    
    {"ols_reserve", &Options::ols_reserve}, {"ols_walk", &Options::ols_walk},{"fir_bx_t16", &Options::fir_bx_t16}, {"fir_bank_per", &Options::fir_bank_per}, {"ols_keep_overlap", &Options::ols_keep_overlap}, {"fir_dn_fold", &Options::fir_dn_fold}, {"fir_up_rep", &Options::fir_up_rep}, {"iir_seq", &Options::iir_seq}, {"psd_f32_image", &Options::psd_f32_image}, {"iir_up_jump", &Options::iir_up_jump}, {"iir_dn_t96", &Options::iir_dn_t96}, {"iir_up_lean", &Options::iir_up_lean}, {"iir_planar", &Options::iir_planar}, 
    {"iir_dn_full", &Options::iir_dn_full}, {"iir_no_mfma", &Options::iir_no_mfma}, 
    {"iir_two_pass", &Options::iir_two_pass}, {"iir_par", &Options::iir_par}, {"iir_par_v32", &Options::iir_par_v32}, {"iir_up_fused", &Options::iir_up_fused}, {"fir_up_ols_min", &Options::fir_up_ols_min}, {"fir_updn_fused", &Options::fir_updn_fused}, {"fir_up4k", &Options::fir_up4k}, {"fir_up4k_group", &Options::fir_up4k_group}, {"fir_up4k_staged", &Options::fir_up4k_staged}, {"fir_up2k", &Options::fir_up2k}, {"fir_dn4k", &Options::fir_dn4k}, {"fir_up_pair", &Options::fir_up_pair}, {"fir_up_rows_min", &Options::fir_up_rows_min}, {"iir_dn_compact", &Options::iir_dn_compact}, 
    {"shard_two_launches", &Options::shard_two_launches}, {"shard_probe", &Options::shard_probe}, {"shard_halo_state", &Options::shard_halo_state},
    {"shard_self_halo", &Options::shard_self_halo}, {"dist_force_comm", &Options::dist_force_comm},
    {"host_chunk_log2", &Options::host_chunk_log2}, {"host_pipeline", &Options::host_pipeline}, {"host_multi_slot", &Options::host_multi_slot}, {"pulse_mf_variant", &Options::pulse_mf_variant},
};
int parse_opt(const char *name, const char *v)
{
    if (!strcmp(name, "fir_algo")) {
        if (!strcmp(v, "direct")) return SKDSP_FIR_DIRECT;
        if (!strcmp(v, "ols")) return SKDSP_FIR_OLS;
        if (!strcmp(v, "auto")) return SKDSP_FIR_AUTO;
    }
    if (!*v) return 1;  // SKDSP_X= (set, empty) switches X on
    return atoi(v);
}
Options options_from_env()
{
    Options o;
    for (const OptEntry &e : kOptTable) {
        char key[64] = "SKDSP_";
        size_t k = 6;
        for (const char *p = e.name; *p && k + 1 < sizeof(key); ++p) key[k++] = (char)toupper((unsigned char)*p);
        key[k] = 0;
        if (const char *v = getenv(key)) o.*(e.field) = parse_opt(e.name, v);
    }
    return o;
}
}  // namespace

Options &opt()
{
    static Options o = options_from_env();
    return o;
}

static int init_locked(int device)
{
    Context &c = ctx();
    if (c.ready) {
        SK_CHECK(device < 0 || device == c.device, SKDSP_ERR_BADARG,
                 "skdsp_init: slot %d is already bound to device %d", c.slot, c.device);
        return SKDSP_OK;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_error("no HIP device available (hipGetDeviceCount -> %d, %s): the MI355X path has no CPU fallback",
                  ndev, e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        (void)hipGetLastError();
        return SKDSP_ERR_NODEVICE;
    }
    if (device < 0) device = 0;
    SK_CHECK(device < ndev, SKDSP_ERR_NODEVICE, "skdsp_init: device %d out of range (%d visible)", device, ndev);
    SK_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    SK_HIP(hipGetDeviceProperties(&prop, device));
    c.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    SK_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    SK_HIP(hipEventCreate(&c.ev_start));
    SK_HIP(hipEventCreate(&c.ev_stop));
    c.device = device;
    c.slot = t_slot;
    c.ready = true;
    {
        std::lock_guard<std::mutex> lk(g_slots_mu);
        if (g_nslots < t_slot + 1) g_nslots = t_slot + 1;
    }
    return SKDSP_OK;
}

int ensure_init()
{
    Context &c = ctx();
    if (c.ready) {
        // several slots: make sure this thread's HIP device is the slot's (threads start on device 0)
        if (g_nslots > 1) SK_HIP(hipSetDevice(c.device));
        return SKDSP_OK;
    }
    std::lock_guard<std::mutex> lk(c.mu);
    return init_locked(opt().device);
}

int ws_reserve(int slot, size_t bytes, void **out)
{
    Context &c = ctx();
    if (bytes > c.ws_bytes[slot]) {
        if (c.ws[slot]) {
            SK_HIP(hipStreamSynchronize(c.stream));
            SK_HIP(hipFree(c.ws[slot]));
            c.ws[slot] = nullptr;
            c.ws_bytes[slot] = 0;
        }
        size_t cap = bytes + bytes / 8 + 4096;
        SK_HIP(hipMalloc(&c.ws[slot], cap));
        c.ws_bytes[slot] = cap;
    }
    *out = c.ws[slot];
    return SKDSP_OK;
}

}  // namespace skdsp

using namespace skdsp;

static thread_local char g_path[256];
void skdsp::note_path(const char *engine)
{
    const size_t len = strlen(g_path), add = strlen(engine);
    if (len >= add && strcmp(g_path + len - add, engine) == 0 && (len == add || g_path[len - add - 1] == ',')) return;   // (the same engine again)
    if (add == 0) return;
    if (len + add + 2 >= sizeof(g_path)) return;
    if (len) g_path[len] = ',';
    memcpy(g_path + len + (len ? 1 : 0), engine, add + 1);
}

extern "C" {

const char *skdsp_last_error(void) { return g_err; }
int skdsp_debug_path(char *buf, int cap, int clear)
{
    if (buf && cap > 0) {
        strncpy(buf, g_path, (size_t)cap - 1);
        buf[cap - 1] = 0;
    }
    if (clear) g_path[0] = 0;
    return SKDSP_OK;
}
const char *skdsp_version(void) { return "skdsp-hip 0.1.0 (gfx950)"; }

int skdsp_init(int device)
{
    std::lock_guard<std::mutex> lk(ctx().mu);
    return init_locked(device);
}

static int shutdown_slot(Context &c)
{
    std::lock_guard<std::mutex> lk(c.mu);
    if (!c.ready) return SKDSP_OK;
    (void)hipSetDevice(c.device);
    (void)hipStreamSynchronize(c.stream);
    pipe_free(c);
    for (int i = 0; i < 4; ++i) {
        if (c.ws[i]) (void)hipFree(c.ws[i]);
        c.ws[i] = nullptr;
        c.ws_bytes[i] = 0;
    }
    (void)hipEventDestroy(c.ev_start);
    (void)hipEventDestroy(c.ev_stop);
    if (c.comm_stream) {
        (void)hipStreamSynchronize(c.comm_stream);
        (void)hipEventDestroy(c.ev_in);
        (void)hipEventDestroy(c.ev_halo);
        if (c.halo_flag) (void)hipFree(c.halo_flag);
        c.halo_flag = nullptr;
        (void)hipStreamDestroy(c.comm_stream);
        c.comm_stream = nullptr;
        c.ev_in = c.ev_halo = nullptr;
    }
    (void)hipStreamDestroy(c.stream);
    if (c.async_err) (void)hipHostFree(c.async_err);
    c.async_err = nullptr;
    c.ready = false;
    c.device = -1;
    return SKDSP_OK;
}

int skdsp_shutdown(void)
{
    for (int s = kMaxSlots - 1; s >= 0; --s) (void)shutdown_slot(ctx_of(s));
    std::lock_guard<std::mutex> lk(g_slots_mu);
    g_nslots = 0;
    return SKDSP_OK;
}

int skdsp_init_devices(const int *devices, int ndev)
{
    SK_CHECK(devices && ndev >= 1 && ndev <= kMaxSlots, SKDSP_ERR_BADARG, "init_devices: 1..%d devices", kMaxSlots);
    const int home = t_slot;
    int rc = SKDSP_OK;
    for (int s = 0; s < ndev && !rc; ++s) {
        t_slot = s;
        std::lock_guard<std::mutex> lk(ctx().mu);
        rc = init_locked(devices[s]);
    }
    t_slot = home;
    if (!rc && ctx().ready) SK_HIP(hipSetDevice(ctx().device));
    return rc;
}

int skdsp_slot_count(void) { return slot_count(); }

int skdsp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int skdsp_device_info(char *name, int name_cap, int *compute_units, int64_t *hbm_bytes, int *clock_khz)
{
    API_BEGIN;
    hipDeviceProp_t prop;
    SK_HIP(hipGetDeviceProperties(&prop, ctx().device));
    if (name && name_cap > 0) {
        // (boxes without the marketing-name table -- /opt/amdgpu/share/libdrm/amdgpu.ids -- report an empty name: the architecture string then stands alone)
        if (prop.name[0]) snprintf(name, (size_t)name_cap, "%s (%s)", prop.name, prop.gcnArchName);
        else snprintf(name, (size_t)name_cap, "%s, %d CUs", prop.gcnArchName, prop.multiProcessorCount);
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    if (clock_khz) *clock_khz = prop.clockRate;
    return SKDSP_OK;
}

int skdsp_malloc(void **dptr, int64_t bytes)
{
    API_BEGIN;
    SK_CHECK(dptr && bytes >= 0, SKDSP_ERR_BADARG, "skdsp_malloc: bad arguments");
    SK_HIP(hipMalloc(dptr, (size_t)(bytes > 0 ? bytes : 1)));
    return SKDSP_OK;
}
int skdsp_free(void *dptr)
{
    API_BEGIN;
    if (dptr) {
        SK_HIP(hipStreamSynchronize(ctx().stream));
        SK_HIP(hipFree(dptr));
    }
    return SKDSP_OK;
}
// page-locked host memory for result arrays (the Python layer recycles these blocks: _ffi.PinnedPool)
int skdsp_host_alloc(void **hptr, int64_t bytes)
{
    API_BEGIN;
    SK_CHECK(hptr && bytes > 0, SKDSP_ERR_BADARG, "host_alloc: bad arguments");
    SK_HIP(hipHostMalloc(hptr, (size_t)bytes, hipHostMallocPortable));
    return SKDSP_OK;
}
int skdsp_host_free(void *hptr)
{
    if (hptr) SK_HIP(hipHostFree(hptr));
    return SKDSP_OK;
}
int skdsp_memcpy_h2d(void *dst, const void *src, int64_t bytes)
{
    API_BEGIN;
    if (bytes > 0) SK_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, ctx().stream));
    return sync_checked();
}
int skdsp_memcpy_d2h(void *dst, const void *src, int64_t bytes)
{
    API_BEGIN;
    if (bytes > 0) SK_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, ctx().stream));
    return sync_checked();
}
int skdsp_memcpy_d2d(void *dst, const void *src, int64_t bytes)
{
    API_BEGIN;
    if (bytes > 0) SK_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, ctx().stream));
    return SKDSP_OK;
}
int skdsp_memset(void *dst, int value, int64_t bytes)
{
    API_BEGIN;
    if (bytes > 0) SK_HIP(hipMemsetAsync(dst, value, (size_t)bytes, ctx().stream));
    return SKDSP_OK;
}
int skdsp_sync(void)
{
    API_BEGIN;
    return sync_checked();
}
int skdsp_timer_start(void)
{
    API_BEGIN;
    SK_HIP(hipEventRecord(ctx().ev_start, ctx().stream));
    return SKDSP_OK;
}
int skdsp_timer_stop(float *ms)
{
    API_BEGIN;
    SK_HIP(hipEventRecord(ctx().ev_stop, ctx().stream));
    SK_HIP(hipEventSynchronize(ctx().ev_stop));
    float t = 0.f;
    SK_HIP(hipEventElapsedTime(&t, ctx().ev_start, ctx().ev_stop));
    if (ms) *ms = t;
    ctx().last_timer_ms = (double)t;
    return async_err_check(ctx());
}
double skdsp_last_kernel_ms(void) { return ctx().ready ? ctx().last_timer_ms : -1.0; }
int skdsp_fill_noise_dev(void *x_dev, int64_t n, int dtype, uint64_t seed, int64_t first_index)
{
    API_BEGIN;
    SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "fill_noise: bad dtype %d", dtype);
    return fill_noise_launch(x_dev, n, dtype, seed, first_index, ctx().stream);
}

int skdsp_set_option(const char *name, int value)
{
    SK_CHECK(name, SKDSP_ERR_BADARG, "set_option: null name");
    for (const OptEntry &e : kOptTable)
        if (!strcmp(e.name, name)) {
            opt().*(e.field) = value;
            return SKDSP_OK;
        }
    SK_CHECK(false, SKDSP_ERR_BADARG, "set_option: unknown option '%s'", name);
}

int skdsp_get_option(const char *name, int *value)
{
    SK_CHECK(name && value, SKDSP_ERR_BADARG, "get_option: null argument");
    for (const OptEntry &e : kOptTable)
        if (!strcmp(e.name, name)) {
            *value = opt().*(e.field);
            return SKDSP_OK;
        }
    SK_CHECK(false, SKDSP_ERR_BADARG, "get_option: unknown option '%s'", name);
}

int skdsp_set_wide_output(skdsp_handle hh, int on)
{
    HandleBase *b = reinterpret_cast<HandleBase *>(hh);
    SK_CHECK(b && (b->kind == H_FIR || b->kind == H_IIR), SKDSP_ERR_BADARG, "set_wide_output: not a filter handle");
    std::lock_guard<std::mutex> lk(b->mu);
    b->wide_out = on != 0;
    return SKDSP_OK;
}

int skdsp_destroy(skdsp_handle hh)
{
    if (!hh) return SKDSP_OK;
    HandleBase *b = reinterpret_cast<HandleBase *>(hh);
    if (ctx().ready) {
        std::lock_guard<std::mutex> lk(ctx().mu);
        (void)hipStreamSynchronize(ctx().stream);
        delete b;
    } else {
        delete b;
    }
    return SKDSP_OK;
}

}  // extern "C"
