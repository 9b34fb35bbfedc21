"""ctypes binding of libskdsp_hip.so (the C ABI declared in include/skdsp.h).

No PyTorch, no CPU fallback: if the library or a HIP device is missing the calls
raise -- the product path must fail loudly rather than silently run elsewhere.
"""
import ctypes
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libskdsp_hip.so"

F32, C64, F64, C128 = 0, 1, 2, 3
FIR_AUTO, FIR_DIRECT, FIR_OLS = 0, 1, 2

_NP_OF = {F32: np.float32, C64: np.complex64, F64: np.float64, C128: np.complex128}
_CODE_OF = {np.dtype(np.float32): F32, np.dtype(np.complex64): C64, np.dtype(np.float64): F64,
            np.dtype(np.complex128): C128}

# every symbol include/skdsp.h declares (tests check the built library exports all of them)
SYMBOLS = [
    "skdsp_init", "skdsp_shutdown", "skdsp_debug_path", "skdsp_device_count", "skdsp_device_info", "skdsp_last_error", "skdsp_version",
    "skdsp_set_option", "skdsp_get_option", "skdsp_init_devices", "skdsp_slot_count", "skdsp_host_chunk_plan",
    "skdsp_host_alloc", "skdsp_host_free", "skdsp_malloc", "skdsp_free", "skdsp_memcpy_h2d", "skdsp_memcpy_d2h", "skdsp_memcpy_d2d", "skdsp_memset",
    "skdsp_sync", "skdsp_timer_start", "skdsp_timer_stop", "skdsp_last_kernel_ms", "skdsp_fill_noise_dev",
    "skdsp_fir_create", "skdsp_fir_set_algo", "skdsp_fir_get_algo", "skdsp_fir_filter", "skdsp_fir_filter_dev",
    "skdsp_fir_filter_rows", "skdsp_fir_filter_rows_dev", "skdsp_fir_filter_sharded", "skdsp_fir_bank_create", "skdsp_fir_bank_dev",
    "skdsp_fir_up", "skdsp_fir_up_dev", "skdsp_fir_dn", "skdsp_fir_dn_dev", "skdsp_fir_updn", "skdsp_fir_updn_dev",
    "skdsp_sos_create", "skdsp_tf_create", "skdsp_tf2sos", "skdsp_iir_filter", "skdsp_iir_filter_dev", "skdsp_iir_up",
    "skdsp_iir_up_dev", "skdsp_iir_dn", "skdsp_iir_dn_dev", "skdsp_iir_state_len", "skdsp_iir_filter_state_dev",
    "skdsp_iir_filter_rows", "skdsp_iir_filter_rows_dev", "skdsp_sos_par_info", "skdsp_iir_sequential",
    "skdsp_sos_filter", "skdsp_sos_up", "skdsp_sos_dn",
    "skdsp_upsample", "skdsp_upsample_dev", "skdsp_downsample", "skdsp_downsample_dev", "skdsp_set_wide_output", "skdsp_destroy",
    "skdsp_farrow_len", "skdsp_farrow_dev", "skdsp_farrow", "skdsp_psd_dev", "skdsp_psd",
    "skdsp_viterbi_create", "skdsp_viterbi_out_len", "skdsp_viterbi_reset", "skdsp_viterbi_decode", "skdsp_viterbi_decode_dev",
    "skdsp_viterbi_decode_rows", "skdsp_viterbi_decode_rows_dev",
    "skdsp_blockcode_create", "skdsp_blockcode_encode", "skdsp_blockcode_encode_dev", "skdsp_blockcode_decode", "skdsp_blockcode_decode_dev",
    "skdsp_convcode_create", "skdsp_convcode_encode_rows", "skdsp_convcode_encode_rows_dev", "skdsp_puncture_out_len", "skdsp_depuncture_out_len",
    "skdsp_puncture_rows", "skdsp_puncture_rows_dev", "skdsp_depuncture_rows", "skdsp_depuncture_rows_dev", "skdsp_bit_count_rows", "skdsp_bit_count_rows_dev",
    "skdsp_gray_map_rows", "skdsp_gray_map_rows_dev", "skdsp_qam_scale_rows", "skdsp_qam_scale_rows_dev", "skdsp_qam_demap_rows", "skdsp_qam_demap_rows_dev",
    "skdsp_mpsk_demap_rows", "skdsp_mpsk_demap_rows_dev",
    "skdsp_awgn_rows_dev", "skdsp_awgn_bits_rows_dev", "skdsp_awgn_sigma_rows_dev", "skdsp_random_bits_rows_dev", "skdsp_pn_rows_dev",
    "skdsp_ofdm_tx_rows", "skdsp_ofdm_tx_rows_dev", "skdsp_ofdm_rx_rows", "skdsp_ofdm_rx_rows_dev", "skdsp_ofdm_equalize_rows", "skdsp_ofdm_equalize_rows_dev",
    "skdsp_lag_corr_len", "skdsp_lag_corr", "skdsp_lag_corr_dev", "skdsp_sym_count_rows", "skdsp_sym_count_rows_dev",
    "skdsp_pulse_create", "skdsp_pulse_mf_out_len", "skdsp_pulse_shape_rows", "skdsp_pulse_shape_rows_dev", "skdsp_pulse_mf_rows", "skdsp_pulse_mf_rows_dev",
    "skdsp_carrier_rows", "skdsp_carrier_rows_dev", "skdsp_time_step_rows_dev", "skdsp_phase_step_rows_dev", "skdsp_nda_rows", "skdsp_nda_rows_dev",
    "skdsp_dist_unique_id", "skdsp_dist_init", "skdsp_dist_shutdown", "skdsp_dist_comm_count", "skdsp_dist_barrier",
    "skdsp_dist_allreduce_max", "skdsp_dist_allreduce_sum", "skdsp_dist_sendrecv", "skdsp_dist_allgather", "skdsp_dist_halo_exchange", "skdsp_fir_filter_shard_dev",
]

_lib = None
_lock = threading.Lock()


class SkdspError(RuntimeError):
    pass


def lib_path():
    # SKDSP_LIB: developer override to A/B an alternative build of the same library
    return os.environ.get("SKDSP_LIB") or os.path.join(_HERE, LIB_NAME)


def load():
    """dlopen the library and declare prototypes.  Does NOT touch the GPU."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            raise SkdspError(
                "%s not found next to the package: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C scikit-dsp-comm_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
        L = ctypes.CDLL(path)
        vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        pvp = ctypes.POINTER(ctypes.c_void_p)
        L.skdsp_last_error.restype = ctypes.c_char_p
        L.skdsp_version.restype = ctypes.c_char_p
        L.skdsp_init.argtypes = [ci]
        if hasattr(L, "skdsp_debug_path"):   # (absent from older builds of the library that SKDSP_LIB may point at for A/B timing)
            L.skdsp_debug_path.argtypes = [ctypes.c_char_p, ci, ci]
        L.skdsp_init_devices.argtypes = [ctypes.POINTER(ci), ci]
        p64 = ctypes.POINTER(i64)
        L.skdsp_host_chunk_plan.argtypes = [i64, ci, ci, i64, ci, i64, p64, p64, p64, p64, p64, p64]
        L.skdsp_set_option.argtypes = [ctypes.c_char_p, ci]
        L.skdsp_get_option.argtypes = [ctypes.c_char_p, ctypes.POINTER(ci)]
        L.skdsp_device_info.argtypes = [ctypes.c_char_p, ci, ctypes.POINTER(ci), ctypes.POINTER(i64), ctypes.POINTER(ci)]
        L.skdsp_host_alloc.argtypes = [pvp, i64]
        L.skdsp_host_free.argtypes = [vp]
        L.skdsp_malloc.argtypes = [pvp, i64]
        L.skdsp_free.argtypes = [vp]
        for f in (L.skdsp_memcpy_h2d, L.skdsp_memcpy_d2h, L.skdsp_memcpy_d2d):
            f.argtypes = [vp, vp, i64]
        L.skdsp_memset.argtypes = [vp, ci, i64]
        L.skdsp_timer_stop.argtypes = [ctypes.POINTER(ctypes.c_float)]
        L.skdsp_fill_noise_dev.argtypes = [vp, i64, ci, ctypes.c_uint64, i64]
        L.skdsp_fir_create.argtypes = [vp, ci, ci, ci, pvp]
        L.skdsp_fir_set_algo.argtypes = [vp, ci]
        L.skdsp_fir_get_algo.argtypes = [vp, i64, ctypes.POINTER(ci)]
        L.skdsp_fir_filter.argtypes = [vp, vp, i64, vp]
        L.skdsp_fir_filter_sharded.argtypes = [vp, vp, i64, vp, ci]
        L.skdsp_fir_filter_dev.argtypes = [vp, vp, i64, i64, vp]
        L.skdsp_fir_filter_rows.argtypes = [vp, vp, i64, i64, vp]
        L.skdsp_fir_filter_rows_dev.argtypes = [vp, vp, i64, i64, i64, i64, vp]
        L.skdsp_fir_up.argtypes = [vp, vp, i64, ci, vp]
        L.skdsp_fir_up_dev.argtypes = [vp, vp, i64, i64, ci, vp]
        L.skdsp_fir_dn.argtypes = [vp, vp, i64, ci, vp]
        L.skdsp_fir_dn_dev.argtypes = [vp, vp, i64, i64, ci, vp]
        L.skdsp_fir_updn.argtypes = [vp, vp, i64, ci, ci, vp]
        L.skdsp_fir_updn_dev.argtypes = [vp, vp, i64, i64, ci, ci, vp]
        L.skdsp_sos_create.argtypes = [vp, ci, ci, pvp]
        L.skdsp_tf_create.argtypes = [vp, ci, vp, ci, ci, pvp]
        L.skdsp_tf2sos.argtypes = [vp, ci, vp, ci, vp, ctypes.POINTER(ci)]
        L.skdsp_iir_filter.argtypes = [vp, vp, i64, vp]
        L.skdsp_iir_filter_dev.argtypes = [vp, vp, i64, vp]
        L.skdsp_iir_state_len.argtypes = [vp, ctypes.POINTER(ci)]
        L.skdsp_iir_filter_state_dev.argtypes = [vp, vp, i64, vp, vp, vp]
        L.skdsp_iir_filter_rows.argtypes = [vp, vp, i64, i64, vp]
        L.skdsp_iir_filter_rows_dev.argtypes = [vp, vp, i64, i64, i64, i64, vp]
        L.skdsp_sos_par_info.argtypes = [vp, ci, vp, ctypes.POINTER(ci)]
        if hasattr(L, "skdsp_iir_sequential"):
            L.skdsp_iir_sequential.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_double)]
        L.skdsp_iir_up.argtypes = [vp, vp, i64, ci, vp]
        L.skdsp_iir_up_dev.argtypes = [vp, vp, i64, ci, vp]
        L.skdsp_iir_dn.argtypes = [vp, vp, i64, ci, vp]
        L.skdsp_iir_dn_dev.argtypes = [vp, vp, i64, ci, vp]
        L.skdsp_sos_filter.argtypes = [vp, vp, i64, vp]
        L.skdsp_sos_up.argtypes = [vp, vp, i64, ci, vp]
        L.skdsp_sos_dn.argtypes = [vp, vp, i64, ci, vp]
        L.skdsp_last_kernel_ms.restype = ctypes.c_double
        L.skdsp_upsample.argtypes = [vp, i64, ci, ci, vp]
        L.skdsp_upsample_dev.argtypes = [vp, i64, ci, ci, ctypes.c_double, vp]
        L.skdsp_downsample.argtypes = [vp, i64, ci, ci, ci, vp]
        L.skdsp_downsample_dev.argtypes = [vp, i64, ci, ci, ci, vp]
        L.skdsp_destroy.argtypes = [vp]
        if hasattr(L, "skdsp_farrow"):
            dbl = ctypes.c_double
            L.skdsp_farrow_len.argtypes = [i64, dbl, dbl, p64]
            L.skdsp_farrow_dev.argtypes = [vp, i64, ci, dbl, dbl, ci, dbl, i64, i64, ci, vp]
            L.skdsp_farrow.argtypes = [vp, i64, ci, dbl, dbl, ci, dbl, ci, vp]
        if hasattr(L, "skdsp_psd"):
            pd = ctypes.POINTER(ctypes.c_double)
            L.skdsp_psd_dev.argtypes = [vp, i64, ci, pd, ci, ci, i64, i64, vp]
            L.skdsp_psd.argtypes = [vp, i64, ci, pd, ci, ci, i64, i64, vp]
        if hasattr(L, "skdsp_fir_bank_create"):
            L.skdsp_fir_bank_create.argtypes = [vp, ci, ci, p64, ci, ci, ci, pvp]
            L.skdsp_fir_bank_dev.argtypes = [vp, vp, i64, vp, i64]
        if hasattr(L, "skdsp_viterbi_create"):
            L.skdsp_viterbi_create.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, ci, pvp]
            L.skdsp_viterbi_out_len.argtypes = [vp, i64, p64]
            L.skdsp_viterbi_reset.argtypes = [vp]
            L.skdsp_viterbi_decode.argtypes = [vp, vp, i64, ci, ci, ci, vp]
            L.skdsp_viterbi_decode_dev.argtypes = [vp, vp, i64, ci, ci, ci, vp]
            L.skdsp_viterbi_decode_rows.argtypes = [vp, vp, i64, i64, ci, ci, ci, vp]
            L.skdsp_viterbi_decode_rows_dev.argtypes = [vp, vp, i64, i64, ci, ci, ci, vp]
        if hasattr(L, "skdsp_blockcode_create"):
            L.skdsp_blockcode_create.argtypes = [ci, ci, vp, vp, vp, pvp]
            for name in ("encode", "encode_dev", "decode", "decode_dev"):
                getattr(L, "skdsp_blockcode_" + name).argtypes = [vp, vp, i64, vp]
        if hasattr(L, "skdsp_convcode_create"):
            u64 = ctypes.c_uint64
            L.skdsp_convcode_create.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, pvp]
            L.skdsp_convcode_encode_rows.argtypes = L.skdsp_convcode_encode_rows_dev.argtypes = [vp, vp, i64, i64, vp, i64, vp, vp]
            L.skdsp_puncture_out_len.argtypes = L.skdsp_depuncture_out_len.argtypes = [i64, u64, u64, ci, p64]
            L.skdsp_puncture_rows.argtypes = L.skdsp_puncture_rows_dev.argtypes = [vp, i64, i64, ci, u64, u64, ci, vp]
            L.skdsp_depuncture_rows.argtypes = L.skdsp_depuncture_rows_dev.argtypes = [vp, i64, i64, ci, u64, u64, ci, vp, vp]
            L.skdsp_bit_count_rows.argtypes = L.skdsp_bit_count_rows_dev.argtypes = [vp, i64, vp, i64, i64, i64, ci, vp]
        if hasattr(L, "skdsp_gray_map_rows"):
            dbl = ctypes.c_double
            L.skdsp_gray_map_rows.argtypes = [vp, i64, i64, ci, ci, vp, vp, ci, ci, vp]
            L.skdsp_gray_map_rows_dev.argtypes = [vp, i64, i64, i64, ci, ci, vp, vp, ci, ci, vp, i64]
            L.skdsp_qam_scale_rows.argtypes = L.skdsp_qam_scale_rows_dev.argtypes = [vp, i64, i64, i64, i64, i64, ci, ci, dbl, vp]
            L.skdsp_qam_demap_rows.argtypes = [vp, i64, i64, i64, i64, i64, ci, ci, vp, vp]
            L.skdsp_qam_demap_rows_dev.argtypes = [vp, i64, i64, i64, i64, i64, ci, ci, vp, vp, i64]
            L.skdsp_mpsk_demap_rows.argtypes = [vp, i64, i64, i64, i64, i64, ci, ci, dbl, dbl, vp]
            L.skdsp_mpsk_demap_rows_dev.argtypes = [vp, i64, i64, i64, i64, i64, ci, ci, dbl, dbl, vp, i64]
        if hasattr(L, "skdsp_awgn_rows_dev"):
            dbl, u64 = ctypes.c_double, ctypes.c_uint64
            L.skdsp_awgn_rows_dev.argtypes = [vp, i64, ci, vp, i64, ci, i64, i64, vp, vp, dbl, dbl, u64, i64, i64]
            L.skdsp_awgn_bits_rows_dev.argtypes = [vp, i64, vp, i64, i64, i64, vp, dbl, u64, i64, i64]
            L.skdsp_awgn_sigma_rows_dev.argtypes = [vp, i64, i64, i64, ci, ci, dbl, dbl, dbl, vp, vp]
            L.skdsp_random_bits_rows_dev.argtypes = [vp, i64, i64, i64, u64, i64, i64]
            L.skdsp_pn_rows_dev.argtypes = [vp, ci, vp, vp, i64, i64, i64, i64]
        if hasattr(L, "skdsp_ofdm_tx_rows_dev"):
            dbl = ctypes.c_double
            L.skdsp_ofdm_tx_rows.argtypes = [vp, i64, i64, ci, ci, ci, ci, ci, ci, vp]
            L.skdsp_ofdm_tx_rows_dev.argtypes = [vp, i64, i64, i64, ci, ci, ci, ci, ci, ci, vp, i64]
            L.skdsp_ofdm_rx_rows.argtypes = [vp, i64, i64, ci, ci, ci, ci, ci, ci, dbl, vp, vp, vp]
            L.skdsp_ofdm_rx_rows_dev.argtypes = [vp, i64, i64, i64, ci, ci, ci, ci, ci, ci, dbl, vp, vp, i64, vp]
            L.skdsp_ofdm_equalize_rows.argtypes = [vp, i64, i64, ci, ci, ci, dbl, vp, vp, vp]
            L.skdsp_ofdm_equalize_rows_dev.argtypes = [vp, i64, i64, i64, ci, ci, ci, dbl, vp, vp, i64, vp]
        if hasattr(L, "skdsp_lag_corr"):
            L.skdsp_lag_corr_len.argtypes = [i64, i64, p64, p64]
            L.skdsp_lag_corr.argtypes = [vp, ci, vp, ci, i64, i64, ci, vp, vp, vp]
            L.skdsp_lag_corr_dev.argtypes = [vp, ci, vp, ci, i64, i64, ci, vp, vp]
            L.skdsp_sym_count_rows.argtypes = L.skdsp_sym_count_rows_dev.argtypes = [vp, ci, i64, i64, vp, ci, i64, i64, i64, i64, i64, i64, ci, ci, ci, vp]
        if hasattr(L, "skdsp_pulse_create"):
            pd = ctypes.POINTER(ctypes.c_double)
            L.skdsp_pulse_create.argtypes = [vp, ci, ci, pvp]
            L.skdsp_pulse_mf_out_len.argtypes = [i64, i64, i64, p64]
            L.skdsp_pulse_shape_rows.argtypes = [vp, vp, i64, i64, ci, pd, vp]
            L.skdsp_pulse_shape_rows_dev.argtypes = [vp, vp, i64, i64, i64, ci, pd, vp, i64]
            L.skdsp_pulse_mf_rows.argtypes = [vp, vp, i64, i64, i64, i64, vp]
            L.skdsp_pulse_mf_rows_dev.argtypes = [vp, vp, i64, i64, i64, i64, i64, vp, i64]
        if hasattr(L, "skdsp_carrier_rows"):
            dbl = ctypes.c_double
            L.skdsp_carrier_rows.argtypes = [vp, i64, i64, i64, i64, i64, ci, ci, ci, ci, ci, dbl, dbl, vp, dbl, dbl, vp, vp, ci, vp, vp, vp, vp]
            L.skdsp_carrier_rows_dev.argtypes = [vp, i64, i64, i64, i64, i64, ci, ci, ci, ci, ci, dbl, dbl, vp, vp, dbl, vp, vp, ci, vp, vp, vp, vp, i64]
            L.skdsp_time_step_rows_dev.argtypes = [vp, i64, i64, i64, ci, i64, i64, i64, vp, vp, i64, i64]
            L.skdsp_phase_step_rows_dev.argtypes = [vp, i64, i64, i64, ci, i64, i64, dbl, dbl, vp, vp, i64]
        if hasattr(L, "skdsp_nda_rows"):
            dbl = ctypes.c_double
            L.skdsp_nda_rows.argtypes = [vp, i64, i64, i64, i64, ci, ci, ci, ci, dbl, dbl, vp, vp, dbl, dbl, dbl, ci, ci, i64, vp, vp, vp]
            L.skdsp_nda_rows_dev.argtypes = [vp, i64, i64, i64, i64, ci, ci, ci, ci, dbl, dbl, vp, vp, dbl, dbl, dbl, ci, ci, i64, vp, vp, vp, i64]
        L.skdsp_dist_unique_id.argtypes = [vp]
        L.skdsp_dist_init.argtypes = [ci, ci, vp]
        L.skdsp_dist_comm_count.argtypes = [ctypes.POINTER(ci)]
        L.skdsp_dist_allreduce_max.argtypes = [ctypes.POINTER(ctypes.c_double)]
        L.skdsp_dist_allreduce_sum.argtypes = [ctypes.POINTER(ctypes.c_double)]
        L.skdsp_set_wide_output.argtypes = [vp, ci]
        L.skdsp_dist_allgather.argtypes = [vp, vp, i64]
        L.skdsp_dist_sendrecv.argtypes = [vp, ci, vp, ci, i64]
        L.skdsp_dist_allgather.argtypes = [vp, vp, i64]
        L.skdsp_dist_halo_exchange.argtypes = [vp, i64, i64, ci]
        L.skdsp_fir_filter_shard_dev.argtypes = [vp, vp, i64, vp]
        _lib = L
        return _lib


_EXC = {-1: ValueError, -2: SkdspError, -3: MemoryError, -4: SkdspError, -5: SkdspError, -6: NotImplementedError}


def check(rc):
    if rc != 0:
        msg = load().skdsp_last_error().decode("utf-8", "replace")
        raise _EXC.get(rc, SkdspError)("skdsp[%d]: %s" % (rc, msg))


def init(device=None):
    """Bind this process: one GPU (default: SKDSP_DEVICE, else LOCAL_RANK, else 0), or -- when SKDSP_DEVICES is set to
    "all" or a list like "0,1,2,3" and no launcher gave this process a rank -- one slot per listed GPU (init_devices)."""
    L = load()
    if device is None:
        devs = os.environ.get("SKDSP_DEVICES")
        if devs and "LOCAL_RANK" not in os.environ and "SKDSP_DEVICE" not in os.environ:
            return init_devices(devs)
        device = int(os.environ.get("SKDSP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    check(L.skdsp_init(int(device)))


def init_devices(devices="all"):
    """One slot per GPU: the host-array FIR calls (multirate_FIR.filter / .up / .dn on long NumPy vectors) then use all
    of them from one process.  devices: "all", "0,1,2" or a sequence of indices; returns the number of slots."""
    L = load()
    if isinstance(devices, str):
        devices = list(range(L.skdsp_device_count())) if devices.strip().lower() == "all" else [int(v) for v in devices.split(",") if v.strip()]
    devices = [int(d) for d in devices]
    if not devices:
        raise SkdspError("no HIP device available: the MI355X path has no CPU fallback")
    arr = (ctypes.c_int * len(devices))(*devices)
    check(L.skdsp_init_devices(arr, len(devices)))
    return L.skdsp_slot_count()


def host_chunk_plan(n, L=1, M=1, hist=0, chunk_log2=24):
    """[(in_begin, in_end, in_hist, out_begin, out_end)] of every chunk the host-pointer entry points would use."""
    lib = load()
    v = [ctypes.c_int64(0) for _ in range(6)]
    check(lib.skdsp_host_chunk_plan(int(n), int(L), int(M), int(hist), int(chunk_log2), 0, *[ctypes.byref(a) for a in v]))
    out = []
    for k in range(v[0].value):
        check(lib.skdsp_host_chunk_plan(int(n), int(L), int(M), int(hist), int(chunk_log2), k, *[ctypes.byref(a) for a in v]))
        out.append(tuple(a.value for a in v[1:]))
    return out


def set_option(name, value):
    """Run-time switch of the library (struct Options in csrc/skdsp_internal.hpp); returns the previous value."""
    L = load()
    old = ctypes.c_int(0)
    check(L.skdsp_get_option(name.encode(), ctypes.byref(old)))
    check(L.skdsp_set_option(name.encode(), int(value)))
    return old.value


def get_option(name):
    v = ctypes.c_int(0)
    check(load().skdsp_get_option(name.encode(), ctypes.byref(v)))
    return v.value


class option:
    """with _ffi.option("iir_planar", 1): ...  -- temporary switch (tests, A/B timing)."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False


def debug_path(clear=True):
    """Names of the kernel families this thread's calls launched since the last clear (tests: which engine did a shape reach?)."""
    buf = ctypes.create_string_buffer(256)
    check(load().skdsp_debug_path(buf, 256, 1 if clear else 0))
    return buf.value.decode().split(",") if buf.value else []


def device_info():
    L = load()
    name = ctypes.create_string_buffer(256)
    cus, hbm, clk = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int(0)
    check(L.skdsp_device_info(name, 256, ctypes.byref(cus), ctypes.byref(hbm), ctypes.byref(clk)))
    return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value, "clock_khz": clk.value}


def code_of(dtype):
    try:
        return _CODE_OF[np.dtype(dtype)]
    except KeyError:
        raise TypeError("unsupported signal dtype %r (float32/complex64/float64/complex128)" % (dtype,))


def np_of(code):
    return _NP_OF[code]


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a.size else ctypes.c_void_p(0)


# --------------------------------------------------------------------------
# device-resident arrays (used by bench.py / sharding; not part of the reference surface)
# --------------------------------------------------------------------------
class DeviceArray:
    """n samples of `dtype` in HBM with `headroom` samples of valid-able space in front
    (the halo / history region: x[-headroom..-1])."""

    def __init__(self, n, dtype, headroom=0):
        L = load()
        self.n = int(n)
        self.code = code_of(dtype)
        self.dtype = np.dtype(dtype)
        esz = self.dtype.itemsize
        # keep x[0] 256-byte aligned whatever the headroom is
        self._pad = ((int(headroom) * esz + 255) // 256) * 256
        self.headroom = int(headroom)
        base = ctypes.c_void_p(0)
        check(L.skdsp_malloc(ctypes.byref(base), self._pad + self.n * esz + 256))
        self._base = base.value
        self.ptr = self._base + self._pad
        self._fin = weakref.finalize(self, _free_dev, self._base)
        if self._pad:
            check(L.skdsp_memset(ctypes.c_void_p(self._base), 0, self._pad))

    @classmethod
    def from_host(cls, a, headroom=0):
        a = np.ascontiguousarray(a)
        d = cls(a.size, a.dtype, headroom)
        check(load().skdsp_memcpy_h2d(ctypes.c_void_p(d.ptr), _ptr(a), a.nbytes))
        return d

    def write(self, a, at=0):
        """Copy host samples to x[at .. at+len(a)); negative `at` addresses the headroom."""
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if at < -self.headroom or at + a.size > self.n:
            raise ValueError("write outside the device array")
        if a.size:
            check(load().skdsp_memcpy_h2d(ctypes.c_void_p(self.ptr + at * self.dtype.itemsize), _ptr(a), a.nbytes))

    def to_host(self, start=0, count=None):
        start = int(start)
        count = self.n - start if count is None else int(count)
        out = np.empty(count, dtype=self.dtype)
        esz = self.dtype.itemsize
        check(load().skdsp_memcpy_d2h(_ptr(out), ctypes.c_void_p(self.ptr + start * esz), out.nbytes))
        return out

    def window(self, start, count):
        """A non-owning view of samples [start, start + count) (kernels that write a slice of a larger device buffer)."""
        if start < 0 or start + count > self.n:
            raise ValueError("window outside the device array")
        v = object.__new__(DeviceArray)
        v.n, v.code, v.dtype, v.headroom, v._pad = int(count), self.code, self.dtype, 0, 0
        v._base = None
        v.ptr = self.ptr + int(start) * self.dtype.itemsize
        v._fin = lambda: None
        v._owner = self   # keeps the allocation alive
        return v

    def fill_noise(self, seed, first_index=0):
        check(load().skdsp_fill_noise_dev(ctypes.c_void_p(self.ptr), self.n, self.code, int(seed), int(first_index)))
        return self

    def free(self):
        self._fin()


class DeviceBytes:
    """nbytes of HBM addressed by the byte (the bit streams of BlockCodeKernel's *_dev calls, at any alignment): ptr is 256-byte aligned."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        base = ctypes.c_void_p(0)
        check(load().skdsp_malloc(ctypes.byref(base), self.nbytes))
        self.ptr = base.value
        self._fin = weakref.finalize(self, _free_dev, self.ptr)

    def write(self, a, at=0):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if at < 0 or at + a.size > self.nbytes:
            raise ValueError("write outside the device bytes")
        check(load().skdsp_memcpy_h2d(ctypes.c_void_p(self.ptr + int(at)), _ptr(a), a.nbytes))

    def read(self, at=0, count=None):
        count = self.nbytes - int(at) if count is None else int(count)
        if at < 0 or at + count > self.nbytes:
            raise ValueError("read outside the device bytes")
        out = np.empty(count, dtype=np.uint8)
        check(load().skdsp_memcpy_d2h(_ptr(out), ctypes.c_void_p(self.ptr + int(at)), out.nbytes))
        return out

    def free(self):
        self._fin()


def _free_dev(base):
    try:
        load().skdsp_free(ctypes.c_void_p(base))
    except Exception:
        pass


def sync():
    check(load().skdsp_sync())


def timer_start():
    check(load().skdsp_timer_start())


def timer_stop():
    ms = ctypes.c_float(0.0)
    check(load().skdsp_timer_stop(ctypes.byref(ms)))
    return float(ms.value)


# --------------------------------------------------------------------------
# handles
# --------------------------------------------------------------------------
def _destroy(h):
    try:
        load().skdsp_destroy(ctypes.c_void_p(h))
    except Exception:
        pass


_WIDE = {np.dtype(np.float32): np.dtype(np.float64), np.dtype(np.complex64): np.dtype(np.complex128)}


class _PinnedBlock:
    """One page-locked block; exposes its bytes through __array_interface__ and goes back to the pool when the last
    ndarray view of it dies."""

    def __init__(self, pool, ptr, nbytes):
        self.pool, self.ptr, self.nbytes = pool, ptr, nbytes
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    def __del__(self):
        try:
            self.pool._give_back(self.ptr, self.nbytes)
        except Exception:
            pass


class PinnedPool:
    """Result arrays of long host-array calls come from recycled page-locked blocks.

    A copy back into a fresh np.empty array pays for the population of its pages and their first device access
    (31 ms per 512 MiB instead of 12, and another 26 ms when NumPy unmaps it again: tools/host_pipe_time.py); a
    page-locked block receives the DMA at the link rate and is handed to the next call of the same size when its
    array is garbage collected.  The arrays are ordinary writable ndarrays whose .base chain ends in the block: they do
    NOT own their memory (ndarray.resize refuses them; np.copy gives an owning array).
    max_bytes bounds what the pool keeps for reuse; max_live_bytes bounds the page-locked memory in the hands of live
    result arrays plus the pool (beyond it results are ordinary np.empty arrays); 0 switches the pool off.
    The lock is re-entrant and nothing is allocated while it is held: a block's finaliser (_give_back) can run inside
    any allocation -- including one made by this class -- when the cyclic collector fires."""

    GRANULE = 2 << 20

    def __init__(self, max_bytes=4 << 30, min_bytes=32 << 20, max_live_bytes=None):
        self.max_bytes, self.min_bytes = int(max_bytes), int(min_bytes)
        self.max_live_bytes = int(max_live_bytes) if max_live_bytes is not None else 4 * self.max_bytes
        self._free = {}      # rounded size -> [ptr]
        self._kept = 0
        self._live = 0       # bytes of blocks currently wrapped by result arrays
        self._lock = threading.RLock()

    def empty(self, count, dtype):
        dtype = np.dtype(dtype)
        nbytes = int(count) * dtype.itemsize
        if self.max_bytes <= 0 or nbytes < self.min_bytes:
            return np.empty(count, dtype=dtype)
        size = -(-nbytes // self.GRANULE) * self.GRANULE
        ptr = None
        with self._lock:
            lst = self._free.get(size)
            if lst:
                ptr = lst.pop()
                self._kept -= size
                self._live += size
            elif self._live + self._kept + size > self.max_live_bytes:
                size = 0   # cap on page-locked host memory reached
            else:
                self._live += size   # reserved before the allocation below (which runs outside the lock)
        if size == 0:
            return np.empty(count, dtype=dtype)
        if ptr is None:
            p = ctypes.c_void_p(0)
            try:
                check(load().skdsp_host_alloc(ctypes.byref(p), size))
            except Exception:
                with self._lock:
                    self._live -= size
                return np.empty(count, dtype=dtype)   # no page-locked memory left: an ordinary array
            ptr = p.value
        block = _PinnedBlock(self, ptr, size)
        return np.asarray(block)[:nbytes].view(dtype)

    def _give_back(self, ptr, size):
        keep = False
        with self._lock:
            self._live -= size
            lst = self._free.get(size)
            if self._kept + size <= self.max_bytes and lst is not None:
                lst.append(ptr)          # (list.append of an int allocates nothing the collector tracks)
                self._kept += size
                keep = True
        if keep:
            return
        if self._kept + size <= self.max_bytes:
            fresh = [ptr]                # first block of this size: the list is built OUTSIDE the lock
            with self._lock:
                if self._kept + size <= self.max_bytes:
                    cur = self._free.get(size)
                    if cur is None:
                        self._free[size] = fresh
                    else:
                        cur.append(ptr)
                    self._kept += size
                    return
        load().skdsp_host_free(ctypes.c_void_p(ptr))

    def trim(self):
        """Release every block the pool holds for reuse."""
        with self._lock:
            old, self._free, self._kept = self._free, {}, 0
        for lst in old.values():
            for p in lst:
                load().skdsp_host_free(ctypes.c_void_p(p))


result_pool = PinnedPool(int(os.environ.get("SKDSP_PINNED_POOL_BYTES", str(4 << 30))))


class _HostCalls:
    """Shared by FirKernel / IirKernel: output allocation for the host-pointer entry points.
    wide=True asks the library for float64/complex128 results from a float32/complex64 handle
    (widened on the device: skdsp_set_wide_output)."""
    _wide_state = False
    _call_lock = None

    def _host(self, count, dtype, wide, call):
        """One host-pointer call: the per-handle result-width switch and the call it applies to form one critical section,
        so an object shared between threads cannot get the other thread's width."""
        if self._call_lock is None:
            self.__dict__.setdefault("_call_lock", threading.Lock())
        with self._call_lock:
            y = self._out(count, dtype, wide)
            call(y)
            return y

    def _out(self, count, dtype, wide):
        dtype = np.dtype(dtype)
        wide = bool(wide) and dtype in _WIDE
        if wide != self._wide_state:
            check(load().skdsp_set_wide_output(ctypes.c_void_p(self.h), int(wide)))
            self._wide_state = wide
        return result_pool.empty(count, _WIDE[dtype] if wide else dtype)


class FirKernel(_HostCalls):
    """A device FIR handle for one (taps, signal dtype) pair."""

    def __init__(self, taps, code):
        L = load()
        taps = np.asarray(taps)
        self.taps_complex = bool(np.iscomplexobj(taps))
        t = np.ascontiguousarray(taps, dtype=np.complex128 if self.taps_complex else np.float64)
        self.ntaps = int(t.size)
        self.code = code
        h = ctypes.c_void_p(0)
        check(L.skdsp_fir_create(_ptr(t), self.ntaps, int(self.taps_complex), code, ctypes.byref(h)))
        self.h = h.value
        self._fin = weakref.finalize(self, _destroy, self.h)

    def set_algo(self, algo):
        check(load().skdsp_fir_set_algo(ctypes.c_void_p(self.h), int(algo)))

    def algo_for(self, n):
        a = ctypes.c_int(0)
        check(load().skdsp_fir_get_algo(ctypes.c_void_p(self.h), int(n), ctypes.byref(a)))
        return a.value

    # host vectors ------------------------------------------------------
    def filter(self, x, wide=False):
        return self._host(x.size, x.dtype, wide, lambda y: check(load().skdsp_fir_filter(ctypes.c_void_p(self.h), _ptr(x), x.size, _ptr(y))))

    def filter_sharded(self, x, ngpu=0, wide=False):
        """.filter(x) over the first ngpu slots bound by init_devices (0: all): contiguous sample blocks, halos from the host array."""
        return self._host(x.size, x.dtype, wide,
                          lambda y: check(load().skdsp_fir_filter_sharded(ctypes.c_void_p(self.h), _ptr(x), x.size, _ptr(y), int(ngpu))))

    def up(self, x, L, wide=False):
        return self._host(x.size * L, x.dtype, wide, lambda y: check(load().skdsp_fir_up(ctypes.c_void_p(self.h), _ptr(x), x.size, int(L), _ptr(y))))

    def dn(self, x, M, wide=False):
        return self._host(x.size // M, x.dtype, wide, lambda y: check(load().skdsp_fir_dn(ctypes.c_void_p(self.h), _ptr(x), x.size, int(M), _ptr(y))))

    def updn(self, x, L, M, wide=False):
        return self._host((x.size * L) // M, x.dtype, wide, lambda y: check(load().skdsp_fir_updn(ctypes.c_void_p(self.h), _ptr(x), x.size, int(L), int(M), _ptr(y))))

    # device vectors ----------------------------------------------------
    def filter_dev(self, xd, yd, n=None, n_hist=0):
        n = xd.n if n is None else n
        check(load().skdsp_fir_filter_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, n_hist, ctypes.c_void_p(yd.ptr)))

    def up_dev(self, xd, yd, L, n=None, n_hist=0):
        n = xd.n if n is None else n
        check(load().skdsp_fir_up_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, n_hist, int(L), ctypes.c_void_p(yd.ptr)))

    def dn_dev(self, xd, yd, M, n=None, n_hist=0):
        n = xd.n if n is None else n
        check(load().skdsp_fir_dn_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, n_hist, int(M), ctypes.c_void_p(yd.ptr)))

    def updn_dev(self, xd, yd, L, M, n=None, n_hist=0):
        n = xd.n if n is None else n
        check(load().skdsp_fir_updn_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, n_hist, int(L), int(M),
                                         ctypes.c_void_p(yd.ptr)))

    def filter_rows(self, x2, wide=False):
        """x2: C-contiguous (rows, n): every row filtered from rest in ONE call (one pitched copy each way, one launch)."""
        rows, n = x2.shape
        y = self._host(x2.size, x2.dtype, wide, lambda y: check(load().skdsp_fir_filter_rows(ctypes.c_void_p(self.h), _ptr(x2), n, rows, _ptr(y))))
        return y.reshape(rows, n)

    def filter_rows_dev(self, xd, yd, n, rows, x_stride=None, y_stride=None):
        check(load().skdsp_fir_filter_rows_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, rows, n if x_stride is None else x_stride,
                                                n if y_stride is None else y_stride, ctypes.c_void_p(yd.ptr)))

    def filter_shard_dev(self, xd, yd, n=None):
        n = xd.n if n is None else n
        check(load().skdsp_fir_filter_shard_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, ctypes.c_void_p(yd.ptr)))


class FirBank:
    """A bank of frequency-shifted copies of one FIR over ONE float32 / complex64 signal (csrc/fir_bank.hip):
    band j = taps[n] * exp(2j pi ((shifts[j] n) mod period) / period); every output row is complex64."""

    def __init__(self, taps, shifts, period, dtype):
        L = load()
        taps = np.asarray(taps)
        self.taps_complex = bool(np.iscomplexobj(taps))
        t = np.ascontiguousarray(taps, dtype=np.complex128 if self.taps_complex else np.float64)
        sh = np.ascontiguousarray(shifts, dtype=np.int64)
        if t.ndim != 1 or sh.ndim != 1:
            raise ValueError("FirBank: taps and shifts must be one-dimensional")
        self.ntaps, self.nbands = int(t.size), int(sh.size)
        self.dtype = np.dtype(dtype)
        self.code = code_of(self.dtype)
        h = ctypes.c_void_p(0)
        check(L.skdsp_fir_bank_create(_ptr(t), self.ntaps, int(self.taps_complex), sh.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                      self.nbands, int(period), self.code, ctypes.byref(h)))
        self.h = h.value
        self._fin = weakref.finalize(self, _destroy, self.h)

    def filter_dev(self, xd, yd, row_stride=None, n=None):
        """Row j of the result at yd[j * row_stride : j * row_stride + n] (complex64), from rest; row_stride defaults to n."""
        n = xd.n if n is None else int(n)
        row_stride = n if row_stride is None else int(row_stride)
        if xd.dtype != self.dtype or yd.dtype != np.complex64:
            raise ValueError("FirBank: the signal must be %s and the rows complex64" % self.dtype)
        if n < 0 or n > xd.n or row_stride < n or (self.nbands - 1) * row_stride + n > yd.n:
            raise ValueError("FirBank: %d rows of %d samples, %d apart, do not fit the arrays" % (self.nbands, n, row_stride))
        check(load().skdsp_fir_bank_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, ctypes.c_void_p(yd.ptr), row_stride))


class ViterbiKernel:
    """A device Viterbi decoder handle (csrc/viterbi.hip): rate 1/2 or 1/3, K = 3 ... 9, decision depth 1 ... 128.  The handle carries the
    decoder state of its decode() calls; decode_rows() starts every row from rest and leaves that state alone."""
    HARD, SOFT, UNQUANT = 0, 1, 2
    X_DTYPE = {0: np.int8, 1: np.int16, 2: np.float64}   # hard, soft (values already truncated), unquant

    def __init__(self, polys, depth):
        L = load()
        arr = (ctypes.c_char_p * len(polys))(*[str(g).encode() for g in polys])
        h = ctypes.c_void_p(0)
        check(L.skdsp_viterbi_create(arr, len(polys), int(depth), ctypes.byref(h)))
        self.h = h.value
        self._fin = weakref.finalize(self, _destroy, self.h)

    def out_len(self, nval):
        n = ctypes.c_int64(0)
        check(load().skdsp_viterbi_out_len(ctypes.c_void_p(self.h), int(nval), ctypes.byref(n)))
        return n.value

    def reset(self):
        check(load().skdsp_viterbi_reset(ctypes.c_void_p(self.h)))

    def _x(self, x, metric, ndim):
        x = np.ascontiguousarray(x, dtype=self.X_DTYPE[metric])
        if x.ndim != ndim:
            raise ValueError("ViterbiKernel: the received values must be %d-dimensional" % ndim)
        return x

    def decode(self, x, metric, quant_level=3):
        """n received values -> out_len(n) bytes 0 / 1, continuing from the handle's state."""
        x = self._x(x, metric, 1)
        y = np.empty(self.out_len(x.size), dtype=np.uint8)
        check(load().skdsp_viterbi_decode(ctypes.c_void_p(self.h), _ptr(x), x.size, metric, metric, int(quant_level), _ptr(y)))
        return y

    def decode_rows(self, x, metric, quant_level=3):
        """(nrow, n) received values -> (nrow, out_len(n)) bytes, every row from rest, one launch."""
        x = self._x(x, metric, 2)
        nrow, n = x.shape
        y = np.empty((nrow, self.out_len(n)), dtype=np.uint8)
        check(load().skdsp_viterbi_decode_rows(ctypes.c_void_p(self.h), _ptr(x), n, nrow, metric, metric, int(quant_level), _ptr(y)))
        return y

    def decode_dev(self, x_ptr, n, metric, quant_level, y_ptr):
        check(load().skdsp_viterbi_decode_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(x_ptr), int(n), metric, metric, int(quant_level), ctypes.c_void_p(y_ptr)))

    def decode_rows_dev(self, x_ptr, n, nrow, metric, quant_level, y_ptr):
        check(load().skdsp_viterbi_decode_rows_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(x_ptr), int(n), int(nrow), metric, metric, int(quant_level),
                                                   ctypes.c_void_p(y_ptr)))


class BlockCodeKernel:
    """A device block-code handle (csrc/blockcode.hip): n = 2^j - 1, k = n - j, j = 3 ... 16, the code given as its three tables of j-bit
    words (fec_block.py: the table form).  Bits are bytes 0 / 1 on both sides; every call is one launch."""

    def __init__(self, n, k, enc, syn, trap):
        self.n, self.k = int(n), int(k)
        enc, syn, trap = (np.ascontiguousarray(t, dtype=np.uint32) for t in (enc, syn, trap))
        if enc.shape != (self.k,) or syn.shape != (self.n,) or trap.shape != (self.k,):
            raise ValueError("BlockCodeKernel: the tables hold k, n and k words")
        h = ctypes.c_void_p(0)
        check(load().skdsp_blockcode_create(self.n, self.k, _ptr(enc), _ptr(syn), _ptr(trap), ctypes.byref(h)))
        self.h = h.value
        self._fin = weakref.finalize(self, _destroy, self.h)

    def _run(self, fn, x, per_in, per_out):
        x = np.ascontiguousarray(x, dtype=np.uint8)
        if x.ndim != 2 or x.shape[1] != per_in:
            raise ValueError("BlockCodeKernel: the bits must be (nblocks, %d) bytes" % per_in)
        y = np.empty((x.shape[0], per_out), dtype=np.uint8)
        check(fn(ctypes.c_void_p(self.h), _ptr(x), x.shape[0], _ptr(y)))
        return y

    def encode(self, bits):
        """(nblocks, k) bytes 0 / 1 -> (nblocks, n) bytes"""
        return self._run(load().skdsp_blockcode_encode, bits, self.k, self.n)

    def decode(self, code):
        """(nblocks, n) bytes 0 / 1 -> (nblocks, k) bytes"""
        return self._run(load().skdsp_blockcode_decode, code, self.n, self.k)

    def encode_dev(self, bits_ptr, nblocks, code_ptr):
        check(load().skdsp_blockcode_encode_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(bits_ptr), int(nblocks), ctypes.c_void_p(code_ptr)))

    def decode_dev(self, code_ptr, nblocks, bits_ptr):
        check(load().skdsp_blockcode_decode_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(code_ptr), int(nblocks), ctypes.c_void_p(bits_ptr)))


MAX_PATTERN = 64


def pattern_masks(puncture_pattern):
    """(mask1, mask2, L_pp) of a puncture pattern (two strings of 0 / 1): digit k is bit k.  ValueError for what the kernels do not serve --
    more than 64 digits, unequal lengths, unequal numbers of ones (the reference cannot serve the last two either), no ones at all."""
    if len(puncture_pattern) != 2:
        raise ValueError("a puncture pattern is two strings of 0 / 1 (the G1 and the G2 stream)")
    p1, p2 = (str(p) for p in puncture_pattern)
    if set(p1 + p2) - {'0', '1'}:
        raise ValueError("a puncture pattern is two strings of 0 / 1")
    if len(p1) != len(p2):
        raise ValueError("the two puncture patterns must have the same length (got %d and %d digits)" % (len(p1), len(p2)))
    if not 1 <= len(p1) <= MAX_PATTERN:
        raise ValueError("puncture patterns of 1 ... %d digits are served (got %d)" % (MAX_PATTERN, len(p1)))
    if p1.count('1') != p2.count('1') or p1.count('1') == 0:
        raise ValueError("the two puncture patterns must keep the same, non-zero number of bits (got %d and %d)" % (p1.count('1'), p2.count('1')))
    return int(p1[::-1], 2), int(p2[::-1], 2), len(p1)


def puncture_out_len(n, puncture_pattern, depuncture=False):
    """Elements per output row of puncture_rows / depuncture_rows for rows of n elements: the C library's own length function."""
    m1, m2, L_pp = pattern_masks(puncture_pattern)
    out = ctypes.c_int64(0)
    fn = load().skdsp_depuncture_out_len if depuncture else load().skdsp_puncture_out_len
    check(fn(int(n), m1, m2, L_pp, ctypes.byref(out)))
    return out.value


def _rows2d(x, what):
    x = np.ascontiguousarray(x)
    if x.ndim != 2:
        raise ValueError("%s: a 2-D array, one frame per row" % what)
    if x.dtype.itemsize not in (1, 2, 4, 8) or x.dtype.kind not in "biuf":
        raise ValueError("%s: elements of 1, 2, 4 or 8 bytes (got %s)" % (what, x.dtype))
    return x


def puncture_rows(x, puncture_pattern):
    """(nrow, n) elements of 1, 2, 4 or 8 bytes -> (nrow, puncture_out_len(n)) of the same dtype (csrc/convcode.hip: puncture_kernel)"""
    x = _rows2d(x, "puncture_rows")
    m1, m2, L_pp = pattern_masks(puncture_pattern)
    y = np.empty((x.shape[0], puncture_out_len(x.shape[1], puncture_pattern)), dtype=x.dtype)
    check(load().skdsp_puncture_rows(_ptr(x), x.shape[1], x.shape[0], x.dtype.itemsize, m1, m2, L_pp, _ptr(y)))
    return y


def depuncture_rows(x, puncture_pattern, erase):
    """(nrow, n) elements -> (nrow, depuncture_out_len(n)) of the same dtype; erase is converted to that dtype the way NumPy's astype does
    (float -> integer: toward zero)."""
    x = _rows2d(x, "depuncture_rows")
    m1, m2, L_pp = pattern_masks(puncture_pattern)
    e = np.array([erase]).astype(x.dtype)
    y = np.empty((x.shape[0], puncture_out_len(x.shape[1], puncture_pattern, True)), dtype=x.dtype)
    check(load().skdsp_depuncture_rows(_ptr(x), x.shape[1], x.shape[0], x.dtype.itemsize, m1, m2, L_pp, _ptr(e), _ptr(y)))
    return y


def puncture_rows_dev(x_ptr, n, nrow, elem_bytes, puncture_pattern, y_ptr):
    m1, m2, L_pp = pattern_masks(puncture_pattern)
    check(load().skdsp_puncture_rows_dev(ctypes.c_void_p(x_ptr), int(n), int(nrow), int(elem_bytes), m1, m2, L_pp, ctypes.c_void_p(y_ptr)))


def depuncture_rows_dev(x_ptr, n, nrow, dtype, puncture_pattern, erase, y_ptr):
    """dtype: the elements' NumPy dtype (erase is converted to it on the host)"""
    m1, m2, L_pp = pattern_masks(puncture_pattern)
    e = np.array([erase]).astype(dtype)
    check(load().skdsp_depuncture_rows_dev(ctypes.c_void_p(x_ptr), int(n), int(nrow), e.dtype.itemsize, m1, m2, L_pp, _ptr(e), ctypes.c_void_p(y_ptr)))


def bit_count_rows(tx, rx, invert=False, n=None):
    """Two 2-D byte arrays with the same number of rows -> int64[nrow]: the positions among the first n (default: the narrower width) of
    row r where tx and rx differ (invert: agree) (csrc/convcode.hip: bitcount_kernel)"""
    tx, rx = np.ascontiguousarray(tx, dtype=np.uint8), np.ascontiguousarray(rx, dtype=np.uint8)
    if tx.ndim != 2 or rx.ndim != 2 or tx.shape[0] != rx.shape[0]:
        raise ValueError("bit_count_rows: two 2-D arrays with the same number of rows")
    n = min(tx.shape[1], rx.shape[1]) if n is None else int(n)
    if n < 0 or n > min(tx.shape[1], rx.shape[1]):
        raise ValueError("bit_count_rows: n beyond a row")
    counts = np.zeros(tx.shape[0], dtype=np.int64)
    check(load().skdsp_bit_count_rows(_ptr(tx), tx.shape[1], _ptr(rx), rx.shape[1], n, tx.shape[0], int(bool(invert)), _ptr(counts)))
    return counts


def bit_count_rows_dev(tx_ptr, tx_stride, rx_ptr, rx_stride, n, nrow, invert, counts_ptr):
    """Device pointers; the strides are bytes from row to row, a start offset is part of the pointer; counts: nrow int64, 8-byte aligned."""
    check(load().skdsp_bit_count_rows_dev(ctypes.c_void_p(tx_ptr), int(tx_stride), ctypes.c_void_p(rx_ptr), int(rx_stride), int(n), int(nrow), int(bool(invert)),
                                          ctypes.c_void_p(counts_ptr)))


class ConvCodeKernel:
    """A convolutional encoder handle (csrc/convcode.hip): rate 1/2 or 1/3, K = 3 ... 9, the polynomials read as ViterbiKernel reads them.
    Bits are bytes 0 / 1; a state is the reference's state string (K - 1 digits, newest first) read as a binary number, one byte per row."""

    def __init__(self, polys):
        arr = (ctypes.c_char_p * len(polys))(*[str(g).encode() for g in polys])
        h = ctypes.c_void_p(0)
        check(load().skdsp_convcode_create(arr, len(polys), ctypes.byref(h)))
        self.h = h.value
        self.R, self.K = len(polys), len(str(polys[0]))
        self._fin = weakref.finalize(self, _destroy, self.h)

    def encode_rows(self, bits, states=None):
        """(nrow, n) bytes 0 / 1, states: None (rest) or uint8[1 | nrow] -> ((nrow, R n) bytes, uint8[nrow] final states)"""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        if bits.ndim != 2:
            raise ValueError("ConvCodeKernel: the bits must be (nrow, n) bytes")
        nrow, n = bits.shape
        st = np.zeros(0, dtype=np.uint8) if states is None else np.ascontiguousarray(states, dtype=np.uint8).reshape(-1)
        code, out = np.empty((nrow, self.R * n), dtype=np.uint8), np.zeros(nrow, dtype=np.uint8)
        check(load().skdsp_convcode_encode_rows(ctypes.c_void_p(self.h), _ptr(bits), n, nrow, _ptr(st), st.size, _ptr(code), _ptr(out)))
        return code, out

    def encode_rows_dev(self, bits_ptr, n, nrow, states_in_ptr, nstates_in, code_ptr, states_out_ptr):
        """Device pointers throughout; states_in_ptr / states_out_ptr may be 0 (rest / not wanted)."""
        check(load().skdsp_convcode_encode_rows_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(bits_ptr), int(n), int(nrow), ctypes.c_void_p(states_in_ptr or None),
                                                    int(nstates_in), ctypes.c_void_p(code_ptr), ctypes.c_void_p(states_out_ptr or None)))

    puncture_rows = staticmethod(puncture_rows)
    puncture_rows_dev = staticmethod(puncture_rows_dev)
    depuncture_rows = staticmethod(depuncture_rows)
    depuncture_rows_dev = staticmethod(depuncture_rows_dev)


# --------------------------------------------------------------------------
# Gray symbol mapping (csrc/symmap.hip): the two ends of an M-QAM / M-PSK BER loop
# --------------------------------------------------------------------------
QAM, MPSK = 0, 1
_SYM_ORDERS = {QAM: (2, 4, 16, 64, 256), MPSK: (2, 4, 8, 16, 32)}
_SYM_ERR = {QAM: 'M must be 2, 4, 16, 64, 256', MPSK: 'M must be 2, 4, 8, 16, or 32'}


def sym_bits(kind, mod):
    """Bits per symbol of the order; ValueError with the reference's text for an order the family does not have."""
    if kind not in _SYM_ORDERS or mod not in _SYM_ORDERS[kind]:
        raise ValueError(_SYM_ERR.get(kind, "kind must be QAM (0) or MPSK (1)"))
    return int(mod).bit_length() - 1


def gray_table(kind, mod, dtype=np.complex128):
    """(tab_re, tab_im) float64: the constellation by MSB-first word, computed with the reference's own NumPy operations
    (digitalcom.py:1626-1681, 1784-1826); for complex64 output rounded to float32 here.  QAM of 4 points and more: the sqrt(mod) levels."""
    bps = sym_bits(kind, mod)
    if mod == 2:
        pts = (2 * np.arange(2) - 1).astype(np.complex128)
    elif kind == QAM:
        x_m = np.sqrt(mod) - 1
        lut = _bin2gray(bps // 2)
        pts = ((2 * lut - x_m) + 1j * (2 * lut - x_m)) / x_m      # complex / real scalar, as x_IQ / x_m
    else:
        lut = _bin2gray(bps)
        pts = np.exp(1j * (2 * np.pi * lut / mod + (np.pi / mod if mod == 4 else 0.0)))
    if np.dtype(dtype) == np.complex64:
        pts = pts.astype(np.complex64).astype(np.complex128)
    elif np.dtype(dtype) != np.complex128:
        raise TypeError("gray_map: complex64 or complex128 symbols (got %s)" % np.dtype(dtype))
    return np.ascontiguousarray(pts.real), np.ascontiguousarray(pts.imag)


def gray_levels(kind, mod, dtype=np.complex128):
    """((tab_re, tab_im), scale): the points as the *_gray_encode_bb transmitters hold them BEFORE pulse shaping -- QAM of 4 points and more: the
    integer levels 2 lut - x_m, which the transmitter divides by x_m = sqrt(mod) - 1 behind the shaping filter (scale = 1 / x_m: NumPy divides a
    complex array by a real scalar as a multiplication of each component by the reciprocal) -- and None where there is no scale"""
    if kind == QAM and mod > 2:
        bps = sym_bits(kind, mod)
        x_m = np.sqrt(mod) - 1
        lv = np.ascontiguousarray(2 * _bin2gray(bps // 2) - x_m, dtype=np.float64)
        if np.dtype(dtype) not in (np.dtype(np.complex64), np.dtype(np.complex128)):
            raise TypeError("gray_map: complex64 or complex128 symbols (got %s)" % np.dtype(dtype))
        return (lv, np.zeros_like(lv)), (None if x_m == 1 else float(1.0 / x_m))
    return gray_table(kind, mod, dtype), None


def _bin2gray(width):
    """the reference's bin2gray tables: entry k is the running XOR of k's bits from the MSB down"""
    v = np.arange(2 ** width)
    shift = 1
    while shift < width:
        v = v ^ (v >> shift)
        shift *= 2
    return v


def qam_scale_const(mod):
    """c of s = np.std(x_hat) * c (digitalcom.py:1703)"""
    return float(np.sqrt(3 / (2 * (mod - 1))))


def _mpsk_rot():
    r = np.exp(-1j * np.pi / 4)
    return float(r.real), float(r.imag)


def _sym_rows(x, what):
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("%s: a 2-D array, one frame per row" % what)
    if x.dtype not in (np.complex64, np.complex128):
        raise TypeError("%s: complex64 or complex128 symbols (got %s)" % (what, x.dtype))
    return np.ascontiguousarray(x)


def sym_count(width, start, step):
    """Symbols of a row of `width` elements read as row[start::step]"""
    if start < 0 or step < 1:
        raise ValueError("need start >= 0 and step >= 1")
    return max(0, (width - start + step - 1) // step)


def gray_map_rows(bits, kind, mod, dtype=np.complex128):
    """(nrow, nbits) bytes 0 / 1 -> (nrow, nbits // bps) points of `dtype` (csrc/symmap.hip: symmap_kernel); trailing bits that do not fill a
    symbol are dropped."""
    bps = sym_bits(kind, mod)
    bits = np.asarray(bits)
    if bits.ndim != 2:
        raise ValueError("gray_map_rows: a 2-D array, one frame per row")
    n = bits.shape[1] // bps
    bits = np.ascontiguousarray(bits[:, :n * bps], dtype=np.uint8)
    tre, tim = gray_table(kind, mod, dtype)
    y = np.empty((bits.shape[0], n), dtype=dtype)
    check(load().skdsp_gray_map_rows(_ptr(bits), n, bits.shape[0], kind, mod, _ptr(tre), _ptr(tim), tre.size, code_of(dtype), _ptr(y)))
    return y


def gray_map_rows_host(bits, kind, mod, dtype=np.complex128, table=None):
    """gray_map_rows in NumPy (no GPU): the same table (or `table`, as gray_levels returns it), looked up by the MSB-first words -- the yardstick of the kernel."""
    bps = sym_bits(kind, mod)
    bits = np.asarray(bits)
    n = bits.shape[1] // bps
    words = (bits[:, :n * bps].reshape(bits.shape[0], n, bps).astype(np.int64) & 1) @ (2 ** np.arange(bps - 1, -1, -1))
    tre, tim = gray_table(kind, mod, dtype) if table is None else table
    y = np.empty(words.shape, dtype=np.complex128)
    if kind == QAM and mod > 2:
        half = bps // 2
        y.real, y.imag = tre[words >> half], tre[words & (2 ** half - 1)]
    else:
        y.real, y.imag = tre[words], tim[words]
    return y.astype(dtype)


def gray_map_rows_dev(bits_ptr, bits_stride, n, nrow, kind, mod, dtype, y_ptr, y_stride=None, table=None):
    """Device pointers: n symbols per row from bps n bytes; bits_stride in bytes, y_stride in elements (default n); table: (tab_re, tab_im) in place
    of gray_table's (gray_levels: the points before the transmitter's scale)."""
    tre, tim = gray_table(kind, mod, dtype) if table is None else table
    check(load().skdsp_gray_map_rows_dev(ctypes.c_void_p(bits_ptr), int(bits_stride), int(n), int(nrow), kind, mod, _ptr(tre), _ptr(tim), tre.size, code_of(dtype),
                                         ctypes.c_void_p(y_ptr), int(n if y_stride is None else y_stride)))


def qam_scale_rows(x, mod, start=0, step=1):
    """(nrow, width) complex -> float64[nrow]: r = 1 / (np.std(row[start::step]) * sqrt(3 / (2 (mod - 1)))) (csrc/symmap.hip: symscale_kernel)"""
    sym_bits(QAM, mod)
    x = _sym_rows(x, "qam_scale_rows")
    n = sym_count(x.shape[1], start, step)
    r = np.empty(x.shape[0], dtype=np.float64)
    check(load().skdsp_qam_scale_rows(_ptr(x), x.shape[1], int(start), int(step), n, x.shape[0], code_of(x.dtype), mod, qam_scale_const(mod), _ptr(r)))
    return r


def qam_scale_rows_dev(x_ptr, x_stride, start, step, n, nrow, dtype, mod, r_ptr):
    """Device pointers; x_stride, start, step in elements; r: nrow float64, left on the device (and not checked)."""
    check(load().skdsp_qam_scale_rows_dev(ctypes.c_void_p(x_ptr), int(x_stride), int(start), int(step), int(n), int(nrow), code_of(dtype), mod, qam_scale_const(mod),
                                          ctypes.c_void_p(r_ptr)))


def gray_demap_rows(x, kind, mod, start=0, step=1, r=None):
    """(nrow, width) complex -> (nrow, bps n) bytes 0 / 1, n = len(row[start::step]) (csrc/symmap.hip: symdemap_kernel).  QAM: r is the rows'
    scale, float64[nrow] (qam_scale_rows, or the caller's own)."""
    bps = sym_bits(kind, mod)
    x = _sym_rows(x, "gray_demap_rows")
    n = sym_count(x.shape[1], start, step)
    bits = np.empty((x.shape[0], bps * n), dtype=np.uint8)
    L = load()
    if kind == QAM:
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
        if r.size != x.shape[0]:
            raise ValueError("gray_demap_rows: one scale per row")
        check(L.skdsp_qam_demap_rows(_ptr(x), x.shape[1], int(start), int(step), n, x.shape[0], code_of(x.dtype), mod, _ptr(r), _ptr(bits)))
    else:
        check(L.skdsp_mpsk_demap_rows(_ptr(x), x.shape[1], int(start), int(step), n, x.shape[0], code_of(x.dtype), mod, *_mpsk_rot(), _ptr(bits)))
    return bits


def gray_demap_rows_dev(x_ptr, x_stride, start, step, n, nrow, dtype, kind, mod, bits_ptr, bits_stride=None, r_ptr=None):
    """Device pointers; bits_stride in bytes (default bps n); QAM: r_ptr is the device pointer of the rows' scales."""
    bps = sym_bits(kind, mod)
    bs = int(bps * n if bits_stride is None else bits_stride)
    if kind == QAM:
        check(load().skdsp_qam_demap_rows_dev(ctypes.c_void_p(x_ptr), int(x_stride), int(start), int(step), int(n), int(nrow), code_of(dtype), mod,
                                              ctypes.c_void_p(r_ptr or None), ctypes.c_void_p(bits_ptr), bs))
    else:
        check(load().skdsp_mpsk_demap_rows_dev(ctypes.c_void_p(x_ptr), int(x_stride), int(start), int(step), int(n), int(nrow), code_of(dtype), mod, *_mpsk_rot(),
                                               ctypes.c_void_p(bits_ptr), bs))


# --------------------------------------------------------------------------
# The AWGN channel and the bit sources (csrc/channel.hip): the middle and the start of a device-resident BER loop
# --------------------------------------------------------------------------
TAG_NORMAL, TAG_BITS = 0, 1
SIGMA_AWGN, SIGMA_AWGN2 = 0, 1
_U32 = np.uint64(0xffffffff)
_LN2_HI, _LN2_LO = float.fromhex("0x1.62e42feep-1"), float.fromhex("0x1.a39ef35793c76p-33")
_SQRT2, _TWO_PI = float.fromhex("0x1.6a09e667f3bcdp+0"), float.fromhex("0x1.921fb54442d18p+2")


def new_seed():
    """seed=None of the public functions: 64 bits of NumPy's global generator, so a script that calls np.random.seed stays reproducible"""
    return int.from_bytes(np.random.bytes(8), "little")


def philox_host(seed, row, blocks, tag):
    """Philox4x32-10 (csrc/channel_core.hpp: philox) in NumPy: key = the 64-bit seed, counter = (block lo, block hi, row, tag).
    blocks: integers < 2^64 -> four uint64 arrays holding the block's 32-bit words."""
    blocks = np.asarray(blocks, dtype=np.uint64)
    c0, c1 = blocks & _U32, blocks >> np.uint64(32)
    c2 = np.full(blocks.shape, int(row) & 0xffffffff, dtype=np.uint64)
    c3 = np.full(blocks.shape, int(tag) & 0xffffffff, dtype=np.uint64)
    k0, k1 = int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2     # 32 x 32 bits: no overflow
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1, c3, c0, c2 = p1 & _U32, p0 & _U32, n0, n2
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1, c2, c3


def neg_ln_u_host(k):
    """-ln(k 2^-53) for integers 1 ... 2^53: channel_core.hpp's neg_ln_u, operation by operation"""
    m, e = np.frexp(np.asarray(k, dtype=np.uint64).astype(np.float64))      # m in [1/2, 1): exact
    m, e = m * 2.0, e.astype(np.int64) - 1 - 53
    big = m >= _SQRT2
    m, e = np.where(big, m * 0.5, m), e + big
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full(z.shape, 1.0 / 25.0)
    for d in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * z + 1.0 / d
    lnm = 2.0 * s + 2.0 * s * (z * p)
    ne = (-e).astype(np.float64)
    return ne * _LN2_HI + (ne * _LN2_LO - lnm)


def sincos_2pi_host(k):
    """(cos, sin) of 2 pi k 2^-53 for integers 0 ... 2^53 - 1: channel_core.hpp's sincos_2pi, operation by operation"""
    k = np.asarray(k, dtype=np.uint64)
    octant = (k >> np.uint64(50)).astype(np.int64)
    f = k & np.uint64((1 << 50) - 1)
    f = np.where(octant & 1, np.uint64(1 << 50) - f, f)
    x = (f.astype(np.float64) * 2.0 ** -53) * _TWO_PI
    z = x * x
    ps = np.full(z.shape, 1.0 / 355687428096000.0)
    for c in (-1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0):
        ps = c + z * ps
    sx = x + x * (z * ps)
    pc = np.full(z.shape, -1.0 / 6402373705728000.0)
    for c in (1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0):
        pc = c + z * pc
    cx = 1.0 - (0.5 * z - (z * z) * pc)
    sw = ((octant + 1) & 2) != 0
    ca, sa = np.where(sw, sx, cx), np.where(sw, cx, sx)
    return np.where((octant + 2) & 4, -ca, ca), np.where(octant & 4, -sa, sa)


def uniforms_host(seed, row, blocks):
    """(k1 + 1, k2) of the tag-0 blocks: u1 = (k1 + 1) 2^-53 in (0, 1], u2 = k2 2^-53 in [0, 1)"""
    w0, w1, w2, w3 = philox_host(seed, row, blocks, TAG_NORMAL)
    return ((w0 << np.uint64(21)) | (w1 >> np.uint64(11))) + np.uint64(1), (w2 << np.uint64(21)) | (w3 >> np.uint64(11))


def normals_of_uniforms_host(k1p, k2):
    r = np.sqrt(2.0 * neg_ln_u_host(k1p))
    c, s = sincos_2pi_host(k2)
    return r * c, r * s


def normals_host(seed, row, first, n, complex=True):
    """Elements first ... first + n - 1 of row `row` of the normal stream: complex128 (one block each) or float64 (element i is component
    i & 1 of block i >> 1), the same bits as the device kernels and the C++ emulation draw."""
    first, n = int(first), int(n)
    if n <= 0:
        return np.zeros(0, dtype=np.complex128 if complex else np.float64)
    if complex:
        re, im = normals_of_uniforms_host(*uniforms_host(seed, row, np.uint64(first) + np.arange(n, dtype=np.uint64)))
        z = np.empty(n, dtype=np.complex128)
        z.real, z.imag = re, im
        return z
    b0, b1 = first >> 1, (first + n - 1) >> 1
    re, im = normals_of_uniforms_host(*uniforms_host(seed, row, np.uint64(b0) + np.arange(b1 - b0 + 1, dtype=np.uint64)))
    return np.stack([re, im], axis=1).reshape(-1)[first - 2 * b0:first - 2 * b0 + n]


def random_bits_host(seed, row, first, n):
    """Bits first ... first + n - 1 of row `row` of the bit stream, uint8 0 / 1: bit k & 31 of word k >> 5 of block i >> 7, k = i & 127"""
    first, n = int(first), int(n)
    if n <= 0:
        return np.zeros(0, dtype=np.uint8)
    b0, b1 = first >> 7, (first + n - 1) >> 7
    w = np.stack(philox_host(seed, row, np.uint64(b0) + np.arange(b1 - b0 + 1, dtype=np.uint64), TAG_BITS), axis=1)   # (blocks, 4)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(-1).astype(np.uint8)[first - 128 * b0:first - 128 * b0 + n]


def _per_row(v, nrow):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return np.broadcast_to(v, (nrow,)) if v.size == 1 else v


def awgn_rows_host(x2d, g, sigma, seed, dtype=None, first_index=0, first_row=0):
    """awgn_kernel in NumPy: y[r, i] = g[r] x[r, i] + sigma[r] z(seed, first_row + r, first_index + i), the sum in float64 rounded once
    to `dtype` (default: x's); a real x with a complex dtype gets the complex stream."""
    x2d = np.asarray(x2d)
    dtype = np.dtype(x2d.dtype if dtype is None else dtype)
    nrow, n = x2d.shape
    g, sigma = _per_row(g, nrow), _per_row(sigma, nrow)
    cpx = dtype.kind == "c"
    y = np.empty((nrow, n), dtype=np.complex128 if cpx else np.float64)
    for r in range(nrow):
        z = normals_host(seed, first_row + r, first_index, n, cpx)
        xr = x2d[r].astype(np.complex128 if x2d.dtype.kind == "c" else np.float64)
        if not cpx:
            y[r] = g[r] * xr + sigma[r] * z
        elif x2d.dtype.kind == "c":
            y[r].real, y[r].imag = g[r] * xr.real + sigma[r] * z.real, g[r] * xr.imag + sigma[r] * z.imag
        else:
            y[r].real, y[r].imag = g[r] * xr + sigma[r] * z.real, 0.0 + sigma[r] * z.imag
    return y.astype(dtype)


def awgn_bits_rows_host(bits2d, sigma, seed, first_index=0, first_row=0):
    """awgn_bits_kernel in NumPy: the hard decision of 2 b - 1 + sigma z as bytes -- 1, 0, 2 for an exact zero, 3 for not-a-number"""
    bits2d = np.asarray(bits2d, dtype=np.uint8)
    nrow, n = bits2d.shape
    sigma = _per_row(sigma, nrow)
    out = np.empty((nrow, n), dtype=np.uint8)
    for r in range(nrow):
        v = (2.0 * (bits2d[r] & 1) - 1.0) + sigma[r] * normals_host(seed, first_row + r, first_index, n, False)
        out[r] = np.where(v > 0, 1, np.where(v < 0, 0, np.where(v == 0, 2, 3)))
    return out


def awgn_sigma_host(var, mode, ns, es_n0, var_w_dB=0.0):
    """(g, sigma) of a row of variance var: cpx_awgn's (mode SIGMA_AWGN) or cpx_awgn2's (SIGMA_AWGN2) expressions in the reference's order"""
    var = np.asarray(var, dtype=np.float64)
    with np.errstate(all="ignore"):
        if mode == SIGMA_AWGN:
            return np.ones_like(var), np.sqrt(ns * var * 10 ** (-es_n0 / 10.) / 2.)
        var_w = 10 ** (var_w_dB / 10)
        return np.sqrt(1 / ns * var_w / var * 10 ** (es_n0 / 10.)), np.full(var.shape, np.sqrt(var_w / 2))


def _dp(d):
    """the device address of a DeviceArray / DeviceBytes, or the integer itself"""
    return ctypes.c_void_p((d.ptr if hasattr(d, "ptr") else int(d)) if d is not None else None)


def awgn_rows_dev(xd, yd, n, nrow, seed, g=1.0, sigma=1.0, gd=None, sd=None, x_stride=None, y_stride=None, first_index=0, first_row=0,
                  x_dtype=None, y_dtype=None):
    """yd[r, i] = g xd[r, i] + sigma z (csrc/channel.hip: awgn_kernel).  xd, yd: DeviceArrays (or addresses with x_dtype / y_dtype), yd may be
    xd; strides in elements (default n); gd / sd: DeviceArrays of nrow float64 (awgn_sigma_rows_dev), else the scalars g / sigma."""
    xt, yt = code_of(xd.dtype if x_dtype is None else x_dtype), code_of(yd.dtype if y_dtype is None else y_dtype)
    check(load().skdsp_awgn_rows_dev(_dp(xd), int(n if x_stride is None else x_stride), xt, _dp(yd), int(n if y_stride is None else y_stride), yt, int(n), int(nrow),
                                     _dp(gd), _dp(sd), float(g), float(sigma), int(seed) & (2 ** 64 - 1), int(first_index), int(first_row)))


def awgn_bits_rows_dev(xd, yd, n, nrow, seed, sigma=1.0, sd=None, x_stride=None, y_stride=None, first_index=0, first_row=0):
    """bytes 0 / 1 -> hard decisions as bytes (awgn_bits_kernel); xd, yd: DeviceBytes or addresses at any alignment, strides in bytes"""
    check(load().skdsp_awgn_bits_rows_dev(_dp(xd), int(n if x_stride is None else x_stride), _dp(yd), int(n if y_stride is None else y_stride), int(n), int(nrow),
                                          _dp(sd), float(sigma), int(seed) & (2 ** 64 - 1), int(first_index), int(first_row)))


def awgn_sigma_rows_dev(xd, n, nrow, mode, ns, es_n0, gd, sd, var_w_dB=0.0, x_stride=None, dtype=None):
    """gd[r], sd[r] = cpx_awgn's (SIGMA_AWGN) or cpx_awgn2's (SIGMA_AWGN2) gain and sigma from np.var of row r, left on the device; the
    powers of ten are computed here as the reference writes them."""
    if mode == SIGMA_AWGN:
        p, var_w = 10 ** (-es_n0 / 10.), 0.0
    else:
        p, var_w = 10 ** (es_n0 / 10.), 10 ** (var_w_dB / 10)
    check(load().skdsp_awgn_sigma_rows_dev(_dp(xd), int(n if x_stride is None else x_stride), int(n), int(nrow), code_of(xd.dtype if dtype is None else dtype), int(mode),
                                           float(ns), float(p), float(var_w), _dp(gd), _dp(sd)))


def random_bits_rows_dev(yd, n, nrow, seed, y_stride=None, first_index=0, first_row=0):
    """yd[r, i] = bit first_index + i of row first_row + r of the bit stream, one byte each (randbits_kernel)"""
    check(load().skdsp_random_bits_rows_dev(_dp(yd), int(n if y_stride is None else y_stride), int(n), int(nrow), int(seed) & (2 ** 64 - 1), int(first_index), int(first_row)))


def pn_rows_dev(period_d, q, yd, n, nrow, phases_d=None, y_stride=None, first_index=0):
    """yd[r, i] = period[(phases[r] + first_index + i) mod q] (pn_kernel); period_d: q bytes, phases_d: nrow int64 or None, on the device"""
    check(load().skdsp_pn_rows_dev(_dp(period_d), int(q), _dp(phases_d), _dp(yd), int(n if y_stride is None else y_stride), int(n), int(nrow), int(first_index)))


# --------------------------------------------------------------------------
# OFDM (csrc/ofdm.hip): ofdm_tx / ofdm_rx / chan_est_equalize over the rows of a frame set
# --------------------------------------------------------------------------
def ofdm_tx_symbols(nsym, npb):
    """symbols a row of nsym data symbols leaves the transmitter with"""
    return nsym + nsym // (npb - 1) + 1 if npb > 0 else nsym


def ofdm_rx_data_symbols(nsym, npb):
    """data symbols among nsym received ones"""
    return nsym - (nsym + npb - 1) // npb if npb > 0 else nsym


def _hht_ptr(hht, nf):
    """the known channel on the filled carriers as the library takes it: nf complex128 on the host (the array is returned to keep it alive)"""
    if hht is None:
        return None, ctypes.c_void_p(0)
    hht = np.ascontiguousarray(hht, dtype=np.complex128)
    if hht.shape != (nf,):
        raise ValueError("ofdm: the channel table holds one value per filled carrier")
    return hht, _ptr(hht)


def ofdm_tx_rows_dev(xd, yd, nsym, nrow, nf, nc, npb=0, cp=False, ncp=0, x_stride=None, y_stride=None, dtype=None):
    """yd[r] = ofdm_tx of the nsym nf symbols of xd[r] (csrc/ofdm.hip: ofdm_tx_kernel).  xd, yd: DeviceArrays (or addresses with dtype) of
    complex64 / complex128; strides in elements (default: the rows back to back)."""
    n_out = ofdm_tx_symbols(nsym, npb) * (nc + (ncp if cp else 0))
    check(load().skdsp_ofdm_tx_rows_dev(_dp(xd), int(nsym * nf if x_stride is None else x_stride), int(nsym), int(nrow), code_of(xd.dtype if dtype is None else dtype),
                                        int(nf), int(nc), int(npb), int(bool(cp)), int(ncp), _dp(yd), int(n_out if y_stride is None else y_stride)))


def ofdm_rx_rows_dev(xd, zd, nsym, nrow, nf, nc, npb=0, cp=False, ncp=0, alpha=0.95, hht=None, hd=None, x_stride=None, z_stride=None, dtype=None):
    """zd[r] = the equalised carriers of the nsym received symbols of xd[r] (ofdm_rx_kernel, then the estimator kernels for npb > 0); hht: the
    known channel on the nf filled carriers (a host array) or None; hd: nrow nf complex128 for the rows' last estimates (npb > 0)."""
    keep, hp = _hht_ptr(hht, nf)
    n_in, n_out = nsym * (nc + ncp if cp else nc), ofdm_rx_data_symbols(nsym, npb) * nf
    check(load().skdsp_ofdm_rx_rows_dev(_dp(xd), int(n_in if x_stride is None else x_stride), int(nsym), int(nrow), code_of(xd.dtype if dtype is None else dtype), int(nf),
                                        int(nc), int(npb), int(bool(cp)), int(ncp), float(alpha), hp, _dp(zd), int(n_out if z_stride is None else z_stride), _dp(hd)))
    del keep


def ofdm_equalize_rows_dev(zd, od, nsym, nrow, nf, npb, alpha, hd, hht=None, z_stride=None, out_stride=None, dtype=None):
    """chan_est_equalize on the rows of zd, nsym symbols of nf carriers each (ofdm_chanest_kernel, ofdm_equalize_kernel): the data rows to od,
    the rows' last estimates to hd (nrow nf complex128)"""
    keep, hp = _hht_ptr(hht, nf)
    check(load().skdsp_ofdm_equalize_rows_dev(_dp(zd), int(nsym * nf if z_stride is None else z_stride), int(nsym), int(nrow), code_of(zd.dtype if dtype is None else dtype),
                                              int(nf), int(npb), float(alpha), hp, _dp(od), int(ofdm_rx_data_symbols(nsym, npb) * nf if out_stride is None else out_stride),
                                              _dp(hd)))
    del keep


def ofdm_tx_rows(x2d, nf, nc, npb, cp, ncp):
    """host arrays through skdsp_ofdm_tx_rows: x2d (nrow, nsym nf) complex64 / complex128, contiguous"""
    nrow, nsym = x2d.shape[0], x2d.shape[1] // nf
    y = np.empty((nrow, ofdm_tx_symbols(nsym, npb) * (nc + (ncp if cp else 0))), dtype=x2d.dtype)
    check(load().skdsp_ofdm_tx_rows(_ptr(x2d), nsym, nrow, code_of(x2d.dtype), int(nf), int(nc), int(npb), int(bool(cp)), int(ncp), _ptr(y)))
    return y


def ofdm_rx_rows(x2d, nsym, nf, nc, npb, cp, ncp, alpha, hht):
    """host arrays through skdsp_ofdm_rx_rows: x2d (nrow, nsym symbols) -> z (nrow, ndata nf) of x2d's dtype, h (nrow, nf) complex128 (npb > 0) or None"""
    nrow = x2d.shape[0]
    z = np.empty((nrow, ofdm_rx_data_symbols(nsym, npb) * nf), dtype=x2d.dtype)
    h = np.empty((nrow, nf), dtype=np.complex128) if npb > 0 else None
    keep, hp = _hht_ptr(hht, nf)
    check(load().skdsp_ofdm_rx_rows(_ptr(x2d), int(nsym), nrow, code_of(x2d.dtype), int(nf), int(nc), int(npb), int(bool(cp)), int(ncp), float(alpha), hp, _ptr(z),
                                    _ptr(h) if h is not None else ctypes.c_void_p(0)))
    del keep
    return z, h


def ofdm_equalize_rows(z3d, npb, alpha, hht):
    """host arrays through skdsp_ofdm_equalize_rows: z3d (nrow, nsym, nf) -> (nrow, ndata, nf) of z3d's dtype, h (nrow, nf) complex128"""
    nrow, nsym, nf = z3d.shape
    out = np.empty((nrow, ofdm_rx_data_symbols(nsym, npb), nf), dtype=z3d.dtype)
    h = np.empty((nrow, nf), dtype=np.complex128)
    keep, hp = _hht_ptr(hht, nf)
    check(load().skdsp_ofdm_equalize_rows(_ptr(z3d), nsym, nrow, code_of(z3d.dtype), nf, int(npb), float(alpha), hp, _ptr(out), _ptr(h)))
    del keep
    return out, h



# --------------------------------------------------------------------------
# symbol-error tools (csrc/symerr.hip, csrc/symerr_core.hpp): the lag-window correlation behind xcorr / qam_sep and the fused count
# --------------------------------------------------------------------------
SYM_QAM, SYM_QPSK, SYM_BPSK = 0, 1, 2
QAM_LEVELS = {'qpsk': 2, '16qam': 4, '64qam': 8, '256qam': 16}


def lag_corr_len(n, n_lags):
    """(number of lags, first lag) that xcorr keeps of streams of n samples: K = 2 (n // 2), min(2 n_lags + 1, K) lags from -min(n_lags, K / 2)"""
    nl, l0 = ctypes.c_int64(0), ctypes.c_int64(0)
    check(load().skdsp_lag_corr_len(int(n), int(n_lags), ctypes.byref(nl), ctypes.byref(l0)))
    return nl.value, l0.value


def _stream(x, what):
    """x as the symbol-error kernels take it: float32 / complex64 / float64 / complex128 kept, integers as float64, anything else numeric widened"""
    x = np.asarray(x)
    if x.dtype.kind in "biu":
        x = x.astype(np.float64)
    if x.dtype.kind not in "fc":
        raise TypeError("%s: a numeric array (got %s)" % (what, x.dtype))
    if x.dtype not in _CODE_OF:
        x = x.astype(np.complex128 if x.dtype.kind == "c" else np.float64)
    return np.ascontiguousarray(x)


def qam_quantise_host(x, levels):
    """qam_sep's quantiser (digitalcom.py:525-536), componentwise: 2 clip(rint((M - 1)(v + 1) / 2), 0, M - 1) - (M - 1), float64 / complex128"""
    x = np.asarray(x)
    def comp(v):
        q = np.rint((levels - 1) * (v.astype(np.float64) + 1.0) / 2.)
        q = np.where(q > levels - 1, float(levels - 1), q)
        q = np.where(q < 0, 0.0, q)
        return 2 * q - (levels - 1)
    if x.dtype.kind == "c":
        return comp(x.real) + 1j * comp(x.imag)
    return comp(x) + 1j * comp(np.zeros(x.shape))


def lag_corr(a, b, n_lags, quant_levels=0):
    """(R complex128, lags int64, E1, E2): R[i] = sum_n a[(n + lags[i]) mod K] conj(b[n]) over the first K = 2 (len(a) // 2) samples of both streams,
    unnormalised, float64 sums in a fixed order (csrc/symerr.hip: lagcorr_kernel); quant_levels M > 0: a through qam_sep's quantiser at the load"""
    a, b = _stream(a, "lag_corr"), _stream(b, "lag_corr")
    if a.ndim != 1 or b.ndim != 1:
        raise ValueError("lag_corr: one-dimensional streams")
    K = 2 * (a.size // 2)
    if b.size < K:
        raise ValueError("lag_corr: the second stream holds fewer than K = %d samples" % K)
    nl, _ = lag_corr_len(a.size, n_lags)
    lags, r, e = np.zeros(nl, dtype=np.int64), np.zeros(nl, dtype=np.complex128), np.zeros(2)
    check(load().skdsp_lag_corr(_ptr(a), code_of(a.dtype), _ptr(b), code_of(b.dtype), a.size, int(n_lags), int(quant_levels), _ptr(lags), _ptr(r), _ptr(e)))
    return r, lags, float(e[0]), float(e[1])


def lag_corr_host(a, b, n_lags, quant_levels=0):
    """lag_corr by direct summation in NumPy (no GPU): the yardstick of the kernel at test sizes (O(K lags))"""
    a, b = _stream(a, "lag_corr"), _stream(b, "lag_corr")
    K = 2 * (a.size // 2)
    half = K // 2
    nl, l0 = (K, -half) if n_lags >= half else (2 * n_lags + 1, -n_lags)
    a = a[:K].astype(np.complex128) if not quant_levels else qam_quantise_host(a[:K], quant_levels)
    b = b[:K].astype(np.complex128)
    lags = l0 + np.arange(nl, dtype=np.int64)
    r = np.array([np.sum(np.roll(a, -int(l)) * np.conj(b)) for l in lags], dtype=np.complex128).reshape(nl)
    return r, lags, float(np.sum(a.real ** 2 + a.imag ** 2)), float(np.sum(b.real ** 2 + b.imag ** 2))


def lag_corr_dev(ad, bd, n, n_lags, rd, ed, quant_levels=0, a_dtype=None, b_dtype=None):
    """Device-resident form: ad / bd hold the streams (DeviceArray or pointers with a_dtype / b_dtype), rd receives min(2 n_lags + 1, K) complex128,
    ed the two energies (float64)"""
    check(load().skdsp_lag_corr_dev(_dp(ad), code_of(a_dtype or ad.dtype), _dp(bd), code_of(b_dtype or bd.dtype), int(n), int(n_lags), int(quant_levels), _dp(rd), _dp(ed)))


def _sym_mode_check(mode, levels, kphase):
    if mode not in (SYM_QAM, SYM_QPSK, SYM_BPSK):
        raise ValueError("sym_count: mode SYM_QAM, SYM_QPSK or SYM_BPSK")
    if mode == SYM_QAM and levels not in (2, 4, 8, 16):
        raise ValueError("sym_count: QAM of 2, 4, 8 or 16 levels per component")
    if int(kphase) != kphase or not 0 <= kphase <= (1 if mode == SYM_BPSK else 3):
        raise ValueError("sym_count: the rotation is 0 ... 3 (BPSK: 0 or 1)")


def _rot_host(x, mode, kphase):
    """x (1j)^k as swaps and negations (BPSK: (-1)^k on the real part)"""
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    if mode == SYM_BPSK:
        return (-re if kphase & 1 else re), im
    return [(re, im), (-im, re), (-re, -im), (im, -re)][kphase]


def sym_count_rows_host(tx2d, x2d, mode, levels=0, kphase=0, start=0, step=1, n=None, t0=0, r0=0):
    """sym_count_rows in NumPy (no GPU): int64 (nrow, 4) -- the sums of the mode, then the symbols that break a precondition (left out of the sums)"""
    _sym_mode_check(mode, levels, kphase)
    tx, x = np.atleast_2d(_stream(tx2d, "sym_count")), np.atleast_2d(_stream(x2d, "sym_count"))
    if n is None:
        n = min(tx.shape[1] - t0, sym_count(x.shape[1], start, step) - r0)
    t = tx[:, t0:t0 + n].astype(np.complex128)
    r = x[:, start + r0 * step::step][:, :n].astype(np.complex128)
    out = np.zeros((tx.shape[0], 4), dtype=np.int64)
    with np.errstate(all="ignore"):
        if mode == SYM_QAM:
            ok = np.isfinite(t.real) & np.isfinite(t.imag) & np.isfinite(r.real) & np.isfinite(r.imag) & (t.real == np.rint(t.real)) & (t.imag == np.rint(t.imag))
            qr, qi = _rot_host(qam_quantise_host(r, levels), mode, kphase)
            out[:, 0] = np.sum(ok & ((qr != t.real) | (qi != t.imag)), axis=1)
        else:
            xr, xi = _rot_host(r, mode, kphase)
            parts = [(t.real, xr)] if mode == SYM_BPSK else [(t.real, xr), (t.imag, xi)]
            ok = np.isfinite(xr) if mode == SYM_BPSK else np.isfinite(xr) & np.isfinite(xi)
            halves = [((a + 1) / 2, (b + 1) / 2) for a, b in parts]
            for ha, hb in halves:
                ok = ok & (np.abs(ha) < 32768) & (np.abs(hb) < 32768)
            errs = [np.where(ok, ha, 0).astype(np.int16) ^ np.where(ok, hb, 0).astype(np.int16) for ha, hb in halves]
            out[:, 0] = np.sum(errs[0].astype(np.int64), axis=1)
            if mode == SYM_QPSK:
                out[:, 1] = np.sum(errs[1].astype(np.int64), axis=1)
                out[:, 2] = np.sum((errs[0] | errs[1]).astype(np.int64), axis=1)
        out[:, 3] = np.sum(~ok, axis=1)
    return out


def sym_count_rows(tx2d, x2d, mode, levels=0, kphase=0, start=0, step=1, n=None, t0=0, r0=0):
    """int64 (nrow, 4) per row of two 2-D arrays, in one launch (csrc/symerr.hip: symcount_kernel): tx symbol i = tx2d[r, t0 + i], rx symbol i =
    x2d[r, start + (r0 + i) step] rotated by (1j)^kphase; the sums of the mode (skdsp.h), then the count of symbols that break a precondition"""
    _sym_mode_check(mode, levels, kphase)
    tx, x = _stream(tx2d, "sym_count"), _stream(x2d, "sym_count")
    if tx.ndim != 2 or x.ndim != 2 or tx.shape[0] != x.shape[0]:
        raise ValueError("sym_count_rows: two 2-D arrays with the same number of rows")
    if n is None:
        n = min(tx.shape[1] - t0, sym_count(x.shape[1], start, step) - r0)
    if n < 0 or t0 < 0 or r0 < 0 or t0 + n > tx.shape[1] or (n and start + (r0 + n - 1) * step >= x.shape[1]):
        raise ValueError("sym_count_rows: symbols beyond a row")
    counts = np.zeros((tx.shape[0], 4), dtype=np.int64)
    check(load().skdsp_sym_count_rows(_ptr(tx), code_of(tx.dtype), tx.shape[1], int(t0), _ptr(x), code_of(x.dtype), x.shape[1], int(start), int(step), int(r0), int(n),
                                      tx.shape[0], int(mode), int(levels), int(kphase), _ptr(counts)))
    return counts


def sym_count_rows_dev(tx, tx_dtype, tx_stride, t0, x, x_dtype, x_stride, start, step, r0, n, nrow, mode, levels, kphase, counts):
    """Device-resident form: tx / x / counts are DeviceArray / DeviceBytes or pointers; counts receives nrow x int64[4] (zeroed by the call)"""
    check(load().skdsp_sym_count_rows_dev(_dp(tx), code_of(tx_dtype), int(tx_stride), int(t0), _dp(x), code_of(x_dtype), int(x_stride), int(start), int(step), int(r0),
                                          int(n), int(nrow), int(mode), int(levels), int(kphase), _dp(counts)))


# --------------------------------------------------------------------------
# Pulse shaping and matched filtering over frame sets (csrc/pulse.hip): the two filtering stages of a single-carrier BER loop
# --------------------------------------------------------------------------
PULSE_MAX_TAPS, PULSE_MAX_RATE = 2049, 64


def pulse_served(ntaps, rate):
    """does the kernel pair take this filter length and this ns / step?  (outside: the C calls return SKDSP_ERR_UNSUPPORTED)"""
    return 1 <= int(ntaps) <= PULSE_MAX_TAPS and 1 <= int(rate) <= PULSE_MAX_RATE


def _pulse_taps(b):
    b = np.ascontiguousarray(b, dtype=np.float64)
    if b.ndim != 1 or b.size < 1:
        raise ValueError("pulse: b must be a one-dimensional array of at least one real tap")
    return b


def _pulse_rows(x2d, what):
    x = _stream(x2d, what)
    if x.ndim != 2:
        raise ValueError("%s: a 2-D array, one frame per row" % what)
    return x


def _planes(x):
    """the float64 components of a widened signal: [re] or [re, im]"""
    if x.dtype.kind == "c":
        return [np.ascontiguousarray(x.real, dtype=np.float64), np.ascontiguousarray(x.imag, dtype=np.float64)]
    return [x.astype(np.float64)]


def _from_planes(planes, dtype):
    """one rounding to the output dtype"""
    if len(planes) == 1:
        return planes[0].astype(dtype)
    y = np.empty(planes[0].shape, dtype=np.complex128)
    y.real, y.imag = planes
    return y.astype(dtype)


def pulse_shape_rows_host(x2d, b, ns, scale=None):
    """PulseKernel.shape_rows in NumPy (no GPU), the kernel's arithmetic operation for operation: per row lfilter(b, 1, upsample(x, ns)) with float64
    products and sums, acc = b x + acc from the oldest symbol to the newest and from +0, real and imaginary parts apart, the optional factor once behind
    the sum, one rounding to x's dtype.  Vectorised over rows, symbols and phases; the loop runs over the taps of a phase."""
    x, b, ns = _pulse_rows(x2d, "pulse_shape_rows"), _pulse_taps(b), int(ns)
    if ns < 1:
        raise ValueError("pulse_shape_rows: need ns >= 1")
    nrow, n = x.shape
    J = -(-b.size // ns)
    H = J - 1
    out = []
    for s in _planes(x):
        sp = np.zeros((nrow, H + n), dtype=np.float64)
        sp[:, H:] = s
        acc = np.zeros((nrow, n, ns), dtype=np.float64)
        for j in range(J - 1, -1, -1):
            pm = min(ns, b.size - j * ns)          # the phases that have a tap j
            prod = b[j * ns:j * ns + pm][None, None, :] * sp[:, H - j:H - j + n, None]
            acc[:, :, :pm] = prod + acc[:, :, :pm]
        if scale is not None:
            acc = acc * np.float64(scale)
        out.append(acc.reshape(nrow, n * ns))
    return _from_planes(out, x.dtype)


def pulse_mf_rows_host(x2d, b, start=0, step=1):
    """PulseKernel.mf_rows in NumPy (no GPU), the kernel's arithmetic operation for operation: per row lfilter(b, 1, x)[start::step], acc = b x + acc from
    the oldest sample to the newest.  Vectorised over rows and outputs; the loop runs over the taps."""
    x, b, start, step = _pulse_rows(x2d, "matched_filter_rows"), _pulse_taps(b), int(start), int(step)
    nrow, n = x.shape
    n_out = sym_count(n, start, step)
    P = b.size
    out = []
    for s in _planes(x):
        xp = np.zeros((nrow, P - 1 + n), dtype=np.float64)
        xp[:, P - 1:] = s
        acc = np.zeros((nrow, n_out), dtype=np.float64)
        for i in range(P - 1, -1, -1):
            prod = b[i] * xp[:, start + P - 1 - i::step][:, :n_out]
            acc = prod + acc
        out.append(acc)
    return _from_planes(out, x.dtype)


class PulseKernel:
    """A pulse handle (csrc/pulse.hip) for one (real taps, signal dtype) pair: shaping and the decimating matched filter over the rows of a frame set,
    every row from rest, in the one arithmetic recipe pulse_shape_rows_host / pulse_mf_rows_host restate.  Creating it needs no device."""

    def __init__(self, b, dtype):
        b = _pulse_taps(b)
        self.ntaps, self.dtype, self.code = int(b.size), np.dtype(dtype), code_of(dtype)
        h = ctypes.c_void_p(0)
        check(load().skdsp_pulse_create(_ptr(b), self.ntaps, self.code, ctypes.byref(h)))
        self.h = h.value
        self._fin = weakref.finalize(self, _destroy, self.h)

    @staticmethod
    def mf_out_len(n, start=0, step=1):
        v = ctypes.c_int64(0)
        check(load().skdsp_pulse_mf_out_len(int(n), int(start), int(step), ctypes.byref(v)))
        return v.value

    @staticmethod
    def _scale(scale):
        return None if scale is None else ctypes.byref(ctypes.c_double(float(scale)))

    def _rows(self, x2d, what):
        x = _pulse_rows(x2d, what)
        if x.dtype != self.dtype:
            raise TypeError("%s: the handle was made for %s signals (got %s)" % (what, self.dtype, x.dtype))
        return x

    # host arrays -------------------------------------------------------
    def shape_rows(self, x2d, ns, scale=None):
        """(nrow, n) -> (nrow, n ns) of the same dtype"""
        x = self._rows(x2d, "pulse_shape_rows")
        y = np.empty((x.shape[0], x.shape[1] * int(ns)), dtype=x.dtype)
        check(load().skdsp_pulse_shape_rows(ctypes.c_void_p(self.h), _ptr(x), x.shape[1], x.shape[0], int(ns), self._scale(scale), _ptr(y)))
        return y

    def mf_rows(self, x2d, start=0, step=1):
        """(nrow, n) -> (nrow, len(row[start::step])) of the same dtype"""
        x = self._rows(x2d, "matched_filter_rows")
        y = np.empty((x.shape[0], sym_count(x.shape[1], int(start), int(step))), dtype=x.dtype)
        check(load().skdsp_pulse_mf_rows(ctypes.c_void_p(self.h), _ptr(x), x.shape[1], x.shape[0], int(start), int(step), _ptr(y)))
        return y

    # device arrays -----------------------------------------------------
    def shape_rows_dev(self, xd, yd, n, nrow, ns, scale=None, x_stride=None, y_stride=None):
        """xd, yd: DeviceArrays or addresses of the handle's dtype; strides in elements (default n and n ns); the two must not overlap"""
        check(load().skdsp_pulse_shape_rows_dev(ctypes.c_void_p(self.h), _dp(xd), int(n), int(nrow), int(n if x_stride is None else x_stride), int(ns),
                                                self._scale(scale), _dp(yd), int(n * ns if y_stride is None else y_stride)))

    def mf_rows_dev(self, xd, yd, n, nrow, start=0, step=1, x_stride=None, y_stride=None):
        """strides in elements (default n and the output row length); the two must not overlap"""
        n_out = sym_count(int(n), int(start), int(step))
        check(load().skdsp_pulse_mf_rows_dev(ctypes.c_void_p(self.h), _dp(xd), int(n), int(nrow), int(n if x_stride is None else x_stride), int(start), int(step),
                                             _dp(yd), int(n_out if y_stride is None else y_stride)))


# --------------------------------------------------------------------------
# Carrier phase tracking and its impairment helpers over frame sets (csrc/carrier.hip): synchronization.DD_carrier_sync / phase_step / time_step
# --------------------------------------------------------------------------
CAR_OUTPUTS = ("z_prime", "a_hat", "e_phi", "theta_h")
_PIO2_1, _PIO2_2, _PIO2_3 = (float.fromhex(h) for h in ("0x1.921fb54442d10p+0", "0x1.08d313198a2e0p-49", "0x1.b839a252049c1p-104"))
_TWO_OVER_PI, _PI = float.fromhex("0x1.45f306dc9c883p-1"), float.fromhex("0x1.921fb54442d18p+1")
_ATAN_CUTS = tuple(float.fromhex(h) for h in ("0x1.936bb8c5b2da2p-4", "0x1.36a08355c63dcp-2", "0x1.11ab7190834ecp-1", "0x1.a43002ae42850p-1"))
_ATAN_TAB = np.array([[float.fromhex(h) for h in row] for row in (          # k pi / 16, cos and sin of it, (hi, lo) each: symmap_core.hpp's atan2_rn
    ("0x0p+0", "0x0p+0", "0x1p+0", "0x0p+0", "0x0p+0", "0x0p+0"),
    ("0x1.921fb54442d18p-3", "0x1.1a62633145c07p-57", "0x1.f6297cff75cb0p-1", "0x1.562172a361fd3p-56", "0x1.8f8b83c69a60bp-3", "-0x1.26d19b9ff8d82p-57"),
    ("0x1.921fb54442d18p-2", "0x1.1a62633145c07p-56", "0x1.d906bcf328d46p-1", "0x1.457e610231ac2p-56", "0x1.87de2a6aea963p-2", "-0x1.72cedd3d5a610p-57"),
    ("0x1.2d97c7f3321d2p-1", "0x1.a79394c9e8a0ap-56", "0x1.a9b66290ea1a3p-1", "0x1.9f630e8b6dac8p-60", "0x1.1c73b39ae68c8p-1", "0x1.b25dd267f6600p-55"),
    ("0x1.921fb54442d18p-1", "0x1.1a62633145c07p-55", "0x1.6a09e667f3bcdp-1", "-0x1.bdd3413b26456p-55", "0x1.6a09e667f3bcdp-1", "-0x1.bdd3413b26456p-55"))])
_PIO2_DD = (float.fromhex("0x1.921fb54442d18p+0"), float.fromhex("0x1.1a62633145c07p-54"))
_PI_DD = (float.fromhex("0x1.921fb54442d18p+1"), float.fromhex("0x1.1a62633145c07p-53"))


def _sincos_octant_host(x):
    """(sin, cos) of x in [0, pi / 4]: channel_core.hpp's sincos_octant, operation by operation"""
    z = x * x
    ps = np.full(z.shape, 1.0 / 355687428096000.0)
    for c in (-1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0):
        ps = c + z * ps
    pc = np.full(z.shape, -1.0 / 6402373705728000.0)
    for c in (1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0):
        pc = c + z * pc
    return x + x * (z * ps), 1.0 - (0.5 * z - (z * z) * pc)


def sincos_rad_host(x):
    """(sin, cos) of float64 radians, |x| <= 8 (NaN beyond): carrier_core.hpp's sincos_rad, operation by operation"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        ax = np.where(x < 0.0, -x, x)
        ok = ax <= 8.0
        axs = np.where(ok, ax, 0.0)
        k = (axs * _TWO_OVER_PI + 0.5).astype(np.int64)
        dk = k.astype(np.float64)
        t1 = axs - dk * _PIO2_1
        p2 = dk * _PIO2_2
        h0 = t1 - p2
        bb = h0 - t1
        l0 = (t1 - (h0 - bb)) + (-p2 - bb)
        l1 = l0 - dk * _PIO2_3
        h = h0 + l1
        lo = l1 - (h - h0)
        sh, ch = _sincos_octant_host(np.where(h < 0.0, -h, h))
        sh = np.where(h < 0.0, -sh, sh)
        sr, cr = sh + lo * ch, ch - lo * sh
        q = k & 3
        sa, ca = np.where(q & 1, cr, sr), np.where(q & 1, sr, cr)
        sa = np.where(q & 2, -sa, sa)
        ca = np.where((q == 1) | (q == 2), -ca, ca)
        bad = (x - x) / (x - x)
        return np.where(ok, np.where(x < 0.0, -sa, sa), bad), np.where(ok, ca, bad)


def wrap_2pi_host(a):
    """np.mod(a, 2 pi) spelled out as carrier_core.hpp's wrap_2pi computes it: the exact remainder, plus 2 pi when negative, +0 when zero"""
    with np.errstate(invalid="ignore"):
        m = np.fmod(np.asarray(a, dtype=np.float64), _TWO_PI)
        return np.where(m != 0.0, np.where(m < 0.0, m + _TWO_PI, m), 0.0)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """(p, a b - p): the second word is what fma(a, b, -p) returns, from Dekker's split (no overflow or underflow in the partial products)"""
    p = a * b
    ca, cb = a * 134217729.0, b * 134217729.0
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_dot(a, ch, cl, b, dh, dl, sign):
    ph, pl = _two_prod(a, ch)
    qh, ql = _two_prod(b, dh)
    sh, sl = _two_sum(ph, sign * qh)
    return _two_sum(sh, sl + (pl + sign * ql) + (a * cl + sign * (b * dl)))


def _dd_sub(ah, al, bh, bl):
    sh, sl = _two_sum(ah, -bh)
    return _two_sum(sh, sl + (al - bl))


def atan2_rn_host(y, x):
    """symmap_core.hpp's atan2_rn, operation by operation (its fused multiply-adds are exact error terms, formed here by Dekker's product: for
    operands between 2^-400 and 2^400 in magnitude)"""
    y, x = (np.array(v, dtype=np.float64) for v in np.broadcast_arrays(y, x))
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        swap = ay > ax
        hi, lo = np.where(swap, ay, ax), np.where(swap, ax, ay)
        f = np.where(hi > 2.0 ** 1000, 2.0 ** -200, np.where(hi < 2.0 ** -900, 2.0 ** 200, 1.0))
        hi, lo = hi * f, lo * f
        q = lo / hi
        k = 4 - sum((q < c).astype(np.int64) for c in _ATAN_CUTS)
        ah, al, ch, cl, sh, sl = (_ATAN_TAB[k, i] for i in range(6))
        nh, nl = _dd_dot(lo, ch, cl, hi, sh, sl, -1.0)
        dh, dl = _dd_dot(hi, ch, cl, lo, sh, sl, 1.0)
        u = nh / dh
        ph, pl = _two_prod(u, dh)
        rem = (nh - ph) - pl
        u2 = u * u
        ul = ((rem + nl) - u * dl) / dh / (1.0 + u2)
        t = np.full(u.shape, -1.0 / 19.0)
        for c in (1.0 / 17.0, -1.0 / 15.0, 1.0 / 13.0, -1.0 / 11.0, 1.0 / 9.0, -1.0 / 7.0, 1.0 / 5.0, -1.0 / 3.0):
            t = t * u2 + c
        tail = t * u2 * u
        s1h, s1l = _two_sum(ah, u)
        gh, gl = _two_sum(s1h, s1l + (al + ul + tail))
        wh, wl = _dd_sub(_PIO2_DD[0], _PIO2_DD[1], gh, gl)
        gh, gl = np.where(swap, wh, gh), np.where(swap, wl, gl)
        wh, wl = _dd_sub(_PI_DD[0], _PI_DD[1], gh, gl)
        gh = np.where(np.signbit(x), wh, gh)
        out = np.copysign(gh, y)
        out = np.where(x == 0.0, np.copysign(0.5 * _PI, y), out)
        return np.where(y == 0.0, np.copysign(np.where(np.signbit(x), _PI, 0.0), y), out)


def carrier_family(mod_type):
    if mod_type == "MPSK":
        return MPSK
    if mod_type == "MQAM":
        return QAM
    raise ValueError("mod_type must be 'MPSK' or 'MQAM'")


def carrier_gains(BnTs, zeta):
    """(K1, K2) of one loop bandwidth, in the reference's statements (synchronization.py:207-211) on Python floats"""
    BnTs, zeta = float(BnTs), float(zeta)
    Ns, Kp, K0 = 1, 1, 1
    K1 = 4 * zeta / (zeta + 1 / (4 * zeta)) * BnTs / Ns / Kp / K0
    K2 = 4 / (zeta + 1 / (4 * zeta)) ** 2 * (BnTs / Ns) ** 2 / Kp / K0
    return K1, K2


def carrier_gains_rows(BnTs, zeta, nrow):
    """(k1, k2, gains): the scalars and None for one bandwidth, else (0, 0, float64 (nrow, 2)) for one per row"""
    b = np.asarray(BnTs, dtype=np.float64)
    if b.ndim == 0:
        return carrier_gains(b, zeta) + (None,)
    if b.shape != (nrow,):
        raise ValueError("BnTs: a scalar, or one value per row")
    return 0.0, 0.0, np.ascontiguousarray([carrier_gains(v, zeta) for v in b], dtype=np.float64).reshape(nrow, 2)


def carrier_table(fam, mod):
    """(inv_sqrt2, tab_re, tab_im): 1 / np.sqrt(2) (what NumPy's complex quotient by np.sqrt(2) multiplies with) and, for MPSK above 4, the decision
    points np.exp(1j 2 pi a / M) in the reference's own operations; (None, None) otherwise"""
    inv = float(1.0 / np.sqrt(2))
    if fam == MPSK and mod > 4:
        pts = np.array([np.exp(1j * 2 * np.pi * np.complex128(a) / mod) for a in range(mod)], dtype=np.complex128)
        return inv, np.ascontiguousarray(pts.real), np.ascontiguousarray(pts.imag)
    return inv, None, None


def carrier_step_host(fam, mod, type, open_loop, k1, k2, r, back, theta, vi, xr, xi, table):
    """One symbol of every row: carrier_core.hpp's step in NumPy, operation by operation.  k1, k2, r, back, theta, vi, xr, xi: float64 arrays, one
    entry per row; table: carrier_table's.  Returns (zr, zi, ar, ai, e, theta_h, theta, vi), zr / zi before the MQAM factor `back`."""
    inv_sqrt2, tab_re, tab_im = table
    with np.errstate(all="ignore"):
        if fam == QAM:
            xr, xi = xr * r, xi * r
        s, c = sincos_rad_host(theta)
        d = -s
        zr, zi = xr * c - xi * d, xr * d + xi * c
        if fam == MPSK:
            if mod == 2:
                ar, ai = np.sign(zr) + 0.0, np.zeros_like(zr)
            elif mod == 4:
                ar, ai = np.sign(zr) * inv_sqrt2, np.sign(zi) * inv_sqrt2
            else:
                kk = np.rint(atan2_rn_host(zi, zr) * float(mod) / 2.0 / _PI)
                idx = np.where(kk == kk, kk, 0.0).astype(np.int64) & (mod - 1)
                ar, ai = tab_re[idx], tab_im[idx]
        else:
            x_m = 1 if mod == 2 else (1 << (sym_bits(QAM, mod) // 2)) - 1

            def level(v):
                k = np.rint((v + float(x_m)) * 0.5)
                return np.where(k > 0.0, np.minimum(k, float(x_m)), 0.0)
            ar, ai = 2.0 * level(zr) - x_m, 2.0 * level(zi) - x_m
        if type == 0:
            e = zi * ar - zr * ai
        elif type == 1:
            se, ce = sincos_rad_host(atan2_rn_host(zi, zr) - atan2_rn_host(ai, ar))
            e = atan2_rn_host(se, ce)
        else:
            abr, abi = np.abs(ar), np.abs(ai)
            first = abr >= abi
            rat1, rat2 = ai / ar, ar / ai
            e1 = (zi - zr * rat1) * (1.0 / (ar + ai * rat1))
            e2 = (zi * rat2 - zr) * (1.0 / (ai + ar * rat2))
            e = np.where(first, np.where((abr == 0.0) & (abi == 0.0), zi / abr, e1), e2)
        vp = k1 * e
        vi = vi + k2 * e
        th = wrap_2pi_host(theta + (vp + vi))
    return zr, zi, ar, ai, e, th, (np.zeros_like(th) if open_loop else th), vi


def _car_outputs(outputs):
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outputs or any(o not in CAR_OUTPUTS for o in outputs) or len(set(outputs)) != len(outputs):
        raise ValueError("outputs: a non-empty selection of %r" % (CAR_OUTPUTS,))
    return outputs, sum(1 << CAR_OUTPUTS.index(o) for o in outputs)


def _car_args(x2d, fam, mod, type, start, step):
    sym_bits(fam, mod)
    if type not in (0, 1, 2):
        raise ValueError("type must be 0, 1 or 2")
    x = np.asarray(x2d)
    if x.ndim != 2:
        raise ValueError("DD_carrier_sync_rows: a 2-D array, one frame per row")
    if x.dtype not in (np.complex64, np.complex128):
        raise TypeError("DD_carrier_sync: z must be complex64 or complex128 (got %s)" % x.dtype)
    return np.ascontiguousarray(x), sym_count(x.shape[1], int(start), int(step))


def qam_scale_rows_np(x2d, mod, start=0, step=1):
    """r = 1 / (np.std(row[start::step]) c) per row with NumPy's own np.std: what the host restatement of the carrier loop scales MQAM rows with where
    it is not handed the device's deterministic merge (qam_scale_rows), within that merge's documented accuracy of np.std"""
    x = np.asarray(x2d)[:, int(start)::int(step)].astype(np.complex128)
    with np.errstate(all="ignore"):
        return 1.0 / (np.std(x, axis=1) * qam_scale_const(mod)) if x.shape[1] else np.ones(x.shape[0])


def dd_carrier_rows_host(x2d, fam, mod, BnTs, zeta=0.707, type=0, open_loop=False, start=0, step=1, outputs=CAR_OUTPUTS, r=None):
    """dd_carrier_rows in NumPy (no GPU), the kernel's arithmetic operation for operation: vectorised over rows, sequential over symbols.  r: the
    MQAM rows' 1 / scale (default qam_scale_rows_np; pass qam_scale_rows' to restate a device call bit for bit).  Returns the selected arrays."""
    outputs, _ = _car_outputs(outputs)
    x, n = _car_args(x2d, fam, mod, type, start, step)
    nrow = x.shape[0]
    k1, k2, gains = carrier_gains_rows(BnTs, zeta, nrow)
    k1, k2 = (np.full(nrow, k1), np.full(nrow, k2)) if gains is None else (gains[:, 0].copy(), gains[:, 1].copy())
    if fam == QAM:
        r = qam_scale_rows_np(x, mod, start, step) if r is None else np.ascontiguousarray(r, dtype=np.float64).reshape(nrow)
        with np.errstate(all="ignore"):
            back = 1.0 / r
    else:
        r = back = np.ones(nrow)
    table = carrier_table(fam, mod)
    xs = x[:, int(start)::int(step)].astype(np.complex128)
    z, a = np.zeros((nrow, n), dtype=np.complex128), np.zeros((nrow, n), dtype=np.complex128)
    e, t = np.zeros((nrow, n)), np.zeros((nrow, n))
    theta, vi = np.zeros(nrow), np.zeros(nrow)
    for k in range(n if nrow else 0):
        zr, zi, ar, ai, e[:, k], t[:, k], theta, vi = carrier_step_host(fam, mod, type, open_loop, k1, k2, r, back, theta, vi, xs[:, k].real.copy(), xs[:, k].imag.copy(), table)
        with np.errstate(all="ignore"):
            z[:, k].real, z[:, k].imag = (zr * back, zi * back) if fam == QAM else (zr, zi)
        a[:, k].real, a[:, k].imag = ar, ai
    full = dict(z_prime=z.astype(x.dtype), a_hat=a.astype(x.dtype), e_phi=e, theta_h=t)
    return tuple(full[o] for o in outputs)


def dd_carrier_rows(x2d, fam, mod, BnTs, zeta=0.707, type=0, open_loop=False, start=0, step=1, outputs=CAR_OUTPUTS):
    """(nrow, width) complex -> the selected of z_prime, a_hat (x's dtype), e_phi, theta_h (float64), (nrow, n) each with n = len(row[start::step])
    (csrc/carrier.hip: carrier_rows_kernel, behind the MQAM rows' scales by symscale_kernel).  Host arrays, one staged call."""
    outputs, mask = _car_outputs(outputs)
    x, n = _car_args(x2d, fam, mod, type, start, step)
    nrow = x.shape[0]
    k1, k2, gains = carrier_gains_rows(BnTs, zeta, nrow)
    inv, tre, tim = carrier_table(fam, mod)
    full = dict(z_prime=np.zeros((nrow, n), dtype=x.dtype), a_hat=np.zeros((nrow, n), dtype=x.dtype), e_phi=np.zeros((nrow, n)), theta_h=np.zeros((nrow, n)))
    p = {o: (_ptr(full[o]) if o in outputs else None) for o in CAR_OUTPUTS}
    check(load().skdsp_carrier_rows(_ptr(x), n, nrow, x.shape[1], int(start), int(step), code_of(x.dtype), fam, mod, type, int(bool(open_loop)), k1, k2,
                                    None if gains is None else _ptr(gains), qam_scale_const(mod) if fam == QAM else 0.0, inv, None if tre is None else _ptr(tre),
                                    None if tim is None else _ptr(tim), mask, p["z_prime"], p["a_hat"], p["e_phi"], p["theta_h"]))
    return tuple(full[o] for o in outputs)


def dd_carrier_rows_dev(xd, n, nrow, fam, mod, type, open_loop, k1, k2, zd=None, ad=None, ed=None, td=None, gd=None, rd=None, x_stride=None, y_stride=None, start=0, step=1,
                        dtype=None):
    """Device pointers (DeviceArrays or addresses): n symbols per row read at start + k step; strides in elements (default: the window a row is read from, and
    n); zd / ad / ed / td: the outputs to produce (None: not produced); gd: (nrow, 2) float64 gains or None for k1, k2; rd: MQAM, what qam_scale_rows_dev wrote."""
    dt = xd.dtype if dtype is None else dtype
    inv, tre, tim = carrier_table(fam, mod)
    mask = sum(1 << i for i, d in enumerate((zd, ad, ed, td)) if d is not None)
    xs = int(start) + (int(n) - 1) * int(step) + 1 if n else 0
    check(load().skdsp_carrier_rows_dev(_dp(xd), int(n), int(nrow), int(xs if x_stride is None else x_stride), int(start), int(step), code_of(dt), fam, mod, type,
                                        int(bool(open_loop)), float(k1), float(k2), _dp(gd), _dp(rd), inv, None if tre is None else _ptr(tre),
                                        None if tim is None else _ptr(tim), mask, _dp(zd), _dp(ad), _dp(ed), _dp(td), int(n if y_stride is None else y_stride)))


def time_step_len(n, ns, t_step, n_step):
    """len(np.hstack((z[:ns n_step], z[ns n_step + t_step:], np.zeros(t_step)))) for len(z) = n"""
    edge = min(n, ns * n_step)
    return edge + max(0, n - ns * n_step - t_step) + t_step


def time_step_rows_dev(xd, yd, n, nrow, ns, n_step, t_step=0, td=None, n_out=None, x_stride=None, y_stride=None, dtype=None):
    """yd[r, j] = xd[r, j] in front of sample ns n_step, xd[r, j + t_step] behind it, zeros where that leaves the row (csrc/carrier.hip:
    impair_rows_kernel); td: nrow int64 t_steps on the device, else the scalar; n_out: the output row length (default n); strides in elements"""
    n_out = int(n if n_out is None else n_out)
    check(load().skdsp_time_step_rows_dev(_dp(xd), int(n), int(nrow), int(n if x_stride is None else x_stride), code_of(xd.dtype if dtype is None else dtype), int(ns),
                                          int(n_step), int(t_step), _dp(td), _dp(yd), n_out, int(n_out if y_stride is None else y_stride)))


def phase_step_rows_dev(xd, yd, n, nrow, ns, n_step, factor=1.0, fd=None, x_stride=None, y_stride=None, dtype=None):
    """yd[r, j] = xd[r, j ns] f, j < ceil(n / ns): f = 1 + 0j before symbol n_step, `factor` (the caller's np.exp(1j p_step)) or row r of fd ((nrow, 2)
    float64 (re, im) on the device) from there on"""
    n_out = -(-int(n) // int(ns)) if ns >= 1 else 0
    f = complex(factor)
    check(load().skdsp_phase_step_rows_dev(_dp(xd), int(n), int(nrow), int(n if x_stride is None else x_stride), code_of(xd.dtype if dtype is None else dtype), int(ns),
                                           int(n_step), f.real, f.imag, _dp(fd), _dp(yd), int(n_out if y_stride is None else y_stride)))


# --------------------------------------------------------------------------
# Symbol timing recovery over frame sets (csrc/timing.hip): synchronization.NDA_symb_sync
# --------------------------------------------------------------------------
NDA_OUTPUTS = ("zz", "e_tau")
NDA_NORM_THREADS = 256          # timing_core.hpp's kNormThreads: the partial sums of the rows' standard deviation


def nda_gains(BnTs, zeta, Ns):
    """(K1, K2) of one loop bandwidth, in the reference's statements (synchronization.py:67-70) on Python floats"""
    BnTs, zeta = float(BnTs), float(zeta)
    K0 = -1.0
    Kp = 1.0
    K1 = 4 * zeta / (zeta + 1 / (4 * zeta)) * BnTs / Ns / Kp / K0
    K2 = 4 / (zeta + 1 / (4 * zeta)) ** 2 * (BnTs / Ns) ** 2 / Kp / K0
    return K1, K2


def nda_gains_rows(BnTs, zeta, Ns, nrow):
    """(k1, k2, gains): the scalars and None for one bandwidth, else (0, 0, float64 (nrow, 2)) for one per row"""
    b = np.asarray(BnTs, dtype=np.float64)
    if b.ndim == 0:
        return nda_gains(b, zeta, Ns) + (None,)
    if b.shape != (nrow,):
        raise ValueError("BnTs: a scalar, or one value per row")
    return 0.0, 0.0, np.ascontiguousarray([nda_gains(v, zeta, Ns) for v in b], dtype=np.float64).reshape(nrow, 2)


def nda_consts(Ns, L):
    """(rot, inv_ns, inv_len, k_eps): the detector's rotation constants np.exp(-1j 2 pi / Ns kk) as the reference forms them (Ns real parts, then Ns
    imaginary parts), and 1 / float(Ns), 1.0 / (2L + 1), -1 / (2 pi): what NumPy's complex quotients by Ns and 2L + 1 multiply with, and the
    reference's factor in front of np.angle"""
    pts = np.array([np.exp(-1j * 2 * np.pi / Ns * kk) for kk in range(Ns)], dtype=np.complex128)
    return np.ascontiguousarray(np.concatenate([pts.real, pts.imag])), 1 / float(Ns), 1.0 / (2 * L + 1), -1 / (2 * np.pi)


def nda_loop_end(n, Ns):
    """N of the reference for len(z) = n: its loop is range(1, N)"""
    return max(0, Ns * ((n + 1) // Ns - (Ns - 1)))


def nda_iters(n, Ns):
    """the reference's loop iterations for len(z) = n: an exact upper bound of its output length"""
    return max(0, nda_loop_end(n, Ns) - 1)


def np_csum_host(vals):
    """np.sum of complex values in NumPy's order (timing_core.hpp's np_csum): vals a list of (re, im) pairs of arrays"""
    n = len(vals)
    if n < 4:
        sr, si = vals[0]
        for xr, xi in vals[1:]:
            sr, si = sr + xr, si + xi
        return sr, si
    rr, ri = [v[0] for v in vals[:4]], [v[1] for v in vals[:4]]
    i = 4
    while i < n - (n % 4):
        for k in range(4):
            rr[k], ri[k] = rr[k] + vals[i + k][0], ri[k] + vals[i + k][1]
        i += 4
    sr, si = (rr[0] + rr[1]) + (rr[2] + rr[3]), (ri[0] + ri[1]) + (ri[2] + ri[3])
    for xr, xi in vals[i:]:
        sr, si = sr + xr, si + xi
    return sr, si


def _farrow_sum_host(a, c):
    t0, t1, t2, t3 = a[3] * c[0], a[2] * c[1], a[1] * c[2], a[0] * c[3]
    return (t0 + t1) + (t2 + t3)


def nda_interp_host(I_ord, mu, a):
    """one component of the interpolant: timing_core.hpp's interp; a = (z[nn - 1], z[nn], z[nn + 1], z[nn + 2])"""
    if I_ord == 1:
        return mu * a[1] + (1.0 - mu) * a[0]
    if I_ord == 2:
        v2, v1 = 0.5 * _farrow_sum_host(a, (1.0, -1.0, -1.0, 1.0)), 0.5 * _farrow_sum_host(a, (-1.0, 3.0, -1.0, -1.0))
        return (mu * v2 + v1) * mu + a[1]
    v3, v2 = _farrow_sum_host(a, (1 / 6., -1 / 2., 1 / 2., -1 / 6.)), _farrow_sum_host(a, (0.0, 1 / 2., -1.0, 1 / 2.))
    v1 = _farrow_sum_host(a, (-1 / 6., 1.0, -1 / 2., -1 / 3.))
    return ((mu * v3 + v2) * mu + v1) * mu + a[1]


def _nda_outputs(outputs):
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outputs or any(o not in NDA_OUTPUTS for o in outputs) or len(set(outputs)) != len(outputs):
        raise ValueError("outputs: a non-empty selection of %r" % (NDA_OUTPUTS,))
    return outputs, sum(1 << NDA_OUTPUTS.index(o) for o in outputs)


def nda_refused_length(n, Ns, I_ord):
    """True where the reference's own slices run past its array (Ns = 2, I_ord >= 2, an odd length from 3 on: tests/golden/g28_conventions.json)"""
    N = nda_loop_end(n, Ns)
    return N > 1 and I_ord > 1 and N + Ns > n


def _nda_args(x2d, Ns, L, I_ord, start, max_symbols):
    """(x, n, iters, cap): the rows as complex64 / complex128, the frame length behind start, the loop's iterations, the outputs' row length"""
    for v, lo, hi, what in ((Ns, 2, 16, "Ns must be an integer in 2 ... 16"), (L, 0, 8, "L must be an integer in 0 ... 8"), (I_ord, 1, 3, "I_ord must be 1, 2 or 3")):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("NDA_symb_sync: " + what)
    x = np.asarray(x2d)
    if x.ndim != 2:
        raise ValueError("NDA_symb_sync_rows: a 2-D array, one frame per row")
    if x.dtype in (np.float32, np.float64):
        x = x.astype(np.complex64 if x.dtype == np.float32 else np.complex128)      # exact
    if x.dtype not in (np.complex64, np.complex128):
        raise TypeError("NDA_symb_sync: z must be complex64, complex128, float32 or float64 (got %s)" % x.dtype)
    if isinstance(start, (bool, np.bool_)) or not isinstance(start, (int, np.integer)) or not 0 <= start <= x.shape[1]:
        raise ValueError("NDA_symb_sync_rows: start must be an integer inside the rows")
    n = x.shape[1] - int(start)
    if nda_refused_length(n, Ns, I_ord):
        raise ValueError("NDA_symb_sync: with Ns = 2 and I_ord >= 2 a frame of odd length makes the reference's slices run past its array (len(z) = %d)" % n)
    iters = nda_iters(n, int(Ns))
    if max_symbols is None:
        cap = iters
    else:
        if isinstance(max_symbols, (bool, np.bool_)) or not isinstance(max_symbols, (int, np.integer)) or max_symbols < 0:
            raise ValueError("NDA_symb_sync_rows: max_symbols must be a non-negative integer")
        cap = min(int(max_symbols), iters)
    return np.ascontiguousarray(x), n, iters, cap


def _nda_overflow(counts, cap):
    over = np.nonzero(counts > cap)[0]
    if over.size:
        raise ValueError("NDA_symb_sync_rows: rows %s produce more than max_symbols = %d outputs (up to %d)" % (over[:8].tolist() + (["..."] if over.size > 8 else []), cap,
                                                                                                            int(counts.max())))


def nda_std_rows_host(raw, counts):
    """(nrow,) the rows' standard deviations over raw[row, :counts[row]] as nda_norm_kernel forms them: np.std's two passes, each sum as NDA_NORM_THREADS
    strided partial sums (thread t: elements t, t + 256, ... in order) and a tree over them (slot t += slot t + off, off = 128 ... 1)"""
    raw = np.asarray(raw, dtype=np.complex128)
    nrow, cap = raw.shape
    counts = np.asarray(counts, dtype=np.int64)
    T = NDA_NORM_THREADS
    K = -(-max(cap, 1) // T)
    valid = (np.arange(K * T)[None, :] < counts[:, None]).reshape(nrow, K, T)
    pad = np.zeros((nrow, K * T), dtype=np.complex128)
    pad[:, :cap] = raw
    pad = pad.reshape(nrow, K, T)

    def tree(parts):
        parts = parts.copy()
        off = T // 2
        while off >= 1:
            parts[:, :off] = parts[:, :off] + parts[:, off:2 * off]
            off //= 2
        return parts[:, 0]

    def strided(vals):
        acc = np.zeros((nrow, T))
        for k in range(K):
            acc = np.where(valid[:, k], acc + vals[:, k], acc)
        return tree(acc)
    with np.errstate(all="ignore"):
        nf = counts.astype(np.float64)
        mr, mi = strided(pad.real) / nf, strided(pad.imag) / nf
        dr, di = pad.real - mr[:, None, None], pad.imag - mi[:, None, None]
        return np.sqrt(strided(dr * dr + di * di) / nf)


def nda_rows_host(x2d, Ns, L, BnTs, zeta=0.707, I_ord=3, start=0, normalize=True, max_symbols=None, outputs=NDA_OUTPUTS, underflows=False):
    """nda_rows in NumPy (no GPU), the kernel's arithmetic operation for operation: vectorised over rows, sequential over samples.  Returns the selected
    arrays and counts; underflows=True appends, per row, the sample indices nn at which the counter underflowed."""
    outputs, _ = _nda_outputs(outputs)
    x, n, iters, cap = _nda_args(x2d, Ns, L, I_ord, start, max_symbols)
    nrow = x.shape[0]
    k1, k2, gains = nda_gains_rows(BnTs, zeta, Ns, nrow)
    k1, k2 = (np.full(nrow, k1), np.full(nrow, k2)) if gains is None else (gains[:, 0].copy(), gains[:, 1].copy())
    rot, inv_ns, inv_len, k_eps = nda_consts(Ns, L)
    ln = 2 * L + 1
    zp = np.zeros((nrow, n + 1), dtype=np.complex128)
    zp[:, 1:] = x[:, int(start):]
    zpr, zpi = np.ascontiguousarray(zp.real), np.ascontiguousarray(zp.imag)
    zr, zi, et = np.zeros((nrow, iters + 1)), np.zeros((nrow, iters + 1)), np.zeros((nrow, iters + 1))
    cnt, mu, eps, vi = np.zeros(nrow), np.zeros(nrow), np.zeros(nrow), np.zeros(nrow)
    under, mm = np.zeros(nrow, dtype=bool), np.ones(nrow, dtype=np.int64)
    bufr, bufi = np.zeros((nrow, ln)), np.zeros((nrow, ln))
    marks = [[] for _ in range(nrow)]
    with np.errstate(all="ignore"):
        for nn in range(1, iters + 1 if nrow else 1):
            idx = np.nonzero(under)[0]
            if idx.size:
                m = mu[idx]
                cr, ci = np.zeros(idx.size), np.zeros(idx.size)
                for kk in range(Ns):
                    lo = nn + kk - 1
                    ar = [zpr[idx, lo + j] if lo + j <= n else None for j in range(4)]
                    ai = [zpi[idx, lo + j] if lo + j <= n else None for j in range(4)]
                    ir, ii = nda_interp_host(I_ord, m, ar), nda_interp_host(I_ord, m, ai)
                    if kk == 0:
                        zr[idx, mm[idx]], zi[idx, mm[idx]] = ir, ii
                    m2 = ir * ir + ii * ii
                    cr, ci = cr + m2 * rot[kk], ci + m2 * rot[Ns + kk]
                cr, ci = cr * inv_ns, ci * inv_ns
                bufr[idx, 1:], bufi[idx, 1:] = bufr[idx, :-1], bufi[idx, :-1]
                bufr[idx, 0], bufi[idx, 0] = cr, ci
                sr, si = np_csum_host([(bufr[idx, j], bufi[idx, j]) for j in range(ln)])
                eps[idx] = k_eps * atan2_rn_host(si * inv_len, sr * inv_len)
                et[idx, mm[idx]] = eps[idx]
                mm[idx] += 1
            vp = k1 * eps
            vi = vi + k2 * eps
            W = inv_ns + (vp + vi)
            nxt = cnt - W
            under = nxt < 0.0
            if underflows:
                for r in np.nonzero(under)[0]:
                    marks[r].append(nn)
            mu = np.where(under, cnt / W, mu)
            cnt = np.where(under, 1.0 + nxt, nxt)
    counts = mm - 1
    _nda_overflow(counts, cap)
    keep = np.arange(cap)[None, :] < counts[:, None]
    raw = np.zeros((nrow, cap), dtype=np.complex128)
    raw.real, raw.imag = np.where(keep, zr[:, :cap], 0.0), np.where(keep, zi[:, :cap], 0.0)
    e = np.where(keep, et[:, :cap], 0.0)
    if normalize and "zz" in outputs and cap:
        with np.errstate(all="ignore"):
            rcp = 1.0 / nda_std_rows_host(raw, counts)
            zz = np.zeros_like(raw)
            zz.real, zz.imag = np.where(keep, raw.real * rcp[:, None], 0.0), np.where(keep, raw.imag * rcp[:, None], 0.0)
    else:
        zz = raw
    full = dict(zz=zz.astype(x.dtype), e_tau=e)
    out = tuple(full[o] for o in outputs) + (counts,)
    return out + (marks,) if underflows else out


def nda_rows(x2d, Ns, L, BnTs, zeta=0.707, I_ord=3, start=0, normalize=True, max_symbols=None, outputs=NDA_OUTPUTS):
    """(nrow, width) -> the selected of zz (x's complex dtype), e_tau (float64), (nrow, cap) each and zero behind counts[row], then counts (int64)
    (csrc/timing.hip: nda_rows_kernel, then nda_norm_kernel where normalize).  Host arrays, one staged call."""
    outputs, mask = _nda_outputs(outputs)
    x, n, iters, cap = _nda_args(x2d, Ns, L, I_ord, start, max_symbols)
    nrow = x.shape[0]
    k1, k2, gains = nda_gains_rows(BnTs, zeta, Ns, nrow)
    rot, inv_ns, inv_len, k_eps = nda_consts(Ns, L)
    full = dict(zz=np.zeros((nrow, cap), dtype=x.dtype), e_tau=np.zeros((nrow, cap)))
    counts = np.zeros(nrow, dtype=np.int64)
    p = {o: (_ptr(full[o]) if o in outputs else None) for o in NDA_OUTPUTS}
    check(load().skdsp_nda_rows(_ptr(x), n, nrow, x.shape[1], int(start), code_of(x.dtype), int(Ns), int(L), int(I_ord), k1, k2, None if gains is None else _ptr(gains),
                                _ptr(rot), inv_ns, inv_len, k_eps, mask, int(bool(normalize)), cap, p["zz"], p["e_tau"], _ptr(counts)))
    _nda_overflow(counts, cap)
    return tuple(full[o] for o in outputs) + (counts,)


def nda_rows_dev(xd, n, nrow, Ns, L, I_ord, k1, k2, cap, countsd, zd=None, ed=None, gd=None, x_stride=None, y_stride=None, start=0, normalize=True, dtype=None):
    """Device pointers (DeviceArrays or addresses): a row's frame is n samples from `start`; strides in elements (default start + n, and cap); zd / ed: the
    outputs to produce (None: not produced), min(counts[row], cap) elements per row and nothing behind them; countsd: nrow int64; gd: (nrow, 2) float64 gains
    or None for k1, k2.  The caller compares the counts with cap (a row that outgrew it was cut)."""
    dt = xd.dtype if dtype is None else dtype
    rot, inv_ns, inv_len, k_eps = nda_consts(Ns, L)
    mask = sum(1 << i for i, d in enumerate((zd, ed)) if d is not None)
    check(load().skdsp_nda_rows_dev(_dp(xd), int(n), int(nrow), int(int(start) + int(n) if x_stride is None else x_stride), int(start), code_of(dt), int(Ns), int(L), int(I_ord),
                                    float(k1), float(k2), _dp(gd), _ptr(rot), inv_ns, inv_len, k_eps, mask, int(bool(normalize)), int(cap), _dp(zd), _dp(ed), _dp(countsd),
                                    int(cap if y_stride is None else y_stride)))


def device_bytes_of(a):
    """A DeviceBytes holding the bytes of a host array of any dtype"""
    a = np.ascontiguousarray(a)
    d = DeviceBytes(max(a.nbytes, 1))
    if a.nbytes:
        d.write(a.reshape(-1).view(np.uint8))
    return d


class IirKernel(_HostCalls):
    """A device IIR handle: cascaded biquads (sos) or a transfer function (b, a)."""

    def __init__(self, code, sos=None, b=None, a=None):
        L = load()
        self.code = code
        h = ctypes.c_void_p(0)
        if sos is not None:
            s = np.ascontiguousarray(sos, dtype=np.float64)
            check(L.skdsp_sos_create(_ptr(s), int(s.shape[0]), code, ctypes.byref(h)))
        else:
            bb = np.ascontiguousarray(np.atleast_1d(b), dtype=np.float64)
            aa = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
            check(L.skdsp_tf_create(_ptr(bb), bb.size, _ptr(aa), aa.size, code, ctypes.byref(h)))
        self.h = h.value
        self._fin = weakref.finalize(self, _destroy, self.h)
        seq, spread = ctypes.c_int(0), ctypes.c_double(0.0)
        if hasattr(L, "skdsp_iir_sequential"):
            check(L.skdsp_iir_sequential(ctypes.c_void_p(self.h), ctypes.byref(seq), ctypes.byref(spread)))
        self.sequential, self.spread = bool(seq.value), spread.value
        if self.sequential:
            import logging
            logging.getLogger("sk_dsp_comm_amd").warning(
                "IIR cascade of %d sections is ill-conditioned: two float64 evaluations of it (sections in another order) differ by %.1e of "
                "the output; it runs the reference's own sample-by-sample recursion on the GPU (exact, but at a host core's speed)",
                int(np.asarray(sos).shape[0]) if sos is not None else -1, self.spread)

    def filter(self, x, wide=False):
        return self._host(x.size, x.dtype, wide, lambda y: check(load().skdsp_iir_filter(ctypes.c_void_p(self.h), _ptr(x), x.size, _ptr(y))))

    def filter_rows(self, x2, wide=False):
        """x2: C-contiguous (rows, n): every row filtered from rest in ONE call (one copy each way, one launch where the
        parallel-form scan applies)."""
        rows, n = x2.shape
        y = self._host(x2.size, x2.dtype, wide, lambda y: check(load().skdsp_iir_filter_rows(ctypes.c_void_p(self.h), _ptr(x2), n, rows, _ptr(y))))
        return y.reshape(rows, n)

    def filter_rows_dev(self, xd, yd, n, rows, x_stride=None, y_stride=None):
        check(load().skdsp_iir_filter_rows_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, rows, n if x_stride is None else x_stride,
                                                n if y_stride is None else y_stride, ctypes.c_void_p(yd.ptr)))

    def up(self, x, L, wide=False):
        return self._host(x.size * L, x.dtype, wide, lambda y: check(load().skdsp_iir_up(ctypes.c_void_p(self.h), _ptr(x), x.size, int(L), _ptr(y))))

    def dn(self, x, M, wide=False):
        return self._host(x.size // M, x.dtype, wide, lambda y: check(load().skdsp_iir_dn(ctypes.c_void_p(self.h), _ptr(x), x.size, int(M), _ptr(y))))

    def filter_dev(self, xd, yd, n=None):
        n = xd.n if n is None else n
        check(load().skdsp_iir_filter_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, ctypes.c_void_p(yd.ptr)))

    def up_dev(self, xd, yd, L, n=None):
        n = xd.n if n is None else n
        check(load().skdsp_iir_up_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, int(L), ctypes.c_void_p(yd.ptr)))

    def dn_dev(self, xd, yd, M, n=None):
        n = xd.n if n is None else n
        check(load().skdsp_iir_dn_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, int(M), ctypes.c_void_p(yd.ptr)))

    def state_len(self):
        k = ctypes.c_int(0)
        check(load().skdsp_iir_state_len(ctypes.c_void_p(self.h), ctypes.byref(k)))
        return k.value

    def filter_state_dev(self, xd, yd, n=None, zi=None, want_zf=True):
        """Device-resident block streaming: y_dev[0:n] and (returned) the state after sample n-1.
        zi: float64 vector of state_len() entries, None = rest."""
        n = xd.n if n is None else n
        zf = np.zeros(self.state_len()) if want_zf else None
        zi_p = None
        if zi is not None:
            zi = np.ascontiguousarray(zi, dtype=np.float64)
            if zi.size != self.state_len():
                raise ValueError("zi must have %d entries" % self.state_len())
            zi_p = _ptr(zi)
        check(load().skdsp_iir_filter_state_dev(ctypes.c_void_p(self.h), ctypes.c_void_p(xd.ptr), n, zi_p,
                                                 _ptr(zf) if want_zf else None, ctypes.c_void_p(yd.ptr)))
        return zf

    def filter_state(self, x, zi=None):
        """Block streaming from host memory: (y, zf)."""
        x = np.ascontiguousarray(x)
        xd = DeviceArray.from_host(x)
        yd = DeviceArray(x.size, x.dtype)
        try:
            zf = self.filter_state_dev(xd, yd, x.size, zi)
            y = yd.to_host()
        finally:
            xd.free()
            yd.free()
        return y, zf


def sos_par_info(sos):
    """Host only: the partial-fraction expansion the parallel-form scan runs for this cascade (c0, sections (a1, a2, r0, r1),
    cancellation factor, impulse-response error against the cascade, accepted)."""
    s = np.ascontiguousarray(sos, dtype=np.float64).reshape(-1, 6)
    ns = s.shape[0]
    out = np.zeros(5 + 4 * ns)
    ok = ctypes.c_int(0)
    check(load().skdsp_sos_par_info(_ptr(s), ns, _ptr(out), ctypes.byref(ok)))
    return {"c0": out[0], "sections": out[1:1 + 4 * ns].reshape(ns, 4).copy(), "kappa": out[1 + 4 * ns], "ir_err": out[2 + 4 * ns],
            "accepted": bool(ok.value),
            # the float32 from-rest states (7 - 8 biquads, float32 / complex64 signals): worst probe error on 128- / 96-sample chunks, admitted below 5e-7
            # -- per chunk length: .filter and .up by 2 / 4 run 128-sample chunks, .up by 3 runs 96-sample ones (.dn keeps the float64 states)
            "v32_err": out[3 + 4 * ns], "v32_err_t96": out[4 + 4 * ns], "v32_admitted": bool(ok.value) and out[3 + 4 * ns] <= 5e-7,
            "v32_admitted_t96": bool(ok.value) and out[4 + 4 * ns] <= 5e-7}


def tf2sos(b, a):
    """The (b, a) -> second-order-sections factorisation skdsp_tf_create applies (host only)."""
    bb = np.ascontiguousarray(np.atleast_1d(b), dtype=np.float64)
    aa = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
    sos = np.zeros((12, 6))
    ns = ctypes.c_int(0)
    check(load().skdsp_tf2sos(_ptr(bb), bb.size, _ptr(aa), aa.size, _ptr(sos), ctypes.byref(ns)))
    return sos[:ns.value].copy()


def upsample(x, L):
    y = np.empty(x.size * L, dtype=x.dtype)
    check(load().skdsp_upsample(_ptr(x), x.size, int(L), code_of(x.dtype), _ptr(y)))
    return y


FARROW_WIDE, FARROW_F64 = 1, 2   # the `wide` flags of skdsp_farrow / skdsp_farrow_dev (include/skdsp.h)


def farrow_len(n, Ts_old, Ts_new):
    """Output count of the Farrow resampler, len(np.arange(0, Ts_old*(n-3) + Ts_old, Ts_new)); host only."""
    v = ctypes.c_int64(0)
    check(load().skdsp_farrow_len(int(n), float(Ts_old), float(Ts_new), ctypes.byref(v)))
    return v.value


def _farrow_flags(wide, f64):
    return (FARROW_WIDE if wide else 0) | (FARROW_F64 if f64 else 0)


def farrow(x, Ts_old, Ts_new, i_ord, alpha=0.5, wide=False, f64=False):
    """digitalcom.farrow_resample on a host vector: wide=True gives float64 / complex128 results for a float32 / complex64 x,
    f64=True runs such an x in float64 arithmetic."""
    n_out = farrow_len(x.size, Ts_old, Ts_new)
    y = np.empty(n_out, dtype=_WIDE.get(x.dtype, x.dtype) if wide else x.dtype)
    check(load().skdsp_farrow(_ptr(x), x.size, code_of(x.dtype), float(Ts_old), float(Ts_new), int(i_ord), float(alpha),
                              _farrow_flags(wide, f64), _ptr(y)))
    return y


def farrow_dev(xd, yd, Ts_old, Ts_new, i_ord, alpha=0.5, n0=0, count=None, wide=False, f64=False):
    """Outputs [n0, n0 + count) of the Farrow resampler of device array xd into yd[0 .. count) (default: all from n0 on)."""
    if count is None:
        count = farrow_len(xd.n, Ts_old, Ts_new) - int(n0)
    out_dt = _WIDE.get(xd.dtype, xd.dtype) if wide else xd.dtype
    if yd.dtype != out_dt or yd.n < int(count):
        raise ValueError("farrow_dev: y holds %d samples of %s, the call writes %d of %s" % (yd.n, yd.dtype, int(count), out_dt))
    check(load().skdsp_farrow_dev(ctypes.c_void_p(xd.ptr), xd.n, xd.code, float(Ts_old), float(Ts_new), int(i_ord), float(alpha),
                                  int(n0), int(count), _farrow_flags(wide, f64), ctypes.c_void_p(yd.ptr)))


def _psd_window(window):
    w = np.ascontiguousarray(window, dtype=np.float64)
    if w.ndim != 1:
        raise ValueError("psd: the window must be one-dimensional")
    return w, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def psd_accum(x, window, n_fft, step, nseg):
    """The Welch primitive on a host vector (csrc/psd.hip):
    S[k] = sum_{i < nseg} |FFT_{n_fft}(window * x[i step : i step + len(window)])[k]|^2, k < n_fft, float64."""
    w, wp = _psd_window(window)
    S = np.empty(int(n_fft), dtype=np.float64)
    check(load().skdsp_psd(_ptr(x), x.size, code_of(x.dtype), wp, w.size, int(n_fft), int(step), int(nseg), _ptr(S)))
    return S


def psd_accum_dev(xd, Sd, window, n_fft, step, nseg):
    """The same from device array xd into the first n_fft float64 of device array Sd."""
    w, wp = _psd_window(window)
    if Sd.dtype != np.float64 or Sd.n < int(n_fft):
        raise ValueError("psd_accum_dev: S holds %d samples of %s, the call writes %d of float64" % (Sd.n, Sd.dtype, int(n_fft)))
    check(load().skdsp_psd_dev(ctypes.c_void_p(xd.ptr), xd.n, xd.code, wp, w.size, int(n_fft), int(step), int(nseg),
                               ctypes.c_void_p(Sd.ptr)))


def downsample(x, M, p):
    y = np.empty(x.size // M, dtype=x.dtype)
    check(load().skdsp_downsample(_ptr(x), x.size, int(M), int(p), code_of(x.dtype), _ptr(y)))
    return y
