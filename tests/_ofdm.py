"""What tests/test_ofdm_cpu.py and tests/test_gpu_ofdm.py share: the G24 fixtures (tests/golden/gen_golden_ofdm.py), the tolerances of
DESIGN.md 4.19 and the comparison of a result with a float64 reference."""
import json
import os

import numpy as np
from scipy import signal

from conftest import GOLDEN

HC = np.array([1.0, 0.1, -0.05, 0.15, 0.2, 0.05])   # the ofdm_rx docstring's channel: |H| >= 1 - 0.55 = 0.45 on every bin
TOL64 = 1e-12                                         # complex128: 1e-12 max|ref|
TOL32 = 2.0 ** -23                                    # complex64: both sides round a float64 value that differs by ~1e-15: one float32 unit at the peak


def g24():
    g = np.load(os.path.join(GOLDEN, "g24_ofdm.npz"))
    return g, json.loads(str(g["mux"])), json.loads(str(g["cases"]))


def conv24():
    return json.load(open(os.path.join(GOLDEN, "g24_conventions.json")))


def rx_input(g, case):
    """what the generator fed the reference's ofdm_rx: the transmitted frame through the channel"""
    tx = g[case["key"] + "_tx"]
    return signal.lfilter(HC, 1, tx) if tx.size else tx


def close(y, ref, what="", scale=1.0):
    """y against a float64 reference: dtype-exact shape, and max|y - ref| <= tol max|ref| with the tolerance of y's precision; a complex64 y is
    compared with the reference rounded to complex64.  scale: the factor a division by the channel may amplify the bound by."""
    y, ref = np.asarray(y), np.asarray(ref)
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    single = y.dtype == np.complex64
    want = ref.astype(np.complex64) if single else ref
    peak = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(y.astype(np.complex128) - want.astype(np.complex128)))) / (peak if peak > 0 else 1.0)
    assert err <= (TOL32 if single else TOL64 * scale), (what, err)
    return err


def qam16(rng, shape):
    return ((rng.integers(0, 4, shape) * 2 - 3) + 1j * (rng.integers(0, 4, shape) * 2 - 3)).astype(np.complex128)


def check_case_tx(g, case, fn):
    """fn: the public ofdm_tx (or its _host form) on a G24 case, against the reference's result"""
    y = fn(g[case["key"] + "_data"], case["nf"], case["nc"], case["npb"], case["cp"], case["ncp"])
    assert y.dtype == np.complex128
    return close(y, g[case["key"] + "_tx"], ("tx", case["key"]))


def check_case_rx(g, case, fn):
    x, worst = rx_input(g, case), 0.0
    for m in case["rx"]:
        z, H = fn(x, case["nf"], case["nc"], m["npb"], case["cp"], case["ncp"], float(g["alpha"]), HC if m["ht"] else None)
        rz, rH = g["%s_%s_z" % (case["key"], m["mode"])], g["%s_%s_H" % (case["key"], m["mode"])]
        assert z.dtype == np.complex128 and H.dtype == rH.dtype and H.shape == rH.shape == (case["nf"],), (case["key"], m)
        worst = max(worst, close(z, rz, ("rx", case["key"], m["mode"]), 1 / 0.45), close(H, rH, ("H", case["key"], m["mode"])))
    return worst


# ---- the device-resident loop of tests/test_gpu_ofdm.py: bits -> 16-QAM -> OFDM tx -> AWGN -> OFDM rx -> demap -> count, restated in NumPy
LOOP_ROWS, LOOP_SYMS, LOOP_NF, LOOP_NC, LOOP_NCP, LOOP_MOD, LOOP_SIGMA = 4, 64, 32, 64, 8, 16, 0.05
LOOP_SEED = 2401      # fixed on the CPU: loop_host(LOOP_SIGMA)[1], the smallest distance of a decision variable from a threshold, is 3.1e-5


def loop_host(sigma):
    """(per-row error counts, margin): the restatements of the seven device stages, the noise on stream seed + 1.  margin: the smallest distance
    of a demapper decision variable (x r + 3) / 2 from its thresholds 0.5, 1.5, 2.5 -- a 1e-15 difference of the transform, or 1e-13 of the
    scale, cannot move a decision while it is above 1e-9."""
    from sk_dsp_comm_amd import _ffi, digitalcom as dc
    nq = LOOP_SYMS * LOOP_NF
    bits = np.stack([_ffi.random_bits_host(LOOP_SEED, r, 0, 4 * nq) for r in range(LOOP_ROWS)])
    sym = _ffi.gray_map_rows_host(bits, _ffi.QAM, LOOP_MOD, np.complex128)
    tx = np.stack([dc.ofdm_tx_host(r, LOOP_NF, LOOP_NC, 0, True, LOOP_NCP) for r in sym])
    y = _ffi.awgn_rows_host(tx, 1.0, sigma, LOOP_SEED + 1)
    counts, margin = [], np.inf
    for r in range(LOOP_ROWS):
        z = dc.ofdm_rx_host(y[r], LOOP_NF, LOOP_NC, 0, True, LOOP_NCP)[0]
        scale = dc._qam_scale_host(z, LOOP_MOD)
        k = np.concatenate([(z.real * scale + 3) / 2, (z.imag * scale + 3) / 2])
        margin = min(margin, float(np.min(np.abs(k[:, None] - np.array([0.5, 1.5, 2.5])[None, :]))))
        counts.append(int(np.sum(dc._qam_bits_host(z, LOOP_MOD, scale) != bits[r])))
    return np.array(counts, dtype=np.int64), margin
