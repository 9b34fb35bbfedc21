"""digitalcom.farrow_resample without a GPU: a vectorised NumPy restatement of the reference's per-output loop reproduces the
captured reference (g15), the output-count rule equals len(np.arange(...)), the kernel's index algebra (csrc/farrow_core.hpp)
is bit-identical to plain IEEE divisions (host emulation), and every argument convention raises before any device call."""
import inspect
import json
import os
import subprocess

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, digitalcom as dc
from conftest import GOLDEN, ROOT

# the reference's lfilter weights (digitalcom.py:194-209)
_W3 = ([1 / 6., -1 / 2., 1 / 2., -1 / 6.], [0, 1 / 2., -1, 1 / 2.], [-1 / 6., 1, -1 / 2., -1 / 3.], [0, 0, 1])
_W1 = ([0, 1], [0, 0, 1])


def farrow_restated(x, fs_old, fs_new, i_ord=3, alpha=0.5, n0=0, count=None):
    """Outputs [n0, n0 + count) of the reference's farrow_resample, vectorised: the same float64 operations in the same
    order, with lfilter(w, 1, x) as np.convolve(w, x) over only the input span those outputs read."""
    x = np.asarray(x)
    xd = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    Ts_old = 1 / float(fs_old)
    Ts_new = 1 / float(fs_new)
    N = dc._farrow_len(len(x), Ts_old, Ts_new)
    count = N - n0 if count is None else count
    j = np.arange(n0, n0 + count, dtype=np.float64)
    t = j * Ts_new
    n_old = np.floor(t / Ts_old)
    mu = (t - n_old * Ts_old) / Ts_old
    k = n_old.astype(np.int64) + 1
    if count == 0:
        return np.zeros(0, dtype=xd.dtype)
    s, e = int(k.min()) - 3, int(k.max()) + 1          # x[s .. e] (x[i] = 0 for i < 0)
    xp = np.concatenate([np.zeros(3, xd.dtype), xd])[s + 3:e + 4]
    if i_ord == 3:
        ws = _W3
    elif i_ord == 2:
        a = alpha
        ws = ([a, -a, -a, a], [-a, 1 + a, a - 1, -a], [0, 0, 1])
    else:
        ws = _W1
    v = [np.convolve(w, xp)[:len(xp)][k - s] for w in ws]
    if i_ord == 3:
        return ((v[0] * mu + v[1]) * mu + v[2]) * mu + v[3]
    if i_ord == 2:
        return (v[0] + v[1]) * mu + v[2]
    return mu * v[0] + (1 - mu) * v[1]


def g15_cases():
    g = np.load(os.path.join(GOLDEN, "g15_farrow.npz"))
    return g, json.loads(str(g["cases"]))


def test_restatement_reproduces_reference_g15():
    g, cases = g15_cases()
    assert len(cases) >= 500
    for c in cases:
        x, ref = g[c["x"]], g[c["key"]]
        y = farrow_restated(x, c["fs_old"], c["fs_new"], c["i_ord"], c["alpha"])
        assert y.shape == ref.shape and y.dtype == ref.dtype, c
        if c["i_ord"] == 1:
            assert np.array_equal(y, ref), c
        elif ref.size:
            assert np.max(np.abs(y - ref)) <= 1e-14 * np.max(np.abs(x)), c


def test_output_count_rule_matches_arange():
    rng = np.random.default_rng(7)
    for _ in range(100000):
        n = int(rng.integers(0, 200))
        fo = float(rng.choice([rng.uniform(0.1, 50), rng.integers(1, 50), 48000.0, np.pi]))
        fn = float(rng.choice([rng.uniform(0.1, 50), rng.integers(1, 50), 44100.0, np.e]))
        if rng.random() < 0.25:
            fo, fn = -fo, -fn
        elif rng.random() < 0.1:
            fn = -fn
        Ts_old, Ts_new = 1 / fo, 1 / fn
        want = len(np.arange(0, Ts_old * (n - 3) + Ts_old, Ts_new))
        assert dc._farrow_len(n, Ts_old, Ts_new) == want, (n, fo, fn)
        assert _ffi.farrow_len(n, Ts_old, Ts_new) == want, (n, fo, fn)
    with pytest.raises(ValueError):
        _ffi.farrow_len(10, 1.0, 0.0)


def test_farrow_index_algebra_host_emulation(tmp_path):
    """Compiles csrc/farrow_core.hpp for the HOST: n_old and mu bit-identical to plain IEEE t / Ts_old over 10^7 indices per
    ratio up to 2^31, integer ratios included."""
    exe = str(tmp_path / "farrow_emul")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "farrow_emul.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE).stdout.decode()
    assert out.strip().endswith("OK"), out


def test_signature_matches_reference():
    sig = inspect.signature(dc.farrow_resample)
    assert list(sig.parameters) == ["x", "fs_old", "fs_new", "i_ord", "alpha"]
    assert sig.parameters["i_ord"].default == 3 and sig.parameters["alpha"].default == 0.5


_EXC = {"ValueError": ValueError, "ZeroDivisionError": ZeroDivisionError, "AttributeError": AttributeError}


def test_error_conventions_raise_before_any_device_call():
    """Every convention of g15_conventions.json that raises or returns nothing is settled on the host (without a GPU any
    device call would raise SkdspError instead).  int64 input is a deliberate difference (run as float64): not here."""
    conv = json.load(open(os.path.join(GOLDEN, "g15_conventions.json")))
    x10 = np.arange(10.0)
    calls = {
        "i_ord_0": lambda: dc.farrow_resample(x10, 8, 18, i_ord=0),
        "i_ord_4": lambda: dc.farrow_resample(x10, 8, 18, i_ord=4),
        "empty": lambda: dc.farrow_resample(np.zeros(0), 8, 18),
        "len1": lambda: dc.farrow_resample(np.ones(1), 8, 18),
        "len2": lambda: dc.farrow_resample(np.ones(2), 8, 18),
        "fs_old_0": lambda: dc.farrow_resample(x10, 0, 18),
        "fs_new_0": lambda: dc.farrow_resample(x10, 8, 0),
        "fs_new_inf": lambda: dc.farrow_resample(x10, 8, float("inf")),
        "fs_new_negative": lambda: dc.farrow_resample(x10, 8, -18),
        "fs_old_negative": lambda: dc.farrow_resample(x10, -8, 18),
        "list": lambda: dc.farrow_resample([1.0, 2.0, 3.0, 4.0, 5.0], 8, 18),
    }
    for name, call in calls.items():
        want = conv[name]
        if "raises" in want:
            with pytest.raises(_EXC[want["raises"]]):
                call()
        else:
            y = call()
            assert len(y) == want["len"] == 0 and str(y.dtype) == want["dtype"], name
    with pytest.raises(ValueError):
        dc.farrow_resample(np.ones((2, 5)), 8, 18)   # deliberate: ndim != 1
    assert dc.farrow_resample(np.ones(2, np.complex64), 8, 18).dtype == np.complex128
