"""sigsys.psd / my_psd / simple_sa and digitalcom.my_psd without a GPU: the host float64 restatement of the Welch primitive
(sigsys.psd_accum_host) reproduces the captured reference (g16) through the public functions, the segment-count rule
equals the reference's while loop, the signatures are the reference's, every argument convention is settled before any
device call, and the kernel's FFT core (csrc/psd_core.hpp), compiled for the host, agrees with np.fft in float64."""
import inspect
import json
import os
import subprocess
import warnings

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, digitalcom as dc, sigsys as ss
from conftest import GOLDEN, ROOT


def g16_cases():
    g = np.load(os.path.join(GOLDEN, "g16_psd.npz"))
    return g, json.loads(str(g["cases"]))


def g16_input(g, c):
    v = g["x"][:c["Q"]]
    return (v if c["dtype"].startswith("complex") else v.real).astype(c["dtype"])


def g16_call(c, x):
    """(spectrum, frequency axis) of case c on input x through the package's public functions."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (K = 0: the reference's 0/0, reproduced)
        if c["fn"] == "psd":
            return ss.psd(x, **c["args"])
        if c["fn"] == "my_psd":
            return ss.my_psd(x, **c["args"])
        if c["fn"] == "dc_my_psd":
            return dc.my_psd(x, **c["args"])
        f, P = ss.simple_sa(x, **c["args"])
        return P, f


def peak_err(P, ref):
    return float(np.max(np.abs(P - ref))) / float(np.max(np.abs(ref)))


def test_restatement_reproduces_reference_g16(monkeypatch):
    monkeypatch.setattr(ss, "_psd_served", lambda n_fft: False)   # every size through the host restatement
    g, cases = g16_cases()
    assert len(cases) >= 120
    seen = set()
    worst = 0.0
    for c in cases:
        ref, fref = g[c["key"]], g[c["key"] + "_f"]
        P, f = g16_call(c, g16_input(g, c))
        assert P.shape == ref.shape and P.dtype == ref.dtype == np.float64, c
        assert f.shape == fref.shape and np.allclose(f, fref, rtol=1e-15, atol=0), c
        if np.all(np.isnan(ref)):
            assert np.all(np.isnan(P)), c
            seen.add("K0")
            continue
        e = peak_err(P, ref)
        worst = max(worst, e)
        assert e <= 1e-12, (c, e)
        seen.add((c["fn"], c["dtype"]))
    print("worst peak-relative error against the reference: %.2e" % worst)
    assert "K0" in seen and len(seen) == 1 + 4 * 4


def test_segment_count_rule_matches_the_reference_loop():
    rng = np.random.default_rng(16)
    for _ in range(100000):
        n_fft = int(rng.choice([rng.integers(1, 40), 64, 100, 256]))
        ov = float(rng.choice([0, 37, 50, 75, rng.uniform(-20, 99), rng.integers(0, 99)]))
        Q = int(rng.integers(0, 8 * n_fft + 3))
        R = int(np.round(ov / 100 * n_fft))
        if n_fft - R <= 0:
            with pytest.raises(ValueError):
                ss._psd_segments(Q, n_fft, ov)
            continue
        i = 0
        while i * (n_fft - R) + 1 + n_fft <= Q:   # sigsys.py:2570
            i += 1
        assert ss._psd_segments(Q, n_fft, ov) == (n_fft - R, i), (Q, n_fft, ov)


def test_signatures_match_reference():
    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(ss.psd) == [("x", E), ("n_fft", E), ("fs", 1), ("overlap_percent", 50), ("scale_noise", True)]
    assert sig(ss.my_psd) == [("x", E), ("n_fft", 1024), ("fs", 1)]
    assert sig(dc.my_psd) == [("x", E), ("NFFT", 1024), ("Fs", 1)]
    assert sig(ss.simple_sa) == [("x", E), ("NS", E), ("NFFT", E), ("fs", E), ("NAVG", 1), ("window", "boxcar")]


def test_conventions_are_settled_before_any_device_call():
    """Without a GPU any device call raises SkdspError: what raises here, or returns without a spectrum, never got that far."""
    conv = json.load(open(os.path.join(GOLDEN, "g16_conventions.json")))
    xr = np.random.default_rng(1).standard_normal(2000)
    for ov in (100, 100.2, 150):
        with pytest.raises(ValueError):
            ss.psd(xr, 256, overlap_percent=ov)      # deliberate: the reference never terminates
    for call in (lambda: ss.psd(xr.reshape(2, 1000), 256), lambda: ss.my_psd(xr.reshape(2, 1000), 256),
                 lambda: ss.simple_sa(xr.reshape(2, 1000), 128, 512, 1)):
        with pytest.raises(ValueError):              # deliberate: one-dimensional input only
            call()
    assert conv["simple_sa_list"] == {"raises": "AttributeError"}
    with pytest.raises(AttributeError):
        ss.simple_sa(list(xr), 128, 512, 1)
    with pytest.warns(UserWarning):
        out = ss.simple_sa(xr, 128, 512, 1, NAVG=16)
    assert out == (0, 0) and conv["simple_sa_NAVG_gt_K"]["first"]["shape"] == []
    for name, x in (("psd_K0", xr[:256]), ("psd_K0_complex", xr[:100] + 0j), ("psd_empty", np.zeros(0))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            P, f = ss.psd(x, 256)
        want = conv[name]
        assert want["first"]["all_nan"] and np.all(np.isnan(P)) and list(P.shape) == want["first"]["shape"], name
        assert list(f.shape) == want["second"]["shape"] and P.dtype == f.dtype == np.float64, name


def test_c_abi_rejects_bad_arguments_without_a_device():
    x = np.zeros(4096, np.float32)
    w = np.ones(256)
    bad = [
        dict(window=np.ones(1000), n_fft=1000, step=500, nseg=2),    # not a power of two
        dict(window=np.ones(32), n_fft=32, step=16, nseg=2),         # below 64
        dict(window=np.ones(8192), n_fft=8192, step=4096, nseg=1),   # above 4096
        dict(window=np.ones(257), n_fft=256, step=128, nseg=2),      # ns > n_fft
        dict(window=np.ones(0), n_fft=256, step=128, nseg=2),        # ns < 1
        dict(window=w, n_fft=256, step=0, nseg=2),
        dict(window=w, n_fft=256, step=128, nseg=0),
        dict(window=w, n_fft=256, step=128, nseg=32),                # 31 * 128 + 256 > 4096
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            _ffi.psd_accum(x, **kw)


def _emul_inputs(n_fft):
    """(name, x complex64 or float32, ns, step, nseg): noise, a bin-centred tone and DC."""
    rng = np.random.default_rng(n_fft)
    K, step = 6, n_fft // 2
    n = (K - 1) * step + n_fft
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    tone = np.exp(2j * np.pi * (n_fft // 8 + 3) / n_fft * np.arange(n)).astype(np.complex64)
    yield "noise", noise, n_fft, step, K
    yield "tone", tone, n_fft, step, K
    yield "dc", np.ones(n, np.complex64), n_fft, step, K
    yield "real noise", noise.real.copy(), n_fft, step, K - 1          # (an odd count: the last pair is half empty)
    yield "real tone", tone.real.copy(), n_fft, 37, 4
    yield "short window", noise, n_fft - 9, n_fft // 4 + 1, 5


def test_float_core_host_emulation_against_numpy_fft(tmp_path):
    """csrc/psd_core.hpp compiled for the HOST on float32 samples, every n_fft, against np.fft in float64 on the same samples
    and window: the float64 image (the kernel's default) to 1e-12 of the peak bin, the float32 image (option psd_f32_image)
    within the float32 contract, 1e-6."""
    exe = str(tmp_path / "psd_emul")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "psd_emul.cpp"), "-o", exe])
    xf, wf, of = (str(tmp_path / n) for n in ("x.f32", "w.f64", "out.f64"))
    worst = {64: 0.0, 32: 0.0}
    for n_fft in (64, 128, 256, 512, 1024, 2048, 4096):
        for name, x, ns, step, K in _emul_inputs(n_fft):
            w = np.hanning(ns) if name != "dc" else np.ones(ns)
            x.tofile(xf)
            w.tofile(wf)
            ref = ss.psd_accum_host(x, w, n_fft, step, K)
            for bits, tol in ((64, 1e-12), (32, 1e-6)):
                out = subprocess.run([exe, str(n_fft), str(ns), str(step), str(K), str(int(x.dtype.kind == "f")), xf, wf, of, str(bits)],
                                     stdout=subprocess.PIPE).stdout.decode()
                assert out.strip().endswith("OK"), (n_fft, name, out)
                S = np.fromfile(of)
                e = peak_err(S, ref)
                worst[bits] = max(worst[bits], e)
                assert S.shape == ref.shape and e <= tol, (n_fft, name, bits, e)
    print("worst peak-relative error: float64 image %.2e, float32 image %.2e" % (worst[64], worst[32]))
