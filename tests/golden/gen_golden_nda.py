#!/usr/bin/env python3
"""G28: symbol timing recovery -- synchronization.NDA_symb_sync (synchronization.py:43-166) -- results from the REAL reference (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_nda.py

  g28_nda.npz           "cases": JSON list of {key, signal, trim, Ns, L, BnTs, zeta, I_ord, what, seed, S, margin, max_e}: the input is <signal>[:len - trim]
                        (signals are shared between cases) -> <key>_zz, <key>_e_tau as the reference returned them, <key>_raw the restatement's zz in
                        front of zz /= np.std(zz), <key>_under the sample indices nn at which the counter underflowed; "std" of a case is np.std(raw).
                        S is the yardstick of tests/test_nda_cpu.py: the reference's statements once more in float64 (array_equal to the reference, asserted
                        here) and once in np.longdouble / np.clongdouble, and the largest absolute difference between the two runs over raw zz and e_tau --
                        the reference's own rounding noise as the loop amplifies it.
  g28_conventions.json  the signature, the NumPy version, what is kept from the reference with the probe behind each item, and the observations the
                        restatement of the arithmetic rests on

Signals: 300 QPSK or 16-QAM symbols through a raised-cosine pulse (roll-off 0.35, +-6 symbols) at 16 samples per symbol, decimated to Ns samples per symbol
with a chosen phase (a fractional timing offset of phase / 16 symbols).  A case is admitted only if S <= 1e-12, both runs underflow at the same samples,
every CNT - W from the first non-zero epsilon on lies at least 1e-9 from zero (in the longdouble run) and every |e_tau| <= 0.5 - 1e-6.  The cases that share
a signal are admitted together; a signal that fails is drawn again with the next seed; the admission is never relaxed.  Ns = 2 is not captured: its detector
term is real, epsilon is 0 or +-0.5 up to rounding and the run is chaotic.
"""
import inspect
import json
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
# as in gen_golden_carrier.py: NumPy's SIMD dispatch off, so that the capture does not depend on the machine that ran it
DISPATCH_OFF = "FMA3 AVX2 AVX512F AVX512CD AVX512_KNL AVX512_KNM AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"
os.environ["NPY_DISABLE_CPU_FEATURES"] = DISPATCH_OFF
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("SK_DSP_COMM_SRC", "/root/reference/src"))

import numpy as np  # noqa: E402

from sk_dsp_comm import synchronization as sync  # noqa: E402

LD, CLD = np.longdouble, np.clongdouble
N_SYMB, ZETA, OVER, ALPHA, SPAN = 300, 0.707, 16, 0.35, 6


def rc_pulse():
    t = np.arange(-SPAN * OVER, SPAN * OVER + 1) / OVER
    return np.sinc(t) * np.cos(np.pi * ALPHA * t) / (1 - (2 * ALPHA * t) ** 2)


def signal_of(seed, Ns, phase, qam16=False, snr_db=None):
    rng = np.random.default_rng(seed)
    lv = np.array([-3, -1, 1, 3]) / np.sqrt(10) if qam16 else np.array([-1, 1]) / np.sqrt(2)
    s = lv[rng.integers(0, lv.size, N_SYMB)] + 1j * lv[rng.integers(0, lv.size, N_SYMB)]
    up = np.zeros(N_SYMB * OVER, dtype=np.complex128)
    up[::OVER] = s
    x = np.convolve(up, rc_pulse())[SPAN * OVER:SPAN * OVER + N_SYMB * OVER]
    z = x[phase::OVER // Ns][:N_SYMB * Ns] if OVER % Ns == 0 else None
    if z is None:                                    # Ns = 3: 16 is no multiple; resample the 16x waveform at 16 / 3 by linear interpolation
        at = phase + np.arange(N_SYMB * Ns) * (OVER / Ns)
        at = at[at < x.size - 1]
        k = at.astype(int)
        z = x[k] + (at - k) * (x[k + 1] - x[k])
    if snr_db is not None:
        sigma = np.sqrt(np.mean(np.abs(z) ** 2) / (2 * 10 ** (snr_db / 10)))
        z = z + sigma * (rng.standard_normal(z.size) + 1j * rng.standard_normal(z.size))
    return np.ascontiguousarray(z)


def restate(z, Ns, L, BnTs, zeta, I_ord, F, C):
    """the reference's statements, in float64 (F, C = np.float64, np.complex128) or in np.longdouble.  Returns (raw zz, e_tau, underflow samples,
    margin): zz in front of zz /= np.std(zz); margin = min |CNT - W| from the first non-zero epsilon on."""
    wide = F is not np.float64
    K0 = -1.0
    Kp = 1.0
    K1 = F(4 * zeta / (zeta + 1 / (4 * zeta)) * BnTs / Ns / Kp / K0)
    K2 = F(4 / (zeta + 1 / (4 * zeta)) ** 2 * (BnTs / Ns) ** 2 / Kp / K0)
    zz = np.zeros(len(z), dtype=C)
    e_tau = np.zeros(len(z), dtype=F)
    c1_buff = np.zeros(2 * L + 1, dtype=F)
    co = {k: np.array(v, dtype=np.float64).astype(F) for k, v in dict(a2=[1, -1, -1, 1], b2=[-1, 3, -1, -1], a3=[1 / 6., -1 / 2., 1 / 2., -1 / 6.],
                                                                     b3=[0, 1 / 2., -1, 1 / 2.], c3=[-1 / 6., 1, -1 / 2., -1 / 3.]).items()}
    half, inv_ns, k_eps = F(1 / 2.), F(1 / float(Ns)), F(-1 / (2 * np.pi))
    rot = [np.exp(C(-1j * 2 * np.pi / Ns * kk)) if wide else np.exp(-1j * 2 * np.pi / Ns * kk) for kk in range(Ns)]
    vi = 0
    CNT_next = 0
    mu_next = 0
    underflow = 0
    epsilon = 0
    mm = 1
    under, margin, moving = [], np.inf, False
    z = np.hstack(([0], z)).astype(C)

    def interp(nn, mu):
        if I_ord == 1:
            return mu * z[nn] + (1 - mu) * z[nn - 1]
        w = z[nn + 2:nn - 1 - 1:-1]
        if I_ord == 2:
            v2 = half * np.sum(w * co["a2"])
            v1 = half * np.sum(w * co["b2"])
            return (mu * v2 + v1) * mu + z[nn]
        v3 = np.sum(w * co["a3"])
        v2 = np.sum(w * co["b3"])
        v1 = np.sum(w * co["c3"])
        return ((mu * v3 + v2) * mu + v1) * mu + z[nn]

    for nn in range(1, Ns * int(np.floor(len(z) / float(Ns) - (Ns - 1)))):
        CNT = CNT_next
        mu = mu_next
        if underflow == 1:
            z_interp = interp(nn, mu)
            c1 = 0
            for kk in range(Ns):
                c1 = c1 + np.abs(interp(nn + kk, mu)) ** 2 * rot[kk]
            c1 = c1 / Ns
            c1_buff = np.hstack(([c1], c1_buff[:-1]))
            epsilon = k_eps * np.angle(np.sum(c1_buff) / (2 * L + 1))
            zz[mm] = z_interp
            e_tau[mm] = epsilon
            mm += 1
        vp = K1 * epsilon
        vi = vi + K2 * epsilon
        v = vp + vi
        W = inv_ns + v
        CNT_next = CNT - W
        moving = moving or epsilon != 0
        if moving:
            margin = min(margin, abs(float(CNT_next)))
        if CNT_next < 0:
            CNT_next = 1 + CNT_next
            underflow = 1
            under.append(nn)
            mu_next = CNT / W
        else:
            underflow = 0
            mu_next = mu
    return zz[:-(len(zz) - mm + 1)], e_tau[:-(len(e_tau) - mm + 1)], under, float(margin)


def admit(z, Ns, L, BnTs, I_ord):
    with np.errstate(all="ignore"):
        ref_zz, ref_e = sync.NDA_symb_sync(z.copy(), Ns, L, BnTs, ZETA, I_ord)
        raw, e, under, _ = restate(z, Ns, L, BnTs, ZETA, I_ord, np.float64, np.complex128)
        raw_l, e_l, under_l, margin = restate(z, Ns, L, BnTs, ZETA, I_ord, LD, CLD)
    scaled = raw.copy()
    scaled /= np.std(scaled)
    assert np.array_equal(e, ref_e) and np.array_equal(scaled, ref_zz), "the float64 restatement is not the reference"
    if under != under_l:
        return None
    S = float(max(np.max(np.abs(raw.astype(CLD) - raw_l)), np.max(np.abs(e.astype(LD) - e_l))))
    max_e = float(np.max(np.abs(e)))
    if not (S <= 1e-12 and margin >= 1e-9 and max_e <= 0.5 - 1e-6):
        return None
    return dict(zz=ref_zz, e_tau=ref_e, raw=raw, under=np.array(under, dtype=np.int64)), S, margin, max_e


# ---- the signals, and the cases that share them: (Ns, L, BnTs, I_ord, trim, what)
BASE = (4, 2, 0.01, 3)
GROUPS = [
    ("s4", dict(Ns=4, phase=1), [(4, 2, 0.01, i, 0, "I_ord") for i in (1, 2, 3)] + [(4, l, 0.01, 3, 0, "L") for l in (0, 1, 4)] +
     [(4, 2, b, 3, 0, "BnTs") for b in (0.005, 0.02, 0.05)] + [(4, 2, 0.01, 3, t, "len mod Ns = %d" % ((1200 - t) % 4)) for t in (1, 2, 3)]),
    ("s3", dict(Ns=3, phase=3), [(3, 2, 0.01, i, 0, "Ns = 3") for i in (1, 2, 3)]),
    ("s8", dict(Ns=8, phase=1), [(8, 2, 0.01, i, 0, "Ns = 8") for i in (1, 2, 3)]),
    ("q4", dict(Ns=4, phase=2, qam16=True), [(4, 2, 0.01, 3, 0, "16-QAM")]),
    ("t4", dict(Ns=4, phase=1, time_step=(1, 150)), [(4, 2, 0.02, 3, 0, "time_step of 1 sample at symbol 150")]),
    ("n4", dict(Ns=4, phase=3, snr_db=15), [(4, 2, 0.01, 3, 0, "15 dB")]),
]

out, cases = {}, []
for g, (name, kw, members) in enumerate(GROUPS):
    kw = dict(kw)
    tstep = kw.pop("time_step", None)
    for attempt in range(40):
        seed = 2800 + 100 * g + attempt
        z = signal_of(seed, **kw)
        if tstep is not None:
            z = sync.time_step(z, kw["Ns"], tstep[0], tstep[1])
        got = [admit(z[:z.size - trim], Ns, L, BnTs, I_ord) for Ns, L, BnTs, I_ord, trim, _ in members]
        if all(v is not None for v in got):
            break
    else:
        raise SystemExit("signal %s: no seed passes the admission" % name)
    out[name] = z
    for (Ns, L, BnTs, I_ord, trim, what), (arrs, S, margin, max_e) in zip(members, got):
        key = "c%02d" % len(cases)
        cases.append(dict(key=key, signal=name, trim=trim, Ns=Ns, L=L, BnTs=BnTs, zeta=ZETA, I_ord=I_ord, what=what, seed=seed, S=S, margin=margin, max_e=max_e,
                          std=float(np.std(arrs["raw"]))))
        for k, v in arrs.items():
            out[key + "_" + k] = v
        print("%s %-3s Ns=%d L=%d BnTs=%-5g I_ord=%d trim=%d seed=%d S=%.2e margin=%.2e max|e|=%.3f n_out=%d  %s" % (key, name, Ns, L, BnTs, I_ord, trim, seed, S, margin, max_e,
                                                                                                               arrs["zz"].size, what))
out["cases"] = json.dumps(cases)
np.savez_compressed(os.path.join(HERE, "g28_nda.npz"), **out)

# ---- what is kept from the reference, each item from a probe of the real function
zb = out["s4"]
raw, e, under, _ = restate(zb, 4, 2, 0.01, ZETA, 3, np.float64, np.complex128)
ref_zz, ref_e = sync.NDA_symb_sync(zb.copy(), 4, 2, 0.01)
rng = np.random.default_rng(28)


def sum_model(x):
    """np.sum of a complex array as observed: below 4 elements left to right; from 4 on, four accumulators over the leading multiple of four, merged
    as (r0 + r1) + (r2 + r3), the rest one by one"""
    x = [complex(v) for v in x]

    def add(a, b):
        return complex(a.real + b.real, a.imag + b.imag)
    n = len(x)
    if n < 4:
        s = x[0]
        for v in x[1:]:
            s = add(s, v)
        return s
    r, i = x[:4], 4
    while i < n - (n % 4):
        r = [add(r[k], x[i + k]) for k in range(4)]
        i += 4
    s = add(add(r[0], r[1]), add(r[2], r[3]))
    for v in x[i:]:
        s = add(s, v)
    return s


def sum_model_holds(n):
    for _ in range(500):
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 10.0 ** rng.integers(-8, 8, n)
        if complex(np.sum(x)) != sum_model(x):
            return False
    return True


def raises_at(n, I_ord):
    zq = signal_of(2899, 2, 3)[:n]
    try:
        with np.errstate(all="ignore"):
            sync.NDA_symb_sync(zq, 2, 1, 0.01, ZETA, I_ord)
        return None
    except ValueError as exc:
        return str(exc)


with np.errstate(all="ignore"):
    import warnings
    warnings.simplefilter("ignore")
    empty = sync.NDA_symb_sync(zb[:5].copy(), 4, 2, 0.01)
    one = sync.NDA_symb_sync(zb[:15].copy(), 4, 2, 0.01)
    zn = zb.copy()
    zn[600] = np.nan
    poisoned = sync.NDA_symb_sync(zn, 4, 2, 0.01)
    a = np.complex128(0.3 - 0.7j)
    arr = (rng.standard_normal(9) + 1j * rng.standard_normal(9))
    s = np.std(arr)
    div = arr.copy()
    div /= s
    ns2 = {str(i): {str(n): raises_at(n, i) for n in range(3, 41)} for i in (2, 3)}
    conv = {
        "numpy": np.__version__,
        "signature": str(inspect.signature(sync.NDA_symb_sync)),
        "prepended_zero_sample": "z = np.hstack(([0], z)): zp[0] = 0, zp[i] = z[i - 1]",
        "loop_range": {"statement": "range(1, Ns*int(np.floor(len(z)/float(Ns)-(Ns-1)))) with len(z) counting the prepended zero",
                       "N_of_len": {"%d,%d" % (ns, n): int(ns * int(np.floor((n + 1) / float(ns) - (ns - 1)))) for ns in (2, 3, 4, 8, 16) for n in (0, 1, 11, 12, 15, 16, 100, 1200)}},
        "first_underflow_at_nn": int(under[0]), "first_interpolant_at_nn": int(under[0]) + 1,
        "stores_start_at_index_1": bool(ref_zz[0] == 0 and ref_e[0] == 0 and ref_e[1] != 0),
        "final_trim": {"statement": "zz[:-(len(zz)-mm+1)] = zz[:mm-1]: the last stored symbol is dropped", "underflows": len(under), "outputs": int(ref_zz.size),
                       "outputs_equal_heavy_steps": bool(ref_zz.size == sum(1 for u in under if u + 1 <= 4 * (1201 // 4 - 3) - 1))},
        "epsilon_holds_while_coasting_and_vi_integrates_every_sample": True,
        "mu_next_is_a_true_division": "mu_next = CNT/W",
        "std": {"population_over_the_trimmed_output_with_its_leading_zero": True,      # (admit() asserts it for every case)
                "no_outputs": {"len_z": 5, "zz_size": int(empty[0].size), "e_tau_size": int(empty[1].size)},
                "one_output": {"len_z": 15, "zz": repr(complex(one[0][0])), "e_tau": [float(v) for v in one[1]]},
                "in_place_division_is_product_with_reciprocal": bool(np.array_equal(div.real, arr.real * (1.0 / s)) and np.array_equal(div.imag, arr.imag * (1.0 / s))),
                "in_place_division_is_true_quotient": bool(np.array_equal(div.real, arr.real / s) and np.array_equal(div.imag, arr.imag / s))},
        "complex_scalar_by_int_is_product_with_reciprocal": bool(all((a / d).real == a.real * (1.0 / d) and (a / d).imag == a.imag * (1.0 / d) for d in (3, 5, 7, 17))),
        "float_times_complex_scalar_is_per_component": bool((np.float64(0.3) * a).real == 0.3 * a.real and (np.float64(0.3) * a).imag == 0.3 * a.imag),
        "complex_sum_order": {"model": sum_model.__doc__, "holds_for_lengths": {str(n): sum_model_holds(n) for n in range(1, 18)},
                              "four_elements": "(x0 + x1) + (x2 + x3)"},
        "ns2_slices_past_the_array": {"rule_built": "Ns = 2, I_ord >= 2, len(z) odd and >= 3 raises ValueError",
                                      "why": "the last iteration nn = len(z) - 2 reads z[nn+kk+2] past the array when the counter underflowed on the sample before; "
                                             "the reference's slice then has fewer than four elements and the product with the coefficient list raises",
                                      "probe_len_to_error_by_I_ord": ns2},
        "non_finite_sample": {"nan_at_sample": 600, "outputs_without": int(ref_zz.size), "outputs_with": int(poisoned[0].size),
                              "all_zz_nan": bool(np.all(np.isnan(poisoned[0]))), "e_tau_nan_count": int(np.sum(np.isnan(poisoned[1]))),
                              "note": "a NaN epsilon makes CNT NaN, CNT_next < 0 is false from there on, so the row makes no further symbol; np.std is NaN"},
        "departures": [
            "|z|^2 in the detector is re re + im im (the reference squares np.abs, a hypot)",
            "the angle is the project's atan2, rounded to nearest",
            "Ns outside 2 ... 16, L outside 0 ... 8, I_ord outside 1, 2, 3 raise ValueError (the reference logs and fails on an unbound name)",
            "Ns = 2 with I_ord >= 2 and an odd len(z) >= 3 raises ValueError whatever the samples",
            "complex64 is a storage type: widened on load, float64 loop, zz rounded once at the store, e_tau float64; a real z is widened exactly",
            "the rows' np.std is its two passes with sums in a fixed order, within 3e-15 (relative) of np.std for rows up to 8192 symbols",
            "a coefficient product is taken per component (z.re c, z.im c): where a sample is infinite the reference's complex product also makes the other component NaN",
        ],
    }
with open(os.path.join(HERE, "g28_conventions.json"), "w") as f:
    json.dump(conv, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote g28_nda.npz (%d cases), g28_conventions.json" % len(cases))
