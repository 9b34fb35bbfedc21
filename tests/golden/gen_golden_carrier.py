#!/usr/bin/env python3
"""G27: carrier phase tracking -- synchronization.DD_carrier_sync (synchronization.py:169-275), phase_step (:295-313) and time_step (:278-292) --
results from the REAL reference (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_carrier.py

  g27_carrier.npz       "cases": JSON list of {key, mod_type, M, type, snr_db, f0, phi0, BnTs, zeta, open_loop, phase_step, seed, S, min_margin}:
                        <key>_z (complex128, 600 symbols) -> <key>_z_prime, <key>_a_hat, <key>_e_phi, <key>_theta_h as the reference returned them.
                        S is the yardstick of tests/test_carrier_cpu.py: the loop once more in np.longdouble / np.clongdouble (the same statements, the
                        same float64 gains and 2 pi), and the largest absolute difference between the two runs over z_prime and e_phi and the largest
                        circular difference of theta_h -- the reference's own rounding noise as the loop amplifies it.
                        "steps": JSON list of {key, fn, ns, step, n_step}: <key>_z -> <key>_y of phase_step / time_step.
  g27_conventions.json  signatures, the NumPy version, the departures, and the observations the restatement rests on

A case is admitted only if S <= 1e-12, both runs make the same decisions, and every z' lies at least 1e-6 from a decision threshold (in the units of
the decision: the shifted and halved axis for QAM, the angle index for MPSK).  A case that fails is drawn again with the next seed; the admission is
never relaxed.  For MPSK above 4 the reference calls .astype(np.int): the script sets np.int = int first and records that it did.
"""
import inspect
import json
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
# NumPy's complex array product is dispatched by CPU: on a core with FMA3 its SIMD loop fuses (re = fma(a, c, -(b d))), elsewhere it is the written form
# re = a c - b d, im = a d + b c -- which is also what a scalar product gives everywhere.  The capture pins the written form, so that phase_step's
# expected outputs do not depend on the machine that ran this script; the probe below checks that it took, and g27_conventions.json records it.
DISPATCH_OFF = "FMA3 AVX2 AVX512F AVX512CD AVX512_KNL AVX512_KNM AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"
os.environ["NPY_DISABLE_CPU_FEATURES"] = DISPATCH_OFF
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("SK_DSP_COMM_SRC", "/root/reference/src"))

import numpy as np  # noqa: E402

from sk_dsp_comm import synchronization as sync  # noqa: E402

LD, CLD = np.longdouble, np.clongdouble
N_SYMB, ZETA = 600, 0.707
TWO_PI = 2 * np.pi

_pr = np.random.default_rng(27)
_pa, _pb = _pr.standard_normal(4096) + 1j * _pr.standard_normal(4096), np.exp(1j * _pr.standard_normal(4096))
_written = np.array([complex(u) * complex(v) for u, v in zip(_pa, _pb)])        # the scalar product: re = a c - b d, im = a d + b c
assert np.array_equal(_pa * _pb, _written), "NumPy's array product still fuses: the dispatch was not switched off"

# ---- what NumPy >= 1.24 does to the MPSK > 4 branch
z8 = np.exp(1j * 2 * np.pi * np.arange(8) / 8)
had_np_int = hasattr(np, "int")
try:
    sync.DD_carrier_sync(z8, 8, 0.05)
    mpsk8_raises = None
except AttributeError as exc:
    mpsk8_raises = "AttributeError: %s" % exc
if not had_np_int:
    np.int = int


def points(mod_type, M):
    if mod_type == 'MQAM':
        x_m = int(round(np.sqrt(M))) - 1
        lv = 2 * np.arange(x_m + 1) - x_m
        return (lv[:, None] + 1j * lv[None, :]).reshape(-1)
    if M == 2:
        return np.array([-1.0 + 0j, 1.0 + 0j])
    if M == 4:
        return np.array([1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j]) / np.sqrt(2)
    return np.exp(1j * 2 * np.pi * np.arange(M) / M)


def signal_of(seed, mod_type, M, snr_db, f0, phi0):
    rng = np.random.default_rng(seed)
    pts = points(mod_type, M)
    s = pts[rng.integers(0, pts.size, N_SYMB)]
    sigma = np.sqrt(np.mean(np.abs(pts) ** 2) / (2 * 10 ** (snr_db / 10)))
    w = sigma * (rng.standard_normal(N_SYMB) + 1j * rng.standard_normal(N_SYMB))
    return (s + w) * np.exp(1j * (phi0 + 2 * np.pi * f0 * np.arange(N_SYMB)))


def loop_longdouble(z, M, BnTs, zeta, mod_type, det, open_loop):
    """the loop in np.longdouble: the yardstick run.  Returns (z_prime, a_hat, e_phi, theta_h, margins) with margins the distance of every z' from the
    nearest decision threshold, in the decision's units."""
    K1 = LD(4 * zeta / (zeta + 1 / (4 * zeta)) * BnTs)
    K2 = LD(4 / (zeta + 1 / (4 * zeta)) ** 2 * BnTs ** 2)
    z = z.astype(CLD)
    scale = LD(1)
    if mod_type == 'MQAM':
        scale = np.std(z) * np.sqrt(LD(3) / (2 * (M - 1)))
        z = z / scale
    n = len(z)
    zp, ah = np.zeros(n, dtype=CLD), np.zeros(n, dtype=CLD)
    e, th, margin = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.zeros(n)
    theta, vi, two_pi = LD(0), LD(0), LD(TWO_PI)
    for k in range(n):
        zp[k] = z[k] * np.exp(CLD(-1j) * theta)
        if mod_type == 'MPSK':
            u = np.angle(zp[k]) * M / 2 / LD(np.pi)
            if M == 2:
                ah[k] = np.sign(zp[k].real)
                margin[k] = abs((u - LD(0.5)) - np.rint(u - LD(0.5)))
            elif M == 4:
                ah[k] = (np.sign(zp[k].real) + 1j * np.sign(zp[k].imag)) / np.sqrt(LD(2))
                margin[k] = abs(u - np.rint(u))
            else:
                ah[k] = np.exp(CLD(1j) * 2 * LD(np.pi) * np.mod(np.rint(u), M) / M)
                margin[k] = abs((u - LD(0.5)) - np.rint(u - LD(0.5)))
        else:
            x_m = 1 if M == 2 else int(round(np.sqrt(M))) - 1
            sh = (zp[k] + x_m * (1 + 1j)) / 2
            ah[k] = 2 * (np.clip(np.rint(sh.real), 0, x_m) + 1j * np.clip(np.rint(sh.imag), 0, x_m)) - x_m * (1 + 1j)
            cuts = np.arange(x_m) + 0.5
            margin[k] = min(np.min(np.abs(float(sh.real) - cuts)), np.min(np.abs(float(sh.imag) - cuts)))
        if det == 0:
            e[k] = zp[k].imag * ah[k].real - zp[k].real * ah[k].imag
        elif det == 1:
            e[k] = np.angle(np.exp(CLD(1j) * (np.angle(zp[k]) - np.angle(ah[k]))))
        else:
            e[k] = np.imag(zp[k] / ah[k])
        vi = vi + K2 * e[k]
        theta = np.mod(theta + (K1 * e[k] + vi), two_pi)
        th[k] = theta
        if open_loop:
            theta = LD(0)
    return zp * scale, ah, e, th, margin


def circ(d):
    d = np.mod(np.abs(np.asarray(d, dtype=LD)), LD(TWO_PI))
    return np.minimum(d, LD(TWO_PI) - d)


def admit(z, M, BnTs, mod_type, det, open_loop):
    """(outputs of the reference, S, smallest margin) or None"""
    with np.errstate(all="ignore"):
        ref = sync.DD_carrier_sync(z.copy(), M, BnTs, ZETA, mod_type, det, open_loop)
        zp, ah, e, th, margin = loop_longdouble(z, M, BnTs, ZETA, mod_type, det, open_loop)
    S = float(max(np.max(np.abs(ref[0].astype(CLD) - zp)), np.max(np.abs(ref[2].astype(LD) - e)), np.max(circ(ref[3].astype(LD) - th))))
    same = bool(np.all(np.abs(ref[1].astype(CLD) - ah) < 1e-9))
    if not (S <= 1e-12 and same and margin.min() >= 1e-6):
        return None
    return ref, S, float(margin.min())


#        mod_type  M   type snr  f0    phi0  BnTs
TABLE = [('MPSK', 2, 0, 15, 1e-3, 0.3, 0.05), ('MPSK', 2, 1, 15, 1e-3, 0.3, 0.05), ('MPSK', 4, 0, 15, 1e-3, 0.3, 0.05), ('MPSK', 4, 1, 15, 1e-3, 0.3, 0.05),
         ('MPSK', 8, 0, 25, 1e-3, 0.2, 0.05), ('MPSK', 8, 1, 25, 5e-4, 0.2, 0.02), ('MPSK', 16, 0, 30, 0.0, 0.1, 0.02),
         ('MQAM', 4, 0, 20, 1e-3, 0.3, 0.05), ('MQAM', 16, 0, 30, 1e-3, 0.3, 0.05), ('MQAM', 16, 2, 30, 1e-3, 0.3, 0.05), ('MQAM', 16, 1, 30, 5e-4, 0.2, 0.05),
         ('MQAM', 64, 0, 40, 0.0, 0.1, 0.001), ('MQAM', 64, 2, 40, 2e-4, 0.1, 0.02), ('MQAM', 256, 1, 50, 1e-4, 0.05, 0.02), ('MQAM', 256, 2, 50, 1e-4, 0.05, 0.02)]
#        ... and one open-loop case and one with a phase step of 0.4 rad at symbol 200 through the reference's phase_step
EXTRA = [('MPSK', 4, 0, 15, 0.0, 0.3, 0.05, True, None), ('MPSK', 4, 0, 15, 0.0, 0.1, 0.05, False, (0.4, 200))]

out, cases = {}, []
for i, row in enumerate([t + (False, None) for t in TABLE] + EXTRA):
    mod_type, M, det, snr_db, f0, phi0, BnTs, open_loop, pstep = row
    for attempt in range(40):
        seed = 2700 + 100 * i + attempt
        z = signal_of(seed, mod_type, M, snr_db, f0, phi0)
        if pstep is not None:
            z = sync.phase_step(z, 1, pstep[0], pstep[1])
        got = admit(z, M, BnTs, mod_type, det, open_loop)
        if got is not None:
            break
    else:
        raise SystemExit("case %r: no seed passes the admission; lower its BnTs" % (row,))
    ref, S, margin = got
    key = "c%02d" % i
    cases.append(dict(key=key, mod_type=mod_type, M=M, type=det, snr_db=snr_db, f0=f0, phi0=phi0, BnTs=BnTs, zeta=ZETA, open_loop=open_loop,
                      phase_step=pstep, seed=seed, S=S, min_margin=margin))
    out[key + "_z"] = z
    for name, v in zip(("z_prime", "a_hat", "e_phi", "theta_h"), ref):
        out[key + "_" + name] = np.asarray(v)
    print("%s %-5s M=%-3d type=%d seed=%d S=%.2e margin=%.2e" % (key, mod_type, M, det, seed, S, margin))
out["cases"] = json.dumps(cases)

# ---- phase_step / time_step: ns in (1, 4), the step inside, at and beyond the end of a 96-sample waveform
steps = []
rs = np.random.default_rng(2799)
zw = rs.standard_normal(96) + 1j * rs.standard_normal(96)
for ns in (1, 4):
    for n_step in (5, 96 // ns - 1, 96 // ns, 200):
        key = "p%02d" % len(steps)
        steps.append(dict(key=key, fn="phase_step", ns=ns, step=0.4, n_step=n_step))
        out[key + "_z"], out[key + "_y"] = zw, sync.phase_step(zw, ns, 0.4, n_step)
        for t_step in (3, 7):
            key = "p%02d" % len(steps)
            steps.append(dict(key=key, fn="time_step", ns=ns, step=t_step, n_step=n_step))
            out[key + "_z"], out[key + "_y"] = zw, sync.time_step(zw, ns, t_step, n_step)
out["steps"] = json.dumps(steps)
np.savez_compressed(os.path.join(HERE, "g27_carrier.npz"), **out)

# ---- the observations the restatement rests on
zq, zero = np.complex128(0.3 - 0.2j), np.complex128(0j)
with np.errstate(all="ignore"):
    quot = zq / zero
    conv = {
        "numpy": np.__version__,
        "signatures": {f: str(inspect.signature(getattr(sync, f))) for f in ("DD_carrier_sync", "phase_step", "time_step")},
        "mpsk_above_4": {"numpy_had_np_int": had_np_int, "reference_raises": mpsk8_raises, "script_set_np_int_to_int": not had_np_int,
                         "built_instead": "mod(rint(angle * M / 2 / pi), M)"},
        "mod_of_a_negative_sum": {"sum": -1.25, "np_mod": float(np.mod(-1.25, TWO_PI)), "fmod_plus_2pi": float(np.fmod(-1.25, TWO_PI) + TWO_PI),
                                  "tiny_negative_gives_2pi": bool(np.mod(-1e-20, TWO_PI) == TWO_PI), "zero_remainder": float(np.mod(-TWO_PI, TWO_PI))},
        "sign_of_zero": [float(np.sign(0.0)), float(np.sign(-0.0))],
        "rint_ties": {str(v): float(np.rint(v)) for v in (0.5, 1.5, 2.5, -0.5)},
        "quotient_by_zero_decision": {"z": [zq.real, zq.imag], "imag": repr(float(quot.imag)), "real": repr(float(quot.real))},
        "quotient_by_sqrt2": {"is_product_with_reciprocal": bool((np.complex128(1 + 1j) / np.sqrt(2)).real == 1.0 * (1.0 / np.sqrt(2))),
                              "reciprocal": float(1.0 / np.sqrt(2)).hex(), "sqrt_half": float(np.sqrt(0.5)).hex()},
        "exp_of_minus_1j_0": repr(complex(np.exp(-1j * 0))),
        "complex_array_product": {"numpy_dispatch_disabled_for_the_capture": DISPATCH_OFF, "equals_the_written_form_re_ac_minus_bd": True,
                                  "note": "with FMA3 dispatched NumPy's SIMD loop computes re = fma(a, c, -(b d)), im = fma(a, d, b c): machine dependent"},
        "departures": [
            "MPSK above 4: the reference's .astype(np.int) raises AttributeError with NumPy >= 1.24; the documented intent is built, M up to 32",
            "an unsupported M, mod_type or type raises ValueError (the reference prints a message and returns zeros)",
            "z must be complex (the reference fails on a real array when it stores a complex value into zeros_like(z))",
            "complex64 is a storage type: widened on load, float64 loop, z_prime / a_hat rounded once at the store, e_phi / theta_h float64",
            "sincos (2 ulp) and atan2 (rounded to nearest) are the project's own, the same bits on host and device",
            "the MQAM scale is the deterministic moment merge; z / z_scale is z r per component with r = 1 / z_scale, z_prime leaves times 1 / r",
            "phase_step / time_step of complex64 return complex64; negative steps are refused",
        ],
    }
with open(os.path.join(HERE, "g27_conventions.json"), "w") as f:
    json.dump(conv, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote g27_carrier.npz (%d cases, %d steps), g27_conventions.json" % (len(cases), len(steps)))
