#!/usr/bin/env python3
"""G18: the cascades of 7 - 8 biquads on which the float32 from-rest states of iir_par (V32) are tested, and per cascade and chunk
length the three detuned tones the host model of the admission (csrc/iir_par_plan.hpp: par_v32_input_error) ranks worst.

    python tests/golden/gen_golden_v32.py

  g18_v32_designs.npz   "names": the designs as scipy calls; "nsec"; "sos": [design][8][6], rows past nsec zero;
                        "worst_t128", "worst_t96": [design][3] frequencies in rad / sample -- the worst of a 0.001 rad grid over
                        +- 0.03 around every section's resonance, 96 chunks of 128 / 96 samples, by tests/host/iir_par_v32_emul.cpp --rank

The designs are scipy.signal's (data only: SOS rows); config 4 is g7_iir_sos.npz's sos8; the eq* ones are cascades of sigsys.peaking sections --
equalisers with 7 - 8 bands spread over the spectrum (centres in units of the Nyquist frequency: lin = linearly spaced, ho = half octaves down
from 0.9), the cascades of this size the admission still lets through once it probes detuned tones.  Which of them the library admits at which chunk
length is NOT stored: the tests ask the library (_ffi.sos_par_info).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
from sk_dsp_comm_amd.sigsys import peaking  # noqa: E402  (host code)


def equaliser(gains_db, centres, Q):
    """A peaking section per band; centres in units of the Nyquist frequency."""
    return np.array([np.r_[peaking(g, fc, Q, 2.0)] for g, fc in zip(gains_db, centres)])


def designs():
    e = lambda *a, **k: signal.ellip(*a, output="sos", **k)
    c = lambda *a, **k: signal.cheby1(*a, output="sos", **k)
    return [
        ("config4", np.load(os.path.join(HERE, "g7_iir_sos.npz"))["sos8"]),
        ("ellip(7,.5,60,[.45,.55],bp)", e(7, 0.5, 60, [0.45, 0.55], btype="bandpass")),
        ("ellip(7,.5,60,[.45,.55],bs)", e(7, 0.5, 60, [0.45, 0.55], btype="bandstop")),
        ("ellip(8,.5,60,[.3,.6],bp)", e(8, 0.5, 60, [0.3, 0.6], btype="bandpass")),
        ("cheby1(16,.5,.4,hp)", c(16, 0.5, 0.4, btype="highpass")),
        ("cheby1(14,.5,.6)", c(14, 0.5, 0.6)),
        ("cheby1(7,.5,[.2,.4],bs)", c(7, 0.5, [0.2, 0.4], btype="bandstop")),
        ("ellip(14,.5,60,.4)", e(14, 0.5, 60, 0.4)),
        ("cheby1(7,.5,[.2,.7],bp)", c(7, 0.5, [0.2, 0.7], btype="bandpass")),      # (the resonance-only probe admitted it on 128-sample chunks only)
        ("cheby1(16,.5,.8)", c(16, 0.5, 0.8)),                                    # (... on 96-sample chunks only)
        ("ellip(8,.5,60,[.1,.2],bp)[:8]", e(8, 0.5, 60, [0.1, 0.2], btype="bandpass")[:8]),   # refused
        ("butter(8,[.2,.3],bp)", signal.butter(8, [0.2, 0.3], btype="bandpass", output="sos")),   # refused
        ("eq8lin(+12,Q2)", equaliser([12.0] * 8, np.linspace(0.1, 0.9, 8), 2.0)),
        ("eq7lin(+12,Q2)", equaliser([12.0] * 7, np.linspace(0.12, 0.88, 7), 2.0)),      # admitted on 96-sample chunks only
        ("eq8lin(v,Q1)", equaliser([9.0, 6.0, 3.0, 0.5, -3.0, -6.0, 3.0, 9.0], np.linspace(0.1, 0.9, 8), 1.0)),
        ("eq8ho(+6,Q3.5)", equaliser([6.0] * 8, 0.9 * 2.0 ** (-0.5 * np.arange(8)), 3.5)),
    ]


def designs_text(names, soss, worst=None):
    """The text tests/host/iir_par_v32_emul.cpp reads."""
    lines = []
    for i, (name, sos) in enumerate(zip(names, soss)):
        lines.append("design %s %d" % (name, len(sos)))
        lines += [" ".join("%.17g" % v for v in row) for row in sos]
        for T, w in (worst[i] if worst else {}).items():
            lines.append("worst %d %s" % (T, " ".join("%.17g" % v for v in w)))
    return "\n".join(lines) + "\n"


def main():
    ds = designs()
    names = [n for n, _ in ds]
    assert all(len(s) in (7, 8) and s.shape[1] == 6 for _, s in ds)
    with tempfile.TemporaryDirectory() as tmp:
        exe, txt = os.path.join(tmp, "iir_par_v32_emul"), os.path.join(tmp, "designs.txt")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "iir_par_v32_emul.cpp"), "-o", exe])
        with open(txt, "w") as f:
            f.write(designs_text(names, [s for _, s in ds]))
        out = subprocess.run([exe, "--rank", txt], stdout=subprocess.PIPE, check=True).stdout.decode()
    worst = {128: np.zeros((len(ds), 3)), 96: np.zeros((len(ds), 3))}
    for line in out.splitlines():
        w = line.split()
        assert w[0] == "worst" and len(w) == 6, line
        worst[int(w[2])][names.index(w[1])] = [float(v) for v in w[3:]]
    assert np.all(worst[128] > 0) and np.all(worst[96] > 0)
    sos = np.zeros((len(ds), 8, 6))
    for i, (_, s) in enumerate(ds):
        sos[i, :len(s)] = s
    np.savez(os.path.join(HERE, "g18_v32_designs.npz"), names=np.array(names), nsec=np.array([len(s) for _, s in ds]), sos=sos,
             worst_t128=worst[128], worst_t96=worst[96])
    for i, n in enumerate(names):
        print("%-32s %d sections; worst detuned tones T = 128: %s  T = 96: %s" % (n, len(ds[i][1]), np.round(worst[128][i], 4), np.round(worst[96][i], 4)))


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
