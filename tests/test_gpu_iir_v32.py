"""GPU test of the V32 admission of the parallel-form IIR scan (csrc/iir_par.hip, csrc/iir_par_plan.hpp: par_v32_probe): cascades of 7 - 8
biquads from four filter families (tests/golden/g18_v32_designs.npz), float32 and complex64, on the inputs the float32 from-rest states are
worst on -- tones ON and NEAR every section's resonance, the detuned tones the host model ranks worst -- and on noise, DC and Nyquist;
.filter, .dn and .up, which between them run both chunk lengths (128 and 96 samples).  49152 samples: 384 chunks of 128, 512 of 96, several
wave segments.

The reference is the float64 cascade of the CPU oracle (scipy.signal.sosfilt restated).  The bound is the float32 contract: 1e-6 of
max(output peak, 1 % of the forward bound l1(h) max|x|) -- the scale the host probe uses -- at the default options, for every design,
input and call.  Which engine ran is asserted too: `iir_par_v32` is recorded exactly where the library admits the filter at the chunk
length the call runs (_ffi.sos_par_info: v32_admitted for 128, v32_admitted_t96 for 96) -- for .filter and .up; .dn keeps the float64 states.

Measured before the probe ran detuned tones and while .dn took the float32 states (MI355X): BASELINE config 4, admitted at 4.0e-7, 1.46e-6 on a
tone 0.009 rad above its upper edge resonance; 9 of the 10 designs admitted then above 1e-6, up to 2.7e-6.  With the detuned tones in the probe
and .dn still on float32 states: the 8-band equaliser admitted at 4.4e-7 showed 1.6e-6 of the KEPT outputs' peak on .dn(x, 5) of a sine on its
lowest resonance (the full-rate output peaks at 27, every fifth sample at 8.9)."""
import os

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi
from oracle import oracle as orc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL32 = 1e-6
N = 49152
DETUNE = (-0.03, -0.01, -0.003, 0.003, 0.01, 0.03)

_Z = np.load(os.path.join(GOLDEN, "g18_v32_designs.npz"))
NAMES = [str(s) for s in _Z["names"]]

# The parallel form serves filters that forget their state within 4 wave segments.  This low-pass (pole radius 0.9993) does not: every call runs the
# cascade scan kernels (`iir_scan`), which have no float32 from-rest form, whatever the probe says.  The contract holds for it all the same.
NOT_SERVED = {"ellip(14,.5,60,.4)"}

# (name, decimation, interpolation): every call the float32 from-rest states serve
CALLS = [("filter", 1, 1), ("dn3", 3, 1), ("dn4", 4, 1), ("dn5", 5, 1), ("up2", 1, 2), ("up3", 1, 3), ("up4", 1, 4)]


def chunk_length(call, cplx):
    """The chunk length par_choose gives the call at the default options, 7 - 8 biquads: 96 samples for .dn by a divisor of 96 -- through more
    than 4 biquads complex64 signals only where 3 divides M -- and for .up by 3; 128 for the rest."""
    if call in ("dn3", "up3"):
        return 96
    if call == "dn4":
        return 128 if cplx else 96
    return 128


def float32_states(call):
    """.filter and .up may run the float32 from-rest states; .dn never does (the peak of the outputs it keeps is not the probe's scale)."""
    return not call.startswith("dn")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _ffi.init()
    assert "gfx950" in _ffi.device_info()["name"]
    yield


def _design(name):
    i = NAMES.index(name)
    return _Z["sos"][i, :_Z["nsec"][i]].copy(), {128: _Z["worst_t128"][i], 96: _Z["worst_t96"][i]}


def _inputs(sos, worst):
    """name -> (kind, f(i, L)): the full-rate input is f(arange(N), 1); the input of .up by L is f(arange(N // L), L) -- a tone of frequency w is
    cos(L w i) there, so that the zero-stuffed signal has an image on w."""
    rng = np.random.default_rng(18)
    noise = rng.standard_normal(N)
    ins = {"noise": ("plain", lambda i, L: noise[:len(i)]), "dc": ("plain", lambda i, L: np.ones(len(i))), "nyquist": ("plain", lambda i, L: (-1.0) ** i)}
    tone = lambda w, fn: (lambda i, L: fn(L * w * i))
    for k, (a1, a2, r0, r1) in enumerate(_ffi.sos_par_info(sos)["sections"]):
        if a2 > 0 and a1 * a1 < 4 * a2:
            th = float(np.arccos(-a1 / (2 * np.sqrt(a2))))
            ins["res%d cos" % k] = ("res", tone(th, np.cos))
            ins["res%d sin" % k] = ("res", tone(th, np.sin))
            for d in DETUNE:
                if 0 < th + d < np.pi:
                    ins["res%d %+.3f" % (k, d)] = ("detuned", tone(th + d, np.cos))
    for T in (128, 96):
        for j, w in enumerate(worst[T]):
            ins["worst%d_t%d %.4f" % (j, T, w)] = ("worst", tone(float(w), np.cos))
    return ins


def _signal(f, L, dtype):
    x = f(np.arange(N // L, dtype=np.float64), L).astype(np.float32)
    if dtype == np.complex64:
        x = (x + 1j * np.roll(x, 17)).astype(np.complex64)
    return x


@pytest.mark.parametrize("dtype", [np.float32, np.complex64], ids=["float32", "complex64"])
@pytest.mark.parametrize("name", NAMES)
def test_v32_admission_holds_the_contract(name, dtype):
    """Every design, input and call inside 1e-6 at the default options; the float32 engine exactly where the library says it admitted the
    filter; with iir_par_v32 = 0 the float64-state engine, inside the same bound (resonance and stored worst tones).  Printed per chunk length:
    the worst measured error of the admitted engine, the probe's value, their ratio; forced runs (iir_par_v32 = 2) of refused designs are printed
    only."""
    sos, worst = _design(name)
    cplx = dtype == np.complex64
    info = _ffi.sos_par_info(sos)
    assert info["accepted"] and len(sos) in (7, 8)
    served = name not in NOT_SERVED
    admitted = {128: served and info["v32_admitted"], 96: served and info["v32_admitted_t96"]}
    probe = {128: info["v32_err"], 96: info["v32_err_t96"]}
    imp = np.zeros(8192)
    imp[0] = 1.0
    l1h = float(np.sum(np.abs(orc.sos_filter(sos, imp))))
    assert _ffi.get_option("iir_par_v32") == 1
    k = _ffi.IirKernel(_ffi.code_of(dtype), sos=sos)

    # inputs and float64 references, once
    cases = []   # (input name, kind, call, T, x, ref, scale)
    for iname, (kind, f) in _inputs(sos, worst).items():
        x1 = _signal(f, 1, dtype)
        ref1 = orc.sos_filter(sos, x1)
        floor1 = 1e-2 * l1h * float(np.max(np.abs(x1)))
        for call, M, L in CALLS:
            T = chunk_length(call, cplx)
            if L == 1:
                ref = ref1 if M == 1 else orc.downsample(ref1, M)   # (orc.sos_dn: downsample(sos_filter(sos, x), M))
                assert M == 1 or iname != "noise" or np.array_equal(ref, orc.sos_dn(sos, x1, M))
                cases.append((iname, kind, call, T, x1, ref, max(float(np.max(np.abs(ref))), floor1)))
            else:
                xl = _signal(f, L, dtype)
                ref = orc.sos_filter(sos, L * orc.upsample(xl, L))
                cases.append((iname, kind, call, T, xl, ref, max(float(np.max(np.abs(ref))), 1e-2 * l1h * L * float(np.max(np.abs(xl))))))

    def run(call, x):
        _ffi.debug_path()
        if call == "filter":
            y = k.filter(x)
        elif call.startswith("dn"):
            y = k.dn(x, int(call[2:]))
        else:
            y = k.up(x, int(call[2:]))
        return np.asarray(y), _ffi.debug_path()

    failures = []
    worst_on = {128: (0.0, ""), 96: (0.0, "")}
    for iname, kind, call, T, x, ref, scale in cases:
        y, path = run(call, x)
        e = float(np.max(np.abs(y - ref))) / scale
        f32 = bool(admitted[T]) and float32_states(call)
        if ("iir_par" in path) != served or ("iir_par_v32" in path) != f32:
            failures.append("%s %s: path %s, admitted at T = %d: %s" % (call, iname, path, T, admitted[T]))
        if not e <= TOL32:
            failures.append("%s %s (T = %d, %s): %.3e" % (call, iname, T, "float32 states" if f32 else "float64 states", e))
            print("OVER %s %s %s" % (name, np.dtype(dtype).name, failures[-1]))
        if f32 and e > worst_on[T][0]:
            worst_on[T] = (e, "%s %s" % (call, iname))
    for T in (128, 96):
        if admitted[T]:
            print("V32 %s %s T = %d: measured worst %.3e (%s), probe %.3e, ratio %.2f" % (name, np.dtype(dtype).name, T, worst_on[T][0], worst_on[T][1],
                                                                                         probe[T], worst_on[T][0] / probe[T]))
        else:
            print("V32 %s %s T = %d: %s, probe %.3e" % (name, np.dtype(dtype).name, T, "refused" if served else "not served by the parallel form", probe[T]))

    # the float64-state engine on the tones, and the float32 one forced where the probe refused it (printed only)
    tones = [c for c in cases if c[1] in ("res", "worst")]
    worst_off, where_off = 0.0, ""
    with _ffi.option("iir_par_v32", 0):
        for iname, kind, call, T, x, ref, scale in tones:
            y, path = run(call, x)
            e = float(np.max(np.abs(y - ref))) / scale
            if ("iir_par" in path) != served or "iir_par_v32" in path:
                failures.append("iir_par_v32 = 0, %s %s: path %s" % (call, iname, path))
            if not e <= TOL32:
                failures.append("iir_par_v32 = 0, %s %s: %.3e" % (call, iname, e))
            if e > worst_off:
                worst_off, where_off = e, "%s %s" % (call, iname)
    print("F64 %s %s: float64 from-rest states, worst %.3e (%s)" % (name, np.dtype(dtype).name, worst_off, where_off))
    if served and not (admitted[128] and admitted[96]):
        forced = {128: (0.0, ""), 96: (0.0, "")}
        with _ffi.option("iir_par_v32", 2):
            for iname, kind, call, T, x, ref, scale in tones:
                if admitted[T] or not float32_states(call):
                    continue
                y, path = run(call, x)
                e = float(np.max(np.abs(y - ref))) / scale
                if "iir_par_v32" not in path:
                    failures.append("iir_par_v32 = 2, %s %s: path %s" % (call, iname, path))
                if e > forced[T][0]:
                    forced[T] = (e, "%s %s" % (call, iname))
        for T in (128, 96):
            if not admitted[T]:
                print("FORCED %s %s T = %d: float32 states forced on the refused design, worst %.3e (%s), probe %.3e" % (name, np.dtype(dtype).name, T,
                                                                                                                       forced[T][0], forced[T][1], probe[T]))
    assert not failures, "%d of %d: %s" % (len(failures), len(cases), "; ".join(failures[:12]))
