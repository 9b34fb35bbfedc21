"""The transform-based FIR engines held to the error spectrum of a host overlap-save in their own precision (tests/_errspec.py).

Every other accuracy test of these engines asks whether max |y - ref| stays under 1e-6 of the output's peak (1e-10 or 1e-11 in float64), with
low-pass taps.  An error confined to one twiddle entry, one bin of a taps spectrum or one output position of a tile is diluted over the
tile before it reaches that figure (tests/test_errspec_cpu.py shows how far).  Here every engine runs once over 64 + 1 segments of 8192
outputs (L times that for .up) of Gaussian noise and three figures of e = y - ref are taken behind the first segment:

    R   ||e|| / ||ref||                                                     limit 2 x the yardstick's
    A   the largest bin of the averaged 8192-point spectrum of e over the   limit 4 x the yardstick's
        running median of its 129 neighbours (.up: also per output phase)
    B   the largest of |e|^2 per position of the engine's output period V   limit 4 x the yardstick's
        over the median position

The yardstick is the same filter by overlap-save on the host, scipy.fft in complex64 (complex128 for the float64 engines) at the engine's
tile size, measured in the test on the same input against the same reference; no limit is set against a kernel.  R: both sides are a forward
transform, a product and an inverse transform of N points in one precision and differ in how N is split into passes; rounding error grows
like the square root of the number of passes, and three passes against radix-2's thirteen is a factor 2.1 at most.  A and B: noise power 2 : 1
between neighbouring bins or positions is still legitimate (bins with exact twiddles), and the factor leaves that a further 2.

Taps: one unit impulse per polyphase branch (the expected output is a shifted copy of the input, exact in float64 too) and, for the
single-precision engines, the dense full-band chirp against the float64 oracle.

V per engine (csrc/ols_tables.hpp: tile_overlap): fir_ols / fir_ols_rep 8192 - (taps - 1 rounded up to 512), for .dn in
input samples (output j at position j M mod V); fir_up4k / fir_up2k (4096 / 2048 - (taps per phase - 1 rounded up to 256 / 64)) L outputs;
fir_dn4k 4096 - (taps per phase - 1 rounded up to 256) outputs; fir_ols64 4096 - (taps - 1 rounded up to 256), fir_ols64_up that of a phase
times L; fir_bank4k 4096 - (taps - 1 rounded up to 256).  The fused resampler runs whatever AUTO picks, whose period no constant documents:
B is left out there.

The bank has one prototype filter for all rows, so "impulses at different taps" are three impulses of the prototype (the positions of the F = 3
set): row j is sum_i exp(2 pi j ((s_j d_i) mod period) / period) x[n - d_i], three rotated copies of the input.

One positive control per precision runs the unchanged kernel on impulse taps plus delta exp(2 pi j k0 n / 8192) / P, which lifts the taps spectrum
by delta = 3e-6 (complex64) / 3e-15 (complex128) around bin k0, against the reference of the unperturbed taps: the call still meets
today's contract, and A is over its limit with its peak inside the perturbation's main lobe (8192 / (2 P) bins to either side of k0).

Every case prints one line, and all of them are written as JSON to the file that the environment variable SKDSP_ERRSPEC_JSON names, when it is
set; profiles/errspec/README.md holds the table measured when this file was written."""
import contextlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sk_dsp_comm_amd import _ffi, sigsys as ss  # noqa: E402
from oracle import oracle as orc  # noqa: E402
import _errspec as es  # noqa: E402

NOUT = (es.MIN_SEGMENTS + 1) * es.SEG   # outputs analysed per case (per phase for .up)
SEED = 20
R_FACTOR, A_FACTOR, B_FACTOR = 2.0, 4.0, 4.0
_REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _ffi.init()
    assert "gfx950" in _ffi.device_info()["name"]
    yield
    out = os.environ.get("SKDSP_ERRSPEC_JSON")
    if out and _REPORT:
        with open(out, "w") as f:
            json.dump(_REPORT, f, indent=0)


def is_double(dt):
    return np.dtype(dt) in (np.dtype(np.float64), np.dtype(np.complex128))


def is_complex(dt):
    return np.dtype(dt).kind == "c"


class Case:
    """One engine call: what = filter / up / dn / updn, rate = (L, M), the options that force the engine, the engine's name in
    _ffi.debug_path() (None: printed only), its tile size N, the overlap the yardstick takes (None: taps - 1) and the period / step of B."""

    def __init__(self, name, engine, dt, ntaps, what, L=1, M=1, opts=(), force_ols=False, N=8192, overlap=None, period=None, step=1):
        self.name, self.engine, self.dt, self.ntaps, self.what, self.L, self.M = name, engine, dt, ntaps, what, L, M
        self.opts, self.force_ols, self.N, self.overlap, self.period, self.step = dict(opts), force_ols, N, overlap, period, step
        self.F = L if what in ("up", "updn") else M

    def id(self):
        return "%s-%s-%s-%d" % (self.name, np.dtype(self.dt).name, self.what + ("" if self.what == "filter" else
                                "%d" % self.L if self.what == "up" else "%d" % self.M if self.what == "dn" else "%d_%d" % (self.L, self.M)), self.ntaps)


def _cases():
    c = []
    S = (np.complex64, np.float32)
    for dt in S:                                                   # fir_ols: ols_tile_kernel
        for P in (300, 1024, 4097):
            ov, V = es.tile_overlap(P, 512, 8192)
            c.append(Case("ols", "fir_ols", dt, P, "filter", force_ols=True, overlap=ov, period=V))
    ov, V = es.tile_overlap(1024, 512, 8192)
    for dt in S:                                                   # ols_fold_kernel
        for M in (2, 4):
            c.append(Case("fold", "fir_ols", dt, 1024, "dn", M=M, opts={"fir_dn_fold": 1, "fir_dn4k": 0}, force_ols=True, overlap=ov, period=V, step=M))
    c.append(Case("decstore", "fir_ols", np.complex64, 1024, "dn", M=3, opts={"fir_dn4k": 0}, force_ols=True, overlap=ov, period=V, step=3))
    for dt in S:                                                   # ols_rep_kernel
        for L in (4, 12):
            c.append(Case("rep", "fir_ols_rep", dt, 1024, "up", L=L, opts={"fir_up_rep": 2}, force_ols=True, overlap=ov, period=V))
    for dt in S:                                                   # up4k_kernel (five passes or more go to the 2048-point tile unless it is off)
        for P in (1024, 516):
            for L in (2, 3, 4, 12):
                V4 = es.tile_overlap(-(-P // L), 256, 4096)[1]
                c.append(Case("up4k", "fir_up4k", dt, P, "up", L=L, opts={"fir_up4k": 2, "fir_up2k": 0}, N=4096, period=V4 * L))
        V4 = es.tile_overlap(256, 256, 4096)[1]
        c.append(Case("up4k_group2", "fir_up4k", dt, 1024, "up", L=4, opts={"fir_up4k": 2, "fir_up2k": 0, "fir_up4k_group": 2}, N=4096, period=V4 * 4))
    for L in (2, 3, 12):                                           # up2k_kernel
        V2 = es.tile_overlap(-(-516 // L), 64, 2048)[1]
        c.append(Case("up2k", "fir_up2k", np.complex64, 516, "up", L=L, opts={"fir_up4k": 2, "fir_up2k": 2}, N=2048, period=V2 * L))
    for dt in S:                                                   # dn4k_kernel
        for P in (512, 1024):
            for M in (2, 3, 4):
                Vd = es.tile_overlap((P - 1 + M - 1) // M + 1, 256, 4096)[1]
                c.append(Case("dn4k", "fir_dn4k", dt, P, "dn", M=M, opts={"fir_dn4k": 2}, N=4096, period=Vd))
    c.append(Case("updn_auto", None, np.complex64, 512, "updn", L=4, M=3))   # config 3
    for dt in (np.complex128, np.float64):                         # ols64_tile_kernel
        for P in (1024, 2049):
            ov6, V6 = es.tile_overlap(P, 256, 4096)
            c.append(Case("ols64", "fir_ols64", dt, P, "filter", force_ols=True, N=4096, overlap=ov6, period=V6))
            c.append(Case("ols64", "fir_ols64", dt, P, "dn", M=5, force_ols=True, N=4096, overlap=ov6, period=V6, step=5))
            Vu = es.tile_overlap(-(-P // 4), 256, 4096)[1]
            c.append(Case("ols64", "fir_ols64_up", dt, P, "up", L=4, opts={"fir_up_ols_min": -1}, N=4096, period=Vu * 4))
    return c


CASES = _cases()
DENSE = [c for c in CASES if not is_double(c.dt)]


def n_in(case):
    if case.what == "dn":
        return NOUT * case.M
    if case.what == "updn":
        return -(-NOUT * case.M // case.L)
    return NOUT


def taps_and_ref(case, kind, x):
    """(taps, reference); the impulse positions are printed."""
    L, M, F = case.L, case.M, case.F
    if kind == "impulse":
        b, d = es.impulse_taps(case.ntaps, F)
        print("impulse taps at", d.tolist())
        if case.what == "filter":
            return b, es.exact_filter(d, x)
        if case.what == "up":
            return b, es.exact_up(d, x, L)
        if case.what == "dn":
            return b, es.exact_dn(d, x, M)
        return b, es.exact_updn(d, x, L, M)
    b = es.chirp_taps(case.ntaps, F, is_complex(case.dt))
    threads = max(1, min(16, orc.max_threads()))
    u = L * orc.upsample(x, L) if L > 1 else x                      # oracle.fir_up / fir_dn, with the threads fir_filter takes
    y = orc.fir_filter(b, u, nthreads=threads)
    return b, (orc.downsample(y, M) if M > 1 else y)


def run_engine(case, b, x):
    """(y, path) of the one kernel call of a case."""
    k = _ffi.FirKernel(b, _ffi.code_of(np.dtype(case.dt)))
    if case.force_ols:
        k.set_algo(_ffi.FIR_OLS)
    n = len(x)
    count = n * case.L // case.M
    xd = _ffi.DeviceArray.from_host(np.ascontiguousarray(x))
    yd = _ffi.DeviceArray(count, case.dt)
    try:
        _ffi.debug_path()
        with contextlib.ExitStack() as st:
            for name, val in case.opts.items():
                st.enter_context(_ffi.option(name, val))
            if case.what == "filter":
                k.filter_dev(xd, yd)
            elif case.what == "up":
                k.up_dev(xd, yd, case.L)
            elif case.what == "dn":
                k.dn_dev(xd, yd, case.M)
            else:
                k.updn_dev(xd, yd, case.L, case.M)
        _ffi.sync()
        return yd.to_host(), _ffi.debug_path()
    except _ffi.SkdspError as err:   # a device error: nothing more is started on that card in this session
        pytest.exit("%s: %s" % (case.id(), err), returncode=3)
    finally:
        xd.free()
        yd.free()
        k._fin()


def fmt(m):
    return "R %.3g A %.3g (bin %d phase %d) B %s" % (m["R"], m["A"], m["bin"], m["phase"], "-" if m["B"] is None else "%.3g (position %d)" % (m["B"], m["pos"]))


def record(label, path, eng, yard):
    print("%s through %s: %s; yardstick: %s" % (label, path, fmt(eng), fmt(yard)))
    _REPORT.append({"case": label, "path": path, "engine": eng, "yardstick": yard})


def within_limits(label, eng, yard):
    assert eng["R"] <= R_FACTOR * yard["R"], (label, "R", eng, yard)
    assert eng["A"] <= A_FACTOR * yard["A"], (label, "A", eng, yard)
    for i, (a, ya) in enumerate(zip(eng["A_each"], yard["A_each"])):   # .up: all outputs and every phase against the yardstick's own
        assert a <= A_FACTOR * ya, (label, "A of %s" % ("all outputs" if i == 0 else "phase %d" % (i - 1)), a, eng["bin_each"][i], ya)
    if eng["B"] is not None:
        assert eng["B"] <= B_FACTOR * yard["B"], (label, "B", eng, yard)


def check(case, kind):
    x = es.noise(n_in(case), case.dt, SEED)
    b, ref = taps_and_ref(case, kind, x)
    y, path = run_engine(case, b, x)
    if case.engine is not None:
        assert path == [case.engine], (case.id(), path)
    cdt = np.complex128 if is_double(case.dt) else np.complex64
    L_meas = case.L if case.what == "up" else 1
    yy = es.yardstick(b, x, case.N, cdt, case.L, case.M, case.overlap)
    assert yy.shape == ref.shape == y.shape, (yy.shape, ref.shape, y.shape)
    yard = es.measure(yy, ref, L_meas, case.period, case.step)
    eng = es.measure(y, ref, L_meas, case.period, case.step)
    label = "%s %s" % (case.id(), kind)
    record(label, path, eng, yard)
    within_limits(label, eng, yard)


@pytest.mark.parametrize("case", CASES, ids=Case.id)
def test_impulse_taps(case):
    check(case, "impulse")


@pytest.mark.parametrize("case", DENSE, ids=Case.id)
def test_dense_taps(case):
    check(case, "chirp")


def test_bank_rows():
    """The raw bank entry (as tests/test_gpu_caf.py: test_raw_bank_row_stride_and_bad_arguments drives it): three rows of one complex64 signal."""
    P, period, shifts = 1024, 2000, [-3, 0, 5]
    g, d = es.impulse_taps(P, 3)
    print("impulse taps at", d.tolist())
    x = es.noise(NOUT, np.complex64, SEED)
    n = len(x)
    ov, V = es.tile_overlap(P, 256, 4096)
    bank = _ffi.FirBank(g, shifts, period, np.complex64)
    xd = _ffi.DeviceArray.from_host(np.ascontiguousarray(x))
    yd = _ffi.DeviceArray(3 * n, np.complex64)
    try:
        _ffi.debug_path()
        bank.filter_dev(xd, yd)
        _ffi.sync()
        path = _ffi.debug_path()
        y = yd.to_host().reshape(3, n)
    finally:
        xd.free()
        yd.free()
    assert path == ["fir_bank4k"], path
    worst = None
    for j, s in enumerate(shifts):
        bj = ss._caf_band_taps(g, s, period)
        ref = sum(bj[di] * es.exact_filter([di], x) for di in d.tolist())
        yard = es.measure(es.ols_host(bj, x, 4096, np.complex64, ov), ref, 1, V)
        eng = es.measure(y[j], ref, 1, V)
        label = "bank-complex64-row%d(shift %d)-%d impulse" % (j, s, P)
        record(label, path, eng, yard)
        worst = (label, eng, yard) if worst is None or eng["A"] / yard["A"] > worst[1]["A"] / worst[2]["A"] else worst
        within_limits(label, eng, yard)
    print("worst row:", worst[0])


@pytest.mark.parametrize("dt,engine,N,block,delta,old", [(np.complex64, "fir_ols", 8192, 512, 3e-6, 1e-6), (np.complex128, "fir_ols64", 4096, 256, 3e-15, 1e-10)],
                         ids=["complex64", "complex128"])
def test_positive_control(dt, engine, N, block, delta, old):
    """The unchanged kernel, taps whose spectrum is off by `delta` around one bin: inside today's contract, outside this one."""
    P, k0 = 1024, 1234
    ov, V = es.tile_overlap(P, block, N)
    case = Case("control", engine, dt, P, "filter", force_ols=True, N=N, overlap=ov, period=V)
    x = es.noise(NOUT, dt, SEED)
    b, d = es.impulse_taps(P, 1)
    ref = es.exact_filter(d, x)                                     # of the UNPERTURBED taps
    y, path = run_engine(case, b + es.tone_perturbation(P, k0, delta), x)
    assert path == [engine], path
    yard = es.measure(es.yardstick(b, x, N, np.complex128 if is_double(dt) else np.complex64, overlap=ov), ref, 1, V)
    eng = es.measure(y, ref, 1, V)
    e_old = es.peak_err(y, ref)
    record("control-%s delta %g at bin %d (max err / peak %.3g)" % (np.dtype(dt).name, delta, k0, e_old), path, eng, yard)
    assert e_old <= old, "the perturbed call is meant to pass today's contract"
    assert eng["A"] > A_FACTOR * yard["A"], (eng, yard)
    assert abs(eng["bin"] - k0) <= es.SEG // (2 * P), (eng["bin"], k0)
