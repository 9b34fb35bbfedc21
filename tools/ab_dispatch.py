"""Which engine does every branch of the host dispatch code pick, and what does it compute?  A fixed list of small seeded calls, one line each:
    name | engines (skdsp_debug_path) | sha256 of the output bytes | error against a float64 evaluation (relative to the output's peak)
Run it on two builds of the library (SKDSP_LIB=<another build>) and diff the lines: a change that only moves host code must leave every
line of a bit-stable call unchanged.  python tools/ab_dispatch.py"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
import numpy as np
from sk_dsp_comm_amd import _ffi
from oracle import oracle as orc

DT = {"f32": np.float32, "c64": np.complex64, "f64": np.float64, "c128": np.complex128}
rng = np.random.default_rng(12)


def noise(n, dt):
    dt = np.dtype(DT.get(dt, dt))
    if dt.kind == "c":
        return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(dt)
    return rng.standard_normal(n).astype(dt)


def lowpass(P, fc):
    t = np.arange(P) - (P - 1) / 2
    return np.hamming(P) * np.sinc(fc * t) * fc


def wide(x):
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


def fir_ref(b, x, L=1, M=1):
    xs = np.zeros(x.size * L, dtype=wide(x).dtype)
    xs[::L] = L * wide(x)
    y = np.convolve(xs, b)[:xs.size]
    return y[:(xs.size // M) * M:M] if M > 1 else y


def butter_sos(nsec, wc):
    """Butterworth low-pass of order 2 nsec, cutoff wc (of Nyquist), as biquads of unit DC gain (bilinear transform)."""
    N, W, sos = 2 * nsec, np.tan(np.pi * wc / 2), []
    for k in range(nsec):
        p = W * np.exp(1j * (np.pi * (2 * k + 1) / (2 * N) + np.pi / 2))
        z = (1 + p) / (1 - p)
        a1, a2 = -2 * z.real, abs(z) ** 2
        g = (1 + a1 + a2) / 4
        sos.append([g, 2 * g, g, 1.0, a1, a2])
    return np.array(sos)


def real_pole_sos(nsec):
    """Sections with two real poles and a positive impulse response: every l1 norm is a DC gain, so a float32 store between groups costs
    what it costs a Butterworth design at most -- such a cascade is grouped whatever its length."""
    sos = []
    for k in range(nsec):
        p1, p2 = 0.1 + 0.02 * k, 0.6 - 0.015 * k
        g = (1 - p1) * (1 - p2) / 4
        sos.append([g, 2 * g, g, 1.0, -(p1 + p2), p1 * p2])
    return np.array(sos)


def peak_then_notch(nsec):
    """nsec / 2 resonators, then the nsec / 2 FIR sections that cancel them: the whole cascade is the identity, its first half is not --
    a float32 store between groups would cost far more than the float32 contract allows."""
    half = nsec // 2
    return np.array([[1.0, 0, 0, 1.0, -0.5, 0.25]] * half + [[1.0, -0.5, 0.25, 1.0, 0, 0]] * half)


def line(name, y, ref=None, extra=b""):
    path = ",".join(_ffi.debug_path())
    y = np.ascontiguousarray(y)
    err = "-"
    if ref is not None:
        peak = float(np.max(np.abs(ref)))
        err = "%.3e" % (float(np.max(np.abs(wide(y.ravel()) - np.asarray(ref).ravel()))) / (peak if peak > 0 else 1.0))
    print("%s | %s | %s | %s" % (name, path, hashlib.sha256(y.tobytes() + extra).hexdigest(), err), flush=True)


def fir_cases():
    # .filter below and above the overlap-save crossovers (complex64 177 taps, float32 193, float64 128, complex128 24, complex taps 48)
    for dt, taps in (("c64", (96, 256)), ("f32", (96, 256)), ("f64", (64, 256)), ("c128", (16, 64))):
        x = noise(10000, dt)
        for P in taps:
            b = lowpass(P, 0.3)
            line("fir.filter %s %d taps" % (dt, P), _ffi.FirKernel(b, _ffi.code_of(x.dtype)).filter(x), fir_ref(b, x))
    x = noise(10000, "c64")
    for P in (32, 64):
        b = lowpass(P, 0.3) * np.exp(0.4j * np.arange(P))
        line("fir.filter c64 %d complex taps" % P, _ffi.FirKernel(b, _ffi.C64).filter(x), fir_ref(b, x))
    b = lowpass(256, 0.3)
    k = _ffi.FirKernel(b, _ffi.C64)
    k.set_algo(_ffi.FIR_DIRECT)
    line("fir.filter c64 256 taps forced direct", k.filter(x), fir_ref(b, x))
    # a call from rest over fewer samples than taps: a head of the filter
    b = lowpass(1024, 0.2)
    for dt in ("c64", "f32"):
        xs = noise(100, dt)
        line("fir.filter %s 1024 taps n = 100 (head)" % dt, _ffi.FirKernel(b, _ffi.code_of(xs.dtype)).filter(xs), fir_ref(b, xs))
    # more taps than one launch takes: tap segments
    for dt, P in (("f32", 5000), ("f64", 2100)):
        b = lowpass(P, 0.25)
        xs = noise(12000, dt)
        k = _ffi.FirKernel(b, _ffi.code_of(xs.dtype))
        line("fir.filter %s %d taps (segments)" % (dt, P), k.filter(xs), fir_ref(b, xs))
        line("fir.dn(3) %s %d taps (segments)" % (dt, P), k.dn(xs, 3), fir_ref(b, xs, 1, 3))
        line("fir.updn(3, 2) %s %d taps (segments)" % (dt, P), k.updn(xs, 3, 2), fir_ref(b, xs, 3, 2))
    # .dn: matrix-pipe / sliding-window kernels, decimating store, folded inverse, frequency-domain decimator
    for dt in ("c64", "f32", "f64"):
        x = noise(16384, dt)
        for P in (96, 1024) if dt != "f64" else (512,):
            b = lowpass(P, 0.05)
            k = _ffi.FirKernel(b, _ffi.code_of(x.dtype))
            for M in (2, 3, 4, 16):
                line("fir.dn(%d) %s %d taps" % (M, dt, P), k.dn(x, M), fir_ref(b, x, 1, M))
    b = lowpass(300, 0.05)
    x = noise(16384, "f64")
    line("fir.dn(5000) f64 300 taps", _ffi.FirKernel(b, _ffi.F64).dn(x, 5000), fir_ref(b, x, 1, 5000))
    xs = x.astype(np.float32)
    line("fir.dn(5000) f32 300 taps", _ffi.FirKernel(b, _ffi.F32).dn(xs, 5000), fir_ref(b, xs, 1, 5000))
    with _ffi.option("dn_no_ols", 1):   # (the last resort: full-rate filter and a strided copy)
        line("fir.dn(5000) f64 300 taps, dn_no_ols", _ffi.FirKernel(b, _ffi.F64).dn(x, 5000), fir_ref(b, x, 1, 5000))
        line("fir.dn(5000) f32 300 taps, dn_no_ols", _ffi.FirKernel(b, _ffi.F32).dn(xs, 5000), fir_ref(b, xs, 1, 5000))
    # .up: polyphase kernels, tile interpolators, the walk (pairs, rows), output tiles
    for dt in ("c64", "f32", "f64"):
        x = noise(8192, dt)
        for P in (96, 1024) if dt != "f64" else (1024,):
            b = lowpass(P, 0.05)
            k = _ffi.FirKernel(b, _ffi.code_of(x.dtype))
            for L in (2, 4, 7, 12):
                line("fir.up(%d) %s %d taps" % (L, dt, P), k.up(x, L), fir_ref(b, x, L, 1))
    for dt in ("c64", "f32", "f64"):
        x = noise(16384, dt)
        b = lowpass(1024, 0.1)
        k = _ffi.FirKernel(b, _ffi.code_of(x.dtype))
        for L, M in ((3, 2), (4, 3)):
            line("fir.updn(%d, %d) %s 1024 taps" % (L, M, dt), k.updn(x, L, M), fir_ref(b, x, L, M))
    # rows of one launch, host and device form
    for dt, rows, n, P in (("f32", 17, 100, 1024), ("c64", 5, 3000, 200)):
        b = lowpass(P, 0.2)
        x2 = noise(rows * n, dt).reshape(rows, n)
        k = _ffi.FirKernel(b, _ffi.code_of(x2.dtype))
        ref = np.stack([fir_ref(b, r) for r in x2])
        line("fir.filter_rows %s %d x %d, %d taps" % (dt, rows, n, P), k.filter_rows(x2), ref)
        line("fir.filter_rows wide %s %d x %d, %d taps" % (dt, rows, n, P), k.filter_rows(x2, wide=True), ref)
        xd, yd = _ffi.DeviceArray.from_host(x2.ravel()), _ffi.DeviceArray(rows * n, x2.dtype)
        k.filter_rows_dev(xd, yd, n, rows)
        line("fir.filter_rows_dev %s %d x %d, %d taps" % (dt, rows, n, P), yd.to_host(), ref)
        xd.free(); yd.free()


def iir_cases():
    x = {dt: noise(6000, dt) for dt in ("f32", "f64", "c64")}
    designs = [("butter %d sections" % ns, butter_sos(ns, 0.4)) for ns in (1, 8, 10, 12, 20)]
    # (the float32 handle of the 20-section Butterworth design takes its float64 twin: its group boundaries cost 190)
    designs += [("real poles 20 sections (groups)", real_pole_sos(20)),
                ("peak-then-notch 12 sections (one launch sequence)", peak_then_notch(12)),
                ("peak-then-notch 14 sections (float64 twin)", peak_then_notch(14))]
    for name, sos in designs:
        for dt in ("f32", "f64", "c64"):
            k = _ffi.IirKernel(_ffi.code_of(x[dt].dtype), sos=sos)
            line("iir.filter %s %s%s" % (dt, name, " sequential" if k.sequential else ""), k.filter(x[dt]), orc.sos_filter(sos, wide(x[dt])))
    sos = butter_sos(10, 0.4)
    with _ffi.option("iir_seq", 2):
        for dt in ("f32", "c64"):
            k = _ffi.IirKernel(_ffi.code_of(x[dt].dtype), sos=sos)
            line("iir.filter %s butter 10 sections, iir_seq = 2%s" % (dt, " sequential" if k.sequential else ""), k.filter(x[dt]),
                 orc.sos_filter(sos, wide(x[dt])))
    # a transfer function: factored into sections at creation
    sos = butter_sos(3, 0.3)
    b, a = np.ones(1), np.ones(1)
    for s in sos:
        b, a = np.convolve(b, s[:3]), np.convolve(a, s[3:])
    line("tf2sos butter order 6", _ffi.tf2sos(b, a))
    for dt in ("f32", "f64"):
        line("iir.filter %s tf_create butter order 6" % dt, _ffi.IirKernel(_ffi.code_of(x[dt].dtype), b=b, a=a).filter(x[dt]),
             orc.lfilter(b, a, wide(x[dt])))
    # .up, .dn, rows, streaming
    for ns in (4, 10):
        sos = butter_sos(ns, 0.2)
        for dt in ("f32", "c64", "f64"):
            k = _ffi.IirKernel(_ffi.code_of(x[dt].dtype), sos=sos)
            xs = x[dt][:3000]
            for L in (2, 3):
                line("iir.up(%d) %s butter %d sections" % (L, dt, ns), k.up(xs, L), orc.sos_up(sos, wide(xs), L))
            line("iir.dn(3) %s butter %d sections" % (dt, ns), k.dn(x[dt], 3), orc.sos_dn(sos, wide(x[dt]), 3))
            x2 = x[dt][:5 * 1200].reshape(5, 1200)
            ref = np.stack([orc.sos_filter(sos, wide(r)) for r in x2])
            line("iir.filter_rows %s 5 x 1200 butter %d sections" % (dt, ns), k.filter_rows(x2), ref)
            xd, yd = _ffi.DeviceArray.from_host(x2.ravel()), _ffi.DeviceArray(x2.size, x2.dtype)
            k.filter_rows_dev(xd, yd, 1200, 5)
            line("iir.filter_rows_dev %s 5 x 1200 butter %d sections" % (dt, ns), yd.to_host(), ref)
            xd.free(); yd.free()
            y1, z1 = k.filter_state(xs[:1700])
            y2, z2 = k.filter_state(xs[1700:], z1)
            line("iir.filter_state %s two blocks, butter %d sections" % (dt, ns), np.concatenate([y1, y2]), orc.sos_filter(sos, wide(xs)),
                 z1.tobytes() + z2.tobytes())


def resonator_sos(radius=0.997, angle=0.6):
    """One section whose pole pair decays so slowly that a float32 wave segment (8192 or 6144 samples) is not the whole memory: the look-back
    depth K of the parallel form is 2 (128-sample chunks) and 3 (96-sample chunks) for float32, 4 and none for complex64, 6 for float64, none for
    complex128 (tests/host/iir_par_plan_emul.cpp prints them)."""
    return np.array([[1.0, 0.0, 0.0, 1.0, -2 * radius * np.cos(angle), radius ** 2]])


def par_cases():
    """Every row of par_choose (csrc/iir_par_plan.hpp): designs x dtypes x operations at the defaults, then every option that changes the
    decision, for the operations it affects.  25200 samples at the rate of the longer side: divisible by every factor, three 8192-sample and
    four 6144-sample float32 wave segments plus a ragged tail -- look-back, ticket order and tail staging all run."""
    prng = np.random.default_rng(13)
    n, dts = 25200, ("f32", "c64", "f64", "c128")

    def pnoise(m, dt):
        dt = np.dtype(DT[dt])
        if dt.kind == "c":
            return ((prng.standard_normal(m) + 1j * prng.standard_normal(m)) / np.sqrt(2)).astype(dt)
        return prng.standard_normal(m).astype(dt)

    x = {dt: pnoise(3 * n, dt) for dt in dts}
    sos8 = np.load(os.path.join(ROOT, "tests", "golden", "g7_iir_sos.npz"))["sos8"]
    designs = [("butter %d" % ns, butter_sos(ns, 0.2)) for ns in (2, 5, 8)] + [("g7 sos8", sos8), ("resonator 0.997", resonator_sos())]
    DN, UP = (2, 3, 4, 5, 12), (2, 3, 4, 5, 8, 10, 12)
    refs = {}

    def ref(key, fn):
        if key not in refs:
            refs[key] = fn()
        return refs[key]

    def run(tag, dname, sos, dt, ops, m=n):
        k = _ffi.IirKernel(_ffi.code_of(x[dt].dtype), sos=sos)
        xs = x[dt][:m]
        for op, f in ops:
            name = "par%s %s %s %s%s" % (tag, dname, dt, op if f is None else "%s(%d)" % (op, f), "" if m == n else " n = %d" % m)
            if op == "filter":
                line(name, k.filter(xs), ref((dname, dt, op, m), lambda: orc.sos_filter(sos, wide(xs))))
            elif op == "dn":
                line(name, k.dn(xs, f), ref((dname, dt, op, f, m), lambda: orc.sos_dn(sos, wide(xs), f)))
            elif op == "up":
                xi = xs[:m // f]
                line(name, k.up(xi, f), ref((dname, dt, op, f, m), lambda: orc.sos_up(sos, wide(xi), f)))
            else:
                x2 = x[dt].reshape(3, n)
                line(name, k.filter_rows(x2), ref((dname, dt, op), lambda: np.stack([orc.sos_filter(sos, wide(r)) for r in x2])))

    dn_ops, up_ops = [("dn", M) for M in DN], [("up", L) for L in UP]
    every = [("filter", None)] + dn_ops + up_ops + [("rows", None)]
    for dname, sos in designs:
        for dt in dts:
            run("", dname, sos, dt, every)
    four = ("f32", "c64")
    sweeps = [("iir_par_v32", (0, 2), four, [("filter", None)] + dn_ops + [("up", L) for L in (2, 3, 4, 5)] + [("rows", None)], 7),
              ("iir_dn_t96", (0, 2, 3), four, dn_ops, 1), ("iir_up_jump", (0,), dts, [("up", 8), ("up", 12)], 1),
              ("iir_up_lean", (0,), dts, [("up", 2), ("up", 3), ("up", 4)], 1), ("iir_dn_compact", (0,), dts, dn_ops, 1)]
    for option, values, types, ops, min_sections in sweeps:
        for v in values:
            with _ffi.option(option, v):
                for dname, sos in designs:
                    if len(sos) >= min_sections:
                        for dt in types:
                            run(" %s = %d" % (option, v), dname, sos, dt, ops)
    for dt in dts:   # less than one wave segment
        run("", "g7 sos8", sos8, dt, [("filter", None), ("dn", 2), ("dn", 3), ("up", 3), ("up", 12)], 5040)


def one_call_cases():
    for dt in ("f32", "c64"):
        x = noise(5000, dt)
        line("upsample(3) %s" % dt, _ffi.upsample(x, 3))
        line("downsample(4, 1) %s" % dt, _ffi.downsample(x, 4, 1))
        line("farrow order 3 %s" % dt, _ffi.farrow(x, 1.0, 0.7, 3))
        line("psd_accum %s" % dt, _ffi.psd_accum(x, np.hanning(256), 256, 128, 38))
    x = noise(4096, "c64")
    bank = _ffi.FirBank(lowpass(300, 0.1), np.arange(-3, 4), 1000, np.complex64)
    xd, yd = _ffi.DeviceArray.from_host(x), _ffi.DeviceArray(7 * 4096, np.complex64)
    bank.filter_dev(xd, yd)
    line("fir_bank 7 bands, 300 taps", yd.to_host())
    xd.free(); yd.free()


def host_pipeline_cases():
    # vectors of several chunks: the chunk pipeline, then the same on two slots bound to the one GPU
    _ffi.set_option("host_chunk_log2", 10)
    b = lowpass(256, 0.2)
    sos = butter_sos(4, 0.3)
    jobs = []
    for dt in ("c64", "f32"):
        x = noise(5003, dt)
        jobs.append((dt, x, _ffi.FirKernel(b, _ffi.code_of(x.dtype)), _ffi.IirKernel(_ffi.code_of(x.dtype), sos=sos)))

    def calls(tag, ngpus):
        for dt, x, k, i in jobs:
            line("pipeline%s fir.filter %s" % (tag, dt), k.filter(x), fir_ref(b, x))
            line("pipeline%s fir.filter wide %s" % (tag, dt), k.filter(x, wide=True), fir_ref(b, x))
            line("pipeline%s fir.up(2) %s" % (tag, dt), k.up(x, 2), fir_ref(b, x, 2, 1))
            line("pipeline%s fir.dn(3) %s" % (tag, dt), k.dn(x, 3), fir_ref(b, x, 1, 3))
            line("pipeline%s fir.updn(3, 2) wide %s" % (tag, dt), k.updn(x, 3, 2, wide=True), fir_ref(b, x, 3, 2))
            for ng in ngpus:
                line("pipeline%s fir.filter_sharded ngpu = %d %s" % (tag, ng, dt), k.filter_sharded(x, ng), fir_ref(b, x))
            line("pipeline%s iir.filter %s" % (tag, dt), i.filter(x), orc.sos_filter(sos, wide(x)))
            line("pipeline%s iir.filter wide %s" % (tag, dt), i.filter(x, wide=True), orc.sos_filter(sos, wide(x)))

    calls("", (0, 1))
    assert _ffi.init_devices([0, 0]) == 2
    calls(" two slots", (0, 1, 2))


_ffi.init(0)
_ffi.debug_path()
fir_cases()
iir_cases()
par_cases()
one_call_cases()
host_pipeline_cases()
print("lib", os.path.basename(os.environ.get("SKDSP_LIB", "in-tree")), flush=True)
