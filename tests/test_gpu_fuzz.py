"""Randomised differential test of the reference surface (multirate_FIR / multirate_IIR / rate_change .filter/.up/.dn, upsample, downsample)
against scipy.signal on the host: random dtypes, lengths (around tile / segment / chunk boundaries), factors, tap counts and designs,
fixed seeds.  Complements the structured parity tests: its job is the combination nobody thought of."""
import os

import numpy as np
import pytest
from scipy import signal

from sk_dsp_comm_amd import _ffi, multirate_helper as mrh, sigsys as ss
from conftest import rel_err
from _pads import loud as _loud

pytestmark = pytest.mark.gpu

NSEED = int(os.environ.get("SKDSP_FUZZ_SEEDS", "12"))   # (more seeds for a one-off hunt: SKDSP_FUZZ_SEEDS=200)
LENGTHS = [1, 2, 3, 7, 63, 64, 65, 127, 128, 129, 255, 257, 1023, 1024, 1025, 4095, 4097, 7168, 7169, 7170, 8191, 8192, 8193,
           16384 + 5, 3 * 8192 - 1, 65536 + 17, 250_003]
DTYPES = [np.float32, np.complex64, np.float64, np.complex128]


def _signal(rng, n, dt):
    x = rng.standard_normal(n)
    if np.dtype(dt).kind == "c":
        x = x + 1j * rng.standard_normal(n)
    return x.astype(dt)


def _tol(dt, ref, gain=1.0):
    single = np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 4
    return (1e-6 if single else 1e-10) * gain


def _log_close_call(what, err, scale, spread):
    try:
        root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
        os.makedirs(root, exist_ok=True)
        with open(os.path.join(root, "fuzz_close_calls.txt"), "a") as f:
            f.write("%s: err / scale %.3g (err %.3g, scale %.3g, reference spread %.3g)\n" % (what, err / scale, err, scale, spread))
    except OSError:
        pass


def _check(y, ref, dt, what, bound, ref_spread=0.0):
    """1e-6 (1e-10) of the output's peak (north_star's bound, no slack factor) -- or, for outputs far below the input (stop bands, start-up),
    of 1 % of the forward bound.
    ref_spread: how far two float64 evaluations of the reference itself lie apart (sections in another order): a cascade whose
    float64 result is only good to 1e-6 (a 40th-order Chebyshev) cannot be matched closer than that by anybody.  The scans, which combine
    chunk transitions instead of running the recursion sample by sample, would lose 30 - 400 x that spread on such cascades; the library
    therefore probes every cascade of more than 8 sections at creation and runs the ill-conditioned ones through the reference's own
    recursion (csrc/iir_seq.hip).  What is left for the factor is the cascades just below the probe's threshold."""
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    if ref.size == 0:
        return
    scale = max(float(np.max(np.abs(ref))), 1e-2 * bound)
    err = float(np.max(np.abs(y - ref)))
    single = np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 4
    if err > (7e-7 if single else 7e-11) * scale:   # every case in the upper third of the contract is put on record (merged back by gpurun)
        _log_close_call(what, err, scale, ref_spread)
    assert err <= _tol(dt, ref) * scale + 30.0 * ref_spread, "%s: err %.3g, scale %.3g, reference spread %.3g" % (what, err, scale, ref_spread)


@pytest.mark.parametrize("seed", range(NSEED))
def test_fuzz_fir(seed):
    rng = np.random.default_rng(1000 + seed)
    for _ in range(14):
        dt = DTYPES[rng.integers(len(DTYPES))]
        n = int(LENGTHS[rng.integers(len(LENGTHS))])
        ntaps = int(rng.choice([1, 2, 5, 31, 64, 127, 128, 200, 511, 512, 1024, 1500, 4097]))
        b = signal.firwin(ntaps, float(rng.uniform(0.05, 0.8))) if ntaps > 1 else np.array([float(rng.uniform(0.5, 2.0))])
        if rng.random() < 0.2:
            b = rng.standard_normal(ntaps) / np.sqrt(ntaps)
        op = rng.choice(["filter", "up", "dn"])
        f = int(rng.choice([1, 2, 3, 4, 5, 12, 17]))
        x = _signal(rng, n, dt)
        xw = x.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)
        fir = mrh.multirate_FIR(b)
        bound = float(np.sum(np.abs(b)) * np.max(np.abs(x)))
        what = "%s %s n=%d taps=%d f=%d" % (op, np.dtype(dt).name, n, ntaps, f)
        if op == "filter":
            _check(fir.filter(x), signal.lfilter(b, [1], xw), dt, what, bound)
        elif op == "up":
            if n * f > 3_000_000:
                continue
            up = np.zeros(n * f, dtype=xw.dtype)
            up[::f] = f * xw
            _check(fir.up(x, f), signal.lfilter(b, [1], up), dt, what, bound * f)
        else:
            _check(np.asarray(fir.dn(x, f)), signal.lfilter(b, [1], xw)[::f][:n // f], dt, what, bound)


@pytest.mark.parametrize("seed", range(NSEED))
def test_fuzz_iir(seed):
    rng = np.random.default_rng(2000 + seed)
    for _ in range(14):
        dt = DTYPES[rng.integers(len(DTYPES))]
        n = int(LENGTHS[rng.integers(len(LENGTHS))])
        order = int(rng.choice([1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 17, 18, 20, 24, 30, 40]))   # (more than 8 biquads: consecutive groups)
        kind = rng.choice(["butter", "cheby1", "ellip"])
        wn = float(rng.uniform(0.03, 0.6))
        if kind == "butter":
            sos = signal.butter(order, wn, output="sos")
        elif kind == "cheby1":
            sos = signal.cheby1(order, 0.5, wn, output="sos")
        else:
            sos = signal.ellip(min(order, 8), 0.5, 60, wn, output="sos")
        op = rng.choice(["filter", "up", "dn"])
        f = int(rng.choice([1, 2, 3, 4, 5, 6, 8, 12, 16, 17, 24, 48, 96]))   # (the divisors of 96 have kernels of their own: state jump / wave-uniform kept samples)
        x = _signal(rng, n, dt)
        xw = x.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)
        iir = mrh.multirate_IIR(sos)
        # forward bound of the cascade: the l1 norm of its impulse response (numerically) x max|x|
        h = signal.sosfilt(sos, np.r_[1.0, np.zeros(4095)])
        bound = float(np.sum(np.abs(h)) * np.max(np.abs(x)))
        what = "%s %s n=%d %s(%d, %.3f) f=%d" % (op, np.dtype(dt).name, n, kind, order, wn, f)
        def both(v):   # the reference, and the same cascade with its sections in reverse order (equal in exact arithmetic)
            r = signal.sosfilt(sos, v)
            return r, float(np.max(np.abs(r - signal.sosfilt(np.ascontiguousarray(sos[::-1]), v)))) if len(sos) > 8 else 0.0
        if op == "filter":
            ref, spread = both(xw)
            _check(iir.filter(x), ref, dt, what, bound, spread)
        elif op == "up":
            if n * f > 3_000_000:
                continue
            up = np.zeros(n * f, dtype=xw.dtype)
            up[::f] = f * xw
            ref, spread = both(up)
            _check(iir.up(x, f), ref, dt, what, bound * f, spread)
        else:
            ref, spread = both(xw)
            _check(np.asarray(iir.dn(x, f)), ref[::f][:n // f], dt, what, bound, spread)


@pytest.mark.parametrize("seed", range(max(NSEED // 3, 1)))
def test_fuzz_rate_change_and_resamplers(seed):
    rng = np.random.default_rng(3000 + seed)
    for _ in range(10):
        dt = DTYPES[rng.integers(len(DTYPES))]
        n = int(LENGTHS[rng.integers(len(LENGTHS))])
        M = int(rng.choice([2, 3, 4, 6, 12]))
        x = _signal(rng, n, dt)
        xw = x.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)
        fc, order, ftype = float(rng.choice([0.9, 0.7, 0.5])), int(rng.choice([1, 2, 3, 4, 6, 8, 10, 12])), str(rng.choice(["butter", "cheby1"]))
        rc = mrh.rate_change(M, fc, order, ftype)
        # The reference evaluates the TRANSFER FUNCTION (b, a) as one transposed section of order N in float64 (multirate_helper.py:74, 81);
        # for narrow designs that form is ill-conditioned (order 12 at 0.9 / 12: coefficients of alternating sign up to 1e3, results good to
        # ~1e-3).  The same design as second-order sections shows how far the reference itself is from the filter it means:
        sos_true = signal.butter(order, fc / M, output="sos") if ftype == "butter" else signal.cheby1(order, 0.05, fc / M, output="sos")
        h = signal.lfilter(rc.b, rc.a, np.r_[1.0, np.zeros(8191)])
        bound = float(np.sum(np.abs(h)) * np.max(np.abs(x)))
        single = np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 4
        if n * M <= 3_000_000:
            up = np.zeros(n * M, dtype=xw.dtype)
            up[::M] = M * xw
            ref = signal.lfilter(rc.b, rc.a, up)
            spread = float(np.max(np.abs(ref - signal.sosfilt(sos_true, up))))
            y = rc.up(x)
            assert np.max(np.abs(y - ref)) <= (1e-6 if single else 1e-7) * max(np.max(np.abs(ref)), 1e-2 * bound * M) + 3.0 * spread, \
                ("rc.up", np.dtype(dt).name, n, M, order, ftype, spread)
        full = signal.lfilter(rc.b, rc.a, xw)
        spread = float(np.max(np.abs(full - signal.sosfilt(sos_true, xw)))) if n else 0.0
        ref = full[::M][:n // M]
        y = np.asarray(rc.dn(x))
        assert y.shape == ref.shape
        if ref.size:
            assert np.max(np.abs(y - ref)) <= (1e-6 if single else 1e-7) * max(np.max(np.abs(ref)), 1e-2 * bound) + 3.0 * spread, \
                ("rc.dn", np.dtype(dt).name, n, M, order, ftype, spread)
        L = int(rng.choice([1, 2, 3, 7]))
        u = ss.upsample(x, L)
        ru = np.zeros(n * L, dtype=u.dtype)
        ru[::L] = x
        assert np.array_equal(u, ru)
        p = int(rng.integers(0, M))
        if n >= M:
            assert np.array_equal(np.asarray(ss.downsample(x, M, p)), x[p::M][:n // M])


@pytest.mark.parametrize("seed", range(max(NSEED // 2, 1)))
def test_fuzz_nd_and_streaming(seed):
    """N-D arrays filter along the last axis in one call (lfilter / sosfilt semantics); a signal cut at random points and run through
    filter_stream block by block reproduces the one-shot result."""
    rng = np.random.default_rng(4000 + seed)
    for _ in range(6):
        dt = DTYPES[rng.integers(len(DTYPES))]
        single = np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 4
        wide = np.complex128 if np.dtype(dt).kind == "c" else np.float64
        # ---- N-D
        shape = tuple(int(v) for v in rng.choice([1, 2, 3, 5, 17], size=int(rng.integers(1, 3)))) + (int(rng.choice([1, 5, 100, 4099, 8192, 20_001])),)
        x = _signal(rng, int(np.prod(shape)), dt).reshape(shape)
        ntaps = int(rng.choice([3, 64, 127, 300, 1024]))
        b = signal.firwin(ntaps, 0.3)
        sos = signal.butter(int(rng.choice([2, 5, 8, 18, 22, 34])), float(rng.uniform(0.05, 0.5)), output="sos")
        for name, y, ref, bound in (("fir", mrh.multirate_FIR(b).filter(x), signal.lfilter(b, [1], x.astype(wide)), np.sum(np.abs(b))),
                                    ("iir", mrh.multirate_IIR(sos).filter(x), signal.sosfilt(sos, x.astype(wide)),
                                     np.sum(np.abs(signal.sosfilt(sos, np.r_[1.0, np.zeros(4095)]))))):
            _check(y, ref, dt, "%s N-D %s %s" % (name, shape, np.dtype(dt).name), float(bound * np.max(np.abs(x))))
        # ---- streaming
        n = int(rng.choice([10, 1000, 9000, 70_001]))
        x = _signal(rng, n, dt)
        cuts = sorted(set(int(c) for c in rng.integers(0, n + 1, size=int(rng.integers(1, 5)))) | {0, n})
        fir, iir = mrh.multirate_FIR(b), mrh.multirate_IIR(sos)
        yf, yi, zf, zi = [], [], None, None
        for a0, a1 in zip(cuts[:-1], cuts[1:]):
            blk = x[a0:a1]
            if blk.size == 0:
                continue
            o, zf = fir.filter_stream(blk, zi=zf)
            yf.append(o)
            o, zi = iir.filter_stream(blk, zi=zi)
            yi.append(o)
        tol = 2e-6 if single else 1e-10
        for name, got, ref in (("fir", np.concatenate(yf), signal.lfilter(b, [1], x.astype(wide))), ("iir", np.concatenate(yi), signal.sosfilt(sos, x.astype(wide)))):
            assert got.shape == ref.shape
            assert np.max(np.abs(got - ref)) <= tol * max(np.max(np.abs(ref)), 1e-2 * np.max(np.abs(x))), ("%s stream" % name, np.dtype(dt).name, n, cuts)


@pytest.mark.parametrize("seed", range(max(NSEED // 2, 1)))
def test_fuzz_device_views_at_odd_offsets(seed):
    """The *_dev entry points on windows of larger device buffers: element-aligned but not 16-byte-aligned inputs and outputs (the vector
    load / store fast paths must step aside), guard words on both sides of every output must survive, and the loud samples on both sides
    of the input must not show in the result."""
    rng = np.random.default_rng(5000 + seed)
    for _ in range(8):
        dt = DTYPES[rng.integers(len(DTYPES))]
        cplx = np.dtype(dt).kind == "c"
        single = np.dtype(dt).itemsize // (2 if cplx else 1) == 4
        wide = np.complex128 if cplx else np.float64
        n = int(rng.choice([1, 5, 129, 4100, 8192, 8192 * 3 + 7, 70_003]))
        op = str(rng.choice(["filter", "up", "dn"]))
        f = 1 if op == "filter" else int(rng.choice([2, 3, 4, 5, 12]))
        n_out = n if op == "filter" else (n * f if op == "up" else n // f)
        if n_out == 0 or n_out > 2_000_000:
            continue
        ox, oy = int(rng.integers(0, 9)), int(rng.integers(1, 9))
        x = _signal(rng, n, dt)
        xbuf = _ffi.DeviceArray(n + 16, dt)
        ybuf = _ffi.DeviceArray(n_out + 32, dt)
        try:
            xbuf.write(np.concatenate([_loud(ox, dt), x, _loud(16 - ox, dt, ox)]))
            ybuf.write(np.full(n_out + 32, 7.0, dtype=dt))
            xv, yv = xbuf.window(ox, n), ybuf.window(oy, n_out)
            if rng.random() < 0.5:
                ntaps = int(rng.choice([5, 127, 300, 1024]))
                b = signal.firwin(ntaps, 0.25)
                k = _ffi.FirKernel(b, _ffi.code_of(dt))
                full = signal.lfilter(b, [1], x.astype(wide)) if op != "up" else None
                bound = np.sum(np.abs(b))
                name = "fir %d taps" % ntaps
                lf = lambda v: signal.lfilter(b, [1], v)
            else:
                sos = signal.butter(int(rng.choice([2, 5, 8])), float(rng.uniform(0.05, 0.5)), output="sos")
                k = _ffi.IirKernel(_ffi.code_of(dt), sos=sos)
                bound = np.sum(np.abs(signal.sosfilt(sos, np.r_[1.0, np.zeros(4095)])))
                name = "iir %d sections" % len(sos)
                lf = lambda v: signal.sosfilt(sos, v)
            # (half of the FIR cases force the frequency-domain interpolator / decimator where they apply: fir_up4k / fir_up2k / fir_dn4k)
            forced = int(rng.choice([1, 2]))
            import contextlib
            st = contextlib.ExitStack()
            st.enter_context(_ffi.option("fir_up4k", forced))
            st.enter_context(_ffi.option("fir_dn4k", forced))
            if forced == 2:
                st.enter_context(_ffi.option("fir_up_ols_min", -2))
            if op == "filter":
                k.filter_dev(xv, yv)
                ref = lf(x.astype(wide))
            elif op == "up":
                k.up_dev(xv, yv, f)
                up = np.zeros(n * f, dtype=wide)
                up[::f] = f * x.astype(wide)
                ref = lf(up)
                bound = bound * f
            else:
                k.dn_dev(xv, yv, f)
                ref = lf(x.astype(wide))[::f][:n_out]
            st.close()
            got = ybuf.to_host()
            what = "%s %s %s n=%d f=%d offsets %d/%d" % (name, op, np.dtype(dt).name, n, f, ox, oy)
            assert np.all(got[:oy] == 7.0) and np.all(got[oy + n_out:] == 7.0), "guard words overwritten: " + what
            _check(got[oy:oy + n_out], ref, dt, what, float(bound * np.max(np.abs(x))))
        finally:
            xbuf.free()
            ybuf.free()


@pytest.mark.parametrize("seed", range(NSEED))
def test_fuzz_fir_up_walk_forms(seed):
    """multirate_FIR.up and L / M in the frequency domain, forced (option fir_up_ols_min < 0) so that short phases and short signals take it too:
    the walk over (tile, phase) pairs in every form it has -- strided stores, rows + weave, phases in pairs for real signals (even and odd L),
    the every-M-th store -- and (M = 1) the one-workgroup-per-input-tile interpolators fir_up4k / fir_up2k in theirs, on device windows at
    random element offsets (aligned and not), guard words around the output, history in front of the input, loud samples in front of
    the history and behind the window."""
    import contextlib
    rng = np.random.default_rng(7000 + seed)
    for _ in range(10):
        dt = DTYPES[rng.integers(len(DTYPES))]
        cplx = np.dtype(dt).kind == "c"
        wide = np.complex128 if cplx else np.float64
        L = int(rng.choice([2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 33]))
        M = int(rng.choice([1, 1, 1, 2, 3, 5, 7]))
        ntaps = int(rng.integers(2 * L, 40 * L + 1)) if rng.random() < 0.7 else int(rng.choice([1024, 2500, 4097]))
        n = int(rng.choice([8192, 8193, 12_000, 16384 + 5, 3 * 8192 - 1, 40_001]))
        b = signal.firwin(ntaps, 0.9 / max(L, M))
        if cplx and rng.random() < 0.3:
            b = b * np.exp(0.05j * np.arange(ntaps))
        hist = int(rng.choice([0, 0, (ntaps - 1 + L - 1) // L]))
        ox, oy = int(rng.integers(0, 5)), int(rng.integers(0, 5))
        n_out = (n * L) // M
        x = _signal(rng, n + hist, dt)
        xbuf = _ffi.DeviceArray(n + hist + 8, dt)
        ybuf = _ffi.DeviceArray(n_out + 16, dt)
        try:
            xbuf.write(np.concatenate([_loud(ox, dt), x, _loud(8 - ox, dt, ox)]))
            ybuf.write(np.full(n_out + 16, 7.0, dtype=dt))
            k = _ffi.FirKernel(b, _ffi.code_of(dt))
            with contextlib.ExitStack() as st:
                st.enter_context(_ffi.option("fir_up_ols_min", -2))
                # M = 1: the walk (fir_up4k = 0) or the one-workgroup-per-input-tile interpolators in every form they have (four / two phases
                # per store of the 4096-point tile; the 2048-point tile with all phases per thread from five passes on, or always; rows
                # through the staging image or each lane its own)
                tile = int(rng.choice([0, 2, 2]))
                st.enter_context(_ffi.option("fir_up4k", tile))
                st.enter_context(_ffi.option("fir_up2k", int(rng.choice([1, 2]))))
                st.enter_context(_ffi.option("fir_up4k_group", int(rng.choice([2, 4]))))
                st.enter_context(_ffi.option("fir_up4k_staged", int(rng.integers(0, 2))))
                st.enter_context(_ffi.option("fir_up_rows_min", int(rng.choice([-1, 0, 2]))))
                st.enter_context(_ffi.option("fir_up_pair", int(rng.integers(0, 2))))
                st.enter_context(_ffi.option("fir_updn_fused", int(rng.integers(0, 2))))
                k.updn_dev(xbuf.window(ox + hist, n), ybuf.window(oy, n_out), L, M, n_hist=hist)
            up = np.zeros((n + hist) * L, dtype=np.complex128 if np.iscomplexobj(b) else wide)
            up[::L] = L * x.astype(up.dtype)
            ref = signal.lfilter(b, [1], up)[hist * L:][::M][:n_out]
            got = ybuf.to_host()
            what = "%s %s L/M=%d/%d taps=%d n=%d hist=%d offsets %d/%d" % ("tile" if tile and M == 1 else "walk", np.dtype(dt).name, L, M, ntaps, n, hist, ox, oy)
            assert np.all(got[:oy] == 7.0) and np.all(got[oy + n_out:] == 7.0), "guard words overwritten: " + what
            _check(got[oy:oy + n_out], ref, dt, what, float(np.sum(np.abs(b)) * L * np.max(np.abs(x))))
        finally:
            xbuf.free()
            ybuf.free()


@pytest.mark.parametrize("seed", range(max(NSEED // 2, 1)))
def test_fuzz_fir_wide(seed):
    """The FIR corners the first FIR fuzz leaves out: complex taps, tap counts beyond one launch (tap segments), the fused L / M resampler,
    the transform-domain wrappers os_filter / oa_filter (sigsys.py:482-598), the three-stage interp24 / deci24 chains (sigsys.py:2945-3028)."""
    rng = np.random.default_rng(6000 + seed)
    for _ in range(6):
        dt = DTYPES[rng.integers(len(DTYPES))]
        cplx = np.dtype(dt).kind == "c"
        wide = np.complex128 if cplx else np.float64
        n = int(LENGTHS[rng.integers(len(LENGTHS))])
        x = _signal(rng, n, dt)
        xw = x.astype(wide)
        # complex taps / very long filters
        ntaps = int(rng.choice([7, 90, 700, 4097, 6000, 9001]))
        b = rng.standard_normal(ntaps) / np.sqrt(ntaps)
        if rng.random() < 0.5:
            b = b + 1j * rng.standard_normal(ntaps) / np.sqrt(ntaps)
        bound = float(np.sum(np.abs(b)) * np.max(np.abs(x)))
        ref = signal.lfilter(b, [1], xw.astype(np.complex128) if np.iscomplexobj(b) else xw)
        y = mrh.multirate_FIR(b).filter(x)
        _check(np.asarray(y), ref, dt, "filter %s n=%d taps=%d complex taps %s" % (np.dtype(dt).name, n, ntaps, np.iscomplexobj(b)), bound)
        # fused L / M through the C entry (downsample(up(x, L), M))
        L, M = int(rng.choice([2, 3, 4, 5, 7])), int(rng.choice([2, 3, 5, 9]))
        bt = signal.firwin(int(rng.choice([32, 129, 512, 2048, 5000])), 0.9 / max(L, M))   # (long ones: the overlap-save walk with the every-M-th store)
        if n * L <= 3_000_000 and (n * L) // M > 0:
            up = np.zeros(n * L, dtype=wide)
            up[::L] = L * xw
            ref = signal.lfilter(bt, [1], up)[::M][:(n * L) // M]
            y = _ffi.FirKernel(bt, _ffi.code_of(dt)).updn(x, L, M)
            _check(y, ref, dt, "updn %s n=%d %d/%d" % (np.dtype(dt).name, n, L, M), float(np.sum(np.abs(bt)) * L * np.max(np.abs(x))))
        # os_filter / oa_filter: both return real(lfilter(h, 1, x)) (the reference pads P-1 zeros in front for overlap-save and slices them off)
        if not cplx:
            P = int(rng.choice([8, 33, 100]))
            h = signal.firwin(P, 0.3)
            N = int(rng.choice([128, 256, 1024]))
            if n > P:
                refw = signal.lfilter(h, [1], xw)
                single = np.dtype(dt).itemsize == 4
                for name, fn in (("os", ss.os_filter), ("oa", ss.oa_filter)):
                    y = np.asarray(fn(x, h, N))
                    assert y.shape == refw.shape and np.max(np.abs(y - refw)) <= (2e-6 if single else 1e-10) * max(np.max(np.abs(refw)), 1e-2 * np.max(np.abs(x))), (name, n, P, N)
        # interp24 / deci24 on short real signals
        if not cplx and n <= 4097:
            xs = xw[:min(n, 700)]
            y = ss.interp24(xs.astype(dt))
            r = xs
            for Lk in (2, 3, 4):
                bb, aa = signal.butter(10, 1.0 / Lk)
                u = np.zeros(len(r) * Lk)
                u[::Lk] = Lk * r
                r = signal.lfilter(bb, aa, u)
            single = np.dtype(dt).itemsize == 4
            assert np.max(np.abs(y - r)) <= (3e-6 if single else 1e-7) * max(np.max(np.abs(r)), 1e-3), ("interp24", len(xs))


@pytest.mark.parametrize("seed", range(max(NSEED // 2, 1)))
def test_fuzz_host_chunk_pipeline(seed):
    """Host-array calls on vectors cut into small chunks (option host_chunk_log2 = 10 .. 14): every chunk is staged with the history it
    needs (FIR: Ntaps-1 samples, whole output periods for L / M; IIR: the section states from the chunk before) -- the results must not
    depend on where the cuts fall."""
    rng = np.random.default_rng(7000 + seed)
    for _ in range(5):
        dt = DTYPES[rng.integers(len(DTYPES))]
        cplx = np.dtype(dt).kind == "c"
        wide = np.complex128 if cplx else np.float64
        lg = int(rng.integers(10, 15))
        n = int(rng.integers(1, 40)) * (1 << lg) // 8 + int(rng.integers(0, 50))
        x = _signal(rng, n, dt)
        xw = x.astype(wide)
        ntaps = int(rng.choice([3, 64, 200, 1024, 1500]))
        b = signal.firwin(ntaps, 0.3)
        sos = signal.butter(int(rng.choice([2, 5, 8, 11])), float(rng.uniform(0.05, 0.5)), output="sos")
        f = int(rng.choice([2, 3, 4, 5, 12]))
        hb = float(np.sum(np.abs(b)) * np.max(np.abs(x)))
        hs = float(np.sum(np.abs(signal.sosfilt(sos, np.r_[1.0, np.zeros(4095)]))) * np.max(np.abs(x)))
        with _ffi.option("host_chunk_log2", lg):
            fir, iir = mrh.multirate_FIR(b), mrh.multirate_IIR(sos)
            tag = "%s n=%d chunk 2^%d taps=%d f=%d" % (np.dtype(dt).name, n, lg, ntaps, f)
            _check(fir.filter(x), signal.lfilter(b, [1], xw), dt, "fir.filter " + tag, hb)
            _check(iir.filter(x), signal.sosfilt(sos, xw), dt, "iir.filter " + tag, hs)
            _check(np.asarray(fir.dn(x, f)), signal.lfilter(b, [1], xw)[::f][:n // f], dt, "fir.dn " + tag, hb)
            _check(np.asarray(iir.dn(x, f)), signal.sosfilt(sos, xw)[::f][:n // f], dt, "iir.dn " + tag, hs)
            if n * f <= 1_500_000:
                up = np.zeros(n * f, dtype=wide)
                up[::f] = f * xw
                _check(fir.up(x, f), signal.lfilter(b, [1], up), dt, "fir.up " + tag, hb * f)
                _check(iir.up(x, f), signal.sosfilt(sos, up), dt, "iir.up " + tag, hs * f)


def test_fuzz_multi_slot_host_calls():
    """Three slots on the one GPU of the box (skdsp_init_devices([0, 0, 0]): three streams, workspaces, handle clones and worker threads): the
    host-array FIR calls deal their chunks to all of them.  Random lengths, chunk sizes, factors and dtypes against scipy, in a process of its
    own (slots are bound once per process)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys
import numpy as np
from scipy import signal
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'scikit-dsp-comm_amd'))
from sk_dsp_comm_amd import _ffi, multirate_helper as mrh
assert _ffi.init_devices([0, 0, 0]) == 3
rng = np.random.default_rng(77)
bad = []
for case in range(40):
    dt = [np.float32, np.complex64, np.float64, np.complex128][rng.integers(4)]
    cplx = np.dtype(dt).kind == 'c'
    wide = np.complex128 if cplx else np.float64
    single = np.dtype(dt).itemsize // (2 if cplx else 1) == 4
    lg = int(rng.integers(10, 15))
    n = int(rng.integers(2, 60)) * (1 << lg) // 4 + int(rng.integers(0, 50))
    x = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
    x = x.astype(dt)
    ntaps = int(rng.choice([5, 127, 700, 1024]))
    b = signal.firwin(ntaps, 0.3)
    f = int(rng.choice([2, 3, 4, 12]))
    _ffi.set_option('host_chunk_log2', lg)
    fir = mrh.multirate_FIR(b)
    full = signal.lfilter(b, [1], x.astype(wide))
    tol = (2e-6 if single else 1e-10) * max(np.max(np.abs(full)), 1e-2 * np.max(np.abs(x)))
    k = _ffi.FirKernel(b, _ffi.code_of(dt))
    got = {'filter': fir.filter(x), 'dn': np.asarray(fir.dn(x, f)), 'sharded2': k.filter_sharded(x, 2), 'sharded3': k.filter_sharded(x, 0)}
    ref = {'filter': full, 'dn': full[::f][:n // f], 'sharded2': full, 'sharded3': full}
    if n * f <= 1_000_000:
        up = np.zeros(n * f, dtype=wide); up[::f] = f * x.astype(wide)
        got['up'] = fir.up(x, f); ref['up'] = signal.lfilter(b, [1], up)
    for name in got:
        if got[name].shape != ref[name].shape or np.max(np.abs(got[name] - ref[name])) > tol * (f if name == 'up' else 1):
            bad.append((case, name, np.dtype(dt).name, n, lg, ntaps, f))
print('MULTI_SLOT_FUZZ', 'OK' if not bad else bad)
""" % (root, root)
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert b"MULTI_SLOT_FUZZ OK" in out.stdout, out.stdout.decode()[-3000:]
