"""The instrument of tests/_errspec.py, tested without a GPU.

1. The yardstick is steady: for both tap sets, complex64 at 1024 taps, over six seeds, the host overlap-save alone has A <= 2.5 and
   B <= 2.5 (seen: 1.6 - 2.1 and 1.5 - 1.8).  These are the conditions under which 4 x the yardstick stays below 10.
2. The exact references of the impulse taps (y[n] = x[n - d_0]; y[i L + r] = L x[i - (d_r - r) / L]; y[i] = sum_r x[i M - d_r]) agree with
   scipy.signal.lfilter over zero-stuffed and decimated float64 data to 1e-13, for F = 1, L in {3, 4, 12}, M in {2, 3, 4}, (L, M) = (4, 3).
3. The gap this instrument closes, on a float32 model of the 8192-point tile (64 x 128, one inter-pass twiddle table per direction, 1024
   taps, 64 + 1 segments of complex noise).  One entry of a twiddle table off by 1e-5 -- an entry with 16 good bits -- or one bin of the taps
   spectrum off by 1e-6 or 3e-6 leaves max |err| / peak under the 1e-6 every accuracy test of the tile engines asks for:

       fault                                       max err / peak      A (clean model and yardstick: 1.7 - 2.1)
       none                                        2.1e-7 - 2.4e-7     1.7 - 2.1
       forward twiddle entry x (1 + 1e-5)          2.6e-7 - 4.0e-7     15 - 24
       inverse twiddle entry x (1 + 1e-5)          7.4e-7 - 8.4e-7     20 - 24    (B: 38 - 49 against 1.6)
       one bin of the taps spectrum x (1 + 1e-6)   unchanged           17 - 28
       one bin of the taps spectrum x (1 + 3e-6)   unchanged           160 - 250

   Each must stay under 1e-6 and push A over 4 x the yardstick's A of the same input; the inverse-table fault must push B over 4 x the
   yardstick's B as well (it sits on 64 of the tile's 8192 output positions)."""
import numpy as np
import pytest
import scipy.signal as signal

import _errspec as es

P = 1024
N = 8192
NSAMP = (es.MIN_SEGMENTS + 1) * es.SEG
OV, V = es.tile_overlap(P, 512, N)
OLD_CONTRACT = 1e-6


def taps_and_ref(kind, x):
    if kind == "impulse":
        b, d = es.impulse_taps(P, 1)
        return b, es.exact_filter(d, x)
    b = es.chirp_taps(P, 1, True)
    return b, signal.oaconvolve(x.astype(np.complex128), b)[:len(x)]   # float64: 1e-16 of the output, nine decades below what is measured


def test_impulse_positions_are_fixed_and_spread():
    for F, want in ((1, [1023]), (2, [256, 1023]), (3, [1023, 511, 854]), (4, [128, 385, 642, 1023])):
        b, d = es.impulse_taps(P, F)
        print("impulse taps P = %d F = %d: d =" % (P, F), d.tolist())
        assert d.tolist() == want
        assert b[P - 1] == 1.0 and np.count_nonzero(b) == F and np.sum(b) == F
    for Pn, F in ((516, 12), (300, 1), (4097, 1), (2049, 5), (512, 3), (1024, 12)):
        b, d = es.impulse_taps(Pn, F)
        assert np.all(d % F == np.arange(F)) and b[Pn - 1] == 1.0 and np.count_nonzero(b) == F
        T = -(-Pn // F)
        if F > 2:   # spread over the length of the branch: both halves of the taps are used
            assert np.min(d) < Pn // 2 < np.max(d) and len(set((d // F).tolist())) >= F - 1, (Pn, F, d, T)


@pytest.mark.parametrize("kind", ["impulse", "chirp"])
def test_yardstick_is_steady(kind):
    for seed in range(6):
        x = es.noise(NSAMP, np.complex64, seed)
        b, ref = taps_and_ref(kind, x)
        m = es.measure(es.yardstick(b, x, N, np.complex64, overlap=OV), ref, period=V)
        print("yardstick %s seed %d: R %.3g A %.3g (bin %d) B %.3g (position %d)" % (kind, seed, m["R"], m["A"], m["bin"], m["B"], m["pos"]))
        assert m["A"] <= 2.5 and m["B"] <= 2.5, (kind, seed, m)
        assert 5e-8 < m["R"] < 5e-7, m   # float32 transforms: a yardstick in double precision would read 1e-16


def lfilter_ref(b, x, L=1, M=1):
    u = np.zeros(len(x) * L, x.dtype)
    u[::L] = L * x
    return signal.lfilter(b, 1.0, u)[::M][:len(u) // M]


@pytest.mark.parametrize("cplx", [False, True])
def test_exact_references_agree_with_lfilter(cplx):
    rng = np.random.default_rng(5)
    n = 5000
    x = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
    for Pn in (300, 516, 1024):
        b, d = es.impulse_taps(Pn, 1)
        assert np.max(np.abs(es.exact_filter(d, x) - lfilter_ref(b, x))) <= 1e-13
        hist = rng.standard_normal(Pn - 1) + (1j * rng.standard_normal(Pn - 1) if cplx else 0)
        with_hist = signal.lfilter(b, 1.0, np.concatenate([hist, x]))[Pn - 1:]
        assert np.max(np.abs(es.exact_filter(d, x, hist) - with_hist)) <= 1e-13
        for L in (3, 4, 12):
            b, d = es.impulse_taps(Pn, L)
            y = es.exact_up(d, x, L)
            assert y.shape == (n * L,) and np.max(np.abs(y - lfilter_ref(b, x, L))) <= 1e-13, (Pn, L)
        for M in (2, 3, 4):
            b, d = es.impulse_taps(Pn, M)
            y = es.exact_dn(d, x, M)
            assert y.shape == (n // M,) and np.max(np.abs(y - lfilter_ref(b, x, 1, M))) <= 1e-13, (Pn, M)
        b, d = es.impulse_taps(Pn, 4)
        y = es.exact_updn(d, x, 4, 3)
        assert y.shape == (n * 4 // 3,) and np.max(np.abs(y - lfilter_ref(b, x, 4, 3))) <= 1e-13, Pn
    x32 = x.astype(np.complex64 if cplx else np.float32)   # float32 inputs: float64 holds the sum of M of them exactly
    b, d = es.impulse_taps(1024, 4)
    assert np.array_equal(es.exact_dn(d, x32, 4), lfilter_ref(b, x32.astype(x.dtype), 1, 4))


ENTRIES = ((5, 77), (40, 100), (63, 127))   # (k1, n2) of the inter-pass tables
BINS = (100, 4097)


@pytest.fixture(scope="module", params=[0, 1], ids=lambda s: "seed%d" % s)
def clean(request):
    x = es.noise(NSAMP, np.complex64, request.param)
    b, ref = taps_and_ref("chirp", x)
    yard = es.measure(es.yardstick(b, x, N, np.complex64, overlap=OV), ref, period=V)
    model = es.two_pass_model(b, x)
    m = es.measure(model, ref, period=V)
    print("clean model: max err / peak %.3g, R %.3g A %.3g B %.3g; yardstick: R %.3g A %.3g B %.3g"
          % (es.peak_err(model, ref), m["R"], m["A"], m["B"], yard["R"], yard["A"], yard["B"]))
    return x, b, ref, yard, m


def test_clean_model_is_inside_every_limit(clean):
    x, b, ref, yard, m = clean
    assert m["R"] <= 2 * yard["R"] and m["A"] <= 4 * yard["A"] and m["B"] <= 4 * yard["B"], (m, yard)


@pytest.mark.parametrize("which", ["forward", "inverse"])
def test_one_twiddle_entry_with_16_good_bits(clean, which):
    x, b, ref, yard, _ = clean
    for k1, n2 in ENTRIES:
        fwd, inv = es.two_pass_tables()
        (fwd if which == "forward" else inv)[k1, n2] *= np.complex64(1 + 1e-5)
        y = es.two_pass_model(b, x, fwd, inv)
        old, m = es.peak_err(y, ref), es.measure(y, ref, period=V)
        print("%s T[%d, %d] x (1 + 1e-5): max err / peak %.3g, R %.3g, A %.3g (bin %d; yardstick %.3g), B %.3g (position %d; yardstick %.3g)"
              % (which, k1, n2, old, m["R"], m["A"], m["bin"], yard["A"], m["B"], m["pos"], yard["B"]))
        assert old < OLD_CONTRACT, "the fault is meant to pass today's contract"
        assert m["A"] > 4 * yard["A"], (which, k1, n2, m, yard)
        if which == "inverse":
            assert m["B"] > 4 * yard["B"], (k1, n2, m, yard)
            assert m["pos"] % es.N2 == (n2 + OV) % es.N2   # the entry's column n2 of the tile: outputs n = 128 n1 + n2 - overlap
        else:
            assert m["bin"] % es.N1 == k1                  # the entry's row k1: bins k = k1 + 64 k2


@pytest.mark.parametrize("eps", [1e-6, 3e-6])
def test_one_bin_of_the_taps_spectrum(clean, eps):
    x, b, ref, yard, _ = clean
    for k in BINS:
        H = es.model_H(b)
        H[k] *= np.complex64(1 + eps)
        y = es.two_pass_model(b, x, H=H)
        old, m = es.peak_err(y, ref), es.measure(y, ref, period=V)
        print("H[%d] x (1 + %g): max err / peak %.3g, R %.3g, A %.3g (bin %d; yardstick %.3g), B %.3g" % (k, eps, old, m["R"], m["A"], m["bin"], yard["A"], m["B"]))
        assert old < OLD_CONTRACT
        assert m["A"] > 4 * yard["A"] and m["bin"] == k, (k, eps, m, yard)
        assert m["R"] <= 2 * yard["R"]   # (neither R nor today's metric sees it)
