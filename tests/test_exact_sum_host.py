"""The 1024-term exact power of noisereduce_amd/csrc/exact1024.hpp, restated in numpy exactly as the helper indexes it,
against a direct ``np.longdouble`` sum.

Restated: the lane / term split m = lane + 64 i, the lane twiddle w_1024^(f lane) from the 512-entry table with its sign
fold at 512, rho = w_16^f from the same table, two Horner chains of eight terms joined by rho^8 = (-1)^f, sample loads at an
index clamped into the frame's readable terms [a, b) with the select afterwards, the half-wave swap that hands real parts to
lanes 0..31 and imaginary parts to lanes 32..63, five xor steps, lanes 0 and 32.

Bound: the error of |X| stays under 1e-6 delta, delta = 2^-16 ||x w|| (the ambiguity band of the float32 decision).  Float64
rounding of a 1024-term sum is ~1e-8 delta; the nearest target tests/parity_budget.py builds is 6e-3 delta from its
threshold."""
import numpy as np
import pytest

N = 1024
BINS = (0, 1, 15, 16, 17, 255, 256, 257, 511, 512)
# readable terms [a, b) of a frame: full; cut short by the zero padding before sample 0 (a unit's first frames), behind the
# last sample, on both sides; one sample
FRAMES = ((0, 1024), (512, 1024), (256, 1024), (0, 300), (0, 769), (100, 900), (1000, 1001), (63, 65))
BOUND = 1e-6


def _table():
    k = np.arange(512, dtype=np.longdouble)
    pi = np.longdouble("3.14159265358979323846264338327950288")
    a = -2 * pi * k / N
    return (np.cos(a).astype(np.float64) + 1j * np.sin(a).astype(np.float64)).astype(np.complex128)


def _hann():
    pi = np.longdouble("3.14159265358979323846264338327950288")
    return (0.5 - 0.5 * np.cos(2 * pi * np.arange(N, dtype=np.longdouble) / N)).astype(np.float64)


TW = _table()
WIN = _hann()


def _cmul(p, q):
    """Complex product as the kernel forms it: four float64 products, no wider intermediate."""
    return (p.real * q.real - p.imag * q.imag) + 1j * (p.real * q.imag + p.imag * q.real)


def _reduce(z):
    lane = np.arange(64)
    v = np.concatenate([z.real[:32] + z.real[32:], z.imag[:32] + z.imag[32:]])
    for off in (16, 8, 4, 2, 1):
        v = v + v[lane ^ off]
    return v[0] * v[0] + v[32] * v[32]


def form_a(xa, a, b, f, win=WIN):
    """xa: the b - a readable samples (float64 values of the stored dtype); nothing else is read."""
    lane = np.arange(64)
    n = b - a
    jl = (f * lane) & 1023
    wl = np.where(jl >= 512, -TW[jl & 511], TW[jl & 511])
    jr = (f * 64) & 1023
    rho = -TW[jr & 511] if jr >= 512 else TW[jr & 511]

    def horner(i0):
        h = np.zeros(64, np.complex128)
        for i in range(7, -1, -1):
            m = lane + 64 * (i0 + i)
            r = m - a
            xs = xa[np.clip(r, 0, n - 1)]
            xv = np.where((r >= 0) & (r < n), xs, 0.0) * win[m]
            h = _cmul(h, rho) + xv
        return h
    h0, h1 = horner(0), horner(8)
    s = h0 - h1 if f & 1 else h0 + h1
    return _reduce(_cmul(s, wl))


# Form (B) (measured slower than (A) and left out of the library: tools/experiments/exact1024_hann.patch, profiles/onepass_chain.txt
# C; restated here so that the record of its accuracy stays checked): the library's own periodic Hann window factored like the twiddle,
#   cos(2 pi (lane + 64 i) / 1024) = ca CB_i - sa SB_i,  (ca, -sa) = the lane's table entry, (CB_i, SB_i) = (cos, sin)(2 pi i / 16)
def form_b(xa, a, b, f):
    lane = np.arange(64)
    n = b - a
    pi = np.longdouble("3.14159265358979323846264338327950288")
    i16 = np.arange(16, dtype=np.longdouble)
    CB, SB = np.cos(2 * pi * i16 / 16).astype(np.float64), np.sin(2 * pi * i16 / 16).astype(np.float64)
    ca, sa = TW[lane].real, -TW[lane].imag
    jl = (f * lane) & 1023
    wl = np.where(jl >= 512, -TW[jl & 511], TW[jl & 511])
    jr = (f * 64) & 1023
    rho = -TW[jr & 511] if jr >= 512 else TW[jr & 511]

    def horner(i0):
        h = np.zeros(64, np.complex128)
        for i in range(7, -1, -1):
            r = lane + 64 * (i0 + i) - a
            xs = xa[np.clip(r, 0, n - 1)]
            w = 0.5 - 0.5 * (ca * CB[i0 + i] - sa * SB[i0 + i])
            h = _cmul(h, rho) + np.where((r >= 0) & (r < n), xs, 0.0) * w
        return h
    h0, h1 = horner(0), horner(8)
    s = h0 - h1 if f & 1 else h0 + h1
    return _reduce(_cmul(s, wl))


def _direct(xa, a, b, f):
    """|X[f]|^2 in long double from first principles: exact angles, the float64 window values the kernels hold."""
    pi = np.longdouble("3.14159265358979323846264338327950288")
    m = np.arange(a, b)
    xw = xa.astype(np.longdouble) * WIN[m].astype(np.longdouble)
    ang = -2 * pi * np.longdouble((f * m) % N) / N
    re, im = np.sum(xw * np.cos(ang)), np.sum(xw * np.sin(ang))
    return re * re + im * im, np.sqrt(np.sum(xw * xw))


def _samples(dtype, n, seed):
    rng = np.random.default_rng(seed)
    if dtype == "int16":
        return rng.integers(-20000, 20000, n).astype(np.int16).astype(np.float64)
    t = np.arange(n)
    x = rng.standard_normal(n) * 0.1 + 0.5 * np.sin(2 * np.pi * 1000 / 48000 * t)
    return x.astype(dtype).astype(np.float64)


@pytest.mark.parametrize("dtype", ["float32", "float64", "int16"])
@pytest.mark.parametrize("form", ["A", "B"])
def test_exact_sum(form, dtype):
    fn = form_a if form == "A" else form_b
    worst = 0.0
    for fi, (a, b) in enumerate(FRAMES):
        xa = _samples(dtype, b - a, 100 + fi)
        for f in BINS:
            P, nrm = _direct(xa, a, b, f)
            delta = nrm * np.longdouble(2.0) ** -16
            got = np.longdouble(fn(xa, a, b, f))
            err = abs(np.sqrt(got) - np.sqrt(P)) / delta
            worst = max(worst, float(err))
            assert err < BOUND, "form %s %s frame [%d, %d) bin %d: |X| off by %.3e delta" % (form, dtype, a, b, f, err)
    print("form %s %s: largest error of |X| %.3e delta (bound %.0e)" % (form, dtype, worst, BOUND))


def test_hann_factoring_matches_the_window_table():
    """Form (B) rebuilds each window value from the lane's table entry and sixteen constants: within a few float64 ulps of
    the table the library uploads (what form (A) loads)."""
    lane = np.arange(64)
    pi = np.longdouble("3.14159265358979323846264338327950288")
    i16 = np.arange(16, dtype=np.longdouble)
    CB, SB = np.cos(2 * pi * i16 / 16).astype(np.float64), np.sin(2 * pi * i16 / 16).astype(np.float64)
    ca, sa = TW[lane].real, -TW[lane].imag
    for i in range(16):
        w = 0.5 - 0.5 * (ca * CB[i] - sa * SB[i])
        assert np.max(np.abs(w - WIN[lane + 64 * i])) < 4 * np.finfo(np.float64).eps


def test_reduction_sums_the_same_pairs_in_the_same_order():
    """One double per half-wave after the swap = both components through the full six-step butterfly, bit for bit."""
    rng = np.random.default_rng(7)
    z = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    lane = np.arange(64)
    re, im = z.real.copy(), z.imag.copy()
    for off in (32, 16, 8, 4, 2, 1):
        re, im = re + re[lane ^ off], im + im[lane ^ off]
    assert _reduce(z) == re[0] * re[0] + im[0] * im[0]
    assert np.all(re == re[0]) and np.all(im == im[0])


def _terms(s0, e, Lp, lo, hi):
    """exact1024_terms: the terms [a, b) whose sample exists; term m is sample s0 + m of the unit window [0, Lp) and
    element e + m of a row readable in [lo, hi)."""
    first = max(-s0, lo - e)
    end = min(Lp - s0, hi - e)
    return min(max(first, 0), 1024), min(max(end, 0), 1024)


def test_readable_terms_are_view_samples_two_tests():
    """[a, b) holds exactly the terms that pass both range tests of the per-sample path (geom.hpp: view_sample), for frames
    in the zero padding before a row, across chunk seams, behind the last sample and wholly outside; every index the
    clamped loads can form lies inside both ranges."""
    H, padL = 256, 512
    cs, pad = 12288, 3000
    Lp = cs + 2 * pad
    N = 4 * cs + 300
    m = np.arange(1024)
    for chunk in range(-1, 6):
        for lo, hi in ((0, N), (100, N - 77)):
            for t in list(range(0, 8)) + list(range(Lp // H - 4, Lp // H + 6)):
                s0 = t * H - padL
                e = chunk * cs - pad + s0
                a, b = _terms(s0, e, Lp, lo, hi)
                sp, gi = s0 + m, e + m
                ok = (sp >= 0) & (sp < Lp) & (gi >= lo) & (gi < hi)
                want = np.flatnonzero(ok)
                if len(want) == 0:
                    assert a >= b, (chunk, t, a, b)
                    continue
                assert (a, b) == (want[0], want[-1] + 1) and len(want) == b - a, (chunk, t, a, b, want[0], want[-1])
                rc = np.clip(m - a, 0, b - a - 1) + a
                assert np.all(ok[rc]), (chunk, t)
