"""Reference for the velocity-gradient kernels (TEST INFRASTRUCTURE): numpy on the same data, the formulas of include/gfft.h
(gfft_ps_gradient, gfft_ps_gradient_stats).

`grad` works in the field's own precision: each part of each value is one product, so a correct device agrees bit for bit.

`stats` converts to double first, evaluates the per-point expressions of gfft.h in `np.longdouble` (64 mantissa bits where the
platform has them) and sums in long double by numpy's pairwise sum -- its own error, about log2(count) 2^-64 of the magnitude, is
nothing beside the bound below; where long double is no wider than double every sum is a `math.fsum` instead.  Beside each
value stands its MAGNITUDE M: the same expression tree with every leaf replaced by its absolute value, every subtraction by an
addition and the negation of R dropped (`_terms(a, mag=True)`: the same code, so the two cannot drift apart); for a maximum, M
is taken at the maximising point.  The bound

    |got - ref| <= (count + 64) 2^-53 M

holds for ANY order of adding `count` doubles (each addition rounds by at most 2^-53 of a partial sum that never exceeds M) plus
64 roundings per point for the per-point arithmetic (the longest expression, S_ij S_jk S_ki, has 26 operations; each rounds by at
most 2^-53 of a partial result that never exceeds the point's magnitude).  A dropped point shifts a sum by about M / count.
"""
import math

import numpy as np

from tests import dealias_ref as D, scalar_ref as C, spectrum_ref as R

NVAL, NMAX = 20, 3
WIDE = np.finfo(np.longdouble).nmant >= 63
CHUNK = 1 << 17


def grad(f_hat, k):
    """out[c][j] = i k_j f_hat[c] as {-(k_j * Im f), k_j * Re f} in the precision of f_hat: f_hat [m] + block (or the block: out
    [3] + block), k the per-axis wavenumbers of the block (converted to that precision first) -> [m][3] + block"""
    f = np.asarray(f_hat)
    scalar = f.ndim == 3
    if scalar:
        f = f[None]
    rdt = f.real.dtype
    ks = [np.asarray(k[0]).astype(rdt)[:, None, None], np.asarray(k[1]).astype(rdt)[None, :, None], np.asarray(k[2]).astype(rdt)[None, None, :]]
    out = np.empty((f.shape[0], 3) + f.shape[1:], dtype=f.dtype)
    with np.errstate(invalid='ignore'):
        for j in range(3):
            out[:, j].real = -(ks[j] * f.imag)
            out[:, j].imag = ks[j] * f.real
    assert out.real.dtype == rdt
    return out[0] if scalar else out


def bits(a):
    """The bit patterns of a real or complex array"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype in (np.float64, np.complex128) else np.int32)


def _terms(a, mag=False):
    """The per-point quantities of gfft_ps_gradient_stats with its associations, a = the nine A_ij (index 3 i + j) as arrays:
    (maxima [3], summands [17]).  mag=True: the magnitudes -- `a` must then hold absolute values."""
    sub = (lambda x, y: x + y) if mag else (lambda x, y: x - y)
    neg = (lambda x: x) if mag else (lambda x: -x)
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = a
    div = (a00 + a11) + a22
    s01, s02, s12 = 0.5 * (a01 + a10), 0.5 * (a02 + a20), 0.5 * (a12 + a21)
    w0, w1, w2 = sub(a21, a12), sub(a02, a20), sub(a10, a01)
    q00, q11, q22 = a00 * a00, a11 * a11, a22 * a22
    d2 = (q00 + q11) + q22
    p01, p02, p12 = s01 * s01, s02 * s02, s12 * s12
    ss = d2 + 2 * ((p01 + p02) + p12)
    ww = (w0 * w0 + w1 * w1) + w2 * w2
    Q = 0.5 * sub(div * div, d2 + 2 * ((a01 * a10 + a02 * a20) + a12 * a21))
    Rr = neg(sub(a00 * sub(a11 * a22, a12 * a21), a01 * sub(a10 * a22, a12 * a20)) + a02 * sub(a10 * a21, a11 * a20))
    d3 = (a00 * q00 + a11 * q11) + a22 * q22
    sss = (d3 + 3 * ((a00 * (p01 + p02) + a11 * (p01 + p12)) + a22 * (p02 + p12))) + 6 * ((s01 * s02) * s12)
    wsw = ((a00 * (w0 * w0) + a11 * (w1 * w1)) + a22 * (w2 * w2)) + 2 * ((s01 * (w0 * w1) + s02 * (w0 * w2)) + s12 * (w1 * w2))
    o01, o10, o02, o20, o12, o21 = a01 * a01, a10 * a10, a02 * a02, a20 * a20, a12 * a12, a21 * a21
    maxima = [ss, ww, abs(div)]
    sums = [div * div, ss, ww, ss * ss, ww * ww, ss * ww, Q, Rr, Q * Q, Rr * Rr, sss, wsw, d2, d3,
            (q00 * q00 + q11 * q11) + q22 * q22, ((o01 + o10) + (o02 + o20)) + (o12 + o21),
            ((o01 * o01 + o10 * o10) + (o02 * o02 + o20 * o20)) + (o12 * o12 + o21 * o21)]
    return maxima, sums


def pointwise(A):
    """ss, ww, Q, R, sss, wsw per point in double, for the pointwise identities: A [3][3] + any shape"""
    a = list(np.asarray(A).astype(np.float64).reshape((9,) + np.asarray(A).shape[2:]))
    _, s = _terms(a)
    return dict(ss=s[1], ww=s[2], Q=s[6], R=s[7], sss=s[10], wsw=s[11], div=(a[0] + a[4]) + a[8])


def _total(x):
    if WIDE:
        return x.sum(dtype=np.longdouble)
    x = np.asarray(x, dtype=np.float64)
    return np.longdouble(math.fsum(x)) if np.isfinite(x).all() else np.longdouble(x.sum())


def stats(A):
    """(out, mag): out = double[20] as gfft_ps_gradient_stats defines it for A = [3][3][...] (any real precision; converted to
    double first), mag = the magnitude M under each entry."""
    x = np.asarray(A)
    assert x.shape[:2] == (3, 3), x.shape
    x = x.reshape(9, -1).astype(np.float64)          # converted before any arithmetic
    count = x.shape[1]
    hi = np.longdouble if WIDE else np.float64
    vmax, mmax = np.zeros(NMAX, dtype=hi), np.zeros(NMAX, dtype=hi)
    vsum, msum = np.zeros(NVAL - NMAX, dtype=np.longdouble), np.zeros(NVAL - NMAX, dtype=np.longdouble)
    with np.errstate(invalid='ignore'):
        for lo in range(0, count, CHUNK):
            a = list(x[:, lo:lo + CHUNK].astype(hi))
            mx, sm = _terms(a)
            mmx, msm = _terms([np.abs(ai) for ai in a], mag=True)
            for i in range(NMAX):
                v = np.where(np.isnan(mx[i]), -np.inf, mx[i])          # fmax skips a NaN
                at = int(np.argmax(v))
                if v[at] > vmax[i]:
                    vmax[i], mmax[i] = v[at], mmx[i][at]
            for i in range(NVAL - NMAX):
                vsum[i] += _total(sm[i])
                msum[i] += _total(msm[i])
    out = np.concatenate([vmax, vsum]).astype(np.float64)
    mag = np.concatenate([mmax, msum]).astype(np.float64)
    return out, mag


def bound(count, mag):
    return (count + 64) * 2.0 ** -53 * np.asarray(mag)


def assert_stats(got, ref, mag, count, what=''):
    """`got` within (count + 64) 2^-53 M of `ref`, entry by entry (a NaN where the reference has one); returns the worst
    fraction of the bound"""
    got, ref, mag = np.asarray(got), np.asarray(ref), np.asarray(mag)
    assert got.shape == ref.shape == (NVAL,) and got.dtype == np.float64, (what, got.shape, got.dtype)
    b = bound(count, mag)
    worst = 0.0
    for i in range(NVAL):
        if np.isnan(ref[i]):
            assert np.isnan(got[i]), (what, i, got[i])
            continue
        err = abs(got[i] - ref[i])
        worst = max(worst, err / b[i] if b[i] > 0 else (0.0 if err == 0 else np.inf))
        assert err <= b[i], (what, i, got[i], ref[i], err, b[i])
    print('%s: worst |got - ref| / bound = %.4f' % (what, worst))
    return worst


def solenoidal_field(shape, seed, truncate=True):
    """(u_hat [3] + spectral block, k): the forward-normalised transform of a random real field in the box of spectrum_ref,
    truncated by the strict 2/3 rule (truncate=False: every mode stays, the Nyquist planes included) and projected onto
    k . u_hat = 0"""
    rng = np.random.default_rng(seed)
    k, _ = R.wavenumbers(shape, True)
    uh = np.array([np.fft.rfftn(a) for a in rng.standard_normal((3,) + tuple(shape))]) / np.prod(shape)
    if truncate:
        uh = uh * D.keep_mask(k, D.keep_vectors(shape))
    return C.solenoidal(uh, k), k


def tensor(u_hat, k, shape):
    """A [3][3] + shape in double: the backward transforms of grad(u_hat, k)"""
    g = grad(np.asarray(u_hat).astype('D'), k)
    n = float(np.prod(shape))
    return np.array([[np.fft.irfftn(g[i, j], s=shape, axes=(0, 1, 2)) * n for j in range(3)] for i in range(3)])
