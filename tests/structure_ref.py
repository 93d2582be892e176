"""Reference for the structure-function kernel (TEST INFRASTRUCTURE): numpy on the same data, the definition of include/gfft.h
(gfft_ps_structure) restated.

`structure` converts the field to double first, forms per point, separation and component the nine terms with the operation
sequence of gfft.h in `np.longdouble` (64 mantissa bits where the platform has them) and sums in long double by numpy's
pairwise sum -- its own error, about log2(count) 2^-64 of the magnitude, is nothing beside the bound below; where long double
is no wider than double every sum is a `math.fsum` (`gradient_ref._total`).  Beside each value stands its MAGNITUDE M: the same
expression tree with |a|, |b| at the leaves and the subtraction turned into an addition (`_terms(a, b, al, bl, mag=True)`: the
same code, so the two cannot drift apart).  The bound

    |got - ref| <= (count + 16) 2^-53 M

holds for ANY order of adding `count` doubles (each addition rounds by at most 2^-53 of a partial sum that never exceeds M) plus
at most 16 roundings per term for the per-point arithmetic (the longest term, d6 = (d d d)(d d d), has 5; each rounds by at most
2^-53 of a partial result that never exceeds the term's magnitude; a product contracted into the accumulation rounds less,
not more).  A dropped or mis-wrapped point moves a sum by about M / count, far outside the bound.
"""
import numpy as np

from tests.gradient_ref import WIDE, _total, bits      # noqa: F401  (bits: for the tests that compare bit patterns)

NVAL = 9
D1, D2, D3, D4, D5, D6, ABS1, ABS3, MIX = range(NVAL)


def _terms(a, b, al, bl, mag=False):
    """The nine per-point terms of gfft_ps_structure for one component: a = u[c][x], b = u[c][x'], (al, bl) the same of component
    lcomp or None.  mag=True: the magnitudes -- the arguments must then hold absolute values."""
    sub = (lambda x, y: x + y) if mag else (lambda x, y: x - y)
    d = sub(b, a)
    d2 = d * d
    d3 = d2 * d
    d4 = d2 * d2
    d5 = d4 * d
    d6 = d3 * d3
    ad = abs(d)
    ad3 = d2 * ad
    mx = None if al is None else sub(bl, al) * d2
    return [d, d2, d3, d4, d5, d6, ad, ad3, mx]


def structure(u, axis, seps, lcomp=-1):
    """(out, mag): out = double [nsep][ncomp][9] as gfft_ps_structure defines it for u = [ncomp][n0][n1][n2] (any real
    precision; converted to double first), increments along `axis` (0 ... 2) of the block; mag = the magnitude M under
    each entry."""
    x = np.asarray(u)
    assert x.ndim == 4 and 0 <= axis <= 2 and -1 <= lcomp < x.shape[0], (x.shape, axis, lcomp)
    x = x.astype(np.float64)                          # converted before any arithmetic
    hi = np.longdouble if WIDE else np.float64
    n = x.shape[1 + axis]
    x = x.astype(hi)
    ax = np.abs(x)
    out = np.zeros((len(seps), x.shape[0], NVAL), dtype=np.float64)
    mag = np.zeros_like(out)
    with np.errstate(invalid='ignore', over='ignore'):
        for k, r in enumerate(seps):
            assert 0 <= r < n, (r, n)
            idx = (np.arange(n) + int(r)) % n          # x' = x with index[axis] -> (index[axis] + r) mod n[axis]
            y, ay = np.take(x, idx, axis=1 + axis), np.take(ax, idx, axis=1 + axis)
            for c in range(x.shape[0]):
                t = _terms(x[c], y[c], *((x[lcomp], y[lcomp]) if lcomp >= 0 else (None, None)))
                m = _terms(ax[c], ay[c], *((ax[lcomp], ay[lcomp]) if lcomp >= 0 else (None, None)), mag=True)
                for v in range(NVAL):
                    if t[v] is None:
                        continue                       # lcomp = -1: the entry is +0.0 and nothing is formed
                    out[k, c, v] = np.float64(_total(t[v].ravel()))
                    mag[k, c, v] = np.float64(_total(m[v].ravel()))
    return out, mag


def bound(count, mag):
    return (count + 16) * 2.0 ** -53 * np.asarray(mag)


def assert_structure(got, ref, mag, count, what=''):
    """`got` within (count + 16) 2^-53 M of `ref`, entry by entry (a NaN where the reference has one); returns the worst
    fraction of the bound"""
    got, ref, mag = np.asarray(got), np.asarray(ref), np.asarray(mag)
    assert got.shape == ref.shape and got.dtype == np.float64, (what, got.shape, ref.shape, got.dtype)
    b = bound(count, mag)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, 'NaN pattern', np.argwhere(np.isnan(got) != nan))
    err = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, ref)))
    b = np.where(nan, 1.0, b)
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
    worst = float(frac.max()) if frac.size else 0.0
    print('%s: worst |got - ref| / bound = %.3g' % (what, worst))
    bad = np.argwhere(err > b)
    assert bad.size == 0, (what, bad[:4].tolist(), [(got[tuple(i)], ref[tuple(i)], b[tuple(i)]) for i in bad[:4]])
    return worst
