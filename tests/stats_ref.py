"""Reference of gfft_ps_stats / SpectralOps.stats for the tests: numpy and math.fsum.

The input is converted to double first and the powers are formed as the kernel forms them (u u, (u u) u, (u u)(u u), each
a single rounded double product); every sum is then an `fsum` of those terms -- correctly rounded, so the reference
itself carries no summation error and the tests' bound is the kernel's alone:

    |got - ref| <= (count + 4) 2^-53 sum |term|

which holds for ANY order of adding `count` doubles (each of the count - 1 additions rounds by at most 2^-53 of a partial
sum that never exceeds sum |term|), plus the reference's own final rounding.  Maxima and minima are exact in any order.
Entries 0 and 1 are maxima of short sums the kernel may contract into fused multiply-adds: 4 2^-53 relative covers the
(at most four) roundings that differ.  NaN: np.fmax / np.fmin ignore it as fmax / fmin do; fsum propagates it.
"""
import math

import numpy as np

HEAD, PER = 2, 6


def nval(m):
    return HEAD + PER * m


def reference(u, inv_dx):
    """(out, mag): out = double[2 + 6 m] as gfft_ps_stats defines it for u = [m][...], mag = the same layout holding
    sum |term| under each sum (0 under the extrema) for the any-order bound."""
    u = np.asarray(u)
    m = u.shape[0]
    x = u.reshape(m, -1).astype(np.float64)          # converted before any arithmetic
    inv = np.asarray(inv_dx, dtype=np.float64)
    assert inv.shape == (m,)
    out, mag = np.zeros(nval(m)), np.zeros(nval(m))
    if x.shape[1]:
        rate, sq = np.zeros(x.shape[1]), np.zeros(x.shape[1])
        for c in range(m):
            rate = rate + np.abs(x[c]) * inv[c]
            sq = sq + x[c] * x[c]
        out[0] = np.fmax.reduce(rate, initial=0.0)
        out[1] = np.fmax.reduce(sq, initial=0.0)
    for c in range(m):
        xc = x[c]
        xx = xc * xc
        o = HEAD + PER * c
        out[o + 0] = np.fmax.reduce(xc, initial=-np.inf)
        out[o + 1] = np.fmin.reduce(xc, initial=np.inf)
        for j, term in enumerate((xc, xx, xx * xc, xx * xx)):
            out[o + 2 + j] = math.fsum(term) if np.isfinite(term).all() else float(term.sum())
            mag[o + 2 + j] = math.fsum(np.abs(term)) if np.isfinite(term).all() else np.nan
    return out, mag


def reference_int(u, inv_dx):
    """The same for an integer-valued field with 2 inv_dx integer too: int64 arithmetic, every entry exact."""
    u = np.asarray(u)
    m = u.shape[0]
    x = u.reshape(m, -1).astype(np.int64)
    assert np.array_equal(x, u.reshape(m, -1))
    inv2 = np.rint(2 * np.asarray(inv_dx, dtype=np.float64)).astype(np.int64)
    assert np.array_equal(inv2 / 2.0, np.asarray(inv_dx, dtype=np.float64))
    out = np.zeros(nval(m))
    if x.shape[1]:
        out[0] = (np.abs(x) * inv2[:, None]).sum(0).max() / 2.0
        out[1] = (x * x).sum(0).max()
    for c in range(m):
        o = HEAD + PER * c
        out[o + 0] = x[c].max() if x.shape[1] else -np.inf
        out[o + 1] = x[c].min() if x.shape[1] else np.inf
        for j in range(4):
            out[o + 2 + j] = float((x[c] ** (j + 1)).sum())
    return out


def assert_stats(got, ref, mag, count, what=''):
    """`got` within the derived bounds of the module docstring around (ref, mag)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for i in range(len(ref)):
        k = i - HEAD
        if i < HEAD:
            assert abs(got[i] - ref[i]) <= 4 * 2.0 ** -53 * abs(ref[i]), (what, i, got[i], ref[i])
        elif k % PER < 2:
            assert got[i] == ref[i], (what, i, got[i], ref[i])
        elif np.isnan(ref[i]):
            assert np.isnan(got[i]), (what, i, got[i])
        else:
            assert abs(got[i] - ref[i]) <= (count + 4) * 2.0 ** -53 * mag[i], (what, i, got[i], ref[i], mag[i])


def timestep(rate, cfl, dt_max, dt_min=0.0):
    """The formula of gfft_ps_timestep, written out independently of the package"""
    want = cfl / rate if (rate > 0 and not math.isinf(rate) and not math.isnan(rate)) else dt_max
    return min(max(want, dt_min), dt_max)
