"""Reference for the shell co-spectrum (TEST INFRASTRUCTURE): numpy in float64 on the same data, the formulas of
include/gfft.h (gfft_ps_cospectrum), every bin summed with math.fsum.  Boxes and wavenumbers are those of
tests/spectrum_ref.py (no mode on a shell boundary).

The addends are signed, so a bin's error is bounded against the sum of ABSOLUTE terms A, which `reference` returns
beside the bins:
    DOT       A = sum over the bin of |scale| w sum_c (|Re a_c Re b_c| + |Im a_c Im b_c|)
    HELICITY  A = sum over the bin of |scale| w 2 sum |k_i Re a_j Im a_l| over the six terms of the triple product
    row 1: the same with each mode times |k|^2
Any evaluation order of M addends loses at most about (M - 1) u relative to A (u = 2^-53), forming one addend costs at
most about a dozen roundings relative to its absolute terms: per bin |got - ref| <= (M + 16) 2^-52 A, in both
precisions (the device converts its inputs exactly before any arithmetic).  Bins without modes are exactly 0.0.
"""
import math

import numpy as np

from tests.spectrum_ref import BOX, DK, default_nbins, wavenumbers      # noqa: F401  (re-exported for the tests)

DOT, HELICITY = 0, 1


def _parts(a_hat):
    a = np.asarray(a_hat)
    if a.ndim == 3:
        a = a[None]
    return a.real.astype('d'), a.imag.astype('d')


def reference(a_hat, b_hat, k, w, op=DOT, scale=1.0, dk=DK, nbins=None):
    """a_hat, b_hat: [m][n0][n1][n2] complex (any precision; converted first; b_hat ignored for HELICITY).  k, w: the
    vectors of the SAME block.  Returns (bins float64 [2][nbins], modes per bin, A float64 [2][nbins])."""
    ar, ai = _parts(a_hat)
    kx, ky, kz = k[0][:, None, None], k[1][None, :, None], k[2][None, None, :]
    if op == DOT:
        br, bi = _parts(b_hat)
        assert ar.shape == br.shape
        c = np.zeros(ar.shape[1:])
        ca = np.zeros(ar.shape[1:])
        for j in range(ar.shape[0]):
            c += ar[j] * br[j] + ai[j] * bi[j]
            ca += np.abs(ar[j] * br[j]) + np.abs(ai[j] * bi[j])
    else:
        assert ar.shape[0] == 3
        terms = [kx * (ar[1] * ai[2]), -kx * (ar[2] * ai[1]), ky * (ar[2] * ai[0]), -ky * (ar[0] * ai[2]),
                 kz * (ar[0] * ai[1]), -kz * (ar[1] * ai[0])]
        c = 2.0 * sum(np.broadcast_to(t, ar.shape[1:]) for t in terms)
        ca = 2.0 * sum(np.abs(np.broadcast_to(t, ar.shape[1:])) for t in terms)
    k2sq = (kx ** 2 + ky ** 2) + kz ** 2
    b = np.floor(np.sqrt(k2sq) / dk + 0.5).astype(np.int64)
    if nbins is None:
        nbins = int(b.max()) + 1 if b.size else 1
    e = scale * w[None, None, :] * c
    ea = abs(scale) * w[None, None, :] * ca
    order = np.argsort(b, axis=None, kind='stable')
    bs = b.ravel()[order]
    rows = [x.ravel()[order] for x in (e, k2sq * e, ea, k2sq * ea)]
    edges = np.searchsorted(bs, np.arange(nbins + 1))
    out, A = np.zeros((2, nbins)), np.zeros((2, nbins))
    for j in range(nbins):
        lo, hi = edges[j], edges[j + 1]
        out[0, j], out[1, j] = math.fsum(rows[0][lo:hi]), math.fsum(rows[1][lo:hi])
        A[0, j], A[1, j] = math.fsum(rows[2][lo:hi]), math.fsum(rows[3][lo:hi])
    return out, np.diff(edges), A


def bound(modes, A):
    return (modes + 16) * 2.0 ** -52 * A


def assert_bins(got, ref, modes, A, what='', extra=0.0):
    """per bin |got - ref| <= (modes + 16) 2^-52 A (+ `extra`, the bound of a second computed operand); empty bins 0.0"""
    got = np.asarray(got)
    assert got.shape == ref.shape == A.shape and got.dtype == np.float64, (what, got.shape, ref.shape, got.dtype)
    tol = bound(modes, A) + extra
    err = np.abs(got - ref)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print('%s: worst |got - ref| / bound = %.3f' % (what, worst))
    assert np.all(err <= tol), (what, 'worst / bound', worst, np.argwhere(err > tol)[:4].tolist())
    assert np.all(got[:, modes == 0] == 0.0), (what, 'empty bin not zero')
