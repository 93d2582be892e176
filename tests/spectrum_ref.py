"""Reference for the shell spectrum (TEST INFRASTRUCTURE): numpy in float64 on the same data, the formula of
include/gfft.h (gfft_ps_spectrum), every bin summed with math.fsum -- correctly rounded, so the only error budget in
a comparison is the device's.

Boxes: only ones in which every k_i / dk is an integer exactly representable in fp32.  Then (|k| / dk)^2 is an integer
and can never equal (j + 1/2)^2: no mode sits on a shell boundary, and the reference cannot disagree with a correct
device about a bin.  `wavenumbers` asserts it.
"""
import math

import numpy as np

BOX = (2 * np.pi, 4 * np.pi, 2 * np.pi)      # L of the tests: k = (i, i / 2, i), dk = 1/2
DK = 0.5


def wavenumbers(shape, real, L=BOX, dk=DK):
    """Global per-axis wavenumbers (float64) and Hermitian weights of a transform of physical `shape`."""
    k = [np.fft.fftfreq(n, 1. / n) for n in shape]
    if real:
        k[-1] = np.fft.rfftfreq(shape[-1], 1. / shape[-1])
    k = [ki.astype(int) * (2 * np.pi / Li) for ki, Li in zip(k, L)]
    for ki in k:
        assert np.array_equal(ki / dk, np.round(ki / dk)) and np.array_equal(ki.astype('f').astype('d'), ki), 'box with shell-boundary ties'
    w = np.ones(len(k[-1]))
    if real:
        i2 = np.arange(len(w))
        w[(i2 != 0) & (2 * i2 != shape[-1])] = 2
    return k, w


def default_nbins(shape, L=BOX, dk=DK):
    kmax = math.sqrt(sum((n // 2 * 2 * np.pi / Li) ** 2 for n, Li in zip(shape, L)))
    return int(math.floor(kmax / dk + 0.5)) + 1


def reference(u_hat, k, w, dk=DK, nbins=None):
    """u_hat: [m][n0][n1][n2] complex (any precision; converted first).  k, w: the vectors of the SAME block.
    Returns (bins float64 [2][nbins], modes per bin); modes beyond the last bin are dropped."""
    u = np.asarray(u_hat)
    if u.ndim == 3:
        u = u[None]
    re, im = u.real.astype('d'), u.imag.astype('d')
    s = np.zeros(u.shape[1:])
    for c in range(u.shape[0]):
        s += re[c] * re[c] + im[c] * im[c]
    k2sq = (k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2) + k[2][None, None, :] ** 2
    b = np.floor(np.sqrt(k2sq) / dk + 0.5).astype(np.int64)
    if nbins is None:
        nbins = int(b.max()) + 1 if b.size else 1
    e = 0.5 * w[None, None, :] * s
    f = k2sq * e
    order = np.argsort(b, axis=None, kind='stable')
    bs = b.ravel()[order]
    es, fs = e.ravel()[order], f.ravel()[order]
    edges = np.searchsorted(bs, np.arange(nbins + 1))
    out = np.zeros((2, nbins))
    for j in range(nbins):
        out[0, j] = math.fsum(es[edges[j]:edges[j + 1]])
        out[1, j] = math.fsum(fs[edges[j]:edges[j + 1]])
    return out, np.diff(edges)


def assert_bins(got, ref, modes, what=''):
    """All addends are non-negative: any summation order of M addends is off by at most (M - 1) 2^-53 relative, and
    forming one addend costs a few more roundings -- per bin |got - ref| <= (M + 16) 2^-52 ref, for fp32 input too (the
    device converts exactly before any arithmetic).  Empty bins are exactly 0.0."""
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.float64, (what, got.shape, ref.shape, got.dtype)
    tol = (modes + 16) * 2.0 ** -52 * ref
    err = np.abs(got - ref)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print('%s: worst |got - ref| / bound = %.3f' % (what, worst))
    assert np.all(err <= tol), (what, 'worst / bound', worst, np.argwhere(err > tol)[:4].tolist())
    assert np.all(got[:, modes == 0] == 0.0), (what, 'empty bin not zero')
