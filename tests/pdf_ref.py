"""Reference for the histogram kernels (TEST INFRASTRUCTURE): the bin rule of include/gfft.h restated with numpy float64, and
the per-point quantities of gfft_ps_gradient_pdf taken from `gradient_ref.pointwise`.

The rule, for a value x converted to double before any arithmetic and w = float64(nbins) / (hi - lo) formed once:

    t = (x - lo) * w;   x NaN -> the NaN slot;   t < 0 -> below;   t >= nbins -> above;   otherwise bin int(t)

A subtraction followed by a multiply is one defined sequence of IEEE operations (numpy never contracts), and the device
evaluates the gradient quantities with contraction switched off, so every comparison against this file is for EQUALITY of int64
arrays: there is no tolerance anywhere."""
import numpy as np

from tests import gradient_ref as G

TAIL = 3
QUANTITIES = ('ss', 'ww', 'div', 'Q', 'R', 'sss', 'wsw')          # in the order of GFFT_PS_Q_*


def slots(x, lo, hi, nbins):
    """The slot of every value: 0 ... nbins - 1 a bin, nbins below, nbins + 1 above, nbins + 2 NaN"""
    x = np.asarray(x).astype(np.float64).reshape(-1)          # converted before any arithmetic
    lo, hi = np.float64(lo), np.float64(hi)
    w = np.float64(nbins) / (hi - lo)
    with np.errstate(invalid='ignore', over='ignore'):
        t = (x - lo) * w
        nan = np.isnan(x)
        below, above = t < 0, t >= nbins
        inside = ~(nan | below | above)
        s = np.empty(x.shape, dtype=np.int64)
        s[inside] = t[inside].astype(np.int64)                # truncation: t >= 0 here (a -0.0 gives bin 0)
    s[below] = nbins
    s[above] = nbins + 1
    s[nan] = nbins + 2
    return s


def histogram(u, ranges, nbins):
    """int64 [m][nbins + 3] as gfft_ps_histogram defines it: u = [m][...] of any real precision, ranges = m (lo, hi) pairs"""
    u = np.asarray(u)
    out = np.zeros((u.shape[0], nbins + TAIL), dtype=np.int64)
    for c in range(u.shape[0]):
        out[c] = np.bincount(slots(u[c], ranges[c][0], ranges[c][1], nbins), minlength=nbins + TAIL)
    return out


def quantities(A):
    """The seven per-point quantities of A = [3][3][...] in double with the associations of gfft.h, flat, by name"""
    with np.errstate(invalid='ignore', over='ignore'):
        p = G.pointwise(A)
    return {name: np.asarray(p[name]).reshape(-1) for name in QUANTITIES}


def gradient_pdf(A, x, xr, nbx, y=None, yr=None, nby=1):
    """int64 [nbx + 3] (y None) or [nbx * nby + 2] as gfft_ps_gradient_pdf defines it; A = [3][3][...], or what `quantities`
    made of it (a test that bins one tensor many times computes them once)"""
    q = A if isinstance(A, dict) else quantities(A)
    sx = slots(q[x], xr[0], xr[1], nbx)
    if y is None:
        return np.bincount(sx, minlength=nbx + TAIL).astype(np.int64)
    sy = slots(q[y], yr[0], yr[1], nby)
    nan = (sx == nbx + 2) | (sy == nby + 2)
    inside = (sx < nbx) & (sy < nby)
    flat = np.where(nan, nbx * nby + 1, np.where(inside, sx * nby + sy, nbx * nby))          # NaN wins over outside
    return np.bincount(flat, minlength=nbx * nby + 2).astype(np.int64)
