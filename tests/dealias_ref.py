"""Reference for the dealiasing truncation (TEST INFRASTRUCTURE): numpy in float64 on the same data.

The kept set is that of include/gfft.h (gfft_ps_project_dealiased): a box mask from three per-axis keep vectors and
|k|^2 <= kcut * kcut with |k|^2 = (k0^2 + k1^2) + k2^2 in double.  Boxes are those of spectrum_ref (BOX, dk = 1/2): every
k_i is exact in fp32 and every |k|^2 / dk^2 is an integer, so with kcut^2 / dk^2 an exact quarter-integer (kcut = 2.5) or
q + 1/2 the reference and a correct device cannot disagree about a mode, with or without FMA contraction.

`exact_nonlinear` is the yardstick of "alias-free": u x curl u of a field evaluated on a grid twice as fine in every
direction -- fine enough to hold every product of two of its modes -- and restricted to the N-grid's modes.  A field
truncated by the strict 2/3 rule reproduces it on the N-grid in the kept modes to rounding (4e-16 measured at the test shapes);
the looser |n| < 2/3 (N/2 + 1) is off by O(1) (0.55 ... 1.0).
"""
import numpy as np

from tests import forcing_ref as F, spectrum_ref as S


def ints(shape):
    """Global integer wavenumbers of a real transform of physical `shape`, per spectral axis"""
    n = [np.fft.fftfreq(N, 1. / N).astype(int) for N in shape]
    n[-1] = np.fft.rfftfreq(shape[-1], 1. / shape[-1]).astype(int)
    return n


def keep_vectors(shape, rule='2/3'):
    """Global per-axis keep vectors (bool): '2/3' keeps n_i iff 3 |n_i| < N_i; 'loose' is the rule |n_i| < 2/3 (N_i / 2 + 1)
    often seen, which does NOT remove the aliasing error; None keeps everything"""
    n = ints(shape)
    if rule is None:
        return [np.ones(len(ni), dtype=bool) for ni in n]
    if rule == '2/3':
        return [3 * np.abs(ni) < N for ni, N in zip(n, shape)]
    assert rule == 'loose', rule
    return [np.abs(ni) < 2. / 3. * (N // 2 + 1) for ni, N in zip(n, shape)]


def k2sq(k):
    """|k|^2 of every mode of the block whose per-axis wavenumbers are k (float64 vectors): the double expression of the device"""
    return (k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2) + k[2][None, None, :] ** 2


def keep_mask(k, m=None, kcut=np.inf):
    """The kept set as bool [n0][n1][n2]: m = three per-axis vectors of the SAME block as k (None: whole axes; an entry
    None: that axis whole), and |k|^2 <= kcut * kcut, the edge included"""
    keep = np.ones(tuple(len(ki) for ki in k), dtype=bool)
    for ax, mi in enumerate(m or ()):
        if mi is not None:
            ix = [None] * 3
            ix[ax] = slice(None)
            keep = keep & (np.asarray(mi) != 0)[tuple(ix)]
    if np.isfinite(kcut):
        keep = keep & (k2sq(k) <= np.float64(kcut) * np.float64(kcut))
    return keep


def dealiased_rhs(du, uh, k, nu, keep, force=None):
    """forcing_ref.projected (force None) or forcing_ref.forced_rhs (force = (gain, blo, bhi)) in the kept modes, +0 elsewhere"""
    rhs = F.projected(du, uh, k, nu) if force is None else F.forced_rhs(du, uh, k, nu, force[0], force[1], force[2])
    return np.where(keep[None], rhs, 0)


def nonlinear(u_hat, shape, L=S.BOX):
    """The chain of the solver on the grid `shape` itself, unprojected: forward-normalised rfftn of u x curl u with
    u = irfftn(u_hat) and curl u = irfftn(i K x u_hat).  u_hat: [3] + spectral shape"""
    uh = np.asarray(u_hat).astype('D')
    k = [ni * (2 * np.pi / Li) for ni, Li in zip(ints(shape), L)]
    k0, k1, k2 = k[0][:, None, None], k[1][None, :, None], k[2][None, None, :]
    wh = np.array([1j * (k1 * uh[2] - k2 * uh[1]), 1j * (k2 * uh[0] - k0 * uh[2]), 1j * (k0 * uh[1] - k1 * uh[0])])
    npts = float(np.prod(shape))
    u = np.array([np.fft.irfftn(a, s=shape, axes=(0, 1, 2)) for a in uh]) * npts
    w = np.array([np.fft.irfftn(a, s=shape, axes=(0, 1, 2)) for a in wh]) * npts
    return np.array([np.fft.rfftn(a) for a in np.cross(u, w, axis=0)]) / npts


def _places(shape, big):
    """Where the modes of the grid `shape` sit in the spectral array of the finer grid `big`"""
    n = ints(shape)
    return (slice(None), (n[0] % big[0])[:, None, None], (n[1] % big[1])[None, :, None], n[2][None, None, :])


def exact_nonlinear(u_hat, shape, L=S.BOX):
    """u x curl u of the field u_hat without aliasing errors: evaluated on the grid 2 * shape, which holds every sum of two
    wavenumbers of `shape`, and restricted to the modes of `shape`.  (For a field with nothing in its Nyquist planes -- any
    truncated one: a Nyquist mode has no unique place on the finer grid.)"""
    big = tuple(2 * n for n in shape)
    at = _places(shape, big)
    bh = np.zeros((3, big[0], big[1], big[2] // 2 + 1), dtype='D')
    bh[at] = np.asarray(u_hat).astype('D')
    return nonlinear(bh, big, L)[at]
