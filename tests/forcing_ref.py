"""Reference for the band forcing (TEST INFRASTRUCTURE): numpy in float64 on the same data.

The band mask comes from `spectrum_ref.wavenumbers` with the floor(sqrt(k2sq) / dk + 0.5) of `spectrum_ref.reference`; the
boxes are those of spectrum_ref (no mode on a shell boundary: the mask and a correct device cannot disagree).  The right-hand
side is the expressions of tests/test_gpu_dns.py::test_spectral_kernels_against_expressions with the forcing term added
after the projection and the viscous term; the gain is the formula of include/gfft.h (gfft_ps_force_gain), restated.
"""
import math

import numpy as np

from tests import spectrum_ref as S


def shells(k, dk=S.DK):
    """Shell of every mode of the block whose per-axis wavenumbers are k (float64 vectors): int64 [n0][n1][n2]"""
    k2sq = (k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2) + k[2][None, None, :] ** 2
    return np.floor(np.sqrt(k2sq) / dk + 0.5).astype(np.int64)


def band_mask(k, blo, bhi, dk=S.DK):
    b = shells(k, dk)
    return (b >= blo) & (b <= bhi)


def projected(du, uh, k, nu):
    """Projection + viscous term in complex128: rhs = du - (sum du K / K2) K - nu K2 uh"""
    K = np.array(np.broadcast_arrays(k[0][:, None, None], k[1][None, :, None], k[2][None, None, :])).astype(float)
    K2 = np.sum(K * K, 0)
    K_over_K2 = K / np.where(K2 == 0, 1, K2)
    rhs = np.asarray(du).astype('D')
    P_hat = np.sum(rhs * K_over_K2, 0)
    rhs = rhs - P_hat * K
    return rhs - nu * K2 * np.asarray(uh).astype('D')


def forced_rhs(du, uh, k, nu, gain, blo, bhi, dk=S.DK):
    """The forced right-hand side: `projected`, then + gain uh inside the band"""
    return projected(du, uh, k, nu) + float(gain) * np.where(band_mask(k, blo, bhi, dk)[None], np.asarray(uh).astype('D'), 0)


def force_gain(row, blo, bhi, eps, gain_max=math.inf):
    """(gain, E_f): E_f = row[blo] + ... + row[bhi] added serially from 0.0; gain = min(eps / (2 E_f), gain_max), 0 unless
    E_f > 0 and finite"""
    row = np.asarray(row, dtype=np.float64)
    ef = np.float64(0.0)
    for b in range(blo, bhi + 1):
        ef = ef + row[b]
    if not (ef > 0.0 and np.isfinite(ef)):
        return 0.0, float(ef)
    with np.errstate(over='ignore'):
        g = np.float64(eps) / (np.float64(2.0) * ef)
    return float(np.minimum(g, np.float64(gain_max))), float(ef)


def band_term(uh, k, blo, bhi, gain, dk=S.DK):
    """real(gain) * uh inside the band and 0 outside, in uh's own precision: the gain converted once, one rounding per real
    scalar -- what the device leaves in du where du = 0 and nu = 0, exactly"""
    uh = np.asarray(uh)
    g = uh.real.dtype.type(gain)
    out = np.zeros_like(uh)
    m = band_mask(k, blo, bhi, dk)[None]
    out.real[...] = np.where(m, g * uh.real, 0)
    out.imag[...] = np.where(m, g * uh.imag, 0)
    return out
