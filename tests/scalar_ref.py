"""Reference for the passive-scalar kernels (TEST INFRASTRUCTURE): numpy in float64 on the same data, the formulas of
include/gfft.h (gfft_ps_scalar_flux, gfft_ps_scalar_rhs).

    d theta / dt + div(u theta) = kappa lap theta - G . u        (flux form; u solenoidal)

`advect` is the solver's chain on the grid itself -- backward, pointwise product, forward --, `exact_advect` its alias-free
yardstick: the same products on a grid twice as fine in every direction, restricted to the N-grid's modes, built like
dealias_ref.exact_nonlinear.  Fields truncated by the strict 2/3 rule reproduce it on the N-grid in the kept modes to
rounding (3e-16 ... 7e-16 at the test shapes); the loose rule is off by O(1).

`rk4_factor` is the closed form of uniform advection: with u = c constant every mode obeys d = lambda theta, lambda = -i c.k -
kappa |k|^2, and n RK4 steps of size h multiply it by R(lambda h)^n, R(z) = 1 + z + z^2/2 + z^3/6 + z^4/24.
"""
import numpy as np

from tests import dealias_ref as D


def flux(u, theta):
    """flux[s][c] = u[c] * theta[s] in the arrays' own precision: u [3] + shape, theta [m] + shape -> [m][3] + shape"""
    return u[None] * theta[:, None]


def _mesh(k):
    return k[0][:, None, None], k[1][None, :, None], k[2][None, None, :]


def rhs_modes(F, th, kx, ky, kz, kappa, G=None, u=None):
    """d[s] = -i (k . F[s]) - kappa[s] |k|^2 theta[s] - G[s] . u in float64 on any set of modes: F [m][3] + X, th [m] + X,
    u [3] + X, kx / ky / kz broadcastable to X; kappa m floats, G m x 3 floats (with u) or None"""
    F, th = np.asarray(F).astype('D'), np.asarray(th).astype('D')
    kk = kx * kx + ky * ky + kz * kz
    kappa = np.asarray(kappa, dtype='d').reshape(-1)
    d = np.empty_like(th)
    for s in range(th.shape[0]):
        a = kx * F[s, 0] + ky * F[s, 1] + kz * F[s, 2]
        d[s] = -1j * a - (kappa[s] * kk) * th[s]
        if G is not None:
            g, v = np.asarray(G, dtype='d').reshape(-1, 3)[s], np.asarray(u).astype('D')
            d[s] -= g[0] * v[0] + g[1] * v[1] + g[2] * v[2]
    return d


def size_modes(F, th, kx, ky, kz, kappa, G=None, u=None):
    """S = sum_c |k_c| |F_c| + kappa |k|^2 |theta| + sum_c |G_c| |u_c| per mode and scalar: what the rounding of the right-hand
    side scales with; arguments as for rhs_modes"""
    F, th = np.abs(np.asarray(F).astype('D')), np.abs(np.asarray(th).astype('D'))
    ax, ay, az = np.abs(kx), np.abs(ky), np.abs(kz)
    kk = ax * ax + ay * ay + az * az
    kappa = np.asarray(kappa, dtype='d').reshape(-1)
    out = np.empty(th.shape)
    for s in range(th.shape[0]):
        out[s] = ax * F[s, 0] + ay * F[s, 1] + az * F[s, 2] + kappa[s] * kk * th[s]
        if G is not None:
            g, v = np.abs(np.asarray(G, dtype='d').reshape(-1, 3)[s]), np.abs(np.asarray(u).astype('D'))
            out[s] += g[0] * v[0] + g[1] * v[1] + g[2] * v[2]
    return out


def rhs(flux_hat, theta_hat, k, kappa, G=None, u_hat=None, keep=None):
    """rhs_modes on a block: flux_hat [m][3] + block, theta_hat [m] + block, u_hat [3] + block, k the per-axis wavenumbers of
    the block; +0 where `keep` (bool over the block) is false"""
    d = rhs_modes(flux_hat, theta_hat, *_mesh(k), kappa, G, u_hat)
    return d if keep is None else np.where(keep[None], d, 0)


def size(flux_hat, theta_hat, k, kappa, G=None, u_hat=None):
    """size_modes on a block"""
    return size_modes(flux_hat, theta_hat, *_mesh(k), kappa, G, u_hat)


def advect(u_hat, theta_hat, shape):
    """The chain of the solver on the grid `shape` itself: flux_hat[s][c] = forward-normalised rfftn of u_c theta_s with
    u = irfftn(u_hat), theta = irfftn(theta_hat).  u_hat [3] + spectral shape, theta_hat [m] + spectral shape"""
    npts = float(np.prod(shape))
    back = lambda a: np.fft.irfftn(np.asarray(a).astype('D'), s=shape, axes=(0, 1, 2)) * npts
    u, th = np.array([back(a) for a in u_hat]), np.array([back(a) for a in theta_hat])
    f = flux(u, th)
    return np.array([[np.fft.rfftn(c) for c in fs] for fs in f]) / npts


def exact_advect(u_hat, theta_hat, shape):
    """(u theta)^ without aliasing errors: evaluated on the grid 2 * shape, which holds every sum of two wavenumbers of `shape`,
    and restricted to the modes of `shape` (for fields with nothing in their Nyquist planes -- any truncated ones)."""
    big = tuple(2 * n for n in shape)
    at = D._places(shape, big)

    def up(a):
        b = np.zeros((len(a), big[0], big[1], big[2] // 2 + 1), dtype='D')
        b[at] = np.asarray(a).astype('D')
        return b
    f = advect(up(u_hat), up(theta_hat), big)
    return np.array([fs[at] for fs in f])


def solenoidal(u_hat, k):
    """u_hat minus its component along k (k = 0 left alone)"""
    k0, k1, k2 = _mesh(k)
    kk = k0 * k0 + k1 * k1 + k2 * k2
    p = (k0 * u_hat[0] + k1 * u_hat[1] + k2 * u_hat[2]) / np.where(kk == 0, 1, kk)
    return np.array([u_hat[0] - k0 * p, u_hat[1] - k1 * p, u_hat[2] - k2 * p])


def eigenvalue(c, kappa, k):
    """lambda = -i c.k - kappa |k|^2 of uniform advection by the constant velocity c, per mode of the block"""
    k0, k1, k2 = _mesh(k)
    return -1j * (c[0] * k0 + c[1] * k1 + c[2] * k2) - kappa * (k0 * k0 + k1 * k1 + k2 * k2)


def rk4_factor(z):
    """R(z) of one classical Runge-Kutta step on dy/dt = lambda y, z = lambda h"""
    return 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24


RK_A, RK_B = (1. / 6., 1. / 3., 1. / 3., 1. / 6.), (0.5, 0.5, 1.)


def rk4(theta_hat, f, h, n):
    """n classical Runge-Kutta steps of size h on d theta_hat / dt = f(theta_hat), in the order of the solver's stages"""
    t = np.array(theta_hat)
    for _ in range(n):
        t0, t1 = t.copy(), t.copy()
        for rk in range(4):
            d = f(t)
            if rk < 3:
                t = t0 + RK_B[rk] * h * d
            t1 = t1 + RK_A[rk] * h * d
        t = t1
    return t


def uniform(c, shape, dtype='D'):
    """u_hat of the constant velocity c: [3] + spectral shape, c in the mode k = 0"""
    u = np.zeros((3,) + tuple(shape[:2]) + (shape[2] // 2 + 1,), dtype=dtype)
    u[:, 0, 0, 0] = c
    return u

