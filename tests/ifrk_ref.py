"""Reference for the integrating-factor Runge-Kutta stage (TEST INFRASTRUCTURE): numpy in float64, the formulas of
include/gfft.h (gfft_ps_rk_stage_if), written without the package.

    du/dt = -lambda u + N(u),  lambda >= 0 real (nu |k|^2)

With v = exp(lambda t) u the linear term disappears: dv/dt = exp(lambda t) N(exp(-lambda t) v), and classical RK4 on v,
written for u itself with E = exp(-lambda h / 2), is four stages of one form,

    u  = E^q0 u0 + cb h E^qd d        (not formed in the last stage)
    u1 = E^q1 u1 + ca h E^qa d        d = N(u)

with u0 = u1 = u_n before the first stage (TABLE below); u1 is u_{n+1} after the fourth.  Derivation: the classical
slopes are k1 = N(u_n), k2 = N(E u_n + h/2 E k1), k3 = N(E u_n + h/2 k2), k4 = N(E^2 u_n + h E k3) -- the arguments are the
stage values u -- and u_{n+1} = E^2 u_n + h/6 (E^2 k1 + 2 E k2 + 2 E k3 + k4), accumulated in u1; u0 holds u_n throughout.

For N(u) = mu u every step multiplies u by R(mu h) exp(-lambda h), R the stability polynomial of RK4: the closed form the
tests compare with.
"""
import numpy as np

# (cb, ca, q0, qd, q1, qa); None: not used by that stage
TABLE = ((1. / 2., 1. / 6., 1, 1, 2, 2),
         (1. / 2., 1. / 3., 1, 0, 0, 1),
         (1., 1. / 3., 2, 1, 0, 1),
         (None, 1. / 6., None, None, 0, 0))


def factor(lam, h):
    """E = exp(-lambda h / 2)"""
    return np.exp(-(np.asarray(lam, dtype='d') * (0.5 * h)))


def _pow(E, q):
    return np.ones_like(E) if q == 0 else E if q == 1 else E * E


def stage(u0, u1, d, lam, h, cb, ca, q0, qd, q1, qa, with_u=True):
    """One stage in float64 (complex128): returns (u or None, new u1); the inputs are not modified.  lam broadcasts
    against the fields."""
    E = factor(lam, h)
    d, u1 = np.asarray(d).astype('D'), np.asarray(u1).astype('D')
    u = None
    if with_u:
        u = _pow(E, q0) * np.asarray(u0).astype('D') + (cb * h) * _pow(E, qd) * d
    return u, _pow(E, q1) * u1 + (ca * h) * _pow(E, qa) * d


def step(u, N, lam, h):
    """One IFRK4 step of size h on du/dt = -lam u + N(u)"""
    u = np.asarray(u).astype('D')
    u0, u1 = u.copy(), u.copy()
    for cb, ca, q0, qd, q1, qa in TABLE:
        last = cb is None
        new, u1 = stage(u0, u1, N(u), lam, h, cb, ca, q0, qd, q1, qa, with_u=not last)
        if not last:
            u = new
    return u1


def steps(u, N, lam, h, n):
    for _ in range(n):
        u = step(u, N, lam, h)
    return u


def rk4_step(u, f, h):
    """One classical RK4 step on du/dt = f(u), in the textbook form"""
    k1 = f(u)
    k2 = f(u + 0.5 * h * k1)
    k3 = f(u + 0.5 * h * k2)
    k4 = f(u + h * k3)
    return u + (h / 6.) * (k1 + 2 * k2 + 2 * k3 + k4)


def rk4_factor(z):
    """R(z) of one classical Runge-Kutta step on dy/dt = mu y, z = mu h"""
    return 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24


def kk_of(k):
    """|k|^2 over a block from its three per-axis wavenumber vectors"""
    return k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2 + k[2][None, None, :] ** 2


def lam_of(nu, k):
    """lambda[c] = nu[c] |k|^2: [m] + block"""
    return np.asarray(nu, dtype='d').reshape(-1, 1, 1, 1) * kk_of(k)[None]


def bound(lam, h, u0, u1, d, cb, eps):
    """The per-mode error allowed to a stage in a precision of machine epsilon eps: (8 x + 12) eps (|u0| + |u1| + |cb h d|),
    x = lambda h / 2 -- four roundings in the argument of exp, each amplified by x (and doubled in E * E); exp itself
    within 2 ulp, E * E, the products and the multiply-adds; 4 eps for this float64 reference where eps is float64's."""
    x = np.asarray(lam, dtype='d') * (0.5 * h)
    size = np.abs(u1) + (0 if u0 is None else np.abs(u0)) + np.abs((cb or 0.0) * h * d)
    return (8 * x + 12) * eps * size
