"""Host logic of the integrating-factor Runge-Kutta stage (no GPU): the reference scheme of tests/ifrk_ref.py itself (nu = 0 is
classical RK4, the linear closed form, the order), the package's table, the argument checks of gfft_ps_rk_stage_if and the
argument forms of `SpectralOps.rk_stage_if` over a numpy stand-in for the kernel."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import cases, ifrk_ref as I, scalar_ref as C, spectrum_ref as R
from tests.test_forcing_host import ForcingEngine, _h
from tests.test_scalar_host import UNIFORM, ScalarEngine, uniform_bound, uniform_case

EPS = 2.0 ** -52


def test_nu_zero_is_classical_rk4():
    """lambda = 0: every power of E is 1 and the four stages are the textbook step"""
    rng = np.random.default_rng(3)
    u = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    N = lambda v: (0.3 - 0.8j) * v + 0.25 * v * v
    a, b = u.copy(), u.copy()
    for _ in range(5):
        a, b = I.step(a, N, 0.0, 0.05), I.rk4_step(b, N, 0.05)
    err = float(np.abs(a - b).max() / np.abs(b).max())
    print('IFRK4 with lambda = 0 against textbook RK4 after 5 steps: %.2e' % err)
    assert err <= 32 * EPS


@pytest.mark.parametrize('lam_h', [0.0, 0.5, 2.785, 10.0, 50.0])
def test_linear_closed_form(lam_h):
    """du/dt = -lambda u + mu u: n steps give (R(mu h) exp(-lambda h))^n u_0 -- the decay exact, RK4 on the rest -- also at
    lambda h = 50, where explicit RK4 on the whole right-hand side has |R| = 2.4e5 per step.  Relative bound: per step the
    factor carries exp (1 ulp, its argument's rounding amplified by lambda h / 2 ... lambda h: <= 52 eps at 50), E * E and a
    dozen operations: n (2 lambda h + 24) eps."""
    h, n = 0.1, 5
    lam = lam_h / h
    mu = np.array([0.0, -1.5, 2.0j, -0.7 + 3.1j, 0.9 - 0.4j])
    u0 = np.array([1.0, -2.0 + 1.0j, 0.5j, 3.0, 1.0 - 1.0j])
    got = I.steps(u0, lambda v: mu * v, lam, h, n)
    want = (I.rk4_factor(mu * h) * np.exp(-lam * h)) ** n * u0
    err = float((np.abs(got - want) / np.abs(want)).max())
    print('lambda h = %g: relative error against the closed form after %d steps %.2e' % (lam_h, n, err))
    assert err <= n * (2 * lam_h + 24) * EPS, (lam_h, err)
    if lam_h > 2.785:
        assert abs(I.rk4_factor(-lam_h)) > 1, 'explicit RK4 would be stable here'


def test_order_is_four():
    """du/dt = -2 u + u^2, u(0) = 1/2: w = 1 / u obeys w' = 2 w - 1, so u(t) = 2 / (1 + 3 exp(2 t)).  The error at t = 1 with
    10 / 20 / 40 steps is 2.2e-8 / 1.5e-9 / 9.4e-11: it falls by about 16 per halving of h.  (u(0) = 1 is a poor probe: the
    leading error term nearly cancels there and the ratios read 25.)"""
    exact = 2.0 / (1.0 + 3.0 * math.exp(2.0))
    err = [abs(complex(I.steps(np.array([0.5]), lambda v: v * v, 2.0, 1.0 / n, n)[0]) - exact) for n in (10, 20, 40)]
    print('errors at 10 / 20 / 40 steps: %.2e %.2e %.2e, ratios %.2f %.2f' % (err[0], err[1], err[2], err[0] / err[1], err[1] / err[2]))
    for a, b in zip(err, err[1:]):
        assert 12 <= a / b <= 20, err


def test_package_table_is_the_reference_table():
    from mpi4py_fft_amd import spectral
    assert len(spectral.IFRK4) == len(I.TABLE) == 4
    for row, ref in zip(spectral.IFRK4, I.TABLE):
        assert len(row) == 6
        for got, want in zip(row, ref):
            assert want is None or got == want, (row, ref)
    assert all(isinstance(q, int) and 0 <= q <= 2 for row in spectral.IFRK4 for q in row[2:])
    # the package's rows drive the reference's stage to the reference's step (the last row with u = None)
    rng = np.random.default_rng(5)
    u = rng.standard_normal(16) + 1j * rng.standard_normal(16)
    lam, h, N = np.linspace(0, 40, 16), 0.1, (lambda v: (0.2 + 1j) * v - 0.1 * v * v)
    v, u0, u1 = u.copy(), u.copy(), u.copy()
    for rk, (cb, ca, q0, qd, q1, qa) in enumerate(spectral.IFRK4):
        new, u1 = I.stage(u0, u1, N(v), lam, h, cb, ca, q0, qd, q1, qa, with_u=rk < 3)
        v = new if rk < 3 else v
    assert np.array_equal(u1, I.step(u, N, lam, h))


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    assert 'gfft_ps_rk_stage_if' in _lib.EXPORTS and hasattr(lib, 'gfft_ps_rk_stage_if')
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = math.nan, math.inf
    dbl = lambda v: None if v is None else (ctypes.c_double * len(v))(*v)

    def stage(u=p, u0=p, u1=p, du=p, nc=3, nu=(0.03, 0.03, 0.03), k=(p, p, p), n=(2, 2, 2), cb=0.5, ca=1.0 / 6.0, q=(1, 1, 2, 2), h=0.01,
              dt=None, prec=8):
        return lib.gfft_ps_rk_stage_if(u, u0, u1, du, nc, dbl(nu), k[0], k[1], k[2], n[0], n[1], n[2], cb, ca, q[0], q[1], q[2], q[3],
                                       h, dt, prec, None)
    invalid = (dict(u1=None), dict(du=None), dict(nu=None), dict(k=(None, p, p)), dict(k=(p, None, p)), dict(k=(p, p, None)),
               dict(u0=None),                                                        # d_u without d_u0
               dict(nc=0), dict(nc=-1), dict(n=(-1, 2, 2)), dict(n=(2, -1, 2)), dict(n=(2, 2, -1)),
               dict(q=(3, 1, 2, 2)), dict(q=(1, -1, 2, 2)), dict(q=(1, 1, 3, 2)), dict(q=(1, 1, 2, -1)), dict(q=(1, 1, 2, 1 << 20)),
               dict(h=nan), dict(h=inf), dict(h=-inf), dict(prec=3), dict(prec=16))
    for bad in invalid:
        assert stage(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_rk_stage_if: bad argument', bad
    for nu in ((0.03, -0.1, 0.03), (nan, 0.03, 0.03), (0.03, 0.03, inf), (-1e-300, 0.0, 0.0)):
        assert stage(nu=nu) == -1, nu
        assert lib.gfft_last_error() == b'gfft_ps_rk_stage_if: nu must be finite and >= 0', nu
    assert stage(nc=5, nu=(0.1,) * 5) == -2 and lib.gfft_last_error() == b'gfft_ps_rk_stage_if: more than 4 components'
    assert stage(nc=5, nu=(0.1,) * 5, h=nan) == -1 and stage(nc=5, nu=None) == -1      # a bad argument beside it is still one
    for n in ((2, (1 << 30) + 1, 2), (2, 2, (1 << 30) + 1)):
        assert stage(n=n) == -2 and lib.gfft_last_error() == b'gfft_ps_rk_stage_if: axis longer than 2^30', n
        assert stage(n=n, h=nan) == -1 and stage(n=n, nu=(0.03, -0.1, 0.03)) == -1
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device
        assert stage() == -3 and stage(prec=4, nc=1, nu=(0.0,)) == -3 and stage(nc=4, nu=(0.0, 0.1, 0.2, 0.3)) == -3
        assert stage(u=None) == -3 and stage(u=None, u0=None, q=(0, 0, 0, 0)) == -3
        assert stage(u=None, u0=None, q=(7, -3, 0, 0)) == -1                           # powers are checked even where unused
        assert stage(h=nan, dt=p) == -3 and stage(h=-0.01) == -3                       # d_dt given: h is not looked at
        assert stage(q=(0, 0, 0, 0)) == -3 and stage(q=(2, 2, 2, 2)) == -3 and stage(n=(0, 2, 2)) == -3
        assert stage(n=(5, 1 << 30, 1 << 30)) == -3                                   # 2^30 itself is allowed


class IfrkEngine(ScalarEngine):
    """ScalarEngine plus gfft_ps_rk_stage_if restated with numpy (tests/ifrk_ref.py) on host tensors"""

    def ps_rk_stage_if(self, tu, tu0, tu1, tdu, ncomp, nu, k, shape, cb, ca, powers, h, tdt, precision):
        ForcingEngine.log.append(('ps_rk_stage_if', int(ncomp), tuple(float(x) for x in nu), float(cb), float(ca), tuple(powers),
                                  float(h), tdt, tu is None, tu0 is None))
        step = float(h) if tdt is None else float(tdt.reshape(-1)[0])
        blk = (ncomp,) + tuple(shape)
        lam = I.lam_of(nu, [_h(ki).astype('d') for ki in k])
        u, u1 = I.stage(None if tu is None else _h(tu0).reshape(blk), _h(tu1).reshape(blk), _h(tdu).reshape(blk), lam, step, cb, ca,
                        *powers, with_u=tu is not None)
        if tu is not None:
            tu.copy_(torch.as_tensor(u.reshape(tuple(tu.shape)).astype(_h(tu).dtype)))
        tu1.copy_(torch.as_tensor(u1.reshape(tuple(tu1.shape)).astype(_h(tu1).dtype)))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(IfrkEngine())
    ForcingEngine.log = []
    yield
    _lib.set_engine(old)


def _cfield(shape, m, seed):
    gs = (m,) + tuple(shape[:2]) + (shape[2] // 2 + 1,)
    rng = np.random.default_rng(seed)
    return rng.standard_normal(gs) + 1j * rng.standard_normal(gs)


def test_rk_stage_if_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape = (8, 6, 20)
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    k, _ = R.wavenumbers(shape, True)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    u0_h, u1_h, du_h = _cfield(shape, 3, 11), _cfield(shape, 3, 12), _cfield(shape, 3, 13)
    h = 0.05
    row = spectral.IFRK4[0]

    def run(u0, u1, du, nu, cb, ca, powers, with_u=True, **kw):
        tu = torch.full(T(u1).shape, np.nan + 0j, dtype=torch.complex128) if with_u else None
        t0, t1, td = T(u0), T(u1).clone(), T(du)
        ForcingEngine.log = []
        assert ops.rk_stage_if(tu, t0 if with_u else None, t1, td, nu, cb, ca, powers, **kw) is t1
        assert len(ForcingEngine.log) == 1 and ForcingEngine.log[0][0] == 'ps_rk_stage_if'
        assert np.array_equal(_h(t0), u0) and np.array_equal(_h(td), du), 'an input was modified'
        return (None if tu is None else _h(tu).copy()), _h(t1).copy(), ForcingEngine.log[0]
    # [m] fields, nu a float (shared) and a sequence; h a float
    u, u1, call = run(u0_h, u1_h, du_h, 0.03, row[0], row[1], row[2:], h=h)
    assert call[1:7] == (3, (0.03,) * 3, 0.5, 1. / 6., (1, 1, 2, 2), h) and call[7] is None and call[8:] == (False, False)
    ref_u, ref_1 = I.stage(u0_h, u1_h, du_h, I.lam_of([0.03] * 3, k), h, *row)
    assert np.array_equal(u, ref_u) and np.array_equal(u1, ref_1)
    nus = [0.03, 0.0, 0.2]
    for form in (nus, tuple(nus), np.array(nus)):
        u, u1, call = run(u0_h, u1_h, du_h, form, *spectral.IFRK4[2][:2], spectral.IFRK4[2][2:], h=h)
        assert call[2] == tuple(nus)
        ref_u, ref_1 = I.stage(u0_h, u1_h, du_h, I.lam_of(nus, k), h, *spectral.IFRK4[2])
        assert np.array_equal(u, ref_u) and np.array_equal(u1, ref_1)
    assert np.array_equal(u1[1], u1_h[1] + (h / 3) * du_h[1])                    # nu = 0: the plain stage
    # a scalar field in the scalar form; the last row with u = None (u0 None too)
    u, u1, call = run(u0_h[0], u1_h[0], du_h[0], 0.2, *spectral.IFRK4[1][:2], spectral.IFRK4[1][2:], h=h)
    assert call[1:3] == (1, (0.2,)) and u.shape == ops.shape
    assert np.array_equal(u1, I.stage(u0_h[:1], u1_h[:1], du_h[:1], I.lam_of([0.2], k), h, *spectral.IFRK4[1])[1][0])
    last = spectral.IFRK4[3]
    u, u1, call = run(u0_h, u1_h, du_h, nus, last[0], last[1], last[2:], with_u=False, h=h)
    assert u is None and call[8:] == (True, True) and call[5] == (0, 0, 0, 0)
    assert np.array_equal(u1, u1_h + (h / 6) * du_h)
    # dt: a tensor holding the step (element 0 is read); DistArray fields
    tdt = torch.tensor([h, 123.0], dtype=torch.float64)
    u, u1b, call = run(u0_h, u1_h, du_h, nus, row[0], row[1], row[2:], dt=tdt)
    assert call[7] is tdt and call[6] == 0.0
    assert np.array_equal(u1b, run(u0_h, u1_h, du_h, nus, row[0], row[1], row[2:], h=h)[1])
    A, B, Cc, D = (newDistArray(fft, rank=1) for _ in range(4))
    B[...], Cc[...], D[...] = u0_h, u1_h, du_h
    assert ops.rk_stage_if(A, B, Cc, D, 0.03, row[0], row[1], row[2:], h=h) is Cc
    assert np.array_equal(np.asarray(A), I.stage(u0_h, u1_h, du_h, I.lam_of([0.03] * 3, k), h, *row)[0])
    # refusals: nothing reaches the engine
    ForcingEngine.log = []
    z3 = lambda: torch.zeros((3,) + ops.shape, dtype=torch.complex128)
    z5 = lambda: torch.zeros((5,) + ops.shape, dtype=torch.complex128)
    q = (1, 1, 2, 2)
    for bad in (lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), 0.03, 0.5, 0.1, q),                       # neither h nor dt
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), 0.03, 0.5, 0.1, q, h=h, dt=tdt),          # both
                lambda: ops.rk_stage_if(z3(), None, z3(), z3(), 0.03, 0.5, 0.1, q, h=h),                  # u without u0
                lambda: ops.rk_stage_if(z5(), z5(), z5(), z5(), 0.03, 0.5, 0.1, q, h=h),                  # m = 5
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), [0.03, 0.1], 0.5, 0.1, q, h=h),           # two nu for three components
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), -0.03, 0.5, 0.1, q, h=h),
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), [0.03, math.nan, 0.1], 0.5, 0.1, q, h=h),
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), math.inf, 0.5, 0.1, q, h=h),
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), 0.03, 0.5, 0.1, (1, 1, 2), h=h),          # three powers
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), 0.03, 0.5, 0.1, (1, 1, 3, 2), h=h),
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), 0.03, 0.5, 0.1, (1, -1, 2, 2), h=h),
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), 0.03, 0.5, 0.1, (1, 0.5, 2, 2), h=h),
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), 0.03, 0.5, 0.1, q, h=math.nan),
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), 0.03, 0.5, 0.1, q, h=math.inf),
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), 0.03, 0.5, 0.1, q, dt=tdt.float()),       # dt is a double tensor
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3(), 0.03, 0.5, 0.1, q, dt=torch.zeros(0, dtype=torch.float64)),
                lambda: ops.rk_stage_if(z3()[:2], z3(), z3(), z3(), 0.03, 0.5, 0.1, q, h=h),              # u of another m
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3()[:2], 0.03, 0.5, 0.1, q, h=h),
                lambda: ops.rk_stage_if(z3(), z3(), z3()[0], z3(), 0.03, 0.5, 0.1, q, h=h),               # scalar form beside [m]
                lambda: ops.rk_stage_if(z3(), z3(), z3(), z3().to(torch.complex64), 0.03, 0.5, 0.1, q, h=h),   # mixed precision
                lambda: ops.rk_stage_if(z3().to(torch.complex64), z3(), z3(), z3(), 0.03, 0.5, 0.1, q, h=h),
                lambda: ops.rk_stage_if(z3(), z3(), z3().real, z3().real, 0.03, 0.5, 0.1, q, h=h),        # real fields
                lambda: ops.rk_stage_if(z3(), z3(), z3()[:, :, :, ::2], z3()[:, :, :, ::2], 0.03, 0.5, 0.1, q, h=h)):      # strided views
        with pytest.raises((AssertionError, ValueError, TypeError)):
            bad()
    assert ForcingEngine.log == [], 'a refused call reached the engine'
    fft.destroy()


def ifrk_uniform_case(shape, kappa, dtype='D'):
    """(theta_0, keep, (R(-i k.U h) exp(-kappa |k|^2 h))^n per mode, max advective |k.U| h over kept modes, max kappa |k|^2 h
    over kept modes) of uniform advection under IFRK4: the diffusion exact, RK4 on the advection alone"""
    th0, keep, _, _ = uniform_case(shape, dtype)
    k, _ = R.wavenumbers(shape, True)
    h, n = UNIFORM['h'], UNIFORM['n']
    za = C.eigenvalue(UNIFORM['c'], 0.0, k) * h                          # -i k.U h
    lam_h = kappa * I.kk_of(k) * h
    return th0, keep, (I.rk4_factor(za) * np.exp(-lam_h)) ** n, float(np.abs(za[keep]).max()), float(lam_h[keep].max())


def stiff_kappa(shape):
    """A diffusivity at which kappa k_max^2 h > 3 over the kept modes of the uniform case: beyond explicit RK4's 2.785"""
    k, _ = R.wavenumbers(shape, True)
    keep = uniform_case(shape)[1]
    return 3.5 / (float(I.kk_of(k)[keep].max()) * UNIFORM['h'])


@pytest.mark.parametrize('stiff', [False, True], ids=['kappa', 'stiff'])
@pytest.mark.parametrize('shape', [(24, 16, 20), (12, 10, 21)], ids=str)
def test_uniform_advection_closed_form_with_the_integrating_factor(shape, stiff):
    """The numpy chain alone (advect, rhs with kappa = 0 and the 2/3 mask, IFRK4 stages with kappa) stays within
    uniform_bound with zmax the advective |k.U| h: the bound the device chain is held to in test_gpu_ifrk."""
    kappa = stiff_kappa(shape) if stiff else UNIFORM['kappa']
    th0, keep, Rn, zmax, lmax = ifrk_uniform_case(shape, kappa)
    assert (lmax > 3) == stiff and zmax < 0.5
    k, _ = R.wavenumbers(shape, True)
    uh = C.uniform(UNIFORM['c'], shape)
    N = lambda t: C.rhs(C.advect(uh, t, shape), t, k, [0.0], keep=keep)
    got = I.steps(th0, N, I.lam_of([kappa], k), UNIFORM['h'], UNIFORM['n'])
    err = float(np.abs(got - Rn * th0).max() / np.abs(th0).max())
    bound = uniform_bound('d', shape, zmax)
    print('%s kappa = %.4g: max |k.U| h = %.3f, max kappa |k|^2 h = %.3f, numpy IFRK4 chain against the closed form %.2e (bound %.2e)'
          % (shape, kappa, zmax, lmax, err, bound))
    assert err <= bound, (err, bound)
    assert np.all(got[:, ~keep] == 0)
    if stiff:                                            # explicit RK4 on the same problem amplifies the stiffest kept mode
        z = C.eigenvalue(UNIFORM['c'], kappa, k) * UNIFORM['h']
        assert np.abs(C.rk4_factor(z)[keep]).max() > 1
