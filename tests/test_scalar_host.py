"""Host logic of the passive-scalar transport (no GPU): the argument forms of `spectral.scalar_flux` and
`SpectralOps.scalar_rhs` over numpy stand-ins for the kernels, the argument checks of gfft_ps_scalar_flux and
gfft_ps_scalar_rhs, and the reference itself: the flux chain of 2/3-truncated fields is alias-free (the loose rule is
not), it conserves the mean and the variance, and uniform advection follows its closed form."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import cases, dealias_ref as D, scalar_ref as C, spectrum_ref as R
from tests.test_dealias_host import DealiasEngine
from tests.test_forcing_host import ForcingEngine, _field, _h


class ScalarEngine(DealiasEngine):
    """DealiasEngine plus the two scalar entries restated with numpy (tests/scalar_ref.py) on host tensors"""

    def ps_scalar_flux(self, tu, ttheta, tflux, nscalar, count, precision):
        ForcingEngine.log.append(('ps_scalar_flux', int(nscalar), int(count), precision))
        out = C.flux(_h(tu).reshape(3, count), _h(ttheta).reshape(nscalar, count))
        tflux.copy_(torch.as_tensor(out.reshape(tuple(tflux.shape))))

    def ps_scalar_rhs(self, tdtheta, tflux, ttheta, tu, nscalar, kappa, grad, k, m, shape, kcut, precision):
        ForcingEngine.log.append(('ps_scalar_rhs', int(nscalar), tuple(float(x) for x in kappa),
                                  None if grad is None else tuple(tuple(float(x) for x in g) for g in grad), float(kcut), tuple(m), tu))
        kd = [_h(ki).astype('d') for ki in k]
        blk = tuple(shape)
        out = C.rhs(_h(tflux).reshape((nscalar, 3) + blk), _h(ttheta).reshape((nscalar,) + blk), kd, kappa, grad,
                    None if grad is None else _h(tu), self._keep(k, m, kcut))
        tdtheta.copy_(torch.as_tensor(out.reshape(tuple(tdtheta.shape)).astype(_h(tdtheta).dtype)))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(ScalarEngine())
    ForcingEngine.log = []
    yield
    _lib.set_engine(old)


def _cfield(shape, m, seed):
    gs = (m,) + tuple(shape[:2]) + (shape[2] // 2 + 1,)
    rng = np.random.default_rng(seed)
    return rng.standard_normal(gs) + 1j * rng.standard_normal(gs)


def test_scalar_flux_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape = (8, 6, 20)
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    rng = np.random.default_rng(7)
    u_h, th_h = rng.standard_normal((3,) + shape), rng.standard_normal((3,) + shape)
    U = newDistArray(fft, False, rank=1)
    U[...] = u_h
    count = int(np.prod(shape))
    # one scalar: the physical shape itself, out [3] + shape; a DistArray velocity and a DistArray output
    one, out1 = torch.as_tensor(th_h[1].copy()), newDistArray(fft, False, rank=1)
    assert spectral.scalar_flux(U, one, out1) is out1
    assert ForcingEngine.log[-1] == ('ps_scalar_flux', 1, count, 8)
    assert np.array_equal(np.asarray(out1), u_h * th_h[1])
    # [m] + shape, m = 1 ... 4, out [m][3] + shape
    for m in (1, 2, 3, 4):
        th = np.concatenate([th_h, th_h[:1] * 2])[:m]
        out = torch.zeros((m, 3) + shape, dtype=torch.float64)
        assert spectral.scalar_flux(U, torch.as_tensor(th.copy()), out) is out
        assert ForcingEngine.log[-1] == ('ps_scalar_flux', m, count, 8)
        assert np.array_equal(_h(out), C.flux(u_h, th))
    # raw tensors of any physical shape, fp32
    u32, t32, o32 = torch.as_tensor(u_h.reshape(3, -1).astype('f')), torch.as_tensor(th_h[:2].reshape(2, -1).astype('f')), torch.zeros((2, 3, count), dtype=torch.float32)
    spectral.scalar_flux(u32, t32, o32)
    assert ForcingEngine.log[-1] == ('ps_scalar_flux', 2, count, 4) and o32.dtype == torch.float32
    assert np.array_equal(_h(o32), C.flux(_h(u32), _h(t32)))
    n = len(ForcingEngine.log)
    u = torch.as_tensor(u_h.copy())
    t5 = torch.zeros((5,) + shape, dtype=torch.float64)
    for bad in ((u, t5, torch.zeros((5, 3) + shape, dtype=torch.float64)),                       # m = 5
                (u, one, torch.zeros((1, 3) + shape, dtype=torch.float64)),                      # scalar form with [1][3] out
                (u, t5[:2], torch.zeros((3, 2) + shape, dtype=torch.float64)),                   # [3][m] instead of [m][3]
                (u[:2], one, torch.zeros((3,) + shape, dtype=torch.float64)),                    # two velocity components
                (u, one.float(), torch.zeros((3,) + shape, dtype=torch.float64)),                # mixed precision
                (u, one, torch.zeros((3,) + shape, dtype=torch.float32)),
                (u, one[:, :, ::2], torch.zeros((3,) + shape[:2] + (10,), dtype=torch.float64)),  # a strided view
                (u.transpose(1, 2), one.transpose(0, 1), torch.zeros((3, 6, 8, 20), dtype=torch.float64))):
        with pytest.raises(AssertionError):
            spectral.scalar_flux(*bad)
    assert len(ForcingEngine.log) == n, 'a refused call reached the engine'
    fft.destroy()


def test_scalar_rhs_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape = (8, 6, 20)
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    k, _ = R.wavenumbers(shape, True)
    uh_h, th_h, f_h = _field(shape, 5), _cfield(shape, 3, 8), _cfield(shape, 9, 9).reshape((3, 3) + ops.shape)
    uh = newDistArray(fft, rank=1)
    uh[...] = uh_h
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))

    def run(th, f, kappa, *a, **kw):
        d = torch.full(th.shape, np.nan + 0j, dtype=torch.complex128)
        ForcingEngine.log = []
        assert ops.scalar_rhs(d, T(f), T(th), kappa, *a, **kw) is d
        assert len(ForcingEngine.log) == 1 and ForcingEngine.log[0][0] == 'ps_scalar_rhs'
        return _h(d).copy(), ForcingEngine.log[0]
    # one scalar in the scalar form: the spectral shape and [3] + spectral shape; kappa a float
    got, call = run(th_h[0], f_h[0], 0.03)
    assert call[1:5] == (1, (0.03,), None, math.inf) and call[5] == (None, None, None) and call[6] is None
    assert got.shape == ops.shape and np.array_equal(got, C.rhs(f_h[:1], th_h[:1], k, [0.03])[0])
    # [m] fields; kappa a float (shared) and a list
    got, call = run(th_h, f_h, 0.03)
    assert call[1:3] == (3, (0.03, 0.03, 0.03)) and np.array_equal(got, C.rhs(f_h, th_h, k, [0.03] * 3))
    kap = [0.03, 0.0, 0.2]
    got, call = run(th_h, f_h, kap)
    assert call[2] == tuple(kap) and np.array_equal(got, C.rhs(f_h, th_h, k, kap))
    assert np.array_equal(run(th_h[:1], f_h[:1], [0.2])[0], C.rhs(f_h[:1], th_h[:1], k, [0.2]))           # [1] + shape
    assert np.array_equal(run(th_h, f_h, np.array(kap))[0], got) and np.array_equal(run(th_h, f_h, tuple(kap))[0], got)
    # mean_gradient of shape 3 (shared) and m x 3; u_hat a DistArray or a tensor
    g3, g33 = (1.0, -0.5, 0.25), [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-2.0, 0.5, 0.125]]
    got, call = run(th_h, f_h, kap, g3, uh)
    assert call[3] == (g3,) * 3 and call[6] is uh.tensor
    assert np.array_equal(got, C.rhs(f_h, th_h, k, kap, [g3] * 3, uh_h))
    got, call = run(th_h, f_h, kap, mean_gradient=g33, u_hat=T(uh_h))
    assert call[3] == tuple(tuple(g) for g in g33) and np.array_equal(got, C.rhs(f_h, th_h, k, kap, g33, uh_h))
    assert not np.array_equal(got[0], C.rhs(f_h, th_h, k, kap)[0]) and np.array_equal(got[1], C.rhs(f_h, th_h, k, kap)[1])
    assert np.array_equal(run(th_h[0], f_h[0], 0.03, np.array(g3), uh)[0], C.rhs(f_h[:1], th_h[:1], k, [0.03], [g3], uh_h)[0])
    # u_hat without a mean gradient: passed on, with no gradient; the result is that without u_hat
    got, call = run(th_h, f_h, kap, None, uh)
    assert call[3] is None and np.array_equal(got, C.rhs(f_h, th_h, k, kap))
    # dealias forms: a dealias_mask, any 4-sequence, kcut None = inf, None vectors, bool vectors
    mask = ops.dealias_mask('2/3', kcut=2.5)
    keep = D.keep_mask(k, D.keep_vectors(shape), 2.5)
    assert keep.any() and not keep.all()
    got, call = run(th_h, f_h, kap, g33, uh, dealias=mask)
    assert call[4] == 2.5 and all(a is b for a, b in zip(call[5], mask[:3]))
    assert np.array_equal(got, C.rhs(f_h, th_h, k, kap, g33, uh_h, keep)) and np.all(got[:, ~keep] == 0)
    got, call = run(th_h, f_h, kap, dealias=(mask.m0, None, mask.m2, None))
    assert call[4] == math.inf and call[5][1] is None
    k1 = D.keep_mask(k, [_h(mask.m0), None, _h(mask.m2)])
    assert np.array_equal(got, C.rhs(f_h, th_h, k, kap, keep=k1))
    assert np.array_equal(run(th_h, f_h, kap, dealias=[mask.m0.bool(), None, mask.m2, math.inf])[0], got)
    assert np.array_equal(run(th_h, f_h, kap, dealias=ops.dealias_mask(None))[0], C.rhs(f_h, th_h, k, kap))
    assert run(th_h, f_h, kap, dealias=None)[1][4:6] == (math.inf, (None, None, None))
    # refusals: nothing reaches the engine
    ForcingEngine.log = []
    th5, f5 = np.concatenate([th_h, th_h[:2]]), np.concatenate([f_h, f_h[:2]])
    d3, d5 = torch.zeros(th_h.shape, dtype=torch.complex128), torch.zeros(th5.shape, dtype=torch.complex128)
    for bad in (lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), kap, g3),                               # a mean gradient without u_hat
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), kap, mean_gradient=g33),
                lambda: ops.scalar_rhs(d5, T(f5), T(th5), 0.03),                                    # m = 5
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), [0.03, 0.1]),                           # two kappa for three scalars
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), -0.03),
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), [0.03, math.nan, 0.1]),
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), math.inf),
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), kap, (1.0, 0.0), uh),                   # two gradient components
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), kap, g33[:2], uh),                      # 2 x 3 for three scalars
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), kap, (1.0, math.inf, 0.0), uh),
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), kap, g3, T(uh_h[:2])),                  # two velocity components
                lambda: ops.scalar_rhs(d3[:2], T(f_h), T(th_h), kap),                               # dtheta_hat of another m
                lambda: ops.scalar_rhs(d3, T(f_h[:2]), T(th_h), kap),
                lambda: ops.scalar_rhs(d3[0], T(f_h), T(th_h[0]), 0.03),                            # scalar form with an [m][3] flux
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h).to(torch.complex64), kap),               # mixed precision
                lambda: ops.scalar_rhs(d3, T(f_h).to(torch.complex64), T(th_h), kap),
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), kap, dealias=(mask.m0, mask.m1, mask.m2)),
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), kap, dealias=(mask.m0, mask.m1, mask.m2, -1.0)),
                lambda: ops.scalar_rhs(d3, T(f_h), T(th_h), kap, dealias='2/3')):
        with pytest.raises((AssertionError, ValueError, TypeError)):
            bad()
    assert ForcingEngine.log == [], 'a refused call reached the engine'
    fft.destroy()


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    for name in ('gfft_ps_scalar_flux', 'gfft_ps_scalar_rhs'):
        assert name in _lib.EXPORTS
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = math.nan, math.inf
    dbl = lambda v: None if v is None else (ctypes.c_double * len(v))(*v)

    def flux(u=p, th=p, f=p, ns=1, count=8, prec=8):
        return lib.gfft_ps_scalar_flux(u, th, f, ns, count, prec, None)
    for bad in (dict(u=None), dict(th=None), dict(f=None), dict(ns=0), dict(ns=-2), dict(count=-1), dict(prec=3), dict(prec=16)):
        assert flux(**bad) == -1, bad
    assert lib.gfft_last_error() == b'gfft_ps_scalar_flux: bad argument'
    assert flux(ns=5) == -2 and lib.gfft_last_error() == b'gfft_ps_scalar_flux: more than 4 scalars'
    assert flux(ns=5, count=-1) == -1 and flux(ns=64, u=None) == -1       # a bad argument beside it is still a bad argument

    def rhs(d=p, f=p, th=p, u=p, ns=2, kappa=(0.03, 0.1), grad=(1.0, 0.0, 0.0, 0.0, -0.5, 0.25), k=(p, p, p), m=(p, p, p), n=(2, 2, 2),
            kcut=2.5, prec=8):
        return lib.gfft_ps_scalar_rhs(d, f, th, u, ns, dbl(kappa), dbl(grad), k[0], k[1], k[2], m[0], m[1], m[2], n[0], n[1], n[2],
                                      kcut, prec, None)
    invalid = (dict(d=None), dict(f=None), dict(th=None), dict(k=(None, p, p)), dict(k=(p, None, p)), dict(k=(p, p, None)),
               dict(n=(-1, 2, 2)), dict(n=(2, -1, 2)), dict(n=(2, 2, -1)), dict(prec=3), dict(prec=16), dict(kcut=nan), dict(kcut=-1.0),
               dict(kcut=-inf), dict(kcut=-1e-300), dict(ns=0), dict(ns=-1), dict(kappa=None), dict(kappa=(0.03, nan)),
               dict(kappa=(inf, 0.1)), dict(kappa=(0.03, -0.1)), dict(kappa=(-1e-300, 0.1)), dict(u=None),          # grad without d_u_hat
               dict(grad=(1.0, 0.0, 0.0, 0.0, nan, 0.0)), dict(grad=(1.0, 0.0, 0.0, 0.0, 0.0, -inf)))
    for bad in invalid:
        assert rhs(**bad) == -1, bad
        assert rhs(m=(None, None, None), **dict(dict(kcut=inf), **bad)) == -1, bad
    four = dict(ns=4, kappa=(0.0, 0.1, 0.2, 0.3), grad=None, u=None)
    assert rhs(ns=5, kappa=(0.1,) * 5, grad=None) == -2 and lib.gfft_last_error() == b'gfft_ps_scalar_rhs: more than 4 scalars'
    assert rhs(ns=5, kappa=(0.1,) * 5, grad=None, kcut=nan) == -1 and rhs(ns=5, kappa=None, grad=None) == -1
    for n in ((2, (1 << 30) + 1, 2), (2, 2, (1 << 30) + 1)):
        assert rhs(n=n) == -2 and rhs(n=n, **four) == -2, n          # beyond the documented limit: unsupported, not invalid
        assert rhs(n=n, kcut=nan) == -1 and rhs(n=n, kappa=(0.03, -0.1)) == -1
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device
        assert flux() == -3 and flux(ns=4, prec=4, count=0) == -3
        assert rhs() == -3 and rhs(**four) == -3 and rhs(prec=4, kcut=inf, m=(None, None, None)) == -3
        assert rhs(grad=None) == -3 and rhs(grad=None, u=None) == -3 and rhs(kappa=(0.0, 0.0)) == -3
        assert rhs(ns=1, kappa=(0.5,), grad=(0.0, 0.0, 0.0)) == -3 and rhs(kcut=0.0, n=(0, 2, 2)) == -3
        assert rhs(n=(5, 1 << 30, 1 << 30)) == -3                    # 2^30 itself is allowed


SHAPES = [(24, 16, 20), (12, 10, 21), (9, 8, 6)]


def _spectral(shape, m, seed):
    rng = np.random.default_rng(seed)
    return np.array([np.fft.rfftn(a) for a in rng.standard_normal((m,) + shape)]) / np.prod(shape)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_flux_chain_is_alias_free_under_the_strict_rule_only(shape):
    """The reference alone.  Measured: strict 3e-16 ... 5e-16, loose 0.32 ... 0.66."""
    uh, th = _spectral(shape, 3, 23), _spectral(shape, 2, 29)
    k, _ = R.wavenumbers(shape, True)
    err = {}
    for rule in ('2/3', 'loose'):
        m = D.keep_mask(k, D.keep_vectors(shape, rule))
        got, exact = C.advect(uh * m, th * m, shape) * m, C.exact_advect(uh * m, th * m, shape) * m
        err[rule] = float(np.abs(got - exact).max() / np.abs(exact).max())
    print('%s: N-grid flux against the exact convolution, strict rule %.2e, loose rule %.2e' % (shape, err['2/3'], err['loose']))
    assert err['2/3'] <= 1e-14, err
    assert err['loose'] > 0.1, err


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_advection_conserves_mean_and_variance(shape):
    """Solenoidal truncated u, kappa = 0, no mean gradient: the variance transfer sum w Re(conj(theta_hat) d) vanishes against
    its Cauchy-Schwarz size (measured 1e-17 at (24, 16, 20)), and d[0, 0, 0] == 0."""
    k, w = R.wavenumbers(shape, True)
    keep = D.keep_mask(k, D.keep_vectors(shape))
    uh, th = C.solenoidal(_spectral(shape, 3, 31), k) * keep, _spectral(shape, 2, 37) * keep
    div = k[0][:, None, None] * uh[0] + k[1][None, :, None] * uh[1] + k[2][None, None, :] * uh[2]
    assert np.abs(div).max() <= 1e-15 * np.abs(uh).max() * max(np.abs(ki).max() for ki in k)
    d = C.rhs(C.advect(uh, th, shape), th, k, [0.0, 0.0], keep=keep)
    for s in range(2):
        transfer = float((w * (np.conj(th[s]) * d[s]).real).sum())
        scale = math.sqrt(float((w * np.abs(th[s]) ** 2).sum()) * float((w * np.abs(d[s]) ** 2).sum()))
        print('%s scalar %d: variance transfer %.2e of %.2e' % (shape, s, transfer, scale))
        assert scale > 0 and abs(transfer) <= 1e-14 * scale, (transfer, scale)
        assert d[s][0, 0, 0] == 0, 'the mean is not conserved'
    # (with diffusion the variance decays: the transfer is -2 kappa <|grad theta|^2> / 2 < 0)
    d = C.rhs(C.advect(uh, th, shape), th, k, [0.1, 0.1], keep=keep)
    assert float((w * (np.conj(th[0]) * d[0]).real).sum()) < 0


UNIFORM = dict(c=(0.7, -0.4, 0.55), kappa=0.03, h=0.02, n=5)


def uniform_case(shape, dtype='D'):
    """(theta_0, keep, R^n per mode, max |lambda h| over kept modes) of the closed-form case, theta_0 a 2/3-truncated random
    field in `dtype`"""
    k, _ = R.wavenumbers(shape, True)
    keep = D.keep_mask(k, D.keep_vectors(shape))
    th0 = (_spectral(shape, 1, 43) * keep).astype(dtype)
    z = C.eigenvalue(UNIFORM['c'], UNIFORM['kappa'], k) * UNIFORM['h']
    return th0, keep, C.rk4_factor(z) ** UNIFORM['n'], float(np.abs(z[keep]).max())


def uniform_bound(dt, shape, zmax):
    """n (max |lambda h| rounding_tol + 8 eps): each step's four evaluations carry one transform pair's rounding -- rounding_tol
    with its factor 2 -- scaled by h |lambda|, with weights summing to 1; the stage updates add a few eps; |R| <= 1 does not
    amplify."""
    return UNIFORM['n'] * (zmax * cases.rounding_tol(dt, int(np.prod(shape))) + 8 * cases.EPS[dt])


@pytest.mark.parametrize('shape', SHAPES[:2], ids=str)
def test_uniform_advection_closed_form(shape):
    """The numpy chain (advect, rhs with the 2/3 mask, RK4) against R(lambda h)^n theta_0; max |lambda h| = 0.19 at (24, 16, 20)."""
    th0, keep, Rn, zmax = uniform_case(shape)
    k, _ = R.wavenumbers(shape, True)
    uh = C.uniform(UNIFORM['c'], shape)
    assert zmax < 0.5 and np.abs(Rn[keep]).max() <= 1.0
    f = lambda t: C.rhs(C.advect(uh, t, shape), t, k, [UNIFORM['kappa']], keep=keep)
    got = C.rk4(th0, f, UNIFORM['h'], UNIFORM['n'])
    err = float(np.abs(got - Rn * th0).max() / np.abs(th0).max())
    bound = uniform_bound('d', shape, zmax)
    print('%s: max |lambda h| = %.3f, numpy chain against the closed form %.2e (bound %.2e)' % (shape, zmax, err, bound))
    assert err <= bound, (err, bound)
    assert np.all(got[:, ~keep] == 0)
