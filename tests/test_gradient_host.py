"""Host logic of the velocity-gradient diagnostics (no GPU): the argument forms and refusals of `SpectralOps.gradient` and
`SpectralOps.gradient_stats` over numpy stand-ins for the kernels, the rank reduction, the argument checks of gfft_ps_gradient
and gfft_ps_gradient_stats, the closed forms of `gradient_moments`, and the reference itself: on a solenoidal field truncated
by the strict 2/3 rule the Betchov identities hold to rounding, and with the Nyquist planes kept they do not."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import cases, gradient_ref as G, spectrum_ref as R
from tests.test_forcing_host import ForcingEngine, _h
from tests.test_scalar_host import ScalarEngine, _cfield


class GradientEngine(ScalarEngine):
    """ScalarEngine plus the two gradient entries restated with numpy (tests/gradient_ref.py) on host tensors"""

    def ps_gradient(self, tf, tout, ncomp, k, shape, precision):
        ForcingEngine.log.append(('ps_gradient', int(ncomp), tuple(shape), precision))
        out = G.grad(_h(tf).reshape((ncomp,) + tuple(shape)), [_h(ki) for ki in k])
        tout.copy_(torch.as_tensor(out.reshape(tuple(tout.shape))))

    def ps_gradient_stats(self, ta, count, tout, precision):
        ForcingEngine.log.append(('ps_gradient_stats', int(count), precision))
        assert ta.numel() == 9 * count
        tout.copy_(torch.as_tensor(G.stats(_h(ta).reshape(3, 3, count))[0]))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(GradientEngine())
    ForcingEngine.log = []
    yield
    _lib.set_engine(old)


def test_gradient_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape = (8, 6, 20)
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    k, _ = R.wavenumbers(shape, True)
    f_h = _cfield(shape, 4, 3)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    nan = complex(np.nan, np.nan)
    # a velocity: DistArrays, [3] in and the rank-2 layout out
    uh, A_hat = newDistArray(fft, rank=1), newDistArray(fft, rank=2)
    uh[...] = f_h[:3]
    assert tuple(A_hat.shape) == (3, 3) + ops.shape
    assert ops.gradient(uh, A_hat) is A_hat
    assert ForcingEngine.log[-1] == ('ps_gradient', 3, ops.shape, 8)
    assert np.array_equal(G.bits(np.asarray(A_hat)), G.bits(G.grad(f_h[:3], k)))
    # [m] + shape, m = 1 ... 4, tensors
    for m in (1, 2, 3, 4):
        out = torch.full((m, 3) + ops.shape, nan, dtype=torch.complex128)
        assert ops.gradient(T(f_h[:m]), out) is out
        assert ForcingEngine.log[-1] == ('ps_gradient', m, ops.shape, 8)
        assert np.array_equal(G.bits(_h(out)), G.bits(G.grad(f_h[:m], k)))
    # a scalar field: the spectral shape itself, out [3] + shape
    out = torch.full((3,) + ops.shape, nan, dtype=torch.complex128)
    ops.gradient(T(f_h[2]), out)
    assert ForcingEngine.log[-1] == ('ps_gradient', 1, ops.shape, 8)
    assert np.array_equal(G.bits(_h(out)), G.bits(G.grad(f_h[2], k)))
    n = len(ForcingEngine.log)
    f5 = T(np.concatenate([f_h, f_h[:1]]))
    o3 = torch.zeros((3, 3) + ops.shape, dtype=torch.complex128)
    for bad in ((f5, torch.zeros((5, 3) + ops.shape, dtype=torch.complex128)),                   # m = 5
                (T(f_h[0]), torch.zeros((1, 3) + ops.shape, dtype=torch.complex128)),            # scalar form with [1][3] out
                (T(f_h[:1]), torch.zeros((3,) + ops.shape, dtype=torch.complex128)),             # [1] form with [3] out
                (T(f_h[:3]), torch.zeros((9,) + ops.shape, dtype=torch.complex128)),             # [3 m] instead of [m][3]
                (T(f_h[:2]), o3),                                                                # out of another m
                (T(f_h[:3]), o3.to(torch.complex64)),                                            # mixed precision
                (T(f_h[:3]).to(torch.complex64), o3.to(torch.complex64)),                        # a single field on a double transform
                (T(f_h[:3]).real.contiguous(), o3),                                              # a real field
                (T(f_h[:3]), torch.zeros((3, 3) + ops.shape + (2,), dtype=torch.complex128)[..., 0]),      # a strided out
                (T(f_h[:3])[..., :-1], torch.zeros((3, 3) + ops.shape[:2] + (ops.shape[2] - 1,), dtype=torch.complex128))):
        with pytest.raises(AssertionError):
            ops.gradient(*bad)
    assert len(ForcingEngine.log) == n, 'a refused call reached the engine'
    fft.destroy()


@pytest.mark.parametrize('P,grid', [(1, None), (2, [2, 1, 1]), (4, [2, 2, 1])])
def test_gradient_stats_forms_and_rank_reduction(P, grid, engine):
    from mpi4py_fft_amd import PFFT, _lib, newDistArray, spectral
    shape = (8, 8, 20)
    A_h = np.random.default_rng(6).standard_normal((3, 3) + shape)
    ref, mag = G.stats(A_h)
    count = int(np.prod(shape))

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=grid, wire='torch') if P > 1 else PFFT(comm, shape, dtype='d')
        ops = spectral.SpectralOps(fft, R.BOX)
        A = newDistArray(fft, False, rank=2)
        A[...] = A_h[(slice(None),) * 2 + fft.local_slice(False)]
        full = ops.gradient_stats(A)
        local = ops.gradient_stats(A.tensor, reduce=False)
        out = torch.zeros(_lib.PS_GRAD_NVAL, dtype=torch.float64)
        assert ops.gradient_stats(A, out=out, reduce=False) is out
        n = len(ForcingEngine.log)
        t = A.tensor
        for bad in () if P > 1 else (                                                            # (the log is shared by the thread ranks)lambda: ops.gradient_stats(t.to(torch.float32)),                             # a float32 field on a double transform
                    lambda: ops.gradient_stats(t[0]),                                            # [3] + shape
                    lambda: ops.gradient_stats(t.reshape((9,) + tuple(t.shape[2:]))),            # [9] + shape
                    lambda: ops.gradient_stats(t.transpose(0, 1)),                               # not contiguous
                    lambda: ops.gradient_stats(t[..., :-1]),
                    lambda: ops.gradient_stats(t.to(torch.complex128)),
                    lambda: ops.gradient_stats(t, out=torch.zeros(19, dtype=torch.float64), reduce=False),
                    lambda: ops.gradient_stats(t, out=torch.zeros(20, dtype=torch.float32), reduce=False),
                    lambda: ops.gradient_stats(t, out=torch.zeros(40, dtype=torch.float64)[::2], reduce=False)):
            with pytest.raises(AssertionError):
                bad()
        assert P > 1 or len(ForcingEngine.log) == n, 'a refused call reached the engine'
        fft.destroy()
        return full, _h(local).copy(), _h(out).copy()
    res = cases.run_ranks(P, body)
    for full, local, out in res:
        assert isinstance(full, np.ndarray) and full.dtype == np.float64 and full.shape == (20,)
        assert np.array_equal(full, res[0][0]), 'ranks disagree'          # bit for bit
        G.assert_stats(full, ref, mag, count, 'P = %d' % P)
        assert np.array_equal(local, out)
    # the local parts combine to the whole: maxima by max, the rest added in rank order along one grid axis after the other
    assert np.array_equal(np.max([r[1][:3] for r in res], axis=0), res[0][0][:3])
    assert np.allclose(sum(r[1][3:] for r in res), ref[3:], rtol=1e-13, atol=1e-13)
    if P > 1:
        assert any(not np.array_equal(r[1], res[0][0]) for r in res)
    assert (_lib.GS_MAX_SS, _lib.GS_MAX_DIV, _lib.GS_DIV2, _lib.GS_Q, _lib.GS_SSS, _lib.GS_LONG2, _lib.GS_TRANS4) == (0, 2, 3, 9, 13, 15, 19)
    assert _lib.PS_GRAD_NVAL == G.NVAL == 20


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    for name in ('gfft_ps_gradient', 'gfft_ps_gradient_stats'):
        assert name in _lib.EXPORTS
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def grad(f=p, out=p, nc=3, k=(p, p, p), n=(2, 2, 2), prec=8):
        return lib.gfft_ps_gradient(f, out, nc, k[0], k[1], k[2], n[0], n[1], n[2], prec, None)
    for bad in (dict(f=None), dict(out=None), dict(k=(None, p, p)), dict(k=(p, None, p)), dict(k=(p, p, None)), dict(nc=0), dict(nc=-1),
                dict(n=(-1, 2, 2)), dict(n=(2, -1, 2)), dict(n=(2, 2, -1)), dict(prec=3), dict(prec=16), dict(prec=0)):
        assert grad(**bad) == -1, bad
    assert lib.gfft_last_error() == b'gfft_ps_gradient: bad argument'
    assert grad(nc=5) == -2 and lib.gfft_last_error() == b'gfft_ps_gradient: more than 4 components'
    assert grad(nc=5, n=(2, 2, -1)) == -1 and grad(nc=64, f=None) == -1       # a bad argument beside it is still a bad argument
    for n in ((2, (1 << 30) + 1, 2), (2, 2, (1 << 30) + 1)):
        assert grad(n=n) == -2 and grad(n=n, nc=1, prec=4) == -2, n          # beyond the documented limit: unsupported, not invalid
        assert lib.gfft_last_error() == b'gfft_ps_gradient: axis longer than 2^30'
        assert grad(n=n, prec=3) == -1 and grad(n=n, nc=0) == -1

    def stats(a=p, count=8, out=p, prec=8):
        return lib.gfft_ps_gradient_stats(a, count, out, prec, None)
    for bad in (dict(a=None), dict(out=None), dict(count=-1), dict(prec=3), dict(prec=16), dict(prec=0)):
        assert stats(**bad) == -1, bad
    assert lib.gfft_last_error() == b'gfft_ps_gradient_stats: bad argument'
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device
        assert grad() == -3 and grad(nc=1, prec=4) == -3 and grad(nc=4) == -3 and grad(n=(0, 2, 2)) == -3
        assert grad(n=(5, 1 << 30, 1 << 30)) == -3                   # 2^30 itself is allowed
        assert stats() == -3 and stats(count=0, prec=4) == -3


def test_gradient_moments_closed_forms():
    """Every derivative a single sine over one period: flatness 3/2 (longitudinal and transverse), skewness 0; with every
    A_ij equal, S_ij = A_ij and w = 0."""
    from mpi4py_fft_amd import _lib, spectral
    n = 64
    s = np.sin(2 * np.pi * np.arange(n) / n)
    A = np.broadcast_to(s, (3, 3, n)).copy()
    gs, _ = G.stats(A)
    m = spectral.gradient_moments(gs, n, nu=0.25)
    assert isinstance(m, spectral.GradientMoments) and m._fields[:4] == ('strain', 'enstrophy', 'Q', 'R')
    assert abs(m.flatness - 1.5) <= 1e-14 and abs(m.transverse_flatness - 1.5) <= 1e-14 and abs(m.skewness) <= 1e-15
    assert abs(m.strain - 4.5) <= 1e-14 and m.enstrophy == 0.0 and abs(m.dissipation - 2 * 0.25 * 4.5) <= 1e-14
    assert abs(m.dissipation_flatness - 1.5) <= 1e-14 and math.isnan(m.enstrophy_flatness) and math.isnan(m.strain_enstrophy_correlation)
    assert abs(m.div_rms - 3 * math.sqrt(0.5)) <= 1e-14 and abs(m.Q) <= 1e-15 and abs(m.R) <= 1e-15      # rank one: Q = R = 0 pointwise
    assert spectral.gradient_moments(gs, n).dissipation is None
    # hand-made sums: each formula reads the entries it names
    h = np.zeros(_lib.PS_GRAD_NVAL)
    h[[_lib.GS_SS, _lib.GS_WW, _lib.GS_SS2, _lib.GS_WW2, _lib.GS_SSWW]] = [20, 40, 80, 480, 240]
    h[[_lib.GS_Q, _lib.GS_R, _lib.GS_SSS, _lib.GS_WSW, _lib.GS_DIV2]] = [-5, 2.5, -3, 4, 40]
    h[[_lib.GS_LONG2, _lib.GS_LONG3, _lib.GS_LONG4, _lib.GS_TRANS2, _lib.GS_TRANS4]] = [120, -30, 480, 240, 960]
    m = spectral.gradient_moments(h, 10, nu=0.5)
    assert (m.strain, m.enstrophy, m.Q, m.R, m.dissipation) == (2.0, 2.0, -0.5, 0.25, 2.0)
    assert m.skewness == -1.0 / 4.0 ** 1.5 and m.flatness == 16.0 / 16.0 and m.transverse_flatness == 16.0 / 16.0
    assert (m.dissipation_flatness, m.enstrophy_flatness, m.strain_enstrophy_correlation) == (2.0, 3.0, 3.0)
    assert m.betchov == 1.0 and m.div_rms == 2.0
    with pytest.raises(AssertionError):
        spectral.gradient_moments(h[:19], 10)


SHAPES = [(16, 16, 16), (12, 10, 14), (9, 8, 7)]


def residuals(gs, mag, npoints, enstrophy):
    """The global identities of a solenoidal alias-free field, each divided by its magnitude M (the enstrophy check by sum ss)"""
    return {'ss = ww / 2': abs(gs[4] - gs[5] / 2) / mag[4], 'ss = N enstrophy': abs(gs[4] - npoints * enstrophy) / gs[4],
            'sum Q': abs(gs[9]) / mag[9], 'sum R': abs(gs[10]) / mag[10], 'wsw = -4/3 sss': abs(gs[14] + 4.0 / 3.0 * gs[13]) / mag[14]}


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_reference_obeys_the_identities_under_the_strict_rule_only(shape):
    """The reference alone.  Measured: the strict rule leaves 0 ... 2e-16, the field with its Nyquist planes kept 6e-2 ... 1e-1 in
    the worst identity.  The pointwise relation R = -(sss / 3 + wsw / 4) and the divergence are algebra on a trace-free tensor and
    hold either way."""
    n = int(np.prod(shape))
    worst = {}
    for truncate in (True, False):
        uh, k = G.solenoidal_field(shape, 5, truncate)
        w = R.wavenumbers(shape, True)[1]
        enstrophy = float(R.reference(uh, k, w)[0][1].sum())
        A = G.tensor(uh, k, shape)
        gs, mag = G.stats(A)
        res = residuals(gs, mag, n, enstrophy)
        p = G.pointwise(A)
        res_pt = float(np.abs(p['R'] + (p['sss'] / 3 + p['wsw'] / 4)).max() / np.abs(p['R']).max())
        div = gs[2] / math.sqrt(gs[0])
        print('%s %s: %s; pointwise R %.1e, max |div| / sqrt(max ss) %.1e'
              % (shape, 'strict 2/3' if truncate else 'Nyquist planes kept', ', '.join('%s %.1e' % kv for kv in res.items()), res_pt, div))
        assert gs[4] > 0 and res_pt <= 1e-13 and div <= 1e-14, (res_pt, div)
        worst[truncate] = res
    assert max(worst[True].values()) <= 1e-14, worst[True]
    assert max(worst[False].values()) > 1e-3 and worst[False]['ss = N enstrophy'] > 1e-3, worst[False]


def test_reference_magnitudes_and_nan():
    """M bounds |value| entry by entry; a NaN in A[1][2] reaches every sum but those of the diagonal alone and no maximum."""
    A = np.random.default_rng(9).standard_normal((3, 3, 1000)).astype('f')
    gs, mag = G.stats(A)
    assert np.all(np.abs(gs) <= mag) and np.all(mag[[15, 17, 18, 19]] == gs[[15, 17, 18, 19]])
    assert np.array_equal(G.stats(A.astype('d'))[0], gs), 'the input is converted to double first'
    B = A.copy()
    B[1, 2, 321] = np.nan
    gn, _ = G.stats(B)
    nan = [4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 18, 19]
    assert np.isnan(gn[nan]).all() and np.isfinite(np.delete(gn, nan)).all()
    assert np.array_equal(gn[[3, 15, 16, 17]], gs[[3, 15, 16, 17]]) and np.all(gn[:3] <= gs[:3])
    empty, m0 = G.stats(np.zeros((3, 3, 0)))
    assert np.array_equal(empty, np.zeros(20)) and np.array_equal(m0, np.zeros(20))
