"""Host logic of the B-spline interpolation (no GPU): the argument forms and refusals of `SpectralOps.scale_axes`,
`bspline_vectors` and `interpolate` over numpy stand-ins for the two kernels (tests/interp_ref.py), what reaches the engine, the
rank reduction on thread ranks, the argument checks of gfft_ps_scale_axes and gfft_ps_interp through ctypes, and the properties
of the method on the reference itself: partition of unity, the interpolation property, convergence, the split into blocks."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases, interp_ref as I, spectrum_ref as R
from tests.test_forcing_host import ForcingEngine, _h
from tests.test_pdf_host import PdfEngine


class InterpEngine(PdfEngine):
    """PdfEngine plus the two new entries restated with numpy (tests/interp_ref.py) on host tensors; the interpolation is the
    serial double sum of the reference"""

    def ps_scale_axes(self, tf, tout, ncomp, v, shape, precision):
        ForcingEngine.log.append(('ps_scale_axes', int(ncomp), tuple(vi is not None for vi in v), tuple(shape), precision))
        f = _h(tf).reshape((ncomp,) + tuple(shape))
        out = I.scale_axes(f, [None if vi is None else _h(vi) for vi in v])
        tout.copy_(torch.as_tensor(out.reshape(tuple(tout.shape))))

    def ps_interp(self, tc, ncomp, n, start, N, inv_dx, tx, npart, order, tout, precision):
        ForcingEngine.log.append(('ps_interp', int(ncomp), tuple(n), tuple(start), tuple(N), tuple(inv_dx), int(npart), int(order), precision))
        assert tc.numel() == ncomp * int(np.prod(n)) and tuple(tx.shape) == (npart, 3)
        out, _ = I.interp(_h(tc).reshape((ncomp,) + tuple(n)), _h(tx), inv_dx, order, N=N, start=start, acc=np.float64)
        tout.copy_(torch.as_tensor(out.reshape(tuple(tout.shape))))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(InterpEngine())
    ForcingEngine.log = []
    yield
    _lib.set_engine(old)


SHAPE = (8, 6, 20)


def test_scale_axes_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    fft = PFFT(comm.COMM_SELF, SHAPE, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    sshape = ops.shape
    rng = np.random.default_rng(21)
    f_h = rng.standard_normal((5,) + sshape) + 1j * rng.standard_normal((5,) + sshape)
    v_h = [rng.standard_normal(n) for n in sshape]
    F = newDistArray(fft, True, rank=1)
    dev = F.tensor.device
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    v = [T(vi) for vi in v_h]
    F[...] = f_h[:3]
    assert ops.scale_axes(F, v) is F                                   # in place, a DistArray
    assert ForcingEngine.log[-1] == ('ps_scale_axes', 3, (True, True, True), sshape, 8)
    assert np.array_equal(_h(F.tensor), I.scale_axes(f_h[:3], v_h))
    for m in (1, 2, 3, 4):                                             # out of place, each vector None in turn
        for drop in (None, 0, 1, 2):
            vv = [None if a == drop else v[a] for a in range(3)]
            out = torch.zeros((m,) + sshape, dtype=torch.complex128, device=dev)
            src = T(f_h[:m])
            assert ops.scale_axes(src, vv, out=out) is out
            assert ForcingEngine.log[-1][1:3] == (m, tuple(a != drop for a in range(3)))
            assert np.array_equal(_h(out), I.scale_axes(f_h[:m], [None if a == drop else v_h[a] for a in range(3)]))
            assert np.array_equal(_h(src), f_h[:m])
    s1 = T(f_h[0])                                                     # a scalar field: the spectral shape itself
    assert ops.scale_axes(s1, (None, None, None)) is s1 and np.array_equal(_h(s1), f_h[0])
    assert ForcingEngine.log[-1][1:3] == (1, (False, False, False))
    n = len(ForcingEngine.log)
    t3 = T(f_h[:3])
    for bad in (lambda: ops.scale_axes(T(f_h), v),                                                 # m = 5
                lambda: ops.scale_axes(t3.to(torch.complex64), v),                                 # a single field on a double transform
                lambda: ops.scale_axes(t3, [vi.to(torch.float32) for vi in v]),                    # ... and single vectors
                lambda: ops.scale_axes(t3.real.contiguous(), v),                                   # not complex
                lambda: ops.scale_axes(t3.transpose(1, 2), v),                                     # not contiguous (and another shape)
                lambda: ops.scale_axes(t3[..., :-1], v),
                lambda: ops.scale_axes(t3, v[:2]),                                                 # two vectors
                lambda: ops.scale_axes(t3, [v[0], v[1], v[2][:-1]]),                               # a vector of the wrong length
                lambda: ops.scale_axes(t3, [v[0], v[1], torch.cat([v[2], v[2]])[::2]]),            # ... not contiguous
                lambda: ops.scale_axes(t3, [v_h[0], v[1], v[2]]),                                  # a numpy vector
                lambda: ops.scale_axes(t3, v, out=torch.zeros((2,) + sshape, dtype=torch.complex128, device=dev)),
                lambda: ops.scale_axes(t3, v, out=torch.zeros((3,) + sshape, dtype=torch.complex64, device=dev)),
                lambda: ops.scale_axes(t3[0], v, out=torch.zeros((1,) + sshape, dtype=torch.complex128, device=dev))):
        with pytest.raises(AssertionError):
            bad()
    assert len(ForcingEngine.log) == n, 'a refused call reached the engine'
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_bspline_vectors(dt, engine):
    from mpi4py_fft_amd import PFFT, comm, spectral
    shape = (8, 6, 21)                                                 # even, even, odd (no Nyquist column on the last axis)
    fft = PFFT(comm.COMM_SELF, shape, dtype=dt)
    ops = spectral.SpectralOps(fft, R.BOX)
    assert ops.bspline_vectors(2) == (None, None, None)
    v = ops.bspline_vectors(4)
    rdt = np.float64 if dt == 'd' else np.float32
    want = I.bspline_vectors(shape, 4, real=True, dtype=rdt)
    ulp = np.finfo(rdt).eps
    for vi, wi, n in zip(v, want, ops.shape):
        vi = _h(vi)
        assert vi.dtype == rdt and vi.shape == (n,) and np.array_equal(vi, wi)
        assert vi[0] == 1.0 and np.all(vi >= 1.0) and np.all(vi <= 3.0 * (1 + 2 * ulp))
    assert abs(_h(v[0])[4] - 3.0) <= 2 * 3.0 * ulp and abs(_h(v[1])[3] - 3.0) <= 2 * 3.0 * ulp          # the Nyquist index of an even axis
    assert _h(v[2]).max() < 3.0 - 1e-3                                                                 # an odd axis has none
    # entry n against the symbol written out: 1 / ((2 + cos(2 pi n / N)) / 3), n = 0, 1, ..., -1
    n0 = np.fft.fftfreq(8, 1. / 8)
    assert np.allclose(_h(v[0]), 3.0 / (2.0 + np.cos(2 * np.pi * n0 / 8)), rtol=4 * ulp, atol=0)
    for bad in (lambda: ops.bspline_vectors(3), lambda: ops.bspline_vectors(6), lambda: ops.bspline_vectors(0)):
        with pytest.raises(AssertionError):
            bad()
    fft.destroy()


def test_interpolate_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    fft = PFFT(comm.COMM_SELF, SHAPE, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    assert ops.pstart == (0, 0, 0) and ops.pshape == SHAPE
    inv_dx = tuple(n / l for n, l in zip(SHAPE, R.BOX))
    rng = np.random.default_rng(22)
    c_h = rng.standard_normal((5,) + SHAPE)
    x_h = rng.uniform(-20.0, 30.0, (37, 3))
    U = newDistArray(fft, False, rank=1)
    dev = U.tensor.device
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    x = T(x_h)
    U[...] = c_h[:3]
    for order in (2, 4):
        got = ops.interpolate(U, x, order=order)                       # a velocity as a DistArray
        assert ForcingEngine.log[-1] == ('ps_interp', 3, SHAPE, (0, 0, 0), SHAPE, inv_dx, 37, order, 8)
        want, M = I.interp(c_h[:3], x_h, inv_dx, order)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (37, 3)
        assert np.all(np.abs(got - want) <= I.bound(M, order))
        for m in (1, 2, 3, 4):
            got = ops.interpolate(T(c_h[:m]), x, order=order)
            assert ForcingEngine.log[-1][1] == m and got.shape == (37, m)
            assert np.array_equal(got, I.interp(c_h[:m], x_h, inv_dx, order, acc=np.float64)[0])
        got = ops.interpolate(T(c_h[2]), x, order=order)               # a scalar field: [P]
        assert got.shape == (37,) and np.array_equal(got, I.interp(c_h[2:3], x_h, inv_dx, order, acc=np.float64)[0][:, 0])
    assert ops.interpolate(U, x).shape == (37, 3) and ForcingEngine.log[-1][7] == 4          # order defaults to 4
    out = torch.full((37, 2), -7.0, dtype=torch.float64, device=dev)
    assert ops.interpolate(T(c_h[:2]), x, order=2, out=out, reduce=False) is out
    assert np.array_equal(_h(out), I.interp(c_h[:2], x_h, inv_dx, 2, acc=np.float64)[0])
    assert isinstance(ops.interpolate(T(c_h[:2]), x, reduce=False), torch.Tensor)
    assert ops.interpolate(U, x[:0]).shape == (0, 3)                   # no particles
    n = len(ForcingEngine.log)
    t3 = T(c_h[:3])
    for bad in (lambda: ops.interpolate(T(c_h), x),                                                # m = 5
                lambda: ops.interpolate(t3.to(torch.float32), x),                                  # a single field on a double transform
                lambda: ops.interpolate(t3.transpose(1, 2), x),                                    # not contiguous (and another shape)
                lambda: ops.interpolate(t3[..., :-1], x),
                lambda: ops.interpolate(t3.to(torch.complex128), x),
                lambda: ops.interpolate(t3, x.to(torch.float32)),                                  # x not double
                lambda: ops.interpolate(t3, x_h),                                                  # ... not a tensor
                lambda: ops.interpolate(t3, x.reshape(-1)),                                        # ... not [P][3]
                lambda: ops.interpolate(t3, x[:, :2]),
                lambda: ops.interpolate(t3, T(np.zeros((37, 6)))[:, ::2]),                         # ... not contiguous
                lambda: ops.interpolate(t3, x, order=3),
                lambda: ops.interpolate(t3, x, order=6),
                lambda: ops.interpolate(t3, x, out=torch.zeros((37, 2), dtype=torch.float64, device=dev), reduce=False),
                lambda: ops.interpolate(t3, x, out=torch.zeros((37, 3), dtype=torch.float32, device=dev), reduce=False),
                lambda: ops.interpolate(t3, x, out=torch.zeros((37, 6), dtype=torch.float64, device=dev)[:, ::2], reduce=False),
                lambda: ops.interpolate(t3[0], x, out=torch.zeros((37, 1), dtype=torch.float64, device=dev), reduce=False)):
        with pytest.raises(AssertionError):
            bad()
    assert len(ForcingEngine.log) == n, 'a refused call reached the engine'
    fft.destroy()


@pytest.mark.parametrize('nranks,grid', [(1, None), (2, [2, 1, 1]), (4, [2, 2, 1])])
@pytest.mark.parametrize('order', [2, 4])
def test_rank_reduction(nranks, grid, order, engine):
    """Every rank adds the stencil points it owns; the reduced result is the same bits on every rank and the whole interpolant
    to (order^3 + 64 + ranks) 2^-53 M_p; the engine sees each rank's own start and n."""
    from mpi4py_fft_amd import PFFT, newDistArray, spectral
    shape = (8, 8, 20)
    inv_dx = tuple(n / l for n, l in zip(shape, R.BOX))
    rng = np.random.default_rng(23)
    c_h = rng.standard_normal((3,) + shape)
    x_h = rng.uniform(-15.0, 25.0, (50, 3))
    want, M = I.interp(c_h, x_h, inv_dx, order)

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=grid, wire='torch') if nranks > 1 else PFFT(comm, shape, dtype='d')
        ops = spectral.SpectralOps(fft, R.BOX)
        U = newDistArray(fft, False, rank=1)
        sl = fft.local_slice(False)
        U[...] = c_h[(slice(None),) + sl]
        x = torch.as_tensor(x_h, device=U.tensor.device)
        full = ops.interpolate(U, x, order=order)
        local = _h(ops.interpolate(U, x, order=order, reduce=False)).copy()
        fft.destroy()
        return full, local, ops.pstart, ops.pshape, tuple((s.start, s.stop - s.start) for s in sl)
    res = cases.run_ranks(nranks, body)
    for full, local, pstart, pshape, sl in res:
        assert isinstance(full, np.ndarray) and full.shape == (50, 3) and np.array_equal(full, res[0][0])
        assert np.all(np.abs(full - want) <= I.bound(M, order, nranks))
        assert pstart == tuple(s[0] for s in sl) and pshape == tuple(s[1] for s in sl)
        part, _ = I.interp(c_h[(slice(None),) + tuple(slice(a, a + n) for a, n in sl)], x_h, inv_dx, order, N=shape, start=pstart, acc=np.float64)
        assert np.array_equal(local, part)
    if nranks > 1:
        assert any(not np.array_equal(r[1], res[0][1]) for r in res)
        assert sorted(r[2] for r in res) == sorted(set(r[2] for r in res)), 'two ranks claim one block'


def test_partition_of_unity_and_planted_positions():
    """A constant field returns the constant within the bound, wherever the particle is -- also where the stencil is wider than
    the axis --; positions that are not finite, or too large to have a fraction, give NaN rows and leave the others alone."""
    rng = np.random.default_rng(24)
    for shape in ((8, 6, 20), (5, 3, 7), (3, 2, 5)):
        inv_dx = [n / l for n, l in zip(shape, R.BOX)]
        x = rng.uniform(-30.0, 40.0, (200, 3))
        x[:8] = [[0, 0, 0], [R.BOX[0], R.BOX[1], R.BOX[2]], [-5e-324, 0, 0], [np.nextafter(0, -1), -1e-300, -1e-17],
                 [1000 * R.BOX[0], -1000 * R.BOX[1], 3.0], [np.nan, 1, 1], [1, -np.inf, 1], [1, 1, 1e300]]
        c = np.full((1,) + shape, 2.75)
        for order in (2, 4):
            for acc in (np.float64, np.longdouble):
                out, M = I.interp(c, x, inv_dx, order, acc=acc)
                assert np.isnan(out[5:8]).all() and np.isnan(M[5:8]).all()
                ok = np.r_[0:5, 8:200]
                assert np.all(np.abs(out[ok] - 2.75) <= I.bound(M[ok], order)) and np.all(np.abs(M[ok] - 2.75) <= 1e-14)


def test_double_sum_against_its_long_double_twin():
    """The serial double sum stays within (order^3 + 32) 2^-53 M_p of the long-double one"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip('np.longdouble is double here: nothing to compare')
    rng = np.random.default_rng(25)
    for N in (16, 32):
        c = rng.standard_normal((2, N, N, N))
        x = rng.uniform(-10.0, 20.0, (400, 3))
        for order in (2, 4):
            d, _ = I.interp(c, x, [N / (2 * np.pi)] * 3, order, acc=np.float64)
            l, M = I.interp(c, x, [N / (2 * np.pi)] * 3, order)
            assert np.all(np.abs(d - l) <= I.bound(M, order, -32))


def test_blocks_resum_to_the_whole():
    """Two slabs along axis 0, and 2 x 2 pencils, add up to the whole within the bound; a block's share counts only its own points"""
    shape = (8, 6, 20)
    rng = np.random.default_rng(26)
    c = rng.standard_normal((2,) + shape)
    x = rng.uniform(-15.0, 25.0, (300, 3))
    inv_dx = [n / l for n, l in zip(shape, R.BOX)]
    for order in (2, 4):
        whole, M = I.interp(c, x, inv_dx, order)
        for cuts in ([(0, 4), (4, 4)], None):
            blocks = [((a, 0, 0), (n, 6, 20)) for a, n in cuts] if cuts else [((a, b, 0), (4, 3, 20)) for a in (0, 4) for b in (0, 3)]
            total, Mt = 0, 0
            for start, n in blocks:
                sl = tuple(slice(s, s + k) for s, k in zip(start, n))
                part, Mp = I.interp(c[(slice(None),) + sl], x, inv_dx, order, N=shape, start=start, acc=np.float64)
                total, Mt = total + part, Mt + Mp
            assert np.all(np.abs(total - whole) <= I.bound(M, order, len(blocks)))
            assert np.all(np.abs(Mt - M) <= 1e-13 * M)


def test_interpolation_property_and_convergence():
    """At grid points the prefiltered order-4 interpolant returns the samples (the order-2 one trivially); on the 400 points of
    the table the 32^3 error is at most 1/3 (order 2) and 1/8 (order 4) of the 16^3 error"""
    x = I.convergence_points()
    exact = I.smooth_field(x[:, 0], x[:, 1], x[:, 2])
    err = {}
    for N in (16, 32):
        f = I.grid_samples(N)
        inv_dx = [N / (2 * np.pi)] * 3
        rng = np.random.default_rng(27)
        cells = rng.integers(-2 * N, 3 * N, (300, 3))
        xg = cells * (2 * np.pi / N)
        for order in (2, 4):
            c = I.coefficients(f, order)[None]
            at_grid, _ = I.interp(c, xg, inv_dx, order)
            # a cell index times 2 pi / N times N / (2 pi) may land an ulp beside the integer: the interpolant is continuous, and
            # |grad f| <= 4 moves it by less than 4 * 48 * 2^-52 (in units of the grid spacing times its slope)
            want = f[cells[:, 0] % N, cells[:, 1] % N, cells[:, 2] % N]
            assert np.abs(at_grid[:, 0] - want).max() <= 1e-12 * np.abs(f).max()
            out, _ = I.interp(c, x, inv_dx, order)
            err[order, N] = float(np.abs(out[:, 0] - exact).max())
    assert err[2, 32] <= err[2, 16] / 3 and err[4, 32] <= err[4, 16] / 8, err
    assert 0.05 < err[2, 16] < 0.2 and 1e-3 < err[4, 16] < 1e-2, err


def test_scale_axes_reference():
    """One multiply per part: -0.0, inf and NaN go where IEEE puts them, in both precisions; None axes contribute nothing"""
    for cdt, rdt in ((np.complex128, np.float64), (np.complex64, np.float32)):
        rng = np.random.default_rng(28)
        f = (rng.standard_normal((2, 3, 4, 5)) + 1j * rng.standard_normal((2, 3, 4, 5))).astype(cdt)
        v = [rng.standard_normal(n).astype(rdt) for n in (3, 4, 5)]
        f[0, 1, 2, 3] = complex(-0.0, np.inf)
        v[2][1] = np.nan
        out = I.scale_axes(f, v)
        g = ((v[0][:, None, None] * v[1][None, :, None]).astype(rdt) * v[2][None, None, :]).astype(rdt)
        assert out.dtype == cdt and np.array_equal(out.real, f.real * g, equal_nan=True) and np.array_equal(out.imag, f.imag * g, equal_nan=True)
        assert np.isnan(out[..., 1]).all() and np.isinf(out[0, 1, 2, 3].imag)
        assert np.array_equal(I.scale_axes(f, (None, None, None)).view(rdt), f.view(rdt), equal_nan=True)
        only1 = I.scale_axes(f, (None, v[1], None))
        assert np.array_equal(only1.real, f.real * v[1][None, None, :, None], equal_nan=True)


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    for name in ('gfft_ps_scale_axes', 'gfft_ps_interp'):
        assert name in _lib.EXPORTS
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    I64 = lambda v: None if v is None else (ctypes.c_int64 * 3)(*v)
    D3 = lambda v: None if v is None else (ctypes.c_double * 3)(*v)

    def scale(out=p, f=p, nc=3, v=(p, p, p), n=(2, 2, 2), prec=8):
        return lib.gfft_ps_scale_axes(out, f, nc, v[0], v[1], v[2], n[0], n[1], n[2], prec, None)
    for bad in (dict(out=None), dict(f=None), dict(nc=0), dict(nc=-1), dict(n=(-1, 2, 2)), dict(n=(2, -1, 2)), dict(n=(2, 2, -1)),
                dict(prec=3), dict(prec=16), dict(prec=0)):
        assert scale(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_scale_axes: bad argument'
    assert scale(nc=5) == -2 and lib.gfft_last_error() == b'gfft_ps_scale_axes: more than 4 components'
    for n in (((1 << 30) + 1, 2, 2), (2, (1 << 30) + 1, 2), (2, 2, (1 << 30) + 1)):
        assert scale(n=n) == -2 and lib.gfft_last_error() == b'gfft_ps_scale_axes: axis longer than 2^30'
    assert scale(nc=5, f=None) == -1 and scale(n=(2, 2, (1 << 30) + 1), prec=5) == -1                 # bad beside unsupported

    def interp(c=p, nc=3, n=(2, 2, 2), start=(0, 0, 0), N=(4, 4, 4), inv_dx=(1.0, 1.0, 1.0), x=p, np_=2, order=4, out=p, prec=8):
        return lib.gfft_ps_interp(c, nc, I64(n), I64(start), I64(N), D3(inv_dx), x, np_, order, out, prec, None)
    for bad in (dict(c=None), dict(x=None), dict(out=None), dict(n=None), dict(start=None), dict(N=None), dict(inv_dx=None), dict(nc=0),
                dict(nc=-2), dict(np_=-1), dict(prec=3), dict(prec=16), dict(prec=0)):
        assert interp(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_interp: bad argument'
    for order in (0, 1, 3, 5, 6, 8, -4):
        assert interp(order=order) == -1 and lib.gfft_last_error() == b'gfft_ps_interp: order must be 2 or 4'
    for bad in (dict(n=(0, 2, 2)), dict(n=(2, -1, 2)), dict(N=(4, 0, 4)), dict(N=(4, 4, -4)), dict(start=(3, 0, 0)), dict(start=(0, 0, -1)),
                dict(n=(2, 2, 5)), dict(start=(0, 5, 0)), dict(start=(1 << 62, 0, 0), n=(1 << 62, 2, 2))):
        assert interp(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_interp: a block needs n >= 1, N >= 1 and 0 <= start, start + n <= N'
    for bad in (dict(inv_dx=(0.0, 1.0, 1.0)), dict(inv_dx=(1.0, -1.0, 1.0)), dict(inv_dx=(1.0, 1.0, np.inf)), dict(inv_dx=(np.nan, 1.0, 1.0))):
        assert interp(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_interp: inv_dx must be finite and > 0'
    assert interp(nc=5) == -2 and lib.gfft_last_error() == b'gfft_ps_interp: more than 4 components'
    assert interp(nc=5, order=3) == -1 and interp(nc=5, inv_dx=(0.0, 1.0, 1.0)) == -1 and interp(nc=5, c=None) == -1      # bad beside unsupported
    # (every call above is refused: a refused call dereferences no pointer.  Good calls are made only where there is no device)
    if not torch.cuda.is_available():
        assert scale() == -3 and scale(v=(None, None, None)) == -3 and scale(nc=1, prec=4, v=(None, p, None)) == -3 and scale(n=(0, 2, 2)) == -3
        assert scale(out=p, f=p) == -3                                                            # in place
        assert interp() == -3 and interp(order=2, prec=4, nc=1) == -3 and interp(np_=0) == -3
        assert interp(n=(2, 1, 3), start=(1, 0, 0), N=(3, 1, 3)) == -3                             # N < order: the stencil wraps onto itself
        assert interp(n=(2, 2, 2), start=(2, 2, 2)) == -3                                          # start + n == N
