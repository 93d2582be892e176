"""Host logic of the one-pass PDFs (no GPU): the argument forms and refusals of `SpectralOps.histogram` and
`SpectralOps.gradient_pdf` over numpy stand-ins for the kernels, the rank reduction, `pdf` / `joint_pdf`, the argument checks of
gfft_ps_histogram and gfft_ps_gradient_pdf, and the reference (tests/pdf_ref.py) against np.histogram."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases, pdf_ref as P, spectrum_ref as R
from tests.test_forcing_host import ForcingEngine, _h
from tests.test_gradient_host import GradientEngine


class PdfEngine(GradientEngine):
    """GradientEngine plus the two histogram entries restated with numpy (tests/pdf_ref.py) on host tensors"""

    def ps_histogram(self, tu, ncomp, count, lo, hi, nbins, tout, precision):
        ForcingEngine.log.append(('ps_histogram', int(ncomp), int(count), tuple(lo), tuple(hi), int(nbins), precision))
        assert tu.numel() == ncomp * count
        out = P.histogram(_h(tu).reshape(ncomp, count), list(zip(lo, hi)), nbins)
        tout.copy_(torch.as_tensor(out.reshape(tuple(tout.shape))))

    def ps_gradient_pdf(self, ta, count, qx, xr, nbx, qy, yr, nby, tout, precision):
        ForcingEngine.log.append(('ps_gradient_pdf', int(count), int(qx), tuple(xr), int(nbx), int(qy), tuple(yr), int(nby), precision))
        assert ta.numel() == 9 * count
        A = _h(ta).reshape(3, 3, count)
        y = None if qy < 0 else P.QUANTITIES[qy]
        tout.copy_(torch.as_tensor(P.gradient_pdf(A, P.QUANTITIES[qx], xr, nbx, y, yr, nby)))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(PdfEngine())
    ForcingEngine.log = []
    yield
    _lib.set_engine(old)


def test_constants_follow_the_header():
    from mpi4py_fft_amd import _lib, spectral
    assert _lib.PS_PDF_TAIL == P.TAIL == 3 and _lib.PS_Q_NONE == -1 and _lib.PS_Q_COUNT == 7
    assert [spectral.QUANTITIES[n] for n in P.QUANTITIES] == list(range(7))
    assert (_lib.PS_Q_SS, _lib.PS_Q_WW, _lib.PS_Q_DIV, _lib.PS_Q_Q, _lib.PS_Q_R, _lib.PS_Q_SSS, _lib.PS_Q_WSW) == tuple(range(7))


def test_histogram_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape = (8, 6, 20)
    count = int(np.prod(shape))
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    u_h = np.random.default_rng(11).standard_normal((4,) + shape)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    # a velocity as a DistArray, one range for all components
    U = newDistArray(fft, False, rank=1)
    U[...] = u_h[:3]
    got = ops.histogram(U, (-2.5, 2.5), 7)
    assert ForcingEngine.log[-1] == ('ps_histogram', 3, count, (-2.5,) * 3, (2.5,) * 3, 7, 8)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == (3, 10)
    assert np.array_equal(got, P.histogram(u_h[:3], [(-2.5, 2.5)] * 3, 7)) and np.all(got.sum(axis=1) == count)
    # m = 1 ... 4 with a range per component
    for m in (1, 2, 3, 4):
        rg = [(-1.0 - c, 2.0 + 0.5 * c) for c in range(m)]
        got = ops.histogram(T(u_h[:m]), rg, 64)
        assert ForcingEngine.log[-1][1] == m and got.shape == (m, 67)
        assert np.array_equal(got, P.histogram(u_h[:m], rg, 64))
    # a scalar field: the physical shape itself, a flat row back; out= and reduce=False
    got = ops.histogram(T(u_h[2]), (-1.0, 1.0), 5)
    assert got.shape == (8,) and np.array_equal(got, P.histogram(u_h[2:3], [(-1.0, 1.0)], 5)[0])
    out = torch.full((2, 8), -7, dtype=torch.int64)
    assert ops.histogram(T(u_h[:2]), (-1.0, 1.0), 5, out=out, reduce=False) is out
    assert np.array_equal(_h(out), P.histogram(u_h[:2], [(-1.0, 1.0)] * 2, 5))
    assert isinstance(ops.histogram(T(u_h[:2]), (-1.0, 1.0), 5, reduce=False), torch.Tensor)
    n = len(ForcingEngine.log)
    t3 = T(u_h[:3])
    tiny = np.nextafter(0.0, 1.0)
    for bad in (lambda: ops.histogram(T(np.concatenate([u_h, u_h[:1]])), (-1, 1), 4),               # m = 5
                lambda: ops.histogram(t3.to(torch.float32), (-1, 1), 4),                            # a single field on a double transform
                lambda: ops.histogram(t3.transpose(1, 2), (-1, 1), 4),                              # not contiguous (and another shape)
                lambda: ops.histogram(t3[..., :-1], (-1, 1), 4),
                lambda: ops.histogram(t3.to(torch.complex128), (-1, 1), 4),
                lambda: ops.histogram(t3, (-1, 1), 0),                                              # bins
                lambda: ops.histogram(t3, (-1, 1), -3),
                lambda: ops.histogram(t3, (-1, 1), 4097),
                lambda: ops.histogram(t3, (-1, 1), 4.0),
                lambda: ops.histogram(t3, (1, 1), 4),                                               # ranges
                lambda: ops.histogram(t3, (2, 1), 4),
                lambda: ops.histogram(t3, (-np.inf, 1), 4),
                lambda: ops.histogram(t3, (0, np.nan), 4),
                lambda: ops.histogram(t3, (-1.7e308, 1.7e308), 4),                                  # hi - lo overflows
                lambda: ops.histogram(t3, (0.0, tiny), 4096),                                       # bins / (hi - lo) overflows
                lambda: ops.histogram(t3, [(-1, 1), (-1, 1)], 4),                                   # two pairs for three components
                lambda: ops.histogram(t3, (-1, 1, 2), 4),
                lambda: ops.histogram(t3, (-1, 1), 4, out=torch.zeros((3, 6), dtype=torch.int64), reduce=False),
                lambda: ops.histogram(t3, (-1, 1), 4, out=torch.zeros((3, 7), dtype=torch.int32), reduce=False),
                lambda: ops.histogram(t3, (-1, 1), 4, out=torch.zeros((3, 7), dtype=torch.float64), reduce=False),
                lambda: ops.histogram(t3, (-1, 1), 4, out=torch.zeros((3, 14), dtype=torch.int64)[:, ::2], reduce=False),
                lambda: ops.histogram(T(u_h[0]), (-1, 1), 4, out=torch.zeros((1, 7), dtype=torch.int64), reduce=False)):
        with pytest.raises(AssertionError):
            bad()
    assert len(ForcingEngine.log) == n, 'a refused call reached the engine'
    fft.destroy()


def test_gradient_pdf_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, _lib, comm, newDistArray, spectral
    shape = (8, 6, 20)
    count = int(np.prod(shape))
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    A_h = np.random.default_rng(12).standard_normal((3, 3) + shape)
    A = newDistArray(fft, False, rank=2)
    A[...] = A_h
    flat = A_h.reshape(3, 3, count)
    for q, name in enumerate(P.QUANTITIES):
        got = ops.gradient_pdf(A, name, range=(-2.0, 3.0), bins=16)
        assert ForcingEngine.log[-1] == ('ps_gradient_pdf', count, q, (-2.0, 3.0), 16, -1, (0.0, 1.0), 1, 8)
        assert got.dtype == np.int64 and got.shape == (19,) and got.sum() == count
        assert np.array_equal(got, P.gradient_pdf(flat, name, (-2.0, 3.0), 16))
    rg = ((-4.0, 4.0), (-3.0, 5.0))
    got = ops.gradient_pdf(A, 'R', 'Q', range=rg, bins=(3, 5))
    assert ForcingEngine.log[-1] == ('ps_gradient_pdf', count, _lib.PS_Q_R, rg[0], 3, _lib.PS_Q_Q, rg[1], 5, 8)
    assert got.shape == (17,) and got.sum() == count and got[15] > 0
    assert np.array_equal(got, P.gradient_pdf(flat, 'R', rg[0], 3, 'Q', rg[1], 5))
    got = ops.gradient_pdf(A.tensor, 'ww', 'ss', range=rg, bins=8)                     # an int: both axes
    assert ForcingEngine.log[-1][4] == 8 and ForcingEngine.log[-1][7] == 8 and got.shape == (66,)
    out = torch.full((66,), -7, dtype=torch.int64)
    assert ops.gradient_pdf(A, 'ww', 'ss', range=rg, bins=8, out=out, reduce=False) is out
    assert np.array_equal(_h(out), got)
    assert ops.gradient_pdf(A, 'Q', 'R', range=rg, bins=(128, 128)).shape == (16386,)
    assert ops.gradient_pdf(A, 'Q', range=rg[0], bins=4096).shape == (4099,)
    n = len(ForcingEngine.log)
    t = A.tensor
    for bad in (lambda: ops.gradient_pdf(t, 'q', range=(-1, 1), bins=4),                         # unknown quantities
                lambda: ops.gradient_pdf(t, None, range=(-1, 1), bins=4),
                lambda: ops.gradient_pdf(t, 'Q', 'rr', range=rg, bins=4),
                lambda: ops.gradient_pdf(t, 'Q'),                                                # no range, no bins
                lambda: ops.gradient_pdf(t, 'Q', range=(-1, 1)),
                lambda: ops.gradient_pdf(t, 'Q', bins=4),
                lambda: ops.gradient_pdf(t, 'Q', range=rg, bins=4),                              # two ranges for one quantity
                lambda: ops.gradient_pdf(t, 'Q', 'R', range=(-1, 1), bins=4),                    # one range for two
                lambda: ops.gradient_pdf(t, 'Q', range=(-1, 1), bins=(4, 4)),
                lambda: ops.gradient_pdf(t, 'Q', range=(-1, 1), bins=0),
                lambda: ops.gradient_pdf(t, 'Q', range=(-1, 1), bins=4097),
                lambda: ops.gradient_pdf(t, 'Q', 'R', range=rg, bins=(0, 4)),
                lambda: ops.gradient_pdf(t, 'Q', 'R', range=rg, bins=(129, 128)),
                lambda: ops.gradient_pdf(t, 'Q', 'R', range=rg, bins=(4, 4, 4)),
                lambda: ops.gradient_pdf(t, 'Q', 'R', range=((1, 1), (0, 1)), bins=4),
                lambda: ops.gradient_pdf(t, 'Q', 'R', range=((0, 1), (0, np.inf)), bins=4),
                lambda: ops.gradient_pdf(t, 'Q', range=(3, -3), bins=4),
                lambda: ops.gradient_pdf(t[0], 'Q', range=(-1, 1), bins=4),                      # [3] + shape
                lambda: ops.gradient_pdf(t.reshape((9,) + tuple(t.shape[2:])), 'Q', range=(-1, 1), bins=4),
                lambda: ops.gradient_pdf(t.transpose(0, 1), 'Q', range=(-1, 1), bins=4),
                lambda: ops.gradient_pdf(t.to(torch.float32), 'Q', range=(-1, 1), bins=4),
                lambda: ops.gradient_pdf(t, 'Q', range=(-1, 1), bins=4, out=torch.zeros(6, dtype=torch.int64), reduce=False),
                lambda: ops.gradient_pdf(t, 'Q', range=(-1, 1), bins=4, out=torch.zeros(7, dtype=torch.float64), reduce=False),
                lambda: ops.gradient_pdf(t, 'Q', 'R', range=rg, bins=4, out=torch.zeros(19, dtype=torch.int64), reduce=False)):
        with pytest.raises(AssertionError):
            bad()
    assert len(ForcingEngine.log) == n, 'a refused call reached the engine'
    fft.destroy()


@pytest.mark.parametrize('nranks,grid', [(1, None), (2, [2, 1, 1]), (4, [2, 2, 1])])
def test_rank_reduction_is_exact(nranks, grid, engine):
    from mpi4py_fft_amd import PFFT, newDistArray, spectral
    shape = (8, 8, 20)
    count = int(np.prod(shape))
    rng = np.random.default_rng(13)
    u_h, A_h = rng.standard_normal((3,) + shape), rng.standard_normal((3, 3) + shape)
    hr, jr = [(-2.5, 2.5), (-1.0, 1.5), (0.0, 3.0)], ((-3.0, 3.0), (-4.0, 2.0))
    want_h = P.histogram(u_h, hr, 7)
    want_1 = P.gradient_pdf(A_h.reshape(3, 3, count), 'ss', (0.0, 12.0), 9)
    want_j = P.gradient_pdf(A_h.reshape(3, 3, count), 'R', jr[0], 3, 'Q', jr[1], 5)

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=grid, wire='torch') if nranks > 1 else PFFT(comm, shape, dtype='d')
        ops = spectral.SpectralOps(fft, R.BOX)
        U, A = newDistArray(fft, False, rank=1), newDistArray(fft, False, rank=2)
        U[...] = u_h[(slice(None),) + fft.local_slice(False)]
        A[...] = A_h[(slice(None),) * 2 + fft.local_slice(False)]
        full = (ops.histogram(U, hr, 7), ops.gradient_pdf(A, 'ss', range=(0.0, 12.0), bins=9),
                ops.gradient_pdf(A, 'R', 'Q', range=jr, bins=(3, 5)))
        local = _h(ops.histogram(U, hr, 7, reduce=False)).copy()
        fft.destroy()
        return full, local
    res = cases.run_ranks(nranks, body)
    for full, local in res:
        for got, want in zip(full, (want_h, want_1, want_j)):
            assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
        assert np.all(local.sum(axis=1) == count // nranks)
    assert np.array_equal(sum(r[1] for r in res), want_h)
    if nranks > 1:
        assert any(not np.array_equal(r[1], res[0][1]) for r in res)


def test_pdf_and_joint_pdf_integrate_to_the_share_in_range():
    from mpi4py_fft_amd import spectral
    rng = np.random.default_rng(14)
    x = rng.standard_normal(20000)
    x[:5] = np.nan
    lo, hi, nbins = -1.5, 2.0, 35
    c = P.histogram(x[None], [(lo, hi)], nbins)[0]
    p = spectral.pdf(c, (lo, hi))
    assert isinstance(p, spectral.Pdf) and p.centres.shape == p.density.shape == (nbins,)
    width = (hi - lo) / nbins
    assert np.allclose(p.centres, lo + (np.arange(nbins) + 0.5) * width, rtol=0, atol=1e-14)
    assert (p.below, p.above, p.nan) == (int(c[nbins]), int(c[nbins + 1]), 5) and p.below > 0 and p.above > 0
    share = c[:nbins].sum() / float(len(x) - 5)
    assert abs(p.density.sum() * width - share) <= 1e-14 and 0.5 < share < 1
    # against numpy's density, which normalises by the in-range count instead
    ref, _ = np.histogram(x[~np.isnan(x)], bins=nbins, range=(lo, hi), density=True)
    assert np.allclose(p.density, ref * share, rtol=1e-12, atol=0)
    pooled = spectral.pdf(c + c, (lo, hi))                       # rows add before normalising
    assert np.allclose(pooled.density, p.density, rtol=1e-15, atol=0) and pooled.nan == 10
    A = rng.standard_normal((3, 3, 5000))
    A[1, 2, 7] = np.nan
    rg, bins = ((-2.0, 2.0), (-3.0, 1.0)), (6, 4)
    cj = P.gradient_pdf(A, 'R', rg[0], bins[0], 'Q', rg[1], bins[1])
    j = spectral.joint_pdf(cj, rg, bins)
    assert isinstance(j, spectral.JointPdf) and j.density.shape == bins and j.xcentres.shape == (6,) and j.ycentres.shape == (4,)
    assert (j.outside, j.nan) == (int(cj[24]), 1) and j.outside > 0
    share = cj[:24].sum() / 4999.0
    assert abs(j.density.sum() * (4.0 / 6) * (4.0 / 4) - share) <= 1e-14 and 0.3 < share < 1
    assert j.density[2, 1] == cj[2 * 4 + 1] / (4999.0 * (4.0 / 6) * 1.0)          # bin bx * nby + by
    sq = spectral.joint_pdf(P.gradient_pdf(A, 'R', rg[0], 5, 'Q', rg[1], 5), rg, 5)
    assert sq.density.shape == (5, 5)
    for bad in (lambda: spectral.pdf(c[:3], (lo, hi)), lambda: spectral.pdf(c.astype('d'), (lo, hi)),
                lambda: spectral.joint_pdf(cj, rg, (4, 5)), lambda: spectral.joint_pdf(cj[:-1], rg, bins)):
        with pytest.raises(AssertionError):
            bad()


def test_reference_against_numpy_histogram():
    """Values kept a relative 1e-9 away from every edge: np.histogram (which bins by searching its edge array) and the rule
    (which multiplies) must then agree exactly; the edge cases themselves are stated by hand."""
    rng = np.random.default_rng(15)
    for lo, hi, nbins in ((-2.5, 2.5, 7), (0.0, 1.0, 64), (-1.0, 3.0, 4096), (-3.0, -1.0, 1)):
        x = rng.uniform(lo - 1.0, hi + 1.0, 50000)
        edges = np.linspace(lo, hi, nbins + 1)
        near = np.abs(x[:, None] - edges[np.clip(np.searchsorted(edges, x)[:, None] + np.array([-1, 0]), 0, nbins)]).min(axis=1)
        x = x[near > 1e-9 * (hi - lo)]
        got = P.histogram(x[None], [(lo, hi)], nbins)[0]
        ref, _ = np.histogram(x, bins=nbins, range=(lo, hi))
        assert np.array_equal(got[:nbins], ref) and got[nbins] == (x < lo).sum() and got[nbins + 1] == (x > hi).sum() and got[nbins + 2] == 0
        assert got.sum() == len(x)
    lo, hi, nbins = -2.5, 2.5, 4
    x = np.array([lo, hi, np.nextafter(hi, -np.inf), np.nextafter(lo, -np.inf), np.inf, -np.inf, np.nan, -0.0, 5e-324, 0.0])
    # (the value below hi: x - lo = 5 - 2^-51 is a tie that rounds to 5, so t = nbins -- "within rounding of hi" is above)
    assert list(P.slots(x, lo, hi, nbins)) == [0, 5, 5, 4, 5, 4, 6, 2, 2, 2]
    assert list(P.slots(np.array([np.nextafter(1.0, 0.0), 1.0]), 0.0, 1.0, 4)) == [3, 5]          # ... and here it is not: the last bin
    assert list(P.slots(np.array([-0.0, 0.0, 5e-324, -5e-324]), 0.0, 1.0, 3)) == [0, 0, 0, 3]
    assert list(P.slots(np.array([0.3], dtype='f'), 0.0, 1.0, 10)) == [3]          # float32 0.3 > 0.3: converted first, then binned
    assert P.histogram(np.zeros((2, 0)), [(0, 1)] * 2, 5).tolist() == [[0] * 8] * 2


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    for name in ('gfft_ps_histogram', 'gfft_ps_gradient_pdf'):
        assert name in _lib.EXPORTS
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    D = lambda *v: (ctypes.c_double * len(v))(*v)
    tiny = 5e-324

    def hist(u=p, nc=3, count=8, lo=(-1.0,) * 4, hi=(1.0,) * 4, nbins=16, out=p, prec=8):
        return lib.gfft_ps_histogram(u, nc, count, None if lo is None else D(*lo), None if hi is None else D(*hi), nbins, out, prec, None)
    for bad in (dict(u=None), dict(out=None), dict(lo=None), dict(hi=None), dict(nc=0), dict(nc=-1), dict(count=-1), dict(nbins=0),
                dict(nbins=-4), dict(prec=3), dict(prec=16), dict(prec=0)):
        assert hist(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_histogram: bad argument'
    for bad in (dict(lo=(1.0,) * 4), dict(lo=(2.0,) * 4), dict(lo=(-np.inf,) * 4), dict(hi=(np.inf,) * 4), dict(hi=(np.nan,) * 4),
                dict(lo=(np.nan,) * 4), dict(lo=(-1.7e308,) * 4, hi=(1.7e308,) * 4), dict(lo=(0.0,) * 4, hi=(tiny,) * 4, nbins=4096),
                dict(lo=(-1.0, -1.0, 3.0, -1.0))):                             # the third component's range alone
        assert hist(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_histogram: a range must be finite with lo < hi'
    assert hist(nc=5) == -2 and lib.gfft_last_error() == b'gfft_ps_histogram: more than 4 components'
    assert hist(nbins=4097) == -2 and lib.gfft_last_error() == b'gfft_ps_histogram: more than 4096 bins'
    assert hist(nc=1, count=1 << 62) == -2 and lib.gfft_last_error() == b'gfft_ps_histogram: more than 2^32 points per workgroup'
    assert hist(nc=4, nbins=4096, count=1 << 41) == -2 and hist(nc=1, nbins=4096, count=1 << 43) == -2
    assert hist(nc=5, count=-1) == -1 and hist(nbins=4097, u=None) == -1 and hist(nbins=4097, lo=(1.0,) * 4) == -1      # bad beside unsupported

    def gpdf(a=p, count=8, qx=_lib.PS_Q_R, xr=(-1.0, 1.0), nbx=8, qy=_lib.PS_Q_Q, yr=(-1.0, 1.0), nby=8, out=p, prec=8):
        return lib.gfft_ps_gradient_pdf(a, count, qx, xr[0], xr[1], nbx, qy, yr[0], yr[1], nby, out, prec, None)
    none = _lib.PS_Q_NONE
    for bad in (dict(a=None), dict(out=None), dict(count=-1), dict(nbx=0), dict(nby=0), dict(nbx=-1), dict(qx=none), dict(qx=7), dict(qx=-2),
                dict(qy=7), dict(qy=-2), dict(qy=none, nby=2), dict(qy=none, nby=0), dict(prec=3), dict(prec=16), dict(prec=0)):
        assert gpdf(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_gradient_pdf: bad argument'
    for bad in (dict(xr=(1.0, 1.0)), dict(xr=(2.0, 1.0)), dict(xr=(-np.inf, 1.0)), dict(xr=(0.0, np.nan)), dict(yr=(1.0, 1.0)),
                dict(yr=(0.0, np.inf)), dict(xr=(-1.7e308, 1.7e308)), dict(yr=(0.0, tiny), nby=4096, nbx=2), dict(qy=none, nby=1, xr=(3.0, -3.0))):
        assert gpdf(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_gradient_pdf: a range must be finite with lo < hi'
    assert gpdf(qy=none, nby=1, nbx=4097) == -2 and lib.gfft_last_error() == b'gfft_ps_gradient_pdf: more than 4096 bins'
    assert gpdf(nbx=129, nby=128) == -2 and lib.gfft_last_error() == b'gfft_ps_gradient_pdf: more than 16384 joint bins'
    assert gpdf(nbx=1 << 20, nby=1 << 20) == -2
    assert gpdf(count=1 << 62) == -2 and lib.gfft_last_error() == b'gfft_ps_gradient_pdf: more than 2^32 points per workgroup'
    assert gpdf(nbx=129, nby=128, a=None) == -1 and gpdf(qy=none, nby=1, nbx=4097, prec=5) == -1
    # (every call above is refused: a refused call dereferences no pointer.  A good call with these host pointers must never
    # reach a device, so good calls are made only where there is none)
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device
        assert hist(nc=2, lo=(-1.0, -1.0, 3.0, -1.0)) == -3                    # a bad third range that two components do not read
        assert gpdf(qy=none, nby=1, yr=(np.nan, -np.inf)) == -3                # the y range of a 1-D table is ignored
        assert gpdf(nbx=8192, nby=2) == -3                                     # 16384 joint bins are allowed, however they split
        assert hist() == -3 and hist(nc=1, prec=4) == -3 and hist(nc=4, nbins=4096) == -3 and hist(count=0) == -3
        assert gpdf() == -3 and gpdf(nbx=128, nby=128, prec=4) == -3 and gpdf(qy=none, nby=1, nbx=4096) == -3 and gpdf(count=0) == -3
        for q in range(7):
            assert gpdf(qx=q, qy=none, nby=1) == -3 and gpdf(qx=6 - q, qy=q) == -3
