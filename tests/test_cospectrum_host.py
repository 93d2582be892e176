"""Host logic of the two-field diagnostics (no GPU): `SpectralOps.cospectrum / transfer / helicity_spectrum` and their
rank reduction over a numpy stand-in for the kernel, `spectral.flux`, and the argument checks of gfft_ps_cospectrum."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases, cospectrum_ref as C, spectrum_ref as R
from tests.host_engine import HostEngine


class CospectrumEngine(HostEngine):
    """HostEngine plus gfft_ps_spectrum / gfft_ps_cospectrum restated with numpy on host tensors."""

    def ps_spectrum(self, tu, ncomp, k, w2, shape, dk, nbins, tout, precision):
        u = tu.numpy().reshape((ncomp,) + tuple(shape))
        w = np.ones(shape[2]) if w2 is None else w2.numpy().astype('d')
        tout.copy_(torch.as_tensor(R.reference(u, [ki.numpy().astype('d') for ki in k], w, dk, nbins)[0]))

    def ps_cospectrum(self, ta, tb, ncomp, op, scale, k, w2, shape, dk, nbins, tout, precision):
        a = ta.numpy().reshape((ncomp,) + tuple(shape))
        b = None if tb is None else tb.numpy().reshape((ncomp,) + tuple(shape))
        assert (op == C.HELICITY) == (tb is None)
        w = np.ones(shape[2]) if w2 is None else w2.numpy().astype('d')
        bins = C.reference(a, b, [ki.numpy().astype('d') for ki in k], w, op, scale, dk, nbins)[0]
        tout.copy_(torch.as_tensor(bins))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(CospectrumEngine())
    yield
    _lib.set_engine(old)


def _field(shape, m, seed):
    gs = shape[:2] + (shape[2] // 2 + 1,)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m,) + gs) + 1j * rng.standard_normal((m,) + gs)).astype('D')


@pytest.mark.parametrize('P,grid', [(1, None), (2, [2, 1, 1]), (4, [2, 2, 1]), (4, [4, 1, 1])])
def test_cospectrum_and_its_rank_reduction(P, grid, engine):
    from mpi4py_fft_amd import PFFT, newDistArray, spectral
    shape = (8, 8, 20)
    GA, GB = _field(shape, 3, 3), _field(shape, 3, 4)
    k, w = R.wavenumbers(shape, True)
    ref, modes, A = C.reference(GA, GB, k, w)
    href, _, hA = C.reference(GA, None, k, w, C.HELICITY)
    assert (ref[0] < 0).any() and (ref[0] > 0).any() and (href[0] < 0).any(), 'the case has no negative bins'

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=grid, wire='torch') if P > 1 else PFFT(comm, shape, dtype='d')
        ops = spectral.SpectralOps(fft, R.BOX)
        ah, bh = newDistArray(fft, rank=1), newDistArray(fft, rank=1)
        ah[...] = GA[(slice(None),) + fft.local_slice(True)]
        bh[...] = GB[(slice(None),) + fft.local_slice(True)]
        full = ops.cospectrum(ah, bh)
        local = ops.cospectrum(ah, bh, reduce=False)
        out = torch.zeros((2, 5), dtype=torch.float64)
        assert ops.cospectrum(ah, bh, scale=-2.0, nbins=5, out=out, reduce=False) is out
        scalar = ops.cospectrum(ah[1], bh[1])
        T = ops.transfer(ah, bh)
        H = ops.helicity_spectrum(ah)
        hel = ops.helicity(ah)
        same = ops.cospectrum(ah, ah, scale=0.5)
        E = ops.spectrum(ah)
        with pytest.raises(AssertionError, match='precision'):          # a complex64 field on a double transform
            ops.cospectrum(ah, bh.tensor.to(torch.complex64))
        with pytest.raises(AssertionError):                             # a scalar against a vector field
            ops.cospectrum(ah, bh[0])
        with pytest.raises(AssertionError, match='three'):
            ops.helicity_spectrum(ah[0])
        fft.destroy()
        return full, local.numpy().copy(), out.numpy().copy(), scalar, T, H, hel, same, E
    res = cases.run_ranks(P, body)
    for full, local, first5, scalar, T, H, hel, same, E in res:
        assert isinstance(full, np.ndarray) and full.dtype == np.float64 and full.shape == (2, R.default_nbins(shape))
        for x, y in zip((full, T, H), res[0][:1] + res[0][4:6]):
            assert np.array_equal(x, y), 'ranks disagree'                 # bit for bit
        C.assert_bins(full, ref, modes, A, 'P = %d' % P)
        assert np.array_equal(T, full)
        C.assert_bins(H, href, modes, hA, 'helicity, P = %d' % P)
        assert hel == H[0].sum()
        sref, _, sA = C.reference(GA[1], GB[1], k, w)
        C.assert_bins(scalar, sref, modes, sA, 'scalar fields')
        assert np.all(np.abs(same - E) <= (modes + 16) * 2.0 ** -52 * E), 'cospectrum(u, u, 0.5) is not spectrum(u)'
    # the local parts add up to the whole -- negative bins included --, and a short `out` holds the first shells unclipped
    assert np.all(np.abs(sum(r[1] for r in res) - ref) <= C.bound(modes, A))
    assert np.all(np.abs(sum(r[2] for r in res) + 2.0 * ref[:, :5]) <= 2.0 * C.bound(modes, A)[:, :5])
    if P > 1:
        assert any(not np.array_equal(r[1], res[0][0]) for r in res)


def test_flux():
    from mpi4py_fft_amd import spectral
    T = np.array([[0.0, -3.0, 1.0, 1.5, 0.5], [0.0, -3.0, 4.0, 13.5, 8.0]])
    want = np.array([0.0, 3.0, 2.0, 0.5, 0.0])
    pi = spectral.flux(T)
    assert isinstance(pi, np.ndarray) and pi.dtype == np.float64 and np.array_equal(pi, want)
    assert np.array_equal(spectral.flux(T[0]), want)                    # row 0 alone
    assert pi[-1] == -T[0].sum()
    assert np.array_equal(T[0], [0.0, -3.0, 1.0, 1.5, 0.5])             # the argument is left alone


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    DOT, HEL = _lib.PS_DOT, _lib.PS_HELICITY

    def call(a=p, b=p, ncomp=3, op=DOT, scale=1.0, k0=p, k1=p, k2=p, w2=p, n=(2, 2, 2), dk=1.0, nbins=4, out=p, prec=8):
        return lib.gfft_ps_cospectrum(a, b, ncomp, op, scale, k0, k1, k2, w2, n[0], n[1], n[2], dk, nbins, out, prec, None)
    assert 'gfft_ps_cospectrum' in _lib.EXPORTS and (DOT, HEL) == (0, 1)
    for bad in (dict(a=None), dict(b=None), dict(k0=None), dict(k1=None), dict(k2=None), dict(out=None), dict(op=2), dict(op=-1),
                dict(ncomp=0), dict(op=HEL, ncomp=1), dict(op=HEL, ncomp=4), dict(op=HEL, a=None), dict(nbins=0),
                dict(dk=0.0), dict(dk=-1.0), dict(dk=float('nan')), dict(scale=float('inf')), dict(scale=float('nan')),
                dict(prec=3), dict(n=(-1, 2, 2)), dict(n=(2, -1, 2)), dict(n=(2, 2, -1))):
        assert call(**bad) == -1, bad
    assert call(nbins=4097) == -2                       # beyond the documented limit: unsupported, not invalid
    assert call(nbins=1 << 20) == -2
    assert call(n=(1, (1 << 30) + 1, 1)) == -2 and call(n=(1, 1, (1 << 30) + 1)) == -2
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device: no weights, helicity without a second field, one component
        assert call(w2=None) == -3 and call(op=HEL, b=None) == -3 and call(ncomp=1) == -3 and call(scale=-0.5) == -3
