"""Host logic of the spectral diagnostics (no GPU): Hermitian weights, default shells, the rank reduction of
`SpectralOps.spectrum` over a numpy stand-in for the kernel, and the argument checks of gfft_ps_spectrum."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases, spectrum_ref as R
from tests.host_engine import HostEngine


class SpectrumEngine(HostEngine):
    """HostEngine plus gfft_ps_spectrum restated with numpy (tests/spectrum_ref.py) on host tensors."""
    calls = 0

    def ps_spectrum(self, tu, ncomp, k, w2, shape, dk, nbins, tout, precision):
        SpectrumEngine.calls += 1
        u = tu.numpy().reshape((ncomp,) + tuple(shape))
        w = np.ones(shape[2]) if w2 is None else w2.numpy().astype('d')
        bins, _ = R.reference(u, [ki.numpy().astype('d') for ki in k], w, dk, nbins)
        tout.copy_(torch.as_tensor(bins))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(SpectrumEngine())
    yield
    _lib.set_engine(old)


@pytest.mark.parametrize('shape,dt', [((8, 6, 20), 'd'), ((8, 6, 21), 'd'), ((8, 6, 20), 'f'), ((8, 6, 10), 'D'), ((8, 6, 9), 'F')])
def test_hermitian_weights_one_rank(shape, dt, engine):
    from mpi4py_fft_amd import PFFT, comm, spectral
    fft = PFFT(comm.COMM_SELF, shape, dtype=dt)
    w = spectral.hermitian_weights(fft)
    n = shape[2]
    if dt in 'fd':
        want = np.full(n // 2 + 1, 2.0)
        want[0] = 1
        if n % 2 == 0:
            want[-1] = 1
    else:
        want = np.ones(n)
    assert w.dtype == (torch.float64 if dt in 'dD' else torch.float32)
    assert np.array_equal(w.numpy(), want)
    assert np.array_equal(w.numpy(), R.wavenumbers(shape, dt in 'fd')[1])
    fft.destroy()


@pytest.mark.parametrize('shape', [(8, 8, 20), (8, 8, 21)])
@pytest.mark.parametrize('grid', [[2, 2, 1], [4, 1, 1]], ids=['pencil', 'slab'])
def test_hermitian_weights_follow_a_distributed_axis(shape, grid, engine):
    """On a pencil grid the halved axis of the spectral array is distributed: every rank holds the weights of ITS
    columns, and the blocks put together in global order are the one-rank vector."""
    from mpi4py_fft_amd import PFFT, spectral

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=grid, wire='torch')
        s = fft.local_slice(True)[2]
        w = spectral.hermitian_weights(fft).numpy().copy()
        assert len(w) == fft.shape(True)[2]
        fft.destroy()
        return s.start, s.stop, w
    res = cases.run_ranks(4, body)
    full = R.wavenumbers(shape, True)[1]
    for start, stop, w in res:
        assert np.array_equal(w, full[start:stop])
    if grid[1] > 1:
        assert any(stop - start < len(full) for start, stop, _ in res), 'axis 2 was not distributed: the case shows nothing'
    blocks = sorted({(a, b) for a, b, _ in res})
    assert blocks[0][0] == 0 and blocks[-1][1] == len(full) and all(x[1] == y[0] for x, y in zip(blocks, blocks[1:]))


@pytest.mark.parametrize('shape,nb', [((24, 16, 20), 33), ((12, 10, 21), 25), ((8, 8, 8), 13)])
def test_default_shells(shape, nb, engine):
    from mpi4py_fft_amd import PFFT, comm, spectral
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    assert ops.dk == 0.5 and ops.default_nbins() == nb == R.default_nbins(shape)
    assert np.array_equal(ops.shells(4), [0, 0.5, 1.0, 1.5])
    # nothing is dropped: the last default shell holds the corner mode
    k, w = R.wavenumbers(shape, True)
    _, modes = R.reference(np.ones((1,) + tuple(len(ki) for ki in k)), k, w)
    assert len(modes) == nb and modes[-1] > 0
    assert spectral.SpectralOps(fft).dk == 1.0          # L = 2 pi: unit shells
    fft.destroy()


def _field(shape, dt, m, seed=3):
    real = dt in 'fd'
    gs = shape[:2] + ((shape[2] // 2 + 1) if real else shape[2],)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m,) + gs) + 1j * rng.standard_normal((m,) + gs)).astype('D' if dt in 'dD' else 'F')


@pytest.mark.parametrize('P,grid', [(1, None), (2, [2, 1, 1]), (4, [2, 2, 1]), (4, [4, 1, 1])])
def test_spectrum_and_its_rank_reduction(P, grid, engine):
    from mpi4py_fft_amd import PFFT, newDistArray, spectral
    shape = (8, 8, 20)
    G = _field(shape, 'd', 3)
    k, w = R.wavenumbers(shape, True)
    ref, modes = R.reference(G, k, w)

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=grid, wire='torch') if P > 1 else PFFT(comm, shape, dtype='d')
        ops = spectral.SpectralOps(fft, R.BOX)
        uh = newDistArray(fft, rank=1)
        uh[...] = G[(slice(None),) + fft.local_slice(True)]
        full = ops.spectrum(uh)
        local = ops.spectrum(uh, reduce=False)
        out = torch.zeros((2, 5), dtype=torch.float64)
        assert ops.spectrum(uh, nbins=5, out=out, reduce=False) is out
        scalar = ops.spectrum(uh[1])
        with pytest.raises(AssertionError, match='precision'):          # a complex64 field on a double transform
            ops.spectrum(uh.tensor.to(torch.complex64))
        e, z = ops.energy(uh), ops.enstrophy(uh)
        fft.destroy()
        return full, local.numpy().copy(), out.numpy().copy(), scalar, e, z
    res = cases.run_ranks(P, body)
    for full, local, first5, scalar, e, z in res:
        assert isinstance(full, np.ndarray) and full.dtype == np.float64 and full.shape == (2, R.default_nbins(shape))
        assert np.array_equal(full, res[0][0]), 'ranks disagree'          # bit for bit
        R.assert_bins(full, ref, modes, 'P = %d' % P)
        assert e == full[0].sum() and z == full[1].sum()
        R.assert_bins(scalar, R.reference(G[1], k, w)[0], modes, 'scalar field')
    # the local parts add up to the whole, and a short `out` holds the first shells unclipped
    assert np.allclose(sum(r[1] for r in res), ref, rtol=1e-13, atol=0)
    assert np.allclose(sum(r[2] for r in res), ref[:, :5], rtol=1e-13, atol=0)
    if P > 1:
        assert any(not np.array_equal(r[1], res[0][0]) for r in res)


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(u=p, ncomp=3, k0=p, k1=p, k2=p, w2=p, n=(2, 2, 2), dk=1.0, nbins=4, out=p, prec=8):
        return lib.gfft_ps_spectrum(u, ncomp, k0, k1, k2, w2, n[0], n[1], n[2], dk, nbins, out, prec, None)
    assert 'gfft_ps_spectrum' in _lib.EXPORTS
    for bad in (dict(u=None), dict(k0=None), dict(k1=None), dict(k2=None), dict(out=None), dict(ncomp=0), dict(nbins=0),
                dict(dk=0.0), dict(dk=-1.0), dict(dk=float('nan')), dict(prec=3), dict(n=(2, -1, 2))):
        assert call(**bad) == -1, bad
    assert call(nbins=1 << 20) == -2                    # beyond the documented limit: unsupported, not invalid
    if not torch.cuda.is_available():
        assert call(w2=None) == -3                      # a good call gets as far as looking for a device
