"""gfft_ps_spectrum / SpectralOps.spectrum on the device against the fsum reference of tests/spectrum_ref.py.

Bound (derived there, not measured): per bin |got - ref| <= (modes in the bin + 16) 2^-52 ref, in both precisions; empty
bins exactly 0.  Boxes without shell-boundary ties only (L = (2 pi, 4 pi, 2 pi), dk = 1/2).

Launch geometry the shapes are chosen against (csrc/spectral.hip): workgroups of 256 lanes, V modes per lane (V = 1 in
fp64; V = 2 in fp32 when the mode count is even, else 1), each workgroup owning one contiguous chunk of flat modes and
walking it 256 V modes at a time; at most 2048 workgroups.  So a workgroup takes a SECOND step only beyond
2048 * 256 * V modes = 524 288 (fp64) / 1 048 576 (fp32): the two `sweep` shapes are the smallest convenient ones past
that.  Lanes combine equal neighbouring bins inside rows of 16 lanes; rows of the array shorter than that (4, 6, 7, 11),
longer than a wave (129) and |k2| rising then falling along a row (complex transforms) are all here.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, spectrum_ref as R

SWEEP = {'d': 2048 * 256 * 1, 'f': 2048 * 256 * 2}


def _field(shape, dt, m, seed=11):
    real = dt in 'fd'
    gs = tuple(shape[:2]) + ((shape[2] // 2 + 1) if real else shape[2],)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m,) + gs) + 1j * rng.standard_normal((m,) + gs)).astype('D' if dt in 'dD' else 'F')


_REF = {}


def _reference(shape, dt, m):
    """(field, k, w, bins, modes per bin) -- computed once per case and shared, never modified"""
    key = (tuple(shape), dt, m)
    if key not in _REF:
        G = _field(shape, dt, m)
        k, w = R.wavenumbers(shape, dt in 'fd')
        bins, modes = R.reference(G, k, w)
        for a in (G, bins, modes):
            a.setflags(write=False)
        _REF[key] = (G, k, w, bins, modes)
    return _REF[key]


def _ops(comm, shape, dt, **kw):
    from mpi4py_fft_amd import PFFT, spectral
    fft = PFFT(comm, shape, dtype=dt, **kw)
    return fft, spectral.SpectralOps(fft, R.BOX)


def _device_field(fft, G, m):
    """m = 3: a vector field (newDistArray rank 1); m = 1: a scalar field holding G[0]"""
    from mpi4py_fft_amd import newDistArray
    assert m in (1, 3) and G.shape[0] == m
    uh = newDistArray(fft, rank=1 if m == 3 else 0)
    uh[...] = np.array(G[(slice(None),) + fft.local_slice(True)] if m == 3 else G[0][fft.local_slice(True)])
    return uh


CASES = [
    ((24, 16, 20), 'd', 3), ((24, 16, 20), 'f', 3), ((24, 16, 20), 'd', 1),     # Nyquist column, rows of 11
    ((12, 10, 21), 'd', 3), ((12, 10, 21), 'f', 1),                              # odd: no Nyquist column
    ((10, 12, 14), 'D', 3), ((10, 12, 14), 'F', 1),                              # weights all one, |k2| rises then falls
    ((4, 6, 256), 'd', 3), ((4, 6, 256), 'f', 3),                                # rows of 129: longer than a wave
    ((72, 64, 6), 'd', 1), ((72, 64, 6), 'f', 3),                                # rows of 4: 16 rows per wave
    ((9, 5, 12), 'f', 3), ((9, 5, 12), 'd', 1),                                  # 315 modes, odd: fp32 takes the 8-byte loads
    ((96, 100, 112), 'd', 1), ((128, 100, 168), 'f', 1),                         # sweep: every workgroup steps twice
]


@pytest.mark.parametrize('shape,dt,m', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_spectrum_matches_the_fsum_reference(shape, dt, m):
    from mpi4py_fft_amd import comm
    G, k, w, ref, modes = _reference(shape, dt, m)
    if shape in ((96, 100, 112), (128, 100, 168)):
        assert G[0].size > SWEEP[dt.lower()], 'the shape no longer exceeds one sweep of the launch'
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    uh = _device_field(fft, G, m)
    got = ops.spectrum(uh)
    assert got.shape == (2, R.default_nbins(shape)) == ref.shape
    R.assert_bins(got, ref, modes, (shape, dt, m))
    if m == 1:                      # a scalar field is the one-component vector field
        R.assert_bins(ops.spectrum(uh.tensor[None]), ref, modes, (shape, dt, 'as [1] + shape'))
    assert abs(ops.energy(uh) - got[0].sum()) <= 1e-12 * got[0].sum() and abs(ops.enstrophy(uh) - got[1].sum()) <= 1e-12 * got[1].sum()
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('nbins', [5, 1])
def test_short_histograms_drop_the_outer_modes(dt, nbins):
    """nbins below the default: the bins equal the reference's first ones -- nothing is clipped into the last bin."""
    from mpi4py_fft_amd import comm
    shape, m = (24, 16, 20), 3
    G, k, w, ref, modes = _reference(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    got = ops.spectrum(_device_field(fft, G, m), nbins=nbins)
    assert got.shape == (2, nbins)
    R.assert_bins(got, np.ascontiguousarray(ref[:, :nbins]), modes[:nbins], (dt, nbins))
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('nbins', [2048, 4096])
def test_many_shells(dt, nbins):
    """Histograms of 2048 shells and of the documented limit, 4096 (all 64 KiB of LDS a workgroup gets), through an
    explicit dk = 1/128: every k_i / dk is still an integer, so still no ties.  The field's largest |k| / dk is 2063.9 (shell 2064):
    2048 shells drop the corner modes, 4096 hold everything and leave the upper half exactly zero."""
    from mpi4py_fft_amd import comm
    shape, m, dk = (24, 16, 20), 3, 1.0 / 128
    G = _reference(shape, dt, m)[0]
    k, w = R.wavenumbers(shape, True, dk=dk)
    ref, modes = R.reference(G, k, w, dk, nbins)
    assert modes.sum() < G[0].size if nbins == 2048 else (modes.sum() == G[0].size and modes[2064] > 0 and not modes[2065:].any())
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    got = ops.spectrum(_device_field(fft, G, m), nbins=nbins, dk=dk)
    R.assert_bins(got, ref, modes, (dt, nbins))
    assert np.array_equal(ops.shells(nbins, dk), np.arange(nbins) / 128)
    fft.destroy()


def test_misaligned_fp32_field():
    """u_hat starts 8 bytes into its allocation: an even mode count, but the kernel must take the 8-byte loads."""
    from mpi4py_fft_amd import comm
    shape, dt, m = (24, 16, 20), 'f', 3
    G, k, w, ref, modes = _reference(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    big = torch.zeros(G.size + 1, dtype=torch.complex64, device='cuda')
    uh = big[1:].view(G.shape)
    uh.copy_(torch.as_tensor(np.array(G)))
    assert uh.is_contiguous() and uh.data_ptr() % 16 == 8 and G[0].size % 2 == 0
    R.assert_bins(ops.spectrum(uh), ref, modes, 'u_hat off by 8 bytes')
    fft.destroy()


def test_more_shells_than_the_limit_is_an_error():
    from mpi4py_fft_amd import comm, _lib
    shape = (24, 16, 20)
    fft, ops = _ops(comm.COMM_SELF, shape, 'd')
    with pytest.raises(_lib.GfftError, match='unsupported'):
        ops.spectrum(_device_field(fft, _reference(shape, 'd', 3)[0], 3), nbins=4097, dk=1.0 / 128)
    fft.destroy()


# (shape, index into the spectral array, Hermitian weight)
SINGLE = {
    'k=0': ((24, 16, 20), (0, 0, 0), 1), 'k2=0': ((24, 16, 20), (3, 5, 0), 1), 'nyquist': ((24, 16, 20), (2, 3, 10), 1),
    'odd-last': ((12, 10, 21), (2, 3, 10), 2), 'most-negative-k0': ((24, 16, 20), (12, 1, 4), 2),
    'generic': ((24, 16, 20), (5, 7, 3), 2), 'generic-negative': ((12, 10, 21), (9, 8, 6), 2),
}


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('name', sorted(SINGLE))
def test_single_mode(name, dt):
    """u_hat zero but for one entry: exactly one bin is non-zero and holds w |a|^2 / 2 (row 1: times |k|^2) -- a wrong
    weight or a shell off by one shows undiluted."""
    from mpi4py_fft_amd import comm
    shape, idx, wt = SINGLE[name]
    k, w = R.wavenumbers(shape, True)
    assert w[idx[2]] == wt
    a = 0.75 - 1.25j                                    # |a|^2 = 2.125, exact in both precisions
    ksq = k[0][idx[0]] ** 2 + k[1][idx[1]] ** 2 + k[2][idx[2]] ** 2
    b = int(np.floor(np.sqrt(ksq) / R.DK + 0.5))
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    if name == 'most-negative-k0':
        assert k[0][idx[0]] == -shape[0] // 2
    uh = _device_field(fft, np.zeros((1,) + tuple(fft.global_shape(True)), dtype=fft.dtype(True)), 1)
    uh[idx] = a
    got = ops.spectrum(uh)
    want = np.zeros_like(got)
    want[0, b] = 0.5 * wt * 2.125
    want[1, b] = ksq * want[0, b]
    modes = np.zeros(got.shape[1], dtype=int)
    modes[b] = 1
    assert np.count_nonzero(got[0]) == 1 and np.count_nonzero(got[1]) == (1 if ksq else 0), (name, got)
    R.assert_bins(got, want, modes, name)
    fft.destroy()


@pytest.mark.parametrize('shape,dt', [((24, 16, 20), 'd'), ((12, 10, 21), 'f'), ((10, 12, 14), 'D')])
def test_parseval(shape, dt):
    """sum_k E(k) of the forward-normalised transform = <u.u>/2 in physical space, to the transform's rounding"""
    from mpi4py_fft_amd import comm, newDistArray
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    rng = np.random.default_rng(5)
    U = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if dt == 'D' else 0)
    u = newDistArray(fft, False)
    u[...] = U.astype(dt)
    want = 0.5 * float(np.mean(np.abs(U.astype(dt).astype('D')) ** 2))
    got = ops.energy(fft.forward(u))
    tol = cases.rounding_tol(dt, int(np.prod(shape)))
    print('parseval %s %s: rel err %.3e (tol %.3e)' % (shape, dt, abs(got - want) / want, tol))
    assert abs(got - want) <= tol * want
    fft.destroy()


@pytest.mark.parametrize('P,grid', [(2, [2, 1, 1]), (4, [4, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'slab4', 'pencil4'])
@pytest.mark.parametrize('shape,dt', [((24, 16, 20), 'd'), ((12, 10, 21), 'f')])
def test_thread_ranks(P, grid, shape, dt):
    """Every rank holds the same bins bit for bit, and they match the one-rank result within the bound."""
    from mpi4py_fft_amd import comm
    m = 3 if dt == 'd' else 1
    G, k, w, ref, modes = _reference(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    one = ops.spectrum(_device_field(fft, G, m))
    fft.destroy()

    def body(c):
        fft, ops = _ops(c, shape, dt, grid=grid)
        got = ops.spectrum(_device_field(fft, G, m))
        local = fft.shape(True)
        fft.destroy()
        return got, tuple(local)
    res = cases.run_ranks(P, body)
    if grid[1] > 1:
        assert any(loc[2] < len(k[2]) for _, loc in res), 'the halved axis was not distributed'
    for got, _ in res:
        assert np.array_equal(got, res[0][0]), 'ranks disagree'
        R.assert_bins(got, ref, modes, (P, grid, 'vs reference'))
        assert np.all(np.abs(got - one) <= (modes + 16) * 2.0 ** -52 * ref), (P, grid, 'vs one rank')


def test_example_returns_the_spectrum():
    """examples/dns_taylor_green.py at 64^3: sum E(k) of the final U_hat is the solver's known answer."""
    import importlib.util
    import os
    from mpi4py_fft_amd import comm
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_spectrum', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    energy, E = mod.solve(comm.COMM_SELF, spectrum=True)
    assert round(energy - 0.124953117517, 7) == 0, energy
    assert E.shape[0] == 2 and E.dtype == np.float64
    assert round(float(E[0].sum()) - 0.124953117517, 7) == 0, E[0].sum()
    assert isinstance(mod.solve(comm.COMM_SELF, nsteps=1), float)          # the default return value is unchanged


def test_replay_from_a_captured_graph():
    """reduce=False with out= only enqueues the kernels and allocates nothing after the first call.  The replayed bins
    are held to the same bound as the eager ones (the waves of a workgroup add to its histogram in arrival order: bins
    repeat to rounding, not bit for bit)."""
    from mpi4py_fft_amd import comm
    shape, dt, m = (24, 16, 20), 'd', 3
    G, k, w, ref, modes = _reference(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    uh = _device_field(fft, G, m)
    nb = ref.shape[1]
    out = torch.zeros((2, nb), dtype=torch.float64, device=uh.tensor.device)
    assert ops.spectrum(uh, out=out, reduce=False) is out
    torch.cuda.synchronize()
    eager = out.cpu().numpy().copy()
    R.assert_bins(eager, ref, modes, 'eager')
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.spectrum(uh, out=out, reduce=False)          # warm-up on another stream: its scratch exists now
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.spectrum(uh, out=out, reduce=False)
    for _ in range(2):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().copy()
        R.assert_bins(got, ref, modes, 'replay')
        assert np.all(np.abs(got - eager) <= (modes + 16) * 2.0 ** -52 * ref)
    fft.destroy()
