"""gfft_ps_cospectrum / SpectralOps.cospectrum, transfer, helicity_spectrum on the device against the fsum reference of
tests/cospectrum_ref.py.

Bound (derived there, not measured): per bin |got - ref| <= (modes in the bin + 16) 2^-52 A with A the bin's sum of
ABSOLUTE terms, in both precisions; empty bins exactly 0.  Boxes without shell-boundary ties only (L = (2 pi, 4 pi, 2 pi),
dk = 1/2), except where a test names its own box.

The launch geometry is the spectrum's (tests/test_gpu_spectrum.py): 256 lanes, V modes per lane, at most 2048
workgroups, a second step per workgroup only beyond 2048 * 256 * V modes.  New here: V = 2 (fp32) needs BOTH fields
16-byte aligned, and the addends are signed.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, cospectrum_ref as C, spectrum_ref as R

SWEEP = {'d': 2048 * 256 * 1, 'f': 2048 * 256 * 2}
# (shape, index into the spectral array, Hermitian weight): the entries of tests/test_gpu_spectrum.py's SINGLE table that
# cover k = 0, k2 = 0, the Nyquist column, an odd last axis and the most negative k0
SINGLE = {
    'k=0': ((24, 16, 20), (0, 0, 0), 1), 'k2=0': ((24, 16, 20), (3, 5, 0), 1), 'nyquist': ((24, 16, 20), (2, 3, 10), 1),
    'odd-last': ((12, 10, 21), (2, 3, 10), 2), 'most-negative-k0': ((24, 16, 20), (12, 1, 4), 2),
}


def _field(shape, dt, m, seed):
    real = dt in 'fd'
    gs = tuple(shape[:2]) + ((shape[2] // 2 + 1) if real else shape[2],)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m,) + gs) + 1j * rng.standard_normal((m,) + gs)).astype('D' if dt in 'dD' else 'F')


_REF = {}


def _reference(shape, dt, m, op=C.DOT):
    """(a, b, k, w, bins, modes per bin, A) -- computed once per case and shared, never modified"""
    key = (tuple(shape), dt, m, op)
    if key not in _REF:
        GA, GB = _field(shape, dt, m, 11), _field(shape, dt, m, 12)
        k, w = R.wavenumbers(shape, dt in 'fd')
        bins, modes, A = C.reference(GA, GB, k, w, op)
        for x in (GA, GB, bins, modes, A):
            x.setflags(write=False)
        _REF[key] = (GA, GB, k, w, bins, modes, A)
    return _REF[key]


def _ops(comm, shape, dt, L=R.BOX, **kw):
    from mpi4py_fft_amd import PFFT, spectral
    fft = PFFT(comm, shape, dtype=dt, **kw)
    return fft, spectral.SpectralOps(fft, L)


def _device_field(fft, G, m):
    """m = 3: a vector field (newDistArray rank 1); m = 1: a scalar field holding G[0]"""
    from mpi4py_fft_amd import newDistArray
    assert m in (1, 3) and G.shape[0] == m
    uh = newDistArray(fft, rank=1 if m == 3 else 0)
    uh[...] = np.array(G[(slice(None),) + fft.local_slice(True)] if m == 3 else G[0][fft.local_slice(True)])
    return uh


DOT_CASES = [
    ((24, 16, 20), 'd', 3), ((24, 16, 20), 'f', 3),                              # Nyquist column, rows of 11
    ((12, 10, 21), 'f', 1),                                                      # odd last axis
    ((10, 12, 14), 'D', 3),                                                      # complex transform
    ((4, 6, 256), 'f', 3),                                                       # rows of 129: longer than a wave
    ((72, 64, 6), 'd', 1),                                                       # rows of 4
    ((9, 5, 12), 'f', 3),                                                        # 315 modes, odd: the 8-byte loads
    ((96, 100, 112), 'd', 1), ((128, 100, 168), 'f', 1),                         # sweep: every workgroup steps twice
]


@pytest.mark.parametrize('shape,dt,m', DOT_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_dot_matches_the_fsum_reference(shape, dt, m):
    from mpi4py_fft_amd import comm
    GA, GB, k, w, ref, modes, A = _reference(shape, dt, m)
    if shape in ((96, 100, 112), (128, 100, 168)):
        assert GA[0].size > SWEEP[dt.lower()], 'the shape no longer exceeds one sweep of the launch'
    assert (ref[0] < 0).any() and (ref[0] > 0).any()
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    ah, bh = _device_field(fft, GA, m), _device_field(fft, GB, m)
    got = ops.cospectrum(ah, bh)
    assert got.shape == (2, R.default_nbins(shape)) == ref.shape
    C.assert_bins(got, ref, modes, A, (shape, dt, m))
    C.assert_bins(ops.transfer(ah, bh), ref, modes, A, (shape, dt, m, 'transfer'))
    C.assert_bins(ops.cospectrum(ah, bh, scale=-0.375), -0.375 * ref, modes, 0.375 * A, (shape, dt, m, 'scale'))
    fft.destroy()


@pytest.mark.parametrize('shape,dt', [((24, 16, 20), 'd'), ((12, 10, 21), 'f'), ((10, 12, 14), 'D'), ((4, 6, 256), 'f'),
                                      ((96, 100, 112), 'd')], ids=lambda v: str(v).replace(' ', ''))
def test_helicity_matches_the_fsum_reference(shape, dt):
    """... and agrees, within the sum of both bounds, with the co-spectrum of u_hat and a stored curl.  The stored curl
    is formed in double in every case (for an fp32 field from its exactly converted copy, on a double transform of the
    same shape): both sides then see the same numbers, and the curl's own rounding, at most three per term relative to
    the absolute terms A counts, sits inside the sixteen the bound allows."""
    from mpi4py_fft_amd import comm, newDistArray
    GA, _, k, w, ref, modes, A = _reference(shape, dt, 3, C.HELICITY)
    if shape == (96, 100, 112):
        assert GA[0].size > SWEEP['d']
    assert (ref[0] < 0).any() and (ref[0] > 0).any()
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    uh = _device_field(fft, GA, 3)
    got = ops.helicity_spectrum(uh)
    C.assert_bins(got, ref, modes, A, (shape, dt, 'helicity'))
    assert abs(ops.helicity(uh) - got[0].sum()) <= 2.0 ** -40 * A[0].sum()
    if dt == 'f':
        fft.destroy()
        fft, ops = _ops(comm.COMM_SELF, shape, 'd')
        uh = _device_field(fft, GA.astype('D'), 3)
    wh = ops.curl(uh, newDistArray(fft, rank=1))
    dot = ops.cospectrum(uh, wh)
    _, _, A2 = C.reference(GA, np.asarray(wh), k, w)
    both = C.bound(modes, A) + C.bound(modes, A2)
    worst = float((np.abs(got - dot) / np.maximum(both, 1e-300)).max())
    print('%s %s: helicity vs cospectrum(u, curl u): worst / (sum of bounds) = %.3f' % (shape, dt, worst))
    assert np.all(np.abs(got - dot) <= both)
    fft.destroy()


def test_misaligned_fp32_operand():
    """b_hat starts 8 bytes into its allocation: an even mode count, but the kernel must take the 8-byte loads."""
    from mpi4py_fft_amd import comm
    shape, dt, m = (24, 16, 20), 'f', 3
    GA, GB, k, w, ref, modes, A = _reference(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    ah = _device_field(fft, GA, m)
    big = torch.zeros(GB.size + 1, dtype=torch.complex64, device=ah.tensor.device)
    bh = big[1:].view(GB.shape)
    bh.copy_(torch.as_tensor(np.array(GB)))
    assert bh.is_contiguous() and bh.data_ptr() % 16 == 8 and ah.tensor.data_ptr() % 16 == 0 and GA[0].size % 2 == 0
    C.assert_bins(ops.cospectrum(ah, bh), ref, modes, A, 'b_hat off by 8 bytes')
    ref_ba = C.reference(GB, GA, k, w)[0]
    C.assert_bins(ops.cospectrum(bh, ah), ref_ba, modes, A, 'a_hat off by 8 bytes')
    fft.destroy()


@pytest.mark.parametrize('shape,dt,m', [((24, 16, 20), 'd', 3), ((24, 16, 20), 'f', 3), ((12, 10, 21), 'f', 1), ((10, 12, 14), 'D', 3)],
                         ids=lambda v: str(v).replace(' ', ''))
def test_cospectrum_of_a_field_with_itself_is_its_spectrum(shape, dt, m):
    from mpi4py_fft_amd import comm
    GA = _reference(shape, dt, m)[0]
    k, w = R.wavenumbers(shape, dt in 'fd')
    ref, modes = R.reference(GA, k, w)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    uh = _device_field(fft, GA, m)
    same, E = ops.cospectrum(uh, uh, scale=0.5), ops.spectrum(uh)
    R.assert_bins(same, ref, modes, (shape, dt, 'cospectrum(u, u, 0.5) vs the spectrum reference'))
    assert np.all(np.abs(same - E) <= (modes + 16) * 2.0 ** -52 * ref), 'cospectrum(u, u, 0.5) is not spectrum(u)'
    fft.destroy()


def _single(name):
    shape, idx, wt = SINGLE[name]
    k, w = R.wavenumbers(shape, True)
    assert w[idx[2]] == wt
    kv = np.array([k[0][idx[0]], k[1][idx[1]], k[2][idx[2]]])
    if name == 'most-negative-k0':
        assert kv[0] == -shape[0] // 2
    return shape, idx, wt, k, w, kv, int(np.floor(np.sqrt((kv ** 2).sum()) / R.DK + 0.5))


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('name', sorted(SINGLE))
def test_single_mode(name, dt):
    """Both fields zero but for one entry (values exact in both precisions): exactly one bin is non-zero and holds
    w Re(conj(a) b) -- negative here -- and, row 1, |k|^2 times it."""
    from mpi4py_fft_amd import comm
    shape, idx, wt, k, w, kv, b = _single(name)
    a, bv = 0.75 - 1.25j, -0.5 + 0.25j                   # Re(conj(a) b) = -0.375 - 0.3125 = -0.6875
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    gs = tuple(fft.global_shape(True))
    GA, GB = np.zeros((1,) + gs, dtype=fft.dtype(True)), np.zeros((1,) + gs, dtype=fft.dtype(True))
    GA[(0,) + idx], GB[(0,) + idx] = a, bv
    got = ops.cospectrum(_device_field(fft, GA, 1), _device_field(fft, GB, 1))
    ksq = float((kv ** 2).sum())
    want = np.zeros_like(got)
    want[0, b] = wt * -0.6875
    want[1, b] = ksq * want[0, b]
    assert np.array_equal(got, want), (name, got[:, b], want[:, b])
    assert np.count_nonzero(got[0]) == 1 and np.count_nonzero(got[1]) == (1 if ksq else 0)
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('name', sorted(SINGLE))
def test_single_mode_helicity(name, dt):
    """One mode with Re a = r, Im a = m (exact in both precisions): the only non-zero bin holds w 2 K . (r x m)."""
    from mpi4py_fft_amd import comm
    shape, idx, wt, k, w, kv, b = _single(name)
    r, m = np.array([0.75, -0.5, 0.25]), np.array([0.5, 1.25, -1.0])
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    G = np.zeros((3,) + tuple(fft.global_shape(True)), dtype=fft.dtype(True))
    G[(slice(None),) + idx] = r + 1j * m
    got = ops.helicity_spectrum(_device_field(fft, G, 3))
    h = wt * 2.0 * float(np.dot(kv, np.cross(r, m)))     # (small dyadic numbers: exact)
    assert (h == 0.0) == (name == 'k=0')
    ref, modes, A = C.reference(G, None, k, w, C.HELICITY)
    assert ref[0, b] == h and np.count_nonzero(ref[0]) == (1 if h else 0)
    C.assert_bins(got, ref, modes, A, name)
    assert np.count_nonzero(got[0]) == (1 if h else 0) and (got[1, b] == float((kv ** 2).sum()) * got[0, b])
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('sign', [1, -1])
def test_helical_mode_saturates_realizability(sign, dt):
    """u_hat = alpha (1, +-i, 0) at K = (0, 0, 4): H = +-2 |K| E there, the closed form of a helical wave."""
    from mpi4py_fft_amd import comm
    shape, idx, alpha = (24, 16, 20), (0, 0, 4), 0.75
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    G = np.zeros((3,) + tuple(fft.global_shape(True)), dtype=fft.dtype(True))
    G[(0,) + idx], G[(1,) + idx] = alpha, sign * 1j * alpha
    uh = _device_field(fft, G, 3)
    H, E = ops.helicity_spectrum(uh), ops.spectrum(uh)
    want = np.zeros_like(H)
    want[0, 8] = sign * 2 * 2.0 * 4.0 * alpha ** 2       # w 2 kz alpha^2, shell |K| / dk = 8
    want[1, 8] = 16.0 * want[0, 8]
    assert np.array_equal(H, want) and H[0, 8] == sign * 2 * 4.0 * E[0, 8] and ops.helicity(uh) == want[0, 8]
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('nbins', [5, 1])
def test_short_histograms_drop_the_outer_modes(dt, nbins):
    from mpi4py_fft_amd import comm
    shape, m = (24, 16, 20), 3
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    GA, GB, k, w, ref, modes, A = _reference(shape, dt, m)
    ah, bh = _device_field(fft, GA, m), _device_field(fft, GB, m)
    got = ops.cospectrum(ah, bh, nbins=nbins)
    assert got.shape == (2, nbins)
    C.assert_bins(got, np.ascontiguousarray(ref[:, :nbins]), modes[:nbins], np.ascontiguousarray(A[:, :nbins]), (dt, nbins))
    _, _, _, _, href, _, hA = _reference(shape, dt, m, C.HELICITY)
    C.assert_bins(ops.helicity_spectrum(ah, nbins=nbins), np.ascontiguousarray(href[:, :nbins]), modes[:nbins],
                  np.ascontiguousarray(hA[:, :nbins]), (dt, nbins, 'helicity'))
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_the_longest_histogram(dt):
    """4096 shells, the documented limit, through dk = 1/128 (every k_i / dk still an integer): everything is held, the
    last occupied shell is 2064 and the upper half is exactly zero.  One more shell is refused."""
    from mpi4py_fft_amd import comm, _lib
    shape, m, dk, nbins = (24, 16, 20), 3, 1.0 / 128, 4096
    GA, GB = _reference(shape, dt, m)[:2]
    k, w = R.wavenumbers(shape, True, dk=dk)
    ref, modes, A = C.reference(GA, GB, k, w, C.DOT, 1.0, dk, nbins)
    assert modes.sum() == GA[0].size and modes[2064] > 0 and not modes[2065:].any()
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    ah, bh = _device_field(fft, GA, m), _device_field(fft, GB, m)
    C.assert_bins(ops.cospectrum(ah, bh, nbins=nbins, dk=dk), ref, modes, A, (dt, nbins))
    with pytest.raises(_lib.GfftError, match='unsupported'):
        ops.cospectrum(ah, bh, nbins=4097, dk=dk)
    with pytest.raises(_lib.GfftError, match='unsupported'):
        ops.helicity_spectrum(ah, nbins=4097, dk=dk)
    fft.destroy()


@pytest.mark.parametrize('shape,dt', [((24, 16, 20), 'd'), ((12, 10, 21), 'f'), ((10, 12, 14), 'D')])
def test_parseval(shape, dt):
    """sum_k of the co-spectrum of two forward-normalised transforms = <a.b> in physical space (Re <conj(a) b> for
    complex fields), to the transforms' rounding"""
    from mpi4py_fft_amd import comm, newDistArray
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    rng = np.random.default_rng(5)
    hats, phys = [], []
    for _ in range(2):
        U = (rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if dt == 'D' else 0)).astype(dt)
        u = newDistArray(fft, False)
        u[...] = U
        hats.append(fft.forward(u, newDistArray(fft, True)))
        phys.append(U.astype('D'))
    want = float(np.mean((np.conj(phys[0]) * phys[1]).real))
    norm = float(np.sqrt(np.mean(np.abs(phys[0]) ** 2) * np.mean(np.abs(phys[1]) ** 2)))
    got = float(ops.cospectrum(hats[0], hats[1])[0].sum())
    tol = cases.rounding_tol(dt, int(np.prod(shape)))
    print('parseval %s %s: |got - want| / norm = %.3e (tol %.3e)' % (shape, dt, abs(got - want) / norm, tol))
    assert abs(got - want) <= tol * norm
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_abc_flow(dt):
    """u = (A sin z + C cos y, B sin x + A cos z, C sin y + B cos x) on (2 pi)^3 is its own curl: all helicity sits in
    shell 1, H(1) = 2 E(1) = A^2 + B^2 + C^2."""
    from mpi4py_fft_amd import comm, newDistArray
    n, (A, B, Cc) = 16, (1.0, 0.5, 0.25)
    fft, ops = _ops(comm.COMM_SELF, (n, n, n), dt, L=None)
    assert ops.dk == 1.0
    x, y, z = np.meshgrid(*[np.arange(n) * 2 * np.pi / n] * 3, indexing='ij')
    U = np.stack([A * np.sin(z) + Cc * np.cos(y), B * np.sin(x) + A * np.cos(z), Cc * np.sin(y) + B * np.cos(x)]).astype(dt)
    u, uh = newDistArray(fft, False, rank=1), newDistArray(fft, rank=1)
    u[...] = U
    for j in range(3):
        fft.forward(u[j], uh[j])
    H, E = ops.helicity_spectrum(uh), ops.spectrum(uh)
    want = A * A + B * B + Cc * Cc
    assert want == 1.3125
    tol = cases.rounding_tol(dt, n ** 3) * want
    print('ABC %s: H(1) - %.4f = %.3e, 2 E(1) - H(1) = %.3e, largest other bin %.3e (tol %.3e)'
          % (dt, want, H[0, 1] - want, 2 * E[0, 1] - H[0, 1], np.abs(np.delete(H[0], 1)).max(), tol))
    assert abs(H[0, 1] - want) <= tol and abs(2 * E[0, 1] - want) <= tol
    assert np.all(np.abs(np.delete(H[0], 1)) <= tol)
    assert abs(ops.helicity(uh) - want) <= tol
    fft.destroy()


@pytest.mark.parametrize('shape,dt', [((12, 10, 21), 'd'), ((16, 16, 16), 'f')])
def test_rotational_form_conserves_energy(shape, dt):
    """N = u x curl u is orthogonal to u at every grid point, so sum_k T(k) = <u.N> = 0 exactly in exact arithmetic,
    aliasing included: what is left is the rounding of the four transforms, relative to 2 sqrt(E(u) E(N))."""
    from mpi4py_fft_amd import comm, newDistArray, spectral
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    rng = np.random.default_rng(9)
    u, w, n = (newDistArray(fft, False, rank=1) for _ in range(3))
    uh, wh, nh = (newDistArray(fft, rank=1) for _ in range(3))
    u[...] = rng.standard_normal((3,) + tuple(shape)).astype(dt)
    for j in range(3):
        fft.forward(u[j], uh[j])
    ops.curl(uh, wh)
    for j in range(3):
        fft.backward(wh[j], w[j])
    spectral.cross(u, w, n)
    for j in range(3):
        fft.forward(n[j], nh[j])
    T = ops.transfer(uh, nh)
    scale = 2 * np.sqrt(ops.energy(uh) * ops.energy(nh))
    tol = cases.rounding_tol(dt, int(np.prod(shape)))
    print('rotational form %s %s: |sum T| / (2 sqrt(E_u E_N)) = %.3e (tol %.3e); max |T| = %.3e'
          % (shape, dt, abs(T[0].sum()) / scale, tol, np.abs(T[0]).max()))
    assert np.abs(T[0]).max() > 100 * tol * scale, 'T(k) itself vanishes: the case shows nothing'
    assert abs(T[0].sum()) <= tol * scale
    assert abs(spectral.flux(T)[-1] + T[0].sum()) <= 2.0 ** -40 * np.abs(T[0]).sum()
    fft.destroy()


@pytest.mark.parametrize('P,grid', [(2, [2, 1, 1]), (4, [4, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'slab4', 'pencil4'])
@pytest.mark.parametrize('shape,dt', [((24, 16, 20), 'd'), ((12, 10, 21), 'f')])
def test_thread_ranks(P, grid, shape, dt):
    """Every rank holds the same bins bit for bit, and they match the reference within the bound, for both ops."""
    from mpi4py_fft_amd import comm
    GA, GB, k, w, ref, modes, A = _reference(shape, dt, 3)
    _, _, _, _, href, _, hA = _reference(shape, dt, 3, C.HELICITY)

    def body(c):
        fft, ops = _ops(c, shape, dt, grid=grid)
        ah, bh = _device_field(fft, GA, 3), _device_field(fft, GB, 3)
        got, hel = ops.cospectrum(ah, bh), ops.helicity_spectrum(ah)
        local = fft.shape(True)
        fft.destroy()
        return got, hel, tuple(local)
    res = cases.run_ranks(P, body)
    if grid[1] > 1:
        assert any(loc[2] < len(k[2]) for _, _, loc in res), 'the halved axis was not distributed'
    for got, hel, _ in res:
        assert np.array_equal(got, res[0][0]) and np.array_equal(hel, res[0][1]), 'ranks disagree'
        C.assert_bins(got, ref, modes, A, (P, grid, 'dot'))
        C.assert_bins(hel, href, modes, hA, (P, grid, 'helicity'))


def test_example_returns_the_transfer_spectrum():
    """examples/dns_taylor_green.py at 64^3: the energy is the solver's known answer and the nonlinear term of the final
    state moves energy between shells without creating any (the bound of test_rotational_form_conserves_energy)."""
    import importlib.util
    import os
    from mpi4py_fft_amd import comm, spectral
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_transfer', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    st = {}
    energy, T = mod.solve(comm.COMM_SELF, transfer=True, stats=st)
    assert round(energy - 0.124953117517, 7) == 0, energy
    assert T.shape[0] == 2 and T.dtype == np.float64
    tol = cases.rounding_tol('d', 64 ** 3) * 2 * np.sqrt(energy * st['nonlinear_energy'])    # (energy = energy(U_hat))
    print('example: sum T = %.3e (tol %.3e), max |T| = %.3e, max |flux| = %.3e'
          % (T[0].sum(), tol, np.abs(T[0]).max(), np.abs(spectral.flux(T)).max()))
    assert np.abs(T[0]).max() > 0 and abs(T[0].sum()) <= tol
    assert abs(st['helicity']) <= cases.rounding_tol('d', 64 ** 3) * 2 * energy, 'the Taylor-Green vortex has no helicity'
    assert isinstance(mod.solve(comm.COMM_SELF, nsteps=1), float)          # the default return value is unchanged


@pytest.mark.parametrize('op', ['dot', 'helicity'])
def test_replay_from_a_captured_graph(op):
    """reduce=False with out= only enqueues the kernels and allocates nothing after the first call.  The replayed bins
    are held to the same bound as the eager ones, against the reference and against each other."""
    from mpi4py_fft_amd import comm
    shape, dt, m = (24, 16, 20), 'd', 3
    GA, GB, k, w, ref, modes, A = _reference(shape, dt, m, C.DOT if op == 'dot' else C.HELICITY)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    ah, bh = _device_field(fft, GA, m), _device_field(fft, GB, m)
    out = torch.zeros((2, ref.shape[1]), dtype=torch.float64, device=ah.tensor.device)

    def run():
        return ops.cospectrum(ah, bh, out=out, reduce=False) if op == 'dot' else ops.helicity_spectrum(ah, out=out, reduce=False)
    assert run() is out
    torch.cuda.synchronize()
    eager = out.cpu().numpy().copy()
    C.assert_bins(eager, ref, modes, A, 'eager')
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run()                                            # warm-up on another stream: its scratch exists now
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(2):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().copy()
        C.assert_bins(got, ref, modes, A, 'replay')
        assert np.all(np.abs(got - eager) <= C.bound(modes, A))
    fft.destroy()
