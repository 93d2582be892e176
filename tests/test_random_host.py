"""Host logic of the random fields (no GPU): the reference's Philox against the Random123 known answers, the properties the
definition promises checked on the reference itself (tests/random_ref.py), `model_spectrum`, the Python wrappers
(`random_solenoidal`, `scale_shells`, `random_field`, `white_noise_force`) over a numpy stand-in for the kernels, on one rank and
two, and the argument checks of gfft_ps_random_field / gfft_ps_scale_shells that need no device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases, random_ref as R
from tests.host_engine import HostEngine

SHAPES = [(8, 8, 8), (6, 10, 8), (7, 9, 5)]


class RandomEngine(HostEngine):
    """HostEngine plus the kernels `SpectralOps` calls here, restated with numpy (tests/random_ref.py) on host tensors."""
    seen = []

    def ps_random_field(self, tout, ncomp, n, start, N, k, project, dk, tamp, nbins, seed, stream_id, add, precision):
        RandomEngine.seen.append(dict(ncomp=int(ncomp), n=tuple(n), start=tuple(start), N=tuple(N), project=bool(project), dk=dk,
                                      nbins=int(nbins), seed=seed, stream=stream_id, add=bool(add), amp=tamp is not None))
        assert tout.numel() == ncomp * int(np.prod(n))
        G, zero, _ = R.random_field(n, start, N, [ki.numpy() for ki in k], seed, stream_id, ncomp, project, dk,
                                    None if tamp is None else tamp.numpy(), nbins)
        v = torch.as_tensor(G.astype(np.complex128 if precision == 8 else np.complex64)).reshape(tout.shape)
        if add:
            tout += v
        else:
            tout.copy_(v)

    def ps_scale_shells(self, tf, tout, ncomp, k, dk, ttab, nbins, shape, precision):
        f = tf.numpy().reshape((ncomp,) + tuple(shape))
        tout.copy_(torch.as_tensor(R.scale_shells(f, [ki.numpy() for ki in k], ttab.numpy()[:nbins], dk)).reshape(tout.shape))

    def ps_spectrum(self, tu, ncomp, k, w, shape, dk, nbins, tout, precision):
        f = tu.numpy().reshape((ncomp,) + tuple(shape))
        tout.zero_()
        tout[0].copy_(torch.as_tensor(R.spectrum(f, [ki.numpy() for ki in k], w.numpy(), dk, nbins)))

    def ps_rk_stage(self, tu, tu0, tu1, tdu, count, cb, ca, precision):
        assert tu is None
        tu1 += ca * tdu


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(RandomEngine())
    RandomEngine.seen = []
    yield
    _lib.set_engine(old)


def test_philox_known_answers():
    """Philox4x32-10 of Random123 (kat_vectors): counter, key -> output"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in R.philox4x32(ctr, key)) == want
    # on arrays: every lane its own counter
    r = R.philox4x32((np.array([0, 0x243f6a88], dtype=np.uint64), np.array([0, 0x85a308d3], dtype=np.uint64),
                      np.array([0, 0x13198a2e], dtype=np.uint64), np.array([0, 0x03707344], dtype=np.uint64)), (0, 0))
    assert int(r[0][0]) == 0x6627e8d5 and int(r[0][1]) != 0x6627e8d5
    # the uniforms: exact doubles strictly inside (0, 1), the centres of 2^52 cells
    lo, hi = np.array([0, 0xffffffff], dtype=np.uint64), np.array([0, 0xffffffff], dtype=np.uint64)
    u = R.uniform(lo, hi)
    assert u[0] == 2.0 ** -53 and u[1] == 1.0 - 2.0 ** -53 and 0 < u[0] and u[1] < 1


def _mirror(G, N):
    idx = [(-np.arange(n)) % n for n in N]
    return G[:, idx[0]][:, :, idx[1]][:, :, :, idx[2]]


@pytest.mark.parametrize('N,share', list(zip(SHAPES, (0.33, 0.35, 0.003))))
def test_reference_field_is_hermitian_real_and_solenoidal(N, share):
    G, zero, gnorm = R.full_field(N, False, 7, 0)
    assert np.array_equal(_mirror(G, N), np.conj(G))                     # bit for bit
    assert np.array_equal(_mirror(zero[None], N)[0], zero) and zero[0, 0, 0]
    u = np.fft.ifftn(G.astype(np.complex128), axes=(1, 2, 3))
    assert np.abs(u.imag).max() <= 1e-16 * max(1.0, np.abs(u.real).max()) * 10
    K = np.meshgrid(*R.wavenumbers(N, False), indexing='ij')
    assert float(np.abs(sum(K[j] * G[j] for j in range(3))).max()) <= 3e-15
    assert abs(zero.mean() - share) < 0.005
    for a in range(3):                                                   # Nyquist planes of the even axes
        if N[a] % 2 == 0:
            assert zero.take(N[a] // 2, axis=a).all()
    # the r2c field is the stored half of the c2c field, and a block is a slice of the whole
    Gr, zr, _ = R.full_field(N, True, 7, 0)
    assert np.array_equal(Gr, G[..., :N[2] // 2 + 1]) and np.array_equal(zr, zero[..., :N[2] // 2 + 1])
    n, start = (N[0] - 2, 2, N[2] - 1), (1, N[1] - 3, 1)
    sl = tuple(slice(s, s + m) for s, m in zip(start, n))
    Gb, _, _ = R.random_field(n, start, N, [k[s] for k, s in zip(R.wavenumbers(N, False), sl)], 7, 0)
    assert np.array_equal(Gb, G[(slice(None),) + sl])
    # another stream, seed or component: other numbers on every surviving mode
    for other in (R.full_field(N, False, 7, 1)[0], R.full_field(N, False, 8, 0)[0]):
        assert (other[:, ~zero] != G[:, ~zero]).any(axis=0).all()        # (per mode: the projection zeroes a component along K)
    P = R.full_field(N, False, 7, 0, ncomp=4, project=False)[0]
    assert len({complex(P[c][~zero][0]) for c in range(4)}) == 4


def test_reference_statistics():
    """32^3, seed 7, stream 0: mean sum_c |u_c|^2 within 5 standard errors of 4; two streams uncorrelated"""
    N = (32, 32, 32)
    G, zero, _ = R.full_field(N, True, 7, 0)
    e = (np.abs(G) ** 2).sum(axis=0)[~zero].astype(np.float64)
    assert abs(e.mean() - 4.0) <= 5 * e.std() / np.sqrt(e.size)
    H = R.full_field(N, True, 7, 1)[0]
    a, b = G[:, ~zero].astype(np.complex128).ravel(), H[:, ~zero].astype(np.complex128).ravel()
    corr = abs(np.vdot(a, b)) / np.sqrt(np.vdot(a, a).real * np.vdot(b, b).real)
    assert corr <= 5 / np.sqrt(e.size)
    # without the projection every part is a standard normal: 2 per component
    P = R.full_field(N, True, 7, 0, ncomp=1, project=False)[0]
    p = (np.abs(P[0]) ** 2)[~zero].astype(np.float64)
    assert abs(p.mean() - 2.0) <= 5 * p.std() / np.sqrt(p.size)


def test_bound_constant_is_derived_and_small():
    assert R.BOUND_C == 20 and R.BOUND_C <= 64


def test_model_spectrum():
    from mpi4py_fft_amd import spectral
    k = np.arange(56, dtype=np.float64)
    for kind in ('gaussian', 'karman'):
        E = spectral.model_spectrum(k, kind, 4.0, 0.7)
        assert E.shape == k.shape and E[0] == 0 and (E[1:] > 0).all()
        assert abs(E.sum() - 1.5 * 0.49) <= 1e-15
    g = spectral.model_spectrum(k, 'gaussian', 4.0, 1.0)
    assert int(np.argmax(g)) == 4                                        # d/dk k^4 exp(-2 k^2 / kp^2) = 0 at k = kp
    assert np.allclose(g[2] / g[1], 16 * np.exp(-2 * 3 / 16.0), rtol=1e-14)
    v = spectral.model_spectrum(k, 'karman', 2.0, 1.0)
    assert np.allclose(v[40] / v[20], 16 * (101.0 / 401.0) ** (17.0 / 6.0), rtol=1e-13)
    assert abs(np.log(v[40] / v[20]) / np.log(2.0) + 5.0 / 3.0) < 0.05                   # the inertial slope far above k_peak
    for bad in (dict(kind='pao'), dict(k_peak=0.0), dict(u_rms=-1.0), dict(k=np.zeros(3))):
        kw = dict(k=k, kind='gaussian', k_peak=4.0, u_rms=1.0)
        kw.update(bad)
        with pytest.raises(AssertionError):
            spectral.model_spectrum(**kw)


def test_random_field_table_on_the_reference():
    """fill at unit amplitude, spectrum, table, scale_shells: the shell spectrum of the result is E to rounding"""
    from mpi4py_fft_amd import spectral
    N = (12, 10, 16)
    K = R.wavenumbers(N, True)
    nb = 8
    G = R.full_field(N, True, 3, 0, nbins=nb)[0].astype(np.complex128)
    w2 = np.full(N[2] // 2 + 1, 2.0)
    w2[0] = w2[-1] = 1.0
    have = R.spectrum(G, K, w2, 1.0, nb)
    E = spectral.model_spectrum(np.arange(nb), 'gaussian', 3.0, 1.0)
    tab = R.shell_table(E, have)
    assert tab[0] == 0 and have[0] == 0 and (tab[1:] > 0).all()
    got = R.spectrum(R.scale_shells(G, K, tab, 1.0), K, w2, 1.0, nb)
    assert np.allclose(got[1:], E[1:], rtol=1e-12, atol=0) and got[0] == 0


def test_wrappers_on_one_rank(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    N = (8, 6, 20)
    fft = PFFT(comm.COMM_SELF, N, dtype='d')
    ops = spectral.SpectralOps(fft)
    shape = (8, 6, 11)
    u = newDistArray(fft, True, rank=1)
    assert ops.random_solenoidal(u, 11, stream=5) is u
    call = RandomEngine.seen[-1]
    assert call == dict(ncomp=3, n=shape, start=(0, 0, 0), N=N, project=True, dk=1.0, nbins=ops.default_nbins(), seed=11, stream=5,
                        add=False, amp=False)
    ref, zero, _ = R.full_field(N, True, 11, 5)
    assert np.array_equal(u.tensor.numpy(), ref.astype(np.complex128))
    # add on top of itself, amplitude tables as numpy and as a tensor, a scalar field without the projection
    ops.random_solenoidal(u, 11, stream=5, add=True)
    assert np.array_equal(u.tensor.numpy(), 2 * ref.astype(np.complex128)) and RandomEngine.seen[-1]['add']
    amp = np.array([0, 1, 2, 0, 0.5])
    ops.random_solenoidal(u, 11, amp=amp)
    assert RandomEngine.seen[-1]['nbins'] == 5 and RandomEngine.seen[-1]['amp']
    want = R.full_field(N, True, 11, 0, amp=amp, nbins=5)[0].astype(np.complex128)
    assert np.array_equal(u.tensor.numpy(), want)
    ops.random_solenoidal(u, 11, amp=torch.as_tensor(amp))
    assert np.array_equal(u.tensor.numpy(), want)
    s = newDistArray(fft, True)
    ops.random_solenoidal(s, 2, project=False, nbins=4)
    assert RandomEngine.seen[-1]['ncomp'] == 1 and not RandomEngine.seen[-1]['project']
    assert np.array_equal(s.tensor.numpy(), R.full_field(N, True, 2, 0, ncomp=1, project=False, nbins=4)[0][0].astype(np.complex128))
    for bad in (dict(out=s), dict(seed=-1), dict(seed=1 << 64), dict(stream=1 << 62), dict(stream=-1), dict(dk=0.0),
                dict(amp=amp, nbins=4), dict(amp=np.zeros((2, 2))), dict(amp=torch.zeros(4)), dict(nbins=0)):
        kw = dict(out=u, seed=1)
        kw.update(bad)
        with pytest.raises(AssertionError):
            ops.random_solenoidal(**kw)
    with pytest.raises(AssertionError, match='precision'):
        ops.random_solenoidal(u.tensor.to(torch.complex64), 1)
    # scale_shells: in place returns its argument; out of place leaves the input; a short table zeroes the rest
    ops.random_solenoidal(u, 11)
    f = u.tensor.numpy().copy()
    tab = np.array([0.0, 2.0, 0.5, 3.0])
    v = newDistArray(fft, True, rank=1)
    assert ops.scale_shells(u, tab, out=v) is v and np.array_equal(u.tensor.numpy(), f)
    assert np.array_equal(v.tensor.numpy(), R.scale_shells(f, [k.numpy() for k in ops.K], tab, 1.0))
    assert ops.scale_shells(u, torch.as_tensor(tab)) is u and np.array_equal(u.tensor.numpy(), v.tensor.numpy())
    for bad in (dict(table=np.zeros(0)), dict(table=torch.zeros(3)), dict(out=s), dict(dk=-1.0)):
        kw = dict(f_hat=u, table=tab)
        kw.update(bad)
        with pytest.raises(AssertionError):
            ops.scale_shells(**kw)
    # random_field: the spectrum of the result is the model's, shell by shell
    nb = ops.default_nbins()
    E = spectral.model_spectrum(ops.shells(nb), 'karman', 2.0, 1.3)
    table = ops.random_field(u, E, seed=5)
    have = ops.spectrum(u)[0]
    filled = table > 0
    assert table.shape == (nb,) and not filled[0] and filled[1:4].all()
    assert np.allclose(have[filled], E[filled], rtol=1e-12, atol=0) and not have[~filled].any()
    with pytest.raises(AssertionError):
        ops.random_field(u, -E, seed=5)
    # white_noise_force: sum w |f|^2 / 2 = eps dt exactly, only in the band, and a fresh field every step
    w = newDistArray(fft, True, rank=1)
    before = u.tensor.numpy().copy()
    e0 = ops.spectrum(u)[0]
    fac = ops.white_noise_force(u, w, step=3, eps=0.25, dt=0.01, band=(2, 3), seed=9)
    assert RandomEngine.seen[-1]['stream'] == 3 and RandomEngine.seen[-1]['seed'] == 9 and RandomEngine.seen[-1]['nbins'] == 4
    df = u.tensor.numpy() - before
    assert np.allclose(df, fac * w.tensor.numpy(), rtol=1e-13, atol=1e-15)
    inj = R.spectrum(df, [k.numpy() for k in ops.K], ops.W.numpy(), 1.0, nb)
    assert np.allclose(inj.sum(), 0.25 * 0.01, rtol=1e-12) and not inj[:2].any() and not inj[4:].any()
    e1 = ops.spectrum(u)[0]
    wk =ops.W.numpy()[None, None, None, :]
    cross = float((wk * (np.conj(before) * df).real).sum())
    assert np.allclose(e1.sum() - e0.sum(), 0.25 * 0.01 + cross, rtol=1e-10, atol=1e-14)
    w3 = w.tensor.numpy().copy()
    ops.white_noise_force(u, w, step=4, eps=0.25, dt=0.01, band=(2, 3), seed=9)
    assert (w.tensor.numpy()[w3 != 0] != w3[w3 != 0]).all()
    assert ops.white_noise_force(u, w, step=4, eps=0.25, dt=0.01, band=(40, 41), seed=9) == 0.0       # an empty band
    fft.destroy()


@pytest.mark.parametrize('P,grid', [(2, [2, 1, 1]), (4, [2, 2, 1])])
def test_the_field_does_not_depend_on_the_cut(P, grid, engine):
    from mpi4py_fft_amd import PFFT, newDistArray, spectral
    N = (8, 8, 20)
    ref = R.full_field(N, True, 21, 2)[0].astype(np.complex128)
    E = spectral.model_spectrum(np.arange(9), 'gaussian', 3.0, 1.0)

    def body(comm):
        fft = PFFT(comm, N, dtype='d', grid=grid, wire='torch')
        ops = spectral.SpectralOps(fft)
        u = newDistArray(fft, True, rank=1)
        ops.random_solenoidal(u, 21, stream=2)
        sl = tuple(fft.local_slice(True))
        got = u.tensor.numpy().copy()
        table = ops.random_field(u, E, seed=4)
        spec = ops.spectrum(u, nbins=9)[0]
        fft.destroy()
        return sl, got, table, spec
    res = cases.run_ranks(P, body)
    starts = set()
    for sl, got, table, spec in res:
        assert np.array_equal(got, ref[(slice(None),) + sl])
        assert np.array_equal(table, res[0][2]) and np.array_equal(spec, res[0][3])          # every rank the same table
        assert np.allclose(spec[1:], E[1:], rtol=1e-12, atol=0)
        starts.add(tuple(s.start for s in sl))
    assert len(starts) == P


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    for name in ('gfft_ps_random_field', 'gfft_ps_scale_shells'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def i64(*v):
        return (ctypes.c_int64 * len(v))(*v)

    def rf(out=p, ncomp=3, n=i64(8, 6, 11), start=i64(0, 0, 0), N=i64(8, 6, 20), k0=p, k1=p, k2=p, project=1, dk=1.0, amp=p, nbins=8,
           seed=1, stream_id=0, add=0, prec=8):
        return lib.gfft_ps_random_field(out, ncomp, n, start, N, k0, k1, k2, project, dk, amp, nbins, seed, stream_id, add, prec, None)
    INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -3
    for bad in (dict(out=None), dict(n=None), dict(start=None), dict(N=None), dict(k0=None), dict(k1=None), dict(k2=None),   # a null pointer
                dict(ncomp=0), dict(ncomp=5), dict(ncomp=-1),                                    # ncomp outside 1 .. 4
                dict(ncomp=1), dict(ncomp=4),                                                    # project with ncomp != 3
                dict(nbins=0), dict(nbins=-3), dict(dk=0.0), dict(dk=-1.0), dict(dk=float('nan')),
                dict(n=i64(-1, 6, 11)), dict(n=i64(8, 6, -1)),                                   # a negative extent
                dict(start=i64(1, 0, 0)), dict(start=i64(0, 0, 10)), dict(n=i64(8, 7, 11)), dict(start=i64(0, -1, 0)),   # outside the grid
                dict(N=i64(8, 0, 20)),
                dict(stream_id=1 << 62), dict(stream_id=(1 << 64) - 1),
                dict(prec=3), dict(prec=16)):
        assert rf(**bad) == INVALID, bad
    assert rf(stream_id=1 << 62) == INVALID and b'2^62' in lib.gfft_last_error()
    big = (1 << 30) + 1
    assert rf(n=i64(1, big, 1), N=i64(8, big, 20)) == UNSUPPORTED and rf(n=i64(1, 1, big), N=i64(8, 6, 2 * big)) == UNSUPPORTED
    assert b'2^30' in lib.gfft_last_error()
    assert rf(n=i64(1, 1, 1), N=i64(1 << 21, 1 << 21, 1 << 21)) == UNSUPPORTED

    def ss(out=p, f=p, ncomp=3, k0=p, k1=p, k2=p, dk=1.0, tab=p, nbins=8, n=(8, 6, 11), prec=8):
        return lib.gfft_ps_scale_shells(out, f, ncomp, k0, k1, k2, dk, tab, nbins, n[0], n[1], n[2], prec, None)
    for bad in (dict(out=None), dict(f=None), dict(k0=None), dict(k1=None), dict(k2=None), dict(tab=None), dict(ncomp=0),
                dict(nbins=0), dict(dk=0.0), dict(dk=float('nan')), dict(n=(-1, 6, 11)), dict(n=(8, 6, -11)), dict(prec=2)):
        assert ss(**bad) == INVALID, bad
    assert ss(ncomp=5) == UNSUPPORTED and b'4 components' in lib.gfft_last_error()
    assert ss(n=(2, big, 2)) == UNSUPPORTED and b'2^30' in lib.gfft_last_error()
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device
        assert rf() == NO_DEVICE and rf(amp=None) == NO_DEVICE and rf(ncomp=4, project=0, prec=4) == NO_DEVICE
        assert rf(stream_id=(1 << 62) - 1, seed=(1 << 64) - 1, add=1) == NO_DEVICE
        assert rf(n=i64(2, 3, 8), start=i64(1500, 7, 1000), N=i64(2048, 2048, 2048)) == NO_DEVICE
        assert rf(n=i64(0, 6, 11)) == NO_DEVICE
        assert ss() == NO_DEVICE and ss(ncomp=1, prec=4) == NO_DEVICE and ss(out=p, f=p) == NO_DEVICE
