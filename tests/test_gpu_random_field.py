"""gfft_ps_random_field and gfft_ps_scale_shells on the device: against tests/random_ref.py (numpy; long double behind the
exact uniforms) within the derived bound, against themselves for everything the definition promises bit for bit (call against
call, add against fill, mirror against conjugate, r2c against c2c, fp32 against rounded fp64, two ranks against one, a block of a
huge grid against the reference and against the block of its mirrors), and end to end through SpectralOps.

Launch geometry the cases are chosen against (csrc/spectral.hip, launch_ps_random_field; `_lanes` below restates it and the
cases assert what they rely on).  A lane takes V neighbouring modes along i2 -- 16 bytes per store: V = 1 in fp64; in fp32 V = 2
where n2 is even and the base is 16-byte aligned, else 1 -- and count / V lanes stride over at most RF_MAX_WG = 2048 workgroups
of 256.
  (8, 6, 20) c2c: n2 = 20, V = 2 in fp32; r2c: n2 = 11, V = 1.  (5, 3, 7): everything odd, no Nyquist index anywhere, V = 1
  (r2c: n2 = 4, V = 2 in fp32).  (8, 6, 20) one element into an allocation: fp32 V = 1 with an even n2, fp64 still 16-byte aligned.
  Walking: (64, 128, 128) r2c = 64 x 128 x 65 = 532480 modes > 2048 x 256 = 524288 lanes, V = 1 in both precisions (n2 = 65): the
  smallest round shape whose lanes take a second mode.
gfft_ps_scale_shells has the geometry of gfft_ps_scale_axes (ps_grid: up to 16384 workgroups), which tests/test_gpu_interp.py walks.

Bound (derived in random_ref.py, not measured): |got - ref| <= 20 x 2^-53 amp ||G||_2 per part, + 2^-24 |ref| in fp32.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, random_ref as R
from tests.arena import Arena

DEV = 'cuda'
BYTES = {'d': 8, 'f': 4}
CPLX = {'d': np.complex128, 'f': np.complex64}
TCPLX = {'d': torch.complex128, 'f': torch.complex64}
SHAPES = {'even': (8, 6, 20), 'odd': (5, 3, 7)}
RF_MAX_WG = 2048
WORST = {}


def _stored(N, r2c):
    return (N[0], N[1], N[2] // 2 + 1 if r2c else N[2])


def _lanes(n, dt, aligned=True):
    """(V, lanes, workgroups) of launch_ps_random_field"""
    count = int(np.prod(n))
    V = 2 if (dt == 'f' and n[2] % 2 == 0 and aligned) else 1
    lanes = count // V
    return V, lanes, min(-(-lanes // 256), RF_MAX_WG)


def _kdev(N, r2c, dt, start=(0, 0, 0), n=None):
    n = _stored(N, r2c) if n is None else n
    return [torch.as_tensor(k[s:s + m].astype(dt)).to(DEV) for k, s, m in zip(R.wavenumbers(N, r2c), start, n)]


def _fill(N, r2c, dt, seed, stream, ncomp=3, project=True, amp=None, nbins=64, add=False, init=None, misaligned=False,
          start=(0, 0, 0), n=None, dk=1.0):
    """gfft_ps_random_field straight through the engine into a flat device tensor prefilled with `init` (default: NaN)"""
    from mpi4py_fft_amd import _lib
    n = _stored(N, r2c) if n is None else tuple(n)
    count = int(np.prod(n))
    buf = torch.empty(ncomp * count + 1, dtype=TCPLX[dt], device=DEV)
    t = buf[1:] if misaligned else buf[:-1]
    assert t.data_ptr() % 16 == (8 if misaligned and dt == 'f' else 0)
    t.copy_(torch.as_tensor(np.full(ncomp * count, complex(np.nan, np.nan) if init is None else init, dtype=CPLX[dt])))
    tamp = None if amp is None else torch.as_tensor(np.asarray(amp, dtype=np.float64)).to(DEV)
    _lib.engine().ps_random_field(t, ncomp, n, start, N, _kdev(N, r2c, dt, start, n), project, dk, tamp, nbins, seed, stream, add,
                                  BYTES[dt])
    return t.cpu().numpy().reshape((ncomp,) + n)


@functools.lru_cache(maxsize=None)
def _reference(N, r2c, seed, stream, ncomp=3, project=True, amp=None, nbins=64):
    """(field, zeroed, amp ||G||) of the whole spectral array: computed once per case, never modified"""
    out = R.full_field(N, r2c, seed, stream, ncomp=ncomp, project=project, amp=None if amp is None else np.array(amp), nbins=nbins)
    for a in out:
        a.setflags(write=False)
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex128 else np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _conj_equal(a, b):
    """a == conj(b) value for value, nothing NaN: the same bits on every non-zero part (a zeroed mode is +0 on both sides)"""
    return a.dtype == b.dtype and a.shape == b.shape and not np.isnan(a).any() and np.array_equal(a, np.conj(b))


def _mirrored(G, N):
    idx = [(-np.arange(m)) % m for m in N]
    return G[:, idx[0]][:, :, idx[1]][:, :, :, idx[2]]


# ---- against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ncomp,project', [(1, False), (3, True), (3, False), (4, False)])
@pytest.mark.parametrize('r2c', [True, False], ids=['r2c', 'c2c'])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', ['even', 'odd', 'misaligned'])
def test_device_within_the_bound(kind, dt, r2c, ncomp, project):
    N = SHAPES['even' if kind == 'misaligned' else kind]
    n = _stored(N, r2c)
    V, lanes, nwg = _lanes(n, dt, kind != 'misaligned')
    if kind == 'misaligned' and dt == 'f':
        assert V == 1 and n[2] % 2 == (1 if r2c else 0)
    if kind == 'even' and dt == 'f' and not r2c:
        assert V == 2
    ref, zero, gnorm = _reference(N, r2c, 7, 3, ncomp, project)
    got = _fill(N, r2c, dt, 7, 3, ncomp, project, misaligned=kind == 'misaligned')
    assert not np.isnan(got.view(got.real.dtype)).any(), 'a mode was not written'
    share = R.worst_share(got, ref, gnorm, dt == 'f')
    WORST[(kind, dt, r2c, ncomp, project)] = share
    print('random field %s %s %s ncomp %d project %d: worst share of the bound %.4f (of all cases so far %.4f)'
          % (kind, dt, 'r2c' if r2c else 'c2c', ncomp, project, share, max(WORST.values())))
    assert share <= 1.0, share
    z = got[:, zero]
    assert not z.real.any() and not z.imag.any() and not np.signbit(z.real).any() and not np.signbit(z.imag).any()      # +0


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_amplitudes_and_shell_width_against_the_reference(dt):
    """a table with a zero in it, fewer shells than the grid holds, dk = 1/2, a box that is not 2 pi"""
    N, amp = (8, 6, 20), (0.0, 1.5, 0.0, 0.25, 3.0)
    L = (2 * np.pi, np.pi, 4 * np.pi)
    from mpi4py_fft_amd import _lib
    for r2c in (True, False):
        n = _stored(N, r2c)
        K = R.wavenumbers(N, r2c, L)
        ref, zero, gnorm = R.random_field(n, (0, 0, 0), N, [k.astype(dt) for k in K], 5, 1, dk=0.5, amp=np.array(amp), nbins=5)
        t = torch.full((3,) + n, complex(np.nan, np.nan), dtype=TCPLX[dt], device=DEV)
        _lib.engine().ps_random_field(t, 3, n, (0, 0, 0), N, [torch.as_tensor(k.astype(dt)).to(DEV) for k in K], True, 0.5,
                                      torch.as_tensor(np.array(amp)).to(DEV), 5, 5, 1, False, BYTES[dt])
        got = t.cpu().numpy()
        assert 0.3 < zero.mean() < 1.0 and (~zero).sum() > 20
        assert R.worst_share(got, ref, gnorm, dt == 'f') <= 1.0


# ---- exactness -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', ['even', 'odd'])
def test_bit_for_bit_properties(kind, dt):
    N = SHAPES[kind]
    c2c = _fill(N, False, dt, 11, 2)
    r2c = _fill(N, True, dt, 11, 2)
    assert _same(c2c, _fill(N, False, dt, 11, 2)) and _same(r2c, _fill(N, True, dt, 11, 2, misaligned=True))     # call against call
    # add on zeros: equal value for value (0 + x = x; a part the projection left as -0 comes out of the addition as +0)
    assert np.array_equal(r2c, _fill(N, True, dt, 11, 2, add=True, init=0.0))
    # the mirror mode is the conjugate of its partner: across the whole c2c block ...
    assert _conj_equal(_mirrored(c2c, N), c2c)
    # ... and inside the r2c block on the plane k2 = 0, the one plane of it that holds both partners
    plane = r2c[..., :1]
    assert _conj_equal(_mirrored(plane, (N[0], N[1], 1)), plane) and plane.any()
    # the r2c field is the stored half of the c2c field; its last planes -- Nyquist (zero) and Nyquist-adjacent -- mirror into the other half
    h = N[2] // 2 + 1
    assert _same(r2c, np.ascontiguousarray(c2c[..., :h]))
    if N[2] % 2 == 0:
        assert not r2c[..., h - 1].any()
    adj = h - 2 if N[2] % 2 == 0 else h - 1
    assert r2c[..., adj].any() and _conj_equal(_mirrored(c2c, N)[..., adj], r2c[..., adj])
    # with L = 2 pi the wavenumbers are the same numbers in both precisions: the fp32 field is the fp64 field rounded once
    if dt == 'f':
        for r, field in ((True, r2c), (False, c2c)):
            assert _same(field, _fill(N, r, 'd', 11, 2).astype(np.complex64))
    # without the projection too
    p4 = _fill(N, False, dt, 11, 2, ncomp=4, project=False)
    assert _conj_equal(_mirrored(p4, N), p4) and _same(np.ascontiguousarray(p4[..., :h]), _fill(N, True, dt, 11, 2, ncomp=4, project=False))
    assert _same(np.ascontiguousarray(p4[:1]), _fill(N, False, dt, 11, 2, ncomp=1, project=False))       # a component is its own stream


def test_zeroed_modes_and_add():
    """Nyquist planes, the mean, shells beyond the table and shells of amplitude zero are +0; with add they are left alone"""
    N, amp = (8, 6, 20), (1.0, 1.0, 0.0, 2.0, 1.0)
    for dt in 'df':
        for r2c in (True, False):
            n = _stored(N, r2c)
            K = np.meshgrid(*R.wavenumbers(N, r2c), indexing='ij')
            b = R.shell_of(K[0], K[1], K[2], 1.0)
            g = np.meshgrid(*[np.arange(m) for m in n], indexing='ij')
            want = (b >= 5) | (b == 2) | (b == 0) | (2 * g[0] == N[0]) | (2 * g[1] == N[1]) | (2 * g[2] == N[2])
            ref, zero, gnorm = _reference(N, r2c, 4, 0, 3, True, amp, 5)
            assert np.array_equal(zero, want) and 0 < (~zero).sum() < zero.size
            got = _fill(N, r2c, dt, 4, 0, amp=amp, nbins=5)
            assert _same(got[:, zero], np.zeros_like(got[:, zero])) and (got[:, ~zero] != 0).any(axis=0).all()
            # add over NaN: the zeroed entries keep the very bits they had, the others took part in an addition
            sentinel = np.array([0], dtype=CPLX[dt])
            _bits(sentinel)[...] = 0x7ff8000000abcdef if dt == 'd' else 0x7fc0abcd
            over = _fill(N, r2c, dt, 4, 0, amp=amp, nbins=5, add=True, init=sentinel[0])
            assert (_bits(over[:, zero]) == _bits(sentinel)[0]).all() and np.isnan(over[:, ~zero].real).all()
            # add over a finite field: untouched where zeroed, the sum in the field's precision elsewhere
            base = complex(3.5, -1.25)
            over = _fill(N, r2c, dt, 4, 0, amp=amp, nbins=5, add=True, init=base)
            assert (over[:, zero] == base).all()
            rdt = np.float64 if dt == 'd' else np.float32
            assert np.array_equal(over.real, np.where(zero[None], rdt(3.5), rdt(3.5) + got.real))
            assert np.array_equal(over.imag, np.where(zero[None], rdt(-1.25), rdt(-1.25) + got.imag))


def test_two_thread_ranks_hold_slices_of_the_one_rank_field():
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    N = (8, 6, 20)
    E = np.array([0, 1.0, 2.0, 0.5, 0.25, 0.1])

    def run(c, **kw):
        fft = PFFT(c, N, dtype='d', **kw)
        ops = spectral.SpectralOps(fft)
        u = newDistArray(fft, True, rank=1)
        ops.random_solenoidal(u, 31, stream=9)
        plain = np.asarray(u).copy()
        table = ops.random_field(u, E, seed=31)
        out = (tuple(fft.local_slice(True)), plain, np.asarray(u).copy(), table)
        fft.destroy()
        return out
    _, one, one_scaled, one_table = run(comm.COMM_SELF)
    ref, _, gnorm = _reference(N, True, 31, 9)
    assert R.worst_share(one, ref, gnorm) <= 1.0
    res = cases.run_ranks(2, lambda c: run(c, grid=[2, 1, 1]))
    assert len({tuple(s.start for s in sl) for sl, _, _, _ in res}) == 2
    for sl, plain, scaled, table in res:
        assert _same(plain, np.ascontiguousarray(one[(slice(None),) + sl]))
        assert np.array_equal(table, res[0][3]), 'the ranks scale by different tables'
        # the reduced spectrum differs from the one-rank one by rounding, and so may the table: a few units in the last place
        assert np.allclose(table, one_table, rtol=1e-14, atol=0)
        assert np.allclose(scaled, one_scaled[(slice(None),) + sl], rtol=1e-14, atol=0)


# ---- the 64-bit linear index -------------------------------------------------------------------------------------------------
def _capi_block(N, n, start, seed, stream, dt='d'):
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    i64 = lambda v: (ctypes.c_int64 * 3)(*v)
    k = _kdev(N, False, dt, start, n)
    out = torch.full((3,) + tuple(n), complex(np.nan, np.nan), dtype=TCPLX[dt], device=DEV)
    rc = lib.gfft_ps_random_field(out.data_ptr(), 3, i64(n), i64(start), i64(N), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(), 1,
                                  1.0, None, 4096, seed, stream, 0, BYTES[dt], _lib.current_stream())
    assert rc == 0, lib.gfft_last_error()
    return out.cpu().numpy()


def test_linear_index_beyond_32_bits():
    """a small block of a 2048^3 grid whose linear indices exceed 2^32, against the reference; and the block that holds its mirrors"""
    N, n, start = (2048, 2048, 2048), (2, 3, 8), (1500, 7, 1000)
    assert (start[0] * N[1] + start[1]) * N[2] + start[2] > 1 << 32
    stream = (1 << 61) + 12345                               # the high word of the stream, too
    got = _capi_block(N, n, start, 99, stream)
    K = [k[s:s + m] for k, s, m in zip(R.wavenumbers(N, False), start, n)]
    ref, zero, gnorm = R.random_field(n, start, N, K, 99, stream, nbins=4096)
    assert not zero.any() and R.worst_share(got, ref, gnorm) <= 1.0
    # the mirrors: index N - g, i.e. 548, 547 / 2041 ... 2039 / 1048 ... 1041, inside the block (546, 2038, 1040) + (3, 4, 9)
    mstart, mn = (546, 2038, 1040), (3, 4, 9)
    other = _capi_block(N, mn, mstart, 99, stream)
    sel = np.ix_(range(3), *[[N[a] - (start[a] + i) - mstart[a] for i in range(n[a])] for a in range(3)])
    assert _conj_equal(np.ascontiguousarray(other[sel]), got) and got.all()
    # the mirror block draws from the partner's counter: its canonical index is the smaller one
    mref = R.random_field(mn, mstart, N, [k[s:s + m] for k, s, m in zip(R.wavenumbers(N, False), mstart, mn)], 99, stream, nbins=4096)
    assert R.worst_share(other, mref[0], mref[2]) <= 1.0


# ---- streams, seeds and statistics -------------------------------------------------------------------------------------------
def test_streams_seeds_and_statistics():
    N = (32, 32, 32)
    ref, zero, gnorm = _reference(N, True, 7, 0)
    a = _fill(N, True, 'd', 7, 0)
    assert R.worst_share(a, ref, gnorm) <= 1.0
    modes = int((~zero).sum())
    e = (np.abs(a) ** 2).sum(axis=0)[~zero]
    print('mean |u_hat|^2 = %.4f +- %.4f over %d modes' % (e.mean(), e.std() / np.sqrt(modes), modes))
    assert abs(e.mean() - 4.0) <= 5 * e.std() / np.sqrt(modes)
    for other in (_fill(N, True, 'd', 7, 1), _fill(N, True, 'd', 8, 0), _fill(N, True, 'd', 7, 1 << 32)):
        assert (other[:, ~zero] != a[:, ~zero]).any(axis=0).all() and not other[:, zero].any()
        x, y = a[:, ~zero].ravel(), other[:, ~zero].ravel()
        corr = abs(np.vdot(x, y)) / np.sqrt(np.vdot(x, x).real * np.vdot(y, y).real)
        assert corr <= 5 / np.sqrt(modes), corr


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_walks_past_one_grid_sweep(dt):
    N = (64, 128, 128)
    n = _stored(N, True)
    V, lanes, nwg = _lanes(n, dt)
    assert V == 1 and nwg == RF_MAX_WG and RF_MAX_WG * 256 < lanes <= 2 * RF_MAX_WG * 256        # some lanes take a second mode
    assert int(np.prod((64, 128, 64))) <= RF_MAX_WG * 256                                     # and no rounder shape below does
    ref, zero, gnorm = _reference(N, True, 3, 0, 3, True, None, 128)
    got = _fill(N, True, dt, 3, 0, nbins=128)
    assert R.worst_share(got, ref, gnorm, dt == 'f') <= 1.0


# ---- gfft_ps_scale_shells ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 3, 4])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', ['even r2c', 'even c2c', 'odd', 'misaligned'])
def test_scale_shells_equals_the_reference(kind, dt, m):
    from mpi4py_fft_amd import _lib
    N, r2c = (SHAPES['odd'], True) if kind == 'odd' else (SHAPES['even'], kind != 'even c2c')
    n = _stored(N, r2c)
    count = int(np.prod(n))
    rng = np.random.default_rng(41)
    f = (rng.standard_normal((m,) + n) + 1j * rng.standard_normal((m,) + n)).astype(CPLX[dt])
    tab = np.array([1.0, 2.0, -0.5, 1e-3, 3.0, 0.0, 7.0][:3 if kind == 'odd' else 7])
    K = [k.astype(dt) for k in R.wavenumbers(N, r2c)]
    far = R.shell_of(*np.meshgrid(*K, indexing='ij'), 1.0) >= len(tab)
    f[:, far] = complex(np.nan, np.nan)                      # beyond the table: stored as +0 whatever it holds
    f[0, 1, 1, 1] = complex(np.inf, -0.0)
    f[0, 0, 0, 0] = complex(np.nan, 1.0)                     # shell 0 is inside it: the NaN stays
    want = R.scale_shells(f, K, tab, 1.0)
    assert not far[1, 1, 1] and far.sum() > 10 and not far.all() and _same(want[:, far], np.zeros_like(want[:, far]))
    kd, td = _kdev(N, r2c, dt), torch.as_tensor(tab).to(DEV)
    off = 1 if kind == 'misaligned' else 0
    bi, bo = (torch.empty(m * count + 1, dtype=TCPLX[dt], device=DEV) for _ in range(2))
    ti, to = bi[off:off + m * count], bo[off:off + m * count]
    ti.copy_(torch.as_tensor(f.ravel()))
    to.fill_(complex(np.nan, np.nan))
    _lib.engine().ps_scale_shells(ti, to, m, kd, 1.0, td, len(tab), n, BYTES[dt])
    assert _same(to.cpu().numpy().reshape(f.shape), want) and _same(ti.cpu().numpy().reshape(f.shape), f)
    _lib.engine().ps_scale_shells(ti, ti, m, kd, 1.0, td, len(tab), n, BYTES[dt])                 # in place
    assert _same(ti.cpu().numpy().reshape(f.shape), want)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_random_field_reproduces_a_model_spectrum():
    from mpi4py_fft_amd import PFFT, _lib, comm, newDistArray, spectral
    N = (32, 32, 32)
    fft = PFFT(comm.COMM_SELF, N, dtype='d')
    ops = spectral.SpectralOps(fft)
    u_hat = newDistArray(fft, True, rank=1)
    nb = 16
    for kind in ('gaussian', 'karman'):
        E = spectral.model_spectrum(ops.shells(nb), kind, 4.0, 0.8)
        table = ops.random_field(u_hat, E, seed=7)
        have = ops.spectrum(u_hat)
        assert table.shape == (nb,) and table[0] == 0 and (table[1:] > 0).all()
        assert have[0][0] == 0 and not have[0][nb:].any()
        assert np.all(np.abs(have[0][1:nb] - E[1:]) <= 1e-12 * E[1:]), (have[0][:nb] / E - 1)
        assert abs(ops.energy(u_hat) - 1.5 * 0.64) <= 1e-12
    # divergence at rounding level, in physical space
    A_hat = newDistArray(fft, True, rank=2)
    A = newDistArray(fft, False, rank=2)
    ops.gradient(u_hat, A_hat)
    for i in range(3):
        for j in range(3):
            fft.backward(A_hat[i][j], A[i][j])
    gs = ops.gradient_stats(A)
    assert gs[_lib.GS_MAX_SS] > 0.1 and gs[_lib.GS_MAX_DIV] <= 1e-13 * np.sqrt(gs[_lib.GS_MAX_SS]) * 100
    fft.destroy()
    # a complex transform: the backward transform of the field is real by construction
    fft = PFFT(comm.COMM_SELF, (16, 12, 10), dtype='D')
    ops = spectral.SpectralOps(fft)
    u_hat = newDistArray(fft, True, rank=1)
    u = newDistArray(fft, False, rank=1)
    ops.random_field(u_hat, spectral.model_spectrum(ops.shells(8), 'gaussian', 3.0, 1.0), seed=2)
    for c in range(3):
        fft.backward(u_hat[c], u[c])
    phys = np.asarray(u)
    assert np.abs(phys.real).max() > 0.5 and np.abs(phys.imag).max() <= 1e-14 * np.abs(phys.real).max()
    fft.destroy()


def test_white_noise_force_injects_eps_dt_plus_the_cross_term():
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    N = (16, 16, 16)
    fft = PFFT(comm.COMM_SELF, N, dtype='d')
    ops = spectral.SpectralOps(fft)
    u_hat, work = newDistArray(fft, True, rank=1), newDistArray(fft, True, rank=1)
    ops.random_field(u_hat, spectral.model_spectrum(ops.shells(8), 'gaussian', 2.0, 1.0), seed=1)
    before = newDistArray(fft, True, rank=1)
    before.tensor.copy_(u_hat.tensor)
    e0 = ops.energy(u_hat)
    eps, dt = 0.3, 0.02
    fac = ops.white_noise_force(u_hat, work, step=17, eps=eps, dt=dt, band=(2, 3), seed=5)
    assert fac > 0
    cross = fac * float(ops.cospectrum(before, work)[0].sum())
    inj = ops.spectrum(work)[0]
    assert not inj[:2].any() and not inj[4:].any() and abs(fac * fac * inj.sum() - eps * dt) <= 1e-13 * eps * dt * 10
    assert abs(cross) > 1e-6                                   # the step's cross term is there, and is accounted for
    assert abs((ops.energy(u_hat) - e0) - (eps * dt + cross)) <= 1e-12 * e0
    # the next step draws another field
    w0 = np.asarray(work).copy()
    ops.white_noise_force(u_hat, work, step=18, eps=eps, dt=dt, band=(2, 3), seed=5)
    w1 = np.asarray(work)
    assert (w1[:, (w0 != 0).any(axis=0)] != w0[:, (w0 != 0).any(axis=0)]).any(axis=0).all()
    fft.destroy()


# ---- guard bands -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['d', 'f'])
def test_nothing_is_written_outside_the_field(dt):
    """the output in a guarded arena, at a 256-byte boundary and one element past it; fill, add and scale_shells"""
    from mpi4py_fft_amd import _lib
    for N, r2c in (((8, 6, 20), True), ((8, 6, 20), False), ((5, 3, 7), True)):
        n = _stored(N, r2c)
        kd = _kdev(N, r2c, dt)
        tab = torch.as_tensor(np.array([1.0, 2.0, 0.5, 0.25])).to(DEV)
        for ncomp, project in ((3, True), (4, False)):
            plain = _fill(N, r2c, dt, 13, 1, ncomp, project)
            for off in (0, 1):
                what = (N, r2c, dt, ncomp, project, off)
                A = Arena((ncomp,) + n, CPLX[dt], offset_elems=off)
                A.array[...] = np.full((ncomp,) + n, complex(np.nan, np.nan), dtype=CPLX[dt])
                _lib.engine().ps_random_field(A.array.tensor, ncomp, n, (0, 0, 0), N, kd, project, 1.0, None, 64, 13, 1, False, BYTES[dt])
                torch.cuda.synchronize()
                A.check(what + ('fill',))
                assert _same(np.asarray(A.array), plain), what
                _lib.engine().ps_random_field(A.array.tensor, ncomp, n, (0, 0, 0), N, kd, project, 1.0, None, 64, 13, 1, True, BYTES[dt])
                torch.cuda.synchronize()
                A.check(what + ('add',))
                assert _same(np.asarray(A.array), plain + plain), what
                _lib.engine().ps_scale_shells(A.array.tensor, A.array.tensor, ncomp, kd, 1.0, tab, 4, n, BYTES[dt])
                torch.cuda.synchronize()
                A.check(what + ('scale_shells',))
                assert _same(np.asarray(A.array), R.scale_shells(plain + plain, [k.cpu().numpy() for k in kd], tab.cpu().numpy(), 1.0)), what


# ---- the example ---------------------------------------------------------------------------------------------------------------
def test_example_starts_random_and_is_forced_white():
    """examples/dns_taylor_green.py with init=('random', ...): the energy at step 0 is 3 u_rms^2 / 2 (the 2/3 rule then removes the
    tail of the model spectrum), the run repeats bit for bit, and forcing=('white', ...) adds eps h per step up to the cross term."""
    import importlib.util
    import os
    from mpi4py_fft_amd import comm
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_random', path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    kw = dict(M=5, dt=0.005, nu=0.01, init=('random', 7, 3.0, 0.5))
    e0 = ex.solve(comm.COMM_SELF, nsteps=0, **kw)
    assert abs(e0 - 1.5 * 0.25) <= 1e-12
    e2 = ex.solve(comm.COMM_SELF, nsteps=2, **kw)
    assert 0.9 * e0 < e2 < e0 and e2 == ex.solve(comm.COMM_SELF, nsteps=2, **kw)              # decays, and repeats
    st = {}
    ef = ex.solve(comm.COMM_SELF, nsteps=2, stats=st, forcing=('white', 2.0, 2, 3), **kw)
    assert st['white_factor'] > 0 and ef != e2 and abs(ef - e2) < 4 * 2.0 * 0.005 + 4 * np.sqrt(2 * e2 * 2.0 * 0.005)
    assert ex.solve(comm.COMM_SELF, nsteps=2, forcing=('white', 0.0, 2, 3), **kw) == e2                          # eps = 0: the unforced run
