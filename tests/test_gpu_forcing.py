"""gfft_ps_force_gain / gfft_ps_project_forced on the device against tests/forcing_ref.py (numpy, float64) and against
gfft_ps_project itself.

Boxes without shell-boundary ties only (spectrum_ref.BOX, dk = 1/2), so the reference mask and a correct device cannot
disagree about a mode.  Bounds are derived, not measured:
  * du = 0, nu = 0: an in-band scalar is real(gain) * u with ONE rounding in the field's precision -- exact equality;
  * out of band: the bits of gfft_ps_project;
  * in band, general: |out - p - g u| <= 4 eps (|p| + |g u|) with p the plain projection's value -- one rounding for the
    gain's conversion, one or none for the product (FMA contraction allowed), one for the sum, times a margin of 4/3;
  * gfft_ps_force_gain: the host formula `spectral.force_gain` on the same bins, exactly.

Launch geometry the shapes are chosen against (csrc/spectral.hip): the projection is grid-stride, 256 lanes per workgroup,
at most 16384 workgroups, a lane's mode is its flat index.  (24, 16, 20) and (12, 10, 21) have spectral blocks 24 x 16 x 11
and 12 x 10 x 11: rows of 11, shorter than a wave, 17 and 6 workgroups, the last one ragged; in-band modes sit at both ends
of axis 0 (the negative wavenumbers).  (160, 160, 328) has 160 x 160 x 165 = 4 224 000 modes > 16384 * 256: lanes take a
second grid-stride step, and the plane k0 = -1 lies wholly in it.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, forcing_ref as F, spectrum_ref as R

SHAPES = [(24, 16, 20), (12, 10, 21)]
NU = 0.03
GAIN = 0.37
EPS_REAL = {'d': 2.0 ** -52, 'f': 2.0 ** -23}


def _bits(a):
    """The bit patterns of a complex or real array (so that -0.0 != 0.0 and a NaN equals itself)"""
    a = np.ascontiguousarray(a)
    r = a.view(a.real.dtype)
    return r.view('u8' if r.dtype == np.float64 else 'u4')


_REF = {}


def _fields(shape, dt):
    """(u_hat, du_hat, k, w): random [3] + spectral shape in the precision under test, no zero entry; computed once per
    case and shared, never modified"""
    key = (tuple(shape), dt)
    if key not in _REF:
        gs = (3,) + tuple(shape[:2]) + (shape[2] // 2 + 1,)
        rng = np.random.default_rng(23)
        uh = (rng.standard_normal(gs) + 1j * rng.standard_normal(gs)).astype(dt.upper())
        du = (rng.standard_normal(gs) + 1j * rng.standard_normal(gs)).astype(dt.upper())
        assert np.all(uh.real != 0) and np.all(uh.imag != 0)
        k, w = R.wavenumbers(shape, True)
        for a in (uh, du):
            a.setflags(write=False)
        _REF[key] = (uh, du, k, w)
    return _REF[key]


def _ops(comm, shape, dt, **kw):
    from mpi4py_fft_amd import PFFT, spectral
    fft = PFFT(comm, shape, dtype=dt, **kw)
    return fft, spectral.SpectralOps(fft, R.BOX)


def _dev(fft, G):
    from mpi4py_fft_amd import newDistArray
    a = newDistArray(fft, rank=1)
    a[...] = np.array(G[(slice(None),) + fft.local_slice(True)])
    return a


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_exact_mask_every_shell(shape, dt):
    """du = 0, nu = 0: what the kernel leaves is real(gain) * u inside the numpy mask, with a single rounding, and 0
    outside -- for every single shell, so the conservative pre-filter rejects nothing and the exact test admits nothing."""
    from mpi4py_fft_amd import comm
    uh, _, k, _ = _fields(shape, dt)
    nbins = R.default_nbins(shape)
    assert nbins == {(24, 16, 20): 33, (12, 10, 21): 25}[shape]
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    U, D = _dev(fft, uh), _dev(fft, uh)
    bands = [(b, b) for b in range(nbins)] + [(1, 2), (0, nbins - 1), (nbins + 2, nbins + 5)]
    covered = 0
    for blo, bhi in bands:
        D.tensor.zero_()
        ops.project(D, U, 0.0, force=(GAIN, (blo, bhi)))
        got = np.asarray(D).copy()
        mask = F.band_mask(k, blo, bhi)
        want = F.band_term(uh, k, blo, bhi, GAIN)
        assert np.array_equal(got.real, want.real) and np.array_equal(got.imag, want.imag), (shape, dt, blo, bhi, int(mask.sum()))
        assert np.all(got.real[:, mask] != 0) and np.all(got[:, ~mask] == 0)
        if blo == bhi:
            covered += int(mask.sum())
        elif blo == 0:
            assert mask.all()
        elif blo > nbins:
            assert not mask.any()
    assert covered == uh[0].size, 'the single shells do not tile the block'
    # the counts the shapes were chosen for: shells 0..4 hold the same modes in both
    assert [int(F.band_mask(k, b, b).sum()) for b in range(5)] == [1, 2, 11, 18, 37]
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_general_case(shape, dt):
    from mpi4py_fft_amd import comm
    uh, du, k, _ = _fields(shape, dt)
    nbins = R.default_nbins(shape)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    U, P = _dev(fft, uh), _dev(fft, du)
    ops.project(P, U, NU)
    p = np.asarray(P).copy()
    assert np.abs(p - F.projected(du, uh, k, NU)).max() <= (1e-13 if dt == 'd' else 2e-5) * np.abs(p).max()
    gu = GAIN * uh.astype('D')
    for blo, bhi in ((0, 0), (2, 3), (0, nbins - 1)):
        D = _dev(fft, du)
        ops.project(D, U, NU, force=(GAIN, (blo, bhi)))
        got = np.asarray(D).copy()
        m = F.band_mask(k, blo, bhi)
        assert m.any()
        assert np.array_equal(_bits(got[:, ~m]), _bits(p[:, ~m])), (shape, dt, blo, bhi, 'out of band differs from gfft_ps_project')
        worst = 0.0
        for part in ('real', 'imag'):
            o, q, t = (getattr(x, part)[:, m].astype('d') for x in (got, p, gu))
            err, tol = np.abs(o - q - t), 4 * EPS_REAL[dt] * (np.abs(q) + np.abs(t))
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (shape, dt, blo, bhi, part, float((err / tol).max()))
        print('%s %s band (%d, %d): worst |out - p - g u| / bound = %.3f' % (shape, dt, blo, bhi, worst))
        assert not np.array_equal(got[:, m], p[:, m])
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_gain_by_value_equals_gain_on_the_device(dt):
    from mpi4py_fft_amd import comm
    shape = (24, 16, 20)
    uh, du, k, _ = _fields(shape, dt)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    U = _dev(fft, uh)
    for gain in (GAIN, 1.0 / 3.0, -2.5e-3):
        A, B = _dev(fft, du), _dev(fft, du)
        g = torch.tensor([gain, 123.0], dtype=torch.float64, device='cuda')
        ops.project(A, U, NU, force=(gain, (1, 4)))
        ops.project(B, U, NU, force=(g, (1, 4)))
        torch.cuda.synchronize()
        a, b = np.asarray(A).copy(), np.asarray(B).copy()
        assert np.array_equal(_bits(a), _bits(b)), (dt, gain)
        assert not np.array_equal(a, du)
        assert g.cpu().tolist() == [gain, 123.0]                    # read only
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_force_gain_kernel_equals_the_host_formula(dt):
    """On the bins ONE device spectrum call produced, copied to the host: gain and E_f equal `spectral.force_gain` exactly."""
    from mpi4py_fft_amd import _lib, comm, spectral
    shape, nb = (24, 16, 20), 8
    uh, _, k, _ = _fields(shape, dt)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    U = _dev(fft, uh)
    spec = ops.spectrum(U, nbins=nb, reduce=False)
    E = spec.cpu().numpy().copy()
    assert np.all(E[0] > 0)
    out = torch.full((2,), -7.0, dtype=torch.float64, device='cuda')

    def device(s, blo, bhi, eps, gmax):
        out.fill_(-7.0)
        _lib.engine().ps_force_gain(s, nb, blo, bhi, eps, gmax, out)
        return tuple(out.cpu().tolist())
    free = spectral.force_gain(E, (2, 4), 0.1)
    assert free[0] == 0.1 / (2.0 * ((E[0][2] + E[0][3]) + E[0][4])) and free[1] == (E[0][2] + E[0][3]) + E[0][4]
    for band, eps, gmax in (((2, 4), 0.1, np.inf), ((0, nb - 1), 0.1, np.inf), ((3, 3), 7.0, np.inf),      # unclamped
                            ((2, 4), 0.1, free[0] / 3), ((2, 4), 0.1, 1e-300),                               # clamped
                            ((2, 4), 0.0, np.inf), ((2, 4), 0.0, 0.5)):                                      # nothing to inject
        got, want = device(spec, band[0], band[1], eps, gmax), spectral.force_gain(E, band, eps, gmax)
        assert got == want, (band, eps, gmax, got, want)
        assert (want[0] == gmax) == (gmax < np.inf) or eps == 0.0
        assert (want[0] == 0.0) == (eps == 0.0) and want[1] > 0
    # an all-zero band: a field with those shells zeroed
    z = np.array(uh)
    z[:, F.band_mask(k, 2, 4)] = 0
    zspec = ops.spectrum(_dev(fft, z), nbins=nb, reduce=False)
    Ez = zspec.cpu().numpy().copy()
    assert np.all(Ez[:, 2:5] == 0) and Ez[0][1] > 0 and Ez[0][5] > 0
    assert device(zspec, 2, 4, 0.1, np.inf) == (0.0, 0.0) == spectral.force_gain(Ez, (2, 4), 0.1)
    assert device(zspec, 1, 5, 0.1, np.inf) == spectral.force_gain(Ez, (1, 5), 0.1) != (0.0, 0.0)
    # a NaN in a band bin: no gain
    nspec = spec.clone()
    nspec[0, 3] = float('nan')
    En = nspec.cpu().numpy().copy()
    got, want = device(nspec, 2, 4, 0.1, np.inf), spectral.force_gain(En, (2, 4), 0.1)
    assert got[0] == 0.0 == want[0] and np.isnan(got[1]) and np.isnan(want[1])
    assert device(nspec, 4, 5, 0.1, np.inf) == spectral.force_gain(En, (4, 5), 0.1)          # beside the band it is not read
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_injection_identity(shape, dt):
    """F = g u in the band with g = eps / (2 E_f): the injected power sum w Re(conj(u) . F) is eps.  Bound: the any-order
    bound of spectrum_ref.assert_bins ((M + 16) 2^-52, all addends non-negative) on E_f and on the co-spectrum sum, plus
    the three roundings of the general case (4 eps with its margin)."""
    from mpi4py_fft_amd import comm
    uh, _, k, _ = _fields(shape, dt)
    eps = 0.1
    M = uh[0].size
    nbins = R.default_nbins(shape)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    U = _dev(fft, uh)
    for band in ((0, 0), (2, 3), (3, 3), (0, nbins - 1)):
        g, ef = ops.forcing_gain(U, eps, band)
        assert g > 0 and ef > 0 and g == eps / (2.0 * ef)
        Fh = _dev(fft, np.zeros_like(uh))
        ops.project(Fh, U, 0.0, force=(g, band))
        power = float(ops.cospectrum(U, Fh)[0].sum())
        tol = eps * (4 * EPS_REAL[dt] + 2 * (M + 16) * 2.0 ** -52)
        print('%s %s band %s: |power - eps| / eps = %.3e (bound %.3e)' % (shape, dt, band, abs(power - eps) / eps, tol / eps))
        assert abs(power - eps) <= tol, (shape, dt, band, power)
    fft.destroy()


def test_past_one_grid_sweep():
    """fp32, 4 224 000 modes: more than 16384 * 256, so lanes take a second grid-stride step (the plane k0 = -1, which holds
    in-band modes, lies wholly in it).  Straight through the engine on the wavenumbers of spectrum_ref."""
    from mpi4py_fft_amd import _lib
    shape, band = (160, 160, 328), (2, 3)
    k, _ = R.wavenumbers(shape, True)
    sshape = tuple(len(ki) for ki in k)
    count = int(np.prod(sshape))
    assert sshape == (160, 160, 165) and count > 16384 * 256
    mask = F.band_mask(k, *band)
    assert mask[0].any() and mask[-1].any() and (sshape[0] - 1) * sshape[1] * sshape[2] >= 16384 * 256 and k[0][-1] == -1.0
    K = [torch.as_tensor(ki.astype('f'), device='cuda') for ki in k]
    gen = torch.Generator(device='cuda').manual_seed(29)
    U = torch.randn((3,) + sshape + (2,), dtype=torch.float32, device='cuda', generator=gen)
    D0 = torch.randn((3,) + sshape + (2,), dtype=torch.float32, device='cuda', generator=gen)
    eng = _lib.engine()
    plain, forced = D0.clone(), D0.clone()
    eng.ps_project(plain, U, K, sshape, NU, 4)
    eng.ps_project_forced(forced, U, K, sshape, NU, R.DK, band[0], band[1], GAIN, None, 4)
    m = torch.as_tensor(mask, device='cuda')
    same = (plain.view(torch.int32) == forced.view(torch.int32)).all(-1)          # [3] + sshape: both halves of a mode
    assert bool(same[:, ~m].all()), 'out of band differs from gfft_ps_project'
    assert not bool(same[:, m].any()), 'an in-band mode was left unforced'
    # du = 0, nu = 0: exactly real(gain) * u in the band (one rounding), 0 elsewhere
    forced.zero_()
    eng.ps_project_forced(forced, U, K, sshape, 0.0, R.DK, band[0], band[1], GAIN, None, 4)
    assert bool((forced[:, ~m] == 0).all())
    got = forced[:, m].cpu().numpy()
    want = np.float32(GAIN) * U[:, m].cpu().numpy()
    assert want.dtype == np.float32 and got.shape == (3, int(mask.sum()), 2) and np.array_equal(got, want)
    assert np.all(got != 0)


@pytest.mark.parametrize('P,grid', [(2, [2, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'pencil4'])
def test_thread_ranks(P, grid):
    """forcing_gain gives every rank the same bits and agrees with the fsum reference spectrum; with one explicit gain each
    rank's forced block is bit for bit its part of the one-rank result; the device-resident form refuses a grid of ranks."""
    from mpi4py_fft_amd import comm, spectral
    shape, dt, band, eps = (24, 16, 20), 'd', (2, 3), 0.1
    uh, du, k, w = _fields(shape, dt)
    ref, _ = R.reference(uh, k, w)
    M = uh[0].size
    want = spectral.force_gain(ref, band, eps)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    D = _dev(fft, du)
    ops.project(D, _dev(fft, uh), NU, force=(GAIN, band))
    one = np.asarray(D).copy()
    fft.destroy()

    def body(c):
        fft, ops = _ops(c, shape, dt, grid=grid)
        U, D = _dev(fft, uh), _dev(fft, du)
        got = ops.forcing_gain(U, eps, band)
        ops.project(D, U, NU, force=(GAIN, band))
        block = np.asarray(D).copy()
        with pytest.raises(AssertionError, match='one-rank'):
            ops.forcing_gain(U, eps, band, out=torch.zeros(2, dtype=torch.float64, device='cuda'))
        sl = fft.local_slice(True)
        fft.destroy()
        return got, block, sl
    res = cases.run_ranks(P, body)
    for got, block, sl in res:
        assert got == res[0][0], 'ranks disagree'
        assert abs(got[1] - want[1]) <= (M + 16) * 2.0 ** -52 * want[1] and abs(got[0] - want[0]) <= (M + 16) * 2.0 ** -52 * want[0]
        assert np.array_equal(_bits(block), _bits(one[(slice(None),) + tuple(sl)])), (P, grid, sl)
    assert len({str(sl) for _, _, sl in res}) == P


def test_forced_projection_replays_from_a_captured_graph():
    """forcing_gain(out=g) followed by project(force=(g, band)) under torch.cuda.graph: a replay follows the field it finds
    -- E_f is quadratic, so the gain quarters when the field doubles -- and the projection uses that gain."""
    from mpi4py_fft_amd import comm
    shape, dt, band, eps = (24, 16, 20), 'd', (2, 3), 0.1
    uh, du, k, _ = _fields(shape, dt)
    M = uh[0].size
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    U, D, D0 = _dev(fft, uh), _dev(fft, du), _dev(fft, du)
    g = torch.zeros(2, dtype=torch.float64, device='cuda')

    def stage():
        ops.forcing_gain(U, eps, band, out=g)
        ops.project(D, U, NU, force=(g, band))

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        stage()                                          # warm-up on another stream: scratch and the kept tensor exist now
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stage()
    host = ops.forcing_gain(U, eps, band)
    seen = []
    for scale in (1.0, 2.0):
        U.tensor.mul_(scale)
        D.tensor.copy_(D0.tensor)
        g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        gain, ef = g.cpu().tolist()
        seen.append((gain, ef))
        assert gain == eps / (2.0 * ef)
        E = _dev(fft, du)
        ops.project(E, U, NU, force=(gain, band))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(np.asarray(D)), _bits(np.asarray(E))), scale
        assert not np.array_equal(np.asarray(D), np.asarray(D0))
    # each E_f lies within the any-order bound (M + 16) 2^-52 of its exact value, and those are exactly a factor 4 apart
    tol = (2 * (M + 16) + 2) * 2.0 ** -52
    assert abs(seen[0][1] - host[1]) <= tol * host[1] and abs(seen[0][0] - host[0]) <= tol * host[0]
    assert abs(seen[1][1] - 4 * seen[0][1]) <= tol * 4 * seen[0][1], seen
    assert abs(seen[1][0] - seen[0][0] / 4) <= tol * seen[0][0] / 4, seen
    fft.destroy()


def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_forcing', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_DNS = {}
DNS = dict(M=5, nsteps=4, dt=0.01)
DNS_EPS = 0.1


def _dns(kind):
    """Energies of the unforced and of the host-gain forced run, computed once"""
    from mpi4py_fft_amd import comm
    if kind not in _DNS:
        st = {}
        e = _example().solve(comm.COMM_SELF, stats=st, forcing=None if kind == 'unforced' else (DNS_EPS, 3, 3), **DNS)
        _DNS[kind] = (e, st)
    return _DNS[kind]


def test_dns_with_zero_injection_is_the_unforced_run():
    from mpi4py_fft_amd import comm
    st = {}
    e = _example().solve(comm.COMM_SELF, forcing=(0.0, 3, 3), stats=st, **DNS)
    assert e == _dns('unforced')[0], (e, _dns('unforced')[0])
    assert st['gain'] == 0.0 and st['band_energy'] > 0.1


def test_dns_injects_at_the_prescribed_rate():
    """The Taylor-Green field has all its energy in shell 3 of this box (|K| = sqrt 3, dk = 1/2; asserted).  The injection
    is eps at each step's start; within a step the band energy grows by 2 g dt = 0.8 %, leakage out of the band over
    t = 0.04 is O(t^2), the viscous difference is 3 % of 2e-5: the ratio lies within about [0.99, 1.02], and the bounds
    leave a five-fold margin."""
    from mpi4py_fft_amd import comm
    e0, E = _example().solve(comm.COMM_SELF, M=5, nsteps=0, spectrum=True)
    assert E[0][3] > 0.12 and abs(E[0].sum() - E[0][3]) <= 1e-20 * E[0][3] and abs(e0 - E[0][3]) <= 1e-12, (e0, E[0][:6])
    (unforced, _), (forced, st) = _dns('unforced'), _dns('forced')
    ratio = (forced - unforced) / (DNS_EPS * DNS['nsteps'] * DNS['dt'])
    print('injected / (eps t) = %.5f; last gain %.6f, band energy %.6f' % (ratio, st['gain'], st['band_energy']))
    assert 0.9 <= ratio <= 1.1, (forced, unforced, ratio)
    assert abs(2 * st['gain'] * st['band_energy'] - DNS_EPS) <= 4 * 2.0 ** -52 * DNS_EPS


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_dns_device_gain_equals_host_gain(graph):
    """The gain kept in device memory gives the solution of the gain computed on the host to rounding (not bit for bit: the
    spectrum's bins repeat only to rounding), also when the whole forced RK4 step replays from a HIP graph."""
    from mpi4py_fft_amd import comm
    host, sh = _dns('forced')
    sd = {}
    dev = _example().solve(comm.COMM_SELF, forcing=(DNS_EPS, 3, 3), device_gain=True, graph=graph, stats=sd, **DNS)
    assert abs(dev - host) <= 1e-12, (dev, host)
    assert abs(sd['gain'] - sh['gain']) <= 1e-12 * sh['gain'] and abs(sd['band_energy'] - sh['band_energy']) <= 1e-12 * sh['band_energy']
