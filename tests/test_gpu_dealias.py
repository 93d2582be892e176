"""gfft_ps_project_dealiased / gfft_ps_dealias on the device against tests/dealias_ref.py (numpy, float64) and against
gfft_ps_project / gfft_ps_project_forced themselves.

Boxes without ties only (spectrum_ref.BOX, dk = 1/2: every |k|^2 / dk^2 is an integer; the cuts are kcut = 2.5 and
kcut = sqrt(q + 1/2) dk), so the reference mask and a correct device cannot disagree about a mode.  The contract is exact:
  * a kept mode carries the bits of gfft_ps_project, or of gfft_ps_project_forced where forced;
  * a truncated mode carries the bits of +0.0, whatever du_hat and u_hat hold there;
  * gfft_ps_dealias leaves the bits of a kept mode alone.
Only the end-to-end chain has a rounding bound, derived in its test.

Launch geometry the shapes are chosen against (csrc/spectral.hip): grid-stride, 256 lanes per workgroup, at most 16384
workgroups, a lane's mode is its flat index.  (24, 16, 20) and (12, 10, 21) have spectral blocks 24 x 16 x 11 and 12 x 10 x 11:
rows of 11, shorter than a wave, 17 and 6 workgroups, the last one ragged; the 2/3 rule keeps 1155 of 4224 and 343 of 1320
modes, so kept and truncated lanes share waves.  (160, 160, 328) has 4 224 000 modes > 16384 * 256: a second grid-stride step.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, dealias_ref as D, forcing_ref as F, spectrum_ref as R

SHAPES = [(24, 16, 20), (12, 10, 21)]
KEPT = {(24, 16, 20): (1155, 4224), (12, 10, 21): (343, 1320)}
NU = 0.03
GAIN = 0.37
BAND = (4, 12)                      # 1.75 <= |k| < 6.25: straddles the box cut and every spherical cut below
QS = (17, 40, 150)                  # kcut = sqrt(q + 1/2) dk = 2.09, 3.18, 6.13: |k|^2 / dk^2 is an integer, no ties


def _bits(a):
    """The bit patterns of a complex or real array (so that -0.0 != 0.0 and a NaN equals itself)"""
    a = np.ascontiguousarray(a)
    r = a.view(a.real.dtype)
    return r.view('u8' if r.dtype == np.float64 else 'u4')


def _kcut(q):
    return float(np.sqrt(q + 0.5) * R.DK)


_REF = {}


def _fields(shape, dt):
    """(u_hat, du_hat, k, w): random [3] + spectral shape in the precision under test; computed once per case and shared,
    never modified"""
    key = (tuple(shape), dt)
    if key not in _REF:
        gs = (3,) + tuple(shape[:2]) + (shape[2] // 2 + 1,)
        rng = np.random.default_rng(31)
        uh = (rng.standard_normal(gs) + 1j * rng.standard_normal(gs)).astype(dt.upper())
        du = (rng.standard_normal(gs) + 1j * rng.standard_normal(gs)).astype(dt.upper())
        k, w = R.wavenumbers(shape, True)
        for a in (uh, du):
            a.setflags(write=False)
        _REF[key] = (uh, du, k, w)
    return _REF[key]


def _masks(shape, k):
    """name -> (rule for dealias_mask, kcut, numpy keep mask, straddled by BAND?)"""
    v = D.keep_vectors(shape)
    ones = [np.ones(len(ki), dtype=bool) for ki in k]
    out = {'2/3': ('2/3', None, D.keep_mask(k, v), True)}
    for q in QS:
        out['kcut q=%d' % q] = (None, _kcut(q), D.keep_mask(k, None, _kcut(q)), True)
    out['2/3 + kcut'] = ('2/3', _kcut(40), D.keep_mask(k, v, _kcut(40)), True)
    out['one axis + kcut'] = ([None, v[1], None], _kcut(150), D.keep_mask(k, [None, v[1], None], _kcut(150)), True)
    out['only k = 0'] = (None, 0.0, D.keep_mask(k, None, 0.0), False)
    out['all-keep, no vectors'] = (None, None, D.keep_mask(k), False)
    out['all-keep, vectors of ones'] = (ones, None, D.keep_mask(k, ones), False)
    out['keep-nothing'] = ([ones[0], np.zeros(len(k[1]), dtype=bool), ones[2]], None, np.zeros_like(out['2/3'][2]), False)
    return out


def _ops(comm, shape, dt, **kw):
    from mpi4py_fft_amd import PFFT, spectral
    fft = PFFT(comm, shape, dtype=dt, **kw)
    return fft, spectral.SpectralOps(fft, R.BOX)


def _dev(fft, G):
    from mpi4py_fft_amd import newDistArray
    a = newDistArray(fft, rank=1)
    a[...] = np.array(G[(slice(None),) + fft.local_slice(True)])
    return a


def _plain(fft, ops, uh, du):
    """What gfft_ps_project and gfft_ps_project_forced (BAND) leave: the bits a kept mode must carry"""
    U, P, Q = _dev(fft, uh), _dev(fft, du), _dev(fft, du)
    ops.project(P, U, NU)
    ops.project(Q, U, NU, force=(GAIN, BAND))
    return U, np.asarray(P).copy(), np.asarray(Q).copy()


def _check(got, want, keep, what):
    assert np.array_equal(_bits(got[:, keep]), _bits(want[:, keep])), (what, 'a kept mode differs from the projection without a mask')
    assert not _bits(got[:, ~keep]).any(), (what, 'a truncated mode is not +0.0')


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_bits(shape, dt):
    from mpi4py_fft_amd import comm
    uh, du, k, _ = _fields(shape, dt)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    U, p, pf = _plain(fft, ops, uh, du)
    assert np.abs(p - F.projected(du, uh, k, NU)).max() <= (1e-13 if dt == 'd' else 2e-5) * np.abs(p).max()
    band = F.band_mask(k, *BAND)
    assert not np.array_equal(p[:, band], pf[:, band]) and np.all(p != 0) and np.all(pf != 0)
    for name, (rule, kcut, keep, straddled) in _masks(shape, k).items():
        mask = ops.dealias_mask(rule, kcut)
        if straddled:
            assert (band & keep).any() and (band & ~keep).any() and (~band & keep).any(), (shape, name)
        for force, want in ((None, p), ((GAIN, BAND), pf)):
            Dv = _dev(fft, du)
            ops.project(Dv, U, NU, force=force, dealias=mask)
            _check(np.asarray(Dv).copy(), want, keep, (shape, dt, name, force))
    assert (int(_masks(shape, k)['2/3'][2].sum()), uh[0].size) == KEPT[shape]
    assert int(_masks(shape, k)['only k = 0'][2].sum()) == 1
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_inclusive_edge(shape, dt):
    """kcut = 2.5: kcut^2 = 6.25 exactly, and modes such as k = (2, 1.5, 0) and (0, 2.5, 0) have |k|^2 = 6.25 exactly: kept.
    The next larger |k|^2 is not."""
    from mpi4py_fft_amd import comm
    uh, du, k, _ = _fields(shape, dt)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    U, p, _ = _plain(fft, ops, uh, du)
    k2 = D.k2sq(k)
    edge, nxt = k2 == 6.25, k2 == k2[k2 > 6.25].min()
    assert edge.sum() >= 4 and nxt.any() and k2[nxt][0] <= 7.25
    Dv = _dev(fft, du)
    ops.project(Dv, U, NU, dealias=ops.dealias_mask(None, 2.5))
    got = np.asarray(Dv).copy()
    assert np.array_equal(_bits(got[:, edge]), _bits(p[:, edge])) and np.all(got[:, edge] != 0), 'the edge is not inclusive'
    assert not _bits(got[:, nxt]).any()
    _check(got, p, k2 <= 6.25, (shape, dt))
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_nan_in_truncated_modes(shape, dt):
    """du_hat and u_hat are NaN at every truncated mode: the output is +0.0 there (nothing was loaded), and the kept modes
    carry the bits they carry without the NaNs."""
    from mpi4py_fft_amd import comm
    uh, du, k, _ = _fields(shape, dt)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    _, p, pf = _plain(fft, ops, uh, du)
    rule, kcut, keep, _ = _masks(shape, k)['2/3 + kcut']
    mask = ops.dealias_mask(rule, kcut)
    un, dn = np.array(uh), np.array(du)
    un[:, ~keep] = np.nan + 1j * np.nan
    dn[:, ~keep] = np.nan + 1j * np.nan
    Un = _dev(fft, un)
    for force, want in ((None, p), ((GAIN, BAND), pf)):
        Dv = _dev(fft, dn)
        ops.project(Dv, Un, NU, force=force, dealias=mask)
        _check(np.asarray(Dv).copy(), want, keep, (shape, dt, force))
    # (the same data without the mask does carry the NaNs through)
    Dv = _dev(fft, dn)
    ops.project(Dv, Un, NU)
    assert np.isnan(np.asarray(Dv)[:, ~keep].real).all()
    fft.destroy()


def test_past_one_grid_sweep():
    """fp32, 4 224 000 modes: more than 16384 * 256, so lanes take a second grid-stride step; the plane k0 = -1 lies wholly
    in it and holds kept and truncated modes.  Straight through the engine; the mask is dealias_ref's, and on the planes
    k0 = 0 and k0 = -1 the values are compared with dealias_ref.dealiased_rhs as well."""
    from mpi4py_fft_amd import _lib
    shape = (160, 160, 328)
    k, _ = R.wavenumbers(shape, True)
    sshape = tuple(len(ki) for ki in k)
    count = int(np.prod(sshape))
    assert sshape == (160, 160, 165) and count > 16384 * 256
    v = D.keep_vectors(shape)
    assert [int(x.sum()) for x in v] == [107, 107, 110]
    keep = D.keep_mask(k, v)
    assert keep[-1].any() and not keep[-1].all() and (sshape[0] - 1) * sshape[1] * sshape[2] >= 16384 * 256 and k[0][-1] == -1.0
    K = [torch.as_tensor(ki.astype('f'), device='cuda') for ki in k]
    M = [torch.as_tensor(x.astype(np.uint8), device='cuda') for x in v]
    gen = torch.Generator(device='cuda').manual_seed(37)
    U = torch.randn((3,) + sshape + (2,), dtype=torch.float32, device='cuda', generator=gen)
    D0 = torch.randn((3,) + sshape + (2,), dtype=torch.float32, device='cuda', generator=gen)
    eng = _lib.engine()
    plain, got = D0.clone(), D0.clone()
    eng.ps_project(plain, U, K, sshape, NU, 4)
    eng.ps_project_dealiased(got, U, K, M, sshape, NU, np.inf, None, 4)
    m = torch.as_tensor(keep, device='cuda')
    same = (plain.view(torch.int32) == got.view(torch.int32)).all(-1)             # [3] + sshape: both halves of a mode
    assert bool(same[:, m].all()), 'a kept mode differs from gfft_ps_project'
    assert not bool(got.view(torch.int32)[:, ~m].any()), 'a truncated mode is not +0.0'
    assert bool((got[:, m] != 0).any(-1).all())
    for i0 in (0, sshape[0] - 1):
        kk = [k[0][i0:i0 + 1], k[1], k[2]]
        c = lambda t: np.ascontiguousarray(t[:, i0:i0 + 1].cpu().numpy(), dtype='d').view('D')[..., 0]
        ref = D.dealiased_rhs(c(D0), c(U), kk, NU, keep[i0:i0 + 1])
        assert np.abs(c(got) - ref).max() <= 2e-5 * np.abs(ref).max(), i0
    # gfft_ps_dealias on the same block: kept modes untouched, the others +0.0
    f = D0.clone()
    eng.ps_dealias(f, 3, K, M, sshape, np.inf, 4)
    same = (f.view(torch.int32) == D0.view(torch.int32)).all(-1)
    assert bool(same[:, m].all()) and not bool(f.view(torch.int32)[:, ~m].any())


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_dealias_in_place(shape, dt):
    """SpectralOps.dealias on one- and three-component fields and a scalar-shaped field: a NaN, a -0.0 and a denormal
    planted among the kept modes survive bit for bit (kept modes are neither read nor written), truncated modes -- NaN
    before -- are +0.0."""
    from mpi4py_fft_amd import comm
    uh, _, k, _ = _fields(shape, dt)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    tiny = np.finfo(uh.real.dtype).tiny
    for name in ('2/3', 'kcut q=40', '2/3 + kcut', 'all-keep, no vectors', 'keep-nothing'):
        rule, kcut, keep, _ = _masks(shape, k)[name]
        mask = ops.dealias_mask(rule, kcut)
        src = np.array(uh)
        src[:, ~keep] = np.nan + 1j * np.nan
        where = np.argwhere(keep)
        if len(where):
            assert len(where) >= 3
            for c in range(3):
                a, b, d = (tuple(w) for w in where[[0, len(where) // 2, -1]])
                src[c][a] = complex(np.nan, -0.0)
                src[c][b] = complex(-0.0, tiny / 4)                  # a denormal
                src[c][d] = complex(tiny / 8, np.nan)
        for form in ('vector', 'one', 'scalar'):
            t = torch.as_tensor(src if form == 'vector' else src[1:2] if form == 'one' else src[1], device='cuda').contiguous()
            assert ops.dealias(t, mask) is t
            got = t.cpu().numpy().reshape((-1,) + keep.shape)
            want = src if form == 'vector' else src[1:2]
            assert np.array_equal(_bits(got[:, keep]), _bits(want[:, keep])), (shape, dt, name, form, 'a kept mode changed')
            assert not _bits(got[:, ~keep]).any(), (shape, dt, name, form, 'a truncated mode is not +0.0')
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_spectrum_after_dealias(shape, dt):
    """After `dealias` with a spherical cut every bin above floor(kcut / dk + 1/2) is exactly 0.0 and the rest are the bins of
    the numpy-masked field (spectrum_ref.assert_bins)."""
    from mpi4py_fft_amd import comm
    uh, _, k, w = _fields(shape, dt)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    for rule, q in ((None, 40), ('2/3', 150)):
        kcut = _kcut(q)
        keep = D.keep_mask(k, D.keep_vectors(shape, rule), kcut)
        U = _dev(fft, uh)
        ops.dealias(U, ops.dealias_mask(rule, kcut))
        got = ops.spectrum(U)
        top = int(np.floor(kcut / R.DK + 0.5))
        assert 0 < top < got.shape[1] - 1 and np.all(got[:, top + 1:] == 0.0) and got[0, top] > 0, (shape, dt, q, top)
        ref, modes = R.reference(np.where(keep[None], uh, 0), k, w)
        R.assert_bins(got, ref, modes, '%s %s %s q=%d' % (shape, dt, rule, q))
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_alias_free_end_to_end(shape, dt):
    """curl -> backward x 6 -> cross -> forward x 3 -> project(nu = 0, dealias=mask) of a field truncated by the 2/3 rule
    equals, in the kept modes, the projected EXACT convolution (dealias_ref.exact_nonlinear, evaluated on the 2N-grid).
    Bound: the same kernels without truncation, on the untruncated field, against numpy's evaluation of the same chain on
    the N-grid (aliased alike, so only rounding separates them) err by e0 = max |error| / max |reference|; the dealiased
    chain runs those kernels on fewer non-zero modes and gets 4 max(e0, eps log2(nelem)) -- the 4 for the different data,
    the floor so that a luckily small e0 does not tighten it.  An aliased result misses by the size of the aliasing
    error, O(0.1 ... 1) of the reference: more than ten orders of magnitude above the bound in fp64."""
    from mpi4py_fft_amd import comm, newDistArray, spectral
    rng = np.random.default_rng(41)
    u = rng.standard_normal((3,) + shape)
    full = (np.array([np.fft.rfftn(a) for a in u]) / np.prod(shape)).astype(dt.upper())
    k, _ = R.wavenumbers(shape, True)
    keep = D.keep_mask(k, D.keep_vectors(shape))
    trunc = np.where(keep[None], full, 0).astype(dt.upper())
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    mask = ops.dealias_mask('2/3')
    U, W, X = (newDistArray(fft, False, rank=1) for _ in range(3))
    W_hat, dU = newDistArray(fft, rank=1), newDistArray(fft, rank=1)

    def chain(field, **kw):
        U_hat = _dev(fft, field)
        ops.curl(U_hat, W_hat)
        for j in range(3):
            fft.backward(U_hat[j], U[j])
            fft.backward(W_hat[j], W[j])
        spectral.cross(U, W, X)
        for j in range(3):
            fft.forward(X[j], dU[j])
        U_hat = _dev(fft, field)                                  # (afresh: nothing here relies on backward keeping its input)
        ops.project(dU, U_hat, 0.0, **kw)
        return np.asarray(dU).copy().astype('D')
    zero = np.zeros_like(full)
    ref0 = F.projected(D.nonlinear(full, shape), zero, k, 0.0)
    got0 = chain(full)
    e0 = float(np.abs(got0 - ref0).max() / np.abs(ref0).max())
    ref = F.projected(D.exact_nonlinear(trunc, shape), zero, k, 0.0)
    got = chain(trunc, dealias=mask)
    err = float(np.abs(got - ref)[:, keep].max() / np.abs(ref[:, keep]).max())
    bound = 4 * max(e0, cases.rounding_tol(dt, int(np.prod(shape)), 1.0))
    # how far an aliased result is: the chain on the UNtruncated field, in the kept modes, against the exact convolution
    aliased = float(np.abs(got0 - ref)[:, keep].max() / np.abs(ref[:, keep]).max())
    print('%s %s: undealiased chain against numpy e0 = %.3e; dealiased chain against the exact convolution %.3e (bound %.3e); '
          'without truncating the input %.3e' % (shape, dt, e0, err, bound, aliased))
    assert not _bits(got.astype(dt.upper())[:, ~keep]).any()
    assert err <= bound, (shape, dt, err, bound, e0)
    fft.destroy()


@pytest.mark.parametrize('P,grid', [(2, [2, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'pencil4'])
def test_thread_ranks(P, grid):
    """Each rank's dealiased, forced block is bit for bit its part of the one-rank result: the mask vectors are sliced as K is."""
    from mpi4py_fft_amd import comm
    shape, dt = (24, 16, 20), 'd'
    uh, du, k, _ = _fields(shape, dt)
    rule, kcut, keep, _ = _masks(shape, k)['2/3 + kcut']
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    Dv = _dev(fft, du)
    ops.project(Dv, _dev(fft, uh), NU, force=(GAIN, BAND), dealias=ops.dealias_mask(rule, kcut))
    one = np.asarray(Dv).copy()
    fft.destroy()
    assert not _bits(one[:, ~keep]).any() and np.all(one[:, keep] != 0)

    def body(c):
        fft, ops = _ops(c, shape, dt, grid=grid)
        U, Dv, S = _dev(fft, uh), _dev(fft, du), _dev(fft, du)
        mask = ops.dealias_mask(rule, kcut)
        ops.project(Dv, U, NU, force=(GAIN, BAND), dealias=mask)
        ops.dealias(S, mask)
        block, alone = np.asarray(Dv).copy(), np.asarray(S).copy()
        sl = fft.local_slice(True)
        fft.destroy()
        return block, alone, sl
    res = cases.run_ranks(P, body)
    for block, alone, sl in res:
        at = (slice(None),) + tuple(sl)
        assert np.array_equal(_bits(block), _bits(one[at])), (P, grid, sl)
        assert np.array_equal(_bits(alone), _bits(np.where(keep[None], du, 0)[at])), (P, grid, sl)
    assert len({str(sl) for _, _, sl in res}) == P


def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_dealias', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example():
    """The dealiased Taylor-Green run: fused kernels against the array-sized torch expressions with the same mask, and
    against its own replay from a HIP graph; the recorded energy; and the undealiased run's known answer."""
    from mpi4py_fft_amd import comm
    ex = _example()
    fused = ex.solve(comm.COMM_SELF, dealias='2/3')
    base = ex.solve(comm.COMM_SELF, dealias='2/3', fused=False)
    graph = ex.solve(comm.COMM_SELF, dealias='2/3', graph=True)
    plain = ex.solve(comm.COMM_SELF)
    print('dealiased energy %.15f (torch expressions %.15f, graph %.15f); undealiased %.15f' % (fused, base, graph, plain))
    assert abs(fused - base) <= 1e-10, (fused, base)
    assert abs(fused - graph) <= 1e-12, (fused, graph)
    assert round(plain - 0.124953117517, 7) == 0, plain
    assert abs(fused - ex.DEALIASED_ENERGY) <= 1e-9, (fused, ex.DEALIASED_ENERGY)
