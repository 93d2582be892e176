"""Host logic of the dealiasing truncation (no GPU): the mask vectors of `SpectralOps.dealias_mask` and their slicing over a
grid of ranks, the `dealias=` argument forms of `SpectralOps.project` and `SpectralOps.dealias` over numpy stand-ins for
the kernels, the argument checks of gfft_ps_project_dealiased and gfft_ps_dealias, and the reference itself: the strict
2/3 rule is alias-free, the looser rule often seen is not."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import dealias_ref as D, forcing_ref as F, spectrum_ref as R
from tests.test_forcing_host import ForcingEngine, _field, _h


class DealiasEngine(ForcingEngine):
    """ForcingEngine plus the two dealiasing entries restated with numpy (tests/dealias_ref.py) on host tensors"""

    @staticmethod
    def _keep(k, m, kcut):
        return D.keep_mask([_h(ki).astype('d') for ki in k], [None if mi is None else _h(mi) for mi in m], kcut)

    def ps_project_dealiased(self, tdu, tu, k, m, shape, nu, kcut, force, precision):
        ForcingEngine.log.append(('ps_project_dealiased', float(nu), float(kcut), force, tuple(m)))
        kd = [_h(ki).astype('d') for ki in k]
        f = None
        if force is not None:
            dk, blo, bhi, gain, tgain = force
            f = (float(gain) if tgain is None else float(tgain.reshape(-1)[0]), blo, bhi)
            assert dk == R.DK
        out = D.dealiased_rhs(_h(tdu), _h(tu), kd, nu, self._keep(k, m, kcut), f)
        tdu.copy_(torch.as_tensor(out.astype(_h(tdu).dtype)))

    def ps_dealias(self, tf, ncomp, k, m, shape, kcut, precision):
        ForcingEngine.log.append(('ps_dealias', int(ncomp), float(kcut), tuple(m)))
        keep = self._keep(k, m, kcut)
        a = _h(tf).reshape((ncomp,) + tuple(shape))             # (a view of the tensor's memory: in place)
        a[:, ~keep] = 0


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(DealiasEngine())
    ForcingEngine.log = []
    yield
    _lib.set_engine(old)


STRICT = {48: 15, 21: 6, 64: 21}             # N: the largest |n| with 3 |n| < N


def test_the_rule_is_strict():
    for N, top in STRICT.items():
        assert 3 * top < N <= 3 * (top + 1)
    for shape in ((48, 64, 21), (21, 48, 64)):
        for keep, n, N in zip(D.keep_vectors(shape), D.ints(shape), shape):
            assert np.array_equal(keep, np.abs(n) <= STRICT[N]), (shape, N)
            assert not keep[np.abs(n) * 2 == N].any() and keep[0]          # the Nyquist plane is never kept


@pytest.mark.parametrize('shape', [(48, 64, 21), (21, 48, 64)], ids=str)
@pytest.mark.parametrize('P,grid', [(1, None), (2, [2, 1, 1]), (4, [2, 2, 1])])
def test_mask_vectors_are_slices_of_the_global_ones(P, grid, shape, engine):
    from mpi4py_fft_amd import PFFT, spectral
    from tests import cases
    n = D.ints(shape)
    want = [np.abs(ni) <= STRICT[N] for ni, N in zip(n, shape)]
    own = [np.arange(len(ni)) % 3 != 1 for ni in n]                         # a rule of the caller's own

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=grid, wire='torch') if P > 1 else PFFT(comm, shape, dtype='d')
        ops = spectral.SpectralOps(fft, R.BOX)
        sl = tuple(fft.local_slice(True))
        a, b, c = ops.dealias_mask(), ops.dealias_mask(None, kcut=2.5), ops.dealias_mask([own[0], None, own[2]])
        assert isinstance(a, spectral.DealiasMask) and a.kcut == math.inf == c.kcut and b == (None, None, None, 2.5)
        assert c.m1 is None and ops.dealias_mask('2/3', 3.0).kcut == 3.0
        for m in a[:3] + (c.m0, c.m2):
            assert m.dtype == torch.uint8 and m.is_contiguous() and m.device == ops.K[0].device
        assert tuple(len(m) for m in a[:3]) == ops.shape
        with pytest.raises(AssertionError):
            ops.dealias_mask('3/2')
        with pytest.raises(AssertionError):
            ops.dealias_mask([own[0][:-1], None, None])                     # not the global length
        with pytest.raises(AssertionError):
            ops.dealias_mask(kcut=-1.0)
        fft.destroy()
        return sl, [_h(m).astype(bool) for m in a[:3]], [_h(c.m0).astype(bool), _h(c.m2).astype(bool)]
    res = cases.run_ranks(P, body)
    seen = [np.zeros(len(ni), dtype=int) for ni in n]
    for sl, got, got_own in res:
        for ax in range(3):
            assert np.array_equal(got[ax], want[ax][sl[ax]]), (P, shape, ax, sl)
            seen[ax][sl[ax]] += 1
        assert np.array_equal(got_own[0], own[0][sl[0]]) and np.array_equal(got_own[1], own[2][sl[2]])
    assert all(s.min() >= 1 for s in seen), 'the ranks do not cover the axes'
    assert len({str(sl) for sl, _, _ in res}) == P


def test_project_dealias_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape, nu = (8, 6, 20), 0.03
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    k, _ = R.wavenumbers(shape, True)
    uh_h, du_h = _field(shape, 5), _field(shape, 6)
    uh, du = newDistArray(fft, rank=1), newDistArray(fft, rank=1)
    uh[...] = uh_h

    def run(*a, **kw):
        du[...] = du_h
        ForcingEngine.log = []
        assert ops.project(du, uh, nu, *a, **kw) is du
        assert len(ForcingEngine.log) == 1
        return np.asarray(du).copy(), ForcingEngine.log[-1]
    # dealias=None: the old engine entries with the old arguments, positional calls included
    plain, call = run()
    assert call == ('ps_project', nu)
    assert run(dealias=None)[1] == call and run(None)[1] == call and run(None, None)[1] == call
    forced, call = run((0.37, (2, 3)))
    assert call == ('ps_project_forced', nu, 0.5, 2, 3, 0.37, None)
    assert run(force=(0.37, (2, 3)), dealias=None)[1] == call
    # the mask of dealias_mask, with and without force=
    mask = ops.dealias_mask('2/3', kcut=2.5)
    keep = D.keep_mask(k, D.keep_vectors(shape), 2.5)
    assert keep.any() and not keep.all() and int(keep.sum()) < int(D.keep_mask(k, D.keep_vectors(shape)).sum())
    got, call = run(dealias=mask)
    assert call[:4] == ('ps_project_dealiased', nu, 2.5, None) and all(a is b for a, b in zip(call[4], mask[:3]))
    assert np.array_equal(got[:, keep], plain[:, keep]) and np.all(got[:, ~keep] == 0)
    got, call = run(force=(0.37, (2, 3)), dealias=mask)
    assert call[:4] == ('ps_project_dealiased', nu, 2.5, (0.5, 2, 3, 0.37, None))
    assert np.array_equal(got[:, keep], forced[:, keep]) and np.all(got[:, ~keep] == 0)
    band = F.band_mask(k, 2, 3)
    assert (band & keep).any() and (band & ~keep).any() and not np.array_equal(forced[:, keep], plain[:, keep])
    g = torch.tensor([0.37, -9.0], dtype=torch.float64)
    got2, call = run(force=(g, (2, 3), None), dealias=mask)
    assert call[3][:4] == (0.5, 2, 3, 0.0) and call[3][4] is g and np.array_equal(got2, got)
    # any 4-sequence; kcut None = inf; None vectors; bool vectors
    got, call = run(dealias=(mask.m0, None, mask.m2, None))
    assert call[2] == math.inf and call[4][1] is None
    k1 = D.keep_mask(k, [_h(mask.m0), None, _h(mask.m2)])
    assert np.array_equal(got[:, k1], plain[:, k1]) and np.all(got[:, ~k1] == 0)
    assert np.array_equal(run(dealias=[mask.m0.bool(), None, mask.m2, math.inf])[0], got)
    assert np.array_equal(run(dealias=ops.dealias_mask(None))[0], plain)           # keeps everything
    assert np.all(run(dealias=ops.dealias_mask(None, kcut=0.0))[0][:, 1:] == 0)
    for bad in ((mask.m0, mask.m1, mask.m2), (mask.m0, mask.m1, mask.m2, -1.0), (mask.m0, mask.m1, mask.m2, math.nan),
                (mask.m1, mask.m0, mask.m2, None), (mask.m0.double(), None, None, None), (_h(mask.m0), None, None, None),
                (torch.ones((len(mask.m0), 2), dtype=torch.uint8)[:, 0], None, None, None), '2/3'):
        with pytest.raises((AssertionError, ValueError, TypeError)):
            run(dealias=bad)
    with pytest.raises((AssertionError, ValueError)):
        run(force=(math.nan, (1, 2)), dealias=mask)                          # the forced projection's own conditions
    # SpectralOps.dealias: [m] + shape and scalar shape, in place, returns its argument
    ForcingEngine.log = []
    du[...] = du_h
    assert ops.dealias(du, mask) is du
    one = torch.as_tensor(du_h[0].copy())
    assert ops.dealias(one, mask) is one
    assert [c[:3] for c in ForcingEngine.log] == [('ps_dealias', 3, 2.5), ('ps_dealias', 1, 2.5)]
    got = np.asarray(du)
    assert np.array_equal(got[:, keep], du_h[:, keep]) and np.all(got[:, ~keep] == 0)
    assert np.array_equal(_h(one)[keep], du_h[0][keep]) and np.all(_h(one)[~keep] == 0)
    fft.destroy()


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    for name in ('gfft_ps_project_dealiased', 'gfft_ps_dealias'):
        assert name in _lib.EXPORTS
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = math.nan, math.inf

    def proj(du=p, u=p, k0=p, k1=p, k2=p, m=(p, p, p), n=(2, 2, 2), nu=0.03, kcut=2.5, forced=0, dk=0.5, blo=2, bhi=4, g=0.37,
             dg=None, prec=8):
        return lib.gfft_ps_project_dealiased(du, u, k0, k1, k2, m[0], m[1], m[2], n[0], n[1], n[2], nu, kcut, forced, dk, blo, bhi,
                                             g, dg, prec, None)
    band = (dict(dk=0.0), dict(dk=-0.5), dict(dk=nan), dict(blo=-1), dict(blo=5), dict(bhi=1), dict(g=nan), dict(g=inf), dict(g=-inf))
    for bad in (dict(du=None), dict(u=None), dict(k0=None), dict(k1=None), dict(k2=None), dict(n=(-1, 2, 2)), dict(n=(2, -1, 2)),
                dict(n=(2, 2, -1)), dict(prec=3), dict(prec=16), dict(kcut=nan), dict(kcut=-1.0), dict(kcut=-inf), dict(kcut=-1e-300)):
        assert proj(**bad) == -1, bad
        assert proj(forced=1, **bad) == -1, bad
    for bad in band:
        assert proj(forced=1, **bad) == -1, bad           # the forced projection's own conditions, when forced
        assert proj(forced=7, **bad) == -1, bad
    for n in ((2, (1 << 30) + 1, 2), (2, 2, (1 << 30) + 1)):
        assert proj(n=n) == -2, n                         # beyond the documented limit: unsupported, not invalid
        assert proj(n=n, kcut=nan) == -1                  # (and a bad argument beside it is still a bad argument)

    def deal(f=p, ncomp=3, k=(p, p, p), m=(p, p, p), n=(2, 2, 2), kcut=2.5, prec=8):
        return lib.gfft_ps_dealias(f, ncomp, k[0], k[1], k[2], m[0], m[1], m[2], n[0], n[1], n[2], kcut, prec, None)
    for bad in (dict(f=None), dict(ncomp=0), dict(ncomp=-3), dict(k=(None, p, p)), dict(k=(p, None, p)), dict(k=(p, p, None)),
                dict(k=(None, None, None), kcut=0.0), dict(n=(-1, 2, 2)), dict(n=(2, -1, 2)), dict(n=(2, 2, -1)), dict(prec=3),
                dict(prec=16), dict(kcut=nan), dict(kcut=-1.0), dict(kcut=-inf)):
        assert deal(**bad) == -1, bad
    for n in ((2, (1 << 30) + 1, 2), (2, 2, (1 << 30) + 1)):
        assert deal(n=n) == -2, n
        assert deal(n=n, ncomp=0) == -1
    assert lib.gfft_last_error() == b'gfft_ps_dealias: bad argument'
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device
        assert proj() == -3 and proj(prec=4, kcut=inf, m=(None, None, None)) == -3 and proj(kcut=0.0, n=(0, 2, 2)) == -3
        for ok in band:
            assert proj(forced=0, **ok) == -3, ok         # the band arguments are not looked at when unforced
        assert proj(forced=1) == -3 and proj(forced=1, g=nan, dg=p) == -3
        assert proj(n=(5, 1 << 30, 1 << 30)) == -3        # 2^30 itself is allowed
        assert deal() == -3 and deal(ncomp=1, prec=4, m=(None, p, None)) == -3
        assert deal(k=(None, None, None), kcut=inf) == -3  # no wavenumbers are needed without a spherical cut


@pytest.mark.parametrize('shape', [(24, 16, 20), (12, 10, 21), (9, 8, 6)], ids=str)
def test_strict_rule_is_alias_free_and_the_loose_rule_is_not(shape):
    """The reference alone.  Measured: strict 3e-16 ... 4e-16, loose 0.55 ... 1.0."""
    rng = np.random.default_rng(23)
    u = rng.standard_normal((3,) + shape)
    uh = np.array([np.fft.rfftn(a) for a in u]) / np.prod(shape)
    k, _ = R.wavenumbers(shape, True)
    err = {}
    for rule in ('2/3', 'loose'):
        m = D.keep_mask(k, D.keep_vectors(shape, rule))
        t = uh * m
        got, exact = D.nonlinear(t, shape) * m, D.exact_nonlinear(t, shape) * m
        err[rule] = float(np.abs(got - exact).max() / np.abs(exact).max())
    print('%s: N-grid against exact convolution, strict rule %.2e, loose rule %.2e' % (shape, err['2/3'], err['loose']))
    assert err['2/3'] <= 1e-14, err
    assert err['loose'] > 0.1, err
