"""Host logic of the band forcing (no GPU): the rank reduction of `SpectralOps.forcing_gain` over numpy stand-ins for the
kernels, the `force=` argument forms of `SpectralOps.project`, the gain formula, and the argument checks of
gfft_ps_force_gain and gfft_ps_project_forced."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import cases, forcing_ref as F, spectrum_ref as R
from tests.host_engine import HostEngine


def _h(t):
    """A tensor's values on the host (the arrays live on the default device, which is the GPU where there is one)"""
    return t.detach().cpu().numpy()


class ForcingEngine(HostEngine):
    """HostEngine plus the spectrum, the projection and the two forcing entries restated with numpy (tests/spectrum_ref.py,
    tests/forcing_ref.py) on host tensors.  `log` records every call's name and scalar arguments."""
    log = []

    def ps_spectrum(self, tu, ncomp, k, w2, shape, dk, nbins, tout, precision):
        ForcingEngine.log.append(('ps_spectrum', int(nbins), float(dk)))
        u = _h(tu).reshape((ncomp,) + tuple(shape))
        w = np.ones(shape[2]) if w2 is None else _h(w2).astype('d')
        bins, _ = R.reference(u, [_h(ki).astype('d') for ki in k], w, dk, nbins)
        tout.copy_(torch.as_tensor(bins))

    def ps_project(self, tdu, tu, k, shape, nu, precision):
        ForcingEngine.log.append(('ps_project', float(nu)))
        kd = [_h(ki).astype('d') for ki in k]
        tdu.copy_(torch.as_tensor(F.projected(_h(tdu), _h(tu), kd, nu).astype(_h(tdu).dtype)))

    def ps_force_gain(self, tspec, nbins, blo, bhi, eps, gain_max, tgain):
        ForcingEngine.log.append(('ps_force_gain', int(nbins), int(blo), int(bhi), float(eps), float(gain_max)))
        assert tuple(tspec.shape) == (2, nbins)
        tgain.copy_(torch.as_tensor(F.force_gain(_h(tspec)[0], blo, bhi, eps, gain_max), dtype=torch.float64))

    def ps_project_forced(self, tdu, tu, k, shape, nu, dk, blo, bhi, gain, tgain, precision):
        ForcingEngine.log.append(('ps_project_forced', float(nu), float(dk), int(blo), int(bhi), float(gain), tgain))
        g = float(gain) if tgain is None else float(tgain.reshape(-1)[0])
        kd = [_h(ki).astype('d') for ki in k]
        tdu.copy_(torch.as_tensor(F.forced_rhs(_h(tdu), _h(tu), kd, nu, g, blo, bhi, dk).astype(_h(tdu).dtype)))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(ForcingEngine())
    ForcingEngine.log = []
    yield
    _lib.set_engine(old)


def _field(shape, seed=3):
    gs = (3,) + tuple(shape[:2]) + (shape[2] // 2 + 1,)
    rng = np.random.default_rng(seed)
    return rng.standard_normal(gs) + 1j * rng.standard_normal(gs)


@pytest.mark.parametrize('P,grid', [(1, None), (2, [2, 1, 1]), (4, [2, 2, 1])])
def test_forcing_gain_and_its_rank_reduction(P, grid, engine):
    from mpi4py_fft_amd import PFFT, newDistArray, spectral
    shape, band, eps = (8, 8, 20), (1, 3), 0.1
    G = _field(shape)
    k, w = R.wavenumbers(shape, True)
    ref, modes = R.reference(G, k, w)
    want_g, want_ef = F.force_gain(ref[0], band[0], band[1], eps)
    M = int(modes[band[0]:band[1] + 1].sum())
    assert M > 0 and want_g > 0

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=grid, wire='torch') if P > 1 else PFFT(comm, shape, dtype='d')
        ops = spectral.SpectralOps(fft, R.BOX)
        uh = newDistArray(fft, rank=1)
        uh[...] = G[(slice(None),) + fft.local_slice(True)]
        got = ops.forcing_gain(uh, eps, band)
        clamped = ops.forcing_gain(uh, eps, band, gain_max=want_g / 2)
        coarse = ops.forcing_gain(uh, eps, (1, 1), dk=1.0)
        out = torch.zeros(2, dtype=torch.float64)
        if P == 1:
            assert ops.forcing_gain(uh, eps, band, out=out) is out
            first = ops._force_spec
            ops.forcing_gain(uh, eps, band, out=out)
            assert ops._force_spec is first, 'the second call allocated'
        else:
            with pytest.raises(AssertionError, match='one-rank'):
                ops.forcing_gain(uh, eps, band, out=out)
        fft.destroy()
        return got, clamped, coarse, out.numpy().copy()
    res = cases.run_ranks(P, body)
    for got, clamped, coarse, out in res:
        assert isinstance(got, tuple) and all(isinstance(x, float) for x in got)
        assert got == res[0][0], 'ranks disagree'                          # bit for bit
        assert abs(got[1] - want_ef) <= (M + 16) * 2.0 ** -52 * want_ef
        assert abs(got[0] - want_g) <= (M + 16) * 2.0 ** -52 * want_g
        assert clamped == (want_g / 2, got[1])
        # dk = 1: shell 1 holds what shells 1..2 of dk = 1/2 hold but for the modes that move to shell 0 or 2; just a different number
        assert coarse[1] > 0 and coarse != got
        if P == 1:
            assert tuple(out) == got
    # only bhi + 1 bins are asked of the kernel, with the dk given
    spec = [c for c in ForcingEngine.log if c[0] == 'ps_spectrum']
    assert {c[1:] for c in spec} == {(4, 0.5), (2, 1.0)}
    if P == 1:
        assert ('ps_force_gain', 4, 1, 3, eps, math.inf) in ForcingEngine.log


def test_project_force_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape, nu = (8, 6, 20), 0.03
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    k, _ = R.wavenumbers(shape, True)
    uh_h, du_h = _field(shape, 5), _field(shape, 6)
    uh, du = newDistArray(fft, rank=1), newDistArray(fft, rank=1)
    uh[...] = uh_h

    def run(**kw):
        du[...] = du_h
        ForcingEngine.log = []
        assert ops.project(du, uh, nu, **kw) is du
        return np.asarray(du).copy(), ForcingEngine.log[-1]
    plain, call = run()
    assert call == ('ps_project', nu) and len(ForcingEngine.log) == 1          # force=None is today's call
    assert np.array_equal(run(force=None)[0], plain)
    got, call = run(force=(0.37, (2, 3)))
    assert call == ('ps_project_forced', nu, 0.5, 2, 3, 0.37, None)          # dk defaults to the object's
    m = F.band_mask(k, 2, 3)
    assert m.any() and not m.all()
    assert np.array_equal(got[:, ~m], plain[:, ~m]) and np.allclose(got[:, m], plain[:, m] + 0.37 * uh_h[:, m], rtol=1e-14)
    assert run(force=(0.37, (2, 3), None))[1] == call
    assert run(force=(0.37, [0, 0], 1.0))[1] == ('ps_project_forced', nu, 1.0, 0, 0, 0.37, None)
    assert run(force=(np.float64(2.0), (np.int64(1), np.int64(1))))[1][1:6] == (nu, 0.5, 1, 1, 2.0)
    g = torch.tensor([0.25, -9.0], dtype=torch.float64)
    got2, call = run(force=(g, (2, 3)))
    assert call[:5] == ('ps_project_forced', nu, 0.5, 2, 3) and call[6] is g
    assert np.array_equal(got2, run(force=(0.25, (2, 3)))[0]) and g.tolist() == [0.25, -9.0]
    for bad in ((math.nan, (1, 2)), (math.inf, (1, 2)), (0.1, (2, 1)), (0.1, (-1, 2)), (0.1, (1, 2), 0.0), (0.1, (1, 2), -1.0),
                (0.1,), (0.1, (1, 2), 0.5, 7), (torch.tensor([0.1], dtype=torch.float32), (1, 2)),
                (torch.zeros(0, dtype=torch.float64), (1, 2)), (torch.zeros((2, 2), dtype=torch.float64)[:, 0], (1, 2))):
        with pytest.raises((AssertionError, ValueError)):
            run(force=bad)
    fft.destroy()


def test_force_gain_formula():
    from mpi4py_fft_amd import spectral
    f = spectral.force_gain
    E = np.array([[0.5, 0.25, 0.125, 2.0], [9.0, 9.0, 9.0, 9.0]])
    assert f(E, (1, 2), 0.3) == (0.3 / (2.0 * 0.375), 0.375)                  # unclamped; row 0 of a [2][nbins] array
    assert f(E[0], (1, 2), 0.3) == f(E, (1, 2), 0.3)                          # or the row itself
    assert f(E, (0, 0), 0.3) == (0.3, 0.5) and f(E, (0, 3), 1.0) == (1.0 / 5.75, 2.875)
    assert f(E, (1, 2), 0.3, gain_max=0.125) == (0.125, 0.375)                # the clamp binds
    assert f(E, (1, 2), 0.3, gain_max=math.inf) == f(E, (1, 2), 0.3)
    assert f(E, (1, 2), 0.0) == (0.0, 0.375)                                  # nothing to inject
    assert f(np.zeros(4), (1, 2), 0.3) == (0.0, 0.0)                          # an empty band: no gain, not a division by zero
    assert f([1.0, -3.0, 1.0], (0, 2), 0.3) == (0.0, -1.0)                    # not an energy
    g, ef = f([1.0, math.nan, 1.0], (0, 2), 0.3)
    assert g == 0.0 and math.isnan(ef)
    assert f([1.0, math.inf, 1.0], (0, 2), 0.3) == (0.0, math.inf)
    assert f([1.0, math.nan, 1.0], (2, 2), 0.3) == (0.15, 1.0)                # a NaN outside the band is not read
    # serial, in bin order from 0.0: 1e16 + 1 + 1 loses both ones, 1 + 1 + 1e16 keeps them
    assert f([1e16, 1.0, 1.0], (0, 2), 1.0)[1] == 1e16 and f([1.0, 1.0, 1e16], (0, 2), 1.0)[1] == 1e16 + 2
    assert f([1e-320], (0, 0), 1.0) == (math.inf, 1e-320) and f([1e-320], (0, 0), 1.0, 50.0) == (50.0, 1e-320)
    for E_, band, eps, gmax in ((E, (1, 2), 0.3, math.inf), (E, (0, 3), 7.0, 0.5), (np.zeros(3), (0, 2), 1.0, 1.0),
                                ([1e16, 1.0, 1.0], (0, 2), 1.0, math.inf)):
        assert f(E_, band, eps, gmax) == F.force_gain(np.asarray(E_, dtype='d').reshape(-1, np.shape(E_)[-1])[0], band[0], band[1], eps, gmax)
    for band in ((2, 1), (-1, 2), (0, 4)):
        with pytest.raises(AssertionError):
            f(E, band, 0.3)


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    for name in ('gfft_ps_force_gain', 'gfft_ps_project_forced'):
        assert name in _lib.EXPORTS
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = math.nan, math.inf

    def gain(spec=p, nbins=8, blo=2, bhi=4, eps=0.1, gmax=inf, out=p):
        return lib.gfft_ps_force_gain(spec, nbins, blo, bhi, eps, gmax, out, None)
    for bad in (dict(spec=None), dict(out=None), dict(nbins=0), dict(nbins=-1), dict(blo=-1), dict(blo=5), dict(bhi=8),
                dict(bhi=1), dict(eps=nan), dict(eps=inf), dict(eps=-inf), dict(eps=-0.1), dict(gmax=nan), dict(gmax=0.0),
                dict(gmax=-1.0), dict(gmax=-inf)):
        assert gain(**bad) == -1, bad

    def proj(du=p, u=p, k0=p, k1=p, k2=p, n=(2, 2, 2), nu=0.03, dk=0.5, blo=2, bhi=4, g=0.37, dg=None, prec=8):
        return lib.gfft_ps_project_forced(du, u, k0, k1, k2, n[0], n[1], n[2], nu, dk, blo, bhi, g, dg, prec, None)
    for bad in (dict(du=None), dict(u=None), dict(k0=None), dict(k1=None), dict(k2=None), dict(n=(-1, 2, 2)), dict(n=(2, -1, 2)),
                dict(n=(2, 2, -1)), dict(prec=3), dict(prec=16), dict(dk=0.0), dict(dk=-0.5), dict(dk=nan), dict(blo=-1),
                dict(blo=5), dict(bhi=1), dict(g=nan), dict(g=inf), dict(g=-inf)):
        assert proj(**bad) == -1, bad
    for n in ((2, (1 << 30) + 1, 2), (2, 2, (1 << 30) + 1)):
        assert proj(n=n) == -2, n                       # beyond the documented limit: unsupported, not invalid
        assert proj(n=n, dk=0.0) == -1                   # (and a bad argument beside it is still a bad argument)
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device
        assert gain() == -3 and gain(blo=0, bhi=0, nbins=1, eps=0.0, gmax=1e-300) == -3 and gain(bhi=7) == -3
        assert proj() == -3 and proj(prec=4, blo=0, bhi=0) == -3 and proj(n=(0, 2, 2)) == -3
        assert proj(g=nan, dg=p) == -3                   # `gain` is not looked at when d_gain is given
        assert proj(n=(5, 1 << 30, 1 << 30)) == -3       # 2^30 itself is allowed
