"""Host logic of the physical-space statistics (no GPU): the rank reduction of `SpectralOps.stats` over a numpy stand-in
for the kernel, the inv_dx defaults, `moments`, the time-step formula, and the argument checks of gfft_ps_stats,
gfft_ps_timestep and gfft_ps_rk_stage_dt."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import cases, stats_ref as R
from tests.host_engine import HostEngine

BOX = (2 * np.pi, 4 * np.pi, 2 * np.pi)


class StatsEngine(HostEngine):
    """HostEngine plus gfft_ps_stats restated with numpy / fsum (tests/stats_ref.py) on host tensors."""
    seen = []

    def ps_stats(self, tu, ncomp, count, inv_dx, tout, precision):
        StatsEngine.seen.append((int(ncomp), [float(x) for x in inv_dx]))
        assert tu.numel() == ncomp * count
        out, _ = R.reference(tu.numpy().reshape(ncomp, count), inv_dx)
        tout.copy_(torch.as_tensor(out))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(StatsEngine())
    StatsEngine.seen = []
    yield
    _lib.set_engine(old)


def _field(shape, m, seed=4):
    return np.random.default_rng(seed).standard_normal((m,) + tuple(shape))


@pytest.mark.parametrize('P,grid', [(1, None), (2, [2, 1, 1]), (4, [2, 2, 1]), (4, [4, 1, 1])])
def test_stats_and_their_rank_reduction(P, grid, engine):
    from mpi4py_fft_amd import PFFT, newDistArray, spectral
    shape = (8, 8, 20)
    G = _field(shape, 3)
    inv = [s / l for s, l in zip(shape, BOX)]
    ref, mag = R.reference(G, inv)

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=grid, wire='torch') if P > 1 else PFFT(comm, shape, dtype='d')
        ops = spectral.SpectralOps(fft, BOX)
        u = newDistArray(fft, False, rank=1)
        u[...] = G[(slice(None),) + fft.local_slice(False)]
        full = ops.stats(u)
        local = ops.stats(u, reduce=False)
        out = torch.zeros(R.nval(3), dtype=torch.float64)
        assert ops.stats(u, out=out, reduce=False) is out
        scalar = ops.stats(u[1])
        rate = ops.cfl_rate(u)
        dt = ops.timestep(u, 0.5, 10.0)
        with pytest.raises(AssertionError, match='precision'):          # a float32 field on a double transform
            ops.stats(u.tensor.to(torch.float32))
        fft.destroy()
        return full, local.numpy().copy(), out.numpy().copy(), scalar, rate, dt
    res = cases.run_ranks(P, body)
    count = int(np.prod(shape))
    for full, local, out, scalar, rate, dt in res:
        assert isinstance(full, np.ndarray) and full.dtype == np.float64 and full.shape == (R.nval(3),)
        assert np.array_equal(full, res[0][0]), 'ranks disagree'          # bit for bit
        R.assert_stats(full, ref, mag, count, 'P = %d' % P)
        assert np.array_equal(local, out)
        assert rate == full[0] and isinstance(rate, float)
        assert isinstance(dt, float) and dt == R.timestep(full[0], 0.5, 10.0) and dt < 10.0
        sref, smag = R.reference(G[1:2], [0.0])
        R.assert_stats(scalar, sref, smag, count, 'scalar field')
        assert scalar[0] == 0.0
    # the local parts combine to the whole
    assert max(r[1][0] for r in res) == ref[0] and min(r[1][3] for r in res) == ref[3]
    assert np.allclose(sum(r[1][4:8] for r in res), ref[4:8], rtol=1e-13, atol=1e-13)
    if P > 1:
        assert any(not np.array_equal(r[1], res[0][0]) for r in res)


def test_an_empty_rank_does_not_disturb_the_extrema(engine):
    """A rank whose block is empty holds the identities (0, 0, then -inf, +inf, 0, 0, 0, 0 per component): combined with
    another rank's values they change nothing, bit for bit -- negative maxima and positive minima included."""
    from mpi4py_fft_amd import PFFT, spectral
    shape = (8, 8, 20)
    G = _field(shape, 3)
    G[0] = -1.0 - np.abs(G[0])                        # max u_0 < 0: an identity of 0 would win
    G[1] = 1.0 + np.abs(G[1])                         # min u_1 > 0
    ref, _ = R.reference(G, [1.0, 2.0, 0.5])
    empty, _ = R.reference(np.zeros((3, 0)), [1.0, 2.0, 0.5])
    assert np.array_equal(empty, [0, 0] + [-np.inf, np.inf, 0, 0, 0, 0] * 3)

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=[2, 1, 1], wire='torch')
        ops = spectral.SpectralOps(fft, BOX)
        got = ops._reduce_stats(torch.as_tensor(ref if comm.Get_rank() == 1 else empty))
        fft.destroy()
        return got
    for got in cases.run_ranks(2, body):
        assert np.array_equal(got, ref) and got[2] < 0 < got[9]


def test_inv_dx_defaults(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape = (8, 6, 20)
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    u = newDistArray(fft, False, rank=1)
    u[...] = _field(shape, 3)
    ops = spectral.SpectralOps(fft, BOX)
    ops.stats(u)
    assert StatsEngine.seen[-1] == (3, [8 / BOX[0], 6 / BOX[1], 20 / BOX[2]])
    ops.stats(u[0])
    assert StatsEngine.seen[-1] == (1, [0.0])
    ops.stats(u.tensor[:2].contiguous())
    assert StatsEngine.seen[-1] == (2, [0.0, 0.0])
    ops.stats(u, inv_dx=[1.0, 0.0, 3.0])
    assert StatsEngine.seen[-1] == (3, [1.0, 0.0, 3.0])
    spectral.SpectralOps(fft).stats(u)                 # L = 2 pi
    assert StatsEngine.seen[-1] == (3, [n / (2 * np.pi) for n in shape])
    fft.destroy()


def test_moments_of_a_sine():
    from mpi4py_fft_amd import spectral
    n = 4096
    x = np.sin(2 * np.pi * np.arange(n) / n)
    st, _ = R.reference(np.stack([x, 2.0 + 3.0 * x]), [0.0, 0.0])
    mo = spectral.moments(st, n)
    assert mo.shape == (2, 4)
    assert np.allclose(mo[0], [0.0, 0.5, 0.0, 1.5], rtol=0, atol=1e-14)
    # shifted and scaled: mean 2, variance 9/2, the same shape factors (cancellation costs a few digits)
    assert np.allclose(mo[1], [2.0, 4.5, 0.0, 1.5], rtol=0, atol=1e-12)


def test_timestep_formula(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    f = spectral.timestep_from_rate
    assert f(4.0, 0.5, 1.0) == 0.125                                   # unclamped
    assert f(4.0, 0.5, 0.0625) == 0.0625                               # dt_max binds
    assert f(400.0, 0.5, 1.0, 0.01) == 0.01                            # dt_min binds
    assert f(3.0, 0.7, 1.0) == 0.7 / 3.0
    for r in (0.0, -1.0, math.inf, math.nan):                          # nothing to limit / not a usable rate: dt_max
        assert f(r, 0.5, 0.25, 0.01) == 0.25
    for r, c, hi, lo in ((4.0, 0.5, 1.0, 0.0), (1e-30, 0.5, 1.0, 0.0), (1e30, 0.5, 1.0, 1e-3), (math.inf, 1.0, 2.0, 1.0)):
        assert f(r, c, hi, lo) == R.timestep(r, c, hi, lo)
    # through the object: the rate is the reduced stats' entry 0
    shape = (8, 6, 20)
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft, BOX)
    u = newDistArray(fft, False, rank=1)
    u[...] = 0
    assert ops.timestep(u, 0.5, 0.25) == 0.25                          # a field at rest
    u[...] = _field(shape, 3)
    rate = R.reference(np.asarray(u), ops.inv_dx)[0][0]
    assert ops.timestep(u, 0.5, 100.0) == 0.5 / rate
    assert ops.timestep(u, 0.5, 100.0, dt_min=50.0) == 50.0
    with pytest.raises(AssertionError):
        ops.timestep(u, 0.0, 1.0)
    with pytest.raises(AssertionError):
        ops.timestep(u, 0.5, 1.0, dt_min=2.0)
    fft.destroy()


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    for name in ('gfft_ps_stats', 'gfft_ps_timestep', 'gfft_ps_rk_stage_dt'):
        assert name in _lib.EXPORTS
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = math.nan, math.inf

    def inv(*v):
        return (ctypes.c_double * len(v))(*v)

    def stats(u=p, ncomp=3, count=8, inv_dx=inv(1.0, 0.0, 2.0), out=p, prec=8):
        return lib.gfft_ps_stats(u, ncomp, count, inv_dx, out, prec, None)
    for bad in (dict(u=None), dict(inv_dx=None), dict(out=None), dict(ncomp=0), dict(ncomp=-1), dict(count=-1),
                dict(inv_dx=inv(1.0, nan, 1.0)), dict(inv_dx=inv(1.0, 1.0, inf)), dict(inv_dx=inv(-1.0, 1.0, 1.0)),
                dict(prec=3), dict(prec=16)):
        assert stats(**bad) == -1, bad
    assert stats(ncomp=5, inv_dx=inv(1.0, 1.0, 1.0, 1.0, 1.0)) == -2     # beyond four components: unsupported, not invalid

    def step(st=p, cfl=0.5, lo=0.0, hi=1.0, dt=p):
        return lib.gfft_ps_timestep(st, cfl, lo, hi, dt, None)
    for bad in (dict(st=None), dict(dt=None), dict(cfl=0.0), dict(cfl=-1.0), dict(cfl=nan), dict(cfl=inf), dict(lo=-1e-3),
                dict(lo=2.0), dict(lo=nan), dict(hi=inf), dict(hi=nan), dict(lo=inf, hi=inf)):
        assert step(**bad) == -1, bad

    def rk(u=p, u0=p, u1=p, du=p, count=8, dt=p, prec=8):
        return lib.gfft_ps_rk_stage_dt(u, u0, u1, du, count, 0.5, 0.25, dt, prec, None)
    for bad in (dict(u0=None), dict(u1=None), dict(du=None), dict(dt=None), dict(count=-1), dict(prec=3)):
        assert rk(**bad) == -1, bad
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device
        assert stats() == -3 and stats(count=0) == -3 and stats(ncomp=4, inv_dx=inv(0.0, 0.0, 0.0, 0.0), prec=4) == -3
        assert step() == -3 and step(lo=1.0, hi=1.0) == -3
        assert rk() == -3 and rk(u=None, u0=None) == -3
