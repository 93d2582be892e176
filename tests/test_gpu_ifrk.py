"""gfft_ps_rk_stage_if on the device against tests/ifrk_ref.py (numpy, float64), against gfft_ps_rk_stage (nu = 0: the same
bits), against itself (device step against host step, ranks against one rank) and end to end against the closed form of
uniform advection with exact diffusion.

Launch geometry the cases are chosen against (csrc/spectral.hip): grid-stride, 256 lanes per workgroup, a lane's mode is its
flat index and it takes the components in turn.  (24, 16, 20) and (12, 10, 21) have spectral blocks 24 x 16 x 11 = 4224 and
12 x 10 x 11 = 1320 modes: rows of 11, shorter than a wave, 17 and 6 workgroups, the last one ragged.  One component and three
with one nu are the instantiation with one exp per mode; four with mixed nu (one of them 0) the one with an exp per component.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, ifrk_ref as I, scalar_ref as C, spectrum_ref as R
from tests.test_gpu_dealias import _bits, _ops
from tests.test_ifrk_host import ifrk_uniform_case, stiff_kappa
from tests.test_scalar_host import UNIFORM, uniform_bound

DEV = 'cuda'
SHAPES = [(24, 16, 20), (12, 10, 21)]
H = 0.05
NCOMP = [1, 3, 4]
NAN = complex(float('nan'), float('nan'))


def _kkmax(shape):
    return float(I.kk_of(R.wavenumbers(shape, True)[0]).max())


def _nus(shape, m, xmax=20.0):
    """nu per component with max nu |k|^2 H / 2 = xmax: one value for m = 1 and 3, mixed (one of them 0) for m = 4"""
    nu = 2 * xmax / (_kkmax(shape) * H)
    return [nu] * m if m < 4 else [nu, 0.0, nu / 3, nu / 10]


_REF = {}


def _fields(shape, dt, m):
    """(u0, u1, du, k): random [m] + spectral block in the precision under test; computed once per case, shared, read-only"""
    key = (tuple(shape), dt, m)
    if key not in _REF:
        blk = (m,) + tuple(shape[:2]) + (shape[2] // 2 + 1,)
        rng = np.random.default_rng(59)
        mk = lambda: (rng.standard_normal(blk) + 1j * rng.standard_normal(blk)).astype(dt.upper())
        u0, u1, du = mk(), mk(), mk()
        for a in (u0, u1, du):
            a.setflags(write=False)
        _REF[key] = (u0, u1, du, R.wavenumbers(shape, True)[0])
    return _REF[key]


def _t(a, sl=None):
    """A host array (or its block `sl` of the three spectral axes) as a contiguous device tensor (a copy)"""
    a = np.asarray(a)
    if sl is not None:
        a = a[(slice(None),) * (a.ndim - 3) + tuple(sl)]
    return torch.as_tensor(np.array(a, order='C'), device=DEV)


def _stage(ops, u0, u1, du, nu, row, with_u=True, sl=None, **step):
    """(u or None, u1) of one device stage on copies of the host fields; u starts NaN-filled"""
    t0, t1, td = _t(u0, sl), _t(u1, sl), _t(du, sl)
    tu = torch.full_like(t1, NAN) if with_u else None
    assert ops.rk_stage_if(tu, t0 if with_u else None, t1, td, nu, row[0], row[1], row[2:], **(step or dict(h=H))) is t1
    assert torch.equal(t0, _t(u0, sl)) and torch.equal(td, _t(du, sl)), 'a stage modified u0 or du'
    return (None if tu is None else tu.cpu().numpy()), t1.cpu().numpy()


@pytest.mark.parametrize('m', NCOMP)
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_stage_against_reference(shape, dt, m):
    """Each of the four stage forms of IFRK4: per mode |got - ref| <= (8 x + 12) eps (|u0| + |u1| + |cb h du|), x = lambda h / 2
    up to 20 (ifrk_ref.bound has the derivation), the reference formed in float64 from the same rounded fields."""
    from mpi4py_fft_amd import comm, spectral
    u0, u1, du, k = _fields(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    nus = _nus(shape, m)
    lam = I.lam_of(nus, k)
    assert 19.9 <= float(lam.max()) * H / 2 <= 20.1
    eps = cases.EPS[dt]
    for rk, row in enumerate(spectral.IFRK4):
        with_u = rk < 3
        got_u, got_1 = _stage(ops, u0, u1, du, nus if m > 1 else nus[0], row, with_u)
        ref_u, ref_1 = I.stage(u0, u1, du, lam, H, *row, with_u=with_u)
        bound = I.bound(lam, H, u0, u1, du, row[0] if with_u else None, eps)
        worst = [float((np.abs(got_1 - ref_1) / bound).max())]
        if with_u:
            worst.append(float((np.abs(got_u - ref_u) / bound).max()))
            assert got_u.dtype == u0.dtype and not np.isnan(got_u.real).any()
        print('%s %s m=%d stage %d: worst |got - ref| / ((8 x + 12) eps S) = %s, x up to %.1f'
              % (shape, dt, m, rk + 1, ' / '.join('%.3f' % w for w in worst), float(lam.max()) * H / 2))
        assert got_1.dtype == u1.dtype and max(worst) <= 1.0, (shape, dt, m, rk, worst)
    if m == 1:                                            # the scalar form: the spectral shape itself
        row = spectral.IFRK4[0]
        a = _stage(ops, u0[0], u1[0], du[0], nus[0], row)
        b = _stage(ops, u0, u1, du, nus, row)
        assert np.array_equal(_bits(a[0]), _bits(b[0][0])) and np.array_equal(_bits(a[1]), _bits(b[1][0]))
    fft.destroy()


@pytest.mark.parametrize('with_u', [True, False], ids=['u', 'no-u'])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_nu_zero_is_rk_stage_bit_for_bit(shape, dt, with_u):
    """nu = 0: every power of E is exactly 1 and the result carries the bits of spectral.rk_stage with the host products cb h
    and ca h -- for every row of the table (powers 0, 1 and 2), for one, three and four components, and for the component
    whose nu is 0 among others that decay."""
    from mpi4py_fft_amd import asdevice, comm, spectral
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    h = 0.012345678901234567
    for m in NCOMP:
        u0, u1, du, k = _fields(shape, dt, m)
        for row in spectral.IFRK4:
            t0, t1, td = asdevice(np.array(u0)), asdevice(np.array(u1)), asdevice(np.array(du))
            tu = asdevice(np.full_like(u1, np.nan)) if with_u else None
            spectral.rk_stage(tu, t0 if with_u else None, t1, td, row[0] * h, row[1] * h)
            got_u, got_1 = _stage(ops, u0, u1, du, [0.0] * m if m > 1 else 0.0, row, with_u, h=h)
            assert np.array_equal(_bits(got_1), _bits(np.asarray(t1))), (shape, dt, m, row)
            assert not np.array_equal(got_1, u1)
            if with_u:
                assert np.array_equal(_bits(got_u), _bits(np.asarray(tu))), (shape, dt, m, row)
            if m == 4:
                mixed_u, mixed_1 = _stage(ops, u0, u1, du, _nus(shape, 4), row, with_u, h=h)
                assert np.array_equal(_bits(mixed_1[1]), _bits(got_1[1])), (shape, dt, row)
                assert not with_u or np.array_equal(_bits(mixed_u[1]), _bits(got_u[1])), (shape, dt, row)
                assert row[4:] == (0, 0) or not np.array_equal(mixed_1[0], got_1[0])
    fft.destroy()


@pytest.mark.parametrize('m', [3, 4])
@pytest.mark.parametrize('dt', ['d', 'f'])
def test_device_step_is_the_host_step_and_follows_a_replay(dt, m):
    """dt= (a device tensor) gives the bits of h= for the same double; captured under torch.cuda.graph, a replay uses whatever
    dt[0] holds then."""
    from mpi4py_fft_amd import comm, spectral
    shape = SHAPES[0]
    u0, u1, du, k = _fields(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    nus = _nus(shape, m)
    h = 0.012345678901234567
    hdev = torch.tensor([h, 123.0], dtype=torch.float64, device=DEV)
    for rk, row in enumerate(spectral.IFRK4):
        a = _stage(ops, u0, u1, du, nus, row, rk < 3, h=h)
        b = _stage(ops, u0, u1, du, nus, row, rk < 3, dt=hdev)
        assert np.array_equal(_bits(a[1]), _bits(b[1])) and (rk == 3 or np.array_equal(_bits(a[0]), _bits(b[0]))), (dt, m, rk)
    assert hdev.cpu().tolist() == [h, 123.0]                    # read only
    row = spectral.IFRK4[0]
    t0, t1, td = _t(u0), _t(u1), _t(du)
    tu = torch.empty_like(t1)

    def stage():
        ops.rk_stage_if(tu, t0, t1, td, nus, row[0], row[1], row[2:], dt=hdev)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        stage()                                          # warm-up on another stream, as test_gpu_stats does before a capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        stage()
    for step in (h, 2.5 * h):
        hdev[0] = step
        t1.copy_(_t(u1))
        tu.fill_(NAN)
        g.replay()
        torch.cuda.synchronize()
        want = _stage(ops, u0, u1, du, nus, row, h=step)
        assert np.array_equal(_bits(tu.cpu().numpy()), _bits(want[0])) and np.array_equal(_bits(t1.cpu().numpy()), _bits(want[1])), (dt, m, step)
    fft.destroy()


@pytest.mark.parametrize('m', NCOMP)
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_pure_decay(shape, dt, m):
    """du = 0: the four stages give exp(-nu |K|^2 h) u_n within the bound of one stage, (8 x + 12) eps (|u0| + |u1|) with
    u0 = u1 = u_n, up to lambda h = 50, a step at which explicit RK4 amplifies by |R(-50)| = 2.4e5.  Zero modes stay zero."""
    from mpi4py_fft_amd import comm, spectral
    un, _, _, k = _fields(shape, dt, m)
    un = np.array(un)
    zero = np.zeros(un.shape[1:], dtype=bool)
    zero[::3, 1::2, ::2] = True
    un[:, zero] = 0
    un[0][zero] = -0.0                                   # (a negative zero among them)
    nus = _nus(shape, m, xmax=25.0)
    lam = I.lam_of(nus, k)
    assert 49.9 <= float(lam.max()) * H <= 50.1 and abs(I.rk4_factor(-float(lam.max()) * H)) > 1e5
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    t0, t1, td = _t(un), _t(un), torch.zeros_like(_t(un))
    tu = torch.full_like(t1, NAN)
    for rk, row in enumerate(spectral.IFRK4):
        ops.rk_stage_if(tu if rk < 3 else None, t0, t1, td, nus, row[0], row[1], row[2:], h=H)
    got = t1.cpu().numpy()
    want = np.exp(-lam * H) * un.astype('D')
    bound = I.bound(lam, H, un, un, 0 * un, 0.0, cases.EPS[dt])
    ok = ~zero
    worst = float((np.abs(got - want)[:, ok] / bound[:, ok]).max())
    print('%s %s m=%d: pure decay up to lambda h = %.1f, worst |got - exact| / bound = %.3f' % (shape, dt, m, float(lam.max()) * H, worst))
    assert worst <= 1.0, (shape, dt, m, worst)
    assert np.all(got[:, zero] == 0) and np.all(tu.cpu().numpy()[:, zero] == 0)
    assert float(np.abs(got).max()) <= float(np.abs(un).max()) and np.all(got[:, ok] != 0)
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_untouched_inputs(dt):
    """u = None: u0 is not read -- a NaN-filled u0 leaves no NaN in u1 and stays NaN --; u0 and du keep their bits in every
    stage (checked in _stage for every call of this file); u is written everywhere."""
    from mpi4py_fft_amd import comm, spectral
    shape, m = SHAPES[1], 4
    u0, u1, du, k = _fields(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    nus = _nus(shape, m)
    for row in spectral.IFRK4:
        t0, t1, td = torch.full_like(_t(u0), NAN), _t(u1), _t(du)
        ops.rk_stage_if(None, t0, t1, td, nus, row[0], row[1], row[2:], h=H)
        want = _stage(ops, u0, u1, du, nus, row, with_u=False)[1]
        assert np.array_equal(_bits(t1.cpu().numpy()), _bits(want)) and not np.isnan(want.real).any(), (dt, row)
        assert bool(torch.isnan(torch.view_as_real(t0)).all()) and torch.equal(td, _t(du)), (dt, row)
        got_u = _stage(ops, u0, u1, du, nus, row, with_u=True)[0]
        assert not np.isnan(got_u.real).any() and not np.isnan(got_u.imag).any(), (dt, row)
    fft.destroy()


def test_thread_ranks():
    """Each rank's block of a two-rank grid is bit for bit its slice of the one-rank result: K is sliced with the block."""
    from mpi4py_fft_amd import comm, spectral
    shape, dt, m = (24, 16, 20), 'd', 4
    u0, u1, du, k = _fields(shape, dt, m)
    nus = _nus(shape, m)
    row = spectral.IFRK4[0]
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    one = _stage(ops, u0, u1, du, nus, row)
    fft.destroy()

    def body(c):
        fft, ops = _ops(c, shape, dt, grid=[2, 1, 1])
        sl = fft.local_slice(True)
        block = _stage(ops, u0, u1, du, nus, row, sl=sl)
        fft.destroy()
        return block, sl
    res = cases.run_ranks(2, body)
    for (bu, b1), sl in res:
        at = (slice(None),) + tuple(sl)
        assert np.array_equal(_bits(bu), _bits(one[0][at])) and np.array_equal(_bits(b1), _bits(one[1][at])), sl
    assert len({str(sl) for _, sl in res}) == 2


def _uniform_chain(shape, dt, kappa):
    """n IFRK4 steps of uniform advection on the device: backward, scalar_flux, three forwards, scalar_rhs with kappa = 0 and
    the 2/3 mask, rk_stage_if with kappa"""
    from mpi4py_fft_amd import comm, newDistArray, spectral
    th0, keep, Rn, zmax, lmax = ifrk_uniform_case(shape, kappa, dt.upper())
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    mask = ops.dealias_mask('2/3')
    U, UT = newDistArray(fft, False, rank=1), newDistArray(fft, False, rank=1)
    U_hat, UT_hat = newDistArray(fft, rank=1), newDistArray(fft, rank=1)
    Theta = newDistArray(fft, False)
    T_hat, T0, T1, dT, work = (newDistArray(fft) for _ in range(5))
    U_hat[...] = C.uniform(UNIFORM['c'], shape, dt.upper())
    for j in range(3):
        fft.backward(U_hat[j], U[j])
    T_hat[...] = th0[0]
    h = UNIFORM['h']
    for _ in range(UNIFORM['n']):
        T0.tensor.copy_(T_hat.tensor)
        T1.tensor.copy_(T_hat.tensor)
        for rk, row in enumerate(spectral.IFRK4):
            work.tensor.copy_(T_hat.tensor)                   # (nothing here relies on backward keeping its input)
            fft.backward(work, Theta)
            spectral.scalar_flux(U, Theta, UT)
            for j in range(3):
                fft.forward(UT[j], UT_hat[j])
            ops.scalar_rhs(dT, UT_hat, T_hat, 0.0, dealias=mask)
            ops.rk_stage_if(T_hat if rk < 3 else None, T0, T1, dT, kappa, row[0], row[1], row[2:], h=h)
        T_hat.tensor.copy_(T1.tensor)
    got = np.asarray(T_hat).copy()
    fft.destroy()
    err = float(np.abs(got.astype('D') - Rn * th0[0].astype('D')).max() / np.abs(th0).max())
    return got, keep, err, zmax, lmax


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_uniform_advection_end_to_end(shape, dt):
    """n = 5 IFRK4 steps against the closed form (R(-i k.U h) exp(-kappa |k|^2 h))^n theta_0 -- the diffusion exact, RK4 on
    the advection -- within test_scalar_host.uniform_bound with zmax the advective |k.U| h alone.  The numpy chain sits at
    8.8e-16 against 1.4e-14 at (24, 16, 20) (test_ifrk_host)."""
    got, keep, err, zmax, lmax = _uniform_chain(shape, dt, UNIFORM['kappa'])
    bound = uniform_bound(dt, shape, zmax)
    print('%s %s: device IFRK4 chain against the closed form %.3e (bound %.3e), max |k.U| h = %.3f, max kappa |k|^2 h = %.3f'
          % (shape, dt, err, bound, zmax, lmax))
    assert not _bits(got[~keep]).any()
    assert err <= bound, (shape, dt, err, bound)


def test_uniform_advection_with_stiff_diffusion():
    """The same chain with kappa raised until kappa k_max^2 h = 3.5 > 2.785: explicit RK4 amplifies the stiffest kept mode,
    the integrating factor stays within the same bound."""
    shape, dt = SHAPES[0], 'd'
    kappa = stiff_kappa(shape)
    got, keep, err, zmax, lmax = _uniform_chain(shape, dt, kappa)
    bound = uniform_bound(dt, shape, zmax)
    print('%s %s kappa = %.4g: device IFRK4 chain against the closed form %.3e (bound %.3e), max kappa |k|^2 h = %.3f'
          % (shape, dt, kappa, err, bound, lmax))
    assert lmax > 3 and not _bits(got[~keep]).any()
    assert err <= bound, (err, bound)


def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_ifrk', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NU = 0.000625


def test_example():
    """The Taylor-Green run at 64^3 with integrator='ifrk4': nu k^2 h is 2e-5 at the vortex's wavenumber, so the energy is the
    explicit path's to seven places; it equals the recorded IF_ENERGY, replays from a HIP graph, and carries a scalar to the
    explicit path's variance."""
    from mpi4py_fft_amd import comm
    ex = _example()
    e = ex.solve(comm.COMM_SELF, integrator='ifrk4')
    eg = ex.solve(comm.COMM_SELF, integrator='ifrk4', graph=True)
    st = {}
    es = ex.solve(comm.COMM_SELF, integrator='ifrk4', scalar=(NU, (1, 0, 0)), stats=st)
    print('ifrk4 energy %.15f (graph %.15f, with a scalar %.15f), IF_ENERGY %r; scalar variance %.15f against %.15f: relative %.3e'
          % (e, eg, es, ex.IF_ENERGY, st['scalar_variance'], ex.SCALAR_VARIANCE, abs(st['scalar_variance'] - ex.SCALAR_VARIANCE) / ex.SCALAR_VARIANCE))
    assert round(e - 0.124953117517, 7) == 0, e
    assert abs(e - ex.IF_ENERGY) <= 1e-9, (e, ex.IF_ENERGY)
    assert abs(eg - e) <= 1e-12, (eg, e)
    assert round(es - 0.124953117517, 7) == 0, es            # the scalar is passive
    assert abs(st['scalar_variance'] - ex.SCALAR_VARIANCE) <= 1e-6 * ex.SCALAR_VARIANCE, (st, ex.SCALAR_VARIANCE)
