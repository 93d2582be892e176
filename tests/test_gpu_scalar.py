"""gfft_ps_scalar_flux / gfft_ps_scalar_rhs on the device against tests/scalar_ref.py (numpy, float64), against themselves
(masked against unmasked, ranks against one rank) and end to end against the closed form of uniform advection.

Launch geometry the cases are chosen against (csrc/spectral.hip): both kernels are grid-stride, 256 lanes per workgroup, at
most 16384 workgroups.
  * flux: a lane moves V = 16 bytes of reals (2 in fp64, 4 in fp32) where V divides `count` and u, theta and flux all start
    16-byte aligned, else one real.  count = 315 is odd: V = 1, two workgroups, the second ragged (59 lanes).  count = 2520
    = 8 * 315: V = 2 or 4, 1260 or 630 lanes' worth: five or three workgroups, the last ragged, and every component of every
    field still starts 16-byte aligned (2520 * 4 = 630 * 16).  The same 2520 values one element into a larger buffer are
    misaligned: V = 1, ten workgroups -- all three fields misaligned, or one of them alone.  160 x 160 x 328 = 8 396 800 points
    in fp64 are 4 198 400 lanes' worth > 16384 * 256: the last 4096 lanes take a second grid-stride step on the 16-byte path.
  * rhs: a lane's mode is its flat index; the shapes, their blocks and kept counts are those of test_gpu_dealias.  One and
    two scalars are unrolled, three and four loop over the scalars: m = 1 and m = 3 reach both; with and without the mean
    gradient and with and without a mask are the four instantiations of each.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, dealias_ref as D, scalar_ref as C, spectrum_ref as R
from tests.test_gpu_dealias import _bits, _masks, _ops
from tests.test_scalar_host import UNIFORM, uniform_bound, uniform_case

DEV = 'cuda'
SHAPES = [(24, 16, 20), (12, 10, 21)]
KAPPA = {1: [0.03], 3: [0.03, 0.0, 0.2]}
GRAD = {1: [[1.0, -0.5, 0.25]], 3: [[1.0, 0.0, 0.0], [0.3, -0.7, 0.11], [-2.0, 0.5, 0.125]]}
TORCH = {'d': torch.float64, 'f': torch.float32}


def _same_bits(a, b):
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def _inside(n, dtype, gen, lead):
    """A contiguous [lead][n] view one element into a larger buffer: not 16-byte aligned"""
    buf = torch.randn(lead * n + 1, dtype=dtype, device=DEV, generator=gen)
    v = buf[1:].view(lead, n)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize('m', [1, 3, 4])
@pytest.mark.parametrize('dt', ['d', 'f'])
def test_flux_bit_for_bit(dt, m):
    from mpi4py_fft_amd import spectral
    gen = torch.Generator(device=DEV).manual_seed(11)
    dtype = TORCH[dt]
    for count in (315, 2520):
        u = torch.randn((3, count), dtype=dtype, device=DEV, generator=gen)
        th = torch.randn((m, count), dtype=dtype, device=DEV, generator=gen)
        assert u.data_ptr() % 16 == 0 and th.data_ptr() % 16 == 0
        out = torch.full((m, 3, count), float('nan'), dtype=dtype, device=DEV)
        assert spectral.scalar_flux(u, th, out) is out
        assert _same_bits(out, u[None] * th[:, None]), (dt, m, count)
        if m == 1:                                            # the scalar form: theta the shape itself, out [3] + shape
            o1 = torch.full((3, count), float('nan'), dtype=dtype, device=DEV)
            spectral.scalar_flux(u, th[0], o1)
            assert _same_bits(o1, out[0]), (dt, count)
    # misaligned bases fall back to one element per lane: all three fields, then each alone
    count = 2520
    for which in ('all', 'u', 'theta', 'flux'):
        u = _inside(count, dtype, gen, 3) if which in ('all', 'u') else torch.randn((3, count), dtype=dtype, device=DEV, generator=gen)
        th = _inside(count, dtype, gen, m) if which in ('all', 'theta') else torch.randn((m, count), dtype=dtype, device=DEV, generator=gen)
        out = _inside(count, dtype, gen, 3 * m).view(m, 3, count) if which in ('all', 'flux') else torch.empty((m, 3, count), dtype=dtype, device=DEV)
        out.fill_(float('nan'))
        spectral.scalar_flux(u, th, out)
        assert _same_bits(out, u[None] * th[:, None]), (dt, m, which)


def test_flux_past_one_grid_sweep():
    """fp64, m = 1, 8 396 800 points on the 16-byte path: 4 198 400 lanes' worth against 16384 * 256"""
    from mpi4py_fft_amd import spectral
    shape = (160, 160, 328)
    count = int(np.prod(shape))
    assert count % 2 == 0 and count // 2 > 16384 * 256
    gen = torch.Generator(device=DEV).manual_seed(13)
    u = torch.randn((3,) + shape, dtype=torch.float64, device=DEV, generator=gen)
    th = torch.randn(shape, dtype=torch.float64, device=DEV, generator=gen)
    out = torch.full((3,) + shape, float('nan'), dtype=torch.float64, device=DEV)
    spectral.scalar_flux(u, th, out)
    assert _same_bits(out, u * th[None])


_REF = {}


def _fields(shape, dt, m):
    """(F [m][3], theta [m], u [3], k): random spectral blocks in the precision under test; computed once per case and
    shared, never modified"""
    key = (tuple(shape), dt, m)
    if key not in _REF:
        blk = tuple(shape[:2]) + (shape[2] // 2 + 1,)
        rng = np.random.default_rng(47)
        mk = lambda lead: (rng.standard_normal(lead + blk) + 1j * rng.standard_normal(lead + blk)).astype(dt.upper())
        F, th, u = mk((m, 3)), mk((m,)), mk((3,))
        for a in (F, th, u):
            a.setflags(write=False)
        _REF[key] = (F, th, u, R.wavenumbers(shape, True)[0])
    return _REF[key]


def _t(a, sl=None):
    """A host array (or its block `sl` of the three spectral axes) as a contiguous device tensor"""
    a = np.asarray(a)
    if sl is not None:
        a = a[(slice(None),) * (a.ndim - 3) + tuple(sl)]
    return torch.as_tensor(np.array(a, order='C'), device=DEV)           # (a copy: the shared fields are read-only)


def _run(ops, F, th, u, kappa, G=None, dealias=None, sl=None):
    d = torch.full(_t(th, sl).shape, float('nan'), dtype=_t(th, sl).dtype, device=DEV)
    assert ops.scalar_rhs(d, _t(F, sl), _t(th, sl), kappa, G, None if u is None else _t(u, sl), dealias=dealias) is d
    return d.cpu().numpy()


@pytest.mark.parametrize('m', [1, 3])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_rhs_against_reference(shape, dt, m):
    """Per mode |got - ref| <= 16 eps S, S = sum_c |k_c| |F_c| + kappa |k|^2 |theta| + sum_c |G_c| |u_c|, the reference formed in
    float64 from the same rounded inputs.  The 16 is derived: at most 7 products, each with up to 4 roundings before it
    (kk, kappa kk), summed in at most 6 adds, give <= 11 eps S; FMA contraction only lowers that."""
    from mpi4py_fft_amd import comm
    F, th, u, k = _fields(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    eps = cases.EPS[dt]
    for G in (GRAD[m], None):
        got = _run(ops, F, th, u if G else None, KAPPA[m], G)
        ref, S = C.rhs(F, th, k, KAPPA[m], G, u), C.size(F, th, k, KAPPA[m], G, u)
        worst = float((np.abs(got - ref) / np.maximum(16 * eps * S, 1e-300)).max())
        print('%s %s m=%d G=%s: worst |got - ref| / (16 eps S) = %.3f' % (shape, dt, m, G is not None, worst))
        assert got.dtype == th.dtype and np.all(np.abs(got - ref) <= 16 * eps * S), (shape, dt, m, worst)
    # one scalar in the scalar form, a shared kappa and a shared gradient
    one = _run(ops, F[0], th[0], u, KAPPA[m][0], GRAD[m][0])
    assert np.array_equal(_bits(one), _bits(_run(ops, F[:1], th[:1], u, KAPPA[m][:1], GRAD[m][:1])[0]))
    if m == 3:
        shared = _run(ops, F, th, u, 0.03, GRAD[3][1])
        assert np.array_equal(_bits(shared), _bits(_run(ops, F, th, u, [0.03] * 3, [GRAD[3][1]] * 3)))
    fft.destroy()


@pytest.mark.parametrize('m', [1, 3])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_masks_bitwise(shape, dt, m):
    """Every mask of test_gpu_dealias, with and without the mean gradient: kept modes carry the bits of the unmasked call,
    truncated modes +0.0; and with NaN planted in every truncated mode of all inputs the output does not change."""
    from mpi4py_fft_amd import comm
    F, th, u, k = _fields(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    nan = np.nan + 1j * np.nan
    for G in (GRAD[m], None):
        plain = _run(ops, F, th, u if G else None, KAPPA[m], G)
        assert np.all(plain != 0) or G is None                # (without a mean gradient the mode k = 0 is 0)
        for name, (rule, kcut, keep, _) in _masks(shape, k).items():
            mask = ops.dealias_mask(rule, kcut)
            got = _run(ops, F, th, u if G else None, KAPPA[m], G, mask)
            what = (shape, dt, m, G is not None, name)
            assert np.array_equal(_bits(got[:, keep]), _bits(plain[:, keep])), (what, 'a kept mode differs from the call without a mask')
            assert not _bits(got[:, ~keep]).any(), (what, 'a truncated mode is not +0.0')
            Fn, tn, un = np.array(F), np.array(th), np.array(u)
            Fn[:, :, ~keep] = nan
            tn[:, ~keep] = nan
            un[:, ~keep] = nan
            again = _run(ops, Fn, tn, un if G else None, KAPPA[m], G, mask)
            assert np.array_equal(_bits(again), _bits(got)), (what, 'a truncated mode was loaded')
    # (the same data without the mask does carry the NaNs through)
    rule, kcut, keep, _ = _masks(shape, k)['2/3 + kcut']
    Fn = np.array(F)
    Fn[:, :, ~keep] = nan
    assert np.isnan(_run(ops, Fn, th, None, KAPPA[m])[:, ~keep].real).all()
    fft.destroy()


@pytest.mark.parametrize('m', [1, 3])
@pytest.mark.parametrize('dt', ['d', 'f'])
def test_no_mean_gradient_reads_no_u_hat(dt, m):
    from mpi4py_fft_amd import comm
    shape = SHAPES[0]
    F, th, u, k = _fields(shape, dt, m)
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    for dealias in (None, ops.dealias_mask('2/3')):
        want = _run(ops, F, th, None, KAPPA[m], dealias=dealias)
        got = _run(ops, F, th, np.full_like(u, np.nan + 1j * np.nan), KAPPA[m], None, dealias=dealias)
        assert not np.isnan(want.real).any() and np.array_equal(_bits(got), _bits(want)), (dt, m, dealias is not None)
    fft.destroy()


def test_rhs_past_one_grid_sweep():
    """fp32, m = 1, masked, 4 224 000 modes > 16384 * 256, straight through the engine: a strided sample of modes and the last
    1024 (all in the second grid-stride step) against the reference, kept modes to 16 eps S, truncated ones +0.0."""
    from mpi4py_fft_amd import _lib
    shape = (160, 160, 328)
    k, _ = R.wavenumbers(shape, True)
    blk = tuple(len(ki) for ki in k)
    count = int(np.prod(blk))
    assert blk == (160, 160, 165) and count > 16384 * 256
    v = D.keep_vectors(shape)
    K = [torch.as_tensor(ki.astype('f'), device=DEV) for ki in k]
    M = [torch.as_tensor(x.astype(np.uint8), device=DEV) for x in v]
    gen = torch.Generator(device=DEV).manual_seed(53)
    cplx = lambda lead: torch.view_as_complex(torch.randn(lead + blk + (2,), dtype=torch.float32, device=DEV, generator=gen))
    F, th, u = cplx((1, 3)), cplx((1,)), cplx((3,))
    d = torch.full_like(th, float('nan'))
    _lib.engine().ps_scalar_rhs(d, F, th, u, 1, KAPPA[1], GRAD[1], K, M, blk, np.inf, 4)
    idx = np.unique(np.concatenate([np.arange(0, count, 997), np.arange(count - 1024, count)]))
    assert (idx >= 16384 * 256).sum() >= 1024
    i0, i1, i2 = np.unravel_index(idx, blk)
    keep = v[0][i0] & v[1][i1] & v[2][i2]
    assert keep.any() and (~keep).any() and keep[idx >= 16384 * 256].any() and (~keep)[idx >= 16384 * 256].any()
    at = torch.as_tensor(idx, device=DEV)
    pick = lambda t: t.reshape(t.shape[:-3] + (count,))[..., at].cpu().numpy()
    got, Fs, ts, us = pick(d), pick(F), pick(th), pick(u)
    kx, ky, kz = k[0][i0], k[1][i1], k[2][i2]
    ref, S = C.rhs_modes(Fs, ts, kx, ky, kz, KAPPA[1], GRAD[1], us), C.size_modes(Fs, ts, kx, ky, kz, KAPPA[1], GRAD[1], us)
    assert np.all(np.abs(got - ref)[:, keep] <= 16 * cases.EPS['f'] * S[:, keep])
    assert not _bits(got[:, ~keep]).any() and np.all(got[:, keep] != 0)
    # and over the whole block: nothing but +0.0 outside the mask, nothing left unwritten inside
    m = torch.as_tensor(D.keep_mask(k, v), device=DEV)
    assert not bool(torch.view_as_real(d).view(torch.int32)[:, ~m].any()) and not bool(torch.isnan(torch.view_as_real(d)[:, m]).any())


@pytest.mark.parametrize('P,grid', [(2, [2, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'pencil4'])
def test_thread_ranks(P, grid):
    """Each rank's block is bit for bit its slice of the one-rank result: K and the mask vectors are sliced alike."""
    from mpi4py_fft_amd import comm
    shape, dt, m = (24, 16, 20), 'd', 3
    F, th, u, k = _fields(shape, dt, m)
    rule, kcut, keep, _ = _masks(shape, k)['2/3 + kcut']
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    one = _run(ops, F, th, u, KAPPA[m], GRAD[m], ops.dealias_mask(rule, kcut))
    fft.destroy()
    assert not _bits(one[:, ~keep]).any() and np.all(one[:, keep] != 0)

    def body(c):
        fft, ops = _ops(c, shape, dt, grid=grid)
        sl = fft.local_slice(True)
        block = _run(ops, F, th, u, KAPPA[m], GRAD[m], ops.dealias_mask(rule, kcut), sl)
        fft.destroy()
        return block, sl
    res = cases.run_ranks(P, body)
    for block, sl in res:
        assert np.array_equal(_bits(block), _bits(one[(slice(None),) + tuple(sl)])), (P, grid, sl)
    assert len({str(sl) for _, sl in res}) == P


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_uniform_advection_end_to_end(shape, dt):
    """backward, scalar_flux, three forwards, scalar_rhs with the 2/3 mask, rk_stage: n = 5 RK4 steps of uniform advection
    against the closed form R(lambda h)^n theta_0,
        max |theta_hat - R^n theta_0| / max |theta_0| <= n (max |lambda h| rounding_tol(dt, nelem) + 8 eps)
    (test_scalar_host.uniform_bound has the derivation).  The numpy chain in the same precision sits at 9.1e-16 (d) and 1.9e-7
    (f) against bounds of 1.4e-14 and 7.7e-6 at (24, 16, 20)."""
    from mpi4py_fft_amd import comm, newDistArray, spectral
    th0, keep, Rn, zmax = uniform_case(shape, dt.upper())
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
        for rk in range(4):
            work.tensor.copy_(T_hat.tensor)                   # (nothing here relies on backward keeping its input)
            fft.backward(work, Theta)
            spectral.scalar_flux(U, Theta, UT)
            for j in range(3):
                fft.forward(UT[j], UT_hat[j])
            ops.scalar_rhs(dT, UT_hat, T_hat, UNIFORM['kappa'], dealias=mask)
            spectral.rk_stage(T_hat if rk < 3 else None, T0, T1, dT, C.RK_B[rk] * h if rk < 3 else 0.0, C.RK_A[rk] * h)
        T_hat.tensor.copy_(T1.tensor)
    got = np.asarray(T_hat).astype('D')
    want = Rn * th0[0].astype('D')
    err = float(np.abs(got - want).max() / np.abs(th0).max())
    bound = uniform_bound(dt, shape, zmax)
    print('%s %s: device chain against the closed form %.3e (bound %.3e), max |lambda h| = %.3f' % (shape, dt, err, bound, zmax))
    assert not _bits(np.asarray(T_hat)[~keep]).any()
    assert err <= bound, (shape, dt, err, bound)
    fft.destroy()


def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_scalar', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NU = 0.000625
_RUN = {}


def _fused(ex):
    """(energy, stats) of the fused scalar run on one rank: computed once, shared by the two example tests"""
    if 'fused' not in _RUN:
        from mpi4py_fft_amd import comm
        st = {}
        _RUN['fused'] = (ex.solve(comm.COMM_SELF, scalar=(NU, (1, 0, 0)), stats=st), st)
    return _RUN['fused']


def test_example():
    """The Taylor-Green run with a passive scalar against a mean gradient: fused kernels against the array-sized torch
    expressions, against their own replay from a HIP graph and against the recorded variance; the velocity is untouched."""
    from mpi4py_fft_amd import comm
    ex = _example()
    energy, fused = _fused(ex)
    base, graph = {}, {}
    eb = ex.solve(comm.COMM_SELF, scalar=(NU, (1, 0, 0)), stats=base, fused=False)
    eg = ex.solve(comm.COMM_SELF, scalar=(NU, (1, 0, 0)), stats=graph, graph=True)
    v = fused['scalar_variance']
    print('scalar variance %.15f (torch expressions %.15f, graph %.15f), flux %s; energy %.15f'
          % (v, base['scalar_variance'], graph['scalar_variance'], fused['scalar_flux'], energy))
    assert abs(v - base['scalar_variance']) <= 1e-10 * v, (fused, base)
    assert abs(v - graph['scalar_variance']) <= 1e-12 * v, (fused, graph)
    assert abs(v - ex.SCALAR_VARIANCE) <= 1e-9 * ex.SCALAR_VARIANCE, (v, ex.SCALAR_VARIANCE)
    for e in (energy, eb, eg):
        assert round(e - 0.124953117517, 7) == 0, e
    assert len(fused['scalar_flux']) == 3 and fused['scalar_flux'][0] < 0            # down the gradient
    assert max(abs(a - b) for a, b in zip(fused['scalar_flux'], base['scalar_flux'])) <= 1e-10 * abs(fused['scalar_flux'][0])


def test_example_on_two_thread_ranks():
    ex = _example()
    energy, fused = _fused(ex)

    def body(c):
        st = {}
        return ex.solve(c, scalar=(NU, (1, 0, 0)), stats=st), st
    for e, st in cases.run_ranks(2, body):
        assert abs(st['scalar_variance'] - fused['scalar_variance']) <= 1e-10 * fused['scalar_variance'], (st, fused)
        assert round(e - 0.124953117517, 7) == 0, e
