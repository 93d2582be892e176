"""gfft_ps_curl, gfft_ps_cross, gfft_ps_project and gfft_ps_rk_stage on the device against tests/vector_ref.py (numpy, long
double, from the same rounded inputs and the block's own wavenumber vectors), element by element against bounds derived there:
|got - ref| <= 2 eps S for curl, cross and the stage, 8 eps S_j for the projection, per real scalar.  Beside that: the
divergence of the projected field from the device's output alone, the mode k = 0, planted -0.0 / +0.0 / NaN values, ranks
against one rank bit for bit, and a block past one grid sweep against float64 on the device.  No comparison here uses the
norm of a field.

Launch geometry the cases are chosen against (csrc/spectral.hip): one mode (curl, projection) or one point / real scalar
(cross, stage) per lane, 256 lanes per workgroup, at most 16384 workgroups, grid-stride; a lane's mode is its flat index, its
wavenumbers three lookups by i0 = e / (n1 n2), i1, i2.
  * (8, 6, 20): spectral block 8 x 6 x 11 = 528 modes, three workgroups with the last one ragged; 960 points.
  * (5, 3, 7): 5 x 3 x 4 = 60 modes, one partial wave; every axis odd, no Nyquist plane; 105 points.
  * (24, 16, 20), (12, 10, 21): 4224 and 1320 modes, rows of 11, 17 and 6 workgroups; also the blocks the ranks split.
  * (160, 160, 328): 160 x 160 x 165 = 4 224 000 modes > 16384 * 256: a second grid-stride step, which holds all of the plane
    k0 = -1.  This plain projection is what the forced and dealiased sweep tests compare against.
The box is spectrum_ref.BOX: k1 = i1 / 2 is not an integer, and (0, +-1/2, 0) are modes with 0 < |k|^2 < 1.

What the cases are there to catch (each tried on a deliberately wrong build of the kernels): a projection skipped for
|k|^2 < 1 and a k0 looked up one plane short both fail test_curl_and_projection_per_mode, test_planted_values and the sweep; an
fp32 1 / |k|^2 formed from a |k|^2 cut to 12 -- or to 16 -- significant bits fails the sweep alone, because every |k|^2 of this
box below 1024 is exact in 12 bits: the large block is also the only one whose wavenumbers exercise the low bits.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, spectrum_ref as R, vector_ref as V
from tests.test_vector_host import CA, CB, NUS, SHAPES, fields

DEV = 'cuda'
NAN = float('nan')


def _bits(a):
    """The bit patterns of an array (so that -0.0 != 0.0 and a NaN equals itself)"""
    a = np.ascontiguousarray(a)
    r = a.view(a.real.dtype)
    return r.view('u8' if r.dtype == np.float64 else 'u4')


def _dev(a):
    return torch.as_tensor(np.array(a), device=DEV)


def _unwritten(like):
    """a device array of the shape and type of `like` that holds NaN (every part) where nothing has been stored"""
    dtype = torch.from_numpy(np.empty(0, dtype=like.dtype)).dtype
    return torch.full(like.shape, complex(NAN, NAN) if like.dtype.kind == 'c' else NAN, dtype=dtype, device=DEV)


def _ops(comm, shape, dt, **kw):
    from mpi4py_fft_amd import PFFT, spectral
    fft = PFFT(comm, shape, dtype=dt, **kw)
    ops = spectral.SpectralOps(fft, R.BOX)
    return fft, ops


def _own_k(ops, k):
    """The wavenumber vectors the kernels read, on the host; they are the reference's"""
    own = [ki.cpu().numpy() for ki in ops.K]
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(own, k))
    return own


def _same(t, a, what):
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(a)), (what, 'a read-only operand was written')


def _curl(ops, uh):
    U, W = _dev(uh), _unwritten(uh)
    assert ops.curl(U, W) is W
    _same(U, uh, 'curl')
    return W.cpu().numpy()


def _project(ops, du, uh, nu):
    U, D = _dev(uh), _dev(du)
    assert ops.project(D, U, nu) is D
    _same(U, uh, 'project')
    return D.cpu().numpy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_curl_and_projection_per_mode(shape, dt):
    """Every real scalar of the curl within 2 eps S and of the projection (nu = 0.03 and 0) within 8 eps S_j of the long-double
    reference; with nu = 0 the divergence |sum_j k_j got_j| <= 8 eps sum_j |k_j| S_j from the output alone; at k = 0 the
    projection returns du in value and the curl is zero."""
    from mpi4py_fft_amd import comm
    uh, du, k, _, _ = fields(shape, dt)
    eps = cases.EPS[dt]
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    k = _own_k(ops, k)
    assert k[1][1] == 0.5
    got = _curl(ops, uh)
    assert got.dtype == uh.dtype
    V.assert_within(got, V.curl(uh, k), V.curl_size(uh, k), V.C_CURL, eps, 'curl %s %s' % (shape, dt))
    assert np.all(got[:, 0, 0, 0] == 0), 'the curl of the mode k = 0'
    for nu in NUS:
        got = _project(ops, du, uh, nu)
        assert got.dtype == du.dtype
        V.assert_within(got, V.projected(du, uh, k, nu), V.projected_size(du, uh, k, nu), V.C_PROJECT, eps,
                        'project nu=%g %s %s' % (nu, shape, dt))
        assert np.array_equal(got[:, 0, 0, 0], du[:, 0, 0, 0]), ('the mode k = 0 is not du', nu)
        if nu == 0:
            div, bound = np.abs(V.divergence(got, k)), V.LD(V.C_PROJECT * eps) * V.divergence_size(du, k)
            assert np.all(bound.reshape(-1, 2)[1:] > 0) and not bound[0, 0, 0].any()
            worst = float((div.reshape(-1, 2)[1:] / bound.reshape(-1, 2)[1:]).max())
            print('divergence %s %s: worst / bound = %.3f' % (shape, dt, worst))
            assert np.all(div <= bound), (shape, dt, worst)
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_cross_and_stage_per_point(shape, dt):
    """a x b on the physical block and the Runge-Kutta stage on real and on complex fields, each real scalar within 2 eps S;
    with u=None only u1 is written: a sentinel-filled u next to it keeps its bits."""
    from mpi4py_fft_amd import spectral
    uh, du, _, a, b = fields(shape, dt)
    eps = cases.EPS[dt]
    A, B, C = _dev(a), _dev(b), _unwritten(a)
    assert spectral.cross(A, B, C) is C
    _same(A, a, 'cross')
    _same(B, b, 'cross')
    V.assert_within(C.cpu().numpy(), V.cross(a, b), V.cross_size(a, b), V.C_CROSS, eps, 'cross %s %s' % (shape, dt))
    for kind, x0, x1, d in (('complex', uh, du, uh[::-1]), ('real', a, b, a[::-1])):
        x0, x1, d = (np.ascontiguousarray(x) for x in (x0, x1, d))
        (ru, r1), (Su, S1) = V.rk_stage(x0, x1, d, CB, CA), V.rk_size(x0, x1, d, CB, CA)
        U0, U1, D, U = _dev(x0), _dev(x1), _dev(d), _unwritten(x0)
        spectral.rk_stage(U, U0, U1, D, CB, CA)
        _same(U0, x0, 'rk_stage')
        _same(D, d, 'rk_stage')
        V.assert_within(U.cpu().numpy(), ru, Su, V.C_RK, eps, 'rk_stage u %s %s %s' % (kind, shape, dt))
        V.assert_within(U1.cpu().numpy(), r1, S1, V.C_RK, eps, 'rk_stage u1 %s %s %s' % (kind, shape, dt))
        # u=None, with and without u0: u1 as before (the same bits); a sentinel-filled u and the neighbours of u1 keep theirs
        first = U1.cpu().numpy()
        U.fill_(7.25)
        for u0 in (None, U0):
            U1 = torch.full((3,) + tuple(U0.shape), 7.25, dtype=U0.dtype, device=DEV)
            U1[1] = _dev(x1)
            spectral.rk_stage(None, u0, U1[1], D, 0.0, CA)
            assert np.array_equal(_bits(U1[1].cpu().numpy()), _bits(first)), (kind, 'u=None changes u1')
            assert bool((U1[0] == 7.25).all()) and bool((U1[2] == 7.25).all()), (kind, 'a neighbour of u1 was written')
            assert bool((U == 7.25).all()), (kind, 'u was written without being passed')
            _same(U0, x0, 'rk_stage')
            _same(D, d, 'rk_stage')


def _plant(f, c):
    """-0.0, +0.0 and NaN in the real part (a real field: the value) of component c, three different modes or points, in the
    style of test_gpu_gradient._spectral_block; returns the flat place of the NaN"""
    f = np.array(f)
    flat = f.reshape(3, -1)
    if f.dtype.kind == 'c':
        flat[c, 3], flat[c, 7], flat[c, 17] = complex(-0.0, 2.5), complex(0.0, -1.5), complex(np.nan, 0.75)
    else:
        flat[c, 3], flat[c, 7], flat[c, 17] = -0.0, 0.0, np.nan
    return f, 17


def _nan_places(ref):
    """[(component, flat mode, part), ...] of the NaNs of a reference [3] + block (+ [2])"""
    r = ref.reshape(3, -1, 2) if ref.ndim == 5 else ref.reshape(3, -1, 1)
    return [tuple(int(i) for i in w) for w in np.argwhere(np.isnan(r))]


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', [(8, 6, 20), (5, 3, 7)], ids=str)
def test_planted_values(shape, dt):
    """A NaN in the real part of one component of one mode reaches the parts of that mode that it feeds and nothing else: the
    result has a NaN where and only where the reference has one (asserted by vector_ref.assert_within), every other real scalar
    is finite and within its bound, zeros of either sign included."""
    from mpi4py_fft_amd import comm, spectral
    uh, du, k, a, b = fields(shape, dt)
    eps = cases.EPS[dt]
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    k = _own_k(ops, k)
    # projection: the real parts of all three components of the mode
    dp, at = _plant(du, 1)
    for nu in NUS:
        ref = V.projected(dp, uh, k, nu)
        assert _nan_places(ref) == [(0, at, 0), (1, at, 0), (2, at, 0)]
        V.assert_within(_project(ops, dp, uh, nu), ref, V.projected_size(dp, uh, k, nu), V.C_PROJECT, eps,
                        'planted project nu=%g %s %s' % (nu, shape, dt))
    # curl: the imaginary parts of the two other components
    up, at = _plant(uh, 1)
    ref = V.curl(up, k)
    assert _nan_places(ref) == [(0, at, 1), (2, at, 1)]
    V.assert_within(_curl(ops, up), ref, V.curl_size(up, k), V.C_CURL, eps, 'planted curl %s %s' % (shape, dt))
    # cross: the two other components of the point
    ap, at = _plant(a, 1)
    ref = V.cross(ap, b)
    assert _nan_places(ref) == [(0, at, 0), (2, at, 0)]
    C = _unwritten(a)
    spectral.cross(_dev(ap), _dev(b), C)
    V.assert_within(C.cpu().numpy(), ref, V.cross_size(ap, b), V.C_CROSS, eps, 'planted cross %s %s' % (shape, dt))
    # stage: that real scalar of u and of u1
    for kind, x0, x1, d in (('complex', uh, du, dp), ('real', a, b, ap)):
        (ru, r1), (Su, S1) = V.rk_stage(x0, x1, d, CB, CA), V.rk_size(x0, x1, d, CB, CA)
        assert _nan_places(ru) == [(1, 17, 0)] == _nan_places(r1)
        U, U1 = _unwritten(x0), _dev(x1)
        spectral.rk_stage(U, _dev(x0), U1, _dev(d), CB, CA)
        V.assert_within(U.cpu().numpy(), ru, Su, V.C_RK, eps, 'planted rk_stage u %s %s %s' % (kind, shape, dt))
        V.assert_within(U1.cpu().numpy(), r1, S1, V.C_RK, eps, 'planted rk_stage u1 %s %s %s' % (kind, shape, dt))
    fft.destroy()


@pytest.mark.parametrize('shape', [(24, 16, 20), (12, 10, 21)], ids=str)
@pytest.mark.parametrize('P,grid', [(2, [2, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'pencil4'])
def test_thread_ranks(P, grid, shape):
    """Each rank's block of the curl and of the projection is bit for bit its slice of the one-rank result on the same global
    field: the wavenumber vectors are sliced as the field is, and a mode's result depends on nothing but the mode."""
    from mpi4py_fft_amd import comm, newDistArray
    nu = NUS[0]
    for dt in ('d', 'f'):
        uh, du, _, _, _ = fields(shape, dt)
        fft, ops = _ops(comm.COMM_SELF, shape, dt)
        one_curl, one_proj = _curl(ops, uh), _project(ops, du, uh, nu)
        fft.destroy()

        def body(c):
            fft, ops = _ops(c, shape, dt, grid=grid)
            at = (slice(None),) + tuple(fft.local_slice(True))
            U, D, W = (newDistArray(fft, rank=1) for _ in range(3))
            U[...] = np.array(uh[at])
            D[...] = np.array(du[at])
            W.tensor.fill_(complex(NAN, NAN))
            ops.curl(U, W)
            ops.project(D, U, nu)
            out = np.asarray(W).copy(), np.asarray(D).copy(), at
            fft.destroy()
            return out
        res = cases.run_ranks(P, body)
        for w, d, at in res:
            assert w.shape == one_curl[at].shape and w.size > 0
            assert np.array_equal(_bits(w), _bits(one_curl[at])), (P, grid, dt, at, 'curl')
            assert np.array_equal(_bits(d), _bits(one_proj[at])), (P, grid, dt, at, 'project')
        assert len({str(at) for _, _, at in res}) == P


def test_past_one_grid_sweep():
    """fp32, 4 224 000 modes: more than 16384 * 256, so lanes take a second grid-stride step, and the plane k0 = -1 lies wholly
    in it.  Straight through the engine, as the forced and dealiased sweep tests call it; every real scalar of gfft_ps_project
    and gfft_ps_curl against the same formulas evaluated by torch in float64 on the device from the same float32 inputs, with
    the bounds of vector_ref (a float64 evaluation is off by 2^-29 of them)."""
    from mpi4py_fft_amd import _lib
    shape, nu, eps = (160, 160, 328), NUS[0], cases.EPS['f']
    k, _ = R.wavenumbers(shape, True)
    sshape = tuple(len(ki) for ki in k)
    count = int(np.prod(sshape))
    assert sshape == (160, 160, 165) and count > 16384 * 256
    assert (sshape[0] - 1) * sshape[1] * sshape[2] >= 16384 * 256 and k[0][-1] == -1.0
    K = [torch.as_tensor(ki.astype('f'), device=DEV) for ki in k]
    gen = torch.Generator(device=DEV).manual_seed(89)
    U = torch.randn((3,) + sshape + (2,), dtype=torch.float32, device=DEV, generator=gen)
    D0 = torch.randn((3,) + sshape + (2,), dtype=torch.float32, device=DEV, generator=gen)
    keep_u = U.clone()
    eng = _lib.engine()
    got = D0.clone()
    eng.ps_project(got, U, K, sshape, nu, 4)
    W = torch.full_like(U, NAN)
    eng.ps_curl(U, W, K, sshape, 4)
    assert torch.equal(U.view(torch.int32), keep_u.view(torch.int32)), 'u_hat was written'
    del keep_u
    kd = [K[0].double()[:, None, None, None], K[1].double()[None, :, None, None], K[2].double()[None, None, :, None]]
    ka = [x.abs() for x in kd]
    kk = kd[0] * kd[0] + kd[1] * kd[1] + kd[2] * kd[2]
    q = torch.where(kk == 0, torch.ones_like(kk), kk)

    def check(what, got_j, ref_j, S_j, c, j):
        r = (got_j.double() - ref_j).abs() / (c * eps * S_j)
        bad = ~(r <= 1.0)                                                    # (a NaN counts as a failure)
        last = float(r[-1].max())
        print('sweep %s[%d] f: worst / bound = %.3f (plane k0 = -1: %.3f)' % (what, j, float(r.max()), last))
        assert not bool(bad.any()), (what, j, int(bad.sum()), float(r.max()))
    d, u = D0.double(), U.double()
    p = (d[0] * kd[0] + d[1] * kd[1] + d[2] * kd[2]) / q
    pa = (d[0].abs() * ka[0] + d[1].abs() * ka[1] + d[2].abs() * ka[2]) / q
    for j in range(3):
        ref = d[j] - kd[j] * p - (nu * kk) * u[j]
        S = d[j].abs() + ka[j] * pa + (nu * kk) * u[j].abs()
        assert bool((S > 0).all())
        check('project', got[j], ref, S, V.C_PROJECT, j)
    del d, p, pa
    for j, (b, c) in enumerate(((1, 2), (2, 0), (0, 1))):
        w = kd[b] * u[c] - kd[c] * u[b]                                      # (k x u)_j, part by part
        ref = torch.stack([-w[..., 1], w[..., 0]], dim=-1)                    # times i
        S = (ka[b] * u[c].abs() + ka[c] * u[b].abs()).flip(-1)
        ok = S > 0                                                            # (S = 0 where both wavenumbers are 0: the result is 0)
        assert int((~ok).sum()) <= 2 * max(sshape) and bool((W[j][~ok] == 0).all())
        check('curl', torch.where(ok, W[j], torch.zeros_like(W[j])), torch.where(ok, ref, torch.zeros_like(ref)),
              torch.where(ok, S, torch.ones_like(S)), V.C_CURL, j)
