"""Host side of the four base kernels (no GPU): the reference tests/vector_ref.py against independent statements of the same
mathematics; its bounds against an emulation of each kernel's operation order in the precision under test; the wrappers
`SpectralOps.curl`, `SpectralOps.project`, `spectral.cross` and `spectral.rk_stage` over a recording stand-in engine; and the
argument checks of gfft_ps_curl, gfft_ps_cross, gfft_ps_project and gfft_ps_rk_stage."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases, forcing_ref as F, spectrum_ref as R, vector_ref as V
from tests.test_forcing_host import ForcingEngine, _h

SHAPES = [(8, 6, 20), (5, 3, 7), (24, 16, 20), (12, 10, 21)]
NUS = (0.03, 0.0)
CB, CA = 0.25, 1.0 / 6.0            # CA is not representable in fp32: the conversion of the coefficient rounds

_REF = {}


def fields(shape, dt):
    """(u_hat, du_hat, k, a, b): random complex [3] + spectral block and real [3] + physical block in the precision under test,
    and the block's wavenumber vectors IN THAT PRECISION; computed once per case and shared, never modified"""
    key = (tuple(shape), dt)
    if key not in _REF:
        blk = (3,) + tuple(shape[:2]) + (shape[2] // 2 + 1,)
        rng = np.random.default_rng(83)
        cplx = lambda: (rng.standard_normal(blk) + 1j * rng.standard_normal(blk)).astype(dt.upper())
        uh, du = cplx(), cplx()
        a, b = (rng.standard_normal((3,) + tuple(shape)).astype(dt) for _ in range(2))
        k = [ki.astype(dt) for ki in R.wavenumbers(shape, True)[0]]
        for x in [uh, du, a, b] + k:
            x.setflags(write=False)
        _REF[key] = (uh, du, k, a, b)
    return _REF[key]


def _mesh(k):
    return np.array(np.broadcast_arrays(k[0][:, None, None], k[1][None, :, None], k[2][None, None, :]))


# ---- the reference against independent statements ---------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_reference_against_independent_statements(shape):
    uh, du, k, a, b = fields(shape, 'd')
    e = 2.0 ** -52
    K = _mesh(k)
    # curl = i K x u on the full meshes; cross = np.cross: float64 evaluations, a few roundings of theirs each
    want = 1j * np.cross(K, uh, axis=0)
    S = V.curl_size(uh, k)
    assert np.all(np.abs(V.join(V.curl(uh, k)) - want) <= 4 * e * (S[..., 0] + S[..., 1]))
    assert np.all(np.abs(V.cross(a, b) - np.cross(a, b, axis=0)) <= 4 * e * V.cross_size(a, b))
    assert np.all(V.cross_size(a, b) > 0) and np.all(S[:, 1:, 1:, 1:] > 0) and not S[:, 0, 0, 0].any()          # k = 0: no curl
    for nu in NUS:
        S = V.projected_size(du, uh, k, nu)
        got = V.join(V.projected(du, uh, k, nu))
        assert np.all(np.abs(got - F.projected(du, uh, k, nu)) <= 16 * e * (S[..., 0] + S[..., 1])), nu
    # a projection: applied twice it is itself, and its result is orthogonal to k -- both to the LONG-DOUBLE rounding
    el = float(np.finfo(V.LD).eps)
    zero = np.zeros_like(uh)
    once = V.projected(du, zero, k, 0.0)
    twice = V.projected(V.join(once), zero, k, 0.0)
    S = V.projected_size(du, zero, k, 0.0)
    assert np.all(np.abs(twice - once) <= 32 * el * S)
    assert np.all(np.abs(V.divergence(V.join(once), k)) <= 32 * el * V.divergence_size(du, k))
    assert np.array_equal(once[:, 0, 0, 0], V.parts(du)[:, 0, 0, 0])             # k = 0: du itself
    assert not np.array_equal(once, V.parts(du))
    # the Runge-Kutta stage, complex and real
    for x0, x1, d in ((uh, du, uh[::-1]), (a, b, a[::-1])):
        u, u1 = V.rk_stage(x0, x1, d, CB, CA)
        Su, S1 = V.rk_size(x0, x1, d, CB, CA)
        wide = V.join if x0.dtype.kind == 'c' else (lambda p: p)
        tot = (lambda s: s[..., 0] + s[..., 1]) if x0.dtype.kind == 'c' else (lambda s: s)
        assert np.all(np.abs(wide(u) - (x0 + CB * d)) <= 4 * e * tot(Su))
        assert np.all(np.abs(wide(u1) - (x1 + CA * d)) <= 4 * e * tot(S1))
        none, again = V.rk_stage(None, x1, d, CB, CA)
        assert none is None and np.array_equal(again, u1) and V.rk_size(None, x1, d, CB, CA)[0] is None


# ---- the bounds against the kernels' operation order -----------------------------------------------------------------------
def emulate_curl(uh, k):
    """ps_curl_kernel in the arrays' own precision, one rounding per operation (no contraction)"""
    kx, ky, kz = k[0][:, None, None], k[1][None, :, None], k[2][None, None, :]
    out = np.empty_like(uh)
    for j, (p, q, kp, kq) in enumerate(((2, 1, ky, kz), (0, 2, kz, kx), (1, 0, kx, ky))):
        wx = kp * uh[p].real - kq * uh[q].real
        wy = kp * uh[p].imag - kq * uh[q].imag
        out[j].real, out[j].imag = -wy, wx
    return out


def emulate_cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def emulate_project(du, uh, k, nu):
    """ps_project_kernel's operation order: kk, inv, p from d_i (k_i inv), d -= p k, d -= ((real)nu kk) u"""
    real = du.real.dtype.type
    K = [k[0][:, None, None], k[1][None, :, None], k[2][None, None, :]]
    kk = K[0] * K[0] + K[1] * K[1] + K[2] * K[2]
    inv = real(1) / np.where(kk == 0, real(1), kk)
    v = real(nu) * kk
    out = np.empty_like(du)
    for part in ('real', 'imag'):
        d = [getattr(du[j], part) for j in range(3)]
        p = d[0] * (K[0] * inv) + d[1] * (K[1] * inv) + d[2] * (K[2] * inv)
        for j in range(3):
            setattr(out[j], part, (d[j] - p * K[j]) - v * getattr(uh[j], part))
    return out


def emulate_rk(u0, u1, du, cb, ca):
    real = du.real.dtype.type
    return u0 + real(cb) * du, u1 + real(ca) * du


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_emulated_kernels_stay_within_the_bounds(dt):
    """The derived bounds hold for an unfused evaluation in the kernels' order; the worst ratios are printed (the projection
    reaches 1.6 ... 1.9 of its 8 eps S, the divergence 0.11 of its bound: the bounds are not fitted to them)."""
    eps = cases.EPS[dt]
    worst = {}

    def note(name, got, ref, S, c):
        assert got.real.dtype == np.dtype(dt)
        r = V.ratio(got, ref, S, c, eps)
        worst[name] = max(worst.get(name, 0.0), float(r.max()))
    for shape in SHAPES:
        uh, du, k, a, b = fields(shape, dt)
        note('curl', emulate_curl(uh, k), V.curl(uh, k), V.curl_size(uh, k), V.C_CURL)
        note('cross', emulate_cross(a, b), V.cross(a, b), V.cross_size(a, b), V.C_CROSS)
        for nu in NUS:
            got = emulate_project(du, uh, k, nu)
            note('project', got, V.projected(du, uh, k, nu), V.projected_size(du, uh, k, nu), V.C_PROJECT)
            assert np.array_equal(got[:, 0, 0, 0], du[:, 0, 0, 0])
            if nu == 0:
                r = np.abs(V.divergence(got, k)) / np.maximum(V.LD(V.C_PROJECT * eps) * V.divergence_size(du, k), V.LD(1e-300))
                worst['divergence'] = max(worst.get('divergence', 0.0), float(r.max()))
        for x0, x1, d in ((uh, du, uh[::-1]), (a, b, a[::-1])):
            gu, g1 = emulate_rk(x0, x1, d, CB, CA)
            (ru, r1), (Su, S1) = V.rk_stage(x0, x1, d, CB, CA), V.rk_size(x0, x1, d, CB, CA)
            note('rk_stage u', gu, ru, Su, V.C_RK)
            note('rk_stage u1', g1, r1, S1, V.C_RK)
    for name, w in worst.items():
        print('%s emulated %s: worst / bound = %.3f' % (dt, name, w))
    assert max(worst.values()) <= 1.0 and min(worst.values()) > 0.05, worst
    # the derivations, in units of eps S: 1 for curl and cross, 1.5 for the stage, 5.5 for the projection
    assert worst['curl'] <= 1.0 / V.C_CURL and worst['cross'] <= 1.0 / V.C_CROSS, worst
    assert max(worst['rk_stage u'], worst['rk_stage u1']) <= 1.5 / V.C_RK and worst['project'] <= 5.5 / V.C_PROJECT, worst


def test_a_lost_digit_is_seen():
    """What the bound is for: an fp32 projection whose 1 / |k|^2 keeps 12 bits misses it by orders of magnitude where |k|^2 has
    more bits than that, and a curl that reads a neighbouring wavenumber misses it everywhere on that plane."""
    shape, dt = (24, 16, 20), 'f'
    uh, du, k, _, _ = fields(shape, dt)
    big = [np.float32(64.0) * ki + np.float32(0.5) for ki in k]             # |k|^2 needs more than 12 bits
    ref, S = V.projected(du, uh, big, 0.0), V.projected_size(du, uh, big, 0.0)
    assert float(V.ratio(emulate_project(du, uh, big, 0.0), ref, S, V.C_PROJECT, cases.EPS[dt]).max()) <= 1.0
    K = [big[0][:, None, None], big[1][None, :, None], big[2][None, None, :]]
    kk = K[0] * K[0] + K[1] * K[1] + K[2] * K[2]
    inv = np.float32(1) / (kk.view('u4') & np.uint32(0xFFFFF000)).view('f')
    bad = np.empty_like(du)
    for part in ('real', 'imag'):
        d = [getattr(du[j], part) for j in range(3)]
        p = d[0] * (K[0] * inv) + d[1] * (K[1] * inv) + d[2] * (K[2] * inv)
        for j in range(3):
            setattr(bad[j], part, d[j] - p * K[j])
    assert float(V.ratio(bad, ref, S, V.C_PROJECT, cases.EPS[dt]).max()) > 50.0
    k0 = k[0].copy()
    k0[-1] = k0[-2]
    r = V.ratio(emulate_curl(uh, [k0, k[1], k[2]]), V.curl(uh, k), V.curl_size(uh, k), V.C_CURL, cases.EPS[dt])
    assert float(r[:, :-1].max()) <= 1.0 and float(r[1:, -1].min()) > 1e3


# ---- the wrappers over a recording engine ----------------------------------------------------------------------------------
class VectorEngine(ForcingEngine):
    """ForcingEngine (which has the projection) plus the curl, the cross product and the stage restated with numpy on host
    tensors; every call is recorded with its count or shape and its precision"""

    @staticmethod
    def _put(t, a):
        t.copy_(torch.as_tensor(np.ascontiguousarray(a).astype(_h(t).dtype)).reshape(t.shape))

    def ps_curl(self, tu, tout, k, shape, precision):
        ForcingEngine.log.append(('ps_curl', tuple(shape), precision))
        self._put(tout, V.join(V.curl(_h(tu), [_h(ki) for ki in k])))

    def ps_project(self, tdu, tu, k, shape, nu, precision):
        super().ps_project(tdu, tu, k, shape, nu, precision)
        ForcingEngine.log[-1] += (tuple(shape), precision)

    def ps_cross(self, ta, tb, tout, count, precision):
        ForcingEngine.log.append(('ps_cross', int(count), precision))
        self._put(tout, V.cross(_h(ta), _h(tb)))

    def ps_rk_stage(self, tu, tu0, tu1, tdu, count, cb, ca, precision):
        ForcingEngine.log.append(('ps_rk_stage', int(count), float(cb), float(ca), precision, tu is not None, tu0 is not None))
        u, u1 = V.rk_stage(None if tu is None else _h(tu0), _h(tu1), _h(tdu), cb, ca)
        wide = V.join if _h(tdu).dtype.kind == 'c' else (lambda p: p)
        if tu is not None:
            self._put(tu, wide(u))
        self._put(tu1, wide(u1))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(VectorEngine())
    ForcingEngine.log = []
    yield
    _lib.set_engine(old)


def _strided(t):
    """the values and shape of t in memory that is not contiguous"""
    wide = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    view = wide[..., ::2]
    view.copy_(t)
    assert view.shape == t.shape and not view.is_contiguous()
    return view


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_wrappers_reach_the_engine_or_refuse(dt, engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape, nu = (8, 6, 20), 0.03
    other = 'f' if dt == 'd' else 'd'
    prec, eps = (8, 2.0 ** -52) if dt == 'd' else (4, 2.0 ** -23)
    uh, du, k, a, b = fields(shape, dt)
    fft = PFFT(comm.COMM_SELF, shape, dtype=dt)
    ops = spectral.SpectralOps(fft, R.BOX)
    blk, npts = ops.shape, int(np.prod(shape))
    assert blk == uh.shape[1:] and all(np.array_equal(_h(x), y) for x, y in zip(ops.K, k))

    def spec(src=None, d=dt):
        x = newDistArray(fft, rank=1)
        if src is not None:
            x[...] = np.array(src)
        return x if d == dt else torch.as_tensor(np.asarray(x).astype(d.upper()), device=x.tensor.device)

    def phys(src=None, d=dt):
        x = newDistArray(fft, False, rank=1)
        if src is not None:
            x[...] = np.array(src)
        return x if d == dt else torch.as_tensor(np.asarray(x).astype(d), device=x.tensor.device)

    def calls():
        out, ForcingEngine.log = ForcingEngine.log, []
        return out

    def refused(f, *args):
        with pytest.raises(AssertionError):
            f(*args)
        assert calls() == [], 'the engine was reached'
    # ---- the good calls: count, precision and the result of the stand-in
    U, W, D = spec(uh), spec(), spec(du)
    assert ops.curl(U, W) is W and calls() == [('ps_curl', blk, prec)]
    assert np.abs(np.asarray(W) - V.join(V.curl(uh, k))).max() <= 64 * eps
    assert ops.curl(U.tensor, W.tensor) is W.tensor and calls() == [('ps_curl', blk, prec)]           # plain tensors too
    assert ops.project(D, U, nu) is D and calls() == [('ps_project', nu, blk, prec)]
    A, B, C = phys(a), phys(b), phys()
    assert spectral.cross(A, B, C) is C and calls() == [('ps_cross', npts, prec)]
    assert np.abs(np.asarray(C) - V.cross(a, b)).max() <= 64 * eps
    U0, U1, Un = spec(uh), spec(du), spec()
    spectral.rk_stage(Un, U0, U1, D, CB, CA)
    assert calls() == [('ps_rk_stage', 2 * 3 * int(np.prod(blk)), CB, CA, prec, True, True)]           # complex: two reals each
    spectral.rk_stage(None, None, U1, D, 0.0, CA)
    spectral.rk_stage(None, U0, U1, D, 0.0, CA)                                  # u0 without u: allowed, not read
    assert calls() == [('ps_rk_stage', 2 * 3 * int(np.prod(blk)), 0.0, CA, prec, False, False),
                       ('ps_rk_stage', 2 * 3 * int(np.prod(blk)), 0.0, CA, prec, False, True)]
    spectral.rk_stage(C, A, B, phys(a), CB, CA)
    assert calls() == [('ps_rk_stage', 3 * npts, CB, CA, prec, True, True)]                            # real: one each
    flat = [torch.as_tensor(np.arange(7, dtype=dt), device=U.tensor.device) for _ in range(3)]
    spectral.rk_stage(None, None, flat[1], flat[2], CB, CA)                       # any one shape
    assert calls() == [('ps_rk_stage', 7, CB, CA, prec, False, False)]
    # ---- refused before the engine: operands of different dtype
    refused(ops.curl, U, spec(d=other))
    refused(ops.curl, spec(uh, other), W)
    refused(ops.project, D, spec(uh, other), nu)
    refused(ops.project, spec(du, other), U, nu)
    refused(spectral.cross, A, B, phys(d=other))
    refused(spectral.cross, A, phys(b, other), C)
    refused(spectral.rk_stage, Un, U0, U1, spec(du, other), CB, CA)
    refused(spectral.rk_stage, spec(d=other), U0, U1, D, CB, CA)
    refused(spectral.rk_stage, None, None, U1, phys(a), CB, CA)                   # complex u1, real du
    refused(ops.curl, phys(a), phys())                                           # a real field is no spectral field
    refused(spectral.cross, U, U0, W)                                            # and a complex one no physical field
    # ---- a non-contiguous operand
    refused(ops.curl, _strided(U.tensor), W)
    refused(ops.curl, U, _strided(W.tensor))
    refused(ops.project, _strided(D.tensor), U, nu)
    refused(ops.project, D, _strided(U.tensor), nu)
    refused(spectral.cross, A, _strided(B.tensor), C)
    refused(spectral.cross, A, B, _strided(C.tensor))
    refused(spectral.rk_stage, Un, U0, _strided(U1.tensor), D, CB, CA)
    refused(spectral.rk_stage, Un, _strided(U0.tensor), U1, D, CB, CA)
    refused(spectral.rk_stage, None, None, U1, _strided(D.tensor), CB, CA)
    # ---- a field of the other precision than the transform's, consistent in itself
    refused(ops.curl, spec(uh, other), spec(d=other))
    refused(ops.project, spec(du, other), spec(uh, other), nu)
    # ---- u without u0
    refused(spectral.rk_stage, Un, None, U1, D, CB, CA)
    # ---- wrong shapes
    refused(ops.curl, U.tensor[:2], W.tensor[:2])
    refused(ops.curl, U, W.tensor[:, :-1].contiguous())
    refused(ops.project, D.tensor[:, :, :-1].contiguous(), U.tensor[:, :, :-1].contiguous(), nu)
    refused(ops.project, D, U.tensor[0], nu)
    refused(spectral.cross, A.tensor[:2], B.tensor[:2], C.tensor[:2])
    refused(spectral.cross, A, B, C.tensor[:, :-1].contiguous())
    refused(spectral.rk_stage, Un, U0, U1, D.tensor[:2], CB, CA)
    refused(spectral.rk_stage, Un.tensor.reshape(-1), U0, U1, D, CB, CA)
    refused(spectral.rk_stage, None, None, flat[0][:5], flat[2], CB, CA)
    fft.destroy()


# ---- the C entries ----------------------------------------------------------------------------------------------------------
def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    for name in ('gfft_ps_curl', 'gfft_ps_cross', 'gfft_ps_project', 'gfft_ps_rk_stage'):
        assert name in _lib.EXPORTS
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def curl(u=p, out=p, k=(p, p, p), n=(2, 2, 2), prec=8):
        return lib.gfft_ps_curl(u, out, k[0], k[1], k[2], n[0], n[1], n[2], prec, None)

    def cross(a=p, b=p, out=p, count=8, prec=8):
        return lib.gfft_ps_cross(a, b, out, count, prec, None)

    def proj(du=p, u=p, k=(p, p, p), n=(2, 2, 2), nu=0.03, prec=8):
        return lib.gfft_ps_project(du, u, k[0], k[1], k[2], n[0], n[1], n[2], nu, prec, None)

    def rk(u=p, u0=p, u1=p, du=p, count=8, cb=CB, ca=CA, prec=8):
        return lib.gfft_ps_rk_stage(u, u0, u1, du, count, cb, ca, prec, None)
    axes = (dict(k=(None, p, p)), dict(k=(p, None, p)), dict(k=(p, p, None)), dict(n=(-1, 2, 2)), dict(n=(2, -1, 2)), dict(n=(2, 2, -1)))
    precs = (dict(prec=0), dict(prec=3), dict(prec=16), dict(prec=-8))
    for bad in (dict(u=None), dict(out=None)) + axes + precs:
        assert curl(**bad) == -1, bad
    assert lib.gfft_last_error() == b'gfft_ps_curl: bad argument'
    for bad in (dict(a=None), dict(b=None), dict(out=None), dict(count=-1)) + precs:
        assert cross(**bad) == -1, bad
    assert lib.gfft_last_error() == b'gfft_ps_cross: bad argument'
    for bad in (dict(du=None), dict(u=None)) + axes + precs:
        assert proj(**bad) == -1, bad
    assert lib.gfft_last_error() == b'gfft_ps_project: bad argument'
    for bad in (dict(u1=None), dict(du=None), dict(u0=None), dict(count=-1)) + precs:
        assert rk(**bad) == -1, bad                          # u0=None with u given: u needs u0
    assert lib.gfft_last_error() == b'gfft_ps_rk_stage: bad argument'
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device
        assert curl() == -3 and curl(prec=4) == -3 and curl(n=(0, 2, 2)) == -3
        assert cross() == -3 and cross(prec=4) == -3 and cross(count=0) == -3
        assert proj() == -3 and proj(prec=4, nu=0.0) == -3 and proj(n=(2, 0, 2)) == -3
        assert rk() == -3 and rk(prec=4, count=0) == -3
        assert rk(u=None) == -3 and rk(u=None, u0=None) == -3          # d_u null is allowed, with or without d_u0
