"""Host logic of the particle-to-grid spread (no GPU): the argument forms and refusals of `SpectralOps.spread` over numpy
stand-ins for the two kernels (tests/spread_ref.py), the default scale_exp rule, what reaches the engine, the assembly of
thread ranks' blocks, an empty rank, the argument checks of gfft_ps_spread and gfft_ps_spread_finish through ctypes, and the
properties of the method on the reference itself: order independence, the split into blocks, the accuracy bound, mass,
adjointness with tests/interp_ref.py and the end-to-end adjoint chain through numpy's FFT."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import cases, interp_ref as I, spectrum_ref as R, spread_ref as S
from tests.test_forcing_host import ForcingEngine, _h
from tests.test_interp_host import InterpEngine


class SpreadEngine(InterpEngine):
    """InterpEngine plus the two new entries restated through tests/spread_ref.py on host tensors"""

    def ps_spread(self, tacc, ncomp, n, start, N, inv_dx, tx, tq, npart, order, scale_exp, tskipped):
        ForcingEngine.log.append(('ps_spread', int(ncomp), tuple(n), tuple(start), tuple(N), tuple(inv_dx), int(npart), int(order), int(scale_exp)))
        assert tacc.dtype == torch.int64 and tacc.numel() == ncomp * int(np.prod(n)) and tuple(tx.shape) == (npart, 3)
        assert tq.numel() == npart * ncomp and tskipped.dtype == torch.int64 and tuple(tskipped.shape) == (1,)
        acc, skipped, _, _, _ = S.spread_int(_h(tq).reshape(npart, ncomp), _h(tx), inv_dx, order, N, start, n, scale_exp, exact=False, acc=_h(tacc))
        tacc.copy_(torch.as_tensor(acc.reshape(tuple(tacc.shape))))
        tskipped += skipped

    def ps_spread_finish(self, tout, tacc, count, factor, clear, precision):
        ForcingEngine.log.append(('ps_spread_finish', int(count), float(factor), bool(clear), precision))
        assert tacc.numel() == count == tout.numel()
        out = S.finish(_h(tacc).reshape(-1), factor, np.float64 if precision == 8 else np.float32)
        tout.copy_(torch.as_tensor(out.reshape(tuple(tout.shape))))
        if clear:
            tacc.zero_()


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(SpreadEngine())
    ForcingEngine.log = []
    yield
    _lib.set_engine(old)


SHAPE = (8, 6, 20)
BLOCKS = ((8, 6, 20), (5, 3, 7), (3, 2, 5))


def _inv_dx(N):
    return tuple(n / l for n, l in zip(N, R.BOX))


def _particles(P, m, seed, span=(-2.0, 3.0)):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((P, m)), rng.uniform(span[0], span[1], (P, 3)) * np.asarray(R.BOX)


def test_spread_argument_forms(engine):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    fft = PFFT(comm.COMM_SELF, SHAPE, dtype='d')
    ops = spectral.SpectralOps(fft, R.BOX)
    inv_dx = _inv_dx(SHAPE)
    q_h, x_h = _particles(37, 4, 61)
    U = newDistArray(fft, False, rank=1)
    dev = U.tensor.device
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    x = T(x_h)
    cnt = int(np.prod(SHAPE))
    for order in (2, 4):
        for m in (1, 2, 3, 4):
            e = S.default_scale_exp(q_h[:, :m])
            got = ops.spread(T(q_h[:, :m]), x, order=order)            # everything defaulted: a new tensor [m] + shape
            assert ForcingEngine.log[-2] == ('ps_spread', m, SHAPE, (0, 0, 0), SHAPE, inv_dx, 37, order, e)
            assert ForcingEngine.log[-1] == ('ps_spread_finish', m * cnt, 1.0 / math.ldexp(1.0, e), True, 8)
            acc, skipped, _, _, _ = S.spread_int(q_h[:, :m], x_h, inv_dx, order, SHAPE, (0, 0, 0), SHAPE, e, exact=False)
            assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and tuple(got.shape) == (m,) + SHAPE and skipped == 0
            assert np.array_equal(_h(got), S.finish(acc, 1.0 / math.ldexp(1.0, e), np.float64))
        got = ops.spread(T(q_h[:, 2]), x, order=order)                 # a scalar: [P] -> the physical shape itself
        assert tuple(got.shape) == SHAPE and ForcingEngine.log[-2][1] == 1
    assert ops.spread(T(q_h[:, :3]), x).shape == (3,) + SHAPE and ForcingEngine.log[-2][7] == 4          # order defaults to 4
    # out as a DistArray, scale_exp, factor, acc and skipped given: acc is added to and comes back cleared; skipped is added to
    acc = torch.zeros((3,) + SHAPE, dtype=torch.int64, device=dev)
    acc[1, 2, 3, 4] = 5
    skipped = torch.full((1,), 7, dtype=torch.int64, device=dev)
    q_bad = q_h[:, :3].copy()
    q_bad[3, 1], q_bad[9, 0] = np.nan, np.inf
    assert ops.spread(T(q_bad), x, order=2, out=U, scale_exp=-3, factor=0.75, acc=acc, skipped=skipped) is U
    assert ForcingEngine.log[-2][-1] == -3 and ForcingEngine.log[-1] == ('ps_spread_finish', 3 * cnt, 0.75 / 0.125, True, 8)
    pre = np.zeros((3,) + SHAPE, dtype=np.int64)
    pre[1, 2, 3, 4] = 5
    want, sk, _, _, _ = S.spread_int(q_bad, x_h, inv_dx, 2, SHAPE, (0, 0, 0), SHAPE, -3, exact=False, acc=pre)
    assert sk == 2 and int(skipped[0]) == 9 and not _h(acc).any()
    assert np.array_equal(_h(U.tensor), S.finish(want, 6.0, np.float64))
    s1 = torch.full(SHAPE, -7.0, dtype=torch.float64, device=dev)         # a scalar q into a scalar out and into [1] + shape
    assert ops.spread(T(q_h[:, 0]), x, out=s1, scale_exp=10) is s1
    s2 = torch.full((1,) + SHAPE, -7.0, dtype=torch.float64, device=dev)
    assert ops.spread(T(q_h[:, :1]), x, out=s2, scale_exp=10) is s2 and np.array_equal(_h(s1), _h(s2)[0])
    none = ops.spread(T(q_h[:0, :2]), x[:0])                           # no particles
    assert tuple(none.shape) == (2,) + SHAPE and not _h(none).any() and ForcingEngine.log[-2][-1] == 0
    n = len(ForcingEngine.log)
    q3 = T(q_h[:, :3])
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)
    for bad in (lambda: ops.spread(T(np.zeros((37, 5))), x),                                       # m = 5
                lambda: ops.spread(T(np.zeros((37, 0))), x),                                       # m = 0
                lambda: ops.spread(q3.to(torch.float32), x),                                       # q not double
                lambda: ops.spread(q_h[:, :3], x),                                                 # ... not a tensor
                lambda: ops.spread(T(np.zeros((37, 6)))[:, ::2], x),                               # ... not contiguous
                lambda: ops.spread(q3.reshape(37, 3, 1), x),
                lambda: ops.spread(q3, x.to(torch.float32)),                                       # x not double
                lambda: ops.spread(q3, x[:36]),                                                    # ... another P
                lambda: ops.spread(q3, x[:, :2]),
                lambda: ops.spread(q3, T(np.zeros((37, 6)))[:, ::2]),
                lambda: ops.spread(q3, x, order=3),
                lambda: ops.spread(q3, x, order=6),
                lambda: ops.spread(q3, x, out=z(2, *SHAPE)),                                       # out of another m
                lambda: ops.spread(q3, x, out=z(*SHAPE)),
                lambda: ops.spread(q3, x, out=z(3, *SHAPE, dt=torch.float32)),                     # ... of the other precision
                lambda: ops.spread(q3, x, out=z(3, *SHAPE[:2], 21)[..., :20]),                     # ... not contiguous
                lambda: ops.spread(q3, x, scale_exp=1001),
                lambda: ops.spread(q3, x, scale_exp=-1001),
                lambda: ops.spread(q3, x, scale_exp=2.0),
                lambda: ops.spread(q3, x, factor=np.inf),
                lambda: ops.spread(q3, x, factor=np.nan),
                lambda: ops.spread(q3, x, acc=z(3, *SHAPE)),                                       # acc not int64
                lambda: ops.spread(q3, x, acc=z(2, *SHAPE, dt=torch.int64)),
                lambda: ops.spread(q3, x, acc=z(*SHAPE, dt=torch.int64)),
                lambda: ops.spread(q3, x, skipped=z(1)),                                           # skipped not int64
                lambda: ops.spread(q3, x, skipped=z(2, dt=torch.int64))):
        with pytest.raises(AssertionError):
            bad()
    assert len(ForcingEngine.log) == n, 'a refused call reached the engine'
    fft.destroy()


def test_single_precision_transform(engine):
    from mpi4py_fft_amd import PFFT, comm, spectral
    fft = PFFT(comm.COMM_SELF, SHAPE, dtype='f')
    ops = spectral.SpectralOps(fft, R.BOX)
    q_h, x_h = _particles(50, 2, 62)
    got = ops.spread(torch.as_tensor(q_h), torch.as_tensor(x_h), order=4, scale_exp=30, factor=3.0)
    assert got.dtype == torch.float32 and ForcingEngine.log[-1] == ('ps_spread_finish', 2 * int(np.prod(SHAPE)), 3.0 / 2.0 ** 30, True, 4)
    acc, _, _, _, _ = S.spread_int(q_h, x_h, _inv_dx(SHAPE), 4, SHAPE, (0, 0, 0), SHAPE, 30, exact=False)
    assert np.array_equal(_h(got), S.finish(acc, 3.0 / 2.0 ** 30, np.float32))
    with pytest.raises(AssertionError):
        ops.spread(torch.as_tensor(q_h), torch.as_tensor(x_h), out=torch.zeros((2,) + SHAPE, dtype=torch.float64))
    fft.destroy()


def test_default_scale_exp_rule():
    """floor(log2(2^62 / S)) with S = max_c sum_p |q[p][c]| over the FINITE entries; clamped; 0 for S = 0"""
    from mpi4py_fft_amd import spectral
    rule = spectral.SpectralOps.spread_scale_exp
    T = torch.as_tensor
    assert rule(T(np.zeros((5, 2)))) == 0 and rule(T(np.zeros((0, 3)))) == 0 and rule(T(np.array([-0.0, 0.0]))) == 0
    assert rule(T(np.array([1.0]))) == 62 and rule(T(np.array([-1.0, 1.0]))) == 61 and rule(T(np.array([1.5]))) == 61
    assert rule(T(np.array([0.75, 0.25, -1.0]))) == 61 and rule(T(np.array([3.0]))) == 60 and rule(T(np.array([4.0]))) == 60
    assert rule(T(np.array([[1.0, -8.0], [1.0, 0.5]]))) == 58                  # the larger column: 8.5
    assert rule(T(np.array([[1.0, np.nan], [np.inf, 2.0], [-np.inf, 1.0]]))) == 60          # column sums 1 and 3 over the finite entries
    assert rule(T(np.array([np.nan, np.inf]))) == 0
    assert rule(T(np.array([2.0 ** -990]))) == 1000 and rule(T(np.array([2.0 ** 1020]))) == -958 and rule(T(np.array([1e308, 1e308]))) == -1000
    assert rule(T(np.array([2.0 ** 1023, 2.0 ** 1023]))) == -1000              # finite entries whose sum is not
    rng = np.random.default_rng(63)
    for scale in (1e-30, 1e-3, 1.0, 37.0, 1e12, 1e200):
        q = np.ldexp(rng.integers(-2 ** 20, 2 ** 20, (200, 3)).astype(np.float64), -20) * scale          # (sums of few-bit values: exact in any order)
        e = rule(T(q))
        assert e == S.default_scale_exp(q)
        Ssum = np.abs(q).sum(axis=0).max()
        assert math.ldexp(Ssum, e) <= 2.0 ** 62 < math.ldexp(Ssum, e + 1)


@pytest.mark.parametrize('nranks,grid', [(2, [2, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'pencil4'])
@pytest.mark.parametrize('order', [2, 4])
def test_thread_ranks_assemble_to_the_whole(nranks, grid, order, engine):
    """x and q replicated: each rank's out is its block of the one-rank field, bit for bit, with no reduction; every rank that
    owns a block counts the same skipped particles; the engine sees each rank's own start and n"""
    from mpi4py_fft_amd import PFFT, comm, spectral
    shape = (8, 8, 20)
    q_h, x_h = _particles(60, 3, 64)
    q_h[7, 1], x_h[11, 2] = np.nan, np.inf

    def body(cm):
        fft = PFFT(cm, shape, dtype='d', grid=grid, wire='torch') if cm.Get_size() > 1 else PFFT(cm, shape, dtype='d')
        ops = spectral.SpectralOps(fft, R.BOX)
        sk = torch.zeros(1, dtype=torch.int64)
        out = ops.spread(torch.as_tensor(q_h), torch.as_tensor(x_h), order=order, scale_exp=40, factor=0.5, skipped=sk)
        res = _h(out).copy(), fft.local_slice(False), int(sk[0]), ops.pstart, ops.pshape
        fft.destroy()
        return res
    whole = cases.run_ranks(1, body)[0][0]
    res = cases.run_ranks(nranks, body)
    seen = np.zeros(shape, dtype=int)
    for out, sl, sk, pstart, pshape in res:
        assert sk == 2 and out.shape == (3,) + pshape
        assert np.array_equal(out, whole[(slice(None),) + tuple(sl)])
        seen[tuple(sl)] += 1
    assert (seen == 1).all(), 'the blocks do not tile the grid'
    assert any(r[0].any() for r in res)


class _EmptyBlockFft:
    """What SpectralOps reads of a transform, for a rank whose physical block is empty (PFFT itself gives every rank of a grid
    at least one plane, so such a rank is stated here directly): a (4, 4, 6) real transform, this rank past the end of axis 0"""
    subcomm = ()

    class forward:
        output_array = torch.zeros(0, dtype=torch.complex128)

    def global_shape(self, spectral=False):
        return (4, 4, 4) if spectral else (4, 4, 6)

    def shape(self, spectral=False):
        return (4, 0, 4) if spectral else (0, 4, 6)

    def local_slice(self, spectral=False):
        return (slice(0, 4), slice(4, 4), slice(0, 4)) if spectral else (slice(4, 4), slice(0, 4), slice(0, 6))

    def dtype(self, spectral=False):
        return np.dtype('D' if spectral else 'd')


def test_an_empty_rank(engine):
    """A rank without a block zero-fills out and launches nothing"""
    from mpi4py_fft_amd import spectral
    ops = spectral.SpectralOps(_EmptyBlockFft(), R.BOX)
    assert ops.pshape == (0, 4, 6) and ops.pstart == (4, 0, 0)
    q_h, x_h = _particles(20, 2, 65)
    out = torch.full((2, 0, 4, 6), -7.0, dtype=torch.float64)
    assert ops.spread(torch.as_tensor(q_h), torch.as_tensor(x_h), order=2, out=out, scale_exp=30) is out
    fresh = ops.spread(torch.as_tensor(q_h[:, 0].copy()), torch.as_tensor(x_h))
    assert tuple(fresh.shape) == (0, 4, 6) and fresh.dtype == torch.float64
    assert ForcingEngine.log == [], 'the empty rank reached the engine'
    with pytest.raises(AssertionError):
        ops.spread(torch.as_tensor(q_h), torch.as_tensor(x_h), order=3)          # the refusals come first here too


# ---- the properties of the method, on the reference ---------------------------------------------------------------------

@pytest.mark.parametrize('order', [2, 4])
@pytest.mark.parametrize('N', BLOCKS)
def test_reference_accuracy_order_and_split(N, order):
    """The fixed-point result lies within n_l 2^-(e+1) + 16 * 2^-53 M_l of the long-double sum; a permutation of the particles
    leaves every integer unchanged; the two slabs of a split concatenate to the whole bit for bit"""
    inv_dx = _inv_dx(N)
    for P in (1, 65, 1000):
        q, x = _particles(P, 2, 66 + P)
        e = S.default_scale_exp(q)
        acc, sk, count, exact, M = S.spread_int(q, x, inv_dx, order, N, (0, 0, 0), N, e)
        assert sk == 0 and count.sum() == P * order ** 3
        err = np.abs(np.ldexp(acc.astype(np.longdouble), -e) - exact)
        assert np.all(err <= S.bound(count, M, e))
        perm = np.random.default_rng(67).permutation(P)
        assert np.array_equal(S.spread_int(q[perm], x[perm], inv_dx, order, N, (0, 0, 0), N, e, exact=False)[0], acc)
        cut = N[0] // 2
        lo = S.spread_int(q, x, inv_dx, order, N, (0, 0, 0), (cut,) + N[1:], e, exact=False)[0]
        hi = S.spread_int(q, x, inv_dx, order, N, (cut, 0, 0), (N[0] - cut,) + N[1:], e, exact=False)[0]
        assert np.array_equal(np.concatenate([lo, hi], axis=1), acc)


@pytest.mark.parametrize('order', [2, 4])
def test_mass(order):
    """sum_l field = sum_p q within P order^3 2^-(e+1) + 16 * 2^-53 sum |q|: the weights sum to one"""
    for N in BLOCKS:
        for P, e in ((1, 50), (65, 40), (1000, 20), (1000, -2)):
            q, x = _particles(P, 3, 68 + P)
            acc, _, _, _, _ = S.spread_int(q, x, _inv_dx(N), order, N, (0, 0, 0), N, e, exact=False)
            total = np.ldexp(acc.reshape(3, -1).astype(np.longdouble).sum(axis=1), -e)
            want = q.astype(np.longdouble).sum(axis=0)
            lim = P * order ** 3 * 2.0 ** -(e + 1) + 16 * S.EPS * np.abs(q).sum(axis=0)
            assert np.all(np.abs(total - want) <= lim), (N, P, e)


@pytest.mark.parametrize('order', [2, 4])
def test_adjoint_of_the_interpolation(order):
    """<interp(c), q> = <c, spread(q)>: the difference stays below (order^3 + 80) 2^-53 sum |w q c| + sum_l |c_l| n_l 2^-(e+1), and, the
    quantisation aside (e = 62 - 11: its term is 2^-40 of the first), well below a tenth of 2^-53 sum |w q c| ... measured
    against the long-double forms of both sides"""
    for N in BLOCKS:
        q, x = _particles(300, 1, 70)
        c = np.random.default_rng(71).standard_normal((1,) + N)
        e = S.default_scale_exp(q)
        acc, _, count, exact, _ = S.spread_int(q, x, _inv_dx(N), order, N, (0, 0, 0), N, e)
        val, _ = I.interp(c, x, _inv_dx(N), order)
        lhs = (val[:, 0] * q[:, 0].astype(np.longdouble)).sum()
        _, Mabs = I.interp(np.abs(c), x, _inv_dx(N), order)
        scale = float((Mabs[:, 0] * np.abs(q[:, 0])).sum())                   # sum |w q c|
        rhs_exact = (c[0].astype(np.longdouble) * exact[0]).sum()
        assert abs(lhs - rhs_exact) <= 0.1 * S.EPS * scale                    # the two long-double sides: one operator and its transpose
        rhs = (c[0].astype(np.longdouble) * np.ldexp(acc[0].astype(np.longdouble), -e)).sum()
        quant = float((np.abs(c[0]) * count).sum()) * 2.0 ** -(e + 1)
        assert abs(lhs - rhs) <= (order ** 3 + 80) * S.EPS * scale + quant


def test_end_to_end_adjoint_chain():
    """scale_axes(rfftn(spread(q, x, 4)), bspline_vectors(4)) against interp(irfftn(scale_axes(f_hat, bspline_vectors(4))), x, 4) at
    16^3 with numpy's FFT: Re <A f_hat, q> = Re <f_hat, A^T q> under the Hermitian-weighted inner product, to cases.rounding_tol of
    the sum of the terms' magnitudes"""
    N = (16, 16, 16)
    inv_dx = [n / (2 * np.pi) for n in N]
    rng = np.random.default_rng(72)
    q, x = rng.standard_normal((200, 1)), rng.uniform(-10.0, 20.0, (200, 3))
    g = np.fft.rfftn(rng.standard_normal(N))                              # a Hermitian spectrum
    bv = I.bspline_vectors(N, 4)
    coeff = np.fft.irfftn(I.scale_axes(g[None], bv)[0], s=N, axes=(0, 1, 2))              # the type-2 side: prefilter, backward, gather
    val, M = I.interp(coeff[None], x, inv_dx, 4)
    lhs = float((val[:, 0] * q[:, 0]).sum())
    e = S.default_scale_exp(q)
    acc, _, _, _, _ = S.spread_int(q, x, inv_dx, 4, N, (0, 0, 0), N, e, exact=False)
    field = S.finish(acc, 1.0 / math.ldexp(1.0, e), np.float64)[0]
    h = I.scale_axes(np.fft.rfftn(field)[None], bv)[0]                    # the type-1 side: scatter, forward, deconvolve
    w = np.full(g.shape[2], 2.0)
    w[0] = w[-1] = 1.0                                                    # (N2 even: the columns 0 and N2 / 2 are their own mirrors)
    terms = (g * np.conj(h)).real * w[None, None, :] / np.prod(N)         # <g, h> over the full spectrum, irfftn's 1 / N^3 included
    rhs = float(terms.sum())
    size = float((M[:, 0] * np.abs(q[:, 0])).sum()) + float(np.abs(terms).sum())
    assert abs(lhs - rhs) <= cases.rounding_tol('d', int(np.prod(N))) * size, (lhs, rhs, size)
    assert abs(lhs) > 1e-6 * size                                         # (the two sides are not both nothing)


# ---- the C entry points -------------------------------------------------------------------------------------------------

def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    for name in ('gfft_ps_spread', 'gfft_ps_spread_finish'):
        assert name in _lib.EXPORTS
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    I64 = lambda v: None if v is None else (ctypes.c_int64 * 3)(*v)
    D3 = lambda v: None if v is None else (ctypes.c_double * 3)(*v)

    def spread(acc=p, nc=3, n=(2, 2, 2), start=(0, 0, 0), N=(4, 4, 4), inv_dx=(1.0, 1.0, 1.0), x=p, q=p, np_=2, order=4, e=10, sk=p):
        return lib.gfft_ps_spread(acc, nc, I64(n), I64(start), I64(N), D3(inv_dx), x, q, np_, order, e, sk, None)
    for bad in (dict(acc=None), dict(x=None), dict(q=None), dict(sk=None), dict(n=None), dict(start=None), dict(N=None), dict(inv_dx=None),
                dict(nc=0), dict(nc=-2), dict(np_=-1)):
        assert spread(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_spread: bad argument'
    for order in (0, 1, 3, 5, 6, 8, -4):
        assert spread(order=order) == -1 and lib.gfft_last_error() == b'gfft_ps_spread: order must be 2 or 4'
    for e in (1001, -1001, 1 << 20, -(1 << 20)):
        assert spread(e=e) == -1 and lib.gfft_last_error() == b'gfft_ps_spread: |scale_exp| must not exceed 1000'
    for bad in (dict(n=(0, 2, 2)), dict(n=(2, -1, 2)), dict(N=(4, 0, 4)), dict(N=(4, 4, -4)), dict(start=(3, 0, 0)), dict(start=(0, 0, -1)),
                dict(n=(2, 2, 5)), dict(start=(0, 5, 0)), dict(start=(1 << 62, 0, 0), n=(1 << 62, 2, 2))):
        assert spread(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_spread: a block needs n >= 1, N >= 1 and 0 <= start, start + n <= N'
    for bad in (dict(inv_dx=(0.0, 1.0, 1.0)), dict(inv_dx=(1.0, -1.0, 1.0)), dict(inv_dx=(1.0, 1.0, np.inf)), dict(inv_dx=(np.nan, 1.0, 1.0))):
        assert spread(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_spread: inv_dx must be finite and > 0'
    assert spread(nc=5) == -2 and lib.gfft_last_error() == b'gfft_ps_spread: more than 4 components'
    big = (1 << 40) + 1
    assert spread(N=(big, 4, 4)) == -2 and lib.gfft_last_error() == b'gfft_ps_spread: block too large'
    assert spread(nc=5, order=3) == -1 and spread(nc=5, inv_dx=(0.0, 1.0, 1.0)) == -1 and spread(nc=5, q=None) == -1 and spread(nc=5, e=2000) == -1

    def finish(out=p, acc=p, count=8, factor=0.5, clear=1, prec=8):
        return lib.gfft_ps_spread_finish(out, acc, count, factor, clear, prec, None)
    for bad in (dict(out=None), dict(acc=None), dict(count=-1), dict(factor=np.inf), dict(factor=-np.inf), dict(factor=np.nan),
                dict(prec=3), dict(prec=16), dict(prec=0)):
        assert finish(**bad) == -1, bad
        assert lib.gfft_last_error() == b'gfft_ps_spread_finish: bad argument'
    # (every call above is refused: a refused call dereferences no pointer.  Good calls are made only where there is no device)
    if not torch.cuda.is_available():
        assert spread() == -3 and spread(order=2, nc=1) == -3 and spread(np_=0) == -3 and spread(e=-1000) == -3 and spread(e=1000) == -3
        assert spread(n=(2, 1, 3), start=(1, 0, 0), N=(3, 1, 3)) == -3                             # N < order: the stencil wraps onto itself
        assert spread(n=(2, 2, 2), start=(2, 2, 2)) == -3                                          # start + n == N
        assert finish() == -3 and finish(count=0) == -3 and finish(clear=0, prec=4) == -3 and finish(factor=0.0) == -3
