"""gfft_ps_histogram / gfft_ps_gradient_pdf on the device against tests/pdf_ref.py: every comparison is for EQUALITY of int64
arrays -- counts are integers, the bin rule is one defined sequence of IEEE double operations, and the device forms the gradient
quantities without fused multiply-adds, exactly as numpy does.

Launch geometry the cases are chosen against (csrc/spectral.hip): that of gfft_ps_stats -- V points per lane and load (16 bytes:
2 in fp64, 4 in fp32, where V divides count and the base is 16-byte aligned; else 1), each workgroup one contiguous chunk of
whole steps of 256 V points, at most 2048 workgroups (fewer for a table beyond 4096 counters: 512 at 16384).  960 points: two
workgroups (fp64) or one (fp32); 105 is odd: V = 1; 960 points one element into an allocation: V = 1 with an even count; 34 816:
68 / 34 workgroups; 1 228 800 (fp64) and 2 621 440 (fp32) exceed 2048 * 256 * V, so every lane takes a second step of its chunk,
and with the large tables many more.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, pdf_ref as P, spectrum_ref as R

DEV = 'cuda'
TORCH = {'d': torch.float64, 'f': torch.float32}
WIDE = {'d': 2, 'f': 4}
KINDS = {'small': (8, 6, 20), 'odd': (5, 3, 7), 'misaligned': (8, 6, 20), 'many workgroups': (32, 32, 34)}
SWEEP_SHAPE = {'d': (128, 96, 100), 'f': (128, 128, 160)}
NBINS = (1, 7, 64, 4096)
RANGES = [(-2.5 + 0.5 * c, 2.5 - 0.25 * c) for c in range(4)]          # component 0: (-2.5, 2.5); all exact in float32
_REF = {}


def _count(kind, dt):
    return int(np.prod(SWEEP_SHAPE[dt] if kind == 'sweep' else KINDS[kind]))


def _geometry(count, dt, aligned=True, max_wg=2048):
    V = WIDE[dt] if (count % WIDE[dt] == 0 and aligned) else 1
    step = 256 * V
    chunk = -(-(-(-count // max_wg)) // step) * step
    return V, chunk, -(-count // chunk) if count else 0


def _max_wg(ncounters):
    return 2048 if ncounters <= 4096 else 2048 * 4096 // ncounters


def _scalar_field(kind, dt):
    """(u [4][count] in the precision under test, {nbins: reference [4][nbins + 3]}): a standard normal field with, in every
    component c, the edge values of ITS range planted; computed once per case, never modified"""
    key = ('u', kind, dt)
    if key not in _REF:
        count = _count(kind, dt)
        u = np.random.default_rng(91).standard_normal((4, count)).astype(dt)
        tiny = np.nextafter(np.array(0, dtype=dt), np.array(1, dtype=dt))          # the smallest denormal of the precision
        for c, (lo, hi) in enumerate(RANGES):
            lo, hi = np.array(lo, dtype=dt), np.array(hi, dtype=dt)
            planted = [lo, hi, np.nextafter(hi, np.array(-np.inf, dtype=dt)), np.inf, -np.inf, np.nan, -0.0, tiny, -tiny]
            at = (np.arange(len(planted)) * 11 + 3 + c) % count
            assert len(set(at)) == len(planted)
            u[c, at] = planted
        ref = {n: P.histogram(u, RANGES, n) for n in NBINS}
        u.setflags(write=False)
        _REF[key] = (u, ref)
    return _REF[key]


def _tensor_field(kind, dt):
    """(A [3][3][count] in the precision under test, its seven quantities in double): computed once per case, never modified"""
    key = ('A', kind, dt)
    if key not in _REF:
        A = np.random.default_rng(71).standard_normal((3, 3, _count(kind, dt))).astype(dt)
        A.setflags(write=False)
        _REF[key] = (A, P.quantities(A))
    return _REF[key]


def _device(a, dt, misaligned=False):
    flat = torch.as_tensor(np.ascontiguousarray(a).reshape(-1).astype(dt))
    if not misaligned:
        t = flat.to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(flat.numel() + 1, dtype=flat.dtype, device=DEV)
    t = buf[1:]
    t.copy_(flat)
    assert t.data_ptr() % 16 != 0
    return t


def _hist(t, m, count, ranges, nbins, dt):
    """gfft_ps_histogram straight through the engine on a flat device tensor, into an array prefilled with garbage"""
    from mpi4py_fft_amd import _lib
    out = torch.full((m, nbins + P.TAIL), -7, dtype=torch.int64, device=DEV)
    _lib.engine().ps_histogram(t, m, count, [r[0] for r in ranges], [r[1] for r in ranges], nbins, out, 8 if dt == 'd' else 4)
    return out.cpu().numpy()


def _gpdf(t, count, x, xr, nbx, dt, y=None, yr=(0.0, 1.0), nby=1):
    """gfft_ps_gradient_pdf straight through the engine on a flat device tensor, into an array prefilled with garbage"""
    from mpi4py_fft_amd import _lib
    n = nbx + P.TAIL if y is None else nbx * nby + 2
    out = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    qy = _lib.PS_Q_NONE if y is None else P.QUANTITIES.index(y)
    _lib.engine().ps_gradient_pdf(t, count, P.QUANTITIES.index(x), xr, nbx, qy, yr, nby, out, 8 if dt == 'd' else 4)
    return out.cpu().numpy()


@pytest.mark.parametrize('m', [1, 2, 3, 4])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', ['small', 'odd', 'misaligned', 'many workgroups', 'sweep'])
def test_histogram_against_reference(kind, dt, m):
    """Every count equal to the reference for 1, 7, 64 and 4096 bins, with exactly lo, exactly hi, the value below hi, +-inf, NaN,
    -0.0 and denormals of either sign planted in every component; garbage in d_out is overwritten; a second call gives the
    identical array."""
    u, ref = _scalar_field(kind, dt)
    count = u.shape[1]
    t = _device(u[:m], dt, kind == 'misaligned')
    for nbins in NBINS:
        # the geometry that runs: 2048 workgroups at most up to 4096 counters, then in inverse proportion (512 at 4 x 4096)
        max_wg = _max_wg(m * nbins)
        V, chunk, nwg = _geometry(count, dt, kind != 'misaligned', max_wg)
        assert V == (WIDE[dt] if kind in ('small', 'many workgroups', 'sweep') else 1)
        assert kind != 'many workgroups' or nwg >= 32
        assert kind != 'sweep' or (nwg > max_wg // 2 and chunk >= 2 * 256 * V and (max_wg < 2048 or chunk == 2 * 256 * V))
        want = ref[nbins][:m]
        got = _hist(t, m, count, RANGES[:m], nbins, dt)
        assert got.dtype == np.int64 and np.all(got.sum(axis=1) == count), (nbins, got.sum(axis=1))
        assert np.array_equal(got, want), (kind, dt, m, nbins, np.argwhere(got != want)[:8].tolist())
        assert np.array_equal(_hist(t, m, count, RANGES[:m], nbins, dt), got), 'the result does not repeat'
        # the planted values: hi and +inf above, -inf below, one NaN; lo itself opens bin 0 (the value below hi goes where the
        # rule's rounding puts it: the reference decides)
        assert np.all(got[:, nbins + 1] >= 2) and np.all(got[:, nbins] >= 1) and np.all(got[:, nbins + 2] == 1)
        assert np.all(got[:, 0] >= 1)


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', ['small', 'sweep'])
def test_constant_field_lands_in_one_bin(kind, dt):
    """Worst contention: every lane of every wave bumps the same counter.  The bin holds `count` -- at the sweep shape more
    than a 16-bit, and far more than a per-step, counter would."""
    count = _count(kind, dt)
    m, nbins, rg = 3, 256, [(-4.0, 4.0)] * 3
    t = torch.full((m * count,), 0.3, dtype=TORCH[dt], device=DEV)
    b = int(P.slots(np.array([0.3], dtype=dt), -4.0, 4.0, nbins)[0])
    assert b == 137
    got = _hist(t, m, count, rg, nbins, dt)
    want = np.zeros((m, nbins + P.TAIL), dtype=np.int64)
    want[:, b] = count
    assert np.array_equal(got, want), (got[:, b], count, got.sum(axis=1))
    # the same through the gradient PDFs: A_ij = 0.3 everywhere puts div = 0.9 (rounded as the rule says) into one bin
    A = torch.full((9 * count,), 0.3, dtype=TORCH[dt], device=DEV)
    x = np.full((3, 3, 1), 0.3, dtype=dt)
    for got, want in ((_gpdf(A, count, 'div', (-4.0, 4.0), nbins, dt), P.gradient_pdf(x, 'div', (-4.0, 4.0), nbins)),
                      (_gpdf(A, count, 'R', (-1.0, 1.0), 16, dt, 'Q', (-1.0, 1.0), 16), P.gradient_pdf(x, 'R', (-1.0, 1.0), 16, 'Q', (-1.0, 1.0), 16))):
        assert want.sum() == 1 and want.max() == 1
        assert np.array_equal(got, want * count), (np.flatnonzero(got), np.flatnonzero(want))


RANGE_1D = {'ss': (0.0, 12.0), 'ww': (0.0, 24.0), 'div': (-3.0, 3.0), 'Q': (-4.0, 4.0), 'R': (-5.0, 5.0), 'sss': (-20.0, 20.0),
            'wsw': (-30.0, 30.0)}


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', ['small', 'odd'])
def test_gradient_pdf_1d_every_quantity(kind, dt):
    """Each of the seven quantities on a random tensor with one NaN off the diagonal and one on it: a NaN lands in the NaN slot
    of exactly the quantities that read it -- div reads the diagonal alone, ww everything but the diagonal."""
    A0, _ = _tensor_field(kind, dt)
    A = np.array(A0)
    count = A.shape[2]
    A[1, 2, 41] = np.nan
    A[0, 0, 77] = np.nan
    q = P.quantities(A)
    t = _device(A, dt)
    for name in P.QUANTITIES:
        want = P.gradient_pdf(q, name, RANGE_1D[name], 64)
        got = _gpdf(t, count, name, RANGE_1D[name], 64, dt)
        assert got.sum() == count and np.array_equal(got, want), (kind, dt, name, np.flatnonzero(got != want)[:8].tolist())
        assert got[66] == {'div': 1, 'ww': 1}.get(name, 2), (name, got[64:])
        assert (got[:64] > 0).sum() > 8 and (kind == 'odd' or got[64] + got[65] > 0), (name, got)      # (105 points may all lie inside)
        assert np.array_equal(_gpdf(t, count, name, RANGE_1D[name], 64, dt), got), 'the result does not repeat'


JOINT = {('R', 'Q'): ((-2.0, 2.0), (-3.0, 1.5)), ('ww', 'ss'): ((0.5, 20.0), (1.0, 9.0))}


@pytest.mark.parametrize('pair', sorted(JOINT), ids='-'.join)
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', ['small', 'odd', 'misaligned', 'sweep'])
def test_gradient_pdf_joint(kind, dt, pair):
    """(R, Q) and (ww, ss) at 1 x 1, 3 x 5 and 128 x 128 bins on ranges that leave points outside, with a NaN planted."""
    A0, _ = _tensor_field(kind, dt)
    A = np.array(A0)
    count = A.shape[2]
    A[2, 0, 13] = np.nan
    q = P.quantities(A) if kind != 'sweep' else None
    if q is None:                                   # the large case: the quantities of the unmodified tensor, one point redone
        q = {k: v.copy() for k, v in _tensor_field(kind, dt)[1].items()}
        for k, v in P.quantities(A[:, :, 13:14]).items():
            q[k][13] = v[0]
    t = _device(A, dt, kind == 'misaligned')
    (x, y), (xr, yr) = pair, JOINT[pair]
    for nbx, nby in ((1, 1), (3, 5), (128, 128)):
        max_wg = _max_wg(nbx * nby)                 # 2048, 2048 and 512 workgroups at most
        V, chunk, nwg = _geometry(count, dt, kind != 'misaligned', max_wg)
        assert kind != 'sweep' or (nwg > max_wg // 2 and chunk == (2 if max_wg == 2048 else 5) * 256 * V)
        want = P.gradient_pdf(q, x, xr, nbx, y, yr, nby)
        got = _gpdf(t, count, x, xr, nbx, dt, y, yr, nby)
        assert got.shape == (nbx * nby + 2,) and got.sum() == count, (got.shape, got.sum())
        assert np.array_equal(got, want), (kind, dt, pair, nbx, nby, np.flatnonzero(got != want)[:8].tolist())
        assert got[-2] > 0 and got[-1] == 1, got[-2:]                     # both pairs read A[2][0]
        assert np.array_equal(_gpdf(t, count, x, xr, nbx, dt, y, yr, nby), got), 'the result does not repeat'


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_empty_block_writes_zeros(dt):
    t = torch.ones(64, dtype=TORCH[dt], device=DEV)
    assert np.array_equal(_hist(t, 3, 0, RANGES[:3], 7, dt), np.zeros((3, 10), dtype=np.int64))
    assert np.array_equal(_hist(t, 4, 0, RANGES, 4096, dt), np.zeros((4, 4099), dtype=np.int64))
    assert np.array_equal(_gpdf(t, 0, 'Q', (-1.0, 1.0), 5, dt), np.zeros(8, dtype=np.int64))
    assert np.array_equal(_gpdf(t, 0, 'R', (-1.0, 1.0), 128, dt, 'Q', (-1.0, 1.0), 128), np.zeros(16386, dtype=np.int64))


def _ops(comm, shape, dt, **kw):
    from mpi4py_fft_amd import PFFT, spectral
    fft = PFFT(comm, shape, dtype=dt, **kw)
    return fft, spectral.SpectralOps(fft, R.BOX)


def test_pdfs_replay_from_a_captured_graph():
    """out= with reduce=False under torch.cuda.graph after one warm-up call on a side stream: the replay follows new contents of
    the fields."""
    from mpi4py_fft_amd import comm, newDistArray
    shape = (8, 6, 20)
    fft, ops = _ops(comm.COMM_SELF, shape, 'd')
    U, A = newDistArray(fft, False, rank=1), newDistArray(fft, False, rank=2)
    rng = np.random.default_rng(93)
    first, second = rng.standard_normal((3, 3) + shape), rng.standard_normal((3, 3) + shape)
    rg = ((-2.0, 2.0), (-3.0, 1.5))
    oh = torch.zeros((3, 19), dtype=torch.int64, device=DEV)
    o1 = torch.zeros(35, dtype=torch.int64, device=DEV)
    oj = torch.zeros(8 * 6 + 2, dtype=torch.int64, device=DEV)

    def enqueue():
        assert ops.histogram(U, (-2.5, 2.5), 16, out=oh, reduce=False) is oh
        assert ops.gradient_pdf(A, 'ss', range=(0.0, 12.0), bins=32, out=o1, reduce=False) is o1
        assert ops.gradient_pdf(A, 'R', 'Q', range=rg, bins=(8, 6), out=oj, reduce=False) is oj
    A[...] = first
    U[...] = first[0]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        enqueue()                                   # warm-up on another stream: its scratch exists now
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    seen = []
    for field in (first, second):
        A[...] = field
        U[...] = field[0]
        for o in (oh, o1, oj):
            o.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        flat = field.reshape(3, 3, -1)
        assert np.array_equal(oh.cpu().numpy(), P.histogram(flat[0], [(-2.5, 2.5)] * 3, 16)), 'the replay does not follow U'
        assert np.array_equal(o1.cpu().numpy(), P.gradient_pdf(flat, 'ss', (0.0, 12.0), 32)), 'the replay does not follow A'
        assert np.array_equal(oj.cpu().numpy(), P.gradient_pdf(flat, 'R', rg[0], 8, 'Q', rg[1], 6)), 'the replay does not follow A'
        seen.append(oj.cpu().numpy().copy())
    assert not np.array_equal(seen[0], seen[1])
    fft.destroy()


@pytest.mark.parametrize('nranks,grid', [(2, [2, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'pencil4'])
def test_thread_ranks(nranks, grid):
    """Every rank holds the whole-array reference exactly."""
    from mpi4py_fft_amd import comm, newDistArray
    shape, dt = (24, 16, 20), 'd'
    count = int(np.prod(shape))
    A_h = np.random.default_rng(97).standard_normal((3, 3) + shape)
    q = P.quantities(A_h.reshape(3, 3, count))
    rg = JOINT[('R', 'Q')]
    want = (P.histogram(A_h[1].reshape(3, count), RANGES[:3], 64), P.gradient_pdf(q, 'wsw', RANGE_1D['wsw'], 64),
            P.gradient_pdf(q, 'R', rg[0], 128, 'Q', rg[1], 128))

    def run(c, **kw):
        fft, ops = _ops(c, shape, dt, **kw)
        A = newDistArray(fft, False, rank=2)
        A[...] = A_h[(slice(None),) * 2 + fft.local_slice(False)]
        got = (ops.histogram(A[1], RANGES[:3], 64), ops.gradient_pdf(A, 'wsw', range=RANGE_1D['wsw'], bins=64),
               ops.gradient_pdf(A, 'R', 'Q', range=rg, bins=128))
        fft.destroy()
        return got
    for res in [run(comm.COMM_SELF)] + cases.run_ranks(nranks, lambda c: run(c, grid=grid)):
        for got, ref in zip(res, want):
            assert got.dtype == np.int64 and np.array_equal(got, ref), (nranks, grid)
    assert want[2][-2] > 0 and want[2].sum() == count


def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_pdf', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example():
    """solve(gradients=True, pdfs=True, dealias='2/3') at its smallest size on one rank and on two thread ranks: every table
    totals N^3 (the pooled one 3 N^3) with an empty NaN slot, both thread ranks hold the same tables, and with pdfs off `stats`
    is what it was."""
    from mpi4py_fft_amd import comm, spectral
    ex = _example()
    M, n = 4, 16 ** 3
    kw = dict(M=M, nsteps=2, gradients=True, dealias='2/3')
    on, off = {}, {}
    ex.solve(comm.COMM_SELF, pdfs=True, stats=on, **kw)
    ex.solve(comm.COMM_SELF, stats=off, **kw)
    assert set(off) == {'gradients'} and set(on) == {'gradients', 'pdfs'} and on['gradients'] == off['gradients']
    with pytest.raises(AssertionError):
        ex.solve(comm.COMM_SELF, M=M, nsteps=1, pdfs=True)                              # without gradients
    with pytest.raises(AssertionError):
        ex.solve(comm.COMM_SELF, M=M, nsteps=1, pdfs=True, gradients=True, fused=False)

    def check(p):
        rq, lc = p['rq_counts'], p['longitudinal_counts']
        assert rq.dtype == lc.dtype == np.int64 and rq.shape == (ex.PDF_BINS ** 2 + 2,) and lc.shape == (ex.PDF_BINS + 3,)
        assert rq.sum() == n and rq[-1] == 0 and lc.sum() == 3 * n and lc[-1] == 0
        assert isinstance(p['rq'], spectral.JointPdf) and isinstance(p['longitudinal'], spectral.Pdf)
        assert p['rq'].density.shape == (ex.PDF_BINS, ex.PDF_BINS) and rq[:-2].sum() > n // 2 and lc[:-3].sum() > n
        assert abs(sum(p['quadrants']) - 1) <= 1e-12 and min(p['quadrants']) >= 0
    check(on['pdfs'])

    def body(c):
        st = {}
        ex.solve(c, pdfs=True, stats=st, **kw)
        return st['pdfs']
    res = cases.run_ranks(2, body)
    for p in res:
        check(p)
        assert np.array_equal(p['rq_counts'], res[0]['rq_counts']) and np.array_equal(p['longitudinal_counts'], res[0]['longitudinal_counts'])
