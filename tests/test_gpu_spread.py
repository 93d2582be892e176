"""gfft_ps_spread and gfft_ps_spread_finish on the device against tests/spread_ref.py, `SpectralOps.spread` on thread ranks, its
adjointness with `SpectralOps.interpolate`, and a captured call.

The accumulator is compared for EQUALITY: every contribution is rounded once to an integer and added by an integer atomic, so
whatever order the adds arrive in the device holds the integers of the numpy restatement.  gfft_ps_spread_finish is compared
for equality too (one conversion, one multiply, one narrowing).  Beside that the fixed-point field is held to the derived
bound n_l 2^-(e + 1) + 16 * 2^-53 M_l against the long-double sum (tests/spread_ref.py), the worst fraction logged in WORST.

Launch geometry the cases are chosen against (csrc/spectral.hip): workgroups of 256 lanes, at most 16384 of them, grid-stride.
  spread: order^2 lanes per particle (the geometry of gfft_ps_interp), so 16 (order 4) or 64 (order 2) particles per workgroup and
  262 144 or 1 048 576 per sweep of the grid.  P = 1: one group, the rest of the workgroup idle; 63 / 64 / 65: the last
  workgroup part-filled, full, one particle in the next (order 2); 1000: many workgroups with a part-filled last one (both
  orders); 262 147 (order 4) and 1 048 579 (order 2): every group takes a second particle.
  finish: a lane takes 16 bytes of out (2 doubles, 4 floats) where out and acc are 16-byte aligned, else one value; the values
  behind the last whole vector go to the first lanes.  Counts 1 ... 9 and 1003 cover every remainder; 'misaligned' starts out
  one element into its allocation (the one-value kernel); 16384 * 256 + 5 values through the one-value kernel and
  2 * 16384 * 256 + 7 (fp64) / 4 * 16384 * 256 + 7 (fp32) through the 16-byte kernel make lanes take a second step."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, interp_ref as I, spectrum_ref as R, spread_ref as S

DEV = 'cuda'
BLOCKS = {'small': (8, 6, 20), 'odd': (5, 3, 7), 'narrow': (3, 2, 5)}          # narrow: the order-4 stencil wraps onto itself
SWEEP = {2: 1048576 + 3, 4: 262144 + 3}
_REF = {}
WORST = {}


def _device(a, dtype=torch.float64, misaligned=False):
    flat = torch.as_tensor(np.array(a).reshape(-1)).to(dtype)          # (a copy: the cached cases are read-only)
    buf = torch.empty(flat.numel() + 1, dtype=dtype, device=DEV)
    t = buf[1:] if misaligned else buf[:-1]
    t.copy_(flat)
    assert (t.data_ptr() % 16 != 0) == misaligned
    return t


def _inv_dx(N):
    return [n / l for n, l in zip(N, R.BOX)]


def _particles(N, P, m=4, seed=81):
    """(q [P][m], x [P][3]) over five box lengths with, from P = 63 on, the edge positions planted in rows 5 ... 21 (rows 15 ... 18 are
    skipped for their position) and the edge values in rows 25 ... 33 (rows 30 ... 32 are skipped for their q: NaN, inf and a value
    beyond the 2^62 guard at every scale_exp the tests use, each in ONE component)"""
    rng = np.random.default_rng(seed)
    L = np.asarray(R.BOX)
    x = rng.uniform(-2.0, 3.0, (P, 3)) * L
    q = rng.standard_normal((P, m))
    if P >= 63:
        dx = L / np.asarray(N)
        below = np.nextafter(0.0, -1.0)
        x[5:22] = [[0, 0, 0], L, [below, 0, 0], [below, below, below], 2 * dx, [1 * dx[0], 0, (N[2] - 1) * dx[2]], -3 * dx,
                   [-0.3 * L[0], -1.7 * L[1], -0.01 * L[2]], 1000 * L + 0.37, -1000 * L - 0.37,
                   [np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1e300, 1, 1], [0.5, 0.25, 0.125], [-1e-300, 1e-300, -1e-17], [L[0], 0, L[2]]]
        q[25], q[26], q[27] = 0.0, -0.0, 1e-30                                # 1e-30 2^e rounds to 0 at every e used here
        q[28, 0], q[29, m - 1] = 2.5, -3.5
        q[30, m - 1], q[31, 0], q[32, m // 2] = np.nan, -np.inf, 1e300
    return q, x


SKIPPED = 7          # rows 15 ... 18 and 30 ... 32 of _particles


def _case(block, P, order, e):
    """(q, x, acc, skipped, count, exact, M) on the whole periodic grid = the block, m = 4; computed once, never modified.  The
    components are independent, so the first m columns of q give the first m of acc"""
    key = (block, P, order, e)
    if key not in _REF:
        N = BLOCKS[block]
        q, x = _particles(N, P)
        ref = (q, x) + S.spread_int(q, x, _inv_dx(N), order, N, (0, 0, 0), N, e)
        for a in ref:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _spread(q, x, m, n, start, N, order, e, acc=None, misaligned=False, inv_dx=None):
    """gfft_ps_spread straight through the engine: (acc as numpy, skipped)"""
    from mpi4py_fft_amd import _lib
    P = len(x)
    tq = _device(np.ascontiguousarray(np.asarray(q).reshape(P, -1)[:, :m]), misaligned=misaligned)
    tx = _device(x, misaligned=misaligned).view(P, 3)
    tacc = _device(np.zeros((m,) + tuple(n), dtype=np.int64) if acc is None else acc, torch.int64, misaligned)
    sk = torch.zeros(1, dtype=torch.int64, device=DEV)
    _lib.engine().ps_spread(tacc, m, n, start, N, _inv_dx(N) if inv_dx is None else inv_dx, tx, tq, P, order, e, sk)
    return tacc.cpu().numpy().reshape((m,) + tuple(n)), int(sk.cpu()[0])


def _accuracy(acc, count, exact, M, e, what):
    """|acc 2^-e - exact| <= n_l 2^-(e+1) + 16 * 2^-53 M_l per point; logs and returns the worst fraction"""
    err = np.abs(np.ldexp(acc.astype(np.longdouble), -e) - exact)
    lim = S.bound(count, M, e)
    hit = np.broadcast_to(count[None] > 0, err.shape)
    frac = float((err[hit] / lim[hit]).max()) if hit.any() else 0.0
    print('%s: worst fraction of the bound %.3f' % (what, frac))
    WORST[what] = frac
    assert np.all(err <= lim), (what, frac)
    return frac


@pytest.mark.parametrize('m', [1, 2, 3, 4])
@pytest.mark.parametrize('order', [2, 4])
@pytest.mark.parametrize('block', ['small', 'odd', 'narrow'])
def test_acc_against_reference(block, order, m):
    """The integers of the restatement and its skipped count for P = 1, 63, 64, 65 and 1000, at a positive and a negative
    scale_exp, with q, x and acc 16-byte aligned and one element into their allocations; the result inside the derived bound"""
    N = BLOCKS[block]
    for P in (1, 63, 64, 65, 1000):
        for e in ((40, -3) if P in (65, 1000) else (40,)):
            q, x, acc, _, count, exact, M = _case(block, P, order, e)
            sk = SKIPPED if P >= 63 else 0
            with np.errstate(all='ignore'):
                bad_rows = [r for r in (30, 31, 32) if P >= 63 and not np.all(np.abs(q[r, :m] * 2.0 ** e) < S.QLIMIT)]
            want_sk = (4 + len(bad_rows)) if P >= 63 else 0                     # a row whose bad value sits in a column >= m is an ordinary row
            if m == 4:
                assert want_sk == sk
            for mis in (False, True):
                got, got_sk = _spread(q, x, m, N, (0, 0, 0), N, order, e, misaligned=mis)
                what = '%s order %d m %d P %d e %d' % (block, order, m, P, e)
                if m == 4:
                    assert np.array_equal(got, acc), what
                else:                                                          # (the skipped rows differ with m: restate for this m)
                    want, ref_sk, _, _, _ = S.spread_int(q[:, :m], x, _inv_dx(N), order, N, (0, 0, 0), N, e, exact=False)
                    assert ref_sk == want_sk and np.array_equal(got, want), what
                assert got_sk == want_sk, what
            if m == 4:
                _accuracy(got, count, exact, M, e, what)


@pytest.mark.parametrize('order', [2, 4])
def test_planted_values(order):
    """inv_dx = 1 and integer positions put a particle ON a grid point (order 2: weight exactly 1 there, 0 on the seven others; order
    4: 1/6, 2/3, 1/6 per axis): at scale_exp = 0 a q of 2.5 and 3.5 gives 2 and 4 (ties to even), -2.5 gives -2, 0.4 and -0.4, 0.0 and
    -0.0 give 0; NaN, inf and 2^62 in ONE component skip the whole particle; 2^62 - 1024 is legal"""
    N = (8, 6, 20)
    x = np.array([[1, 2, 3], [1, 2, 3], [4, 5, 19], [7, 0, 0], [2, 2, 2], [3, 3, 3], [5, 1, 7], [6, 1, 7], [0, 1, 7], [2, 4, 9], [-1, -1, -1]], dtype=np.float64)
    q = np.array([[2.5, 3.5], [0.0, -0.0], [-2.5, 0.4], [-0.4, 0.5], [1.0, np.nan], [np.inf, 1.0], [1.0, 2.0 ** 62], [-(2.0 ** 62), 1.0],
                  [2.0 ** 62 - 1024, -(2.0 ** 62 - 1024)], [1.5, -1.5], [7.0, -8.0]])
    got, sk = _spread(q, x, 2, N, (0, 0, 0), N, order, 0, inv_dx=[1.0, 1.0, 1.0])
    want, ref_sk, _, _, _ = S.spread_int(q, x, [1.0, 1.0, 1.0], order, N, (0, 0, 0), N, 0, exact=False)
    assert sk == ref_sk == 4 and np.array_equal(got, want)
    if order == 2:
        assert got[:, 1, 2, 3].tolist() == [2, 4] and got[:, 4, 5, 19].tolist() == [-2, 0] and got[:, 7, 0, 0].tolist() == [0, 0]
        assert got[:, 0, 1, 7].tolist() == [2 ** 62 - 1024, -(2 ** 62 - 1024)] and got[:, 2, 4, 9].tolist() == [2, -2]
        assert got[:, 7, 5, 19].tolist() == [7, -8]                             # (-1, -1, -1) wraps to the last point
        assert np.count_nonzero(got) == 9 and not got[:, 2, 2, 2].any() and not got[:, 5, 1, 7].any()


@pytest.mark.parametrize('order', [2, 4])
@pytest.mark.parametrize('pieces', ['slab2', 'pencil4'])
def test_sub_blocks(pieces, order):
    """(8, 6, 20) cut into two slabs and into 2 x 2 pencils (start != 0): each piece holds the integers of the restatement for its
    start / n, every piece counts the same skipped particles, and the pieces assemble to the whole bit for bit"""
    N, P, m, e = BLOCKS['small'], 1000, 3, 40
    q, x, whole, _, _, _, _ = _case('small', P, order, e)
    blocks = [((a, 0, 0), (4, 6, 20)) for a in (0, 4)] if pieces == 'slab2' else [((a, b, 0), (4, 3, 20)) for a in (0, 4) for b in (0, 3)]
    total = np.zeros((m,) + N, dtype=np.int64)
    for start, n in blocks:
        want, ref_sk, _, _, _ = S.spread_int(q[:, :m], x, _inv_dx(N), order, N, start, n, e, exact=False)
        got, sk = _spread(q, x, m, n, start, N, order, e)
        assert np.array_equal(got, want) and sk == ref_sk, (pieces, order, start)
        total[(slice(None),) + tuple(slice(s, s + k) for s, k in zip(start, n))] = got
    ref_whole = S.spread_int(q[:, :m], x, _inv_dx(N), order, N, (0, 0, 0), N, e, exact=False)[0]
    assert np.array_equal(total, ref_whole)


@pytest.mark.parametrize('order', [2, 4])
def test_add_semantics(order):
    """Two calls into one acc equal one call on the concatenation; a pre-filled acc keeps its contents; the add wraps modulo
    2^64 as numpy's int64 does"""
    N, m, e = BLOCKS['odd'], 2, 40
    q, x, _, _, _, _, _ = _case('odd', 1000, order, e)
    q = q[:, :m]
    whole, sk = _spread(q, x, m, N, (0, 0, 0), N, order, e)
    first, sk1 = _spread(q[:400], x[:400], m, N, (0, 0, 0), N, order, e)
    both, sk2 = _spread(q[400:], x[400:], m, N, (0, 0, 0), N, order, e, acc=first)
    assert np.array_equal(both, whole) and sk1 + sk2 == sk
    pre = np.random.default_rng(82).integers(-2 ** 62, 2 ** 62, (m,) + N)
    got, _ = _spread(q, x, m, N, (0, 0, 0), N, order, e, acc=pre)
    assert np.array_equal(got, pre + whole)
    near = np.full((m,) + N, np.iinfo(np.int64).max - 5, dtype=np.int64)        # every point that receives wraps
    near[1] = np.iinfo(np.int64).min + 5
    got, _ = _spread(q, x, m, N, (0, 0, 0), N, order, e, acc=near)
    with np.errstate(over='ignore'):
        want = near + whole                                                    # (numpy's int64 add wraps)
    assert np.array_equal(got, want) and (got[0] < 0).any() and (got[1] > 0).any()
    assert np.array_equal(got, S.spread_int(q, x, _inv_dx(N), order, N, (0, 0, 0), N, e, exact=False, acc=near)[0])


@pytest.mark.parametrize('order', [2, 4])
def test_order_independence(order):
    """Shuffled particles give identical integers; 1000 particles on ONE position (every add of a component lands on the same
    order^3 addresses; in 'narrow' several of one particle's own adds do) give the restatement exactly; a second call repeats"""
    for block in ('small', 'narrow'):
        N, m, e = BLOCKS[block], 3, 40
        q, x, acc, _, _, _, _ = _case(block, 1000, order, e)
        perm = np.random.default_rng(83).permutation(1000)
        a, sk_a = _spread(q[perm], x[perm], m, N, (0, 0, 0), N, order, e)
        b, sk_b = _spread(q, x, m, N, (0, 0, 0), N, order, e)
        assert np.array_equal(a, b) and sk_a == sk_b
        one = np.tile(np.array([[0.3, 1.1, 2.9]]) * np.asarray(R.BOX) / np.asarray(N), (1000, 1))
        got, sk = _spread(q, one, m, N, (0, 0, 0), N, order, e)
        want, ref_sk, count, _, _ = S.spread_int(q[:, :m], one, _inv_dx(N), order, N, (0, 0, 0), N, e, exact=False)
        assert np.array_equal(got, want) and sk == ref_sk == 2 and count.max() >= 998          # (m = 3: rows 31 and 32)
        assert np.array_equal(_spread(q, one, m, N, (0, 0, 0), N, order, e)[0], got)


@pytest.mark.parametrize('order', [2, 4])
def test_past_one_sweep(order):
    """More particles than one sweep of the grid holds, m = 1 on (8, 6, 20): every group takes a second particle"""
    N, P, e = BLOCKS['small'], SWEEP[order], 30
    assert P * order * order > 16384 * 256
    q, x = _particles(N, P, m=1, seed=84)
    want, ref_sk, _, _, _ = S.spread_int(q, x, _inv_dx(N), order, N, (0, 0, 0), N, e, exact=False)
    got, sk = _spread(q, x, 1, N, (0, 0, 0), N, order, e)
    assert sk == ref_sk == SKIPPED and np.array_equal(got, want)


# ---- gfft_ps_spread_finish ---------------------------------------------------------------------------------------------

def _finish(acc, factor, dt, clear, misaligned=False):
    from mpi4py_fft_amd import _lib
    rdt = torch.float64 if dt == 'd' else torch.float32
    tacc = _device(acc, torch.int64)
    buf = torch.full((acc.size + 4,), -7.0, dtype=rdt, device=DEV)
    out = buf[1:1 + acc.size] if misaligned else buf[:acc.size]
    assert (out.data_ptr() % 16 != 0) == misaligned
    _lib.engine().ps_spread_finish(out, tacc, acc.size, factor, clear, 8 if dt == 'd' else 4)
    assert (buf[acc.size + (1 if misaligned else 0):] == -7.0).all() and (not misaligned or buf[0] == -7.0), 'finish wrote outside out'
    return out.cpu().numpy(), tacc.cpu().numpy()


def _integers(count, seed=85):
    rng = np.random.default_rng(seed)
    a = rng.integers(-2 ** 62, 2 ** 62, count) >> rng.integers(0, 62, count)          # every magnitude
    a[:min(count, 6)] = [0, 1, -1, 2 ** 53 + 1, -(2 ** 62) - 3, np.iinfo(np.int64).max][:min(count, 6)]          # (2^53 + 1: the conversion rounds)
    return a


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_finish_against_reference(dt):
    """Bit for bit (double)acc * factor narrowed once, for every remainder of the 16-byte vector, clear on and off, out 16-byte
    aligned and not; nothing outside out is written"""
    ndt = np.float64 if dt == 'd' else np.float32
    for count in (1, 2, 3, 4, 5, 6, 7, 8, 9, 1003):
        acc = _integers(count)
        for factor in (2.0 ** -40, 0.75 / 2.0 ** 40, -3.0e-7, 0.0):
            for clear in (True, False):
                for mis in (False, True):
                    out, left = _finish(acc, factor, dt, clear, mis)
                    want = S.finish(acc, factor, ndt)
                    assert np.array_equal(out.view(np.uint64 if dt == 'd' else np.uint32), want.view(np.uint64 if dt == 'd' else np.uint32)), (count, factor, clear, mis)
                    assert np.array_equal(left, np.zeros_like(acc) if clear else acc), (count, factor, clear, mis)


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_finish_past_one_sweep(dt):
    ndt = np.float64 if dt == 'd' else np.float32
    V = 2 if dt == 'd' else 4
    for count, mis in ((16384 * 256 + 5, True), (V * 16384 * 256 + 7, False)):
        acc = _integers(count, seed=86)
        out, left = _finish(acc, 2.0 ** -30, dt, True, mis)
        assert np.array_equal(out, S.finish(acc, 2.0 ** -30, ndt)) and not left.any()


# ---- SpectralOps.spread ------------------------------------------------------------------------------------------------

def _ops(comm, shape, dt, **kw):
    from mpi4py_fft_amd import PFFT, spectral
    fft = PFFT(comm, shape, dtype=dt, **kw)
    return fft, spectral.SpectralOps(fft, R.BOX)


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_spread_is_the_restatement_through_finish(dt):
    """Everything defaulted, and with out / acc / skipped / factor given: the field is finish(spread_int) bit for bit in both
    precisions, a caller's acc comes back cleared, skipped is added to"""
    from mpi4py_fft_amd import comm
    shape, P = BLOCKS['small'], 1000
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    ndt = np.float64 if dt == 'd' else np.float32
    q, x = _particles(shape, P, m=3, seed=87)
    q[32, 1] = np.inf                                                  # (1e300 is finite: it would set the default scale on its own)
    tq, tx = torch.as_tensor(q, device=DEV), torch.as_tensor(x, device=DEV)
    for order in (2, 4):
        e = S.default_scale_exp(q)
        assert ops.spread_scale_exp(tq) == e
        got = ops.spread(tq, tx, order=order)
        acc, sk, _, _, _ = S.spread_int(q, x, _inv_dx(shape), order, shape, (0, 0, 0), shape, e, exact=False)
        assert got.dtype == (torch.float64 if dt == 'd' else torch.float32) and tuple(got.shape) == (3,) + shape
        assert np.array_equal(got.cpu().numpy(), S.finish(acc, 1.0 / math.ldexp(1.0, e), ndt)) and sk == SKIPPED
        out = torch.full((3,) + shape, -7.0, dtype=got.dtype, device=DEV)
        tacc = torch.zeros((3,) + shape, dtype=torch.int64, device=DEV)
        skipped = torch.full((1,), 5, dtype=torch.int64, device=DEV)
        assert ops.spread(tq, tx, order=order, out=out, scale_exp=e - 7, factor=0.3, acc=tacc, skipped=skipped) is out
        acc7, _, _, _, _ = S.spread_int(q, x, _inv_dx(shape), order, shape, (0, 0, 0), shape, e - 7, exact=False)
        assert np.array_equal(out.cpu().numpy(), S.finish(acc7, 0.3 / math.ldexp(1.0, e - 7), ndt))
        assert not tacc.any() and int(skipped.cpu()[0]) == 5 + SKIPPED
    fft.destroy()


@pytest.mark.parametrize('order', [2, 4])
def test_adjoint_of_interpolate_on_the_device(order):
    """<interpolate(c), q> against <c, spread(q)> within (order^3 + 80) 2^-53 sum |w q c| + sum_l |c_l| n_l 2^-(e+1)"""
    from mpi4py_fft_amd import comm
    shape, P = BLOCKS['small'], 1000
    fft, ops = _ops(comm.COMM_SELF, shape, 'd')
    rng = np.random.default_rng(88)
    q, x = rng.standard_normal((P, 3)), rng.uniform(-2.0, 3.0, (P, 3)) * np.asarray(R.BOX)
    c = rng.standard_normal((3,) + shape)
    tq, tx, tc = (torch.as_tensor(a, device=DEV) for a in (q, x, c))
    e = S.default_scale_exp(q)
    val = ops.interpolate(tc, tx, order=order)                           # [P][3] on the host
    field = ops.spread(tq, tx, order=order, scale_exp=e).cpu().numpy()
    lhs = (val.astype(np.longdouble) * q).sum()
    rhs = (c.astype(np.longdouble) * field).sum()
    _, Mabs = I.interp(np.abs(c), x, _inv_dx(shape), order)
    scale = float((Mabs * np.abs(q)).sum())
    _, _, count, _, _ = S.spread_int(q[:, :1], x, _inv_dx(shape), order, shape, (0, 0, 0), shape, e, exact=False)
    quant = float((np.abs(c) * count[None]).sum()) * 2.0 ** -(e + 1)
    lim = (order ** 3 + 80) * S.EPS * scale + quant
    frac = float(abs(lhs - rhs)) / lim
    print('adjointness order %d: |<Ic, q> - <c, Sq>| = %.3e, %.3f of the bound' % (order, float(abs(lhs - rhs)), frac))
    WORST['adjoint order %d' % order] = frac
    assert abs(lhs - rhs) <= lim
    fft.destroy()


@pytest.mark.parametrize('nranks,grid', [(2, [2, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'pencil4'])
def test_thread_ranks(nranks, grid):
    """x and q replicated: the ranks' blocks assemble to the one-rank field with equal bits, with no reduction; every rank counts
    the same skipped particles"""
    from mpi4py_fft_amd import comm
    shape, P = (24, 16, 20), 500
    q, x = _particles(shape, P, m=3, seed=89)

    def run(cm, order):
        kw = dict(grid=grid) if cm.Get_size() > 1 else {}
        fft, ops = _ops(cm, shape, 'd', **kw)
        dev = ops.K[0].device
        sk = torch.zeros(1, dtype=torch.int64, device=dev)
        out = ops.spread(torch.as_tensor(q, device=dev), torch.as_tensor(x, device=dev), order=order, scale_exp=40, factor=0.5, skipped=sk)
        res = out.cpu().numpy().copy(), tuple(fft.local_slice(False)), int(sk.cpu()[0])
        fft.destroy()
        return res
    for order in (2, 4):
        whole = run(comm.COMM_SELF, order)[0]
        acc, _, _, _, _ = S.spread_int(q, x, _inv_dx(shape), order, shape, (0, 0, 0), shape, 40, exact=False)
        assert np.array_equal(whole, S.finish(acc, 0.5 / 2.0 ** 40, np.float64))
        seen = np.zeros(shape, dtype=int)
        for out, sl, sk in cases.run_ranks(nranks, lambda cm: run(cm, order)):
            assert sk == SKIPPED and np.array_equal(out, whole[(slice(None),) + sl])
            seen[sl] += 1
        assert (seen == 1).all()


def test_spread_replays_from_a_captured_graph():
    """scale_exp=, acc= and out= under torch.cuda.graph after one warm-up call on a side stream: the replay follows new positions
    and values and equals an eager call bit for bit; acc is left cleared for the next replay"""
    from mpi4py_fft_amd import comm
    shape, P, e = BLOCKS['small'], 300, 40
    fft, ops = _ops(comm.COMM_SELF, shape, 'd')
    first, second = _particles(shape, P, m=3, seed=90), _particles(shape, P, m=3, seed=91)
    tq, tx = torch.as_tensor(first[0], device=DEV), torch.as_tensor(first[1], device=DEV)
    out2, out4 = (torch.zeros((3,) + shape, dtype=torch.float64, device=DEV) for _ in range(2))
    acc = torch.zeros((3,) + shape, dtype=torch.int64, device=DEV)
    skipped = torch.zeros(1, dtype=torch.int64, device=DEV)

    def enqueue():
        assert ops.spread(tq, tx, order=2, out=out2, scale_exp=e, acc=acc, skipped=skipped) is out2
        assert ops.spread(tq, tx, order=4, out=out4, scale_exp=e, factor=0.5, acc=acc, skipped=skipped) is out4
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        enqueue()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    seen = []
    for q, x in (first, second):
        tq.copy_(torch.as_tensor(q))
        tx.copy_(torch.as_tensor(x))
        out2.fill_(-1)
        out4.fill_(-1)
        skipped.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert not acc.any() and int(skipped.cpu()[0]) == 2 * SKIPPED
        eager2 = ops.spread(tq, tx, order=2, scale_exp=e)
        eager4 = ops.spread(tq, tx, order=4, scale_exp=e, factor=0.5)
        assert torch.equal(out2, eager2) and torch.equal(out4, eager4)
        a4, _, _, _, _ = S.spread_int(q, x, _inv_dx(shape), 4, shape, (0, 0, 0), shape, e, exact=False)
        assert np.array_equal(out4.cpu().numpy(), S.finish(a4, 0.5 / 2.0 ** e, np.float64))
        seen.append(out4.cpu().numpy().copy())
    assert not np.array_equal(seen[0], seen[1])
    fft.destroy()
