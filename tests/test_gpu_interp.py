"""gfft_ps_scale_axes and gfft_ps_interp on the device against tests/interp_ref.py, the thread-rank reduction of
`SpectralOps.interpolate`, the whole chain forward / prefilter / backward / interpolate against an analytic field, a captured
call, and the tracers of examples/dns_taylor_green.py.

gfft_ps_scale_axes is compared for EQUALITY (equal_nan): every value is one multiply by a g that is at most two.
gfft_ps_interp is compared with the long-double reference: |got - ref| <= (order^3 + 64) 2^-53 M_p per entry, M_p = sum |w0 w1 w2 c|,
in both field precisions (the fields hold values that float32 represents, so one reference serves both).

Launch geometry the cases are chosen against (csrc/spectral.hip): workgroups of 256 lanes, at most 16384 of them, grid-stride.
  scale_axes: a lane takes 16 bytes -- one mode in fp64, two in fp32 where n2 is even and both bases are 16-byte aligned, else
  one.  (8, 6, 11) has an odd n2 and (5, 3, 4) an even one; 'misaligned' starts one element into its allocation; the sweep
  shapes exceed 16384 * 256 lanes (4 194 304 modes in fp64, twice that in fp32), so lanes take a second step.
  interp: order^2 lanes per particle, so 16 (order 4) or 64 (order 2) particles per workgroup and 262 144 or 1 048 576 per sweep
  of the grid.  P = 1: one group, the rest of the workgroup idle; 63 / 64 / 65: the last workgroup part-filled, full, one
  particle in the next (order 2); 1000: many workgroups with a part-filled last one (both orders); 262 147 and 1 048 579: every
  group takes a second particle.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, interp_ref as I, spectrum_ref as R

DEV = 'cuda'
TORCH = {'d': torch.float64, 'f': torch.float32}
CTORCH = {'d': torch.complex128, 'f': torch.complex64}
CNP = {'d': np.complex128, 'f': np.complex64}
BLOCKS = {'small': (8, 6, 20), 'odd': (5, 3, 7), 'narrow': (3, 2, 5)}          # narrow: the order-4 stencil is wider than two axes
SWEEP = {2: 1048576 + 3, 4: 262144 + 3}
_REF = {}
WORST = {}


def _device(a, dtype, misaligned=False):
    flat = torch.as_tensor(np.array(a).reshape(-1)).to(dtype)          # (a copy: the cached cases are read-only)
    buf = torch.empty(flat.numel() + 1, dtype=dtype, device=DEV)
    t = buf[1:] if misaligned else buf[:-1]
    t.copy_(flat)
    assert (t.data_ptr() % 16 != 0) == (misaligned and flat.element_size() < 16)          # (a complex128 element keeps 16 bytes)
    return t


# ---- gfft_ps_scale_axes ------------------------------------------------------------------------------------------------

def _spectral_case(shape, dt, seed=31):
    """(f [4] + shape complex, v three real vectors) in the precision under test with -0.0, inf and NaN planted in both;
    computed once per case, never modified"""
    key = ('sa', shape, dt)
    if key not in _REF:
        rng = np.random.default_rng(seed)
        rdt = np.float64 if dt == 'd' else np.float32
        f = (rng.standard_normal((4,) + shape) + 1j * rng.standard_normal((4,) + shape)).astype(CNP[dt])
        v = [rng.standard_normal(n).astype(rdt) for n in shape]
        flat = f.reshape(4, -1)
        for c in range(4):
            flat[c, 3 + c] = complex(-0.0, 0.0)
            flat[c, 7 + c] = complex(np.inf, -1.0)
            flat[c, 12 + c] = complex(1.0, np.nan)
            flat[c, 17 + c] = complex(-np.inf, -0.0)
        v[0][1], v[1][2], v[2][1], v[2][3] = -0.0, np.inf, np.nan, 0.0
        f.setflags(write=False)
        _REF[key] = (f, v)
    return _REF[key]


def _scale(tf, tout, m, tv, shape, dt):
    from mpi4py_fft_amd import _lib
    _lib.engine().ps_scale_axes(tf, tout, m, tv, shape, 8 if dt == 'd' else 4)


def _same(got, want, dt):
    rdt = np.float64 if dt == 'd' else np.float32
    g, w = got.view(rdt), want.view(rdt)
    return np.array_equal(g, w, equal_nan=True) and np.array_equal(np.signbit(g[~np.isnan(w)]), np.signbit(w[~np.isnan(w)]))


@pytest.mark.parametrize('m', [1, 2, 3, 4])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', ['odd n2', 'even n2', 'misaligned'])
def test_scale_axes_against_reference(kind, dt, m):
    """Bit for bit the numpy restatement (the sign of a zero included), out of place and in place, with each vector None in
    turn, all three and none; the input of an out-of-place call is untouched."""
    shape = (5, 3, 4) if kind == 'even n2' else (8, 6, 11)
    f, v = _spectral_case(shape, dt)
    tv = [_device(vi, TORCH[dt]) for vi in v]
    n = int(np.prod(shape))
    for drop in (None, 0, 1, 2, 'all'):
        keep = [drop != 'all' and a != drop for a in range(3)]
        want = I.scale_axes(f[:m], [v[a] if keep[a] else None for a in range(3)])
        vv = tuple(tv[a] if keep[a] else None for a in range(3))
        src = _device(f[:m], CTORCH[dt], kind == 'misaligned')
        out = torch.full((m * n + 1,), -7.0, dtype=CTORCH[dt], device=DEV)[1 if kind == 'misaligned' else 0:][:m * n]
        _scale(src, out, m, vv, shape, dt)
        assert _same(out.cpu().numpy().reshape(want.shape), want, dt), (kind, dt, m, drop)
        assert _same(src.cpu().numpy().reshape(want.shape), f[:m], dt), 'an out-of-place call changed its input'
        _scale(src, src, m, vv, shape, dt)                             # in place
        assert _same(src.cpu().numpy().reshape(want.shape), want, dt), (kind, dt, m, drop, 'in place')


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_scale_axes_past_one_sweep(dt):
    shape = (128, 128, 258) if dt == 'd' else (128, 256, 258)
    assert int(np.prod(shape)) // (1 if dt == 'd' else 2) > 16384 * 256
    rng = np.random.default_rng(32)
    rdt = np.float64 if dt == 'd' else np.float32
    f = rng.standard_normal((1,) + shape + (2,), dtype=rdt).view(CNP[dt])[..., 0]
    v = [rng.standard_normal(n).astype(rdt) for n in shape]
    t = torch.as_tensor(f).to(DEV)
    assert t.data_ptr() % 16 == 0
    _scale(t, t, 1, tuple(torch.as_tensor(vi).to(DEV) for vi in v), shape, dt)
    assert _same(t.cpu().numpy(), I.scale_axes(f, v), dt)


# ---- gfft_ps_interp ----------------------------------------------------------------------------------------------------

def _inv_dx(N):
    return [n / l for n, l in zip(N, R.BOX)]


def _positions(N, P, seed=41):
    """[P][3] doubles over five box lengths with, from P = 63 on, the edge positions planted in rows 5 ... 21; the rows that must
    come back as NaN are 15 ... 18"""
    L = np.asarray(R.BOX)
    x = np.random.default_rng(seed).uniform(-2.0, 3.0, (P, 3)) * L
    if P >= 63:
        dx = L / np.asarray(N)
        below = np.nextafter(0.0, -1.0)
        x[5:22] = [[0, 0, 0], L, [below, 0, 0], [below, below, below], 2 * dx, [1 * dx[0], 0, (N[2] - 1) * dx[2]], -3 * dx,
                   [-0.3 * L[0], -1.7 * L[1], -0.01 * L[2]], 1000 * L + 0.37, -1000 * L - 0.37,
                   [np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1e300, 1, 1], [0.5, 0.25, 0.125], [-1e-300, 1e-300, -1e-17], [L[0], 0, L[2]]]
    return x


def _case(block, P, order):
    """(c [4] + block as float32-representable doubles, x, reference [P][4], M [P][4]): the whole periodic grid = the block;
    computed once, never modified"""
    key = ('ip', block, P, order)
    if key not in _REF:
        N = BLOCKS[block]
        c = np.random.default_rng(42).standard_normal((4,) + N).astype(np.float32).astype(np.float64)
        x = _positions(N, P)
        ref, M = I.interp(c, x, _inv_dx(N), order)
        for a in (c, x, ref, M):
            a.setflags(write=False)
        _REF[key] = (c, x, ref, M)
    return _REF[key]


def _interp(tc, m, n, start, N, tx, P, order, dt):
    """gfft_ps_interp straight through the engine, into an array prefilled with garbage"""
    from mpi4py_fft_amd import _lib
    out = torch.full((P, m), -7.0, dtype=torch.float64, device=DEV)
    _lib.engine().ps_interp(tc, m, n, start, N, _inv_dx(N), tx, P, order, out, 8 if dt == 'd' else 4)
    return out


def _within(got, ref, M, order, extra=0, what=''):
    """NaN rows where the reference has them and nowhere else; every other entry inside the bound; returns the worst fraction"""
    bad = np.isnan(np.asarray(ref, dtype=np.float64))
    assert np.array_equal(np.isnan(got), bad), (what, np.argwhere(np.isnan(got) != bad)[:8].tolist())
    err = np.abs(got.astype(np.longdouble) - ref)[~bad]
    lim = I.bound(M, order, extra)[~bad]
    frac = float((err / np.maximum(lim, 5e-324)).max()) if err.size else 0.0
    print('%s: worst fraction of the bound %.3f' % (what, frac))
    WORST[what] = frac
    assert np.all(err <= lim), (what, frac)
    return frac


@pytest.mark.parametrize('m', [1, 2, 3, 4])
@pytest.mark.parametrize('order', [2, 4])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('block', ['small', 'odd', 'narrow'])
def test_interp_against_reference(block, dt, order, m):
    """Every entry inside the bound for P = 1, 63, 64, 65 and 1000, the field and the positions each one element into their
    allocations, garbage in d_out overwritten, the planted rows NaN and their neighbours not, a second call identical."""
    N = BLOCKS[block]
    for P in (1, 63, 64, 65, 1000):
        c, x, ref, M = _case(block, P, order)
        tc = _device(c[:m], TORCH[dt], misaligned=True)
        tx = _device(x, torch.float64, misaligned=True).view(P, 3)
        out = _interp(tc, m, N, (0, 0, 0), N, tx, P, order, dt)
        got = out.cpu().numpy()
        _within(got, ref[:, :m], M[:, :m], order, what='%s %s order %d m %d P %d' % (block, dt, order, m, P))
        if P >= 63:
            assert np.isnan(got[15:19]).all() and not np.isnan(got[:15]).any() and not np.isnan(got[19:]).any()
        assert np.array_equal(_interp(tc, m, N, (0, 0, 0), N, tx, P, order, dt).cpu().numpy(), got, equal_nan=True), 'the result does not repeat'


@pytest.mark.parametrize('order', [2, 4])
@pytest.mark.parametrize('dt', ['d', 'f'])
def test_interp_past_one_sweep(dt, order):
    """More particles than one sweep of the grid holds, on the small odd block: every group takes a second particle"""
    N, P, m = BLOCKS['odd'], SWEEP[order], 2
    assert P * order * order > 16384 * 256
    c, x, ref, M = _case('odd', P, order)
    tc, tx = _device(c[:m], TORCH[dt]), _device(x, torch.float64).view(P, 3)
    got = _interp(tc, m, N, (0, 0, 0), N, tx, P, order, dt).cpu().numpy()
    _within(got, ref[:, :m], M[:, :m], order, what='sweep %s order %d' % (dt, order))


@pytest.mark.parametrize('order', [2, 4])
def test_a_nan_in_the_field_reaches_its_stencils_only(order):
    N, P, m = BLOCKS['small'], 1000, 3
    c, x, _, _ = _case('small', P, order)
    c = c[:m].copy()
    c[1, 3, 2, 5] = np.nan
    ref, M = I.interp(c, x, _inv_dx(N), order)
    got = _interp(_device(c, torch.float64), m, N, (0, 0, 0), N, _device(x, torch.float64).view(P, 3), P, order, 'd').cpu().numpy()
    hit = np.isnan(np.asarray(ref[:, 1], dtype=np.float64))
    assert 0 < hit.sum() - 4 < P // 2                                   # (four rows are NaN for their positions)
    assert np.array_equal(np.isnan(got), np.isnan(np.asarray(ref, dtype=np.float64)))
    keep = ~np.isnan(np.asarray(ref, dtype=np.float64))
    assert np.all(np.abs(got.astype(np.longdouble) - ref)[keep] <= I.bound(M, order)[keep])


@pytest.mark.parametrize('order', [2, 4])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('pieces', ['slab2', 'pencil4'])
def test_blocks_of_a_whole(pieces, dt, order):
    """(8, 6, 20) cut into two slabs and into 2 x 2 pencils: each piece's share meets the bound against the reference's share for
    that start / n, and the shares added in rank order meet (order^3 + 64 + pieces) 2^-53 M_p against the whole"""
    N, P, m = BLOCKS['small'], 1000, 3
    c, x, whole, M = _case('small', P, order)
    blocks = [((a, 0, 0), (4, 6, 20)) for a in (0, 4)] if pieces == 'slab2' else [((a, b, 0), (4, 3, 20)) for a in (0, 4) for b in (0, 3)]
    tx = _device(x, torch.float64).view(P, 3)
    total = None
    for start, n in blocks:
        piece = c[(slice(0, m),) + tuple(slice(s, s + k) for s, k in zip(start, n))]
        ref, Mp = I.interp(piece, x, _inv_dx(N), order, N=N, start=start)
        got = _interp(_device(piece, TORCH[dt]), m, n, start, N, tx, P, order, dt).cpu().numpy()
        _within(got, ref, Mp, order, what='%s %s order %d piece %s' % (pieces, dt, order, start))
        total = got if total is None else total + got
    _within(total, whole[:, :m], M[:, :m], order, extra=len(blocks), what='%s %s order %d summed' % (pieces, dt, order))


def _ops(comm, shape, dt, **kw):
    from mpi4py_fft_amd import PFFT, spectral
    fft = PFFT(comm, shape, dtype=dt, **kw)
    return fft, spectral.SpectralOps(fft, R.BOX)


@pytest.mark.parametrize('nranks,grid', [(2, [2, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'pencil4'])
def test_thread_ranks(nranks, grid):
    """Every rank holds identical bits, inside the bound widened by the number of ranks"""
    from mpi4py_fft_amd import newDistArray
    shape, P = (24, 16, 20), 500
    c = np.random.default_rng(43).standard_normal((3,) + shape)
    x = _positions(shape, P, seed=44)
    for order in (2, 4):
        ref, M = I.interp(c, x, _inv_dx(shape), order)

        def run(cm):
            fft, ops = _ops(cm, shape, 'd', grid=grid)
            U = newDistArray(fft, False, rank=1)
            U[...] = c[(slice(None),) + fft.local_slice(False)]
            got = ops.interpolate(U, torch.as_tensor(x, device=U.tensor.device), order=order)
            fft.destroy()
            return got
        res = cases.run_ranks(nranks, run)
        for got in res:
            assert isinstance(got, np.ndarray) and got.shape == (P, 3) and np.array_equal(got, res[0], equal_nan=True)
        _within(res[0], ref, M, order, extra=nranks, what='%d thread ranks order %d' % (nranks, order))


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_end_to_end_against_the_analytic_field(dt):
    """forward, scale_axes(bspline_vectors(4)), backward, interpolate at the 400 points of the table at 32^3: the error against
    the analytic values is the reference's own plus the suite's contract level (1e-10 / 1e-4 of max |f|); at grid points the
    interpolant returns the field to that level; the same for order 2 without a prefilter"""
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    N = 32
    tol = 1e-10 if dt == 'd' else 1e-4
    fft = PFFT(comm.COMM_SELF, (N, N, N), dtype=dt)
    ops = spectral.SpectralOps(fft)                                    # the box [0, 2 pi)^3
    f = I.grid_samples(N)
    fmax = np.abs(f).max()
    x = I.convergence_points()
    exact = I.smooth_field(x[:, 0], x[:, 1], x[:, 2])
    cells = np.random.default_rng(45).integers(-2 * N, 3 * N, (300, 3))
    xg = cells * (2 * np.pi / N)
    at_cells = f[cells[:, 0] % N, cells[:, 1] % N, cells[:, 2] % N]
    u, c = newDistArray(fft, False), newDistArray(fft, False)
    u_hat = newDistArray(fft, True)
    u[...] = f
    tx, txg = torch.as_tensor(x, device=DEV), torch.as_tensor(xg, device=DEV)
    for order in (2, 4):
        own, _ = I.interp(I.coefficients(f, order)[None], x, [N / (2 * np.pi)] * 3, order)
        own = float(np.abs(own[:, 0] - exact).max())
        if order == 4:
            fft.forward(u, u_hat)
            assert ops.scale_axes(u_hat, ops.bspline_vectors(4)) is u_hat
            fft.backward(u_hat, c)
            u[...] = f                                                 # (a real backward transform may use its input)
        field = c if order == 4 else u
        got = ops.interpolate(field, tx, order=order)
        assert got.shape == (400,)
        err = float(np.abs(got - exact).max())
        print('end to end %s order %d: error %.3e, the reference\'s own %.3e' % (dt, order, err, own))
        assert err <= own + tol * fmax, (order, err, own)
        at_grid = ops.interpolate(field, txg, order=order)
        assert np.abs(at_grid - at_cells).max() <= tol * fmax, (order, np.abs(at_grid - at_cells).max())
    fft.destroy()


def test_interpolate_replays_from_a_captured_graph():
    """out= with reduce=False under torch.cuda.graph after one warm-up call on a side stream: the replay follows new positions"""
    from mpi4py_fft_amd import comm, newDistArray
    shape, P = BLOCKS['small'], 300
    fft, ops = _ops(comm.COMM_SELF, shape, 'd')
    c = np.random.default_rng(46).standard_normal((3,) + shape)
    U = newDistArray(fft, False, rank=1)
    U[...] = c
    first, second = _positions(shape, P, seed=47), _positions(shape, P, seed=48)
    tx = torch.as_tensor(first, device=DEV)
    out2, out4 = (torch.zeros((P, 3), dtype=torch.float64, device=DEV) for _ in range(2))

    def enqueue():
        assert ops.interpolate(U, tx, order=2, out=out2, reduce=False) is out2
        assert ops.interpolate(U, tx, order=4, out=out4, reduce=False) is out4
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        enqueue()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    seen = []
    for pos in (first, second):
        tx.copy_(torch.as_tensor(pos))
        out2.fill_(-1)
        out4.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        for order, out in ((2, out2), (4, out4)):
            ref, M = I.interp(c, pos, _inv_dx(shape), order)
            _within(out.cpu().numpy(), ref, M, order, what='replay order %d' % order)
        seen.append(out4.cpu().numpy().copy())
    assert not np.array_equal(seen[0], seen[1], equal_nan=True)
    fft.destroy()


# ---- the example -------------------------------------------------------------------------------------------------------

def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_interp', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('order', [4, 2])
def test_example_tracers(order):
    """solve(particles=(64, order, 7)) at its smallest size: one rank and two thread ranks agree to 1e-12 of the box, the fused
    path and the torch index expressions to 1e-10, the energy is that of the run without particles, and on one rank the graph
    replay gives the eager positions bit for bit"""
    from mpi4py_fft_amd import comm
    ex = _example()
    box = 4 * np.pi
    kw = dict(M=4, nsteps=2, particles=(64, order, 7))
    one, base = {}, {}
    e = ex.solve(comm.COMM_SELF, stats=one, **kw)
    assert e == ex.solve(comm.COMM_SELF, M=4, nsteps=2, stats=base) and base == {}
    xp, vp = one['particles'], one['particle_velocity']
    assert set(one) == {'particles', 'particle_velocity'} and xp.shape == vp.shape == (64, 3) and xp.dtype == np.float64
    start = np.random.default_rng(7).uniform(0.0, 1.0, (64, 3)) * np.array([2 * np.pi, 4 * np.pi, 4 * np.pi])
    moved = np.abs(xp - start).max()
    assert 1e-3 < moved < 0.05 and np.abs(vp).max() <= 1.01       # |u| <= 1 in the vortex (the interpolant may overshoot by its error); two steps of 0.01

    def body(c):
        st = {}
        return ex.solve(c, stats=st, **kw), st
    res = cases.run_ranks(2, body)
    for e2, st in res:
        assert abs(e2 - e) <= 1e-12 and np.abs(st['particles'] - xp).max() <= 1e-12 * box
        assert np.array_equal(st['particles'], res[0][1]['particles'])
    unfused = {}
    eu = ex.solve(comm.COMM_SELF, stats=unfused, fused=False, **kw)
    assert abs(eu - e) <= 1e-10 and np.abs(unfused['particles'] - xp).max() <= 1e-10
    assert np.abs(unfused['particle_velocity'] - vp).max() <= 1e-10
    graph = {}
    eg = ex.solve(comm.COMM_SELF, stats=graph, graph=True, **kw)
    assert abs(eg - e) <= 1e-12 and np.array_equal(graph['particles'], xp)


def test_example_particle_check():
    """PARTICLE_CHECK: the sum of all final coordinates of solve(particles=(1000, 4, 7), dealias='2/3'), M = 6, 10 steps; the
    dealiased energy is unchanged by the tracers"""
    from mpi4py_fft_amd import comm
    ex = _example()
    st = {}
    e = ex.solve(comm.COMM_SELF, particles=(1000, 4, 7), dealias='2/3', stats=st)
    total = float(st['particles'].sum())
    print('PARTICLE_CHECK measured: %.15f' % total)
    assert abs(e - ex.DEALIASED_ENERGY) <= 1e-9
    assert ex.PARTICLE_CHECK is not None and abs(total - ex.PARTICLE_CHECK) <= 1e-9 * abs(ex.PARTICLE_CHECK), (total, ex.PARTICLE_CHECK)
