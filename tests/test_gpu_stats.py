"""gfft_ps_stats / gfft_ps_timestep / gfft_ps_rk_stage_dt on the device against tests/stats_ref.py (numpy, fsum, int64).

Bounds (derived in stats_ref.py, not measured): sums within (count + 4) 2^-53 sum |term| of the fsum reference -- true of
any summation order --, maxima and minima exact, entries 0 and 1 within 4 2^-53 relative (FMA contraction is allowed).
Integer-valued fields must come out EXACTLY: every sum is an integer below 2^53, so no order can round.

Launch geometry the shapes are chosen against (csrc/spectral.hip): workgroups of 256 lanes, V points per lane and load
(16 bytes: V = 2 in fp64, 4 in fp32, where count % V == 0 and the base is 16-byte aligned; else V = 1), each workgroup
owning one contiguous chunk of whole steps of 256 V points, at most 2048 workgroups.  So a workgroup takes a SECOND step
only beyond 2048 * 256 * V points = 1 048 576 (fp64) / 2 097 152 (fp32): (96, 100, 112) and (128, 100, 168) are the
spectrum suite's shapes just past that.  9 * 5 * 12 + 1 = 541 points is odd (V = 1, three workgroups of one step, the
last one ragged); a tensor sliced one element in is not 16-byte aligned (V = 1 with an even count).  The 26 values of a
four-component field reduce over 64 lanes, 4 waves and, in the second kernel, over the workgroups 256 at a time.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, stats_ref as R

BOX = (2 * np.pi, 4 * np.pi, 2 * np.pi)
WIDE = {'d': 2, 'f': 4}
SWEEP = {'d': 2048 * 256 * 2, 'f': 2048 * 256 * 4}
SWEEP_SHAPE = {'d': (96, 100, 112), 'f': (128, 100, 168)}
INV = {1: [0.5], 2: [2.0, 0.0], 3: [1.0, 2.0, 0.5], 4: [0.0, 1.0, 2.0, 0.5]}
TDT = {'d': torch.float64, 'f': torch.float32}


def _geometry(count, dt, aligned=True):
    """(V, chunk, workgroups) of a launch, restated from the kernel's comment"""
    V = WIDE[dt] if (count % WIDE[dt] == 0 and aligned) else 1
    step = 256 * V
    chunk = -(-count // 2048)
    chunk = -(-chunk // step) * step
    return V, chunk, -(-count // chunk) if count else 0


def _run(t, m, count, inv, dt):
    """gfft_ps_stats straight through the engine on a flat device tensor"""
    from mpi4py_fft_amd import _lib
    out = torch.full((R.nval(m),), -7.0, dtype=torch.float64, device='cuda')
    _lib.engine().ps_stats(t, m, count, inv, out, 8 if dt == 'd' else 4)
    return out.cpu().numpy()


def _device(G, dt, misaligned=False):
    """G ([m][count] host array) as a flat device tensor; misaligned: its storage starts one element into an allocation"""
    flat = torch.as_tensor(np.ascontiguousarray(G).reshape(-1).astype(dt))
    if not misaligned:
        t = flat.cuda()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(flat.numel() + 1, dtype=flat.dtype, device='cuda')
    t = buf[1:]
    t.copy_(flat)
    assert t.data_ptr() % 16 != 0
    return t


KINDS = {'small': 24 * 16 * 20, 'odd': 9 * 5 * 12 + 1, 'misaligned': 24 * 16 * 20}
EXACT = [(k, dt, m) for dt in 'df' for m in (1, 2, 3, 4) for k in ('small', 'odd', 'misaligned', 'sweep')
         if not (m == 2 and k in ('misaligned', 'sweep'))]


@pytest.mark.parametrize('kind,dt,m', EXACT, ids=lambda v: str(v))
def test_integer_fields_are_exact(kind, dt, m):
    count = int(np.prod(SWEEP_SHAPE[dt])) if kind == 'sweep' else KINDS[kind]
    V, chunk, nwg = _geometry(count, dt, kind != 'misaligned')
    if kind == 'sweep':
        assert count > SWEEP[dt] and V == WIDE[dt] and chunk == 2 * 256 * V, 'the shape no longer exceeds one sweep of the launch'
    else:
        assert V == (WIDE[dt] if kind == 'small' else 1) and nwg > 1
    G = np.random.default_rng(21 + m).integers(-3, 4, size=(m, count))
    want = R.reference_int(G, INV[m])
    got = _run(_device(G, dt, kind == 'misaligned'), m, count, INV[m], dt)
    assert np.array_equal(got, want), (kind, dt, m, got, want)


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_empty_block_writes_the_identities(dt):
    t = torch.zeros(4, dtype=TDT[dt], device='cuda')
    got = _run(t, 3, 0, INV[3], dt)
    assert np.array_equal(got, [0, 0] + [-np.inf, np.inf, 0, 0, 0, 0] * 3)


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_impulses(dt):
    """One 3.0 in a field of zeros: sums exactly 3, 9, 27, 81, extrema exact, every other component untouched -- a point
    counted twice or not at all at a boundary of the launch shows undiluted."""
    m, count = 3, 24 * 16 * 20
    V, chunk, nwg = _geometry(count, dt)
    assert V == WIDE[dt] and nwg >= 2 and chunk < count
    t = torch.zeros(m * count, dtype=TDT[dt], device='cuda')
    places = {'first': (0, 0), 'last': (0, count - 1), 'end of workgroup 0': (0, chunk - 1), 'start of workgroup 1': (0, chunk),
              'second of a V group': (1, 257 * V + 1), 'last component, last point': (m - 1, count - 1),
              'last component': (m - 1, 5)}
    for name, (c, pos) in places.items():
        t[c * count + pos] = 3.0
        got = _run(t, m, count, INV[m], dt)
        t[c * count + pos] = 0.0
        want = np.zeros(R.nval(m))
        want[0], want[1] = 3.0 * INV[m][c], 9.0
        want[2 + 6 * c: 8 + 6 * c] = [3, 0, 3, 9, 27, 81]
        assert np.array_equal(got, want), (name, dt, got, want)
    t[count + 7] = -3.0                              # and a negative one: the minimum, odd powers signed
    got = _run(t, m, count, INV[m], dt)
    want = np.zeros(R.nval(m))
    want[0], want[1] = 3.0 * INV[m][1], 9.0
    want[8:14] = [0, -3, -3, 9, -27, 81]
    assert np.array_equal(got, want), (dt, got, want)


_REF = {}


def _random(kind, dt, m):
    """(field [m][count] in the precision under test, reference, magnitudes) -- computed once per case, never modified"""
    key = (kind, dt, m)
    if key not in _REF:
        count = int(np.prod(SWEEP_SHAPE[dt])) if kind == 'sweep' else KINDS[kind]
        G = np.random.default_rng(31).standard_normal((m, count)).astype(dt)
        ref, mag = R.reference(G, INV[m])
        for a in (G, ref, mag):
            a.setflags(write=False)
        _REF[key] = (G, ref, mag)
    return _REF[key]


RANDOM = [('small', 'd', 3), ('small', 'f', 3), ('odd', 'd', 4), ('odd', 'f', 4), ('misaligned', 'd', 1), ('misaligned', 'f', 3),
          ('sweep', 'd', 1), ('sweep', 'f', 1)]


@pytest.mark.parametrize('kind,dt,m', RANDOM, ids=lambda v: str(v))
def test_random_fields_and_repeatability(kind, dt, m):
    """Within the any-order bound of the fsum reference, and two calls give identical bits."""
    G, ref, mag = _random(kind, dt, m)
    count = G.shape[1]
    t = _device(G, dt, kind == 'misaligned')
    got = _run(t, m, count, INV[m], dt)
    R.assert_stats(got, ref, mag, count, (kind, dt, m))
    again = _run(t, m, count, INV[m], dt)
    assert np.array_equal(got, again), 'the result does not repeat bit for bit'


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_nan_shows_in_the_sums_of_its_component_only(dt):
    G0, _, _ = _random('small', dt, 3)
    G = np.array(G0)
    count = G.shape[1]
    G[1, 4321] = np.nan
    ref, mag = R.reference(G, INV[3])
    assert np.isnan(ref[8 + 2: 8 + 6]).all() and np.isfinite(np.delete(ref, range(10, 14))).all()
    got = _run(_device(G, dt), 3, count, INV[3], dt)
    assert np.isnan(got[10:14]).all(), got
    assert np.isfinite(np.delete(got, range(10, 14))).all(), got
    R.assert_stats(got, ref, mag, count, ('nan', dt))          # the other components, the extrema, [0] and [1]: unchanged


def _ops(comm, shape, dt, **kw):
    from mpi4py_fft_amd import PFFT, spectral
    fft = PFFT(comm, shape, dtype=dt, **kw)
    return fft, spectral.SpectralOps(fft, BOX)


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', [(24, 16, 20), (12, 10, 21)])
def test_parseval(shape, dt):
    """sum_c S2_c / (2 Npoints) in physical space = `energy(u_hat)` of the forward transform, to the transform's rounding:
    the suite's rounding-level bound (2 eps log2 N per transform, tests/cases.py) with head-room for three components."""
    from mpi4py_fft_amd import comm, newDistArray
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    u, uh = newDistArray(fft, False, rank=1), newDistArray(fft, rank=1)
    u[...] = np.random.default_rng(5).standard_normal((3,) + shape).astype(dt)
    st = ops.stats(u)
    n = int(np.prod(shape))
    want = float(sum(st[2 + 6 * c + 3] for c in range(3))) / (2.0 * n)
    for c in range(3):
        fft.forward(u[c], uh[c])
    got = ops.energy(uh)
    tol = 64 * cases.EPS[dt] * np.log2(n)
    print('parseval %s %s: rel err %.3e (tol %.3e)' % (shape, dt, abs(got - want) / want, tol))
    assert abs(got - want) <= tol * want
    # and the object's default inv_dx is N_i / L_i
    assert ops.inv_dx == [s / l for s, l in zip(shape, BOX)]
    fft.destroy()


@pytest.mark.parametrize('P,grid', [(2, [2, 1, 1]), (4, [4, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'slab4', 'pencil4'])
@pytest.mark.parametrize('shape,dt', [((24, 16, 20), 'd'), ((12, 10, 21), 'f')])
def test_thread_ranks(P, grid, shape, dt):
    """Every rank holds the same reduced statistics bit for bit; extrema equal the one-rank result, sums obey the bound."""
    from mpi4py_fft_amd import comm, newDistArray
    G = np.random.default_rng(41).standard_normal((3,) + shape).astype(dt)
    inv = [s / l for s, l in zip(shape, BOX)]
    ref, mag = R.reference(G, inv)
    count = int(np.prod(shape))

    def body(c):
        fft, ops = _ops(c, shape, dt, grid=grid)
        u = newDistArray(fft, False, rank=1)
        u[...] = G[(slice(None),) + fft.local_slice(False)]
        got = ops.stats(u)
        rate = ops.cfl_rate(u)
        fft.destroy()
        return got, rate
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    u = newDistArray(fft, False, rank=1)
    u[...] = G
    one = ops.stats(u)
    fft.destroy()
    R.assert_stats(one, ref, mag, count, 'one rank')
    res = cases.run_ranks(P, body)
    ext = [2 + 6 * c + j for c in range(3) for j in (0, 1)]
    for got, rate in res:
        assert np.array_equal(got, res[0][0]), 'ranks disagree'
        assert np.array_equal(got[ext], one[ext]), (P, grid, 'extrema vs one rank')
        R.assert_stats(got, ref, mag, count, (P, grid))
        assert rate == got[0]


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('with_u', [True, False])
def test_rk_stage_with_a_device_dt_is_bit_identical(dt, with_u):
    """rk_stage(dt=) multiplies cb dt and ca dt on the device; the host path gets the products: the same bits.  1001 reals
    and 333 complex values: neither is a multiple of the 256-lane workgroup."""
    from mpi4py_fft_amd import asdevice, spectral
    rng = np.random.default_rng(8)
    h = 0.012345678901234567
    hdev = torch.tensor([h, 123.0], dtype=torch.float64, device='cuda')
    cb, ca = 0.5, 1.0 / 6.0
    for cplx in (False, True):
        n = 333 if cplx else 1001
        def arr():
            a = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
            return a.astype(dt.upper() if cplx else dt)
        u0, du, acc = asdevice(arr()), asdevice(arr()), arr()
        ua, ub = asdevice(np.zeros_like(acc)), asdevice(np.zeros_like(acc))
        u1a, u1b = asdevice(acc), asdevice(acc)
        spectral.rk_stage(ua if with_u else None, u0 if with_u else None, u1a, du, cb * h, ca * h)
        spectral.rk_stage(ub if with_u else None, u0 if with_u else None, u1b, du, cb, ca, dt=hdev)
        torch.cuda.synchronize()
        assert np.array_equal(np.asarray(u1a), np.asarray(u1b)) and np.array_equal(np.asarray(ua), np.asarray(ub))
        assert not np.array_equal(np.asarray(u1a), acc) and (bool(np.abs(np.asarray(ua)).sum() > 0) == with_u)
        assert hdev.cpu().tolist() == [h, 123.0]                    # read only


def test_timestep_on_the_device_equals_the_host_formula():
    from mpi4py_fft_amd import comm, newDistArray
    shape = (24, 16, 20)
    fft, ops = _ops(comm.COMM_SELF, shape, 'd')
    u = newDistArray(fft, False, rank=1)
    u[...] = np.random.default_rng(13).standard_normal((3,) + shape)
    rate = ops.cfl_rate(u)
    assert rate > 0
    free = 0.7 / rate
    dt = torch.zeros(2, dtype=torch.float64, device='cuda')
    steps = []
    # (cfl, dt_max, dt_min): unclamped, clamped from above, clamped from below
    for cfl, hi, lo in ((0.7, 4 * free, 0.0), (0.7, free / 3, 0.0), (0.7, 100 * free, 10 * free)):
        assert ops.timestep(u, cfl, hi, lo, out=dt) is dt
        got = dt.cpu().numpy().copy()
        host = ops.timestep(u, cfl, hi, lo)
        assert got[0] == host == R.timestep(rate, cfl, hi, lo), (cfl, hi, lo, got, host)
        steps.append(got[0])
        assert got[1] == sum(steps[1:], steps[0]), 'd_dt[1] is the running time'
    assert steps[0] == free and steps[1] == free / 3 and steps[2] == 10 * free
    # a field at rest: nothing to limit, dt_max
    u[...] = 0
    ops.timestep(u, 0.7, 0.25, out=dt)
    assert float(dt[0]) == 0.25
    fft.destroy()


def test_adaptive_stage_replays_from_a_captured_graph():
    """timestep(out=dt) followed by rk_stage(dt=dt) under torch.cuda.graph: a replay follows the field it finds -- the step
    halves exactly when the field doubles -- and the stage uses that step."""
    from mpi4py_fft_amd import asdevice, comm, newDistArray, spectral
    shape = (24, 16, 20)
    fft, ops = _ops(comm.COMM_SELF, shape, 'd')
    u = newDistArray(fft, False, rank=1)
    rng = np.random.default_rng(17)
    u[...] = rng.standard_normal((3,) + shape)
    w0, dw = (asdevice(rng.standard_normal(1001)) for _ in range(2))
    w, w1 = asdevice(np.zeros(1001)), asdevice(np.zeros(1001))
    dt = torch.zeros(2, dtype=torch.float64, device='cuda')

    def stage():
        ops.timestep(u, 0.5, 1e9, out=dt)
        spectral.rk_stage(w, w0, w1, dw, 0.5, 0.25, dt=dt)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        stage()                                          # warm-up on another stream: scratch and the kept tensor exist now
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        stage()
    first = 0.5 / ops.cfl_rate(u)
    seen = []
    for scale in (1.0, 2.0):
        u.tensor.mul_(scale)
        dt.zero_()
        w1.fill(0.0)
        w.fill(-1.0)
        g.replay()
        torch.cuda.synchronize()
        h = float(dt[0])
        seen.append(h)
        wa, w1a = asdevice(np.zeros(1001)), asdevice(np.zeros(1001))
        spectral.rk_stage(wa, w0, w1a, dw, 0.5 * h, 0.25 * h)
        torch.cuda.synchronize()
        assert torch.equal(w.tensor, wa.tensor) and torch.equal(w1.tensor, w1a.tensor) and float(dt[1]) == h
    assert seen[0] == first and seen[1] == first / 2, (seen, first)
    fft.destroy()


def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_stats', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dns_with_a_cfl_that_never_binds_is_the_fixed_step():
    from mpi4py_fft_amd import comm
    mod = _example()
    fixed = mod.solve(comm.COMM_SELF, M=5, nsteps=4)
    st = {}
    free = mod.solve(comm.COMM_SELF, M=5, nsteps=4, cfl=1e6, stats=st)
    assert st['time'] == 0.01 + 0.01 + 0.01 + 0.01
    assert abs(free - fixed) <= 1e-12, (free, fixed)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_dns_device_dt_equals_host_dt(graph):
    """With a cfl that binds, the step kept in device memory gives the energy of the step computed on the host bit for bit
    (the same arithmetic), also when the whole RK4 step replays from a HIP graph."""
    from mpi4py_fft_amd import comm
    mod = _example()
    sh, sd = {}, {}
    host = mod.solve(comm.COMM_SELF, M=5, nsteps=4, cfl=0.02, stats=sh)
    dev = mod.solve(comm.COMM_SELF, M=5, nsteps=4, cfl=0.02, device_dt=True, graph=graph, stats=sd)
    assert 0 < sh['time'] < 0.9 * 4 * 0.01, ('the cfl does not bind: the case shows nothing', sh)
    assert dev == host and sd['time'] == sh['time'], (dev, host, sd, sh)
