"""gfft_ps_gradient / gfft_ps_gradient_stats on the device against tests/gradient_ref.py (numpy; long double sums), against
themselves (call against call, ranks against one rank, replay against a new field) and end to end against the Betchov identities.

Launch geometry the cases are chosen against (csrc/spectral.hip):
  * gradient: one mode per lane, grid-stride, 256 lanes per workgroup, at most 16384 workgroups.  The spectral blocks of the
    physical shapes (8, 6, 20) and (5, 3, 7) hold 528 and 60 modes: three workgroups with a ragged last one, and a single
    partial wave.  A single field takes two modes per lane and step, a grid stride apart (two workgroups for 528 modes, the
    second mode of a lane absent in the ragged end): 208 x 208 x 197 = 8 523 008 modes > 2 * 16384 * 256, so the first 134 400
    lanes take a second grid-stride step, of one mode.
  * gradient_stats: the geometry of gfft_ps_stats -- V points per lane and load (16 bytes: 2 in fp64, 4 in fp32, where V divides
    count and the base is 16-byte aligned; else 1), each workgroup one contiguous chunk of whole steps of 256 V points, at most
    2048 workgroups.  960 points: two workgroups (fp64) or one (fp32); 105 is odd: V = 1; 960 points one element into an
    allocation: V = 1 with an even count; 34 816: 68 / 34 workgroups; 1 228 800 (fp64) and 2 621 440 (fp32) exceed 2048 * 256 * V, so
    every lane adds a second step of its chunk.

Bound of the statistics (derived in gradient_ref.py, not measured): |got - ref| <= (count + 64) 2^-53 M per entry.
"""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, gradient_ref as G, spectrum_ref as R
from tests.test_gradient_host import residuals

DEV = 'cuda'
TORCH = {'d': torch.float64, 'f': torch.float32}
WIDE = {'d': 2, 'f': 4}


def _ops(comm, shape, dt, **kw):
    from mpi4py_fft_amd import PFFT, spectral
    fft = PFFT(comm, shape, dtype=dt, **kw)
    return fft, spectral.SpectralOps(fft, R.BOX)


def _spectral_block(shape, dt, m, seed):
    """[m] + block random modes in the precision under test with -0.0, +0.0 and NaN parts planted; (field, NaN places)"""
    blk = tuple(shape[:2]) + (shape[2] // 2 + 1,)
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((m,) + blk) + 1j * rng.standard_normal((m,) + blk)).astype(dt.upper())
    flat = f.reshape(m, -1)
    flat[0, 3] = complex(-0.0, 2.5)
    flat[0, 7] = complex(1.5, -0.0)
    flat[m - 1, 11] = complex(0.0, 0.0)
    flat[0, 17] = complex(np.nan, 0.75)                # NaN in the real part: the imaginary parts of the three derivatives
    flat[m - 1, 29] = complex(-1.25, np.nan)
    return f


def _assert_same(got, want, what):
    """Bit for bit, signs of zeros included; a NaN where and only where the reference has one"""
    gr, wr = np.ascontiguousarray(got).view(got.real.dtype), np.ascontiguousarray(want).view(want.real.dtype)
    assert gr.shape == wr.shape and gr.dtype == wr.dtype, (what, gr.shape, wr.shape)
    nan = np.isnan(wr)
    assert np.array_equal(np.isnan(gr), nan), (what, 'a NaN left its mode')
    assert np.array_equal(G.bits(gr)[~nan], G.bits(wr)[~nan]), (what, int((G.bits(gr)[~nan] != G.bits(wr)[~nan]).sum()))


@pytest.mark.parametrize('m', [1, 2, 3, 4])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', [(8, 6, 20), (5, 3, 7)], ids=str)
def test_gradient_bit_for_bit(shape, dt, m):
    from mpi4py_fft_amd import comm
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    k, _ = R.wavenumbers(shape, True)
    f = _spectral_block(shape, dt, m, 61 + m)
    want = G.grad(f, k)
    assert np.isnan(want.view(want.real.dtype)).sum() == 6 and (G.bits(want.view(want.real.dtype)) == G.bits(np.array(-0.0, dtype=dt))).any()
    t = torch.as_tensor(f, device=DEV)
    out = torch.full((m, 3) + ops.shape, float('inf'), dtype=t.dtype, device=DEV)
    assert ops.gradient(t, out) is out
    _assert_same(out.cpu().numpy(), want, (shape, dt, m))
    assert np.array_equal(G.bits(t.cpu().numpy().view(want.real.dtype)), G.bits(f.view(want.real.dtype))), 'the input was written'
    if m == 1:                                            # the scalar form: the block itself, out [3] + block
        o1 = torch.full((3,) + ops.shape, float('inf'), dtype=t.dtype, device=DEV)
        ops.gradient(t[0], o1)
        _assert_same(o1.cpu().numpy(), want[0], (shape, dt, 'scalar form'))
    if m == 3:                                            # the layout of newDistArray(fft, rank=2)
        from mpi4py_fft_amd import newDistArray
        uh, A_hat = newDistArray(fft, rank=1), newDistArray(fft, rank=2)
        uh[...] = f
        ops.gradient(uh, A_hat)
        _assert_same(np.asarray(A_hat), want, (shape, dt, 'rank-2 DistArray'))
    fft.destroy()


def test_gradient_past_one_grid_sweep():
    """fp32, m = 1, 8 523 008 modes > 2 * 16384 * 256 (a lane takes two modes per step), straight through the engine, against the
    same products formed by torch"""
    from mpi4py_fft_amd import _lib
    shape = (208, 208, 392)
    k, _ = R.wavenumbers(shape, True)
    blk = tuple(len(ki) for ki in k)
    count = int(np.prod(blk))
    assert blk == (208, 208, 197) and count > 2 * 16384 * 256
    K = [torch.as_tensor(ki.astype('f'), device=DEV) for ki in k]
    gen = torch.Generator(device=DEV).manual_seed(67)
    f = torch.view_as_complex(torch.randn((1,) + blk + (2,), dtype=torch.float32, device=DEV, generator=gen))
    out = torch.full((1, 3) + blk, float('nan'), dtype=torch.complex64, device=DEV)
    _lib.engine().ps_gradient(f, out, 1, K, blk, 4)
    mesh = [K[0][:, None, None], K[1][None, :, None], K[2][None, None, :]]
    got = torch.view_as_real(out).view(torch.int32)
    for j in range(3):
        want = torch.stack([-(mesh[j] * f[0].imag), mesh[j] * f[0].real], dim=-1)
        assert bool(torch.equal(got[0, j], want.view(torch.int32))), j


_REF = {}
KINDS = {'small': (8, 6, 20), 'odd': (5, 3, 7), 'misaligned': (8, 6, 20), 'many workgroups': (32, 32, 34)}
SWEEP_SHAPE = {'d': (128, 96, 100), 'f': (128, 128, 160)}


def _tensor_field(kind, dt):
    """(A [3][3][count] in the precision under test, reference, magnitudes): computed once per case, never modified"""
    key = (kind, dt)
    if key not in _REF:
        count = int(np.prod(SWEEP_SHAPE[dt] if kind == 'sweep' else KINDS[kind]))
        A = np.random.default_rng(71).standard_normal((3, 3, count)).astype(dt)
        ref, mag = G.stats(A)
        for a in (A, ref, mag):
            a.setflags(write=False)
        _REF[key] = (A, ref, mag)
    return _REF[key]


def _device(A, dt, misaligned=False):
    flat = torch.as_tensor(np.ascontiguousarray(A).reshape(-1).astype(dt))
    if not misaligned:
        t = flat.to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(flat.numel() + 1, dtype=flat.dtype, device=DEV)
    t = buf[1:]
    t.copy_(flat)
    assert t.data_ptr() % 16 != 0
    return t


def _run(t, count, dt):
    """gfft_ps_gradient_stats straight through the engine on a flat device tensor"""
    from mpi4py_fft_amd import _lib
    out = torch.full((G.NVAL,), -7.0, dtype=torch.float64, device=DEV)
    _lib.engine().ps_gradient_stats(t, count, out, 8 if dt == 'd' else 4)
    return out.cpu().numpy()


def _geometry(count, dt, aligned=True):
    V = WIDE[dt] if (count % WIDE[dt] == 0 and aligned) else 1
    step = 256 * V
    chunk = -(-(-(-count // 2048)) // step) * step
    return V, chunk, -(-count // chunk) if count else 0


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', ['small', 'odd', 'misaligned', 'many workgroups', 'sweep'])
def test_gradient_stats_against_reference(kind, dt):
    """Every entry within (count + 64) 2^-53 M of the long-double reference, and two calls give identical bits."""
    A, ref, mag = _tensor_field(kind, dt)
    count = A.shape[2]
    V, chunk, nwg = _geometry(count, dt, kind != 'misaligned')
    assert V == (WIDE[dt] if kind in ('small', 'many workgroups', 'sweep') else 1)
    assert (kind != 'many workgroups' or nwg >= 32) and (kind != 'sweep' or (nwg > 1024 and chunk == 2 * 256 * V))
    t = _device(A, dt, kind == 'misaligned')
    got = _run(t, count, dt)
    G.assert_stats(got, ref, mag, count, 'gradient_stats %s %s' % (kind, dt))
    assert np.array_equal(_run(t, count, dt), got), 'the result does not repeat bit for bit'
    assert np.all(got[:3] > 0) and np.all(np.abs(got[3:]) > 0)


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_nan_shows_in_the_sums_that_read_it_only(dt):
    A0, ref0, _ = _tensor_field('small', dt)
    A = np.array(A0)
    count = A.shape[2]
    A[1, 2, 321] = np.nan
    ref, mag = G.stats(A)
    nan = [4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 18, 19]          # every sum but div^2 and the powers of the diagonal
    assert np.isnan(ref[nan]).all() and np.isfinite(np.delete(ref, nan)).all()
    got = _run(_device(A, dt), count, dt)
    assert np.isnan(got[nan]).all(), got
    assert np.isfinite(np.delete(got, nan)).all() and np.all(got[:3] > 0), got
    G.assert_stats(got, ref, mag, count, 'nan %s' % dt)          # the maxima and the other sums: the point is skipped, not the field


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_empty_block_writes_zeros(dt):
    t = torch.ones(16, dtype=TORCH[dt], device=DEV)
    got = _run(t, 0, dt)
    assert np.array_equal(G.bits(got), G.bits(np.zeros(G.NVAL)))


def test_gradient_stats_replays_from_a_captured_graph():
    """out= with reduce=False under torch.cuda.graph after one warm-up call: the replay follows new contents of A."""
    from mpi4py_fft_amd import comm, newDistArray
    shape = (8, 6, 20)
    fft, ops = _ops(comm.COMM_SELF, shape, 'd')
    A = newDistArray(fft, False, rank=2)
    rng = np.random.default_rng(73)
    first, second = rng.standard_normal((3, 3) + shape), rng.standard_normal((3, 3) + shape)
    A[...] = first
    out = torch.zeros(G.NVAL, dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert ops.gradient_stats(A, out=out, reduce=False) is out          # warm-up on another stream: its scratch exists now
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = out.cpu().numpy().copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gradient_stats(A, out=out, reduce=False)
    for field, want in ((first, eager), (second, None)):
        A[...] = field
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().copy()
        if want is None:
            want = ops.gradient_stats(A)
            assert not np.array_equal(want, eager)
        assert np.array_equal(got, want), 'the replay does not follow A'
    fft.destroy()


@pytest.mark.parametrize('P,grid', [(2, [2, 1, 1]), (4, [2, 2, 1])], ids=['slab2', 'pencil4'])
def test_thread_ranks(P, grid):
    """Every rank holds the same reduced statistics bit for bit; they agree with one rank, and with the reference, within the
    bound; the maxima equal the one-rank result."""
    from mpi4py_fft_amd import comm, newDistArray
    shape, dt = (24, 16, 20), 'd'
    A_h = np.random.default_rng(79).standard_normal((3, 3) + shape)
    ref, mag = G.stats(A_h)
    count = int(np.prod(shape))

    def run(c, **kw):
        fft, ops = _ops(c, shape, dt, **kw)
        A = newDistArray(fft, False, rank=2)
        A[...] = A_h[(slice(None),) * 2 + fft.local_slice(False)]
        got = ops.gradient_stats(A)
        fft.destroy()
        return got
    one = run(comm.COMM_SELF)
    G.assert_stats(one, ref, mag, count, 'one rank')
    res = cases.run_ranks(P, lambda c: run(c, grid=grid))
    for got in res:
        assert np.array_equal(got, res[0]), 'ranks disagree'
        assert np.array_equal(got[:3], one[:3]), (P, grid, 'maxima vs one rank')
        assert np.all(np.abs(got - one) <= G.bound(count, mag)), (P, grid, got, one)
        G.assert_stats(got, ref, mag, count, 'P = %d %s' % (P, grid))


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', [(24, 24, 24), (16, 12, 20)], ids=str)
def test_identities_end_to_end(shape, dt):
    """gradient -> nine backward transforms -> gradient_stats on a random solenoidal field truncated by the strict 2/3 rule: the
    residuals of sum ss = sum ww / 2, sum Q = 0, sum R = 0, sum wsw = -4/3 sum sss over their magnitudes M, of sum ss = N
    enstrophy(u_hat) over sum ss, and of the pointwise R = -(sss / 3 + wsw / 4) over max M_R stay below 1e-12 in fp64; in fp32
    the quadratic ones (ss against ww / 2, Q, the enstrophy) below 256 * 2^-23.  Separation thresholds, not measurements: a
    correct chain sits at a few eps log2 N, a wrong index, sign or transposed pair at 1e-2 or worse (test_gradient_host)."""
    from mpi4py_fft_amd import comm, newDistArray
    fft, ops = _ops(comm.COMM_SELF, shape, dt)
    uh_h, k = G.solenoidal_field(shape, 83)
    uh, A_hat, A = newDistArray(fft, rank=1), newDistArray(fft, rank=2), newDistArray(fft, False, rank=2)
    uh[...] = uh_h.astype(dt.upper())
    n = int(np.prod(shape))
    enstrophy = ops.enstrophy(uh)
    assert ops.gradient(uh, A_hat) is A_hat
    for i in range(3):
        for j in range(3):
            fft.backward(A_hat[i][j], A[i][j])
    gs = ops.gradient_stats(A)
    A_h = np.asarray(A)
    _, mag = G.stats(A_h)
    res = residuals(gs, mag, n, enstrophy)
    p = G.pointwise(A_h)
    a = np.abs(A_h.astype('d'))
    mag_r = a[0, 0] * (a[1, 1] * a[2, 2] + a[1, 2] * a[2, 1]) + a[0, 1] * (a[1, 0] * a[2, 2] + a[1, 2] * a[2, 0]) + a[0, 2] * (a[1, 0] * a[2, 1] + a[1, 1] * a[2, 0])
    res['pointwise R'] = float(np.abs(p['R'] + (p['sss'] / 3 + p['wsw'] / 4)).max() / mag_r.max())
    print('%s %s: %s' % (shape, dt, ', '.join('%s %.2e' % kv for kv in res.items())))
    assert gs[4] > 0 and gs[13] != 0
    if dt == 'd':
        assert max(res.values()) <= 1e-12, res
    else:
        quad = [res[key] for key in ('ss = ww / 2', 'sum Q', 'ss = N enstrophy')]
        assert max(quad) <= 256 * 2.0 ** -23, res
    fft.destroy()


def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dns_taylor_green.py')
    spec = importlib.util.spec_from_file_location('dns_taylor_green_gradient', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_RUN = {}


def _fused(ex):
    """The moments of the fused dealiased run on one rank: computed once, shared by the two example tests"""
    if 'fused' not in _RUN:
        from mpi4py_fft_amd import comm
        st = {}
        ex.solve(comm.COMM_SELF, gradients=True, dealias='2/3', stats=st)
        _RUN['fused'] = st['gradients']
    return _RUN['fused']


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def test_example():
    """The dealiased Taylor-Green run with gradients=True: the fused kernels against the array-sized torch expressions in
    every moment, and the skewness against the recorded one."""
    from mpi4py_fft_amd import comm
    ex = _example()
    fused = _fused(ex)
    sb = {}
    ex.solve(comm.COMM_SELF, gradients=True, dealias='2/3', stats=sb, fused=False)
    base = sb['gradients']
    print('fused %s\nbaseline %s' % (fused, base))
    assert fused.dissipation > 0 and fused.skewness < 0 and abs(fused.betchov - 1) <= 1e-9 and fused.div_rms <= 1e-12
    for name in fused._fields:
        x, y = getattr(fused, name), getattr(base, name)
        if name in ('Q', 'R', 'div_rms'):                   # zero to rounding: compared against the scale they vanish on
            scale = {'Q': fused.strain, 'R': fused.strain ** 1.5, 'div_rms': math.sqrt(fused.strain)}[name]
            assert abs(x - y) <= 1e-10 * scale, (name, x, y)
        else:
            assert _rel(x, y) <= 1e-10, (name, x, y)
    assert _rel(fused.skewness, ex.GRADIENT_SKEWNESS) <= 1e-10, (fused.skewness, ex.GRADIENT_SKEWNESS)


def test_example_on_two_thread_ranks():
    ex = _example()
    fused = _fused(ex)

    def body(c):
        st = {}
        ex.solve(c, gradients=True, dealias='2/3', stats=st)
        return st['gradients']
    for got in cases.run_ranks(2, body):
        for name in ('strain', 'enstrophy', 'dissipation', 'skewness', 'flatness', 'transverse_flatness', 'dissipation_flatness',
                     'enstrophy_flatness', 'strain_enstrophy_correlation', 'betchov'):
            assert _rel(getattr(got, name), getattr(fused, name)) <= 1e-12, (name, got, fused)
