"""gfft_ps_structure on the device against tests/structure_ref.py (numpy; long double sums), against exact impulses, against
itself (call against call, ranks against one rank, replay against a new field), against the library's own transform (Parseval)
and against the Taylor-Green vortex.

Launch geometry the cases are chosen against (csrc/spectral.hip, sf_geometry; `_geometry` below restates it and the cases assert
what they rely on).  Workgroups of 256 lanes stage tiles of WHOLE lines of the axis, all m components, in LDS; a tile holds at
most cap = 65536 / (m * bytes per value) points per component (one line if that is longer), at least 1024 where the block allows;
at most 512 workgroups (fewer beyond 1024 values nsep * m * 9 per workgroup), which take the tiles t = w, w + nwg, ...
  * axis 2: a tile = W consecutive lines, W = clamp(min(cap / L, max(ceil(lines / max_wg), ceil(1024 / L))), 1, lines); staging
    loads take 16 bytes (V = 2 in fp64, 4 in fp32) where V divides L and the base is 16-byte aligned, else V = 1.
  * axis 0, 1: per index of the axes in front a tile = W = 2^w <= 256 adjacent columns of the axes behind (`inner` columns in
    all), the largest with W L <= cap and W / 2 < inner, halved while W > 16, W L / 2 >= 1024 and there are fewer tiles than
    max_wg; a ragged last tile has fewer columns; V as above with `inner` in the place of L, and V = 1 where W < V.
  (8, 6, 20): axis 2 -- one tile of 48 lines, 960 points: lanes take 3 or 4 steps; axis 1 -- W = 32 for 20 columns, one ragged
  tile per plane, 8 workgroups, 192 LDS points of which 120 are the block's; axis 0 -- W = 128 for 120 columns, one ragged tile
  of 1024 LDS points, 4 steps per lane.  (5, 3, 7): everything odd, V = 1 (axis 1: W = 8 for 7 columns, 24 points: most lanes
  idle).  (8, 6, 20) one element into an allocation: V = 1 with even sizes.  (32, 32, 34): axis 2 -- 31 lines per tile, 34 tiles, the
  last one of a single line, V = 1 in fp32 (34 = 2 * 17); axis 0 -- W = 32 for 1088 columns, 34 full tiles; axis 1 -- W = 32, two
  tiles per plane, the second with 2 columns, 64 workgroups, V = 1 in fp32.
  (2, 3, 4096) and (4096, 2, 3), m = 4: one line of 4096 exceeds cap -- a tile is one line of all four components, 128 KiB of
  LDS in fp64 (the launch that needs more than 64 KiB), 16 steps per lane; along axis 0 that line is a column of W = 1, V = 1.
  Walking: m = 4, fp64, two separations: cap = 2048 and max_wg = 512.  (232, 232, 20) along axis 2: 102 lines per tile, 528
  tiles > 512, so workgroups 0 - 15 take a second tile; (260, 12, 130) along axis 1: W = 128, two tiles per plane (the second
  with 2 columns), 520 tiles > 512, so workgroups 0 - 7 take a second tile.  Sized as the smallest round shapes whose tile count
  exceeds the cap on the workgroups at the smallest cap (four fp64 components).

Bound (derived in structure_ref.py, not measured): |got - ref| <= (count + 16) 2^-53 M per entry.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cases, structure_ref as R

DEV = 'cuda'
TORCH = {'d': torch.float64, 'f': torch.float32}
WIDE = {'d': 2, 'f': 4}
BYTES = {'d': 8, 'f': 4}
KINDS = {'small': (8, 6, 20), 'odd': (5, 3, 7), 'misaligned': (8, 6, 20), 'many workgroups': (32, 32, 34)}
FIELDS = [(1, 'none'), (3, 'axis'), (4, 'zero')]            # m and lcomp: -1, the axis, 0 (a [u, theta] field)
_REF = {}


def _geometry(shape, axis, m, nsep, dt, aligned=True):
    """sf_geometry of csrc/spectral.hip: dict(V, W, ntiles, nwg, points per full tile)"""
    L, nvalues = shape[axis], nsep * m * 9
    max_wg = 512 if nvalues <= 1024 else 512 * 1024 // nvalues
    cap = 65536 // (m * BYTES[dt])
    if axis == 2:
        lines = shape[0] * shape[1]
        W = max(1, min(cap // L, max(-(-lines // max_wg), -(-1024 // L)), lines))
        V = WIDE[dt] if (L % WIDE[dt] == 0 and aligned) else 1
        ntiles = -(-lines // W)
    else:
        inner, outer = (shape[2], shape[0]) if axis == 1 else (shape[1] * shape[2], 1)
        W = 256
        while W > 1 and (W * L > cap or W // 2 >= inner):
            W //= 2
        while W > 16 and (W // 2) * L >= 1024 and outer * -(-inner // W) < max_wg:
            W //= 2
        V = WIDE[dt] if (W >= WIDE[dt] and inner % WIDE[dt] == 0 and aligned) else 1
        ntiles = outer * -(-inner // W)
    return dict(V=V, W=W, ntiles=ntiles, nwg=min(ntiles, max_wg), points=W * L)


def _seps(n):
    return sorted({0, 1 % n, 2 % n, n - 1} | ({n // 2} if n % 2 == 0 else set()))


def _lcomp(which, axis):
    return {'none': -1, 'axis': axis, 'zero': 0}[which]


def _reference(shape, dt, m, axis, seps, lcomp, seed=83):
    """(u [m] + shape in the precision under test, reference, magnitudes): computed once per case, never modified"""
    key = (tuple(shape), dt, m, axis, tuple(seps), lcomp, seed)
    if key not in _REF:
        u = np.random.default_rng(seed).standard_normal((m,) + tuple(shape)).astype(dt)
        ref, mag = R.structure(u, axis, seps, lcomp)
        for a in (u, ref, mag):
            a.setflags(write=False)
        _REF[key] = (u, ref, mag)
    return _REF[key]


def _device(u, dt, misaligned=False):
    flat = torch.as_tensor(np.ascontiguousarray(u).reshape(-1).astype(dt))
    if not misaligned:
        t = flat.to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(flat.numel() + 1, dtype=flat.dtype, device=DEV)
    t = buf[1:]
    t.copy_(flat)
    assert t.data_ptr() % 16 != 0
    return t


def _run(t, m, shape, axis, seps, lcomp, dt):
    """gfft_ps_structure straight through the engine on a flat device tensor"""
    from mpi4py_fft_amd import _lib
    out = torch.full((len(seps), m, R.NVAL), -7.0, dtype=torch.float64, device=DEV)
    _lib.engine().ps_structure(t, m, shape, axis, seps, lcomp, out, BYTES[dt])
    return out.cpu().numpy()


def _check(shape, dt, m, axis, seps, lcomp, what, misaligned=False):
    u, ref, mag = _reference(shape, dt, m, axis, seps, lcomp)
    t = _device(u, dt, misaligned)
    got = _run(t, m, shape, axis, seps, lcomp, dt)
    worst = R.assert_structure(got, ref, mag, int(np.prod(shape)), what)
    assert np.array_equal(R.bits(_run(t, m, shape, axis, seps, lcomp, dt)), R.bits(got)), 'the result does not repeat bit for bit'
    if lcomp < 0:
        assert np.array_equal(R.bits(got[:, :, R.MIX]), R.bits(np.zeros((len(seps), m)))), 'lcomp = -1: +0.0'
    return got, worst


@pytest.mark.parametrize('m,which', FIELDS)
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('axis', [0, 1, 2])
@pytest.mark.parametrize('kind', list(KINDS))
def test_against_reference(kind, axis, dt, m, which):
    """Every entry within (count + 16) 2^-53 M of the long-double reference at separations 0, 1, 2, n / 2 and n - 1, and two
    calls give identical bits."""
    shape = KINDS[kind]
    seps = _seps(shape[axis])
    g = _geometry(shape, axis, m, len(seps), dt, kind != 'misaligned')
    if kind in ('odd', 'misaligned'):
        assert g['V'] == 1
    if kind == 'many workgroups':
        assert g['nwg'] >= 16 and (g['V'] == WIDE[dt] or (axis != 0 and dt == 'f'))       # rows of 34 = 2 * 17: no 16-byte loads of floats
    got, _ = _check(shape, dt, m, axis, seps, _lcomp(which, axis), 'structure %s axis %d %s m = %d' % (kind, axis, dt, m),
                    kind == 'misaligned')
    assert np.array_equal(R.bits(got[0]), R.bits(np.zeros((m, R.NVAL)))), 'sep = 0 gives zeros'
    assert np.all(got[1:, :, R.D2] > 0)


def test_sixty_four_separations():
    shape, m = (8, 6, 20), 3
    seps = [k % 20 for k in range(64)]
    got, _ = _check(shape, 'd', m, 2, seps, 2, 'structure 64 separations')
    assert np.array_equal(R.bits(got[:20]), R.bits(got[20:40])) and np.array_equal(R.bits(got[:4]), R.bits(got[60:]))


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape,axis', [((2, 3, 4096), 2), ((4096, 2, 3), 0)])
def test_the_longest_axis(shape, axis, dt):
    """One line of 4096 points of four components: the tile that exceeds 64 KiB of LDS in fp64."""
    g = _geometry(shape, axis, 4, 3, dt)
    assert g['points'] == 4096 and g['ntiles'] == 6 and g['W'] == 1
    _check(shape, dt, 4, axis, [1, 2048, 4095], 0, 'structure longest axis %d %s' % (axis, dt))


@pytest.mark.parametrize('shape,axis', [((232, 232, 20), 2), ((260, 12, 130), 1)])
def test_every_tile_count_past_the_workgroups(shape, axis):
    """More tiles than workgroups: the first workgroups walk to a second tile and add it to their running sums."""
    seps = [1, shape[axis] - 1]
    g = _geometry(shape, axis, 4, len(seps), 'd')
    assert g['nwg'] == 512 < g['ntiles'] < 1024 and g['points'] > 256
    _check(shape, 'd', 4, axis, seps, 0, 'structure walking axis %d' % axis)


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('axis', [0, 1, 2])
@pytest.mark.parametrize('n', [7, 20])
def test_impulses_exactly(n, axis, dt):
    """A field that is zero but for one entry 1.0, planted at index 0, n - 1 and an interior point of the axis: at every
    separation 1 ... n - 1 the increment is +1 at one point and -1 at another, so the odd sums are exactly 0.0 and the even and
    absolute ones exactly 2.0; with lcomp = the planted component its mixed entry is the odd sum 0.0.  A wrap that is off by
    one at either end loses or doubles a term."""
    shape = [3, 5, 4]
    shape[axis] = n
    shape = tuple(shape)
    seps = list(range(1, n))
    want = np.zeros((len(seps), 2, R.NVAL))
    want[:, 1, [R.D2, R.D4, R.D6, R.ABS1, R.ABS3]] = 2.0
    for at in (0, n - 1, n // 2 + 1):
        u = np.zeros((2,) + shape, dtype=dt)
        where = [1, 2, 3]
        where[axis] = at
        u[(1,) + tuple(where)] = 1.0
        got = _run(_device(u, dt), 2, shape, axis, seps, 1, dt)
        assert np.array_equal(got, want), (at, np.argwhere(got != want)[:6].tolist())


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_wrapper_repeats_and_out_equals_the_reduced_table(dt):
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape = (8, 6, 20)
    fft = PFFT(comm.COMM_SELF, shape, dtype=dt)
    ops = spectral.SpectralOps(fft)
    u = newDistArray(fft, False, rank=1)
    for axis in range(3):
        seps = _seps(shape[axis])
        G, ref, mag = _reference(shape, dt, 3, axis, seps, axis)
        u[...] = np.array(G)                           # (a writable copy: the cached field stays as it is)
        a = ops.structure_functions(u, axis, seps, lcomp=axis)
        b = ops.structure_functions(u, axis, seps, lcomp=axis)
        assert isinstance(a, np.ndarray) and a.shape == (len(seps), 3, 9) and np.array_equal(R.bits(a), R.bits(b))
        R.assert_structure(a, ref, mag, int(np.prod(shape)), 'wrapper axis %d %s' % (axis, dt))
        out = torch.full((len(seps), 3, 9), -1.0, dtype=torch.float64, device=DEV)
        assert ops.structure_functions(u, axis, seps, lcomp=axis, out=out, reduce=False) is out
        assert np.array_equal(R.bits(out.cpu().numpy()), R.bits(a))
    fft.destroy()


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('axis', [0, 1, 2])
@pytest.mark.parametrize('lcomp', [-1, 0, 1])
def test_nan_reaches_exactly_the_sums_it_enters(axis, lcomp, dt):
    shape, m = (8, 6, 20), 3
    seps = [s for s in _seps(shape[axis]) if s]
    u0, _, _ = _reference(shape, dt, m, axis, seps, lcomp)
    clean = _run(_device(u0, dt), m, shape, axis, seps, lcomp, dt)
    u = np.array(u0)
    u[1, 3, 2, 11] = np.nan
    got = _run(_device(u, dt), m, shape, axis, seps, lcomp, dt)
    own = np.zeros(got.shape, dtype=bool)
    own[:, 1, :R.MIX] = True
    own[:, 1, R.MIX] = lcomp >= 0                     # its own d2 enters its mixed term whenever one is formed
    if lcomp == 1:
        own[:, :, R.MIX] = True                       # and as d_l it enters every component's
    assert np.array_equal(np.isnan(got), own), np.argwhere(np.isnan(got) != own)[:6].tolist()
    assert np.array_equal(R.bits(got[~own]), R.bits(clean[~own])), 'a sum the NaN does not enter has moved'


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_empty_block_writes_zeros(dt):
    t = torch.ones(64, dtype=TORCH[dt], device=DEV)
    for shape, axis in (((0, 6, 20), 2), ((8, 0, 20), 2), ((8, 6, 0), 0)):
        got = _run(t, 3, shape, axis, [0, 1, 5], 0, dt)
        assert np.array_equal(R.bits(got), R.bits(np.zeros((3, 3, R.NVAL)))), shape


def test_replays_from_a_captured_graph():
    """out= with reduce=False under torch.cuda.graph after one warm-up call: the replay follows new contents of u."""
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape, seps = (8, 6, 20), [1, 2, 10]
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft)
    u = newDistArray(fft, False, rank=1)
    rng = np.random.default_rng(89)
    first, second = rng.standard_normal((3,) + shape), rng.standard_normal((3,) + shape)
    u[...] = first
    out = torch.zeros((3, 3, 9), dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert ops.structure_functions(u, 2, seps, lcomp=2, out=out, reduce=False) is out      # warm-up: its scratch exists now
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = out.cpu().numpy().copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.structure_functions(u, 2, seps, lcomp=2, out=out, reduce=False)
    for field, want in ((first, eager), (second, None)):
        u[...] = field
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().copy()
        if want is None:
            want = ops.structure_functions(u, 2, seps, lcomp=2)
            assert not np.array_equal(want, eager)
        assert np.array_equal(got, want), 'the replay does not follow u'
    fft.destroy()


@pytest.mark.parametrize('dt,rtol', [('d', 1e-10), ('f', 1e-4)])
def test_second_order_ties_to_the_transform(dt, rtol):
    """Parseval: with the library's forward transform u_hat (normalised by 1 / N_total, so sum_x u^2 = N_total sum_k w |u_hat|^2,
    w = `hermitian_weights`), sum_x (u(x + r e_a) - u(x))^2 = N_total * 2 sum_k w |u_hat(k)|^2 (1 - cos(2 pi k_a r / N_a)).
    Tolerance: the suite's transform contract, relative 1e-10 in fp64 and 1e-4 in fp32."""
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape = (16, 12, 20)
    fft = PFFT(comm.COMM_SELF, shape, dtype=dt)
    ops = spectral.SpectralOps(fft)
    u = newDistArray(fft, False, rank=1)
    u_hat = newDistArray(fft, True, rank=1)
    G = np.random.default_rng(97).standard_normal((3,) + shape).astype(dt)
    u[...] = G
    for c in range(3):
        fft.forward(u[c], u_hat[c])
    u[...] = G                                         # (a real transform may use its input as workspace)
    P = np.abs(np.asarray(u_hat).astype(np.complex128)) ** 2 * spectral.hermitian_weights(fft).cpu().numpy().astype(np.float64)
    k = [np.fft.fftfreq(shape[0], 1.0 / shape[0]), np.fft.fftfreq(shape[1], 1.0 / shape[1]), np.fft.rfftfreq(shape[2], 1.0 / shape[2])]
    ntot = float(np.prod(shape))
    assert np.allclose(ntot * P.sum(axis=(1, 2, 3)), (G.astype(np.float64) ** 2).sum(axis=(1, 2, 3)), rtol=rtol)     # the normalisation
    for axis in range(3):
        seps = [1, 2, 3, shape[axis] // 2, shape[axis] - 1]
        sf = ops.structure_functions(u, axis, seps)
        for i, r in enumerate(seps):
            f = 1.0 - np.cos(2 * np.pi * k[axis] * r / shape[axis])
            f = f.reshape([-1 if a == axis else 1 for a in range(3)])
            want = ntot * 2.0 * (P * f[None]).sum(axis=(1, 2, 3))
            assert np.all(np.abs(sf[i, :, R.D2] - want) <= rtol * np.abs(want)), (axis, r, sf[i, :, R.D2], want)
    fft.destroy()


def test_taylor_green_second_order_along_x():
    """u_0 = sin x cos y cos z on 32^3 points of (2 pi)^3: d = (sin(x + rho) - sin x) cos y cos z with rho = 2 pi r / 32, so
    <d^2> = (1 - cos rho) <cos^2 y> <cos^2 z> = (1 - cos rho) / 4.  The sampling identity that makes the grid mean equal the
    integral: the mean over N equispaced points of a whole period of cos(j x + phase) is exactly 0 for every integer j that is
    no multiple of N; here sin^2, cos^2 and sin(x + rho) sin x hold j = 0 and 2 only, and N = 32.  Beside the bound stands the
    rounding of the field itself: a and b are each within 2 ulp of the exact samples (sin, cos and two products), which moves
    d^2 by at most 16 * 2^-53 of its magnitude (|a| + |b|)^2."""
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    N = 32
    fft = PFFT(comm.COMM_SELF, (N, N, N), dtype='d')
    ops = spectral.SpectralOps(fft)
    x = 2 * np.pi * np.arange(N) / N
    G = np.zeros((3, N, N, N))
    G[0] = np.sin(x)[:, None, None] * np.cos(x)[None, :, None] * np.cos(x)[None, None, :]
    G[1] = -np.cos(x)[:, None, None] * np.sin(x)[None, :, None] * np.cos(x)[None, None, :]
    u = newDistArray(fft, False, rank=1)
    u[...] = G
    seps = spectral.log_separations(N) + [N - 1]
    sf = ops.structure_functions(u, 0, seps, lcomp=0)
    _, mag = R.structure(G, 0, seps, 0)
    mo = spectral.structure_moments(sf, N ** 3, axis=0)
    assert mo.longitudinal == 0 and mo.transverse == [1, 2]
    for i, r in enumerate(seps):
        want = (1.0 - np.cos(2 * np.pi * r / N)) / 4.0
        tol = (R.bound(N ** 3, mag[i, 0, R.D2]) + 16 * 2.0 ** -53 * mag[i, 0, R.D2]) / N ** 3
        assert abs(mo.S[i, 0, 1] - want) <= tol, (r, mo.S[i, 0, 1], want, tol)
        assert sf[i, 2, R.D2] == 0.0                   # u_2 = 0
    # d is a product of three cosines of independent arguments: its flatness is (<cos^4> / <cos^2>^2)^3 = (3/2)^3 (j <= 4: sampled exactly)
    assert np.allclose(mo.flatness[:, 0], 27.0 / 8.0, rtol=1e-12)
    fft.destroy()


def test_two_thread_ranks_on_a_slab_grid():
    """Both ranks hold the same reduced table bit for bit; it agrees with one rank, and with the reference, within the bound;
    the axis the slab grid splits is refused."""
    from mpi4py_fft_amd import PFFT, comm, newDistArray, spectral
    shape, dt = (24, 16, 20), 'd'
    G = np.random.default_rng(101).standard_normal((3,) + shape)
    count = int(np.prod(shape))
    seps = {a: _seps(shape[a]) for a in (1, 2)}
    refs = {a: R.structure(G, a, seps[a], a) for a in (1, 2)}

    def run(c, **kw):
        fft = PFFT(c, shape, dtype=dt, **kw)
        ops = spectral.SpectralOps(fft)
        u = newDistArray(fft, False, rank=1)
        u[...] = G[(slice(None),) + fft.local_slice(False)]
        got = {a: ops.structure_functions(u, a, seps[a], lcomp=a) for a in (1, 2)}
        if c.Get_size() > 1:
            assert ops.whole_axes() == [1, 2]
            with pytest.raises(AssertionError, match=r'whole axes of this grid are \[1, 2\]'):
                ops.structure_functions(u, 0, [1])
        fft.destroy()
        return got
    one = run(comm.COMM_SELF)
    res = cases.run_ranks(2, lambda c: run(c, grid=[2, 1, 1]))
    for a in (1, 2):
        ref, mag = refs[a]
        R.assert_structure(one[a], ref, mag, count, 'one rank, axis %d' % a)
        for got in res:
            assert np.array_equal(R.bits(got[a]), R.bits(res[0][a])), 'ranks disagree'
            assert np.all(np.abs(got[a] - one[a]) <= R.bound(count, mag)), (a, got[a], one[a])
            R.assert_structure(got[a], ref, mag, count, '2 ranks, axis %d' % a)
