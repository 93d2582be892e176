"""Every pass kernel past its first tile, at small shapes.

A transform kernel is a walk: a workgroup takes a tile, then the tile `grid` further on, and what it carries from one tile to
the next -- LDS regions of the barrier-free exchanges, the fold slot of the truncating store, invariants hoisted behind the
laundered row index, the `tile >= ntiles` guard of the XCD-contiguous order -- is where these kernels were hard to get right.
The small shapes of the suite launch one workgroup per tile, so that state is carried only by the minutes-long cases.  Here the
library's own lever, option "grid_cap", makes few workgroups walk many tiles, and include/gfft.h's promise -- "the arithmetic of
a pass does not depend on its launch form" -- is the oracle: one workgroup walking every tile must give the same BITS as one
workgroup per tile.  The kernels use no atomics; a single differing bit means a tile read state another tile left.

Per case: the baseline (grid_cap = 0) is shown by gfft_plan_pass_launch to run workgroups == tiles in every pass and is held to
the suite's rounding-level bound against the float64 oracle (tests/cases.py assert_close; no tolerance of this file's own); then
fresh plans under caps 1 and 3 -- and, for register kernels under xcd_swizzle = 1, 64 and 72 on batches of >= 150 tiles that are
no multiple of 8 -- must report the same tiles on fewer workgroups and return the baseline's bytes, forward and backward.
Line counts are no multiple of 16 and are grown from the REPORTED tile counts (never from a copy of the kernel tables) until a
cap-1 walk is at least 5 tiles long and the tiles do not divide evenly among 3 (8) workgroups.  (A strided pass whose stores miss
the 128-byte lines takes the XCD-contiguous order on its own and then launches a multiple of 8 workgroups: where that happens the
search moves on to a tile count that is one, so that the baseline is one tile per workgroup; plans of several passes, each
with a tile count of its own, seek the uneven shares without requiring them.  The baseline of the xcd_swizzle = 1 cases runs
with the order switched off.)

Every case prints one row: family, n, mapping, dtype, tiles per pass, workgroups per cap (pytest -s shows the table)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pfft_oracle as O
from tests import cases

CAPS = ((1, -1), (3, -1))                       # (grid_cap, xcd_swizzle)
SWIZZLE_CAPS = ((64, 1), (72, 1), (3, 1))       # ragged last eighth; per_xcd no multiple of grid / 8; below 64 the order falls back


@pytest.fixture
def walk():
    """walk(cap, swizzle = -1) sets the two options -- before the plans of a run are made; they stay through its executes --,
    and the defaults come back afterwards, also after a failure."""
    from mpi4py_fft_amd import _lib

    def set_(cap, swizzle=-1):
        _lib.set_option('grid_cap', cap)
        _lib.set_option('xcd_swizzle', swizzle)
    print()                                     # (the table's rows start their lines)
    yield set_
    _lib.set_option('grid_cap', 0)
    _lib.set_option('xcd_swizzle', -1)


class Run:
    """What one execution of a case left: forward and backward output (host copies), [(tiles, workgroups)] of every pass of both
    plans, gfft_plan_describe of both, and whether libfft fused the truncation."""
    def __init__(self, fwd, bwd, launch, text, fused=False):
        self.fwd, self.bwd, self.launch, self.text, self.fused = fwd, bwd, launch, text, fused


def _hi(dt):
    return 'd' if dt in 'df' else 'D'


class Serial:
    """libfft.FFT(shape, axes, dt) -- optionally a real-to-real kind or a 3/2-rule padding -- on seeded random data: forward
    (normalised: the scale rides on the store) of x, backward of the oracle's spectrum rounded to dt.  Both outputs start as
    NaN, so an entry no tile wrote shows.  Reference: oracle.pfft_oracle.OFFT in float64 on the same (widened) inputs."""
    def __init__(self, family, n, mapping, dt, shape, axes, r2r=None, padding=None, path=None, seed=5):
        self.family, self.n, self.mapping, self.dt = family, n, mapping, dt
        self.shape, self.axes, self.r2r, self.padding, self.path = tuple(shape), tuple(np.atleast_1d(axes)), r2r, padding, path
        hi = _hi(dt)
        kw = {}
        if r2r is not None:
            kw['r2r'] = r2r
        if padding is not None:
            kw['padding'] = padding
        ref = O.OFFT(self.shape, self.axes, hi, **kw)
        self.x = O.rng_array(self.shape, dt, seed)
        self.want = ref.forward(self.x.astype(hi))
        self.spec = self.want.astype(dt if r2r is not None else dt.upper())
        self.wantb = ref.backward(self.spec.astype(self.want.dtype))
        if r2r is not None:
            self.nelem = int(np.prod([O.r2r_logical_n(r2r, self.shape[a]) for a in self.axes]))
        else:
            self.nelem = int(np.prod([self.shape[a] for a in self.axes]))

    def execute(self):
        from mpi4py_fft_amd import FFT, asdevice, fftw
        kw = {}
        if self.r2r is not None:
            fam, typ = O.R2R_KINDS[self.r2r]
            f, b = (fftw.dctn, fftw.idctn) if fam == 'dct' else (fftw.dstn, fftw.idstn)
            kw['transforms'] = {self.axes: (functools.partial(f, type=typ), functools.partial(b, type=typ))}
        if self.padding is not None:
            kw['padding'] = self.padding
        fft = FFT(self.shape, self.axes, dtype=self.dt, **kw)
        try:
            assert tuple(fft.forward.output_array.shape) == self.want.shape, (fft.forward.output_array.shape, self.want.shape)
            plans = (fft.fwd, fft.bck)
            text = [p._eng.plan_describe(p._plan) for p in plans]
            out = asdevice(np.full(self.want.shape, np.nan, dtype=self.spec.dtype))
            fft.forward(asdevice(self.x), dst=out)
            fwd = np.asarray(out).copy()
            back = asdevice(np.full(self.shape, np.nan, dtype=self.dt))
            fft.backward(asdevice(self.spec), dst=back)
            bwd = np.asarray(back).copy()
            return Run(fwd, bwd, cases.plan_launches(plans), text, bool(fft._fused_trunc))
        finally:
            fft.destroy()

    def check(self, run):
        what = (self.family, self.n, self.mapping, self.dt)
        if self.path is not None:
            self.path(self, run)
        cases.assert_close(run.fwd.astype(self.want.dtype), self.want, self.dt, self.nelem, what + ('forward',))
        cases.assert_close(run.bwd.astype(self.wantb.dtype), self.wantb, self.dt, self.nelem, what + ('backward',))


def _settle(build, lines, need, mod, strict):
    """The case and its baseline run (grid_cap = 0) at the first line count, grown from `lines` by what gfft_plan_pass_launch
    REPORTS, at which every pass has at least `need` tiles on as many workgroups, no pass's tiles divide by `mod`, and the
    lines are no multiple of 16.  lines = None: the shape is given; it is taken as it is.  strict = False (plans of several passes with tiles
    of their own each): the divisibility is sought, not required."""
    good = None
    for _ in range(24):
        if lines is not None and lines % 16 == 0:
            lines += 1
        case = build(lines)
        base = case.execute()
        tiles = [t for t, _ in base.launch]
        assert tiles and min(tiles) > 0, (case.family, case.n, base.launch)
        if lines is None:
            return case, base
        if min(tiles) < need:
            lines = -(-lines * need // min(tiles)) + 1
            continue
        if any(w != t for t, w in base.launch):
            # (a pass that takes the XCD-contiguous order on its own -- strided stores off the 128-byte lines -- launches a
            # multiple of 8 workgroups from 64 tiles on: the baseline form needs a tile count that is one)
            lines += 1
            continue
        good = case, base
        even = [t for t in tiles if t % mod == 0]
        if not even:
            return good
        lines += -(-lines // even[0])           # about one tile more of the pass that divides evenly
    assert good is not None and not strict, ('no line count found', case.family, case.n, case.mapping, case.dt, lines, base.launch)
    return good


def _walk_case(walk, build, lines, runs=CAPS, need=5, mod=3, strict=True, base_swizzle=-1):
    """The check of this file for one case; prints its row of the table."""
    walk(0, base_swizzle)
    case, base = _settle(build, lines, need, mod, strict)
    # the launch form of every small test of the suite: one tile per workgroup, and no pass is a persistent fused pair
    # (gfft_plan_pass_launch refuses those: the case would have raised)
    assert all(w == t for t, w in base.launch), (case.family, case.n, case.mapping, case.dt, base.launch)
    case.check(base)
    cols = []
    for cap, swizzle in runs:
        walk(cap, swizzle)
        run = case.execute()
        what = (case.family, case.n, case.mapping, case.dt, 'cap %d' % cap, 'swizzle %d' % swizzle, base.launch, run.launch)
        assert len(run.launch) == len(base.launch), what
        for (t, w), (tb, _) in zip(run.launch, base.launch):
            assert t == tb and w == cap, what                                   # the walk covers all tiles ...
            assert (t >= 5 * w) if cap == 1 else (t > w), what                  # ... and every workgroup goes past its first
        assert cases.same_bits(run.fwd, base.fwd), what + ('forward differs from the one-tile-per-workgroup launch',)
        assert cases.same_bits(run.bwd, base.bwd), what + ('backward differs from the one-tile-per-workgroup launch',)
        cols.append('cap %d%s: %s' % (cap, ' swz' if swizzle > 0 else '', '/'.join(str(w) for _, w in run.launch)))
    walk(0)
    print('walk %-22s n=%-11s %-7s %s  tiles %-24s %s' % (case.family, case.n, case.mapping, case.dt,
                                                        '/'.join(str(t) for t, _ in base.launch), '  '.join(cols)))


def _lines_for(n):
    return 197 if n <= 1024 else 41


# ---- complex lines ----------------------------------------------------------------------------------------------------------
def _regs(case, run):
    for text in run.text:
        passes = [ln for ln in text.splitlines() if 'kernel=' in ln]
        assert len(passes) == 1 and 'kernel=regs-' in passes[0], (case.n, text)


def _generic(case, run):
    assert all('kernel=generic' in t for t in run.text), run.text


def _fourstep(case, run):
    for text in run.text:
        assert '[four-step 1/2' in text and 'fused pair' not in text and len(run.launch) == 4, text       # both passes of both plans reported


def _bluestein(case, run):
    # embed, the transforms of length M around the multiplication, extract: all of them walk
    assert all('multiply by B' in t and 'embed' in t and 'extract' in t for t in run.text), run.text


COMPLEX = {'pow2': ([16, 64, 256, 1024, 2048, 4096], _regs), '3.2^k': ([48, 768], _regs), '5.2^k': ([20, 80, 1000], _regs),
           'unequal-width': ([240, 112, 896], _regs), 'generic': ([22, 121, 343], _generic), 'four-step': ([8192, 9216], _fourstep),
           'bluestein': ([521], _bluestein)}


@pytest.mark.parametrize('dt', ['D', 'F'])
@pytest.mark.parametrize('family', list(COMPLEX))
def test_complex_lines_walk(family, dt, walk):
    lengths, path = COMPLEX[family]
    for n in lengths:
        for mapping in ('rows', 'cols') + (('middle',) if n <= 1024 else ()):
            def build(lines, n=n, mapping=mapping):
                shape, axis = cases.walk_batch(mapping, n, lines)
                return Serial(family, n, mapping, dt, shape, (axis,), path=path)
            _walk_case(walk, build, None if mapping == 'middle' else _lines_for(n), strict=family in ('pow2', '3.2^k', '5.2^k', 'unequal-width', 'generic'))


@pytest.mark.parametrize('dt', ['D', 'F'])
def test_per_column_kernels_walk(dt, walk):
    """Lengths 3, 7, 13 along axis 0 of many adjacent columns: tiny_dft_kernel, one column per thread, blocks of 256 columns."""
    def path(case, run):
        _generic(case, run)
        for t, _ in run.launch:                   # the per-column kernel's unit of work, not the LDS kernel's tile
            assert t == -(-case.shape[1] // 256), (case.shape, run.launch)
    for n in (3, 7, 13):
        _walk_case(walk, lambda lines, n=n: Serial('per-column', n, 'cols', dt, (n, lines), (0,), path=path), 1100)


# ---- packed-real rows, real lines along a strided axis -------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('mapping,lengths,want', [('rows', [64, 2048, 96, 1000, 224], 'packed'), ('cols', [64, 96], 'regs')])
def test_real_lines_walk(mapping, lengths, want, dt, walk):
    def path(case, run):
        assert cases.real_path(run.text) == want, (case.n, want, run.text)
    for n in lengths:
        def build(lines, n=n):
            shape, axis = cases.walk_batch(mapping, n, lines)
            return Serial('real ' + want, n, mapping, dt, shape, (axis,), path=path)
        _walk_case(walk, build, _lines_for(n))


# ---- real-to-real kinds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', [cases.REDFT10, cases.RODFT00, cases.REDFT11], ids=lambda k: cases.R2R_NAMES[k])
def test_r2r_kinds_walk(kind, dt, walk):
    """An even, a type-1 odd (line pitch n != N / 2) and a type-4 kind through the MODE_R2R load / store adapters, at a
    power-of-two and a 3 x 2^k logical length, in the three mappings of cases.R2R_MAPPINGS."""
    for N in (512, 768):
        n = cases.r2r_points(kind, N)
        for mapping in cases.R2R_MAPPINGS:
            def path(case, run, N=N, mapping=mapping):
                assert cases.r2r_path(run.text[:1], N, mapping) == 'adapter' and cases.r2r_path(run.text[1:], N, mapping) == 'adapter', run.text

            def build(lines, n=n, mapping=mapping, path=path):
                shape, axis = cases.walk_batch(mapping, n, lines)
                return Serial('r2r ' + cases.R2R_NAMES[kind], n, mapping, dt, shape, (axis,), r2r=kind, path=path)
            _walk_case(walk, build, None if mapping == 'middle' else 197)


# ---- fused truncating store / zero-padding load ----------------------------------------------------------------------------------
TRUNC = [(1024, 683, 'fused pow2'), (64, 32, 'fused pow2'), (768, 512, 'fused 3^b 2^k'), (240, 161, 'fused unequal-width'), (112, 75, 'stand-alone')]


@pytest.mark.parametrize('dt', ['D', 'F', 'd', 'f'])
@pytest.mark.parametrize('n,kept,family', TRUNC)
def test_fused_truncation_and_padding_walk(n, kept, family, dt, walk):
    """The `fold` slot of the truncating store (forward) and the zero-padding load (backward) across tiles: complex axes and the
    real half-axis, odd and even kept lengths, in the three mappings; the path each plan took asserted as
    tests/test_gpu_trunc_guard.py asserts it."""
    for mapping in cases.TRUNC_MAPPINGS:
        def path(case, run, mapping=mapping):
            got = cases.trunc_path([run.fused] + run.text, n, mapping)
            assert got in cases.trunc_expected_path(n, family, dt, mapping), (n, kept, dt, mapping, got, run.text)

        def build(lines, mapping=mapping, path=path):
            shape, axis = cases.walk_batch(mapping, n, lines)
            return Serial('trunc ' + family, '%d->%d' % (n, kept), mapping, dt, shape, (axis,), padding=n / kept, path=path)
        _walk_case(walk, build, None if mapping == 'middle' else 197)


# ---- XCD-contiguous walks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['D', 'F'])
@pytest.mark.parametrize('mapping', ['rows', 'cols'])
def test_xcd_contiguous_walks_with_a_ragged_eighth(mapping, dt, walk):
    """xcd_swizzle = 1 under caps 64 and 72 on >= 150 tiles, no multiple of 8: XCD x walks tiles x * per_xcd + k, the last eighth
    is short, and only `if (tile >= ntiles) continue` keeps the walk inside the batch.  Under cap 3 the order falls back to the
    plain walk (fewer than 64 workgroups), which must still cover every tile."""
    rdt = dt.lower()
    builds = [
        lambda lines: Serial('swizzle pow2', 256, mapping, dt, *_batch(mapping, 256, lines), path=_regs),
        lambda lines: Serial('swizzle 3.2^k', 48, mapping, dt, *_batch(mapping, 48, lines), path=_regs),
        lambda lines: Serial('swizzle unequal-width', 240, mapping, dt, *_batch(mapping, 240, lines), path=_regs),
        lambda lines: Serial('swizzle r2r REDFT10', 256, mapping, rdt, *_batch(mapping, 256, lines), r2r=cases.REDFT10),
        lambda lines: Serial('swizzle trunc', '64->43', mapping, dt, *_batch(mapping, 64, lines), padding=64 / 43),
    ]
    if mapping == 'rows':
        builds.append(lambda lines: Serial('swizzle real packed', 2048, mapping, rdt, *_batch(mapping, 2048, lines)))
        builds.append(lambda lines: Serial('swizzle real packed', 1000, mapping, rdt, *_batch(mapping, 1000, lines)))
    for build in builds:
        _walk_case(walk, build, 601, runs=SWIZZLE_CAPS, need=150, mod=8, base_swizzle=0)        # (baseline: the plain order, one tile per workgroup)


def _batch(mapping, n, lines):
    shape, axis = cases.walk_batch(mapping, n, lines)
    return shape, (axis,)


# ---- on-chip planes, 3-D schedules -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['D', 'F'])
@pytest.mark.parametrize('n', [32, 64])
def test_planes_on_chip_walk(n, dt, walk):
    """fft_plane2d_kernel: 11 planes on 1 and on 3 workgroups; the plane in LDS is rewritten by the next one's row pass."""
    def path(case, run):
        for text in run.text:
            assert 'planes on chip' in text and text.count('\n') == 2, text
    _walk_case(walk, lambda lines: Serial('planes on chip', '%dx%d' % (n, n), 'planes', dt, (11, n, n), (1, 2), path=path), None)


@pytest.mark.parametrize('shape,dt', [((64, 32, 128), 'D'), ((48, 40, 64), 'D'), ((32, 64, 66), 'd'), ((32, 64, 66), 'f')],
                         ids=lambda v: 'x'.join(str(s) for s in v) if isinstance(v, tuple) else v)
def test_3d_schedules_walk(shape, dt, walk):
    """Schedules with workspace passes, pitched and tile-major, and none of them a fused pair."""
    def path(case, run):
        for text in run.text:
            assert 'fused pair' not in text and 'planes on chip' not in text, text
    _walk_case(walk, lambda lines: Serial('3-D schedule', 'x'.join(str(s) for s in shape), 'all', dt, shape, (0, 1, 2), path=path), None)


# ---- layout adapters (the shapes of tests/test_gpu_layouts.py with more lines) -------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Raw:
    """Plans made at the C ABI on flat device buffers.  A subclass gives: plans(eng) -> (forward, backward) handles; xin / specin,
    the two inputs as they lie in memory; nfwd / nbwd, the elements of the two outputs (prefilled with NaN); natural_fwd /
    natural_bwd, which re-lay an output in the natural order of `want` / `wantb`; ref, the OFFT of the natural transform; scale_b,
    the backward plan's scale.  x / spec are the natural-order inputs."""
    mapping = 'layout'

    def prepare(self, shape, axis, dt, real=False):
        self.dt, self.n = dt, shape[axis]
        hi = _hi(dt)
        self.ref = O.OFFT(shape, (axis,), hi)
        self.x = O.rng_array(shape, dt, 9)
        self.want = self.ref.forward(self.x.astype(hi), normalize=False)
        self.spec = self.want.astype(dt.upper())
        self.wantb = self.ref.backward(self.spec.astype('D'), normalize=True)
        self.scale_b = 1.0 / self.n

    def execute(self):
        import torch
        from mpi4py_fft_amd import _lib
        eng = _lib.engine()
        hs = self.plans(eng)
        try:
            text = [eng.plan_describe(h) for h in hs]
            outs = []
            for h, src, count, odt, scale in ((hs[0], self.xin, self.nfwd, self.spec.dtype, 1.0), (hs[1], self.specin, self.nbwd, self.x.dtype, self.scale_b)):
                a = _dev(src)
                b = torch.full((count,), float('nan'), dtype=torch.from_numpy(np.zeros(1, odt)).dtype, device='cuda')
                eng.execute_ptr(h, a.data_ptr(), b.data_ptr(), scale)
                torch.cuda.synchronize()
                outs.append(b.cpu().numpy())
            return Run(outs[0], outs[1], [tw for h in hs for tw in eng.plan_pass_launch(h)], text)
        finally:
            for h in hs:
                eng.plan_destroy(h)

    def check(self, run):
        what = (self.family, self.n, self.dt)
        assert all(ln.count('kernel=regs-') == 1 for ln in run.text), run.text
        cases.assert_close(self.natural_fwd(run.fwd).astype('D'), self.want, self.dt, self.n, what + ('forward',))
        cases.assert_close(self.natural_bwd(run.bwd).astype(self.wantb.dtype), self.wantb, self.dt, self.n, what + ('backward',))


class SplitRows(Raw):
    """gfft_plan_set_split on a complex row plan: [block][row][n / nb] on the output of the forward, the input of the backward plan."""
    def __init__(self, dt, n, nb, rows):
        self.family, self.nb, self.rows = 'split %d blocks' % nb, nb, rows
        self.prepare((rows, n), 1, dt)
        lay = lambda v: np.ascontiguousarray(v.reshape(rows, nb, n // nb).transpose(1, 0, 2))
        self.xin, self.specin, self.nfwd, self.nbwd = self.x, lay(self.spec), rows * n, rows * n
        self.natural_fwd = lambda b: b.reshape(nb, rows, n // nb).transpose(1, 0, 2).reshape(rows, n)
        self.natural_bwd = lambda b: b.reshape(rows, n)

    def plans(self, eng):
        from mpi4py_fft_amd import _lib
        prec, s = _lib.precision_of(self.dt), (self.rows, self.n)
        hf = eng.plan_create(s, s, (1,), _lib.C2C_FORWARD, prec)
        hb = eng.plan_create(s, s, (1,), _lib.C2C_BACKWARD, prec)
        assert eng.plan_set_split(hf, 1, self.nb) and eng.plan_set_split(hb, 0, self.nb)
        return hf, hb


class UnevenRealRows(Raw):
    """gfft_plan_set_split with 3 blocks on packed-real rows: the n / 2 + 1 entries dealt by the block rule, [block][row][w_b]."""
    def __init__(self, dt, n, rows):
        from mpi4py_fft_amd.pencil import _blockdist
        self.family, self.rows, p = 'uneven 3 blocks, real', rows, 3
        self.prepare((rows, n), 1, dt)
        nh = n // 2 + 1
        cuts = [_blockdist(nh, p, r) for r in range(p)]              # (width, start)
        lay = lambda v: np.concatenate([v[:, s:s + w].reshape(-1) for w, s in cuts])

        def unlay(b):
            out, pos = np.empty((rows, nh), dtype=b.dtype), 0
            for w, s in cuts:
                out[:, s:s + w] = b[pos:pos + rows * w].reshape(rows, w)
                pos += rows * w
            return out
        self.xin, self.specin, self.nfwd, self.nbwd = self.x, lay(self.spec), rows * nh, rows * n
        self.natural_fwd, self.natural_bwd = unlay, lambda b: b.reshape(rows, n)

    def plans(self, eng):
        from mpi4py_fft_amd import _lib
        prec, nh = _lib.precision_of(self.dt), self.n // 2 + 1
        hf = eng.plan_create((self.rows, self.n), (self.rows, nh), (1,), _lib.R2C, prec)
        hb = eng.plan_create((self.rows, nh), (self.rows, self.n), (1,), _lib.C2R, prec)
        assert eng.plan_set_split(hf, 1, 3) and eng.plan_set_split(hb, 0, 3)
        return hf, hb


class TiledRows(Raw):
    """gfft_plan_set_tiles on a row plan: the transformed axis tile-major, [slab i0][tile][row i1][tile entries]."""
    def __init__(self, dt, tile, n, n0):
        self.family, self.tile, self.n0, self.n1 = 'tile-major rows', tile, n0, 8
        n1 = self.n1
        self.prepare((n0, n1, n), 2, dt)
        lay = lambda v: np.ascontiguousarray(v.reshape(n0, n1, n // tile, tile).transpose(0, 2, 1, 3))
        self.xin, self.specin, self.nfwd, self.nbwd = self.x, lay(self.spec), n0 * n1 * n, n0 * n1 * n
        self.natural_fwd = lambda b: b.reshape(n0, n // tile, n1, tile).transpose(0, 2, 1, 3).reshape(n0, n1, n)
        self.natural_bwd = lambda b: b.reshape(n0, n1, n)

    def plans(self, eng):
        from mpi4py_fft_amd import _lib
        prec, n, n0, n1, tile = _lib.precision_of(self.dt), self.n, self.n0, self.n1, self.tile
        slab, tS = n1 * n, n1 * tile
        hf = eng.plan_create_guru(prec, -1, (n, 1, 1), [(n0, n1 * n, slab), (n1, n, tile)])
        hb = eng.plan_create_guru(prec, +1, (n, 1, 1), [(n0, slab, n1 * n), (n1, tile, n)])
        assert hf is not None and hb is not None and eng.plan_set_tiles(hf, 1, tile, tS) and eng.plan_set_tiles(hb, 0, tile, tS)
        return hf, hb


class TiledCols(Raw):
    """gfft_plan_set_tiles on a strided plan: adjacent columns tile-major, [i0][W / tile][n][tile]."""
    def __init__(self, dt, tile, n, W, n0):
        self.family, self.tile, self.W, self.n0 = 'tile-major columns', tile, W, n0
        self.prepare((n0, n, W), 1, dt)
        lay = lambda v: np.ascontiguousarray(v.reshape(n0, n, W // tile, tile).transpose(0, 2, 1, 3))
        self.xin, self.specin, self.nfwd, self.nbwd = self.x, lay(self.spec), n0 * n * W, n0 * n * W
        self.natural_fwd = lambda b: b.reshape(n0, W // tile, n, tile).transpose(0, 2, 1, 3).reshape(n0, n, W)
        self.natural_bwd = lambda b: b.reshape(n0, n, W)

    def plans(self, eng):
        from mpi4py_fft_amd import _lib
        prec, n, n0, W, tile = _lib.precision_of(self.dt), self.n, self.n0, self.W, self.tile
        hf = eng.plan_create_guru(prec, -1, (n, W, tile), [(n0, n * W, n * W), (W, 1, 1)])
        hb = eng.plan_create_guru(prec, +1, (n, tile, W), [(n0, n * W, n * W), (W, 1, 1)])
        assert hf is not None and hb is not None and eng.plan_set_tiles(hf, 1, tile, n * tile) and eng.plan_set_tiles(hb, 0, tile, n * tile)
        return hf, hb


class FlatCols(Raw):
    """gfft_plan_set_flat on a 33-wide strided plan: tiles over the flattened (row, column) index, the input rows stored as a body
    of 32 columns plus the leftover column; both directions read that layout and write the natural (n, n1, W) array."""
    def __init__(self, dt, W, n, n1):
        self.family, self.W, self.n1 = 'flat %d-wide' % W, W, n1
        self.prepare((n, n1, W), 0, dt)
        lw = 128 // np.dtype(dt).itemsize
        self.bw = bw = W - W % lw
        self.E = E = n1 * W + 5

        def lay(v):
            buf = np.zeros((n, E), dtype=v.dtype)
            buf[:, :n1 * bw] = v[:, :, :bw].reshape(n, n1 * bw)
            buf[:, n1 * bw:n1 * W] = v[:, :, bw:].reshape(n, n1 * (W - bw))
            return buf
        self.xin, self.specin, self.nfwd, self.nbwd = lay(self.x), lay(self.spec), n * n1 * W, n * n1 * W
        self.natural_fwd = self.natural_bwd = lambda b: b.reshape(n, n1, W)

    def plans(self, eng):
        from mpi4py_fft_amd import _lib
        prec, n, n1, W, bw, E = _lib.precision_of(self.dt), self.n, self.n1, self.W, self.bw, self.E
        hs = [eng.plan_create_guru(prec, kind, (n, E, n1 * W), [(1, 0, 0), (n1, bw, W), (W, 1, 1)]) for kind in (-1, +1)]
        assert all(h is not None and eng.plan_set_flat(h, bw, n1 * bw, W - bw) for h in hs)
        return hs


@pytest.mark.parametrize('dt', ['D', 'F'])
def test_layout_adapters_walk(dt, walk):
    rdt = dt.lower()
    tile = 16 if dt == 'D' else 32
    _walk_case(walk, lambda rows: SplitRows(dt, 1024, 2, rows), 197)
    _walk_case(walk, lambda rows: SplitRows(dt, 256, 4, rows), 197)
    _walk_case(walk, lambda rows: UnevenRealRows(rdt, 256 if dt == 'D' else 512, rows), 197)
    _walk_case(walk, lambda n0: TiledRows(dt, tile, 256 if dt == 'D' else 512, n0), 25)            # x 8 rows per slab
    _walk_case(walk, lambda n0: TiledCols(dt, tile, 256, 4 * tile, n0), 7)
    _walk_case(walk, lambda n1: FlatCols(dt, 33, 256, n1), 23)
