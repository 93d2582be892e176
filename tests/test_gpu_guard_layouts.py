"""Guard bands round the exchange-buffer layouts, the 3-D schedules and the on-chip planes (see tests/test_gpu_guard_bands.py
for the method and for what it does not cover).

A split, tile-major or flat layout puts entry e of a line somewhere else than e: a last block, tile or leftover column
addressed one unit too far leaves the buffer.  Here the payload IS the exchange buffer, exactly as large as the layout says,
on the smallest case of each test of tests/test_gpu_layouts.py; the geometry of the layouts is that of
tests/test_gpu_tile_walk.py (its Raw cases), the slab-wise uneven blocks of packed-real rows are restated here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import test_gpu_tile_walk as W
from tests.guards import four_ways, serial_case


class SlabRows(W.Raw):
    """gfft_plan_set_split_slabs on packed-real rows (n0 slabs of n1 rows): block b of the n / 2 + 1 entries, width w_b, holds per
    slab its rows cut to the body columns -- w_b rounded down to whole tiles --, [row][body], then the leftover columns
    [row][w_b - body]; a block's slabs back to back, the blocks one after the other."""
    def __init__(self, dt, n, p, tile, n0=3, n1=4):
        from mpi4py_fft_amd.pencil import _blockdist
        self.family, self.p, self.tile, self.n0, self.n1 = 'slab-wise %d uneven blocks' % p, p, tile, n0, n1
        rows, nh = n0 * n1, n // 2 + 1
        self.prepare((rows, n), 1, dt)
        cuts = [_blockdist(nh, p, r) for r in range(p)]              # (width, start)

        def lay(v):
            out = []
            for w, s in cuts:
                blk, bw = v[:, s:s + w].reshape(n0, n1, w), w - w % tile
                out.append(np.concatenate([blk[:, :, :bw].reshape(n0, -1), blk[:, :, bw:].reshape(n0, -1)], axis=1).reshape(-1))
            return np.concatenate(out)

        def unlay(b):
            out, pos = np.empty((rows, nh), dtype=b.dtype), 0
            for w, s in cuts:
                bw = w - w % tile
                slab = b[pos:pos + rows * w].reshape(n0, n1 * w)
                blk = np.concatenate([slab[:, :n1 * bw].reshape(n0, n1, bw), slab[:, n1 * bw:].reshape(n0, n1, w - bw)], axis=2)
                out[:, s:s + w] = blk.reshape(rows, w)
                pos += rows * w
            return out
        assert np.array_equal(unlay(lay(self.spec)), self.spec)
        self.xin, self.specin, self.nfwd, self.nbwd = self.x, lay(self.spec), rows * nh, rows * n
        self.natural_fwd, self.natural_bwd = unlay, lambda b: b.reshape(rows, n)

    def plans(self, eng):
        from mpi4py_fft_amd import _lib
        prec, nh, rows = _lib.precision_of(self.dt), self.n // 2 + 1, self.n0 * self.n1
        hf = eng.plan_create((rows, self.n), (rows, nh), (1,), _lib.R2C, prec)
        hb = eng.plan_create((rows, nh), (rows, self.n), (1,), _lib.C2R, prec)
        assert eng.plan_set_split_slabs(hf, 1, self.p, self.n1, self.tile) and eng.plan_set_split_slabs(hb, 0, self.p, self.n1, self.tile)
        return hf, hb


class TiledBlockRows(W.Raw):
    """gfft_plan_set_tiles on a row plan whose transformed axis is also cut into p blocks (gfft_plan_create_guru's blocks):
    [block][slab i0][tile][row i1][tile entries], the layout of tests/test_gpu_layouts.py's row plans."""
    def __init__(self, dt, tile, n, p, n0=3, n1=8):
        self.family, self.tile, self.p, self.n0, self.n1 = 'tile-major rows in %d blocks' % p, tile, p, n0, n1
        self.prepare((n0, n1, n), 2, dt)
        w = n // p
        lay = lambda v: np.ascontiguousarray(v.reshape(n0, n1, p, w // tile, tile).transpose(2, 0, 3, 1, 4))
        self.xin, self.specin, self.nfwd, self.nbwd = self.x, lay(self.spec), n0 * n1 * n, n0 * n1 * n
        self.natural_fwd = lambda b: b.reshape(p, n0, w // tile, n1, tile).transpose(1, 3, 0, 2, 4).reshape(n0, n1, n)
        self.natural_bwd = lambda b: b.reshape(n0, n1, n)
        assert np.array_equal(self.natural_fwd(lay(self.spec).reshape(-1)), self.spec)

    def plans(self, eng):
        from mpi4py_fft_amd import _lib
        prec, n, n0, n1, tile, p = _lib.precision_of(self.dt), self.n, self.n0, self.n1, self.tile, self.p
        w = n // p
        bstride, slab, tS = n0 * n1 * w, n1 * w, n1 * tile
        hf = eng.plan_create_guru(prec, -1, (n, 1, 1), [(n0, n1 * n, slab), (n1, n, tile)], 1, 0, p, bstride)
        hb = eng.plan_create_guru(prec, +1, (n, 1, 1), [(n0, slab, n1 * n), (n1, tile, n)], p, bstride, 1, 0)
        assert hf is not None and hb is not None and eng.plan_set_tiles(hf, 1, tile, tS) and eng.plan_set_tiles(hb, 0, tile, tS)
        return hf, hb


def raw_case(case):
    """A layout case at the C ABI (gfft_execute on the payloads' addresses): forward into, backward out of the exchange buffer."""
    from mpi4py_fft_amd import _lib
    eng = _lib.engine()
    hs = case.plans(eng)
    try:
        assert all(eng.plan_describe(h).count('kernel=regs-') == 1 for h in hs), [eng.plan_describe(h) for h in hs]
        what = ('layout', case.family, case.n, case.dt)
        four_ways(lambda a, b: eng.execute_ptr(hs[0], a.data_ptr, b.data_ptr, 1.0), np.ascontiguousarray(case.xin).reshape(-1),
                  (case.nfwd,), case.spec.dtype, case.want, case.dt, case.n, what + ('forward',), natural=case.natural_fwd, line_in=case.n,
                  line_out=case.n)
        four_ways(lambda a, b: eng.execute_ptr(hs[1], a.data_ptr, b.data_ptr, case.scale_b), np.ascontiguousarray(case.specin).reshape(-1),
                  (case.nbwd,), case.x.dtype, case.wantb, case.dt, case.n, what + ('backward',), natural=case.natural_bwd, line_in=case.n,
                  line_out=case.n)
    finally:
        for h in hs:
            eng.plan_destroy(h)


@pytest.mark.parametrize('dt', ['D', 'F'])
def test_layout_adapters(dt):
    rdt = dt.lower()
    tile = 16 if dt == 'D' else 32
    raw_case(W.SplitRows(dt, 1024, 2, 19))
    raw_case(W.SplitRows(dt, 256, 4, 19))
    raw_case(W.SplitRows(dt, 256, 4, 1))
    raw_case(W.UnevenRealRows(rdt, 256 if dt == 'D' else 512, 19))
    raw_case(W.TiledRows(dt, tile, 256 if dt == 'D' else 512, 3))            # x 8 rows per slab
    for p in (2, 4):
        raw_case(TiledBlockRows(dt, tile, 256 if dt == 'D' else 512, p))
    raw_case(W.TiledCols(dt, tile, 256, 3 * tile, 3))
    raw_case(W.FlatCols(dt, 17 if dt == 'D' else 33, 128 if dt == 'D' else 256, 6))
    raw_case(SlabRows(rdt, 256, 3, 16) if dt == 'D' else SlabRows(rdt, 64, 2, 32))


# ---- 3-D schedules and on-chip planes: the shapes of tests/test_gpu_tile_walk.py ----------------------------------------------
@pytest.mark.parametrize('shape,dt', [((64, 32, 128), 'D'), ((48, 40, 64), 'D'), ((32, 64, 66), 'd'), ((32, 64, 66), 'f')],
                         ids=lambda v: 'x'.join(str(s) for s in v) if isinstance(v, tuple) else v)
def test_3d_schedules(shape, dt):
    serial_case(shape, (0, 1, 2), dt, ('3-D schedule', shape, dt), in_place=dt == 'D', offsets=())


@pytest.mark.parametrize('dt', ['D', 'F'])
@pytest.mark.parametrize('n', [32, 64])
def test_planes_on_chip(n, dt):
    def path(text):
        assert all('planes on chip' in t for t in text), text
    for planes in (11, 1):
        serial_case((planes, n, n), (1, 2), dt, ('planes on chip', planes, n, dt), path=path if planes > 1 else None,
                    in_place=True, offsets=())
