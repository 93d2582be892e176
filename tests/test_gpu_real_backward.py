"""c2r on spectra that are NOT Hermitian-clean.

Every other c2r of the suite is fed the output of a forward transform or of numpy's rfft*: the imaginary parts of X[0] and
X[n/2] are zero there.  In a pseudo-spectral solver they are not after a nonlinear term, and a 3-D irfftn runs its c2c
axes first, so the k2 = 0 and k2 = N/2 columns reaching the 1-D c2r are complex whenever the user's spectrum is not exactly
Hermitian.  fft_pow2_body.inc promises "imaginary parts of X[0] and X[N] are ignored, as FFTW's c2r does"; each path drops
them in code of its own (the packed body, its UNEVEN / SYS_LD / TRUNC_LOAD branches, tile_load_pad, trunc_kernel, the
mirror load of the full-length lines, embed_kernel), so a leak would make the result depend on which kernel the planner
picked, i.e. on the size.

Input: a seeded complex Gaussian half-spectrum, no entry cleaned (cases.dirty_spectrum).  Reference: the oracle built for
'd' on the input widened to complex128 (numpy runs irfft of complex64 in single precision).  Comparator:
cases.assert_close, the 2 eps log2(points) guard -- tests/test_real_backward_host.py shows, without a GPU, that it rejects
both ways of leaking by more than a factor of 100 at every rows length.  The packed rows promise more than rounding level:
the two parts are ignored bit for bit, so the 1-D cases that run them compare against the same call on the cleaned spectrum
with np.array_equal.  (The fused [strided -> c2r rows] pair cannot be held to that from outside: what its rows ignore is the
output of its own strided pass, and cleaning the pair's input instead changes the answer.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cases
from oracle import pfft_oracle as O

LINES = 5


def _reference(X, shape, axes, **kw):
    return O.OFFT(shape, axes, 'd', **kw).backward(X.astype('D'))


def _offset_array(shape, dtype, skip):
    """A contiguous device array whose first element lies `skip` elements into its allocation."""
    import torch
    from mpi4py_fft_amd.array import DeviceArray, torch_dtype
    count = int(np.prod(shape))
    t = torch.zeros(count + skip, dtype=torch_dtype(np.dtype(dtype)), device='cuda')[skip:].view(*shape)
    return DeviceArray(shape, dtype, tensor=t)


def _rows_c2r(X, n, dt, skip=0):
    """fftw.irfftn(c, s=(n,), axes=(1,)) of the rows of X; returns (result, gfft_plan_describe)."""
    from mpi4py_fft_amd import fftw
    c = _offset_array(X.shape, dt.upper(), skip)
    out = _offset_array((X.shape[0], n), dt, 2 * skip)
    if skip:
        assert c.data_ptr % 32 in (8, 16) and out.data_ptr % 32 in (8, 16), (c.data_ptr, out.data_ptr)
    c[...] = X
    plan = fftw.irfftn(c, s=(n,), axes=(1,), output_array=out)
    text = plan._eng.plan_describe(plan._plan)
    got = np.asarray(plan()).copy()
    assert np.array_equal(np.asarray(c), X)            # (the input is left as it was)
    plan.destroy()
    return got, text


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('n,path', cases.REAL_ROWS)
def test_rows(n, path, dt):
    X = cases.dirty_spectrum((LINES, n // 2 + 1), dt, 100 + n)
    got, text = _rows_c2r(X, n, dt)
    assert cases.real_path([text]) == path, text
    cases.assert_close(got.astype('d'), _reference(X, (LINES, n), (1,)), dt, LINES * n, (n, path, dt))
    if path == 'packed':
        clean, _ = _rows_c2r(cases.clean_edges(X, n), n, dt)
        assert np.array_equal(got, clean), (n, dt, np.abs(got - clean).max())


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('n', [64, 1536, 1000, 480, 48, 34, 121, 9216, 521])
def test_rows_from_a_base_pointer_off_32_byte_alignment(n, dt):
    """Both arrays start one complex entry (8 bytes in fp32, 16 in fp64) into their allocations."""
    X = cases.dirty_spectrum((LINES, n // 2 + 1), dt, 100 + n)
    got, text = _rows_c2r(X, n, dt, skip=1)
    cases.assert_close(got.astype('d'), _reference(X, (LINES, n), (1,)), dt, LINES * n, (n, dt))
    if cases.real_path([text]) == 'packed':
        clean, _ = _rows_c2r(cases.clean_edges(X, n), n, dt, skip=1)
        assert np.array_equal(got, clean), (n, dt)


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('n', [16, 64, 48, 40, 22, 121, 521])
def test_strided_axis(n, dt):
    from mpi4py_fft_amd import fftw, asdevice
    W = 6
    X = cases.dirty_spectrum((n // 2 + 1, W), dt, 200 + n)
    plan = fftw.irfftn(asdevice(X), s=(n,), axes=(0,))
    got = np.asarray(plan()).copy()
    plan.destroy()
    cases.assert_close(got.astype('d'), _reference(X, (n, W), (0,)), dt, n * W, (n, dt))


@pytest.fixture
def schedule():
    from mpi4py_fft_amd import _lib

    def select(on):
        _lib.set_option('fused3', int(on))
        _lib.set_option('fused3_min_mib', 0 if on else 32)      # the 3-D schedule whatever the size
    yield select
    _lib.set_option('fused3', 1)
    _lib.set_option('fused3_min_mib', 32)


@pytest.mark.parametrize('on', [True, False], ids=['schedule', 'per-axis'])
@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', [(16, 16, 32), (32, 16, 64), (12, 10, 21), (24, 16, 20)])
def test_whole_3d_irfftn(shape, dt, on, schedule):
    """The c2c axes run first: the columns k2 = 0 and k2 = N/2 reaching the c2r rows are complex."""
    from mpi4py_fft_amd import fftw, asdevice
    schedule(on)
    X = cases.dirty_spectrum(shape[:2] + (shape[2] // 2 + 1,), dt, 300 + shape[2])
    plan = fftw.irfftn(asdevice(X), s=shape, axes=(0, 1, 2))
    text = plan._eng.plan_describe(plan._plan)
    # the one-rank 3-D schedule takes register-kernel lengths only
    assert ('3-D schedule' in text) == (on and shape in ((16, 16, 32), (32, 16, 64))), text
    got = np.asarray(plan()).copy()
    plan.destroy()
    cases.assert_close(got.astype('d'), _reference(X, shape, (0, 1, 2)), dt, int(np.prod(shape)), (shape, dt, on))


# (padded shape, axis, fused into the transform?): the kept length is round(n / 1.5)
#   96 -> 64 (even) and 32 -> 21 (odd), fused zero-padding load; 40 -> 27, 5^c 2^k: the separate gfft_pad kernel, as the
#   generic length 66 -> 44 (gfft_pad's real arm on an even kept length: the last kept entry is taken .real, as the
#   reference's padding does); 96 -> 64 and 48 -> 32 along a strided axis
PADDED = [((6, 96), 1, True), ((6, 32), 1, True), ((6, 40), 1, False), ((6, 66), 1, False), ((96, 6), 0, None), ((48, 6), 0, None)]


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape,axis,fused', PADDED)
def test_padded_backward(shape, axis, fused, dt):
    from mpi4py_fft_amd import FFT, asdevice
    fft = FFT(shape, axis, dtype=dt, padding=1.5)
    ref = O.OFFT(shape, axis, 'd', padding=1.5)
    if fused is not None:
        assert fft._fused_trunc == fused, (shape, axis, dt)
    X = cases.dirty_spectrum(ref.out_shape, dt, 400 + shape[axis])
    assert tuple(fft.backward.input_array.shape) == ref.out_shape
    got = np.asarray(fft.backward(asdevice(X))).copy()
    fft.destroy()
    cases.assert_close(got.astype('d'), ref.backward(X.astype('D')), dt, int(np.prod(shape)), (shape, axis, dt))


def _split_case(dt):
    return dict(d=(256, 3, 16), f=(64, 2, 32))[dt]          # test_gpu_layouts.py's shapes: n, blocks, tile


def _run_split(X, n, dt, prepare, relay):
    """A C2R rows plan of X's rows with an exchange-buffer layout set by `prepare(engine, plan)` on its input side, the
    buffer filled from `relay(X)`."""
    import torch
    from mpi4py_fft_amd import _lib
    eng = _lib.engine()
    rows, nh = X.shape
    h = eng.plan_create((rows, nh), (rows, n), (1,), _lib.C2R, _lib.precision_of(dt))
    assert prepare(eng, h)
    assert 'packed-real' in eng.plan_describe(h), eng.plan_describe(h)
    buf = torch.from_numpy(np.ascontiguousarray(relay(X))).cuda()
    out = torch.zeros((rows, n), dtype=torch.float64 if dt == 'd' else torch.float32, device='cuda')
    eng.execute_ptr(h, buf.data_ptr(), out.data_ptr(), 1.0)
    torch.cuda.synchronize()
    eng.plan_destroy(h)
    return out.cpu().numpy()


@pytest.mark.parametrize('slabs', [False, True], ids=['split', 'split-slabs'])
@pytest.mark.parametrize('dt', ['d', 'f'])
def test_split_layouts(dt, slabs):
    """plan_set_split / plan_set_split_slabs on the input of a C2R plan: uneven blocks of the half-spectrum axis (the
    Nyquist entry sits alone at the end of the last block), filled from the non-clean spectrum re-laid on the host."""
    from mpi4py_fft_amd.pencil import _blockdist
    n, p, tile = _split_case(dt)
    n0, n1, nh = 3, 4, n // 2 + 1
    rows = n0 * n1
    X = cases.dirty_spectrum((rows, nh), dt, 500 + n)

    def relay(S):
        parts = []
        for r in range(p):
            w, start = _blockdist(nh, p, r)
            blk = S[:, start:start + w]
            if slabs:
                # [block][slab i0][rows of the body, tile-aligned][rows of the leftover columns]
                bw = w - w % tile
                blk = blk.reshape(n0, n1, w)
                blk = np.concatenate([blk[:, :, :bw].reshape(n0, -1), blk[:, :, bw:].reshape(n0, -1)], axis=1)
            parts.append(blk.reshape(-1))
        return np.concatenate(parts)

    def prepare(eng, h):
        return eng.plan_set_split_slabs(h, 0, p, n1, tile) if slabs else eng.plan_set_split(h, 0, p)
    got = _run_split(X, n, dt, prepare, relay)
    cases.assert_close(got.astype('d'), _reference(X, (rows, n), (1,)), dt, rows * n, (dt, slabs))
    clean = _run_split(cases.clean_edges(X, n), n, dt, prepare, relay)
    assert np.array_equal(got, clean), (dt, slabs, np.abs(got - clean).max())


@pytest.fixture
def small_ring():
    """test_gpu_real_pairs.py's: a hand-off ring of 4 planes, the producer 2 ahead, so that 16 planes already fuse."""
    from mpi4py_fft_amd import _lib
    _lib.set_option('fuse2_ring', 4)
    _lib.set_option('fuse2_lag', 2)
    yield
    _lib.set_option('fuse2_ring', 0)
    _lib.set_option('fuse2_lag', 0)
    _lib.set_option('fuse2_kinds', 2046)
    _lib.set_option('fuse2_f32', 1)


@pytest.mark.parametrize('dt,n1,n2,planes,blocks', [('d', 1024, 1024, 16, 1), ('f', 1024, 1024, 16, 2)])
def test_fused_strided_then_c2r_rows_pair(dt, n1, n2, planes, blocks, small_ring):
    """gfft_plan_create_guru2_real(C2R): [strided c2c from the blocks -> c2r rows] as one launch, against the float64
    reference and against the same plan as two launches."""
    import torch
    from mpi4py_fft_amd import _lib
    eng = _lib.engine()
    prec = _lib.precision_of(dt)
    _lib.set_option('fuse2_kinds', 2046)
    if dt == 'f':
        _lib.set_option('fuse2_f32', 2)                    # (the real fp32 pairs are off by default)
    H, nb = n2 // 2 + 1, n1 // blocks
    E = nb * H
    bstride = planes * E
    X = cases.dirty_spectrum((planes, n1, H), dt, 600)
    buf = torch.from_numpy(np.ascontiguousarray(X.reshape(planes, blocks, E).transpose(1, 0, 2))).cuda()
    ref = _reference(X, (planes, n1, n2), (1, 2))

    def run(launches):
        h = eng.plan_create_guru2_real(prec, _lib.C2R, (n1, H, n2), (n2, 1, 1), (planes, E, n1 * n2), blocks, bstride, 1, 0)
        assert h is not None and eng.plan_cost(h)[2] == launches, eng.plan_describe(h)
        out = torch.full((planes, n1, n2), float('nan'), dtype=torch.float64 if dt == 'd' else torch.float32, device='cuda')
        eng.execute_ptr(h, buf.data_ptr(), out.data_ptr(), 1.0)
        torch.cuda.synchronize()
        _lib.check_async()
        eng.plan_destroy(h)
        return out.cpu().numpy()
    one = run(1)
    _lib.set_option('fuse2_kinds', 2046 & ~(512 | 1024))   # the real slab pairs off: two stand-alone launches
    two = run(2)
    nelem = planes * n1 * n2
    cases.assert_close(one.astype('d'), ref, dt, nelem, (dt, 'one launch'))
    cases.assert_close(two.astype('d'), ref, dt, nelem, (dt, 'two launches'))
    cases.assert_close(one.astype('d'), two.astype('d'), dt, nelem, (dt, 'one launch against two'))


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('shape', [(24, 16, 20), (12, 10, 21)])
@pytest.mark.parametrize('P,grid', [(1, None), (2, None), (4, None), (4, [4, 1, 1])], ids=['P1', 'P2', 'P4-pencil', 'P4-slab'])
def test_pfft_backward(P, grid, shape, dt):
    kw = {} if grid is None else dict(grid=grid)
    cases.check_pfft_backward_vs_oracle(P, shape, dt, **kw)


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_pfft_backward_padded(dt):
    cases.check_pfft_backward_vs_oracle(2, (24, 16, 20), dt, padding=[1.5, 1.5, 1.5])
