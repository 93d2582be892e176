"""What gfft_execute refuses on a good plan (include/gfft.h): d_in == d_out on a plan whose two sides are laid out differently,
and a base that is not aligned as the contract asks -- the exact status and gfft_last_error() text, and that a refused call
enqueues nothing (the output keeps its fill).  The Python layer must not send such a call: a misaligned view is copied.
Every address handed over lies inside an allocation large enough for the plan, whatever the call decides."""
import ctypes

import numpy as np
import pytest
import torch

from mpi4py_fft_amd import _lib

pytestmark = pytest.mark.gpu

FWD, BWD, R2C, C2R = _lib.C2C_FORWARD, _lib.C2C_BACKWARD, _lib.R2C, _lib.C2R
IN_PLACE = (b'in-place execution needs the same layout on both sides (this plan re-lays one side out: a tile would overwrite input '
            b'that another tile has yet to read)')


def _execute(h, ptr_in, ptr_out, scale=1.0):
    lib = _lib.lib()
    rc = lib.gfft_execute(h, ctypes.c_void_p(ptr_in), ctypes.c_void_p(ptr_out), scale, _lib.current_stream())
    return rc, lib.gfft_last_error()


def _rows(eng, n=64, rows=8, kind=FWD):
    return eng.plan_create((rows, n), (rows, n), (1,), kind, 8)


def _split_out(eng):
    h = _rows(eng)
    assert eng.plan_set_split(h, 1, 2)
    return h


def _split_in(eng):
    h = _rows(eng, kind=BWD)
    assert eng.plan_set_split(h, 0, 4)
    return h


def _tiled_rows(eng):
    """8 rows of 256 points into [tile][row][16 entries]: 2048 entries on both sides (tests/test_gpu_layouts.py)"""
    n, n1, tile = 256, 8, 16
    h = eng.plan_create_guru(8, -1, (n, 1, 1), [(1, n1 * n, n1 * n), (n1, n, tile)])
    assert h is not None and eng.plan_set_tiles(h, 1, tile, n1 * tile)
    return h


def _tiled_cols(eng):
    """256 x 48 points read from [48 / 16][256][16 columns]: 12288 entries on both sides (tests/test_gpu_layouts.py)"""
    n, w, tile = 256, 48, 16
    h = eng.plan_create_guru(8, -1, (n, tile, w), [(1, n * w, n * w), (w, 1, 1)])
    assert h is not None and eng.plan_set_tiles(h, 0, tile, n * tile)
    return h


def _flat_body(eng):
    """64 x 4 x 17 points, the input rows as 16 body columns plus the leftover one: 4352 entries on both sides"""
    n, n1, w, bw = 64, 4, 17, 16
    h = eng.plan_create_guru(8, -1, (n, n1 * w, n1 * w), [(1, 0, 0), (n1, bw, w), (w, 1, 1)])
    assert h is not None and eng.plan_set_flat(h, bw, n1 * bw, w - bw)
    return h


def _guru_blocks(eng):
    h = eng.plan_create_guru(8, -1, (64, 1, 1), [(8, 64, 32)], 1, 0, 2, 8 * 32)
    assert h is not None
    return h


def _truncating(eng):
    h = _rows(eng)
    assert eng.plan_set_truncation(h, 43)
    return h


RELAID = {'split output': _split_out, 'split input': _split_in, 'tile-major rows': _tiled_rows, 'tile-major columns': _tiled_cols,
          'flat with a body width': _flat_body, 'guru blocks on one side': _guru_blocks, 'fused truncation': _truncating}


@pytest.mark.parametrize('name', list(RELAID))
def test_in_place_is_refused_on_a_plan_with_a_re_laid_out_side(name):
    eng = _lib.engine()
    h = RELAID[name](eng)
    try:
        buf = torch.full((16384,), 7.0, dtype=torch.complex128, device='cuda')          # no plan above spans more
        rc, err = _execute(h, buf.data_ptr(), buf.data_ptr())
        torch.cuda.synchronize()
        assert (rc, err) == (-1, IN_PLACE), (name, rc, err)
        assert bool((buf == 7.0).all()), (name, 'a refused call wrote')
        # ... and out of place the same plan runs
        out = torch.zeros_like(buf)
        rc, err = _execute(h, buf.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (name, rc, err)
    finally:
        eng.plan_destroy(h)


def test_in_place_runs_where_both_sides_have_the_same_layout():
    """natural rows, and the same split on both sides: every tile writes the addresses it read -- the out-of-place bits"""
    eng = _lib.engine()
    x = torch.randn(8, 64, dtype=torch.complex128, generator=torch.Generator().manual_seed(4)).cuda()
    for both in (False, True):
        h = _rows(eng)
        if both:
            assert eng.plan_set_split(h, 0, 2) and eng.plan_set_split(h, 1, 2)
        out, inplace = torch.zeros_like(x), x.clone()
        assert _execute(h, x.data_ptr(), out.data_ptr())[0] == 0 and _execute(h, inplace.data_ptr(), inplace.data_ptr())[0] == 0
        torch.cuda.synchronize()
        eng.plan_destroy(h)
        assert torch.equal(torch.view_as_real(out).view(torch.int64), torch.view_as_real(inplace).view(torch.int64)), both


# (plan: shape in, shape out, axes, kind, precision), byte offsets of d_in / d_out, the refusal
ELEMENT = b' bytes (one element of the array)'
MISALIGNED = [
    (((8, 64), (8, 64), (1,), FWD, 8), 8, 0, b'd_in must be aligned to 16' + ELEMENT),
    (((8, 64), (8, 64), (1,), FWD, 8), 0, 8, b'd_out must be aligned to 16' + ELEMENT),
    (((8, 64), (8, 64), (1,), FWD, 4), 4, 0, b'd_in must be aligned to 8' + ELEMENT),
    (((8, 64), (8, 33), (1,), R2C, 8), 4, 0, b'd_in must be aligned to 8' + ELEMENT),
    (((8, 64), (8, 33), (1,), R2C, 8), 0, 8, b'd_out must be aligned to 16' + ELEMENT),
    (((8, 33), (8, 64), (1,), C2R, 4), 0, 2, b'd_out must be aligned to 4' + ELEMENT),
    (((8, 33), (8, 64), (1,), C2R, 4), 4, 0, b'd_in must be aligned to 8' + ELEMENT),
]


@pytest.mark.parametrize('case', MISALIGNED, ids=[str(i) for i in range(len(MISALIGNED))])
def test_a_base_off_its_element_alignment_is_refused(case):
    (sin, sout, axes, kind, prec), off_in, off_out, message = case
    eng = _lib.engine()
    h = eng.plan_create(sin, sout, axes, kind, prec)
    try:
        a = torch.zeros(8 * 64 * 16 + 64, dtype=torch.uint8, device='cuda')
        b = torch.full((8 * 64 * 16 + 64,), 0x5a, dtype=torch.uint8, device='cuda')
        rc, err = _execute(h, a.data_ptr() + off_in, b.data_ptr() + off_out)
        torch.cuda.synchronize()
        assert (rc, err) == (-1, message), (rc, err)
        assert bool((b == 0x5a).all()), 'a refused call wrote'
    finally:
        eng.plan_destroy(h)


def test_r2r_plans_take_element_aligned_bases():
    """... and a real array needs no more than that: one real of offset on both sides of a real-to-real plan, same bits"""
    eng = _lib.engine()
    h = eng.plan_create_r2r((8, 64), (1,), (5,), 8)
    try:
        x = torch.randn(8 * 64 + 1, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).cuda()
        out0, out1 = torch.zeros(8 * 64, dtype=torch.float64, device='cuda'), torch.zeros(8 * 64 + 1, dtype=torch.float64, device='cuda')
        aligned = x[1:].clone()
        assert aligned.data_ptr() % 16 == 0 and (x.data_ptr() + 8) % 16 == 8
        assert _execute(h, aligned.data_ptr(), out0.data_ptr())[0] == 0
        assert _execute(h, x.data_ptr() + 8, out1.data_ptr() + 8)[0] == 0
        torch.cuda.synchronize()
        assert torch.equal(out0.view(torch.int64), out1[1:].view(torch.int64))
    finally:
        eng.plan_destroy(h)


@pytest.fixture
def small_ring():
    """the fused real pair of 16 planes (tests/test_gpu_real_pairs.py): a hand-off ring of 4 planes, the producer 2 ahead"""
    _lib.set_option('fuse2_ring', 4)
    _lib.set_option('fuse2_lag', 2)
    yield
    _lib.set_option('fuse2_ring', 0)
    _lib.set_option('fuse2_lag', 0)


def test_a_fused_real_pair_asks_for_a_complex_pair_on_its_real_side(small_ring):
    """the one family that needs more than its element's alignment (non-temporal streams typed as two reals): refused, not run"""
    eng = _lib.engine()
    n, planes, H = 1024, 16, 513
    hf = eng.plan_create_guru2_real(8, R2C, (n, n, H), (n, 1, 1), (planes, n * n, n * H))
    hb = eng.plan_create_guru2_real(8, C2R, (n, H, n), (n, 1, 1), (planes, n * H, n * n))
    try:
        assert hf is not None and hb is not None and eng.plan_cost(hf)[2] == 1 and eng.plan_cost(hb)[2] == 1, 'the pairs are not fused'
        real = torch.empty(planes * n * n + 2, dtype=torch.float64, device='cuda')
        spec = torch.empty(planes * n * H, dtype=torch.complex128, device='cuda')
        pair = b' must be aligned to 16 bytes (a fused real pass pair addresses its real side as complex pairs)'
        assert _execute(hf, real.data_ptr() + 8, spec.data_ptr()) == (-1, b'd_in' + pair)
        assert _execute(hb, spec.data_ptr(), real.data_ptr() + 8) == (-1, b'd_out' + pair)
        torch.cuda.synchronize()
    finally:
        eng.plan_destroy(hf)
        eng.plan_destroy(hb)


def test_python_layer_copies_a_view_the_contract_may_exclude():
    """fftw.FFT.__call__ on a real view that starts at an odd element: not run directly but copied into the planned array
    (which then holds it), with the bits of the aligned run; an aligned array is read where it lies."""
    from mpi4py_fft_amd import asdevice, fftw
    from mpi4py_fft_amd.array import DeviceArray
    x = np.random.default_rng(6).standard_normal((19, 64))
    plan = fftw.rfftn(fftw.aligned((19, 64), dtype='d', fill=0), axes=(1,))
    want = np.asarray(plan(asdevice(x))).copy()
    assert not np.asarray(plan.input_array).any()                         # read in place: the planned input is untouched
    raw = torch.zeros(19 * 64 + 1, dtype=torch.float64, device='cuda')
    view = DeviceArray((19, 64), 'd', tensor=raw[1:].view(19, 64))
    view[...] = x
    assert view.data_ptr % 16 == 8 and not fftw.pair_aligned(view)
    got = np.asarray(plan(view)).copy()
    assert np.array_equal(np.asarray(plan.input_array), x)                # copied
    assert np.array_equal(got.view('d'), want.view('d'))
    plan.destroy()
