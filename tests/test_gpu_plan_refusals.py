"""What the plan API refuses once a device is there: the guru creators' length, block-count and batch checks and every
gfft_plan_set_* refusal -- the exact status code and gfft_last_error() text (-2 makes the Python side fall back to pack / unpack
kernels or staged passes without a word, -1 raises) -- and that a refused setter leaves its plan as it was: the plan computes the
same bits before and after.  Plans are 16 to 32 points long on at most 16 lines."""
import ctypes

import pytest

from mpi4py_fft_amd import _lib

pytestmark = pytest.mark.gpu

FWD, R2C, C2R = _lib.C2C_FORWARD, _lib.R2C, _lib.C2R
PRIME = 4099                            # no single-pass kernel is that long
NO_KERNEL = b'no single-pass register kernel for this length'
NO_KERNEL2 = b'no single-pass register kernel for one of the lengths'
BAD_BLOCKS = b'block count not supported for this length'
BATCH = b'batch exceeds 2^31'


def dim(n, is_, os):
    return ctypes.byref(_lib.IoDim(n, is_, os))


def guru(n=16, lines=8, n_keep=0, inb=1, outb=1):
    """[lines][n] -> [lines][n]; blocks `lines * n / blocks` entries apart, as gfft_pack lays them out"""
    hm = (_lib.IoDim * 1)(_lib.IoDim(lines, n // inb, n // outb))
    return ('gfft_plan_create_guru_padded',
            (8, FWD, dim(n, 1, 1), n_keep, 1, hm, inb, lines * (n // inb), outb, lines * (n // outb)))


def guru2(n1=16, n2=16, planes=4, inb=1):
    """`planes` planes of n1 x n2 points, the strided axis in `inb` blocks on the input side"""
    return ('gfft_plan_create_guru2',
            (8, FWD, dim(n1, n2, n2), dim(n2, 1, 1), dim(planes, n1 // inb * n2, n1 * n2), 0, inb, planes * (n1 // inb) * n2, 1, 0))


def guru2_real(n1=16, n2=32, planes=4, outb=1):
    """r2c planes of n1 x n2 reals -> n1 x (n2 / 2 + 1), the strided axis in `outb` blocks on the output side"""
    h = n2 // 2 + 1
    return ('gfft_plan_create_guru2_real',
            (8, R2C, dim(n1, n2, h), dim(n2, 1, 1), dim(planes, n1 * n2, n1 // outb * h), 1, 0, outb, planes * (n1 // outb) * h))


CREATORS = [
    (guru(n=PRIME), -2, NO_KERNEL),
    (guru2(n1=PRIME), -2, NO_KERNEL2),
    (guru2_real(n1=PRIME), -2, NO_KERNEL2),
    (guru(n=16, inb=8), -2, BAD_BLOCKS), (guru(n=64, outb=16), -2, BAD_BLOCKS), (guru(n=48, inb=3), -2, BAD_BLOCKS),
    (guru2(n1=16, inb=8), -2, BAD_BLOCKS), (guru2(n1=64, inb=16), -2, BAD_BLOCKS), (guru2(n1=48, inb=3), -2, BAD_BLOCKS),
    (guru2_real(n1=16, outb=8), -2, BAD_BLOCKS), (guru2_real(n1=64, outb=16), -2, BAD_BLOCKS),
    (guru2_real(n1=48, outb=3), -2, BAD_BLOCKS),
    (guru(n=16, n_keep=17), -1, b'bad kept length'),
    (guru(n=16, lines=2 ** 31), -2, BATCH), (guru2(planes=2 ** 27), -2, BATCH), (guru2_real(planes=2 ** 27), -2, BATCH),
]


@pytest.mark.parametrize('case', CREATORS, ids=['%s-%d' % (c[0][0][17:], i) for i, c in enumerate(CREATORS)])
def test_creator_refusal(case):
    (entry, args), code, message = case
    lib = _lib.lib()
    h = ctypes.c_void_p(0xDEAD0)
    rc = getattr(lib, entry)(ctypes.byref(h), *args)
    err = lib.gfft_last_error()
    print(entry, rc, err)
    assert (rc, err) == (code, message)
    assert h.value is None              # the caller's handle is cleared


# (the plan: shape in, shape out, axes, kind; the refused call: entry, arguments behind the plan; code; message)
ROWS = ((8, 16), (8, 16), (1,), FWD)                  # 8 contiguous lines of 16 points
COLS = ((16, 8), (16, 8), (0,), FWD)                  # 8 strided lines of 16 points
BOTH = ((16, 16), (16, 16), (0, 1), FWD)              # two axes: two passes
REAL = ((8, 32), (8, 17), (1,), R2C)                  # 8 packed-real rows of 32 reals
SPLIT_ONLY = b'split layouts fuse into single-pass plans only'
SETTERS = [
    (ROWS, 'gfft_plan_set_split', (2, 2), -1, b'side must be 0 (input) or 1 (output)'),
    (ROWS, 'gfft_plan_set_split', (0, 3), -2, b'block count must be a power of two'),
    (ROWS, 'gfft_plan_set_split', (1, 8), -2, BAD_BLOCKS),
    (BOTH, 'gfft_plan_set_split', (0, 2), -2, SPLIT_ONLY),
    (ROWS, 'gfft_plan_set_tiles', (0, 3, 16), -1, b'tile must be a power of two >= 2 (0 switches the layout off)'),
    (ROWS, 'gfft_plan_set_flat', (0, 0, 0), -2, b'flat tiles: plain complex strided register-kernel passes only'),
    (COLS, 'gfft_plan_set_flat', (9, 0, 0), -1, b'body width must lie in 0 .. columns per row'),
    (ROWS, 'gfft_plan_set_truncation', (0,), -1, b'bad truncated length'),
    (REAL, 'gfft_plan_set_truncation', (0,), -1, b'bad truncated length'),
    (BOTH, 'gfft_plan_set_truncation', (8,), -2, b'truncation fuses into single-pass plans only'),
    (ROWS, 'gfft_plan_set_split_slabs', (1, 2, 4, 4), -2, b'slab-wise split: the half-spectrum side of packed-real rows only'),
    (REAL, 'gfft_plan_set_split_slabs', (1, 2, 4, 3), -1, b'tile must be a power of two >= 2'),
]


@pytest.fixture(scope='module')
def arrays():
    """one fixed random input per plan shape, on the device"""
    import torch
    g = torch.Generator().manual_seed(20261020)
    made = {}

    def get(shape, real):
        if (shape, real) not in made:
            made[shape, real] = torch.randn(*shape, generator=g, dtype=torch.float64 if real else torch.complex128).cuda()
        return made[shape, real]
    return get


@pytest.mark.parametrize('case', SETTERS, ids=['%s-%d' % (c[1][10:], i) for i, c in enumerate(SETTERS)])
def test_refused_setter_leaves_the_plan_unchanged(case, arrays):
    import torch
    (sin, sout, axes, kind), entry, args, code, message = case
    lib, eng = _lib.lib(), _lib.engine()
    x = arrays(sin, kind == R2C)
    h = eng.plan_create(sin, sout, axes, kind, 8)
    try:
        before, after = (torch.full(sout, float('nan'), dtype=torch.complex128, device='cuda') for _ in range(2))
        eng.plan_execute(h, x, before, 1.0)
        rc = getattr(lib, entry)(h, *args)
        err = lib.gfft_last_error()
        print(entry, args, rc, err)
        assert (rc, err) == (code, message)
        eng.plan_execute(h, x, after, 1.0)
        torch.cuda.synchronize()
        assert not torch.isnan(torch.view_as_real(before)).any()
        assert torch.equal(torch.view_as_real(before).view(torch.int64), torch.view_as_real(after).view(torch.int64))
    finally:
        eng.plan_destroy(h)
