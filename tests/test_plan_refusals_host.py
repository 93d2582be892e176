"""What the plan API refuses before it looks for a device: one call with one fault each, the exact status code and the exact
gfft_last_error() text.  The Python side branches on these codes (-2 becomes None / False and a slower path, -1 raises), so a check
that drifts between the two is silent.  Pointers are stand-ins that a refused call never dereferences.  Passes with or without a
device: the rows whose arguments are accepted go on to the device check and are asserted only where there is none."""
import ctypes

import pytest

from mpi4py_fft_amd import _lib

FWD, BWD, R2C, C2R = _lib.C2C_FORWARD, _lib.C2C_BACKWARD, _lib.R2C, _lib.C2R
NO_DEVICE = (-3, b'no HIP device available (libgfft has no host fallback)')
SEED = 0xDEAD0                          # what a plan handle holds before the call
PTR = ctypes.c_void_p(0x1000)           # a device address nobody reads


def i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def dim(n, is_, os):
    return ctypes.byref(_lib.IoDim(n, is_, os))


H = 'handle'                            # placeholder of the plan handle in a creator's arguments
S88, AX1 = i64(8, 8), ints(1)
P48 = i64(48, 48, 48)
COLS16, ROWS16, PLANES4 = (16, 16, 16), (16, 1, 1), (4, 256, 256)          # a valid guru2 request: 4 planes of 16 x 16 points
RCOLS, RROWS, RPLANES = (16, 16, 9), (16, 1, 1), (4, 256, 144)             # ... and a valid guru2_real R2C one (H = 9)


def guru2(cols=COLS16, rows=ROWS16, planes=PLANES4, precision=8, kind=FWD, inb=1, outb=1, null=None):
    io = [None if null == i else dim(*d) for i, d in enumerate((cols, rows, planes))]
    return (H, precision, kind, io[0], io[1], io[2], 0, inb, 0, outb, 0)


def guru2_real(cols=RCOLS, rows=RROWS, planes=RPLANES, precision=8, kind=R2C, inb=1, ins=0, outb=1, outs=0, null=None):
    io = [None if null == i else dim(*d) for i, d in enumerate((cols, rows, planes))]
    return (H, precision, kind, io[0], io[1], io[2], inb, ins, outb, outs)


def guru(precision=8, kind=FWD, d=(16, 1, 1), rank=1, howmany=((8, 16, 16),), null_dim=False, null_howmany=False):
    hm = None if null_howmany else (_lib.IoDim * 4)(*[_lib.IoDim(*x) for x in howmany])
    return (H, precision, kind, None if null_dim else dim(*d), 0, rank, hm, 1, 0, 1, 0)


# (entry, arguments, code, message); code None: the arguments are accepted and the call goes on to the device check
CREATORS = [
    ('gfft_plan_create', (None, 2, S88, S88, 1, AX1, FWD, 8), -1, b'null argument'),
    ('gfft_plan_create', (H, 0, S88, S88, 1, AX1, FWD, 8), -1, b'bad ndims/naxes'),
    ('gfft_plan_create', (H, 2, S88, S88, 3, ints(0, 1, 0), FWD, 8), -1, b'bad ndims/naxes'),
    ('gfft_plan_create', (H, 2, S88, S88, 1, AX1, FWD, 3), -1, b'precision must be 4 or 8'),
    ('gfft_plan_create', (H, 2, S88, S88, 1, AX1, 5, 8), -2,
     b'only c2c / r2c / c2r kinds are implemented (r2r kinds are out of scope)'),
    ('gfft_plan_create', (H, 2, S88, S88, 2, ints(0, -2), FWD, 8), -1, b'bad or repeated axis'),
    ('gfft_plan_create', (H, 2, i64(8, 0), i64(8, 0), 1, AX1, FWD, 8), -1, b'sizes must be >= 1'),
    ('gfft_plan_create', (H, 2, S88, S88, 1, AX1, R2C, 8), -1, b'r2c: sizes_out[axis] must be n/2+1'),
    ('gfft_plan_create', (H, 2, S88, S88, 1, AX1, C2R, 8), -1, b'c2r: sizes_in[axis] must be n/2+1'),
    ('gfft_plan_create', (H, 2, S88, i64(8, 7), 1, AX1, FWD, 8), -1,
     b'sizes_in and sizes_out may differ only along the halved axis'),
    ('gfft_plan_create', (H, 2, S88, S88, 1, AX1, FWD, 8), None, None),
    ('gfft_plan_create_padded', (H, None, i64(32, 32, 17), R2C, 8), -1, b'null argument'),
    ('gfft_plan_create_padded', (H, P48, i64(32, 32, 17), R2C, 2), -1, b'precision must be 4 or 8'),
    ('gfft_plan_create_padded', (H, P48, i64(32, 32, 17), 7, 8), -1, b'kind must be c2c forward / backward, r2c or c2r'),
    ('gfft_plan_create_padded', (H, P48, i64(32, 32, 26), R2C, 8), -1, b'kept entries must lie in 1 .. transformed entries'),
    ('gfft_plan_create_padded', (H, P48, i64(32, 32, 17), R2C, 8), None, None),
    ('gfft_plan_create_r2r', (H, 2, S88, 1, AX1, None, 8), -1, b'null argument'),
    ('gfft_plan_create_r2r', (H, 17, i64(*[8] * 17), 1, AX1, ints(3), 8), -1, b'bad ndims/naxes'),
    ('gfft_plan_create_r2r', (H, 2, S88, 1, AX1, ints(3), 16), -1, b'precision must be 4 or 8'),
    ('gfft_plan_create_r2r', (H, 2, S88, 1, ints(2), ints(3), 8), -1, b'bad or repeated axis'),
    ('gfft_plan_create_r2r', (H, 2, S88, 1, AX1, ints(2), 8), -2,
     b'r2r kind must be one of REDFT00..RODFT11 (halfcomplex / DHT kinds are not implemented)'),
    ('gfft_plan_create_r2r', (H, 2, i64(8, 0), 1, AX1, ints(3), 8), -1, b'sizes must be >= 1'),
    # two faults in one call: the first one found wins -- precision before kind; axes and kinds entry by entry
    ('gfft_plan_create', (H, 2, S88, S88, 1, AX1, 5, 3), -1, b'precision must be 4 or 8'),
    ('gfft_plan_create_r2r', (H, 2, S88, 2, ints(0, 5), ints(2, 3), 8), -2,
     b'r2r kind must be one of REDFT00..RODFT11 (halfcomplex / DHT kinds are not implemented)'),
    ('gfft_plan_create_r2r', (H, 2, S88, 2, ints(5, 0), ints(2, 3), 8), -1, b'bad or repeated axis'),
    ('gfft_plan_create_guru_padded', guru(null_dim=True), -1, b'null argument'),
    ('gfft_plan_create_guru_padded', guru(null_howmany=True), -1, b'null argument'),
    ('gfft_plan_create_guru_padded', guru(precision=5), -1, b'precision must be 4 or 8'),
    ('gfft_plan_create_guru_padded', guru(kind=R2C), -2, b'guru plans are complex-to-complex'),
    ('gfft_plan_create_guru_padded', guru(rank=4, howmany=((2, 64, 64),) * 4), -2, b'at most three batch dims'),
    ('gfft_plan_create_guru_padded', guru(d=(0, 1, 1)), -1, b'bad transform length'),
    ('gfft_plan_create_guru2', guru2(null=1), -1, b'null argument'),
    ('gfft_plan_create_guru2', guru2(precision=0), -1, b'precision must be 4 or 8'),
    ('gfft_plan_create_guru2', guru2(kind=C2R), -2, b'guru plans are complex-to-complex'),
    ('gfft_plan_create_guru2', guru2(planes=(0, 256, 256)), -1, b'bad length'),
    ('gfft_plan_create_guru2', guru2(rows=(16, 2, 1)), -2, b'the row axis must be contiguous on both sides'),
    ('gfft_plan_create_guru2', guru2(inb=0), -1, b'bad block count'),
    ('gfft_plan_create_guru2', guru2(inb=2, outb=2), -2, b'blocks on one side only'),
    ('gfft_plan_create_guru2_real', guru2_real(null=0), -1, b'null argument'),
    ('gfft_plan_create_guru2_real', guru2_real(precision=1), -1, b'precision must be 4 or 8'),
    ('gfft_plan_create_guru2_real', guru2_real(kind=FWD), -2,
     b'guru2_real plans are r2c / c2r (complex pairs: gfft_plan_create_guru2)'),
    ('gfft_plan_create_guru2_real', guru2_real(cols=(0, 16, 9)), -1, b'bad length'),
    ('gfft_plan_create_guru2_real', guru2_real(rows=(16, 1, 2)), -2, b'the row axis must be contiguous on both sides'),
    ('gfft_plan_create_guru2_real', guru2_real(cols=(16, 0, 9)), -1, b'strides must be positive'),
    ('gfft_plan_create_guru2_real', guru2_real(outb=0), -1, b'bad block count'),
    ('gfft_plan_create_guru2_real', guru2_real(inb=2), -1, b'blocks on the half-spectrum side only (R2C: output, C2R: input)'),
    ('gfft_plan_create_guru2_real', guru2_real(cols=(16, 15, 9)), -1, b'rows of a plane overlap (row stride below the row\'s length)'),
    ('gfft_plan_create_guru2_real', guru2_real(outb=2, outs=8), -1, b'block stride smaller than the block\'s extent'),
]

SHAPE2, SHAPE8 = i64(8, 8), i64(8, 8)
OTHERS = [
    ('gfft_plan_set_truncation', (None, 4), -1, b'null plan'),
    ('gfft_plan_set_split', (None, 0, 2), -1, b'null plan'),
    ('gfft_plan_set_tiles', (None, 0, 4, 16), -1, b'null plan'),
    ('gfft_plan_set_flat', (None, 0, 0, 0), -1, b'null plan'),
    ('gfft_plan_set_split_slabs', (None, 1, 2, 4, 4), -1, b'null plan'),
    ('gfft_plan_status', (None,), -1, b'null plan'),
    ('gfft_plan_cost', (None, None, None, None), -1, b'null plan'),
    ('gfft_execute', (None, PTR, PTR, 1.0, None), -1, b'null argument'),
    ('gfft_plan_describe', (None, ctypes.create_string_buffer(16), 16), -1, b'null argument'),
    ('gfft_set_option', (b'nonesuch', 1), -1, b'unknown option nonesuch'),
    ('gfft_set_option', (None, 1), -1, b'null option name'),
    ('gfft_pack', (PTR, PTR, 2, SHAPE2, 2, 2, 16, None), -1, b'bad shape/axis'),
    ('gfft_pack', (PTR, PTR, 2, SHAPE2, 1, 9, 16, None), -1, b'axis shorter than the number of parts'),
    ('gfft_pack', (PTR, PTR, 2, SHAPE2, 1, 0, 16, None), -1, b'axis shorter than the number of parts'),
    ('gfft_unpack', (PTR, PTR, 2, SHAPE2, 1, 9, 16, None), -1, b'axis shorter than the number of parts'),
    ('gfft_unpack', (PTR, PTR, 2, SHAPE2, 1, 0, 16, None), -1, b'axis shorter than the number of parts'),
    ('gfft_truncate', (PTR, PTR, 2, SHAPE8, 1, 9, 0, 8, 1.0, None), -1, b'bad truncated length'),
    ('gfft_truncate', (PTR, PTR, 2, SHAPE8, 1, 0, 0, 8, 1.0, None), -1, b'bad truncated length'),
    ('gfft_pad', (PTR, PTR, 2, SHAPE8, 1, 9, 0, 8, None), -1, b'bad truncated length'),
    ('gfft_pad', (PTR, PTR, 2, SHAPE8, 1, 0, 0, 8, None), -1, b'bad truncated length'),
    # (a stand-in plan is not dereferenced before the out pointers have been looked at)
    ('gfft_plan_pass_launch', (None, 0, ctypes.pointer(ctypes.c_int64()), ctypes.pointer(ctypes.c_int())), -1, b'null plan'),
    ('gfft_plan_pass_launch', (PTR, 0, None, ctypes.pointer(ctypes.c_int())), -1, b'null argument'),
    ('gfft_plan_pass_launch', (PTR, 0, ctypes.pointer(ctypes.c_int64()), None), -1, b'null argument'),
]

# the keys gfft_set_option accepts and their defaults, from the library's source
OPTION_DEFAULTS = [
    ('grid_cap', 0), ('variant_rows', 0), ('variant_cols', 0), ('force_generic', 0), ('copy_nt', 2), ('fused3', 1), ('plane2d', 1),
    ('fuse2', 1), ('fuse2_ring', 0), ('fuse2_lag', 0), ('fuse2_kinds', 2046), ('fuse2_wait_ms', 2000), ('fuse2_f32', 1),
    ('fuse2_n512', 2), ('c2r_2048', 1), ('fuse2_mixv', 1), ('fuse2_mixed', 1), ('fuse2_f32_n512', 1), ('debug_flat', 0),
    ('flat_out', 1), ('wtile', 1), ('mixv', 1), ('mixv_variant', 0), ('debug_tile_lg', 0), ('debug_tile_side', 0),
    ('debug_tile_stride', 0), ('profile', 0), ('debug_tw_index', 1), ('debug_tw_exp', 0), ('debug_tw_len', 0), ('debug_r2r_index', 1),
    ('debug_r2r_exp', 0), ('debug_r2r_post', 0), ('xcd_swizzle', -1), ('tile_order', -1), ('fused3_min_mib', 32),
]


def _call(entry, args):
    """the call with a seeded handle in place of H; returns (code, last error, the handle afterwards: None = cleared)"""
    lib = _lib.lib()
    h = ctypes.c_void_p(SEED)
    rc = getattr(lib, entry)(*[ctypes.byref(h) if a is H else a for a in args])
    return rc, lib.gfft_last_error(), h.value


def _id(case):
    return '%s-%s' % (case[0][5:], (case[3] or b'accepted').decode().replace(' ', '_')[:40])


@pytest.fixture(scope='module')
def no_device():
    return _lib.device_count() == 0


@pytest.mark.parametrize('case', CREATORS, ids=[_id(c) + '-%d' % i for i, c in enumerate(CREATORS)])
def test_creator_refusal(case, no_device):
    entry, args, code, message = case
    if code is None:
        if not no_device:
            pytest.skip('a device is present: the request is accepted')
        code, message = NO_DEVICE
    rc, err, handle = _call(entry, args)
    assert (rc, err) == (code, message)
    # a refusal past the null-argument check clears the caller's handle; the null-argument check itself comes before that
    if any(a is H for a in args):
        assert handle == (SEED if message == b'null argument' else None)


@pytest.mark.parametrize('case', OTHERS, ids=[_id(c) + '-%d' % i for i, c in enumerate(OTHERS)])
def test_refusal(case):
    entry, args, code, message = case
    rc, err, _ = _call(entry, args)
    assert (rc, err) == (code, message)


def test_destroying_a_null_plan_is_no_error():
    lib = _lib.lib()
    assert lib.gfft_set_option(None, 1) == -1
    assert lib.gfft_plan_destroy(None) == 0
    assert lib.gfft_last_error() == b'null option name'          # untouched


def test_every_option_key_is_accepted():
    lib = _lib.lib()
    assert len(OPTION_DEFAULTS) == 36 and len(set(k for k, _ in OPTION_DEFAULTS)) == 36
    for key, value in OPTION_DEFAULTS:
        assert lib.gfft_set_option(key.encode(), value) == 0, key
