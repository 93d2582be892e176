"""Guard bands round the 3/2-rule paths and the data-movement kernels (see tests/test_gpu_guard_bands.py for the method and for
what it does not cover).

A truncating forward transform writes an output SHORTER than its input, a zero-padding backward transform reads an input
shorter than its output: a store of the full band of the last line, or a load of it, leaves the array.  gfft_pack / gfft_unpack
cut an axis into uneven blocks and move 16 bytes per lane where rows allow it, one item otherwise; gfft_scale walks a flat
array with a grid-stride loop whose last step is ragged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pfft_oracle as O
from tests import cases
from tests.guards import MAPPINGS, OFFSETS, four_ways

# one pair per family of cases.TRUNC_LENGTHS, an even and an odd kept length each
PAIRS = [(64, 32, 'fused pow2'), (64, 43, 'fused pow2'), (48, 32, 'fused 3^b 2^k'), (48, 31, 'fused 3^b 2^k'),
         (240, 160, 'fused unequal-width'), (240, 161, 'fused unequal-width'), (18, 12, 'stand-alone'), (112, 75, 'stand-alone')]
TRUNC_MAPPINGS = cases.TRUNC_MAPPINGS + ('one row', 'one col')


def _padded_case(n, kept, dt, mapping):
    """(shape, axis, float64 oracle, x, want, spec, wantb) of FFT(shape, axis, dt, padding=n / kept) on seeded random data"""
    shape, axis = MAPPINGS[mapping](n)
    hi = 'd' if dt in 'df' else 'D'
    ref = O.OFFT(shape, (axis,), hi, padding=n / kept)
    x = O.rng_array(shape, dt, 6)
    want = ref.forward(x.astype(hi))
    spec = want.astype(dt.upper())
    wantb = ref.backward(spec.astype('D'))
    return shape, axis, ref, x, want, spec, wantb


@pytest.mark.parametrize('dt', ['D', 'F', 'd', 'f'])
@pytest.mark.parametrize('n,kept,family', PAIRS)
def test_padded_transforms(n, kept, family, dt):
    """libfft.FFT(padding=n / kept): the truncating store / zero-padding load fused into the pass where the length has the
    adapters, gfft_truncate / gfft_pad around the plain plan elsewhere -- the path asserted as tests/test_gpu_trunc_guard.py
    asserts it; either way the forward output has `kept` (complex) or kept // 2 + 1 (real) entries per line."""
    from mpi4py_fft_amd import FFT
    assert (n, kept) in cases.TRUNC_LENGTHS[family]
    for mapping in TRUNC_MAPPINGS:
        shape, axis, ref, x, want, spec, wantb = _padded_case(n, kept, dt, mapping)
        what = ('padded', family, n, kept, mapping, dt)
        fft = FFT(shape, axis, dtype=dt, padding=n / kept)
        try:
            assert tuple(fft.forward.output_array.shape) == want.shape and want.shape[axis] == cases.trunc_entries(n, kept, dt in 'df')[0]
            if mapping in cases.TRUNC_MAPPINGS:
                text = [bool(fft._fused_trunc)] + [p._eng.plan_describe(p._plan) for p in (fft.fwd, fft.bck)]
                got = cases.trunc_path(text, n, mapping)
                assert got in cases.trunc_expected_path(n, family, dt, mapping), (what, got, text)
            four_ways(lambda a, b: fft.forward(src=a, dst=b), x, want.shape, spec.dtype, want, dt, n, what + ('forward',))
            four_ways(lambda a, b: fft.backward(src=a, dst=b), spec, shape, dt, wantb, dt, n, what + ('backward',))
        finally:
            fft.destroy()


@pytest.mark.parametrize('dt', ['D', 'F'])
@pytest.mark.parametrize('real', [False, True], ids=['complex axis', 'real half-axis'])
def test_truncate_and_pad_kernels(real, dt):
    """gfft_truncate / gfft_pad on their own, through eng.truncate / eng.pad, on the same pairs: the result is a copy, one
    sum of two entries, or an entry doubled / halved -- compared EXACTLY with the float64 oracle's _truncate / _pad restated in
    the array's own precision."""
    from mpi4py_fft_amd import _lib
    eng = _lib.engine()
    prec = _lib.precision_of(dt)
    for n, kept, _ in PAIRS:
        for mapping in TRUNC_MAPPINGS:
            shape, axis = MAPPINGS[mapping](n)
            ref = O.OFFT(shape, (axis,), dt.lower() if real else dt, padding=n / kept)
            full, keep = ref.full_out_shape, ref.out_shape
            V = O.rng_array(full, dt, 7)
            T = ref._truncate(V)
            assert T.dtype == np.dtype(dt) and T.shape == keep
            what = ('gfft_truncate', n, kept, mapping, dt, real)
            four_ways(lambda a, b: eng.truncate(a.tensor, b.tensor, full, axis, keep[axis], real, prec, 1.0), V, keep, dt, T, dt, n,
                      what, exact=True)
            P = ref._pad(T)
            assert P.dtype == np.dtype(dt) and P.shape == full
            four_ways(lambda a, b: eng.pad(a.tensor, b.tensor, full, axis, keep[axis], real, prec), T, full, dt, P, dt, n,
                      ('gfft_pad',) + what[1:], exact=True)


# the six shapes of tests/test_gpu_serial.py test_pack_unpack_blocks; an axis shorter than nparts + 2 with uneven blocks; rows of
# the inner dims that are (16-byte path) and are not (one item per lane) a multiple of 16 bytes, for every item size
PACKS = [((7, 8, 9), 1, 3, 'd'), ((7, 8, 9), 2, 4, 'D'), ((5, 13), 0, 2, 'f'), ((4, 9, 6), 0, 4, 'D'), ((3, 1025, 4), 1, 2, 'F'),
         ((16, 16, 16), 2, 8, 'D'), ((3, 5, 4), 1, 4, 'd'), ((3, 5, 4), 1, 4, 'f'), ((3, 5, 3), 1, 4, 'f'), ((2, 4, 7), 1, 3, 'F'),
         ((2, 4, 8), 1, 3, 'F'), ((19, 6), 1, 5, 'D'), ((6, 19), 0, 5, 'f'), ((7, 4), 0, 3, 'f')]


@pytest.mark.parametrize('shape,axis,p,dt', PACKS, ids=lambda v: 'x'.join(str(s) for s in v) if isinstance(v, tuple) else str(v))
def test_pack_and_unpack(shape, axis, p, dt):
    from mpi4py_fft_amd import _lib
    eng = _lib.engine()
    a = O.rng_array(shape, dt, 8)
    packed = np.concatenate([np.ascontiguousarray(np.take(a, range(s, s + n), axis=axis)).reshape(-1)
                             for n, s in (O.blockdist(shape[axis], p, i) for i in range(p))]).reshape(shape)
    inner_bytes = int(np.prod(shape[axis + 1:])) * a.itemsize
    what = (shape, axis, p, dt, '16-byte path' if inner_bytes % 16 == 0 else 'one item per lane')
    # (one element of offset takes a 4- or 8-byte item off the 16-byte path: both paths run on the 16-byte-row shapes)
    four_ways(lambda x, y: eng.pack(x.tensor, y.tensor, shape, axis, p, a.itemsize), a, shape, dt, packed, dt, 1,
              ('gfft_pack',) + what, exact=True, offsets=OFFSETS, line_in=shape[-1], line_out=shape[-1])
    four_ways(lambda x, y: eng.unpack(x.tensor, y.tensor, shape, axis, p, a.itemsize), packed, shape, dt, a, dt, 1,
              ('gfft_unpack',) + what, exact=True, offsets=OFFSETS, line_in=shape[-1], line_out=shape[-1])


@pytest.mark.parametrize('dt', ['f', 'd'])
@pytest.mark.parametrize('count', [1, 255, 257, 19 * 1000 + 3])
def test_scale(count, dt):
    """gfft_scale in place: the exact product in the array's precision, the scale rounded to it once."""
    from mpi4py_fft_amd import _lib
    from tests.arena import Arena
    eng = _lib.engine()
    x = O.rng_array((count,), dt, 9)
    s = 1.0 / 3.0
    want = x * np.dtype(dt).type(s)
    assert want.dtype == x.dtype
    for off in (0, 1):
        A = Arena((count,), dt, offset_elems=off)
        A.array[...] = x
        eng.scale(A.array.tensor, count, _lib.precision_of(dt), s)
        A.check(('gfft_scale', count, dt, off))
        assert cases.same_bits(np.asarray(A.array), want), (count, dt, off)
