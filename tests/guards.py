"""The four runs of a guard-band case (TEST INFRASTRUCTURE; tests/test_gpu_guard_*.py): one operation `execute(a, b)` on device
arrays -- input a, output b -- run on ordinary arrays and inside guarded arenas (tests/arena.py).

  unguarded   on asdevice arrays: the bits every other run must reproduce
  clean       input and output each in an arena of their own, finite guards: all four guards intact, the input payload bit
              for bit what it was, the output at rounding level against the float64 oracle (cases.assert_close, no tolerance
              of this file's) or exactly `want` (exact=True: copies), and the unguarded run's bits
  NaN guards  round the INPUT: the clean run's bits -- no output depends on a byte outside the input
  in place    (complex and real-to-real plans) one arena, a == b: guards intact, the out-of-place bits
  offsets     every (input, output) pair of `offsets`: payloads that start that many ELEMENTS past a 256-byte boundary, NaN
              guards round the input again: the clean run's bits, intact guards

Outputs start as NaN, so an entry nobody wrote shows.  Everything a case executes stays inside its arenas: the payloads have
exactly the plan's shapes."""
import functools

import numpy as np

from oracle import pfft_oracle as O
from tests import cases
from tests.arena import Arena


# batches of lines of n points, none a multiple of a kernel tile (T = 1 ... 16 rows, 2 ... 32 columns), and one single line each way
MAPPINGS = {'rows': lambda n: ((19, n), 1), 'cols': lambda n: ((n, 19), 0), 'middle': lambda n: ((3, n, 7), 1),
            'one row': lambda n: ((1, n), 1), 'one col': lambda n: ((n, 1), 0)}
OFFSETS = ((1, 0), (0, 1), (1, 1))              # (input, output) payloads one element past a 256-byte boundary


def _nan(shape, dt):
    return np.full(shape, np.nan, dtype=dt)


def sync():
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def four_ways(execute, x, out_shape, out_dt, want, dt, nelem, what, in_place=False, exact=False, offsets=(), line_in=None,
              line_out=None, natural=None):
    """Runs the case (see the module's docstring) and returns the clean run's output.  `natural`: re-lays an output buffer
    out in the order of `want` before it is compared with it (exchange-buffer layouts); bit comparisons are on the raw buffer."""
    from mpi4py_fft_amd import asdevice
    x = np.ascontiguousarray(x)
    out_dt = np.dtype(out_dt)
    a, b = asdevice(x), asdevice(_nan(out_shape, out_dt))
    execute(a, b)
    plain = np.asarray(b)
    assert cases.same_bits(np.asarray(a), x), (what, 'unguarded run: the input changed')

    def guarded(fill, off_in=0, off_out=0):
        tag = (what, '%s guards' % fill, 'offsets %d / %d' % (off_in, off_out))
        A = Arena(x.shape, x.dtype, fill=fill, offset_elems=off_in, line=line_in)
        B = Arena(out_shape, out_dt, offset_elems=off_out, line=line_out)
        A.array[...] = x
        B.array[...] = _nan(out_shape, out_dt)
        execute(A.array, B.array)
        sync()
        A.check(tag + ('input',))
        B.check(tag + ('output',))
        assert cases.same_bits(np.asarray(A.array), x), tag + ('the input payload changed',)
        return np.asarray(B.array)

    clean = guarded('bytes')
    got = clean if natural is None else natural(clean)
    if exact:
        assert not np.isnan(got).any() and np.array_equal(got, want), (what, 'values')
    else:
        cases.assert_close(got.astype(want.dtype), want, dt, nelem, what)
    assert cases.same_bits(clean, plain), (what, 'guarded and unguarded runs differ')
    assert cases.same_bits(guarded('nan'), clean), (what, 'an output depends on bytes outside the input')
    if in_place:
        assert x.dtype == out_dt and x.shape == tuple(out_shape), what
        C = Arena(x.shape, x.dtype, line=line_in)
        C.array[...] = x
        execute(C.array, C.array)
        sync()
        C.check((what, 'in place'))
        assert cases.same_bits(np.asarray(C.array), clean), (what, 'in-place and out-of-place runs differ')
    for off_in, off_out in offsets:
        assert cases.same_bits(guarded('nan', off_in, off_out), clean), (what, 'element-aligned bases', off_in, off_out)
    return clean


def serial_case(shape, axes, dt, what, r2r=None, path=None, in_place=False, offsets=OFFSETS, capped=False, seed=5):
    """libfft.FFT(shape, axes, dt) -- optionally a real-to-real kind along its one axis -- on seeded random data, forward (normalised) and
    backward (of the oracle's spectrum rounded to dt), each in the four ways of tests/guards.py; both run DIRECTLY on the
    given arrays (src= / dst=).  Reference: oracle.pfft_oracle.OFFT in float64 on the same (widened) inputs."""
    from mpi4py_fft_amd import FFT, fftw
    hi = 'd' if dt in 'df' else 'D'
    okw, kw = {}, {}
    if r2r is not None:
        okw['r2r'] = r2r
        fam, typ = O.R2R_KINDS[r2r]
        f, b = (fftw.dctn, fftw.idctn) if fam == 'dct' else (fftw.dstn, fftw.idstn)
        kw['transforms'] = {tuple(axes): (functools.partial(f, type=typ), functools.partial(b, type=typ))}
    ref = O.OFFT(shape, axes, hi, **okw)
    x = O.rng_array(shape, dt, seed)
    want = ref.forward(x.astype(hi))
    spec = want.astype(dt if r2r is not None else dt.upper())
    wantb = ref.backward(spec.astype(want.dtype))
    nelem = int(np.prod([shape[a] if r2r is None else O.r2r_logical_n(r2r, shape[a]) for a in axes]))
    fft = FFT(shape, axes, dtype=dt, **kw)
    try:
        assert tuple(fft.forward.output_array.shape) == want.shape, (what, fft.forward.output_array.shape, want.shape)
        plans = (fft.fwd, fft.bck)
        if path is not None:
            path([p._eng.plan_describe(p._plan) for p in plans])
        four_ways(lambda a, b: fft.forward(src=a, dst=b), x, want.shape, spec.dtype, want, dt, nelem, what + ('forward',),
                  in_place=in_place, offsets=offsets)
        four_ways(lambda a, b: fft.backward(src=a, dst=b), spec, shape, dt, wantb, dt, nelem, what + ('backward',),
                  in_place=in_place, offsets=offsets)
        if capped:
            launch = cases.plan_launches(plans)
            assert launch and all(w == 1 and t >= 1 for t, w in launch), (what, launch)
    finally:
        fft.destroy()
