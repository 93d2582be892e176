"""The guards of tests/arena.py bite, shown without a broken kernel: a call that is told its arrays have 20 lines is given a
payload of 19.  Everything stays inside the arena: the 20th line is one line of at most a few KiB, the guards are 1 MiB.

  output side   the 20th line is stored into the back guard: `damage()` must place it at payload end ... payload end + one
                line (for strided lines, whose spill interleaves with the payload's tail, only side and count are held)
  input side    the 20th line is loaded from the back guard: with NaN guards round the input the output's 20th line holds
                NaN, with random guards it holds other bits, and the 19 other lines have the same bits both times

-- through every calling path the guard-band matrix uses (fftw plan execute_scaled and the engine's execute_ptr; libfft.FFT
forward / backward with src= / dst=; eng.pack, unpack, truncate, pad, scale), which also proves that each path runs DIRECTLY on
the arrays it is given: a path that copied through a planned array of its own would touch neither guard, and the matrix would
be vacuous."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pfft_oracle as O
from tests import cases
from tests.arena import Arena
from tests.guards import sync

N, LINES = 64, 20


def _short(shape):
    return (shape[0] - 1,) + tuple(shape[1:])


def bites(execute, in_full, in_dt, out_full, out_dt, what, in_place=False):
    """`execute(a, b)` works on arrays of in_full / out_full, lines along axis 0 (the last line is the last in memory)."""
    x = O.rng_array(in_full, in_dt, 3)
    item = np.dtype(out_dt).itemsize
    line = int(np.prod(out_full[1:])) * item
    # ---- output side: full input, the output payload one line short (in place: the one payload is the short one)
    B = Arena(_short(out_full), out_dt)
    if in_place:
        A = B
        A.array[...] = x[:-1]
    else:
        A = Arena(in_full, in_dt)
        A.array[...] = x
    execute(A.array, B.array)
    sync()
    found = B.damage()
    assert len(found) == 1, (what, 'output side', found)
    side, first, last, count = found[0]
    # (a stored byte differs from the guard's random byte 255 times in 256; a scaled value keeps part of its exponent byte)
    assert side == 'back' and 0 <= first < item and line - item <= last < line and count >= 0.75 * line, (what, found, line)
    with pytest.raises(AssertionError):
        B.check(what)
    if in_place:
        return
    A.check(what + ('the full input arena',))
    # ---- input side: the input payload one line short, finite and NaN guards; full output
    outs = {}
    for fill in ('bytes', 'nan'):
        A = Arena(_short(in_full), in_dt, fill=fill)
        A.array[...] = x[:-1]
        B = Arena(out_full, out_dt)
        B.array[...] = np.zeros(out_full, out_dt)
        execute(A.array, B.array)
        sync()
        A.check(what + (fill, 'input'))
        B.check(what + (fill, 'output'))
        outs[fill] = np.asarray(B.array)
    assert cases.same_bits(outs['bytes'][:-1], outs['nan'][:-1]), (what, 'lines that read no guard differ')
    # (a transform spreads the NaN over its whole line; a copy carries it to the entries it copies, a zero fill stays zero)
    assert np.isnan(outs['nan'][-1]).any(), (what, 'the 20th line did not come from the guard')
    assert not cases.same_bits(outs['bytes'][-1], outs['nan'][-1]), what


@pytest.mark.parametrize('dt', ['D', 'F'])
def test_fftw_plan_rows(dt):
    from mpi4py_fft_amd import fftw
    plan = fftw.fftn(fftw.aligned((LINES, N), dtype=dt), axes=(1,))
    bites(lambda a, b: plan.execute_scaled(a, b, 1.0), (LINES, N), dt, (LINES, N), dt, ('fftw rows', dt))
    # ... and gfft_execute on the arrays' addresses, as the layout cases call it
    bites(lambda a, b: plan._eng.execute_ptr(plan._plan, a.data_ptr, b.data_ptr, 1.0), (LINES, N), dt, (LINES, N), dt, ('execute_ptr', dt))
    plan.destroy()


def test_fftw_plan_strided_lines_spill_interleaved():
    """'cols': a plan for (N, 20) on an output of (N, 19): line c of the plan is column c, every row is one entry longer than
    the payload's, and what does not fit -- N entries in all -- lands behind the payload.  Side and count only."""
    from mpi4py_fft_amd import fftw
    plan = fftw.fftn(fftw.aligned((N, LINES), dtype='D'), axes=(0,))
    A = Arena((N, LINES), 'D')
    A.array[...] = O.rng_array((N, LINES), 'D', 3)
    B = Arena((N, LINES - 1), 'D')
    plan.execute_scaled(A.array, B.array, 1.0)
    sync()
    plan.destroy()
    (side, first, last, count), = B.damage()
    assert side == 'back' and first >= 0 and last < N * 16 and 0.9 * N * 16 <= count <= N * 16, (side, first, last, count)
    A.check()


@pytest.mark.parametrize('dt', ['D', 'd'])
def test_libfft_forward_and_backward(dt):
    from mpi4py_fft_amd import FFT
    fft = FFT((LINES, N), (1,), dtype=dt)
    spec = tuple(fft.forward.output_array.shape)
    bites(lambda a, b: fft.forward(src=a, dst=b), (LINES, N), dt, spec, dt.upper(), ('libfft forward', dt))
    bites(lambda a, b: fft.backward(src=a, dst=b), spec, dt.upper(), (LINES, N), dt, ('libfft backward', dt))
    fft.destroy()


def test_libfft_padded_forward_and_backward():
    """both forms of a 3/2-rule transform: 64 -> 43 fused into the pass, 112 -> 75 through gfft_truncate / gfft_pad (whose
    intermediate array is the plan's own: the caller's arrays are the transform's input and the truncation's output)"""
    from mpi4py_fft_amd import FFT
    for n, kept, fused in ((64, 43, True), (112, 75, False)):
        fft = FFT((LINES, n), (1,), dtype='D', padding=n / kept)
        assert bool(fft._fused_trunc) == fused
        bites(lambda a, b: fft.forward(src=a, dst=b), (LINES, n), 'D', (LINES, kept), 'D', ('padded forward', n, kept))
        bites(lambda a, b: fft.backward(src=a, dst=b), (LINES, kept), 'D', (LINES, n), 'D', ('padded backward', n, kept))
        fft.destroy()


@pytest.mark.parametrize('dt,m', [('D', 6), ('f', 8), ('f', 7)])
def test_pack_and_unpack(dt, m):
    """the cut axis is the first one, so the 20th row of the array is the last row of the last block in the packed buffer"""
    from mpi4py_fft_amd import _lib
    eng = _lib.engine()
    shape, item = (LINES, m), np.dtype(dt).itemsize
    bites(lambda a, b: eng.pack(a.tensor, b.tensor, shape, 0, 3, item), shape, dt, shape, dt, ('pack', dt, m))
    bites(lambda a, b: eng.unpack(a.tensor, b.tensor, shape, 0, 3, item), shape, dt, shape, dt, ('unpack', dt, m))


@pytest.mark.parametrize('real', [False, True])
def test_truncate_and_pad(real):
    from mpi4py_fft_amd import _lib
    eng = _lib.engine()
    full, keep = ((LINES, N // 2 + 1), (LINES, 43 // 2 + 1)) if real else ((LINES, N), (LINES, 43))
    bites(lambda a, b: eng.truncate(a.tensor, b.tensor, full, 1, keep[1], real, 8, 1.0), full, 'D', keep, 'D', ('truncate', real))
    bites(lambda a, b: eng.pad(a.tensor, b.tensor, full, 1, keep[1], real, 8), keep, 'D', full, 'D', ('pad', real))


@pytest.mark.parametrize('dt', ['f', 'd'])
def test_scale(dt):
    from mpi4py_fft_amd import _lib
    eng = _lib.engine()
    bites(lambda a, b: eng.scale(b.tensor, LINES * N, _lib.precision_of(dt), 1.0 / 3.0), (LINES, N), dt, (LINES, N), dt, ('scale', dt),
          in_place=True)
