"""The guarded arena of tests/arena.py on a host tensor: layout, fills, and what `check()` reports for a planted stray store.
The GPU guard-band tests (tests/test_gpu_guard_*.py) rest on this mechanism."""
import numpy as np
import pytest
import torch

from tests.arena import ALIGN, GUARD_LINES, GUARD_MIN, Arena, GuardError


@pytest.mark.parametrize('dt', ['f', 'd', 'F', 'D'])
@pytest.mark.parametrize('offset', [0, 1, 3])
def test_layout_and_alignment(dt, offset):
    a = Arena((19, 48), dt, offset_elems=offset, device='cpu')
    item = np.dtype(dt).itemsize
    assert a.guard == GUARD_MIN and a.start >= a.guard and a.buf.numel() - a.end >= a.guard
    assert (a.array.data_ptr - offset * item) % ALIGN == 0 and a.array.data_ptr % item == 0
    assert a.array.shape == (19, 48) and a.array.dtype == np.dtype(dt) and a.nbytes == 19 * 48 * item
    assert a.array.data_ptr == a.buf.data_ptr() + a.start
    a.check()


def test_guard_holds_32_lines_of_a_long_axis():
    a = Arena((3, 8192), 'D', device='cpu')
    assert a.guard == GUARD_LINES * 8192 * 16 > GUARD_MIN
    assert Arena((8192, 3), 'D', device='cpu').guard == a.guard                # the longest axis, wherever it is
    assert Arena((3, 8192), 'D', line=16, device='cpu').guard == GUARD_MIN


def test_guards_are_not_constant():
    a = Arena((4, 4), 'f', device='cpu')
    for lo, hi in ((0, a.start), (a.end, a.buf.numel())):
        g = a.fill[lo:hi]
        assert len(np.unique(g)) == 256 and not np.array_equal(g[:-1], g[1:])


def test_writing_the_payload_leaves_the_guards():
    a = Arena((7, 5), 'D', device='cpu')
    a.array[...] = np.full((7, 5), 1 + 2j)
    a.array.fill(float('nan'))
    a.check()
    assert np.isnan(np.asarray(a.array)).all()


@pytest.mark.parametrize('side,at', [('back', 0), ('back', 77), ('front', -4), ('front', -4096)])
def test_a_stray_store_is_found_and_placed(side, at):
    a = Arena((5, 6), 'd', device='cpu')
    pos = (a.end if side == 'back' else a.start) + at
    a.buf[pos] ^= 0xFF
    a.buf[pos + 3] ^= 0x01
    assert a.damage() == [(side, at, at + 3, 2)]
    with pytest.raises(GuardError) as e:
        a.check('case')
    assert side in str(e.value) and '2 bytes differ' in str(e.value) and 'offsets %d ... %d' % (at, at + 3) in str(e.value)


def test_a_store_of_zeros_or_nan_shows():
    for value in (0.0, float('nan')):
        a = Arena((5, 6), 'd', device='cpu')
        line = a.buf[a.end:a.end + 6 * 8].view(torch.float64)
        line.fill_(value)
        (side, first, last, count), = a.damage()
        assert side == 'back' and first <= 1 and last >= 6 * 8 - 2 and count > 40


@pytest.mark.parametrize('dt,offset', [('f', 0), ('f', 1), ('d', 1), ('F', 1), ('D', 0), ('D', 1)])
def test_nan_fill_surrounds_the_payload_in_its_real_type(dt, offset):
    a = Arena((3, 10), dt, fill='nan', offset_elems=offset, device='cpu')
    rdt = np.dtype('f4' if dt in 'fF' else 'f8')
    raw = a.buf.numpy()
    before = raw[a.start - 4096 * rdt.itemsize:a.start].view(rdt)
    after = raw[a.end:a.end + 4096 * rdt.itemsize].view(rdt)
    assert np.isnan(before).all() and np.isnan(after).all()
    a.array[...] = np.ones((3, 10))
    a.check()
    assert not np.isnan(np.asarray(a.array)).any()
