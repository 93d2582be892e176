"""The base-alignment contract of include/gfft.h where no device is needed: the data-movement entry points refuse an array that is
not aligned as one of its items before they look for a device (exact status and gfft_last_error() text, as
tests/test_plan_refusals_host.py holds the other refusals), and the Python layer stops treating a real view that starts at an odd
element as directly usable.  The refusals of gfft_execute itself -- a misaligned base, d_in == d_out on a plan with a re-laid-out
side -- need a plan, and a plan needs a device: tests/test_gpu_execute_refusals.py holds them."""
import ctypes

import numpy as np
import pytest
import torch

from mpi4py_fft_amd import _lib, fftw
from mpi4py_fft_amd.array import DeviceArray
from mpi4py_fft_amd.mpifft import Transform

P = ctypes.c_void_p
OK, ODD4, ODD8, ODD2 = P(0x1000), P(0x1004), P(0x1008), P(0x1002)
SHAPE = (ctypes.c_int64 * 2)(8, 8)

REFUSALS = [
    ('gfft_pack', (OK, ODD8, 2, SHAPE, 1, 2, 16, None), b'arrays must be aligned to 16 bytes (one element)'),
    ('gfft_pack', (ODD4, OK, 2, SHAPE, 1, 2, 8, None), b'arrays must be aligned to 8 bytes (one element)'),
    ('gfft_unpack', (OK, ODD2, 2, SHAPE, 1, 2, 4, None), b'arrays must be aligned to 4 bytes (one element)'),
    ('gfft_pack', (OK, OK, 2, SHAPE, 1, 2, 12, None), b'itemsize must be 4, 8 or 16'),
    ('gfft_unpack', (OK, OK, 2, SHAPE, 1, 2, 0, None), b'itemsize must be 4, 8 or 16'),
    ('gfft_truncate', (ODD8, OK, 2, SHAPE, 1, 4, 0, 8, 1.0, None), b'arrays must be aligned to 16 bytes (one element)'),
    ('gfft_truncate', (OK, ODD4, 2, SHAPE, 1, 4, 0, 4, 1.0, None), b'arrays must be aligned to 8 bytes (one element)'),
    ('gfft_truncate', (OK, OK, 2, SHAPE, 1, 4, 0, 2, 1.0, None), b'precision must be 4 or 8'),
    ('gfft_pad', (OK, ODD8, 2, SHAPE, 1, 4, 1, 8, None), b'arrays must be aligned to 16 bytes (one element)'),
    ('gfft_pad', (OK, OK, 2, SHAPE, 1, 4, 1, 16, None), b'precision must be 4 or 8'),
    ('gfft_scale', (ODD4, 10, 8, 2.0, None), b'arrays must be aligned to 8 bytes (one element)'),
    ('gfft_scale', (ODD2, 10, 4, 2.0, None), b'arrays must be aligned to 4 bytes (one element)'),
    ('gfft_scale', (OK, 10, 3, 2.0, None), b'precision must be 4 or 8'),
]
# what the contract accepts: one item of alignment is enough (the call goes on to the device check)
ACCEPTED = [
    ('gfft_pack', (ODD8, ODD8, 2, SHAPE, 1, 2, 8, None)),
    ('gfft_unpack', (ODD4, ODD4, 2, SHAPE, 1, 2, 4, None)),
    ('gfft_truncate', (ODD8, ODD8, 2, SHAPE, 1, 4, 0, 4, 1.0, None)),
    ('gfft_scale', (ODD4, 10, 4, 2.0, None)),
]


@pytest.mark.parametrize('case', REFUSALS, ids=['%s-%d' % (c[0][5:], i) for i, c in enumerate(REFUSALS)])
def test_misaligned_arrays_are_refused_before_a_device_is_touched(case):
    entry, args, message = case
    lib = _lib.lib()
    assert (getattr(lib, entry)(*args), lib.gfft_last_error()) == (-1, message)


@pytest.mark.parametrize('case', ACCEPTED, ids=['%s-%d' % (c[0][5:], i) for i, c in enumerate(ACCEPTED)])
def test_one_item_of_alignment_is_enough(case):
    entry, args = case
    if _lib.device_count():
        return                          # (a device is present: the call would run on the stand-in addresses)
    lib = _lib.lib()
    assert getattr(lib, entry)(*args) == -3 and lib.gfft_last_error().startswith(b'no HIP device')


def _view(dt, offset, shape=(3, 8)):
    """A contiguous host DeviceArray that starts `offset` elements into a 64-byte-aligned allocation"""
    count = int(np.prod(shape))
    raw = torch.empty((count + offset + 16) * np.dtype(dt).itemsize, dtype=torch.uint8)
    skip = -raw.data_ptr() % 64
    t = raw[skip:skip + (count + offset) * np.dtype(dt).itemsize].view(torch.from_numpy(np.zeros(1, dt)).dtype)
    a = DeviceArray(shape, dt, tensor=t[offset:].reshape(shape))
    a._keep = raw
    assert a.is_contiguous() and a.data_ptr % 64 == (offset * np.dtype(dt).itemsize) % 64
    return a


@pytest.mark.parametrize('dt,offset,aligned', [('d', 0, True), ('d', 1, False), ('d', 2, True), ('f', 1, False), ('f', 3, False), ('f', 2, True),
                                               ('D', 1, True), ('F', 1, True), ('F', 3, True)])
def test_python_layer_runs_directly_only_on_pair_aligned_arrays(dt, offset, aligned):
    a, ref = _view(dt, offset), _view(dt, 0)
    assert fftw.pair_aligned(a) == aligned
    assert Transform._direct(a, ref) == aligned                 # PFFT: otherwise the copy into the planned array
    plan = fftw.FFT.__new__(fftw.FFT)                            # (the check reads nothing of the plan)
    assert plan._compatible(a, a.shape, a.strides, a.dtype) == aligned
