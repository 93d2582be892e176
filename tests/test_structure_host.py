"""Host logic of the structure functions (no GPU): the shapes, the whole-axis rule and the rank reduction of
`SpectralOps.structure_functions` over a numpy stand-in for the kernel (tests/structure_ref.py), `log_separations`,
`structure_moments`, and the argument checks of gfft_ps_structure that need no device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases, structure_ref as R
from tests.host_engine import HostEngine


class StructureEngine(HostEngine):
    """HostEngine plus gfft_ps_structure restated with numpy (tests/structure_ref.py) on host tensors."""
    seen = []

    def ps_structure(self, tu, ncomp, n, axis, seps, lcomp, tout, precision):
        StructureEngine.seen.append((int(ncomp), tuple(int(x) for x in n), int(axis), [int(r) for r in seps], int(lcomp)))
        assert tu.numel() == ncomp * int(np.prod(n)) and tuple(tout.shape) == (len(seps), ncomp, R.NVAL)
        out, _ = R.structure(tu.numpy().reshape((ncomp,) + tuple(n)), axis, seps, lcomp)
        tout.copy_(torch.as_tensor(out))


@pytest.fixture
def engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(StructureEngine())
    StructureEngine.seen = []
    yield
    _lib.set_engine(old)


def _field(shape, m, seed=11):
    return np.random.default_rng(seed).standard_normal((m,) + tuple(shape))


def test_shapes_layout_and_arguments(engine):
    from mpi4py_fft_amd import PFFT, _lib, comm, newDistArray, spectral
    assert (_lib.SF_D1, _lib.SF_D2, _lib.SF_D3, _lib.SF_D4, _lib.SF_D5, _lib.SF_D6, _lib.SF_ABS1, _lib.SF_ABS3, _lib.SF_MIX) == \
        tuple(range(9)) and _lib.PS_SF_NVAL == 9 == R.NVAL
    shape = (8, 6, 20)
    G = _field(shape, 3)
    fft = PFFT(comm.COMM_SELF, shape, dtype='d')
    ops = spectral.SpectralOps(fft)
    u = newDistArray(fft, False, rank=1)
    u[...] = G
    assert ops.whole_axes() == [0, 1, 2]
    for axis in range(3):
        seps = [0, 1, shape[axis] // 2, shape[axis] - 1]
        sf = ops.structure_functions(u, axis, seps, lcomp=axis)
        assert isinstance(sf, np.ndarray) and sf.dtype == np.float64 and sf.shape == (4, 3, 9)
        assert StructureEngine.seen[-1] == (3, shape, axis, seps, axis)
        ref, mag = R.structure(G, axis, seps, axis)
        assert np.array_equal(sf, ref)
        assert not sf[0].any()                                           # r = 0
        # the layout: [k][c][value], value 1 = sum d^2 > 0, and the mixed entry of the longitudinal component is its sum d^3
        assert (sf[1:, :, _lib.SF_D2] > 0).all()
        assert np.allclose(sf[:, axis, _lib.SF_MIX], sf[:, axis, _lib.SF_D3], rtol=1e-13, atol=1e-13)
        # r and n - r: the same pairs with the sign of d turned
        assert np.allclose(sf[1, :, _lib.SF_D3], -sf[3, :, _lib.SF_D3], rtol=1e-12, atol=1e-12)
        assert np.allclose(sf[1, :, _lib.SF_D4], sf[3, :, _lib.SF_D4], rtol=1e-13)
    # no longitudinal component: -1 reaches the engine and the mixed entries are zeros
    sf = ops.structure_functions(u, 2, [1, 2])
    assert StructureEngine.seen[-1][-1] == -1 and not sf[:, :, _lib.SF_MIX].any()
    # a scalar field: one component
    sc = ops.structure_functions(u[1], 1, [1, 2, 3])
    assert sc.shape == (3, 1, 9) and np.array_equal(sc[:, 0], R.structure(G[1:2], 1, [1, 2, 3])[0][:, 0])
    # out= and reduce=False: the tensor itself
    out = torch.zeros((2, 3, 9), dtype=torch.float64)
    assert ops.structure_functions(u, 0, [1, 3], lcomp=0, out=out, reduce=False) is out
    assert np.array_equal(out.numpy(), ops.structure_functions(u, 0, [1, 3], lcomp=0))
    for bad in (dict(axis=3), dict(axis=-1), dict(seps=[]), dict(seps=[20]), dict(seps=[-1]), dict(seps=list(range(20)) * 4),
                dict(lcomp=3), dict(lcomp=-2), dict(out=torch.zeros((1, 3, 8), dtype=torch.float64)),
                dict(out=torch.zeros((1, 3, 9), dtype=torch.float32))):
        kw = dict(axis=2, seps=[1], lcomp=None)
        kw.update(bad)
        with pytest.raises(AssertionError):
            ops.structure_functions(u, **kw)
    with pytest.raises(AssertionError, match='precision'):               # a float32 field on a double transform
        ops.structure_functions(u.tensor.to(torch.float32), 2, [1])
    fft.destroy()


def test_log_separations():
    from mpi4py_fft_amd.spectral import log_separations
    assert log_separations(256) == [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128]
    assert log_separations(32) == [1, 2, 3, 4, 6, 8, 12, 16]
    assert log_separations(20) == [1, 2, 3, 4, 6, 8]
    assert log_separations(7) == [1, 2, 3]
    assert log_separations(2) == [1] and log_separations(1) == [] and log_separations(3) == [1]
    assert log_separations(64, per_octave=1) == [1, 2, 4, 8, 16, 32]
    assert log_separations(64, per_octave=4) == [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32]
    for N in (5, 48, 100, 4096):
        for p in (1, 2, 3, 4):
            s = log_separations(N, p)
            assert all(isinstance(r, int) for r in s) and s == sorted(set(s)) and s[0] == 1 and s[-1] <= N // 2
            assert len(s) <= 64                                          # one call of structure_functions takes them


def test_structure_moments_on_a_known_table():
    """u_c = A_c sin(2 pi x / n + phase) along axis 2: d = 2 A sin(pi r / n) cos(...), so with s = 2 A sin(pi r / n)
    <d^2> = s^2 / 2, <d^4> = 3 s^4 / 8, <d^6> = 5 s^6 / 16, <|d|> = 2 s / pi, <|d|^3> = 4 s^3 / (3 pi), odd moments 0,
    flatness 3/2."""
    from mpi4py_fft_amd import _lib, spectral
    n, amp = 64, np.array([1.0, 2.0, 0.5])
    x = 2 * np.pi * np.arange(n) / n
    G = np.broadcast_to((amp[:, None] * np.sin(x[None, :] + np.array([0.0, 0.3, 1.1])[:, None]))[:, None, None, :], (3, 2, 3, n))
    seps = [1, 5, 32]
    sf, _ = R.structure(G, 2, seps, lcomp=2)
    mo = spectral.structure_moments(sf, 2 * 3 * n, axis=2)
    assert mo.S.shape == (3, 3, 6) and mo.abs1.shape == mo.abs3.shape == mo.skewness.shape == mo.flatness.shape == mo.mixed.shape == (3, 3)
    assert mo.longitudinal == 2 and mo.transverse == [0, 1]
    s = 2 * amp[None, :] * np.sin(np.pi * np.array(seps)[:, None] / n)
    tol = dict(rtol=1e-13, atol=1e-13)
    assert np.allclose(mo.S[..., 1], s ** 2 / 2, **tol) and np.allclose(mo.S[..., 3], 3 * s ** 4 / 8, **tol)
    assert np.allclose(mo.S[..., 5], 5 * s ** 6 / 16, **tol)
    for p in (0, 2, 4):
        assert np.allclose(mo.S[..., p], 0, **tol)
    assert np.allclose(mo.flatness, 1.5, **tol) and np.allclose(mo.skewness, 0, **tol)
    # |cos| is sampled, not integrated: 64 points give <|cos|> = 2 / pi to 1e-3
    assert np.allclose(mo.abs1, 2 * s / np.pi, rtol=2e-3) and np.allclose(mo.abs3, 4 * s ** 3 / (3 * np.pi), rtol=2e-3)
    assert np.allclose(mo.mixed[:, 2], mo.S[:, 2, 2], **tol)
    # the plain division, the names of _lib and the labels
    raw = np.arange(2 * 4 * 9, dtype=np.float64).reshape(2, 4, 9) + 1
    mo = spectral.structure_moments(raw, 4, axis=0)
    assert np.array_equal(mo.S, raw[..., :6] / 4) and np.array_equal(mo.abs1, raw[..., _lib.SF_ABS1] / 4)
    assert np.array_equal(mo.abs3, raw[..., _lib.SF_ABS3] / 4) and np.array_equal(mo.mixed, raw[..., _lib.SF_MIX] / 4)
    assert np.array_equal(mo.flatness, (raw[..., 3] / 4) / (raw[..., 1] / 4) ** 2)
    assert np.array_equal(mo.skewness, (raw[..., 2] / 4) / (raw[..., 1] / 4) ** 1.5)
    assert mo.longitudinal == 0 and mo.transverse == [1, 2]
    assert spectral.structure_moments(raw, 4).longitudinal is None and spectral.structure_moments(raw[:, :2], 4, axis=1).transverse is None
    zero = spectral.structure_moments(np.zeros((1, 1, 9)), 8)            # r = 0: 0 / 0
    assert np.isnan(zero.flatness).all() and np.isnan(zero.skewness).all()


@pytest.mark.parametrize('P,grid,whole', [(2, [2, 1, 1], [1, 2]), (4, [2, 2, 1], [2])])
def test_the_axis_must_be_whole_on_this_rank(P, grid, whole, engine):
    from mpi4py_fft_amd import PFFT, newDistArray, spectral
    shape = (8, 8, 20)
    G = _field(shape, 3)

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=grid, wire='torch')
        ops = spectral.SpectralOps(fft)
        u = newDistArray(fft, False, rank=1)
        u[...] = G[(slice(None),) + fft.local_slice(False)]
        msgs = {}
        for axis in range(3):
            try:
                ops.structure_functions(u, axis, [1])
            except AssertionError as e:
                msgs[axis] = str(e)
        axes = ops.whole_axes()
        fft.destroy()
        return axes, msgs
    for axes, msgs in cases.run_ranks(P, body):
        assert axes == whole and sorted(msgs) == [a for a in range(3) if a not in whole]
        for axis, text in msgs.items():
            assert 'axis %d is split' % axis in text and 'whole axes of this grid are %s' % whole in text, text


@pytest.mark.parametrize('axis', [1, 2])
def test_rank_reduction_on_a_slab_grid(axis, engine):
    """The sum over the 2 ranks of a slab grid equals the one-rank table within the bound, identical bits on both ranks."""
    from mpi4py_fft_amd import PFFT, newDistArray, spectral
    shape = (8, 6, 20)
    G = _field(shape, 3)
    seps = [0, 1, 2, shape[axis] // 2, shape[axis] - 1]
    ref, mag = R.structure(G, axis, seps, lcomp=axis)

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=[2, 1, 1], wire='torch')
        ops = spectral.SpectralOps(fft)
        u = newDistArray(fft, False, rank=1)
        u[...] = G[(slice(None),) + fft.local_slice(False)]
        full = ops.structure_functions(u, axis, seps, lcomp=axis)
        local = ops.structure_functions(u, axis, seps, lcomp=axis, reduce=False).numpy().copy()
        fft.destroy()
        return full, local
    res = cases.run_ranks(2, body)
    count = int(np.prod(shape))
    for full, local in res:
        assert full.shape == (5, 3, 9) and np.array_equal(full, res[0][0]), 'ranks disagree'       # bit for bit
        R.assert_structure(full, ref, mag, count, 'axis %d, 2 ranks' % axis)
    assert np.array_equal(res[0][0], res[0][1] + res[1][1])             # rank order
    assert not np.array_equal(res[0][1], res[1][1])


def test_bad_arguments_rejected_before_touching_a_device():
    from mpi4py_fft_amd import _lib
    lib = _lib.lib()
    assert 'gfft_ps_structure' in _lib.EXPORTS and hasattr(lib, 'gfft_ps_structure')
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def i64(*v):
        return (ctypes.c_int64 * len(v))(*v)

    def i32(*v):
        return (ctypes.c_int32 * len(v))(*v)

    def call(u=p, ncomp=3, n=i64(8, 6, 20), axis=2, nsep=None, sep=i32(0, 1, 19), lcomp=-1, out=p, prec=8):
        return lib.gfft_ps_structure(u, ncomp, n, axis, (len(sep) if sep is not None else 1) if nsep is None else nsep, sep, lcomp,
                                     out, prec, None)
    INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -3
    for bad in (dict(u=None), dict(n=None), dict(sep=None), dict(out=None),                      # a null pointer
                dict(ncomp=0), dict(ncomp=-1),                                                   # ncomp < 1
                dict(nsep=0), dict(nsep=-1),                                                     # nsep < 1
                dict(axis=-1), dict(axis=3),                                                     # axis outside 0 .. 2
                dict(n=i64(-1, 6, 20)), dict(n=i64(8, -6, 20)),                                  # a negative n
                dict(sep=i32(20)), dict(sep=i32(1, -1)), dict(axis=1, sep=i32(6)), dict(n=i64(8, 6, 0), sep=i32(0)),   # a sep outside [0, n[axis])
                dict(lcomp=-2), dict(lcomp=3), dict(ncomp=1, lcomp=1),                           # lcomp outside [-1, ncomp)
                dict(prec=3), dict(prec=16)):                                                    # precision
        assert call(**bad) == INVALID, bad
    assert call(ncomp=5) == UNSUPPORTED                                                          # ncomp > 4
    assert b'4 components' in lib.gfft_last_error()
    assert call(sep=i32(*range(20)), nsep=65) == UNSUPPORTED and call(sep=i32(*([1] * 65))) == UNSUPPORTED     # nsep > 64
    assert b'64 separations' in lib.gfft_last_error()
    assert call(n=i64(2, 2, 4097), sep=i32(1, 4096)) == UNSUPPORTED                              # an axis longer than the kernel stages
    assert b'4096' in lib.gfft_last_error()
    assert call(n=i64(4097, 2, 2), axis=0, sep=i32(1)) == UNSUPPORTED and call(n=i64(2, 4097, 2), axis=1, sep=i32(1)) == UNSUPPORTED
    if not torch.cuda.is_available():
        # good calls get as far as looking for a device: the longest axis in both precisions, the most separations, no points
        assert call() == NO_DEVICE and call(lcomp=2) == NO_DEVICE and call(ncomp=4, lcomp=0, prec=4) == NO_DEVICE
        assert call(n=i64(2, 2, 4096), sep=i32(4095)) == NO_DEVICE and call(n=i64(2, 2, 4096), sep=i32(4095), prec=4) == NO_DEVICE
        assert call(n=i64(4097, 2, 20)) == NO_DEVICE and call(sep=i32(*([1] * 64))) == NO_DEVICE      # another axis may be longer
        assert call(n=i64(0, 6, 20)) == NO_DEVICE
