"""CPU tests of the REAL slab pair (gfft_plan_create_guru2_real, PFFT._fuse_pairs' real branch): the C ABI declares and
exports the entry and refuses bad geometry before it touches a device; with a checker engine that has the entry, a real
transform on a slab grid runs its first two stages as the pair, and the block / plane geometry of the half-spectrum side
(rows of N2 / 2 + 1 entries) gives the oracle's answer -- without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import cases
from tests.host_engine import HostEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_guru2_real_is_declared_and_exported():
    from mpi4py_fft_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gfft.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+gfft_plan_create_guru2_real\s*\(', text)
    assert hasattr(_lib.lib(), 'gfft_plan_create_guru2_real')
    assert 'gfft_plan_create_guru2_real' in _lib.EXPORTS
    assert hasattr(_lib.HipEngine, 'plan_create_guru2_real')


def _create(prec, kind, cols, rows, planes, in_blocks=1, in_bs=0, out_blocks=1, out_bs=0):
    from mpi4py_fft_amd import _lib
    h = ctypes.c_void_p()
    io = lambda d: ctypes.byref(_lib.IoDim(*[int(x) for x in d]))
    return _lib.lib().gfft_plan_create_guru2_real(ctypes.byref(h), prec, kind, io(cols), io(rows), io(planes),
                                                  in_blocks, in_bs, out_blocks, out_bs)


def test_guru2_real_rejects_bad_geometry_before_touching_a_device():
    """GFFT_ERR_INVALID (-1) for non-positive strides, overlapping rows, blocks on the real side and a block stride below a
    block's extent -- decided from the arguments alone, ahead of any device call."""
    from mpi4py_fft_amd import _lib
    n1, n2, H, npl = 1024, 1024, 513, 4
    R2C, C2R = _lib.R2C, _lib.C2R
    fwd_cols, bwd_cols, rows = (n1, n2, H), (n1, H, n2), (n2, 1, 1)
    assert _create(8, R2C, (n1, 0, H), rows, (npl, n1 * n2, n1 * H)) == -1                 # stride 0
    assert _create(8, R2C, fwd_cols, rows, (npl, n1 * n2, -1)) == -1                       # negative plane stride
    assert _create(8, C2R, (n1, H - 1, n2), rows, (npl, n1 * H, n1 * n2)) == -1            # half-spectrum rows overlap
    assert _create(8, R2C, fwd_cols, rows, (npl, n1 * n2, n1 * H), 2, npl * n1 * n2) == -1        # blocks on the real input
    assert _create(8, C2R, bwd_cols, rows, (npl, n1 * H, n1 * n2), 1, 0, 2, npl * n1 * n2) == -1  # ... on the real output
    assert _create(8, R2C, fwd_cols, rows, (npl, n1 * n2, n1 * H), 1, 0, 4, 0) == -1                # block stride 0
    assert _create(8, C2R, bwd_cols, rows, (npl, 256 * H, n1 * n2), 4, 256 * H - 1) == -1          # one entry short
    assert _create(8, R2C, fwd_cols, rows, (0, n1 * n2, n1 * H)) == -1                     # no planes


class RealPairEngine(HostEngine):
    """The checker engine plus a numpy gfft_plan_create_guru2_real and its execute (HostEngine._execute_guru2 for real
    planes): the geometry of both sides is applied element by element, so a wrong stride, block jump or H shows."""
    def plan_create_guru2_real(self, precision, kind, cols, rows, planes, in_blocks=1, in_block_stride=0, out_blocks=1,
                               out_block_stride=0):
        n1, n2 = int(cols[0]), int(rows[0])
        m = n2 // 2
        if n1 & (n1 - 1) or n1 < 16 or n2 % 2 or m & (m - 1) or m < 16 or tuple(rows[1:]) != (1, 1):
            return None
        nb = in_blocks if kind == 2 else out_blocks
        if (out_blocks if kind == 2 else in_blocks) != 1 or nb & (nb - 1) or nb > 8 or n1 % nb:
            return None
        return dict(guru2_real=True, precision=precision, kind=kind, cols=tuple(int(x) for x in cols), n2=n2,
                    planes=tuple(int(x) for x in planes), inb=(in_blocks, in_block_stride), outb=(out_blocks, out_block_stride))

    def plan_cost(self, h):
        return (0.0, 0.0, 1) if h.get('guru2_real') else super().plan_cost(h)

    def execute_ptr(self, h, ptr_in, ptr_out, scale, stream=None):
        if not h.get('guru2_real'):
            return super().execute_ptr(h, ptr_in, ptr_out, scale, stream)
        rdt = np.float64 if h['precision'] == 8 else np.float32
        cdt = np.complex128 if h['precision'] == 8 else np.complex64
        n1, c_i, c_o = h['cols']
        n2 = h['n2']
        H = n2 // 2 + 1
        npl, p_i, p_o = h['planes']
        fwd = h['kind'] == -2

        def offsets(which, width):
            es, ps = (c_i, p_i) if which == 0 else (c_o, p_o)
            nb, bs = h['inb'] if which == 0 else h['outb']
            e = np.arange(n1)
            per = n1 // nb
            line = (e // per) * bs + (e % per) * es if nb > 1 else e * es
            return np.arange(npl)[:, None, None] * ps + line[None, :, None] + np.arange(width)[None, None, :]

        def view(ptr, off, dt):
            isz = np.dtype(dt).itemsize
            return np.frombuffer((ctypes.c_char * ((int(off.max()) + 1) * isz)).from_address(ptr), dtype=dt)
        oi, oo = offsets(0, n2 if fwd else H), offsets(1, H if fwd else n2)
        fin, fout = view(ptr_in, oi, rdt if fwd else cdt), view(ptr_out, oo, cdt if fwd else rdt)
        a = fin[oi]
        r = np.fft.rfft2(a, axes=(1, 2)) if fwd else np.fft.irfft2(a, s=(n1, n2), axes=(1, 2)) * (n1 * n2)
        fout[oo] = (r * scale).astype(cdt if fwd else rdt)


@pytest.fixture
def real_pair_engine():
    from mpi4py_fft_amd import _lib
    old = _lib.set_engine(RealPairEngine())
    yield
    _lib.set_engine(old)


@pytest.mark.parametrize('P', [2, 4])
def test_real_slab_grid_takes_the_real_pair(P, real_pair_engine):
    """_fuse_pairs takes the real branch: the staged forward runs stages 0 + 1 as the pair, the backward its mirror."""
    from mpi4py_fft_amd import PFFT
    shape = (8 * P, 32, 32)

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=[P, 1, 1], wire='torch')
        got = (list(fft.forward._pairs), list(fft.backward._pairs), len(fft._pair_plans))
        off = PFFT(comm, shape, dtype='d', grid=[P, 1, 1], wire='torch', fuse_pairs=False)
        got += (list(off.forward._pairs),)
        fft.destroy()
        off.destroy()
        return got
    for fwd, bck, nplans, off in cases.run_ranks(P, body):
        assert fwd == [0] and bck == [1] and nplans == 2 and off == []


@pytest.mark.parametrize('P', [2, 4])
def test_real_slab_pair_matches_the_oracle(P, real_pair_engine):
    """The pair's block / plane geometry with H = N2 / 2 + 1 on the half-spectrum side: forward values, round trip and the
    global DFT against the oracle."""
    cases.check_pfft_vs_oracle(P, (8 * P, 32, 32), 'd', grid=[P, 1, 1])


def test_complex_input_keeps_the_complex_branch(real_pair_engine):
    from mpi4py_fft_amd import PFFT
    P, shape = 2, (16, 32, 32)

    def body(comm):
        fft = PFFT(comm, shape, dtype='D', grid=[P, 1, 1], wire='torch')
        kinds = [h.get('guru2', False) for h in fft._pair_plans]
        fft.destroy()
        return kinds
    for kinds in cases.run_ranks(P, body):
        assert kinds == [True, True]
