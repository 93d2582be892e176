"""The two LOCAL stages of a REAL slab-decomposed transform as one launch per direction (gfft_plan_create_guru2_real,
PFFT._fuse_pairs' real branch, pipeline._PairStage(real=True)): [r2c rows -> strided, into the blocks of the all-to-all
buffer] forward, [strided, from the blocks -> c2r rows] backward.  The reference's default dtype is real and its slab
grids run exactly this chain (/root/reference/mpi4py_fft/mpifft.py:313-335).  Pins: numpy's rfft2 on the same planes, the
oracle, the round trip, the two-launch form of the same plans, and the staged and pipelined paths against each other."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cases
from oracle import pfft_oracle as O

KINDS_DEFAULT = 2046              # every pair kind but bit 1 (plan_internal.h Options::fuse2_kinds)
REAL_SLAB_BITS = 512 | 1024       # FUSED_R2C_PLANES_B, FUSED_COLS_C2R_B


def _rounding(dt, nelem):
    return 4 * cases.EPS[dt] * np.log2(nelem)


@pytest.fixture(autouse=True)
def _kinds():
    """The library's default pair kinds (another test file may have left a mask of its own behind), fp32 real pairs off."""
    from mpi4py_fft_amd import _lib
    _lib.set_option('fuse2_kinds', KINDS_DEFAULT)
    yield
    _lib.set_option('fuse2_kinds', KINDS_DEFAULT)
    _lib.set_option('fuse2_f32', 1)


@pytest.fixture
def small_ring():
    """A hand-off ring of 4 planes, the producer 2 ahead: launches of 8 planes already fuse (the automatic ring wants
    ~200 MiB of planes, plan.cpp fused2_ring), so that test arrays stay oracle-sized."""
    from mpi4py_fft_amd import _lib
    _lib.set_option('fuse2_ring', 4)
    _lib.set_option('fuse2_lag', 2)
    yield
    _lib.set_option('fuse2_ring', 0)
    _lib.set_option('fuse2_lag', 0)


@pytest.fixture(scope='module')
def fake_rccl():
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    src, so = os.path.join(here, 'fake_rccl', 'fake_rccl.cpp'), os.path.join(here, 'fake_rccl', 'libfake_rccl.so')
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(['/opt/rocm/bin/hipcc', '-O2', '-std=c++17', '-fPIC', '-shared', '-x', 'hip',
                               '--offload-arch=gfx950', src, '-o', so])
    from mpi4py_fft_amd import _lib
    _lib.check_wire(_lib.lib().gfft_rccl_load(so.encode()))
    yield
    _lib.lib().gfft_rccl_load(None)


def _plans(eng, prec, n1, n2, planes, blocks, E, bstride):
    from mpi4py_fft_amd import _lib
    H = n2 // 2 + 1
    hf = eng.plan_create_guru2_real(prec, _lib.R2C, (n1, n2, H), (n2, 1, 1), (planes, n1 * n2, E), 1, 0, blocks, bstride)
    hb = eng.plan_create_guru2_real(prec, _lib.C2R, (n1, H, n2), (n2, 1, 1), (planes, E, n1 * n2), blocks, bstride, 1, 0)
    return hf, hb


def _run(eng, h, src, dst, scale):
    import torch
    from mpi4py_fft_amd import _lib
    eng.execute_ptr(h, src.data_ptr(), dst.data_ptr(), scale)
    torch.cuda.synchronize()
    _lib.check_async()
    return dst.cpu().numpy()


@pytest.mark.parametrize('dt,n1,n2,planes,blocks,pitch', [
    ('d', 1024, 1024, 16, 1, 0), ('d', 1024, 1024, 16, 2, 0), ('d', 1024, 1024, 20, 8, 24), ('d', 1024, 2048, 16, 2, 16),
    ('f', 1024, 1024, 16, 2, 0), ('f', 1024, 1024, 24, 8, 32)])
def test_guru2_real_plans_against_numpy(dt, n1, n2, planes, blocks, pitch, small_ring):
    """Forward real planes -> half-spectrum planes in `blocks` blocks of the strided axis, planes `pitch` entries further
    apart than their data; backward the mirror -- as ONE launch, against numpy's rfft2, the round trip, and the same plans
    as two stand-alone launches (the real slab bits of fuse2_kinds cleared)."""
    import torch
    from mpi4py_fft_amd import _lib
    eng = _lib.engine()
    prec = 8 if dt == 'd' else 4
    if dt == 'f':
        _lib.set_option('fuse2_f32', 2)                 # (the real fp32 pairs: measured level one-rank, off by default)
    rdt, cdt = (torch.float64, torch.complex128) if dt == 'd' else (torch.float32, torch.complex64)
    H = n2 // 2 + 1
    x = np.random.default_rng(5).standard_normal((planes, n1, n2)).astype(dt)
    nb = n1 // blocks
    E = nb * H + pitch                                   # one plane of one block: rows exactly H entries apart
    bstride = planes * E
    hf, hb = _plans(eng, prec, n1, n2, planes, blocks, E, bstride)
    assert hf is not None and hb is not None
    assert eng.plan_cost(hf)[2] == 1 and eng.plan_cost(hb)[2] == 1, (eng.plan_describe(hf), eng.plan_describe(hb))
    a = torch.from_numpy(x).cuda()
    scale = 1.0 / (n1 * n2)
    got = _run(eng, hf, a, torch.full((blocks * bstride,), float('nan'), dtype=cdt, device='cuda'), scale).reshape(blocks, planes, E)
    want = np.fft.rfftn(x.astype('d'), axes=(1, 2)) * scale
    tol = _rounding(dt, n1 * n2)
    top = np.abs(want).max()
    for j in range(blocks):
        blk = got[j, :, :nb * H].reshape(planes, nb, H)
        err = np.abs(blk - want[:, j * nb:(j + 1) * nb]).max() / top
        assert err <= tol, (j, err, tol)
        if pitch:
            assert np.isnan(got[j, :, nb * H:].real).all()              # the padding between planes is never written
    assert np.array_equal(a.cpu().numpy(), x)                           # input preserved
    buf = torch.from_numpy(got.reshape(-1)).cuda()
    keep = buf.clone()
    back = _run(eng, hb, buf, torch.full((planes, n1, n2), float('nan'), dtype=rdt, device='cuda'), 1.0)
    assert torch.equal(torch.view_as_real(buf).nan_to_num(7.0), torch.view_as_real(keep).nan_to_num(7.0))     # input preserved
    rt = np.linalg.norm(back - x) / np.linalg.norm(x)
    assert rt <= tol, (rt, tol)
    # the same plans as two stand-alone launches each: rounding apart
    _lib.set_option('fuse2_kinds', KINDS_DEFAULT & ~REAL_SLAB_BITS)
    h2f, h2b = _plans(eng, prec, n1, n2, planes, blocks, E, bstride)
    assert eng.plan_cost(h2f)[2] == 2 and eng.plan_cost(h2b)[2] == 2, (eng.plan_describe(h2f), eng.plan_describe(h2b))
    g2 = _run(eng, h2f, a, torch.full((blocks * bstride,), float('nan'), dtype=cdt, device='cuda'), scale).reshape(blocks, planes, E)
    assert np.abs(g2[:, :, :nb * H] - got[:, :, :nb * H]).max() / top <= tol
    if pitch:
        assert np.isnan(g2[:, :, nb * H:].real).all()
    b2 = _run(eng, h2b, buf, torch.full((planes, n1, n2), float('nan'), dtype=rdt, device='cuda'), 1.0)
    assert np.abs(b2 - back).max() / np.abs(x).max() <= tol
    for h in (hf, hb, h2f, h2b):
        eng.plan_destroy(h)


def test_guru2_real_refusals():
    from mpi4py_fft_amd import _lib
    eng = _lib.engine()
    n, H, npl = 1024, 513, 8
    R2C, C2R = _lib.R2C, _lib.C2R
    fc, bc, rows = (n, n, H), (n, H, n), (n, 1, 1)
    # GFFT_ERR_INVALID: blocks on the real side, a block stride below the block's extent
    with pytest.raises(_lib.GfftError):
        eng.plan_create_guru2_real(8, R2C, fc, rows, (npl, n * n, n * H), 2, npl * n * n, 1, 0)
    with pytest.raises(_lib.GfftError):
        eng.plan_create_guru2_real(8, C2R, bc, rows, (npl, n * H, n * n), 1, 0, 2, npl * n * n)
    with pytest.raises(_lib.GfftError):
        eng.plan_create_guru2_real(8, R2C, fc, rows, (npl, n * n, 128 * H), 1, 0, 8, 128 * H - 1)
    # GFFT_ERR_UNSUPPORTED (None): 16 blocks, a strided row axis, a complex kind, lengths without register kernels
    assert eng.plan_create_guru2_real(8, R2C, fc, rows, (npl, n * n, 64 * H), 1, 0, 16, npl * 64 * H) is None
    assert eng.plan_create_guru2_real(8, R2C, fc, (n, 2, 1), (npl, n * n, n * H)) is None
    assert eng.plan_create_guru2_real(8, -1, fc, rows, (npl, n * n, n * H)) is None
    assert eng.plan_create_guru2_real(8, +1, bc, rows, (npl, n * H, n * n)) is None
    assert eng.plan_create_guru2_real(8, R2C, (521, n, H), rows, (npl, 521 * n, 521 * H)) is None
    assert eng.plan_create_guru2_real(8, R2C, (n, 1026, 514), (1026, 1, 1), (npl, n * 1026, n * 514)) is None
    # ... and the complex entry still refuses real kinds
    assert eng.plan_create_guru2(8, R2C, (n, n, n), (n, 1, 1), (npl, n * n, n * n)) is None


@pytest.mark.parametrize('P,shape,dt', [(2, (32, 1024, 1024), 'd'), (4, (64, 1024, 1024), 'd'), (8, (128, 1024, 1024), 'd'),
                                        (2, (32, 1024, 2048), 'd'), (2, (32, 1024, 1024), 'f')])
def test_real_slab_grid_runs_its_local_stages_as_one_launch(P, shape, dt, small_ring, fake_rccl, monkeypatch):
    """PFFT of real input on a slab grid: stage by stage (fuse_pairs=False), staged with the pair, pipelined with the pair
    per chunk of planes -- against the oracle, each other and the round trip; the caller's arrays are left as they were."""
    import torch
    from mpi4py_fft_amd import PFFT, newDistArray, pipeline, _lib
    monkeypatch.setattr(pipeline.Pipeline, 'MIN_CHUNK_BYTES', 0)
    if dt == 'f':
        _lib.set_option('fuse2_f32', 2)
    G = O.rng_array(shape, dt, 29)
    ref = O.OPFFT(P, shape, dtype=dt, grid=[P, 1, 1])
    want = ref.forward(ref.scatter(G))
    nelem = float(np.prod(shape))
    tol, rtol = cases.tol_for(dt, nelem), _rounding(dt, nelem)

    def body(comm):
        r = comm.Get_rank()
        kw = dict(dtype=dt, grid=[P, 1, 1], exchange='direct')
        plain = PFFT(comm, shape, wire='torch', fuse_pairs=False, **kw)
        staged = PFFT(comm, shape, wire='torch', **kw)
        piped = PFFT(comm, shape, wire='native', **kw)
        m = dict(plain_pairs=list(plain.forward._pairs), fwd_pairs=list(staged.forward._pairs),
                 bck_pairs=list(staged.backward._pairs), layout=piped.pipeline and piped.pipeline.layout,
                 chunks=piped.pipeline and piped.pipeline.describe()[0]['chunks'])
        u = newDistArray(staged, False)
        u[...] = G[staged.local_slice(False)]
        keep = np.asarray(u).copy()
        w = want[r]
        scale = np.abs(w).max()
        a0 = np.asarray(plain.forward(u)).copy()
        a = np.asarray(staged.forward(u)).copy()
        b = np.asarray(piped.forward(u)).copy()
        out = newDistArray(piped, True)
        piped.forward(u, out)                          # caller's arrays read / written directly
        m['staged_eq_piped'] = np.array_equal(a, b) and np.array_equal(a, np.asarray(out))
        m['u_kept'] = np.array_equal(np.asarray(u), keep)
        m['err_staged'] = np.abs(a - w).max() / scale
        m['err_plain'] = np.abs(a0 - w).max() / scale
        m['err_pair_vs_plain'] = np.abs(a - a0).max() / scale
        outk = np.asarray(out).copy()
        sl = staged.local_slice(False)
        norm = np.linalg.norm(G[sl])
        r0 = np.asarray(plain.backward()).copy()
        ra = np.asarray(staged.backward()).copy()
        rb = np.asarray(piped.backward()).copy()
        back = newDistArray(piped, False)
        piped.backward(out, back, normalize=True)
        m['out_kept'] = np.array_equal(np.asarray(out), outk)
        m['bwd_staged_eq_piped'] = np.array_equal(ra, rb)
        m['rt_staged'] = np.linalg.norm(ra - G[sl]) / norm
        m['rt_plain'] = np.linalg.norm(r0 - G[sl]) / norm
        m['normalize_ok'] = np.allclose(np.asarray(back) * nelem, rb, rtol=1e-5 if dt == 'f' else 1e-12, atol=0)
        for f in (plain, staged, piped):
            f.destroy()
        torch.cuda.synchronize()
        return m
    for r, m in enumerate(cases.run_ranks(P, body)):
        assert m['plain_pairs'] == [] and m['fwd_pairs'] == [0] and m['bck_pairs'] == [1], m
        assert m['layout'] == 'slab-pair' and m['chunks'] > 1, m
        assert m['staged_eq_piped'] and m['bwd_staged_eq_piped'], 'pipelined pair differs from the staged pair'
        assert m['u_kept'] and m['out_kept'], m
        assert m['err_staged'] <= tol and m['err_plain'] <= tol, (m, tol)
        assert m['err_pair_vs_plain'] <= rtol, (m, rtol)                  # one launch against two: rounding only
        assert m['rt_staged'] <= rtol and m['rt_plain'] <= rtol, (m, rtol)
        assert m['normalize_ok'], m


def test_exchange_check_on_the_piped_real_slab_pair(small_ring, fake_rccl, monkeypatch):
    """selftest.exchange_check -- the positional gate `bench.py --gpus N` admits plans with -- is bit-exact on the pipelined
    real slab pair."""
    from mpi4py_fft_amd import PFFT, pipeline, selftest
    monkeypatch.setattr(pipeline.Pipeline, 'MIN_CHUNK_BYTES', 0)
    P, shape = 2, (32, 1024, 1024)

    def body(comm):
        fft = PFFT(comm, shape, dtype='d', grid=[P, 1, 1], exchange='direct', wire='native')
        layout = fft.pipeline and fft.pipeline.layout
        chk = selftest.exchange_check(fft, comm)
        fft.destroy()
        return layout, chk
    for layout, chk in cases.run_ranks(P, body):
        assert layout == 'slab-pair'
        assert chk['result'] == 'bit-exact', chk
