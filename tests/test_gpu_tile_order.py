"""Option `tile_order` (PassDesc::order, csrc/gfft_internal.h): the order IN TIME in which the stand-alone strided pass of the
complex fp64 power-of-two 3-D schedule requests its tiles and rows.  It changes no byte, no layout and no operation per
element, so forward and backward outputs must be BIT-IDENTICAL to those of the plain order (tile_order = 0) -- no tolerance."""
import pytest

pytestmark = pytest.mark.gpu

# every field of the order word, alone and combined (gfft_internal.h): XCD start offsets, slot rotations, thread-row
# rotations, planes interleaved inside an XCD (2 / 4 / 8 planes, 37 / 1 / 63 planes apart), the hash by position
ORDERS = [-1, 65536, 197, 2 << 12, (1 << 12) | (1 << 18), (1 << 14) | (1 << 18), 2 << 14, 2 << 16, (3 << 16) | (1 << 19),
          (1 << 16) | (63 << 19), 323 | (1 << 16) | (2 << 12) | (1 << 14) | (1 << 18)]


def _fill(t, seed):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    r = torch.view_as_real(t)
    step = max(1, r.shape[0] // 16)
    for i in range(0, r.shape[0], step):      # in slabs: bounds the temporary memory at full size
        r[i:i + step].copy_(torch.randn(r[i:i + step].shape, generator=g, device='cuda', dtype=r.dtype))


def _check(shape, orders):
    import torch
    from mpi4py_fft_amd import PFFT, newDistArray, comm, _lib
    _lib.set_option('fused3_min_mib', 0)          # the 3-D schedule whatever the size
    try:
        fft = PFFT(comm.COMM_SELF, shape, dtype='D')
        desc = fft._fused_plans[0]._eng.plan_describe(fft._fused_plans[0]._plan)
        assert 'padded-pitch workspace' in desc or '3-D schedule' in desc, desc
        u, uh = newDistArray(fft, False), newDistArray(fft, True)
        _fill(u.tensor, 11)
        u0 = u.tensor.clone()
        _lib.set_option('tile_order', 0)
        fft.forward(u, uh)
        assert torch.equal(u.tensor, u0)
        ref_f = uh.tensor.clone()
        fft.backward(uh, u)
        ref_b = u.tensor.clone()
        assert float((ref_b - u0).abs().max().item()) < 1e-10          # (a transform was computed at all)
        for o in orders:
            _lib.set_option('tile_order', o)
            u.tensor.copy_(u0)
            uh.tensor.zero_()
            fft.forward(u, uh)
            assert torch.equal(uh.tensor, ref_f), ('forward', shape, o)
            uh.tensor.copy_(ref_f)
            u.tensor.zero_()
            fft.backward(uh, u)
            assert torch.equal(u.tensor, ref_b), ('backward', shape, o)
        fft.destroy()
    finally:
        _lib.set_option('tile_order', -1)
        _lib.set_option('fused3_min_mib', 32)


@pytest.mark.parametrize('shape', [(128, 128, 128), (256, 512, 128), (64, 1024, 128), (16, 1024, 64)])
def test_tile_order_outputs_bit_identical_small(shape):
    """128^3 and (256,512,128) as the issue sets them (their strided kernels take no order: the option must be inert there),
    plus two shapes whose axis-1 pass IS the 1024-point kernel that takes one -- 8 and 2 planes of 8 / 4 tiles per XCD
    (orders that do not fit such a walk fall back to the plain one, fft_pow2_impl.h launch_pow2_one)."""
    _check(shape, ORDERS)


def test_tile_order_outputs_bit_identical_1024cubed():
    """The headline configuration at full size (five arrays of 16 GiB next to the plan's workspace; the guard of
    tests/test_gpu_large.py)."""
    from tests.test_gpu_large import _free_hbm
    if _free_hbm() < 130 * 2 ** 30:
        pytest.skip('needs ~130 GiB of HBM')
    _check((1024, 1024, 1024), ORDERS)
