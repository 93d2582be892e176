"""Rounding-level and impulse guards of the 3/2-rule truncating store and zero-padding load (libfft.py:263-311 of the model) --
the fourth family beside the complex, the real and the real-to-real ones (tests/test_gpu_rounding_guard.py,
tests/test_gpu_r2r_guard.py).

The rule is written twice in the library: as load / store adapters of the register kernels (fft_pow2_impl.h tile_load_pad /
tile_store_trunc: lower band, upper band shifted by n - N, the fold of entry n - h onto h, the halving on the way back, the
parity of the REAL rule taken from the stored half-length m), instantiated per kernel family and mapping and with the block
offsets of exchange buffers (PassDesc::tr_jump / tr_lgper); and as the stand-alone trunc_kernel of pack.hip for every length
without adapters.  A wrong band edge, a dropped fold or the parity taken from the wrong length touch one or two entries of a
line: on random data an O(1 / sqrt(n)) error in one entry, far below the contract tolerances.  Here:

  * the impulse family (`tests/cases.py trunc_impulse_errors`; exact answers held against the oracle, and shown to see every
    such mistake, by tests/test_trunc_exact_host.py) over every path, mapping and dtype, at the allowance of the complex and
    real families;
  * the proof that it reads the padded plans' own instantiations: a twiddle entry off by 1e-9 / 1e-5 fails it;
  * the stand-alone kernels bit for bit against a numpy restatement of the rule in the field's precision;
  * truncation together with exchange-buffer blocks (gfft_plan_set_truncation + gfft_plan_set_split) bit for bit against
    the packed form of what the truncation-only plan gives.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pfft_oracle as O
from tests import cases

# In units of eps log2 n of the exact answer's peak: the constant of the complex and the real family.  Derived, not fitted: the
# adapters add ONE addition of two entries, each inside that bound already, on a peak of 2; the factors 2 and 0.5 are exact.
# Measured (tools/trunc_impulse_probe.py, profiles/trunc_impulse_probe.txt), worst ratio per path over mappings and dtypes, with
# the unpadded plan of the same length, mapping and dtype on the same inputs in brackets: fused 0.32 (0.28) fp64 / 0.30 (0.30)
# fp32; stand-alone 0.41 (0.41) fp64, n = 8192 / 0.37 (0.35) fp32, n = 521.  The adapters add nothing measurable.
IMPULSE_FACTOR = 2.0


def allowance(dt, n):
    return IMPULSE_FACTOR * cases.EPS[dt] * np.log2(n)


@pytest.mark.parametrize('mapping', cases.TRUNC_MAPPINGS)
@pytest.mark.parametrize('dt', ['D', 'F', 'd', 'f'])
def test_trunc_impulse_responses_at_rounding_level(dt, mapping):
    """Every (n -> kept) of cases.TRUNC_LENGTHS through FFT(..., padding=n / kept): the path each plan took asserted against
    plan.cpp fused_pad_ok (cases.trunc_expected_path), every line of a batch that is no multiple of a kernel tile against its
    exact answer, forward and backward."""
    worst = 0.0
    for n, kept, family in cases.TRUNC_CASES:
        text = []
        ef, eb = cases.trunc_impulse_errors(n, kept, dt, mapping, describe=text)
        path = cases.trunc_path(text, n, mapping)
        assert path in cases.trunc_expected_path(n, family, dt, mapping), (n, kept, dt, mapping, family, path, text)
        unit = cases.EPS[dt] * np.log2(n)
        cases._note('trimp', dt, n, max(ef, eb))
        print('trimp %s %-6s %5d -> %-5d %-11s fwd %.2e (%.2f eps log2 n)  bwd %.2e (%.2f)' % (dt, mapping, n, kept, path, ef, ef / unit, eb, eb / unit))
        worst = max(worst, ef / unit, eb / unit)
        assert ef <= allowance(dt, n), (n, kept, dt, mapping, path, 'forward', ef, ef / unit)
        assert eb <= allowance(dt, n), (n, kept, dt, mapping, path, 'backward', eb, eb / unit)
    assert worst > 0          # (the transforms did run)


@pytest.fixture
def wrong_twiddle():
    from mpi4py_fft_amd import _lib

    def arm(index, exponent, length=0):
        _lib.set_option('debug_tw_len', length)
        _lib.set_option('debug_tw_index', index)
        _lib.set_option('debug_tw_exp', exponent)
    yield arm
    _lib.set_option('debug_tw_exp', 0)
    _lib.set_option('debug_tw_index', 1)
    _lib.set_option('debug_tw_len', 0)


@pytest.mark.parametrize('dt,exponent', [('D', 9), ('F', 5)])
@pytest.mark.parametrize('n,kept', [(64, 32), (768, 512), (960, 640)])
def test_one_wrong_twiddle_entry_fails_the_padded_family(n, kept, dt, exponent, wrong_twiddle):
    """Padded plans made while the hook is armed read tables whose entry 1 is off by 10^-exponent in its real part: the family
    must name it at full size (0.9 delta, as the unpadded families do) in rows and cols, so it does run the PF_TRUNC
    instantiations with their tables -- a family that compared a padded plan with itself would not notice.  Plans made after
    disarming pass again."""
    delta = 10.0 ** -exponent
    wrong_twiddle(1, exponent)
    for mapping in ('rows', 'cols'):
        text = []
        ef, eb = cases.trunc_impulse_errors(n, kept, dt, mapping, describe=text)
        assert cases.trunc_path(text, n, mapping) == 'fused', text
        pf = 2.0 if kept % 2 == 0 else 1.0                            # back to absolute errors (complex: backward peak 1)
        err = max(ef * pf, eb)
        assert max(ef, eb) > allowance(dt, n) and err >= 0.9 * delta, (n, kept, dt, mapping, ef, eb, err / delta)
    wrong_twiddle(1, 0)
    for mapping in ('rows', 'cols'):
        ef, eb = cases.trunc_impulse_errors(n, kept, dt, mapping)     # plans made now read the exact tables
        assert ef <= allowance(dt, n) and eb <= allowance(dt, n), (n, kept, dt, mapping, ef, eb)


# ---- the stand-alone kernels (pack.hip trunc_kernel), bit for bit ------------------------------------------------------
def restate_truncate(P, axis, keep, is_real, scale):
    """The model's truncation (libfft.py:263-284) in P's own precision, then the scale -- the kernel multiplies AFTER the fold.
    Complex: entries 0 ... h, then the last h entries ADDED onto the last h places (for an even keep the place h gets two);
    real: the first keep entries, the last one doubled and made real when keep is even."""
    P = np.moveaxis(P, axis, -1)
    n, h = P.shape[-1], keep // 2
    if is_real:
        T = P[..., :keep].copy()
        if keep % 2 == 0:
            T[..., keep - 1] = 2 * T[..., keep - 1].real          # (imaginary part +0.0)
    else:
        T = np.zeros(P.shape[:-1] + (keep,), dtype=P.dtype)
        T[..., :h + 1] = P[..., :h + 1]
        if h > 0:
            T[..., keep - h:] += P[..., n - h:]
    s = T.real.dtype.type(scale)
    R = np.empty_like(T)
    R.real, R.imag = T.real * s, T.imag * s
    return np.ascontiguousarray(np.moveaxis(R, -1, axis))


def restate_pad(T, axis, n, is_real):
    """The model's zero padding (libfft.py:286-311) in T's own precision; everything outside the kept band is +0.0."""
    T = np.moveaxis(T, axis, -1)
    keep = T.shape[-1]
    h = keep // 2
    V = np.zeros(T.shape[:-1] + (n,), dtype=T.dtype)
    half = T.real.dtype.type(0.5)
    if is_real:
        V[..., :keep] = T
        if keep % 2 == 0:
            V[..., keep - 1] = half * T[..., keep - 1].real
    else:
        V[..., :h + 1] = T[..., :h + 1]
        if h > 0:
            V[..., n - h:] = T[..., keep - h:]
        if keep % 2 == 0:
            for k in (h, n - h):
                V[..., k].real *= half
                V[..., k].imag *= half
    return np.ascontiguousarray(np.moveaxis(V, -1, axis))


def ulps(got, ref):
    """max over both parts of |got - ref| in units of ref's spacing."""
    worst = 0.0
    for g, r in ((got.real, ref.real), (got.imag, ref.imag)):
        worst = max(worst, float((np.abs(g - r) / np.spacing(np.abs(r))).max()))
    return worst


@pytest.mark.parametrize('is_real', [False, True], ids=['complex', 'real'])
@pytest.mark.parametrize('cdt', ['D', 'F'])
def test_standalone_truncate_and_pad_bit_for_bit(cdt, is_real):
    from mpi4py_fft_amd import _lib, asdevice
    eng = _lib.engine()
    prec = _lib.precision_of(cdt)
    for n, keep in ((12, 8), (13, 9), (18, 12), (48, 31), (48, 32), (9, 6)):
        for shape, axis in (((5, n, 3), 1), ((n, 7), 0), ((4, n), 1)):
            tshape = shape[:axis] + (keep,) + shape[axis + 1:]
            P = O.rng_array(shape, cdt, 31)
            for scale in (1.0, 0.25, 1.0 / 48):
                out = asdevice(np.full(tshape, np.nan, dtype=cdt))
                eng.truncate(asdevice(P).tensor, out.tensor, shape, axis, keep, is_real, prec, scale)
                got, ref = np.asarray(out), restate_truncate(P, axis, keep, is_real, scale)
                assert got.shape == ref.shape and got.dtype == ref.dtype
                what = (n, keep, shape, axis, cdt, is_real, scale)
                if scale == 1.0 / 48:
                    assert not np.isnan(got).any() and ulps(got, ref) <= 1.0, (what, ulps(got, ref))
                else:
                    assert np.array_equal(got, ref), (what, np.abs(got - ref).max())
                if is_real and keep % 2 == 0:
                    last = np.take(got, keep - 1, axis=axis).imag
                    assert np.array_equal(last, np.zeros_like(last)) and not np.signbit(last).any(), what
            T = O.rng_array(tshape, cdt, 32)
            out = asdevice(np.full(shape, np.nan, dtype=cdt))
            eng.pad(asdevice(T).tensor, out.tensor, shape, axis, keep, is_real, prec)
            got, ref = np.asarray(out), restate_pad(T, axis, n, is_real)
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (n, keep, shape, axis, cdt, is_real, np.abs(got - ref).max())
            for g, r in ((got.real, ref.real), (got.imag, ref.imag)):
                assert not np.signbit(g[r == 0]).any(), (n, keep, shape, axis, cdt, is_real, 'zeros are +0.0')


# ---- truncation together with exchange-buffer blocks ---------------------------------------------------------------
def _packed(a, axis, p):
    n = a.shape[axis]
    return np.concatenate([np.ascontiguousarray(np.take(a, range(s, s + m), axis=axis)).reshape(-1)
                           for m, s in (O.blockdist(n, p, i) for i in range(p))])


class _Truncated:
    """The forward and the backward plan of one axis with the truncation fused, as libfft.FFT makes them (planned against the
    full spectrum's shape only), run out of place into arrays that start as NaN."""
    def __init__(self, shape, axis, dt, keep):
        from mpi4py_fft_amd import fftw, zeros
        from mpi4py_fft_amd.libfft import _ShapeOnly
        self.real = dt in 'df'
        self.cdt = dt.upper()
        self.shape, self.dt = tuple(shape), dt
        full = list(shape)
        if self.real:
            full[axis] = full[axis] // 2 + 1
        self.tshape = tuple(shape[:axis]) + (keep,) + tuple(shape[axis + 1:])
        U, ghost = zeros(shape, dt), _ShapeOnly(full, self.cdt)
        s = (shape[axis],)
        self.fwd = (fftw.rfftn if self.real else fftw.fftn)(U, s=s, axes=(axis,), output_array=ghost)
        self.bck = (fftw.irfftn if self.real else fftw.ifftn)(ghost, s=s, axes=(axis,), output_array=U)
        assert self.fwd.set_truncation(keep) and self.bck.set_truncation(keep), (shape, axis, dt, keep)

    def forward(self, x):
        from mpi4py_fft_amd import asdevice
        out = asdevice(np.full(self.tshape, np.nan, dtype=self.cdt))
        self.fwd.execute_scaled(asdevice(np.ascontiguousarray(x, dtype=self.dt)), out, 1.0)
        return np.asarray(out).copy()

    def backward(self, spec):
        from mpi4py_fft_amd import asdevice
        out = asdevice(np.full(self.shape, np.nan, dtype=self.dt))
        self.bck.execute_scaled(asdevice(np.ascontiguousarray(spec, dtype=self.cdt).reshape(self.tshape)), out, 1.0)
        return np.asarray(out).copy()

    def destroy(self):
        self.fwd.destroy()
        self.bck.destroy()


def _split_inputs(n, kept, dt, mapping):
    """(shape, axis, keep, [(x, spectrum) ...]): random data and the impulse family of the mapping."""
    shape, axis, x, wf, spec, wb, pf, pb = cases.trunc_impulse_case(n, kept, dt, mapping)
    keep = wf.shape[axis]
    return shape, axis, keep, [(O.rng_array(shape, dt, 41), O.rng_array(wf.shape, dt.upper(), 42)), (x, spec)]


def _check_split(n, kept, dt, mapping, blocks):
    shape, axis, keep, inputs = _split_inputs(n, kept, dt, mapping)
    nat = _Truncated(shape, axis, dt, keep)
    want = [(nat.forward(x), nat.backward(s)) for x, s in inputs]
    assert not any(np.isnan(f).any() or np.isnan(b).any() for f, b in want)
    for p in blocks:
        t = _Truncated(shape, axis, dt, keep)
        assert t.fwd.set_split(1, p) and t.bck.set_split(0, p), (n, kept, dt, mapping, p)
        for (x, s), (wf_, wb_) in zip(inputs, want):
            got = t.forward(x).reshape(-1)
            assert np.array_equal(got, _packed(wf_, axis, p)), (n, kept, dt, mapping, p, 'truncating store into blocks')
            got = t.backward(_packed(s.astype(dt.upper()), axis, p))
            assert np.array_equal(got, wb_), (n, kept, dt, mapping, p, 'zero-padding load from blocks')
        # ... and back to the natural layout
        assert t.fwd.set_split(1, 1) and t.bck.set_split(0, 1)
        assert np.array_equal(t.forward(inputs[0][0]), want[0][0]) and np.array_equal(t.backward(inputs[0][1]), want[0][1])
        t.destroy()
    nat.destroy()


@pytest.mark.parametrize('mapping', ['rows', 'cols', 'middle'])
@pytest.mark.parametrize('dt', ['D', 'F'])
@pytest.mark.parametrize('n,kept', [(96, 64), (48, 32), (1536, 1024), (64, 32)])
def test_truncation_with_exchange_blocks_complex(n, kept, dt, mapping):
    """plan.set_truncation(kept) then plan.set_split(side, p): the forward plan WRITES, the backward plan READS, exactly
    _packed(...) of what the truncation-only plan produces -- equal blocks of the KEPT entries (PassDesc::tr_jump / tr_lgper),
    which only the distributed tests reached, and only by comparing two launch forms of the same code."""
    _check_split(n, kept, dt, mapping, (2, 4, 8))


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('n,kept', [(96, 64), (64, 43)])
def test_truncation_with_exchange_blocks_real_rows(n, kept, dt):
    """Packed-real rows: the blocks follow the block rule over the m kept half-spectrum entries (33 and 22: never even)."""
    _check_split(n, kept, dt, 'rows', (2, 3, 4))


@pytest.mark.parametrize('dt', ['D', 'F'])
def test_truncation_with_exchange_blocks_refusals(dt):
    """The documented refusals return False and leave the plan's results as they were: a block count that does not divide the
    kept length, kept entries per block that are no power of two, a block count that is no power of two."""
    for n, kept, p in ((48, 31, 2), (96, 48, 2), (96, 48, 4), (96, 64, 3), (96, 60, 4)):
        shape, axis, keep, inputs = _split_inputs(n, kept, dt, 'rows')
        x, s = inputs[0]
        t = _Truncated(shape, axis, dt, keep)
        wf_, wb_ = t.forward(x), t.backward(s)
        assert t.fwd.set_split(1, p) is False and t.bck.set_split(0, p) is False, (n, kept, p)
        assert np.array_equal(t.forward(x), wf_) and np.array_equal(t.backward(s), wb_), (n, kept, p)
        t.destroy()
