"""The test of the r2r impulse tests (host only, no GPU, no library).

`tests/cases.py r2r_exact_impulse` is the analytic answer the GPU guards of tests/test_gpu_r2r_guard.py compare against; a
wrong formula there would make them rest on nothing.  So:

  * the closed forms are held against scipy.fft.dct / dst (norm=None) at edge and interior positions -- both sides carry
    float64 rounding only, hence 4 eps64 log2(2n) of the peak value 2;
  * a numpy EMULATION of the library's decomposition -- pre, post, pos0, idx0, N rebuilt from the comment block above
    plan.cpp get_r2r_tables, the tables rounded to the working precision, the inner transform scipy.fft.fft kept in
    complex64 / complex128 -- measures what the decomposition itself loses, with none of the code under test: the
    allowance R2R_IMPULSE_FACTOR = 2.0 (in units of 2 eps log2 N) is judged against that figure, which is re-asserted here
    with the cap 1.0;
  * the same emulation with ONE table entry off by delta gives the 0.9 delta the armed-hook tests ask for: the position list
    shows such an entry at >= 0.98 delta for every kind, either table, and every length from 16 to 4096.
"""
import numpy as np
import pytest
import scipy.fft

from tests import cases

KINDS = sorted(cases.R2R_NAMES)
SCIPY = {cases.REDFT00: (scipy.fft.dct, 1), cases.REDFT10: (scipy.fft.dct, 2), cases.REDFT01: (scipy.fft.dct, 3),
         cases.REDFT11: (scipy.fft.dct, 4), cases.RODFT00: (scipy.fft.dst, 1), cases.RODFT10: (scipy.fft.dst, 2),
         cases.RODFT01: (scipy.fft.dst, 3), cases.RODFT11: (scipy.fft.dst, 4)}
EPS64 = 2.0 ** -52


@pytest.mark.parametrize('kind', KINDS, ids=[cases.R2R_NAMES[k] for k in KINDS])
def test_closed_forms_against_scipy(kind):
    f, typ = SCIPY[kind]
    worst = 0.0
    for n in (2, 3, 5, 16, 31, 33, 64, 257, 1000, 2048):
        for j in sorted({0, 1, n - 1, n - 2, n // 2, n // 3 + 1} & set(range(n))):
            x = np.zeros(n)
            x[j] = 1
            err = float(np.abs(cases.r2r_exact_impulse(kind, n, j) - f(x, type=typ, norm=None)).max())
            worst = max(worst, err)
            assert err <= 4 * EPS64 * np.log2(2 * n) * 2, (cases.R2R_NAMES[kind], n, j, err)
    print('%s closed form vs scipy: worst %.2e' % (cases.R2R_NAMES[kind], worst))


def test_exact_impulse_is_float64_of_a_long_double_result_and_hits_both_edges():
    y = cases.r2r_exact_impulse(cases.REDFT00, 9, 0)
    assert y.dtype == np.float64 and np.array_equal(y, np.ones(9))                    # weight 1 at j = 0 ...
    assert np.array_equal(cases.r2r_exact_impulse(cases.REDFT00, 9, 8), (-1.0) ** np.arange(9))    # ... and at j = n - 1
    assert np.array_equal(cases.r2r_exact_impulse(cases.RODFT01, 6, 5), (-1.0) ** np.arange(6))
    for N in (14, 16, 20, 64, 4096):
        for kind in KINDS:
            n = cases.r2r_points(kind, N)
            pos = cases.r2r_positions(n)
            assert len(pos) == 16 and all(0 <= j < n for j in pos) and {0, 1 % n, n - 1} <= set(pos), (kind, N, pos)


@pytest.mark.parametrize('mapping', cases.R2R_MAPPINGS)
def test_impulse_batches_are_what_scipy_transforms_along_the_axis(mapping):
    """The batches the GPU guard feeds (cases.r2r_impulse_case): one impulse per line along the transformed axis, the expected
    array laid out the same way -- for the type-1 kinds too, whose n is not N / 2."""
    for N in (14, 20, 64):
        for kind in KINDS:
            shape, axis, x, want = cases.r2r_impulse_case(kind, N, mapping)
            n = cases.r2r_points(kind, N)
            assert shape[axis] == n and x.shape == want.shape == shape and x.flags.c_contiguous
            assert np.array_equal(x.sum(axis=axis), np.ones(shape[:axis] + shape[axis + 1:]))
            f, typ = SCIPY[kind]
            assert np.abs(f(x, type=typ, axis=axis, norm=None) - want).max() <= 4 * EPS64 * np.log2(2 * n) * 2, (kind, N, mapping)


# ---- the decomposition of plan.cpp (comment block above get_r2r_tables), in numpy ----------------------------------------
def emu_tables(kind, n, wrong=None):
    """(pre, post, pos0, idx0, N) in long double.  `wrong` = (post?, index, delta): delta added to the real part of that one
    entry before rounding, as the library's test hook does."""
    ld = np.longdouble
    pi = ld(4) * np.arctan(ld(1))
    th = pi / (2 * ld(n))
    j = np.arange(n).astype(ld)
    cis = lambda a: np.cos(a) - 1j * np.sin(a)                # e^{-ia}, complex long double
    one = np.ones(n, dtype=np.clongdouble)
    pre, post, pos0, idx0, N = one, one, 0, 0, 2 * n
    if kind == cases.REDFT00:
        N, pre = 2 * (n - 1), one * np.where((j == 0) | (j == n - 1), 1, 2)
    elif kind == cases.REDFT10:
        post = 2 * cis(j * th)
    elif kind == cases.REDFT01:
        pre = np.where(j == 0, 1, 2) * cis(j * th)
    elif kind == cases.REDFT11:
        pre, post = cis(j * th), 2 * cis((2 * j + 1) * th / 2)
    elif kind == cases.RODFT00:
        N, pos0, idx0, post = 2 * (n + 1), 1, 1, 2j * one
    elif kind == cases.RODFT10:
        idx0, post = 1, 2j * cis((j + 1) * th)
    elif kind == cases.RODFT01:
        pos0, pre = 1, 1j * np.where(j == n - 1, 1, 2) * cis((j + 1) * th)
    else:
        pre, post = cis(j * th), 2j * cis((2 * j + 1) * th / 2)
    pre, post = np.array(pre, dtype=np.clongdouble), np.array(post, dtype=np.clongdouble)
    if wrong is not None:
        (post if wrong[0] else pre)[wrong[1] % n] += ld(wrong[2])
    return pre, post, pos0, idx0, N


def emulate(kind, x, dt, wrong=None):
    """The r2r transform of the lines x[b, :] (float64 in, float64 out) the way the library computes it, in precision `dt`."""
    cdt, rdt = ('D', 'd') if dt == 'd' else ('F', 'f')
    n = x.shape[-1]
    pre, post, pos0, idx0, N = emu_tables(kind, n, wrong)
    pre, post = pre.astype(cdt), post.astype(cdt)
    z = np.zeros(x.shape[:-1] + (N,), dtype=cdt)
    z[..., pos0:pos0 + n] = pre * x.astype(rdt)
    Z = scipy.fft.fft(z, axis=-1)
    assert Z.dtype == np.dtype(cdt)                           # (scipy.fft keeps single precision)
    y = (post * Z[..., idx0:idx0 + n]).real
    assert y.dtype == np.dtype(rdt)
    return y.astype('d')


def emu_impulse_error(kind, N, dt, wrong=None):
    n = cases.r2r_points(kind, N)
    pos = cases.r2r_positions(n)
    x = np.zeros((len(pos), n))
    x[np.arange(len(pos)), pos] = 1
    want = np.stack([cases.r2r_exact_impulse(kind, n, j) for j in pos])
    return float(np.abs(emulate(kind, x, dt, wrong) - want).max())


EMU_LENGTHS = [16, 64, 128, 240, 500, 1042, 4096, 8192]


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_emulated_decomposition_stays_under_half_the_gpu_allowance(dt):
    """Measured here: 0.63 (fp32), 0.75 (fp64), both at N = 1042, in units of 2 eps log2 N; the GPU allowance is 2.0 of
    the same unit."""
    worst = (0.0, None, None)
    for N in EMU_LENGTHS:
        for kind in KINDS:
            r = emu_impulse_error(kind, N, dt) / (2 * cases.EPS[dt] * np.log2(N))
            worst = max(worst, (r, cases.R2R_NAMES[kind], N))
    print('emulated impulse family, %s: worst %.2f x 2 eps log2 N (%s, N = %d)' % ((dt,) + worst))
    assert 0 < worst[0] <= 1.0, worst


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_emulated_decomposition_on_random_data(dt):
    """Random lines against scipy in float64, in units of eps log2 N relative to max |want| (cases.assert_close allows 2):
    measured here 0.30 (fp32), 0.48 (fp64)."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for N in EMU_LENGTHS:
        for kind in KINDS:
            n = cases.r2r_points(kind, N)
            x = rng.standard_normal((4, n)).astype(dt).astype('d')
            f, typ = SCIPY[kind]
            want = f(x, type=typ, axis=-1, norm=None)
            err = float(np.abs(emulate(kind, x, dt) - want).max() / np.abs(want).max())
            worst = max(worst, err / (cases.EPS[dt] * np.log2(N)))
    print('emulated random data, %s: worst %.2f eps log2 N' % (dt, worst))
    assert 0 < worst <= 1.0, worst


@pytest.mark.parametrize('post', [0, 1], ids=['pre', 'post'])
@pytest.mark.parametrize('dt,exponent', [('d', 9), ('d', 11), ('f', 5)])
def test_one_wrong_entry_shows_at_full_size_in_the_emulation(dt, exponent, post):
    """Entry 1 of either table off by delta: the position list shows it at >= 0.98 delta (asserted at the 0.9 the GPU tests
    use, on top of the emulation's own rounding) for every kind and every length from 16 to 4096."""
    delta = 10.0 ** -exponent
    least = 1e30
    for N in (16, 20, 64, 128, 240, 500, 4096):
        for kind in KINDS:
            err = emu_impulse_error(kind, N, dt, wrong=(post, 1, delta))
            least = min(least, err / delta)
            assert err >= 0.9 * delta and err > 2.0 * 2 * cases.EPS[dt] * np.log2(N), (cases.R2R_NAMES[kind], N, dt, post, err / delta)
    print('one wrong %s entry, %s 1e-%d: shown at >= %.3f delta' % ('post' if post else 'pre', dt, exponent, least))
