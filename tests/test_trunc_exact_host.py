"""The test of the 3/2-rule impulse tests (host only, no GPU, no library).

`tests/cases.py trunc_exact_forward` / `trunc_exact_backward` are the analytic answers the GPU guard of
tests/test_gpu_trunc_guard.py compares against; a wrong formula there would make it rest on nothing, and a family whose
impulse positions and bins cannot see a mistake would guard nothing.  So:

  * the closed forms are held against the float64 oracle (`oracle.pfft_oracle.OFFT(..., padding=...)`, numpy's transform
    around a restatement of the model's truncation and padding): even and odd kept lengths, a real axis with m even from an
    odd and from a 2-mod-4 real length and with m odd, padding 1.5, 2.0 and ratios that are no integer multiple of a half,
    every impulse position and every stored bin -- both sides carry float64 rounding only, hence a few ulp of the peak;
  * a numpy MODEL of the adapters the way the kernels write them (lower band, upper band shifted by n - N, the fold of entry
    n - h onto h, the halving on the way back, the c2r mirror), with one mistake switched on at a time, is run on the GPU
    family's own inputs for every (n, kept) of the family: each mistake must move at least one line by 0.4 -- against an
    allowance below 1e-5 of the peak --, or be named by `blind` for that case with the reason it cannot differ there, and
    then AGREE with the exact answer (nothing is skipped).
"""
import numpy as np
import pytest

from oracle import pfft_oracle as O
from tests import cases

EPS64 = 2.0 ** -52

# (n, kept): the pairs the formulas were derived on, and the parities of the real rule: 31 -> m = 16 (m even, real length
# odd), 30 -> 16 (m even, real length 2 mod 4), 32 -> 17 (m odd)
ORACLE_PAIRS = [(48, 32), (64, 32), (48, 31), (80, 63), (96, 64), (45, 30), (240, 161), (46, 31), (94, 63), (12, 8), (13, 9), (27, 18)]


@pytest.mark.parametrize('real', [False, True], ids=['complex', 'real'])
@pytest.mark.parametrize('n,kept', ORACLE_PAIRS)
def test_closed_forms_against_the_oracle(n, kept, real):
    dt = 'd' if real else 'D'
    keep, full = cases.trunc_entries(n, kept, real)
    ref = O.OFFT((n,), 0, dt, padding=n / kept)
    assert ref.out_shape == (keep,) and keep < full
    tol = 4 * EPS64 * np.log2(n) * 2
    worst = 0.0
    for j in sorted(set(cases.r2r_positions(n)) | {0, n // 2}):
        x = np.zeros(n, dtype=dt)
        x[j] = 1
        err = float(np.abs(ref.forward(x, normalize=False) - cases.trunc_exact_forward(n, keep, j, real)).max())
        worst = max(worst, err)
        assert err <= tol, (n, kept, real, 'forward', j, err)
    for kb in range(keep):                                       # every stored bin, three amplitudes
        for a in (1.0, 1j, 0.6 - 0.8j):
            s = np.zeros(keep, dtype='D')
            s[kb] = a
            err = float(np.abs(ref.backward(s) - cases.trunc_exact_backward(n, keep, kb, a, real)).max())
            worst = max(worst, err)
            assert err <= tol, (n, kept, real, 'backward', kb, a, err)
    print('closed forms vs oracle, n = %d kept = %d %s: worst %.2e' % (n, kept, 'real' if real else 'complex', worst))


def test_the_real_rule_takes_its_parity_from_the_stored_half_length():
    """31 real points kept of 48: m = 16 is even, so entry 15 -- no Nyquist entry of a 31-point line -- is doubled and made
    real on the way out and halved on the way back; 32 kept: m = 17, nothing of the kind."""
    T = cases.trunc_exact_forward(48, 16, 5, True)
    assert T.dtype == np.complex128 and T[15].imag == 0.0 and abs(T[15].real - 2 * np.cos(2 * np.pi * 75 / 48)) < 1e-15
    assert abs(abs(cases.trunc_exact_forward(48, 17, 5, True)[15]) - 1) < 1e-15
    assert np.array_equal(cases.trunc_exact_backward(48, 16, 15, 1j, True), np.zeros(48))
    assert np.abs(cases.trunc_exact_backward(48, 17, 15, 1j, True)).max() > 1.9
    # nothing cut: the plain transforms (what the probe sets beside the padded plans)
    for n in (12, 13):
        for real in (False, True):
            keep = cases.trunc_entries(n, n, real)[0]
            x = np.zeros(n)
            x[5] = 1
            want = (np.fft.rfft if real else np.fft.fft)(x)
            assert np.abs(cases.trunc_exact_forward(n, keep, 5, real) - want).max() < 1e-14
            for kb in range(keep):
                s = np.zeros(keep, dtype='D')
                s[kb] = 0.6 - 0.8j
                want = np.fft.irfft(s, n) * n if real else np.fft.ifft(s) * n
                assert np.abs(cases.trunc_exact_backward(n, keep, kb, 0.6 - 0.8j, real) - want).max() < 1e-13, (n, real, kb)


@pytest.mark.parametrize('mapping', cases.TRUNC_MAPPINGS)
def test_impulse_batches_are_what_the_oracle_transforms_along_the_axis(mapping):
    for n, kept in ((18, 12), (48, 31), (64, 43)):
        for dt in 'Dd':
            shape, axis, x, wf, spec, wb, pf, pb = cases.trunc_impulse_case(n, kept, dt, mapping)
            keep = cases.trunc_entries(n, kept, dt == 'd')[0]
            assert shape[axis] == n and wf.shape[axis] == keep and x.flags.c_contiguous and wf.flags.c_contiguous
            assert np.array_equal(x.sum(axis=axis), np.ones(shape[:axis] + shape[axis + 1:]))
            assert np.array_equal((spec != 0).sum(axis=axis), np.ones(shape[:axis] + shape[axis + 1:]))
            ref = O.OFFT(shape, axis, dt, padding=n / kept)
            assert np.abs(ref.forward(x.astype(dt), normalize=False) - wf).max() <= 1e-13
            assert np.abs(ref.backward(spec) - wb).max() <= 1e-13
            assert pb == (2.0 if dt == 'd' else 1.0) and pf == (2.0 if keep % 2 == 0 else 1.0)


# ---- the adapters as the kernels write them (fft_pow2_impl.h tile_store_trunc / tile_load_pad, pack.hip trunc_kernel), in
# numpy, with one mistake at a time ----------------------------------------------------------------------------------
MISTAKES = ('fold dropped (forward)', 'halving dropped (backward)', 'parity from the padded length', 'parity from the real length',
            'upper band shifted by one', 'lower band cut at h - 1', 'mirrored imaginary sign flipped (c2r)', 'Nyquist imaginary part kept')


def model_forward(x, n, kept, real, wrong=None):
    """x (lines, n) -> (lines, keep): numpy's transform, then the truncating store with `wrong` switched on."""
    keep, _ = cases.trunc_entries(n, kept, real)
    even = keep % 2 == 0
    if wrong == 'parity from the padded length':
        even = n % 2 == 0
    if wrong == 'parity from the real length' and real:
        even = kept % 2 == 0
    P = np.fft.rfft(x, axis=-1) if real else np.fft.fft(x, axis=-1)
    T = np.zeros(x.shape[:-1] + (keep,), dtype='D')               # (an entry no thread stores: zero here, NaN on the GPU)
    if real:
        top = keep - 1 if wrong == 'lower band cut at h - 1' else keep
        T[:, :top] = P[:, :top]
        if even and top == keep:
            T[:, keep - 1] = P[:, keep - 1] if wrong == 'fold dropped (forward)' else 2 * P[:, keep - 1]
            if wrong != 'Nyquist imaginary part kept':
                T[:, keep - 1] = T[:, keep - 1].real
        return T
    h = keep // 2
    lo = h if wrong == 'lower band cut at h - 1' else h + 1       # entries 0 ... lo - 1 of the lower band
    T[:, :lo] = P[:, :lo]
    if even and lo == h + 1 and wrong != 'fold dropped (forward)':
        T[:, h] += P[:, n - h]
    sh = 1 if wrong == 'upper band shifted by one' else 0
    for e in range(n - h + (1 if even else 0), n):                # entry n - h of an even keep is the fold's, not stored here
        T[:, e - (n - keep)] = P[:, (e + sh) % n]
    return T


def model_backward(S, n, kept, real, wrong=None):
    """S (lines, keep) -> (lines, n): the zero-padding load with `wrong` switched on, then the transform by its definition
    (for a real line: the Hermitian mirror written out, as a c2r kernel builds it, and the real part)."""
    keep, _ = cases.trunc_entries(n, kept, real)
    even = keep % 2 == 0
    if wrong == 'parity from the padded length':
        even = n % 2 == 0
    if wrong == 'parity from the real length' and real:
        even = kept % 2 == 0
    half = 1.0 if wrong == 'halving dropped (backward)' else 0.5
    if real:
        H = np.zeros(S.shape[:-1] + (n // 2 + 1,), dtype='D')
        top = keep - 1 if wrong == 'lower band cut at h - 1' else keep
        H[:, :top] = S[:, :top]
        if even and top == keep:
            H[:, keep - 1] = half * (S[:, keep - 1] if wrong == 'Nyquist imaginary part kept' else S[:, keep - 1].real)
        X = np.zeros(S.shape[:-1] + (n,), dtype='D')
        X[:, :n // 2 + 1] = H
        X[:, 0] = H[:, 0].real
        mirror = H[:, 1:(n + 1) // 2]
        X[:, n - 1:n // 2:-1] = mirror if wrong == 'mirrored imaginary sign flipped (c2r)' else mirror.conj()
        if n % 2 == 0:
            X[:, n // 2] = H[:, n // 2].real
        return (np.fft.ifft(X, axis=-1) * n).real
    h = keep // 2
    V = np.zeros(S.shape[:-1] + (n,), dtype='D')
    lo = h if wrong == 'lower band cut at h - 1' else h + 1
    V[:, :lo] = S[:, :lo]
    sh = 1 if wrong == 'upper band shifted by one' else 0
    for e in range(n - h, n):
        V[:, e] = S[:, (e - (n - keep) + sh) % keep]
    if even:
        V[:, h] *= half
        V[:, n - h] *= half
    return np.fft.ifft(V, axis=-1) * n


def blind(mistake, n, kept, real):
    """Why `mistake` CANNOT change the answer at (n, kept, real), or None.  Everything listed here is a property of the rule
    itself at that case, not of the inputs: the model with the mistake is then required to AGREE with the exact answer."""
    keep, _ = cases.trunc_entries(n, kept, real)
    even = keep % 2 == 0
    if mistake in ('fold dropped (forward)', 'halving dropped (backward)', 'Nyquist imaginary part kept') and not even:
        return 'odd stored length: no fold, no halving, no Nyquist-like entry'
    if mistake == 'Nyquist imaginary part kept' and not real:
        return 'complex axis: the folded entry keeps its imaginary part by the rule'
    if mistake == 'parity from the padded length' and (n % 2 == 0) == even:
        return 'padded and stored lengths have the same parity'
    if mistake == 'parity from the real length' and (not real or (kept % 2 == 0) == even):
        return 'complex axis' if not real else 'real and stored lengths have the same parity'
    if mistake == 'upper band shifted by one' and real:
        return 'real axis: one band only'
    if mistake == 'mirrored imaginary sign flipped (c2r)' and not real:
        return 'complex axis: no mirror'
    return None


ALL_CASES = [(n, kept, real) for n, kept, _ in cases.TRUNC_CASES for real in (False, True)]


@pytest.mark.parametrize('n,kept,real', ALL_CASES, ids=['%d-%d-%s' % (n, k, 'real' if r else 'complex') for n, k, r in ALL_CASES])
def test_the_family_sees_every_wrong_adapter(n, kept, real):
    """21 lines (the 'middle' mapping's count; 'rows' and 'cols' hold the first 19, which contain every position and every
    bin the 21 do except repeats)."""
    for lines in (19, 21):
        x, wf, spec, wb, pf, pb = cases.trunc_impulse_lines(n, kept, real, lines)
        tol = 64 * EPS64 * np.log2(n) * 2                         # numpy's transform on both sides of the model
        assert np.abs(model_forward(x, n, kept, real) - wf).max() <= tol, (n, kept, real, 'the model itself, forward')
        assert np.abs(model_backward(spec, n, kept, real) - wb).max() <= tol, (n, kept, real, 'the model itself, backward')
        for mistake in MISTAKES:
            df = float(np.abs(model_forward(x, n, kept, real, mistake) - wf).max())
            db = float(np.abs(model_backward(spec, n, kept, real, mistake) - wb).max())
            why = blind(mistake, n, kept, real)
            if why is None:
                assert max(df, db) >= 0.4, (n, kept, real, lines, mistake, df, db)
            else:
                assert max(df, db) <= tol, (n, kept, real, lines, mistake, why, df, db)


def test_no_mistake_is_blind_everywhere_and_every_case_sees_most():
    for mistake in MISTAKES:
        seen = [(n, kept, real) for n, kept, real in ALL_CASES if blind(mistake, n, kept, real) is None]
        assert len(seen) >= 4, (mistake, seen)
        print('%-40s seen at %2d of %d cases' % (mistake, len(seen), len(ALL_CASES)))
    for n, kept, real in ALL_CASES:
        assert sum(blind(m, n, kept, real) is None for m in MISTAKES) >= 2, (n, kept, real)
