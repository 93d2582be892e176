"""Proof, on the host, that the comparator of tests/test_gpu_real_backward.py bites: what a c2r returns that does NOT drop
the imaginary parts of X[0] and X[n/2] is computed in float64 from the two ways a kernel can leak them, and
`cases.assert_close` -- the 2 eps log2(points) guard -- must reject each by a factor of 100 at every rows length and in both
precisions, while it accepts the float64 reference rounded to the test's precision."""
import numpy as np
import pytest

from tests import cases

LINES = 5


def _spectrum(n, dt):
    return cases.dirty_spectrum((LINES, n // 2 + 1), dt, 100 + n).astype('D')


def _reference(X, n):
    return np.fft.irfft(X, n=n, axis=1) * n


def _packed(X, n, leak):
    """c2r of even length n as the packed rows run it: one complex transform of length m = n / 2 on
    Z[k] = (X[k] + conj X[m - k]) + i w^-k (X[k] - conj X[m - k]), x[2j] + i x[2j + 1] = z[j].  `leak`: entry 0 formed
    from X[0] and X[m] as they are, imaginary parts included."""
    m = n // 2
    k = np.arange(m)
    Xe = X if leak else cases.clean_edges(X, n, 1)
    a, b = Xe[:, :m], np.conj(Xe[:, m - k])
    Z = (a + b) + 1j * np.exp(2j * np.pi * k / n) * (a - b)
    z = np.fft.ifft(Z, axis=1) * m
    x = np.empty((X.shape[0], n))
    x[:, 0::2], x[:, 1::2] = z.real, z.imag
    return x


def _full(X, n, leak):
    """c2r as the full-length lines run it: the inverse complex DFT of the mirrored line; the imaginary output cancels
    only if nothing stores it.  `leak`: a .y stored for an .x -- the imaginary output added to the real one."""
    line = np.empty((X.shape[0], n), dtype='D')
    h = n // 2 + 1
    line[:, :h] = X
    line[:, h:] = np.conj(X[:, 1:n - h + 1][:, ::-1])
    y = np.fft.ifft(line, axis=1) * n
    return y.real + y.imag if leak else y.real


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('n,path', cases.REAL_ROWS)
def test_the_guard_rejects_a_c2r_that_keeps_the_ignored_imaginary_parts(n, path, dt):
    X = _spectrum(n, dt)
    assert np.abs(X[:, 0].imag).min() > 0 and (n % 2 or np.abs(X[:, -1].imag).min() > 0)
    ref = _reference(X, n)
    nelem = LINES * n
    guard = cases.rounding_tol(dt, nelem)
    cases.assert_close(ref.astype(dt), ref, dt, nelem, (n, 'the reference, rounded'))
    models = [('full', _full)] + ([('packed', _packed)] if n % 2 == 0 else [])
    for name, model in models:
        # the model without the leak IS the reference (float64 rounding apart) ...
        assert np.abs(model(X, n, False) - ref).max() <= 1e-12 * np.abs(ref).max(), (name, n)
        # ... and with it the guard fails by a clear margin
        bad = model(X, n, True)
        err = float(np.abs(bad - ref).max() / np.abs(ref).max())
        assert err >= 100 * guard, (name, n, dt, err, guard, err / guard)
        with pytest.raises(AssertionError):
            cases.assert_close(bad.astype(dt), ref, dt, nelem, (name, n))
