"""Rounding-level and impulse guards of the real-to-real kinds (DCT / DST I-IV) -- the third family beside the complex and the
real (r2c / c2r) ones of tests/test_gpu_rounding_guard.py.

Every kind is y[k] = Re(post[k] DFT_N(pre x)[idx0 + k]) (plan.cpp plan_r2r_line): two device tables no complex or real
plan reads (get_r2r_tables), index shifts, a zero-fill outside [pos0, pos0 + n) and a bounded store, in two
implementations -- the MODE_R2R load / store adapters of the register kernels, and the embed / extract kernels around a
complex plan.  On random data one wrong table entry is diluted below fp32 rounding; the transform of a unit impulse is the
bare product pre[j] w^((pos0 + j)(idx0 + k)) post[k], so it shows at full size (`tests/cases.py r2r_impulse_errors`, exact
answers `r2r_exact_impulse`, held against scipy by tests/test_r2r_exact_host.py).

The proof that the guard bites: one entry of either table off by 1e-9 / 1e-11 (fp64), 1e-5 (fp32), injected through the
library's test hook (`gfft_set_option "debug_r2r_exp"`, plan.cpp get_r2r_tables), fails it on both paths for every kind,
while the fp32 random-data tolerance tests/test_gpu_r2r.py had alone (5e-5) lets it through.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pfft_oracle as O
from tests import cases

KINDS = sorted(cases.R2R_NAMES)
# In units of 2 eps log2 N (2: the exact answer's peak).  The project's IMPULSE_FACTOR for the inner complex transform these
# kinds run on, itself measured at <= 1.2 (fp64); the decomposition alone, emulated in numpy with none of the code under test
# (tests/test_r2r_exact_host.py), stays at 0.63 (fp32) / 0.75 (fp64).
# Measured (tools/r2r_impulse_probe.py, profiles/r2r_impulse_probe.txt), worst ratio per path over the three mappings:
# adapter 0.33 (fp64) / 0.34 (fp32), N = 64; fallback 0.42 / 0.33, N = 8192; Bluestein 0.35 / 0.35, N = 1042.
R2R_IMPULSE_FACTOR = 2.0


def allowance(dt, N):
    return R2R_IMPULSE_FACTOR * 2 * cases.EPS[dt] * np.log2(N)


@pytest.mark.parametrize('mapping', cases.R2R_MAPPINGS)
@pytest.mark.parametrize('dt', ['d', 'f'])
def test_r2r_impulse_responses_at_rounding_level(dt, mapping):
    """All eight kinds (each inverse is another kind of the list) over every path an r2r line can take -- each confirmed from
    gfft_plan_describe, so that a planner change cannot quietly move a length --, every line of a batch that is no multiple
    of any kernel tile checked against its exact answer."""
    worst = 0.0
    for path, lengths in cases.R2R_LENGTHS.items():
        for N in lengths:
            for kind in KINDS:
                text = []
                err = cases.r2r_impulse_errors(kind, N, dt, mapping, describe=text)
                assert cases.r2r_path(text, N, mapping) == path, (cases.R2R_NAMES[kind], N, dt, mapping, path, text)
                unit = 2 * cases.EPS[dt] * np.log2(N)
                cases._note('r2rimp', dt, N, err / 2)
                print('r2rimp %s %-6s N=%-5d %-9s %s  %.2e (%.2f x 2 eps log2 N)' % (dt, mapping, N, path, cases.R2R_NAMES[kind], err, err / unit))
                worst = max(worst, err / unit)
                assert err <= allowance(dt, N), (cases.R2R_NAMES[kind], N, dt, mapping, path, err, err / unit)
    assert worst > 0          # (the transforms did run)


@pytest.fixture
def wrong_r2r_entry():
    from mpi4py_fft_amd import _lib

    def arm(post, exponent, index=1):
        _lib.set_option('debug_r2r_post', post)
        _lib.set_option('debug_r2r_index', index)
        _lib.set_option('debug_r2r_exp', exponent)
    yield arm
    _lib.set_option('debug_r2r_exp', 0)
    _lib.set_option('debug_r2r_index', 1)
    _lib.set_option('debug_r2r_post', 0)


def random_data_error(kind, N, dt):
    """max |got - want| / max |want| of 19 random rows against scipy in float64: what test_all_kinds_against_scipy compares."""
    from mpi4py_fft_amd import fftw, asdevice
    n = cases.r2r_points(kind, N)
    A = O.rng_array((19, n), dt, 3)
    plan = fftw.get_planned_FFT(asdevice(A), asdevice(np.zeros_like(A)), (1,), [kind])
    got = np.asarray(plan()).astype('d')
    plan.destroy()
    want = O.r2r_1d(A.astype('d'), 1, kind)
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize('post', [0, 1], ids=['pre', 'post'])
@pytest.mark.parametrize('dt,exponent', [('d', 9), ('d', 11), ('f', 5)])
@pytest.mark.parametrize('N,path', [(128, 'adapter'), (240, 'fallback')])
def test_one_wrong_table_entry_fails_the_impulse_guard(N, path, dt, exponent, post, wrong_r2r_entry):
    """Plans made while the hook is armed read a pre (or post) table whose entry 1 is off by 10^-exponent in its real part.
    The impulse family must name it at full size -- 0.9 delta: the emulation of tests/test_r2r_exact_host.py shows it at
    >= 0.98 delta -- for every kind, in the rows and the strided mapping; plans made after disarming pass again.  In fp32 the
    random-data comparison at 5e-5 passes the broken table: it cannot be the only check."""
    delta = 10.0 ** -exponent
    wrong_r2r_entry(post, exponent)
    for kind in KINDS:
        for mapping in ('rows', 'cols'):
            text = []
            err = cases.r2r_impulse_errors(kind, N, dt, mapping, describe=text)
            assert cases.r2r_path(text, N, mapping) == path, text
            assert err > allowance(dt, N) and err >= 0.9 * delta, (cases.R2R_NAMES[kind], N, dt, mapping, post, err, err / delta)
        if dt == 'f':
            rel = random_data_error(kind, N, dt)
            assert rel <= 5e-5, (cases.R2R_NAMES[kind], N, rel)          # the old tolerance lets the broken table through
    wrong_r2r_entry(post, 0)
    for kind in KINDS:
        for mapping in ('rows', 'cols'):
            err = cases.r2r_impulse_errors(kind, N, dt, mapping)          # plans made now read the exact tables
            assert err <= allowance(dt, N), (cases.R2R_NAMES[kind], N, dt, mapping, err)
