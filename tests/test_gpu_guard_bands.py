"""Guard bands round the transforms: no line kernel writes past its output or depends on a byte past its input.

The suite compares values; nothing else in it looks at the memory OUTSIDE the arrays a call was given.  A ragged last tile
without its `row < batch` guard, a type-1 DCT / DST line (pitch n != N / 2) one entry too long, a half spectrum of n // 2 + 1
entries stored as n // 2 + 2 write into whatever the allocator placed behind the output -- some other tensor of a run --, and a
tail tile that loads lines past the batch and USES them reads what the allocator left there, usually finite.  GPU address
sanitizers are not available to this suite, so every case here runs inside guarded arenas (tests/arena.py) in the four ways of
tests/guards.py: guards intact, input preserved, rounding-level parity with the float64 oracle, and bit identity with the
unguarded run, with the run whose input guards hold NaN, and -- complex and real-to-real plans -- with the in-place run.

Batches are never a multiple of a kernel tile: 'rows' (19, n), 'cols' (n, 19), 'middle' (3, n, 7), and one batch of a single
line, (1, n) and (n, 1).  The three families of this file also run with payloads that start ONE ELEMENT past a 256-byte
boundary -- input only, output only, both --: include/gfft.h asks of a base no more than the alignment of one element, and
such a run must give the bits of the aligned one.  A subset runs a second time under option grid_cap = 1, where one
workgroup walks every tile and the last tile is another piece of code.  The other families: tests/test_gpu_guard_trunc.py
(3/2-rule paths, pack / unpack, scale), tests/test_gpu_guard_layouts.py (exchange-buffer layouts, 3-D schedules, on-chip
planes); tests/test_gpu_guard_selftest.py shows that the guards bite.

What this does NOT cover:
  * the scratch regions of multi-pass plans (four-step, Bluestein, embedded real lines, 3-D workspaces) come from the
    library's own pool and cannot be guarded from outside;
  * a load past the input whose value is discarded is not detectable without a sanitizer -- only a dependence on it is."""
import pytest

pytestmark = pytest.mark.gpu

from tests import cases
from tests.guards import MAPPINGS, serial_case


@pytest.fixture
def one_workgroup():
    """grid_cap = 1 for the plans made inside the test; the default comes back afterwards, also after a failure."""
    from mpi4py_fft_amd import _lib
    _lib.set_option('grid_cap', 1)
    yield
    _lib.set_option('grid_cap', 0)


# ---- complex lines: one length per kernel family of tests/test_gpu_rounding_guard.py LENGTHS --------------------------------
def _regs(text):
    for t in text:
        passes = [ln for ln in t.splitlines() if 'kernel=' in ln]
        assert len(passes) == 1 and 'kernel=regs-' in passes[0], t


def _generic(text):
    assert all('kernel=generic' in t for t in text), text


def _fourstep(text):
    assert all('[four-step 1/2' in t for t in text), text


def _bluestein(text):
    assert all('multiply by B' in t and 'embed' in t and 'extract' in t for t in text), text


COMPLEX = {'pow2': ([16, 256, 2048, 4096], _regs), '3.2^k': ([48, 768], _regs), '5.2^k': ([80, 1000], _regs),
           'unequal-width': ([240, 896], _regs), 'generic': ([22, 121, 1331], _generic), 'four-step': ([8192, 9216], _fourstep),
           'bluestein': ([521], _bluestein)}


@pytest.mark.parametrize('dt', ['D', 'F'])
@pytest.mark.parametrize('family', list(COMPLEX))
def test_complex_lines(family, dt):
    lengths, path = COMPLEX[family]
    for n in lengths:
        for mapping, batch in MAPPINGS.items():
            shape, axis = batch(n)
            # the path from gfft_plan_describe, so that a planner change cannot move a length to another kernel unnoticed
            serial_case(shape, (axis,), dt, ('complex', family, n, mapping, dt), path=path, in_place=True)


# ---- real lines: one length per path of cases.REAL_LENGTHS; the half spectrum has n // 2 + 1 entries per line ----------------
REAL = {'packed': [64, 96, 1000], 'regs': [48], 'generic': [15, 121, 22], 'embedded': [9216], 'bluestein': [521]}
# along a strided axis there is no packed form (tests/test_gpu_rounding_guard.py REAL_STRIDED_PATHS)
REAL_STRIDED = {64: 'regs', 96: 'regs', 1000: 'regs', 48: 'regs', 15: 'generic', 121: 'generic', 22: 'generic', 9216: 'embedded',
                521: 'bluestein'}


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('family', list(REAL))
def test_real_lines(family, dt):
    for n in REAL[family]:
        assert n in cases.REAL_LENGTHS[family], n
        for mapping, batch in MAPPINGS.items():
            shape, axis = batch(n)
            expected = {'rows': family, 'cols': REAL_STRIDED[n]}.get(mapping)

            def path(text, expected=expected, n=n, mapping=mapping):
                assert cases.real_path(text) == expected, (n, mapping, expected, text)
            serial_case(shape, (axis,), dt, ('real', family, n, mapping, dt), path=path if expected else None)


# ---- real-to-real kinds: the type-1 kinds have n = N / 2 +- 1 points per line -------------------------------------------------
R2R_N = {64: 'adapter', 768: 'adapter', 32: 'fallback', 240: 'fallback', 1042: 'bluestein'}


@pytest.mark.parametrize('dt', ['d', 'f'])
@pytest.mark.parametrize('kind', sorted(cases.R2R_NAMES), ids=lambda k: cases.R2R_NAMES[k])
def test_r2r_kinds(kind, dt):
    for N, expected in R2R_N.items():
        assert N in cases.R2R_LENGTHS[expected]
        n = cases.r2r_points(kind, N)
        for mapping, batch in MAPPINGS.items():
            shape, axis = batch(n)
            as_mapping = {'one row': 'rows', 'one col': 'cols'}.get(mapping, mapping)

            def path(text, N=N, m=as_mapping, expected=expected):
                assert cases.r2r_path(text[:1], N, m) == expected and cases.r2r_path(text[1:], N, m) == expected, (N, m, text)
            serial_case(shape, (axis,), dt, ('r2r', cases.R2R_NAMES[kind], N, mapping, dt), r2r=kind, in_place=True,
                        path=path if mapping in cases.R2R_MAPPINGS else None)


# ---- one workgroup walks every tile: the last tile of a walk is not the last tile of a one-tile workgroup --------------------
CAPPED = [('pow2', 256), ('3.2^k', 48), ('5.2^k', 80), ('unequal-width', 240), ('generic', 121)]


@pytest.mark.parametrize('dt', ['D', 'F'])
@pytest.mark.parametrize('family,n', CAPPED)
def test_complex_lines_on_one_workgroup(family, n, dt, one_workgroup):
    for mapping in cases.R2R_MAPPINGS:
        shape, axis = MAPPINGS[mapping](n)
        serial_case(shape, (axis,), dt, ('complex, grid_cap 1', family, n, mapping, dt), path=COMPLEX[family][1],
                    in_place=True, offsets=(), capped=True)


@pytest.mark.parametrize('dt', ['d', 'f'])
def test_real_and_r2r_lines_on_one_workgroup(dt, one_workgroup):
    for mapping in cases.R2R_MAPPINGS:
        shape, axis = MAPPINGS[mapping](64)
        serial_case(shape, (axis,), dt, ('real, grid_cap 1', 64, mapping, dt), offsets=(), capped=True)
        for kind in (cases.REDFT00, cases.RODFT00, cases.REDFT10):
            shape, axis = MAPPINGS[mapping](cases.r2r_points(kind, 64))
            serial_case(shape, (axis,), dt, ('r2r, grid_cap 1', cases.R2R_NAMES[kind], 64, mapping, dt), r2r=kind, in_place=True, offsets=(),
                        capped=True)
