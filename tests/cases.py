"""Shared test bodies: the same PFFT / Transfer checks run against the HIP engine on a GPU
(-m gpu) and against the host checker engine on CPU (host-logic tests)."""
import json
import os

import numpy as np

from oracle import pfft_oracle as O
from tests import thread_comm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)


def pfft_case_names():
    p = load('pfft')
    return sorted({k.split('/')[0] for k in p.files})


EPS = {'f': 2.0 ** -23, 'F': 2.0 ** -23, 'd': 2.0 ** -52, 'D': 2.0 ** -52}
CONTRACT = {'fwd': {'f': 2e-4, 'F': 2e-4, 'd': 2e-10, 'D': 2e-10}, 'rt': {'f': 1e-4, 'F': 1e-4, 'd': 1e-10, 'D': 1e-10}}


def rounding_tol(dt, nelem, factor=2.0):
    """What a transform of `nelem` points may lose to ROUNDING: factor * eps * log2(nelem) -- 1.3e-14 in fp64, 7e-6 in fp32 at
    1024^3.  Measured over the whole GPU suite (GFFT_TEST_RATIO_LOG, 19 371 guarded comparisons, profiles/r06_guard_ratios.txt):
    the worst case sits at 0.71 eps log2(nelem) -- 7-point lines --, the BASELINE sizes at 0.1 ... 0.4.  The contract tolerances
    (north_star: 1e-10 round trip / 2e-10 forward in fp64; 1e-4 / 2e-4 in fp32) are 10^3 ... 10^5 times looser: a kernel
    that lost three digits would pass them.  The reference's own serial tests ask for the same level
    (/root/reference/tests/test_libfft.py:17, abstol f = 5e-5, d = 1e-14 on O(1) data).
    Four families are held to it, each with an impulse family of its own beside the random-data comparisons: complex
    (`impulse_errors`), real r2c / c2r (`real_impulse_errors`), real-to-real DCT / DST (`r2r_impulse_errors`; there `nelem`
    counts the LOGICAL points N = 2 (n -+ 1) or 2 n of the complex transform a kind runs on, tests/test_gpu_r2r.py) and the
    3/2-rule truncating store / zero-padding load (`trunc_impulse_errors`; `nelem` is the PADDED length of the line)."""
    return factor * EPS[dt] * max(1.0, float(np.log2(max(2.0, float(nelem)))))


_RATIO_LOG = os.environ.get('GFFT_TEST_RATIO_LOG')


def _note(kind, dt, nelem, err):
    # calibration aid: GFFT_TEST_RATIO_LOG=<file> records every guarded error against its rounding allowance
    if _RATIO_LOG:
        with open(_RATIO_LOG, 'a') as f:
            f.write('%s %s %d %.3e %.3f\n' % (kind, dt, nelem, err, err / rounding_tol(dt, nelem, 1.0)))


def tol_for(dt, nelem=None):
    """forward vs oracle: max|d| <= tol * max|ref|.  Without `nelem` the contract tolerance alone;
    with the number of transformed points the rounding-level guard as well (whichever is tighter)."""
    if nelem is None:
        return CONTRACT['fwd'][dt]
    return min(CONTRACT['fwd'][dt], rounding_tol(dt, nelem))


def assert_close(got, ref, dt, nelem, what=''):
    """max|got - ref| / max|ref| within the contract tolerance AND at rounding level; returns the error."""
    err = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))
    _note('fwd', dt, int(nelem), err)
    assert err <= CONTRACT['fwd'][dt], (what, 'contract', err)
    assert err <= rounding_tol(dt, nelem), (what, 'ROUNDING-LEVEL guard: %.3e > %.3e' % (err, rounding_tol(dt, nelem)))
    return err


def assert_roundtrip(back, orig, dt, nelem, what=''):
    """||back - orig||_2 / ||orig||_2 within the contract tolerance AND at rounding level; returns the error."""
    rel = float(np.linalg.norm(back - orig) / max(np.linalg.norm(orig), 1e-30))
    _note('rt', dt, int(nelem), rel)
    assert rel <= CONTRACT['rt'][dt], (what, 'contract', rel)
    assert rel <= rounding_tol(dt, nelem), (what, 'ROUNDING-LEVEL guard: %.3e > %.3e' % (rel, rounding_tol(dt, nelem)))
    return rel


def run_ranks(P, fn):
    from mpi4py_fft_amd import comm
    if P == 1:
        return [fn(comm.COMM_SELF)]
    return thread_comm.run(P, fn)


def check_pfft_golden(name):
    """PFFT of the product package on P (thread-)ranks vs the fixture the reference produced."""
    from mpi4py_fft_amd import PFFT, newDistArray
    p = load('pfft')
    P = int(p[name + '/P'])
    dt = str(p[name + '/dtype'])
    shape = tuple(int(s) for s in p[name + '/shape'])
    kw = json.loads(str(p[name + '/kw']))
    if 'axes' in kw:
        kw['axes'] = [tuple(a) if isinstance(a, list) else a for a in kw['axes']]
    gin = p[name + '/input']

    def body(comm):
        k = {a: (list(b) if isinstance(b, list) else b) for a, b in kw.items()}
        fft = PFFT(comm, shape, dtype=dt, **k)
        u = newDistArray(fft, False)
        u[...] = gin[fft.local_slice(False)]
        uh = fft.forward(u)
        uh_host = np.asarray(uh).copy()
        ub = np.asarray(fft.backward(uh)).copy()
        pin, pout = fft.pencil
        info = dict(axes=[list(a) for a in fft.axes], grid=[c.Get_size() for c in fft.subcomm],
                    in_subshape=list(pin.subshape), in_substart=list(pin.substart), in_axis=pin.axis,
                    out_subshape=list(pout.subshape), out_substart=list(pout.substart),
                    out_axis=pout.axis, gshape_in=list(fft.global_shape(False)),
                    gshape_out=list(fft.global_shape(True)), nxfftn=len(fft.xfftn),
                    ntransfer=len(fft.transfer),
                    transfers=[[t.comm.Get_size(), list(t.shape), list(t.subshapeA), t.axisA,
                                list(t.subshapeB), t.axisB] for t in fft.transfer])
        # structural asserts of tests/test_mpifft.py:144-164
        assert fft.dtype(True) == fft.forward.output_array.dtype
        assert fft.dtype(False) == fft.forward.input_array.dtype
        assert len(fft.axes) == len(fft.xfftn) == len(fft.transfer) + 1
        assert fft.forward.input_pencil.subshape == fft.forward.input_array.shape
        assert fft.forward.output_pencil.subshape == fft.forward.output_array.shape
        assert fft.backward.input_pencil.subshape == fft.backward.input_array.shape
        assert fft.backward.output_pencil.subshape == fft.backward.output_array.shape
        assert fft.dimensions == len(shape)
        fft.destroy()
        return info, uh_host, ub

    res = run_ranks(P, body)
    tol = tol_for(dt)
    nelem = int(np.prod(shape))
    for r, (info, uh, ub) in enumerate(res):
        ref_info = json.loads(str(p['%s/r%d/info' % (name, r)]))
        for key in ref_info:
            assert info[key] == ref_info[key], (name, r, key, info[key], ref_info[key])
        ref = p['%s/r%d/fwd' % (name, r)]
        assert uh.shape == ref.shape and uh.dtype == ref.dtype, (name, uh.shape, ref.shape)
        assert np.abs(uh - ref).max() <= tol * max(np.abs(ref).max(), 1e-30), \
            (name, r, 'forward', np.abs(uh - ref).max())
        assert_close(uh, ref, dt, nelem, (name, r, 'forward'))            # ... and at rounding level
        refb = p['%s/r%d/bwd' % (name, r)]
        assert ub.shape == refb.shape and ub.dtype == refb.dtype
        assert np.abs(ub - refb).max() <= 10 * tol * max(np.abs(refb).max(), 1e-30), \
            (name, r, 'backward', np.abs(ub - refb).max())
        assert np.abs(ub - refb).max() <= 2 * rounding_tol(dt, nelem) * max(np.abs(refb).max(), 1e-30), (name, r, 'backward, rounding level')


def check_transfer_golden(ci):
    """tests/test_pencil.py's chain on the product Transfer vs what the reference's Alltoallw
    delivered (fixture), plus the fwd.fwd.bwd.bwd identity."""
    from mpi4py_fft_amd import Subcomm, Pencil, asdevice, zeros
    t = load('transfer')
    key = 'transfer%d' % ci
    P = int(t[key + '/P'])
    shape = tuple(int(s) for s in t[key + '/shape'])
    a1, a2, a3 = (int(a) for a in t[key + '/axes'])
    pdim = int(t[key + '/pdim'])
    pdim = None if pdim < 0 else pdim
    G = np.arange(int(np.prod(shape)), dtype='d').reshape(shape)

    def body(comm):
        subcomm = Subcomm(comm, pdim)
        p0 = Pencil(subcomm, shape)
        pA = p0.pencil(a1)
        pB = pA.pencil(a2)
        pC = pB.pencil(a3)
        t1 = Pencil.transfer(pA, pB, 'd')
        t2 = Pencil.transfer(pB, pC, 'd')
        sl = tuple(slice(s, s + n) for s, n in zip(pA.substart, pA.subshape))
        A = asdevice(np.ascontiguousarray(G[sl]))
        B = zeros(pB.subshape)
        C = zeros(pC.subshape)
        t1.forward(A, B)
        t2.forward(B, C)
        A2, B2 = zeros(pA.subshape), zeros(pB.subshape)
        t2.backward(C, B2)
        t1.backward(B2, A2)
        geo = np.array([pA.subshape, pA.substart, pB.subshape, pB.substart, pC.subshape, pC.substart])
        return geo, np.asarray(A), np.asarray(B), np.asarray(C), np.asarray(A2)

    for r, (geo, A, B, C, A2) in enumerate(run_ranks(P, body)):
        assert np.array_equal(geo, t['%s/r%d/geo' % (key, r)])
        assert np.array_equal(A, t['%s/r%d/A' % (key, r)])
        assert np.array_equal(B, t['%s/r%d/B' % (key, r)]), (key, r)
        assert np.array_equal(C, t['%s/r%d/C' % (key, r)]), (key, r)
        assert np.array_equal(A2, A)


def check_pfft_vs_oracle(P, shape, dt, seed=7, **kw):
    """Product PFFT on P ranks vs the oracle on the same seeded input: forward values,
    round trip, and the global-DFT identity for unpadded transforms."""
    from mpi4py_fft_amd import PFFT, newDistArray
    offt = O.OPFFT(P, shape, dtype=dt, **{k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()})
    G = O.rng_array(offt.input_shape, dt, seed)
    ref = offt.forward(offt.scatter(G))

    def body(comm):
        k = {a: (list(b) if isinstance(b, list) else b) for a, b in kw.items()}
        if 'r2r' in k:
            # the oracle's {axes: FFTW kind} spelled as the product's `transforms=` dict of planners
            import functools
            from mpi4py_fft_amd import fftw
            tr = {}
            for axes_, kind in k.pop('r2r').items():
                fam, typ = O.R2R_KINDS[kind]
                fwd, bck = (fftw.dctn, fftw.idctn) if fam == 'dct' else (fftw.dstn, fftw.idstn)
                tr[tuple(axes_)] = (functools.partial(fwd, type=typ), functools.partial(bck, type=typ))
            k['transforms'] = tr
        fft = PFFT(comm, shape, dtype=dt, **k)
        u = newDistArray(fft, False)
        u[...] = G[fft.local_slice(False)]
        uh = np.asarray(fft.forward(u)).copy()
        back = np.asarray(fft.backward()).copy()
        sl = fft.local_slice(False)
        fft.destroy()
        return uh, back, sl

    tol = tol_for(dt)
    for r, (uh, back, sl) in enumerate(run_ranks(P, body)):
        assert uh.shape == ref[r].shape and uh.dtype == ref[r].dtype
        scale = max(np.abs(ref[r]).max(), 1e-30)
        assert np.abs(uh - ref[r]).max() <= tol * scale, (shape, dt, kw, np.abs(uh - ref[r]).max() / scale)
        nelem = int(np.prod(offt.input_shape))
        assert_close(uh, ref[r], dt, nelem, (shape, dt, kw))              # ... and at rounding level
        if not kw.get('padding'):
            d = back - G[sl]
            rel = np.linalg.norm(d) / np.linalg.norm(G[sl])
            assert rel <= (1e-10 if dt in 'dD' else 1e-4), (shape, dt, kw, rel)
            assert_roundtrip(back, G[sl], dt, nelem, (shape, dt, kw))


def check_redistribute_chain(rng, mid=False):
    """A random DistArray (shape, tensor rank, dtype, grid, alignment) walked through four random
    redistributions on thread ranks; after each one every rank must hold exactly its local_slice() of
    the global array.  Returns False when the draw is not a valid configuration."""
    from mpi4py_fft_amd import DistArray
    nd = int(rng.choice([2, 3, 3, 4]))
    pool = [5, 8, 9, 12, 13, 16, 17, 24, 31, 32, 33, 40, 64] if not mid else [16, 33, 64, 100, 128, 129, 256, 257, 512, 513]
    P = int(rng.choice([2, 3, 4, 4, 6, 8, 8]))
    shape = tuple(int(rng.choice(pool)) for _ in range(nd))
    if min(shape) < P or np.prod(shape) > (24_000_000 if mid else 2_000_000):
        return False
    rank = int(rng.choice([0, 0, 1, 2])) if not mid else int(rng.choice([0, 0, 1]))
    dt = str(rng.choice(list('fdFD')))
    align = int(rng.integers(0, nd))
    # how many axes are distributed: 1 (slab) ... nd - 1
    ndist = int(rng.integers(1, nd))
    walk = [int(a) for a in rng.integers(0, nd, size=4)]
    comps = (3,) * rank
    G = (rng.standard_normal(comps + shape) + (1j * rng.standard_normal(comps + shape) if dt in 'FD' else 0)).astype(dt)

    def body(comm):
        from mpi4py_fft_amd.pencil import Subcomm
        dims = [0] * nd
        # the aligned axis is undivided; distribute `ndist` of the others
        others = [a for a in range(nd) if a != align]
        for a in others[ndist:]:
            dims[a] = 1
        dims[align] = 1
        sub = Subcomm(comm, dims)
        a = DistArray(comps + shape, subcomm=sub, dtype=dt, alignment=align, rank=rank)
        sl = a.local_slice()
        a[...] = G[sl]
        bad = []
        cur = a
        for ax in walk:
            cur = cur.redistribute(ax)
            got = np.asarray(cur)
            if cur.alignment != ax and cur.commsizes[rank + ax] != 1:
                bad.append(('alignment', ax, cur.alignment))
            if not np.array_equal(got, G[cur.local_slice()]):
                bad.append(('values', ax, got.shape))
        return bad
    res = run_ranks(P, body)
    assert not any(res), (P, shape, dt, rank, align, ndist, walk, [r for r in res if r][:1])
    return True


def impulse_errors(n, dt, strided, positions=None, lines=19):
    """Twiddle integrity of ONE serial plan of length n: line b of a batch holds a unit impulse at position j_b, so its
    transform is X_b[k] = exp(-2 pi i j_b k / n) -- every output a bare product of the plan's twiddle factors, of modulus
    1: a wrong table entry shows at full size in the outputs it feeds (random data dilutes it by ~1 / (3.5 sqrt(radix)),
    below fp32 rounding for an entry off by 1e-5).  `lines` lines, the positions taken cyclically: 19 by default, no
    multiple of a kernel tile (T = 1 ... 16 rows, 2 ... 32 columns), so the tail tile of every kernel is among them.
    Returns (max |forward - exact|, max |backward(exact) - impulse|), in units of 1 (no normalisation needed: |X| = 1,
    impulse height 1)."""
    from mpi4py_fft_amd import FFT, asdevice
    cdt = 'D' if dt in 'dD' else 'F'
    if positions is None:
        positions = [1, 2, 3, 5, 7, n // 2 + 1, n - 1, n // 3 + 1, n // 4 + 1, 11 % n, n // 5 + 2, n // 7 + 3, 1, n - 2, 13 % n, n // 2 - 1]
    positions = [int(positions[b % len(positions)]) % n for b in range(lines)]
    B = len(positions)
    shape, axis = ((n, B), 0) if strided else ((B, n), 1)
    x = np.zeros(shape, dtype=cdt)
    k = np.arange(n)
    want = np.empty(shape, dtype='D')
    for b, j in enumerate(positions):
        col = np.exp(-2j * np.pi * ((j * k) % n) / n)
        if strided:
            x[j, b] = 1
            want[:, b] = col
        else:
            x[b, j] = 1
            want[b] = col
    fft = FFT(shape, (axis,), dtype=cdt)
    got = np.asarray(fft.forward(asdevice(x), normalize=False)).astype('D')
    ef = float(np.abs(got - want).max())
    back = np.asarray(fft.backward(asdevice(want.astype(cdt)), normalize=True)).astype('D')
    eb = float(np.abs(back - x).max())
    fft.destroy()
    return ef, eb


# real lengths by the kernel family that runs their ROWS (plan.cpp plan_line: real_half_ok, regk_ok, generic_max_n)
REAL_LENGTHS = {'packed': [32, 64, 512, 2048, 8192, 96, 1536, 40, 1000, 8000, 224, 480],      # 2^k; 3^b 2^k; 5^c 2^k; twice 112, 240
                'regs': [16, 48],                        # halves 8 and 24 have no packed kernel: full-length register kernels
                'generic': [7, 9, 15, 121, 343, 1331, 22, 34],
                'embedded': [9216, 16384],               # real-as-complex
                'bluestein': [521, 1009]}
REAL_ROWS = [(n, path) for path, ns in REAL_LENGTHS.items() for n in ns]


def real_impulse_errors(n, dt, strided, lines=16, describe=None):
    """`impulse_errors` for ONE real plan of length n (r2c forward, c2r backward): the packed-real plans read a second
    table, rtw(n), in their Hermitian pass, and the full-length, generic and embedded real lines go through load / store
    adapters of their own -- none of which a complex plan builds.
    Forward: line b holds a unit impulse at j_b, X_b[k] = exp(-2 pi i j_b k / n), k = 0 ... n // 2.
    Backward, unnormalised: line b holds ONE non-zero bin k_b of amplitude a_b -- each of 0, 1, 2, 3, n // 4, n // 3 + 1,
    n // 2 - 1, n // 2 once with a = 1 and once with a = i --, x_j = 2 Re(a e^{2 pi i j k / n}) for an interior bin,
    Re(a) at k = 0 and Re(a) (-1)^j at the Nyquist bin of an even n: a = i there must give zeros.
    Returns (max |forward - exact|, max |backward - exact| / 2): both in units of the exact answer's peak.  `describe`,
    a list, receives gfft_plan_describe of the two plans."""
    from mpi4py_fft_amd import FFT, asdevice
    rdt = 'd' if dt in 'dD' else 'f'
    cdt = rdt.upper()
    h = n // 2 + 1
    positions = [1, 2, 3, 5, 7, n // 2 + 1, n - 1, n // 3 + 1, n // 4 + 1, 11 % n, n // 5 + 2, n // 7 + 3, 1, n - 2, 13 % n, n // 2 - 1]
    positions = [int(j) % n for j in positions][:lines]
    bins = [0, 1, 2, 3, n // 4, n // 3 + 1, n // 2 - 1, n // 2]
    assert all(0 <= k < h for k in bins), (n, bins)
    spikes = ([(k, 1.0) for k in bins] + [(k, 1j) for k in bins])[:lines]
    B = len(positions)
    assert len(spikes) == B
    shape, axis = ((n, B), 0) if strided else ((B, n), 1)
    hshape = (h, B) if strided else (B, h)
    x = np.zeros(shape, dtype=rdt)
    want = np.empty(hshape, dtype='D')
    spec = np.zeros(hshape, dtype=cdt)
    wantb = np.empty(shape, dtype='d')
    k = np.arange(h)
    j = np.arange(n)
    for b, (jb, (kb, a)) in enumerate(zip(positions, spikes)):
        col = np.exp(-2j * np.pi * ((jb * k) % n) / n)
        edge = kb == 0 or 2 * kb == n
        back = (1.0 if edge else 2.0) * (a * np.exp(2j * np.pi * ((j * kb) % n) / n)).real
        if strided:
            x[jb, b], want[:, b], spec[kb, b], wantb[:, b] = 1, col, a, back
        else:
            x[b, jb], want[b], spec[b, kb], wantb[b] = 1, col, a, back
    fft = FFT(shape, (axis,), dtype=rdt)
    if describe is not None:
        describe.extend(p._eng.plan_describe(p._plan) for p in (fft.fwd, fft.bck))
    got = np.asarray(fft.forward(asdevice(x), normalize=False)).astype('D')
    ef = float(np.abs(got - want).max())
    back = np.asarray(fft.backward(asdevice(spec), normalize=False)).astype('d')
    eb = float(np.abs(back - wantb).max()) / 2.0
    fft.destroy()
    return ef, eb


def real_path(describe):
    """Which kernel family ran a serial real plan, from gfft_plan_describe's text."""
    text = '\n'.join(describe)
    if 'multiply by B' in text:
        return 'bluestein'
    if 'embed' in text:
        return 'embedded'
    if 'packed-real' in text:
        return 'packed'
    if 'kernel=generic' in text:
        return 'generic'
    assert 'kernel=regs-' in text, text
    return 'regs'


# ---- the real-to-real family (DCT / DST I-IV): FFTW kind numbers, mpi4py_fft_amd.fftw.FFTW_REDFT00 ... FFTW_RODFT11 ----
REDFT00, REDFT01, REDFT10, REDFT11, RODFT00, RODFT01, RODFT10, RODFT11 = 3, 4, 5, 6, 7, 8, 9, 10
R2R_NAMES = {3: 'REDFT00', 4: 'REDFT01', 5: 'REDFT10', 6: 'REDFT11', 7: 'RODFT00', 8: 'RODFT01', 9: 'RODFT10', 10: 'RODFT11'}
# logical lengths N by the path that runs them (plan.cpp plan_r2r_line): the MODE_R2R load / store adapters of the register
# kernels (powers of two 64 ... 4096 -- the floor and the cap of pow2_r2r_supported --, 3^b 2^k, 5^c 2^k) and the embed /
# extract fallback: below the floor, just past the cap, 5^4 2^3 above 4096, a 3 x 5 x 2^k length (those kernels have no
# adapters), generic lengths with radix 7 and 11, and 2 x 521 through Bluestein
R2R_LENGTHS = {'adapter': [64, 128, 512, 4096, 48, 768, 3456, 20, 500, 4000],
               'fallback': [16, 32, 8192, 5000, 240, 14, 242],
               'bluestein': [1042]}
R2R_MAPPINGS = ('rows', 'cols', 'middle')


def r2r_points(kind, N):
    """Points n of a line of `kind` whose logical (complex) length is N: N = 2 (n - 1), 2 (n + 1) or 2 n."""
    assert N % 2 == 0, N
    return N // 2 + 1 if kind == REDFT00 else N // 2 - 1 if kind == RODFT00 else N // 2


def r2r_positions(n):
    """The impulse positions of `impulse_errors` with the duplicate 1 replaced by 0: both weight-1 edges of REDFT00 (0,
    n - 1), REDFT01 (0) and RODFT01 (n - 1) are hit."""
    return [int(j) % n for j in (1, 2, 3, 5, 7, n // 2 + 1, n - 1, n // 3 + 1, n // 4 + 1, 11 % n, n // 5 + 2, n // 7 + 3, 0, n - 2,
                                 13 % n, n // 2 - 1)]


def r2r_exact_impulse(kind, n, j):
    """The unnormalised transform (FFTW's definition, scipy's norm=None) of the unit impulse at j of n points, k = 0 ... n - 1:
    evaluated in np.longdouble with the integer product of the phase reduced modulo its period first, returned as float64.
      REDFT00  c cos(pi j k / (n - 1)), c = 1 at j in {0, n - 1}, else 2       RODFT00  2 sin(pi (j + 1)(k + 1) / (n + 1))
      REDFT10  2 cos(pi (2j + 1) k / (2n))                                     RODFT10  2 sin(pi (2j + 1)(k + 1) / (2n))
      REDFT01  c cos(pi j (2k + 1) / (2n)), c = 1 at j = 0, else 2             RODFT01  (-1)^k at j = n - 1, else 2 sin(pi (j + 1)(2k + 1) / (2n))
      REDFT11  2 cos(pi (2j + 1)(2k + 1) / (4n))                               RODFT11  2 sin(pi (2j + 1)(2k + 1) / (4n))
    (tests/test_r2r_exact_host.py holds these against scipy.)"""
    ld = np.longdouble
    pi = ld(4) * np.arctan(ld(1))
    j = int(j)
    assert 0 <= j < n and (n >= 2 or kind != REDFT00), (kind, n, j)
    k = np.arange(n, dtype=np.int64)

    def phase(m, half):               # pi m / half, m reduced modulo the period 2 half
        return pi * (m % (2 * half)).astype(ld) / ld(half)
    if kind == REDFT00:
        y = (1 if j in (0, n - 1) else 2) * np.cos(phase(j * k, n - 1))
    elif kind == REDFT10:
        y = 2 * np.cos(phase((2 * j + 1) * k, 2 * n))
    elif kind == REDFT01:
        y = (1 if j == 0 else 2) * np.cos(phase(j * (2 * k + 1), 2 * n))
    elif kind == REDFT11:
        y = 2 * np.cos(phase((2 * j + 1) * (2 * k + 1), 4 * n))
    elif kind == RODFT00:
        y = 2 * np.sin(phase((j + 1) * (k + 1), n + 1))
    elif kind == RODFT10:
        y = 2 * np.sin(phase((2 * j + 1) * (k + 1), 2 * n))
    elif kind == RODFT01:
        y = (1 - 2 * (k % 2)).astype(ld) if j == n - 1 else 2 * np.sin(phase((j + 1) * (2 * k + 1), 2 * n))
    else:
        assert kind == RODFT11, kind
        y = 2 * np.sin(phase((2 * j + 1) * (2 * k + 1), 4 * n))
    return np.asarray(y, dtype=np.float64)


def r2r_impulse_case(kind, N, mapping):
    """(shape, axis, x, want) of the impulse family of one r2r plan: n = r2r_points(kind, N) points along `axis`, line b holds a
    unit impulse at r2r_positions(n)[b mod 16], `want` its exact response in float64.  No batch is a multiple of a kernel
    tile (T = 1 ... 16 rows, 2 ... 32 columns), so the tail code of every adapter runs: 'rows' (19, n); 'cols' (n, 19);
    'middle' (3, n, 7) -- 3 slabs of 7 strided lines."""
    n = r2r_points(kind, N)
    shape, axis = {'rows': ((19, n), 1), 'cols': ((n, 19), 0), 'middle': ((3, n, 7), 1)}[mapping]
    pos = r2r_positions(n)
    lead = shape[:axis] + shape[axis + 1:]
    lines = int(np.prod(lead))
    xl, wl = np.zeros((lines, n)), np.empty((lines, n))          # one line per row, in the order of the other axes
    exact = {}
    for b in range(lines):
        j = pos[b % len(pos)]
        if j not in exact:
            exact[j] = r2r_exact_impulse(kind, n, j)
        xl[b, j] = 1
        wl[b] = exact[j]
    x, want = (np.ascontiguousarray(np.moveaxis(v.reshape(lead + (n,)), -1, axis)) for v in (xl, wl))
    assert x.shape == shape and x.sum() == lines
    return shape, axis, x, want


def r2r_impulse_errors(kind, N, dt, mapping, describe=None):
    """Table and adapter integrity of ONE r2r plan of logical length N (plan.cpp plan_r2r_line): every kind computes
    y[k] = Re(post[k] DFT_N(pre x)[idx0 + k]), so each output of a unit impulse at j is the bare product
    pre[j] w^((pos0 + j)(idx0 + k)) post[k] -- a wrong entry of either table, a wrong index shift, a zero-fill or a store
    that runs past its line (the type-1 kinds have a line pitch n != N / 2) shows at full size, and in the neighbouring
    line: every line is checked, and the output starts as NaN, so an entry left unwritten shows too.
    Out of place through fftw.get_planned_FFT.  Returns max |got - exact| over all lines, in units of 1 (the exact
    answer's peak is 2); `describe`, a list, receives gfft_plan_describe of the plan."""
    from mpi4py_fft_amd import fftw, asdevice
    rdt = 'd' if dt in 'dD' else 'f'
    shape, axis, x, want = r2r_impulse_case(kind, N, mapping)
    a = asdevice(x.astype(rdt))
    b = asdevice(np.full(shape, np.nan, dtype=rdt))
    plan = fftw.get_planned_FFT(a, b, (axis,), [kind])
    if describe is not None:
        describe.append(plan._eng.plan_describe(plan._plan))
    got = np.asarray(plan()).astype('d')
    plan.destroy()
    assert got.shape == want.shape
    err = np.abs(got - want).max()
    return float('inf') if np.isnan(err) else float(err)


def r2r_path(describe, N, mapping):
    """Which implementation ran a serial r2r plan, from gfft_plan_describe's text: 'adapter' is ONE register-kernel pass of
    length N in the mapping's own kernel; the fallback is embed ... extract around a complex plan, with Bluestein's
    multiplication in between for lengths with a large prime factor."""
    text = '\n'.join(describe)
    if 'embed' in text:
        assert 'extract' in text, text
        return 'bluestein' if 'multiply by B' in text else 'fallback'
    passes = [ln for ln in text.splitlines() if 'kernel=' in ln]
    assert len(passes) == 1 and ' n=%d ' % N in passes[0], text
    assert ('kernel=regs-rows' if mapping == 'rows' else 'kernel=regs-cols') in passes[0], text
    return 'adapter'


# ---- the 3/2-rule family: truncating store (forward) / zero-padding load (backward), libfft.py:263-311 of the model ----
# padded (transformed) length n -> kept length (complex entries N of a complex axis; REAL points of a real axis, of which
# m = kept // 2 + 1 half-spectrum entries are stored), by the path plan.cpp fused_pad_ok gives the plan in the shipped build
TRUNC_LENGTHS = {'fused pow2': [(64, 32), (64, 43), (1024, 512), (1024, 683), (4096, 2731)],
                 'fused 3^b 2^k': [(48, 32), (48, 31), (96, 64), (768, 512), (1536, 1024), (3072, 2048)],
                 'fused unequal-width': [(240, 160), (240, 161), (672, 448), (960, 640), (3600, 2400)],
                 'stand-alone': [(40, 27), (80, 63), (1000, 667), (112, 75), (1792, 1195), (18, 12), (27, 18), (343, 229), (8192, 5461),
                                 (521, 347)]}
TRUNC_CASES = [(n, kept, family) for family, pairs in TRUNC_LENGTHS.items() for n, kept in pairs]
TRUNC_MAPPINGS = R2R_MAPPINGS


def trunc_entries(n, kept, real):
    """(entries stored along the axis, entries of the full spectrum): N of n for a complex axis, m = kept // 2 + 1 of
    n // 2 + 1 for a real one.  The two agree when nothing is cut (kept == n): the exact answers below are then those of the
    plain transform -- no fold, no halving --, which is what the probe sets beside the padded plans."""
    return (kept // 2 + 1, n // 2 + 1) if real else (kept, n)


def _cis(m, n, sign):
    """exp(sign 2 pi i m / n) in long double, the integer array m reduced modulo n first."""
    ld = np.longdouble
    th = (ld(8) * np.arctan(ld(1))) * (np.asarray(m, dtype=np.int64) % n).astype(ld) / ld(n)
    return np.cos(th) + (1j * sign) * np.sin(th)


def _kappa(keep):
    k = np.arange(keep, dtype=np.int64)
    return np.where(k <= keep // 2, k, k - keep)


def trunc_exact_forward(n, keep, j, real):
    """The `keep` entries a truncating forward transform of padded length n stores for the unit impulse at j, unnormalised.
      complex   T[k] = exp(-2 pi i j kap(k) / n), kap(k) = k for k <= h = keep // 2, else k - keep; for an even keep the upper
                band's first entry n - h folds onto h: T[h] = 2 cos(2 pi j h / n)
      real      T[k] = exp(-2 pi i j k / n), k < keep = m; for an even m, T[m - 1] = 2 Re(...), imaginary part exactly 0
    (the parity rule is on the TRUNCATED array's length, libfft.py:267 -- for a real axis that is m, not the real length).
    Long double, integer phase products reduced modulo n first; returned as complex128.  tests/test_trunc_exact_host.py
    holds these against the float64 oracle."""
    j = int(j)
    full = n // 2 + 1 if real else n
    assert 0 <= j < n and 1 <= keep <= full, (n, keep, j)
    cut = keep < full
    if real:
        T = _cis(j * np.arange(keep, dtype=np.int64), n, -1)
        if cut and keep % 2 == 0:
            T[keep - 1] = 2 * T[keep - 1].real
    else:
        T = _cis(j * _kappa(keep), n, -1)
        if cut and keep % 2 == 0:
            T[keep // 2] = 2 * T[keep // 2].real
    return np.asarray(T, dtype=np.complex128)


def trunc_exact_backward(n, keep, kb, a, real):
    """The n points a zero-padding backward transform gives for ONE stored bin kb of amplitude a, unnormalised.
      complex   x[j] = a exp(+2 pi i j kap(kb) / n); for an even keep and kb == h, x[j] = a cos(2 pi j h / n) (both copies halved)
      real      kb = 0: Re(a);  even m and kb = m - 1: Re(a) cos(2 pi j kb / n) -- a = i gives zeros --;  otherwise
                2 Re(a exp(+2 pi i j kb / n))
    With nothing cut (keep is the full length) the plain backward transform: Re(a) (-1)^j at the Nyquist bin of an even n."""
    kb = int(kb)
    full = n // 2 + 1 if real else n
    assert 0 <= kb < keep <= full, (n, keep, kb)
    cut = keep < full
    j = np.arange(n, dtype=np.int64)
    a = complex(a)
    if real:
        w = _cis(j * kb, n, +1)
        if kb == 0:
            x = np.full(n, a.real, dtype=np.longdouble)
        elif (cut and keep % 2 == 0 and kb == keep - 1) or (not cut and 2 * kb == n):
            x = a.real * w.real
        else:
            x = 2 * (a.real * w.real - a.imag * w.imag)
        return np.asarray(x, dtype=np.float64)
    w = _cis(j * int(_kappa(keep)[kb]), n, +1)
    if cut and keep % 2 == 0 and kb == keep // 2:
        w = w.real + 0j
    return np.asarray(np.clongdouble(a) * w, dtype=np.complex128)


def trunc_bins(keep, real):
    """The bins of the backward lines, (kb, a) per line: complex 0, 1, 2, h - 1, h, h + 1 (first of the upper band), N - 2,
    N - 1 with a = 1 and again with a = i, then N // 3 + 1 for every further line; real 0, 1, 2, 3, m // 2, m - 3, m - 2, m - 1
    with a = 1 and with a = i, cyclically."""
    if real:
        bins = [0, 1, 2, 3, keep // 2, keep - 3, keep - 2, keep - 1]
    else:
        h = keep // 2
        bins = [0, 1, 2, h - 1, h, h + 1, keep - 2, keep - 1]
    assert all(0 <= k < keep for k in bins), (keep, real, bins)
    return [(k, 1.0) for k in bins] + [(k, 1j) for k in bins]


def trunc_impulse_lines(n, kept, real, lines):
    """The family as (lines, length) arrays, one line per row: x (impulses, n) and its exact truncated transform wf (keep);
    spec (one bin per line, keep) and its exact padded backward transform wb (n); the peaks (pf, pb) errors are taken
    relative to -- 2 where a fold or a 2 Re occurs in the answer, else 1."""
    keep, full = trunc_entries(n, kept, real)
    pos = r2r_positions(n)
    spikes = trunc_bins(keep, real)
    x = np.zeros((lines, n), dtype='d' if real else 'D')
    wf = np.empty((lines, keep), dtype='D')
    spec = np.zeros((lines, keep), dtype='D')
    wb = np.empty((lines, n), dtype='d' if real else 'D')
    ef, eb = {}, {}
    for b in range(lines):
        j = pos[b % len(pos)]
        kb, a = spikes[b % len(spikes)] if (real or b < len(spikes)) else (keep // 3 + 1, 1.0)
        if j not in ef:
            ef[j] = trunc_exact_forward(n, keep, j, real)
        if (kb, a) not in eb:
            eb[kb, a] = trunc_exact_backward(n, keep, kb, a, real)
        x[b, j] = 1
        wf[b] = ef[j]
        spec[b, kb] = a
        wb[b] = eb[kb, a]
    pf = 2.0 if keep < full and keep % 2 == 0 else 1.0
    pb = 2.0 if real else 1.0
    return x, wf, spec, wb, pf, pb


def trunc_impulse_case(n, kept, dt, mapping):
    """The impulse family of ONE padded plan in the mapping's layout ('rows' (19, n), 'cols' (n, 19), 'middle' (3, n, 7), as
    `r2r_impulse_case`: no batch a multiple of a kernel tile): (shape, axis, x, wf, spec, wb, pf, pb) -- x of `shape`, wf / spec
    with `keep` entries along `axis`, wb of `shape`."""
    real = dt in 'df'
    shape, axis = {'rows': ((19, n), 1), 'cols': ((n, 19), 0), 'middle': ((3, n, 7), 1)}[mapping]
    lead = shape[:axis] + shape[axis + 1:]
    x, wf, spec, wb, pf, pb = trunc_impulse_lines(n, kept, real, int(np.prod(lead)))
    x, wf, spec, wb = (np.ascontiguousarray(np.moveaxis(v.reshape(lead + (v.shape[-1],)), -1, axis)) for v in (x, wf, spec, wb))
    assert x.shape == wb.shape == shape and wf.shape == spec.shape
    return shape, axis, x, wf, spec, wb, pf, pb


def trunc_impulse_errors(n, kept, dt, mapping, describe=None):
    """Adapter integrity of ONE padded serial plan, FFT(shape, axis, dt, padding=n / kept), unnormalised and out of place into
    arrays that start as NaN (an entry left unwritten shows): forward the unit impulses of `r2r_positions(n)`, backward one
    stored bin per line (`trunc_bins`), every line against its exact answer (`trunc_exact_forward` / `trunc_exact_backward`).
    A wrong band edge, a dropped fold or halving, parity taken from the wrong length show at full size in the one or two
    entries they touch.  kept == n runs the unpadded plan on the same inputs.
    Returns (forward error, backward error), each max |got - exact| over all lines relative to the exact answer's peak
    (`trunc_impulse_lines`); `describe`, a list, receives `fft._fused_trunc` and gfft_plan_describe of the two plans."""
    from mpi4py_fft_amd import FFT, asdevice
    cdt = dt.upper()
    shape, axis, x, wf, spec, wb, pf, pb = trunc_impulse_case(n, kept, dt, mapping)
    fft = FFT(shape, axis, dtype=dt, padding=n / kept) if kept != n else FFT(shape, axis, dtype=dt)
    assert tuple(fft.forward.output_array.shape) == wf.shape, (n, kept, dt, fft.forward.output_array.shape, wf.shape)
    if describe is not None:
        describe.append(bool(fft._fused_trunc))
        describe.extend(p._eng.plan_describe(p._plan) for p in (fft.fwd, fft.bck))
    out = asdevice(np.full(wf.shape, np.nan, dtype=cdt))
    fft.forward(asdevice(x.astype(dt)), normalize=False, dst=out)
    got = np.asarray(out).astype('D')
    back = asdevice(np.full(shape, np.nan, dtype=dt))
    fft.backward(asdevice(spec.astype(cdt)), normalize=False, dst=back)
    gotb = np.asarray(back).astype(wb.dtype)
    fft.destroy()
    ef, eb = np.abs(got - wf).max() / pf, np.abs(gotb - wb).max() / pb
    return (float('inf') if np.isnan(ef) else float(ef)), (float('inf') if np.isnan(eb) else float(eb))


def trunc_path(describe, n, mapping):
    """'fused' or 'stand-alone' for what `trunc_impulse_errors` left in `describe`: a fused plan pair is ONE register-kernel
    pass each, of length n -- or n / 2, the packed-real form of contiguous real rows."""
    fused, texts = describe[0], describe[1:]
    if not fused:
        return 'stand-alone'
    for text in texts:
        passes = [ln for ln in text.splitlines() if 'kernel=' in ln]
        assert len(passes) == 1 and 'kernel=regs-' in passes[0], text
        assert ' n=%d ' % (n // 2 if 'packed-real' in passes[0] else n) in passes[0], text
        assert ('regs-rows' if mapping == 'rows' else 'regs-cols') in passes[0], text
    return 'fused'


def trunc_expected_path(n, family, dt, mapping):
    """What plan.cpp fused_pad_ok and plan_line give the shipped build, as a set of accepted paths.  The table's exceptions:
      * 5^c 2^k lengths (40, 80, 1000, and the packed-real rows of twice such a length) carry the adapters only in a
        `make VARIANTS=1` library: either path;
      * a REAL transform along a strided axis of an unequal-width length has no register kernel (generic kernel + separate
        truncation);
      * contiguous real rows of 8192 points run packed on the 4096-point kernel, which carries the adapters: fused."""
    real = dt in 'df'
    if family == 'fused unequal-width':
        return {'stand-alone'} if real and mapping != 'rows' else {'fused'}
    if family != 'stand-alone':
        return {'fused'}
    if n in (40, 80, 1000):
        return {'fused', 'stand-alone'}
    if n == 8192 and real and mapping == 'rows':
        return {'fused'}
    return {'stand-alone'}


# ---- launch forms (tests/test_gpu_tile_walk.py): one workgroup per tile against workgroups that walk several ----
def same_bits(a, b):
    """The two arrays hold the same BYTES: NaN payloads and the sign of a zero count, which `==` does not see."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def walk_batch(mapping, n, lines):
    """(shape, axis) of a batch of lines of n points in one of R2R_MAPPINGS: 'rows' (lines, n), 'cols' (n, lines) and the
    3-D 'middle' (5, n, 37) -- (outer, mid, inner) addressing, 185 lines whatever `lines` says."""
    return {'rows': ((lines, n), 1), 'cols': ((n, lines), 0), 'middle': ((5, n, 37), 1)}[mapping]


def plan_launches(plans):
    """[(tiles, workgroups)] of every pass of the given fftw.FFT plans' most recent launches (gfft_plan_pass_launch), in order."""
    return [tw for p in plans for tw in p._eng.plan_pass_launch(p._plan)]


def dirty_spectrum(shape, dt, seed):
    """A seeded complex Gaussian half-spectrum that is NOT Hermitian-clean: the DC and Nyquist entries keep their O(1)
    imaginary parts, as a spectrum does after a nonlinear term."""
    return O.rng_array(shape, np.dtype(dt).char.upper(), seed)


def clean_edges(c, n, axis=-1):
    """`c` with the imaginary parts a c2r of real length n along `axis` ignores set to zero: DC, and Nyquist for an even n."""
    c = c.copy()
    ix = [slice(None)] * c.ndim
    for kk in ([0, n // 2] if n % 2 == 0 else [0]):
        ix[axis] = kk
        c[tuple(ix)] = c[tuple(ix)].real
    return c


def check_pfft_backward_vs_oracle(P, shape, dt, seed=11, **kw):
    """PFFT.backward on P ranks of a global half-spectrum that is not Hermitian-clean (`dirty_spectrum`) against the
    float64 oracle on the same spectrum widened to complex128 -- whatever `dt`: numpy runs irfft of complex64 in single
    precision, so only the 'd' oracle is a high-precision reference."""
    from mpi4py_fft_amd import PFFT, newDistArray
    okw = {k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}
    offt = O.OPFFT(P, shape, dtype='d', **okw)
    G = dirty_spectrum(offt.output_shape, dt, seed)
    ref = offt.backward(offt.scatter(G.astype('D'), forward_output=True))
    nelem = int(np.prod(offt.input_shape))

    def body(comm):
        k = {a: (list(b) if isinstance(b, list) else b) for a, b in kw.items()}
        fft = PFFT(comm, shape, dtype=dt, **k)
        uh = newDistArray(fft, True)
        uh[...] = G[fft.local_slice(True)]
        back = np.asarray(fft.backward(uh)).copy()
        fft.destroy()
        return back

    for r, back in enumerate(run_ranks(P, body)):
        assert back.shape == ref[r].shape and back.dtype == np.dtype(dt), (back.shape, ref[r].shape, back.dtype)
        assert_close(back.astype('d'), ref[r], dt, nelem, (P, shape, dt, kw, r))
