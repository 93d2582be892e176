#!/usr/bin/env python3
"""Developer probe (round 3): the serial stages of one rank of the pipelined C4 / C5 transforms on 8
GPUs, timed on one GPU -- the stage plans exactly as pipeline.Pipeline builds them, on the line-aligned
exchange buffers (pipeline._Aligned) and on the C-order ones of round 2.

  python tools/stage_probe.py [slab|c4|c5|c5odd|all]     (c5odd = a rank of the 513-wide grid column; slab = C3, C4 on 2 ranks
  and C4 on the (8,1,1) grid: the two local stages as two launches against one fused launch, round 6)
  python tools/stage_probe.py realslab     (the same for REAL input: [r2c rows -> strided] / [strided -> c2r rows] as the two
  stand-alone plans the staged path runs against gfft_plan_create_guru2_real whole and per chunk, forms alternating, round 7)
"""
import os, sys
from types import SimpleNamespace as NS
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mpi4py_fft_amd import _lib
from mpi4py_fft_amd import pipeline as P


def timeit(fn, iters=9, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        s.record(); fn(); e.record(); e.synchronize()
        ts.append(s.elapsed_time(e))
    return min(ts)


def fake_stage(axis, shape_in, shape_out=None):
    return NS(axes=(axis,), _padded=False, forward=NS(input_array=NS(shape=shape_in), output_array=NS(shape=shape_out or shape_in)))


def run_case(name, prec, real0, sh0, nh, sh1, sh2, p0, K0, widths, p1, K1):
    isz = 2 * prec
    stages = [fake_stage(2, sh0, sh0[:2] + (nh,)), fake_stage(1, sh1), fake_stage(0, sh2)]
    eng = _lib.engine()
    nbuf = int(max(np.prod(sh1), np.prod(sh2), np.prod(sh0[:2]) * nh) * 1.25) + (1 << 20)
    cdt = torch.complex64 if prec == 4 else torch.complex128
    a = torch.randn(nbuf, dtype=cdt, device='cuda')
    b = torch.empty_like(a)
    alg = [np.prod(sh0) * (prec if real0 else isz) + np.prod(sh0[:2]) * nh * isz, 2 * np.prod(sh1) * isz, 2 * np.prod(sh2) * isz]

    only_dir, only_stage = os.environ.get('STAGE_PROBE_DIR'), os.environ.get('STAGE_PROBE_STAGE')     # profiling runs: one direction / stage per process

    def report(layout, fwd, bwd):
        for i in range(3):
            for tag, st in (('fwd', fwd[i]), ('bwd', bwd[i])):
                if st is None or (only_dir and tag != only_dir) or (only_stage and str(i) != only_stage):
                    continue
                t = timeit(lambda: [st.execute(eng, c, a.data_ptr(), b.data_ptr(), 1.0) for c in range(st.nchunks)])
                print('%-16s %-9s stage %d %s  %d step(s) %8.3f ms  %7.1f GB/s  %4.1f %%' % (
                    name, layout, i, tag, st.nchunks, t, alg[i] / t / 1e6, alg[i] / t / 1e6 / 80), flush=True)

    pipe = NS(precision=prec, isz=isz)
    plan = [dict(p=p0, K=K0, uneven=real0, widths=widths if real0 else None), dict(p=p1, K=K1, uneven=False)]
    al = P._Aligned(pipe, stages, plan, real0)
    assert al.ok, name
    only = os.environ.get('STAGE_PROBE_ONLY')           # profiling runs: one layout per process
    if only in (None, 'aligned'):
        report('aligned', al.fwd, al.bwd)
    # round 2's C-order exchange buffers
    lin = [P.Layout(sh0), P.Layout(sh1, 1, p0, 0, K0), P.Layout(sh2, 0, p1, 2, K1)]
    lout = [P.Layout(sh0, 2, p0, 0, K0) if not real0 else P.Layout(sh0), P.Layout(sh1, 1, p1, 2, K1), P.Layout(sh2)]
    fwd = [None if real0 else P._Stage(sh0, 2, lin[0], lout[0], -1, prec), P._Stage(sh1, 1, lin[1], lout[1], -1, prec),
           P._Stage(sh2, 0, lin[2], lout[2], -1, prec)]
    bwd = [None if real0 else P._Stage(sh0, 2, lout[0], lin[0], +1, prec), P._Stage(sh1, 1, lout[1], lin[1], +1, prec),
           P._Stage(sh2, 0, lout[2], lin[2], +1, prec)]
    if real0:
        fwd[0], bwd[0] = P._RealRows(sh0, p0, K0, True, prec), P._RealRows(sh0, p0, K0, False, prec)
    if only in (None, 'c-order'):
        report('c-order', fwd, bwd)
    for s in al.fwd + al.bwd + fwd + bwd:
        if s is not None:
            s.destroy()
    del a, b
    torch.cuda.empty_cache()


def run_slab(name, prec, N0, N1, N2, p, Ks=(1, 2, 4)):
    """The per-rank stages of a complex transform on a SLAB grid (first redistribution local): the two local stages as
    two stand-alone plans on the shared buffer (round 5: rows natural, then strided into the packed send buffer), as
    one fused launch (gfft_plan_create_guru2) whole and per chunk of planes, and the far stage on pitched slabs."""
    isz = 2 * prec
    eng = _lib.engine()
    cdt = torch.complex64 if prec == 4 else torch.complex128
    M0, N1b = p * N0, N1 // p
    E = P._pitch(N1b * N2, isz)
    nel = N0 * N1 * N2
    a = torch.randn(nel, dtype=cdt, device='cuda')
    mid = torch.empty(nel, dtype=cdt, device='cuda')
    b = torch.empty(max(p * N0 * E, M0 * E), dtype=cdt, device='cuda')
    c = torch.empty(nel, dtype=cdt, device='cuda')
    alg2, alg1 = 4 * nel * isz, 2 * nel * isz

    def line(tag, t, alg, extra=''):
        print('%-12s %-34s %8.3f ms  %7.1f GB/s  %4.1f %%  %s' % (name, tag, t, alg / t / 1e6, alg / t / 1e6 / 80, extra), flush=True)
    # two stand-alone launches: rows natural -> natural, strided natural -> packed [block][plane][rows of the block][cols]
    for kind, tag in ((-1, 'fwd'), (+1, 'bwd')):
        hr = eng.plan_create_guru(prec, kind, (N2, 1, 1), [(N0 * N1, N2, N2)], 1, 0, 1, 0)
        if kind < 0:
            hc = eng.plan_create_guru(prec, kind, (N1, N2, N2), [(N0, N1 * N2, N1b * N2), (N2, 1, 1)], 1, 0, p, N0 * N1b * N2)
            t = timeit(lambda: (eng.execute_ptr(hr, a.data_ptr(), mid.data_ptr(), 1.0), eng.execute_ptr(hc, mid.data_ptr(), b.data_ptr(), 1.0)))
        else:
            hc = eng.plan_create_guru(prec, kind, (N1, N2, N2), [(N0, N1b * N2, N1 * N2), (N2, 1, 1)], p, N0 * N1b * N2, 1, 0)
            t = timeit(lambda: (eng.execute_ptr(hc, b.data_ptr(), mid.data_ptr(), 1.0), eng.execute_ptr(hr, mid.data_ptr(), a.data_ptr(), 1.0)))
        line('two launches %s' % tag, t, alg2)
        eng.plan_destroy(hr)
        eng.plan_destroy(hc)
    for K in Ks:
        if N0 % K:
            continue
        for fwd in (True, False):
            st = P._PairStage((N0, N1, N2), p, K, E, fwd, prec)
            if st.plan is None:
                continue
            pin, pout = (a, b) if fwd else (b, c)
            t = timeit(lambda: [st.execute(eng, q, pin.data_ptr(), pout.data_ptr(), 1.0) for q in range(K)])
            line('pair K=%d %s (%d launch%s per chunk)' % (K, 'fwd' if fwd else 'bwd', st.launches, '' if st.launches == 1 else 'es'), t, alg2)
            st.destroy()
    # (the forward pair the other way round: rows first, the strided pass storing into the blocks)
    h = eng.plan_create_guru2(prec, -1, (N1, N2, N2), (N2, 1, 1), (N0, N1 * N2, E), False, 1, 0, p, N0 * E)
    if h is not None:
        line('pair K=1 fwd [rows -> strided] (%d)' % eng.plan_cost(h)[2], timeit(lambda: eng.execute_ptr(h, a.data_ptr(), b.data_ptr(), 1.0)), alg2)
        eng.plan_destroy(h)
    # the far stage: axis 0 over slabs E apart <-> the natural output
    x = torch.randn(M0 * E, dtype=cdt, device='cuda')
    y = torch.empty(M0 * N1b * N2, dtype=cdt, device='cuda')
    for kind, tag in ((-1, 'fwd'), (+1, 'bwd')):
        si, so = (E, N1b * N2) if kind < 0 else (N1b * N2, E)
        h = eng.plan_create_guru(prec, kind, (M0, si, so), [(N1b, N2, N2), (N2, 1, 1)], 1, 0, 1, 0)
        pin, pout = (x, y) if kind < 0 else (y, x)
        line('far stage (axis 0) %s' % tag, timeit(lambda: eng.execute_ptr(h, pin.data_ptr(), pout.data_ptr(), 1.0)), alg1)
        eng.plan_destroy(h)
    del a, b, c, mid, x, y
    torch.cuda.empty_cache()


def run_real_slab(name, prec, N0, N1, N2, p, Ks=(1, 2, 4), rounds=3):
    """The per-rank local stages of a REAL transform on a slab grid: two stand-alone plans -- packed-real r2c rows natural ->
    natural half spectrum, then the strided pass into the packed send buffer [block][plane][rows of the block][H] (what
    _fuse_packs makes the staged path run); backward the mirror -- against the pair (pipeline._PairStage(real=True),
    gfft_plan_create_guru2_real) whole and per chunk of planes.  Every form is timed once per round, the rounds alternate
    the forms in one process; the best of each is reported with its ratio to the two launches."""
    isz = 2 * prec
    eng = _lib.engine()
    rdt, cdt = (torch.float32, torch.complex64) if prec == 4 else (torch.float64, torch.complex128)
    H = N2 // 2 + 1
    N1b = N1 // p
    E = P._pitch(N1b * H, isz)
    rows = N0 * N1
    x = torch.randn(rows * N2, dtype=rdt, device='cuda')
    y = torch.empty(rows * N2, dtype=rdt, device='cuda')
    mid = torch.empty(rows * H, dtype=cdt, device='cuda')
    b = torch.randn(max(p * N0 * E, rows * H), dtype=cdt, device='cuda')
    alg = rows * (N2 * prec + 3 * H * isz)          # r2c rows (real in, half spectrum out) + strided (read + write)
    forms = {}
    hr_f = eng.plan_create((rows, N2), (rows, H), (1,), _lib.R2C, prec)
    hr_b = eng.plan_create((rows, H), (rows, N2), (1,), _lib.C2R, prec)
    hc_f = eng.plan_create_guru(prec, -1, (N1, H, H), [(N0, N1 * H, N1b * H), (H, 1, 1)], 1, 0, p, N0 * N1b * H)
    hc_b = eng.plan_create_guru(prec, +1, (N1, H, H), [(N0, N1b * H, N1 * H), (H, 1, 1)], p, N0 * N1b * H, 1, 0)
    forms[('fwd', 'two launches')] = lambda: (eng.execute_ptr(hr_f, x.data_ptr(), mid.data_ptr(), 1.0),
                                               eng.execute_ptr(hc_f, mid.data_ptr(), b.data_ptr(), 1.0))
    forms[('bwd', 'two launches')] = lambda: (eng.execute_ptr(hc_b, b.data_ptr(), mid.data_ptr(), 1.0),
                                               eng.execute_ptr(hr_b, mid.data_ptr(), y.data_ptr(), 1.0))
    stages = []
    for K in Ks:
        if N0 % K:
            continue
        for fwd in (True, False):
            st = P._PairStage((N0, N1, N2), p, K, E, fwd, prec, real=True)
            if st.plan is None:
                continue
            stages.append(st)
            pin, pout = (x, b) if fwd else (b, y)
            forms[('fwd' if fwd else 'bwd', 'pair K=%d (%d launch%s per chunk)' % (K, st.launches, '' if st.launches == 1 else 'es'))] = \
                (lambda st=st, pin=pin, pout=pout: [st.execute(eng, q, pin.data_ptr(), pout.data_ptr(), 1.0) for q in range(st.nchunks)])
    best = {k: float('inf') for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            best[k] = min(best[k], timeit(fn))
    for (d, tag), t in best.items():
        ratio = t / best[(d, 'two launches')]
        print('%-18s %s %-34s %8.3f ms  %7.1f GB/s  %4.1f %%  %.3f x two launches' % (
            name, d, tag, t, alg / t / 1e6, alg / t / 1e6 / 80, ratio), flush=True)
    for h in (hr_f, hr_b, hc_f, hc_b):
        eng.plan_destroy(h)
    for st in stages:
        st.destroy()
    del x, y, mid, b
    torch.cuda.empty_cache()


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else 'all'
    print(torch.cuda.get_device_name(0))
    if what == 'chunks':
        for K0, K1 in ((1, 1), (2, 2), (4, 1), (1, 4)):
            run_case('C4@8 K0=%d K1=%d' % (K0, K1), 8, False, (256, 512, 1024), 1024, (256, 1024, 512), (1024, 256, 512), 2, K0, None, 4, K1)
        for K0 in (1, 2):
            run_case('C5@8e K0=%d' % K0, 4, True, (512, 1024, 2048), 1025, (512, 2048, 512), (2048, 512, 512), 2, K0, [513, 512], 4, 1)
        return
    if what in ('slab', 'all'):
        run_slab('C3 (2,1,1)', 8, 256, 512, 512, 2)
        run_slab('C4@2', 8, 512, 1024, 1024, 2)
        run_slab('C4 (8,1,1)', 8, 128, 1024, 1024, 8)
        run_slab('c64 (8,1,1)', 4, 128, 1024, 1024, 8)
        if what == 'slab':
            return
    if what == 'realslab':
        cases = [('r C4@2', 8, 512, 1024, 1024, 2), ('r (8,1,1)', 8, 128, 1024, 1024, 8), ('r 2048 (8,1,1)', 8, 64, 1024, 2048, 8),
                 ('r f32 (8,1,1)', 4, 128, 1024, 1024, 8)]
        only = os.environ.get('STAGE_PROBE_CASE')        # one case per process
        for c in cases:
            if only and only != c[0]:
                continue
            _lib.set_option('fuse2_f32', 2 if c[1] == 4 else 1)       # (the real fp32 pairs: option fuse2_f32 = 2)
            run_real_slab(*c)
        return
    if what in ('c4', 'all'):
        run_case('C4@8', 8, False, (256, 512, 1024), 1024, (256, 1024, 512), (1024, 256, 512), 2, 4, None, 4, 4)
    if what in ('c5', 'all'):
        run_case('C5@8e', 4, True, (512, 1024, 2048), 1025, (512, 2048, 512), (2048, 512, 512), 2, 4, [513, 512], 4, 1)
    if what in ('c5odd', 'all'):
        run_case('C5@8o', 4, True, (512, 1024, 2048), 1025, (512, 2048, 513), (2048, 512, 513), 2, 4, [513, 512], 4, 1)


if __name__ == '__main__':
    main()
