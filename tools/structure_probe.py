#!/usr/bin/env python3
"""Developer probe: the structure functions on the arrays of a real N^3 transform, fp64 and fp32, m = 3, along each axis, at
nsep = 1 (r = 1) and at the separations of `spectral.log_separations(N)`:
  (k) SpectralOps.structure_functions with out= and reduce=False (gfft_ps_structure: the tile kernel and the final combination);
  (t) the route a user has without the entry: per separation one torch `roll`, a difference, the powers and nine `sum`s per
      component set, in double -- array-sized temporaries throughout;
  (d) gfft_probe_copy of the field's own bytes (read + write): the same-run streaming yardstick;
rotating places in one process per precision, HIP events after a warm-up, minimum and median of the rounds.  Every precision is
a child process of its own under its own time limit; after a child that fails nothing more starts.
Reported beside the times: (t) / (k), and at nsep = 1 the bytes per second at which (k) reads the field once as a fraction of
the copy's (read + written) -- at many separations the pass is bound by fp64 arithmetic and LDS reads, not by HBM, and no such
figure is gated.
Gates (exit status 1 when one fails):
  1. (k) is not slower than (t), minimum against minimum, at nsep = 1 and at the logarithmic list, on every axis;
  2. two calls of (k) give identical bits, and (k) agrees with (t) to rounding.
usage: python tools/structure_probe.py [N]   (default 256).  STRUCTURE_PROBE_REPS sets the timed rounds (default 15)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = int(os.environ.get('STRUCTURE_PROBE_REPS', 15))
M = 3


def timed(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def torch_structure(u, axis, seps, lcomp):
    """float64 [nsep][m][9] by torch expressions: the sums of include/gfft.h (gfft_ps_structure), one roll per separation"""
    import torch
    rows = []
    u = u.to(torch.float64)                              # converted before any arithmetic, once per call (fp64: no copy)
    for r in seps:
        d = torch.roll(u, -r, dims=axis + 1) - u
        d2 = d * d
        d3 = d2 * d
        ad = d.abs()
        vals = [d, d2, d3, d2 * d2, d2 * d3, d3 * d3, ad, d2 * ad, d[lcomp][None] * d2]
        rows.append(torch.stack([v.sum(dim=(1, 2, 3)) for v in vals], dim=1))
    return torch.stack(rows)


def child(dt, N):
    import numpy as np
    import torch
    from mpi4py_fft_amd import PFFT, _lib, comm, spectral
    L = _lib.lib()
    print(torch.cuda.get_device_name(0))
    rdt, size = (torch.float64, 8) if dt == 'd' else (torch.float32, 4)
    fft = PFFT(comm.COMM_SELF, [N] * 3, dtype=dt)
    ops = spectral.SpectralOps(fft)
    npts = int(np.prod(ops.pshape))
    u = torch.randn((M,) + ops.pshape, dtype=rdt, device='cuda')
    dst = torch.empty_like(u)
    nbytes = M * npts * size
    st = _lib.current_stream()

    def copy():
        _lib.check(L.gfft_probe_copy(u.data_ptr(), dst.data_ptr(), nbytes, st))
    lists = [('nsep = 1', [1]), ('nsep = %d' % len(spectral.log_separations(N)), spectral.log_separations(N))]
    outs = {len(s): torch.empty((len(s), M, _lib.PS_SF_NVAL), dtype=torch.float64, device='cuda') for _, s in lists}
    forms, ok = [], True
    for axis in range(3):
        for label, seps in lists:
            def kern(axis=axis, seps=seps):
                return ops.structure_functions(u, axis, seps, lcomp=axis, out=outs[len(seps)], reduce=False)

            def route(axis=axis, seps=seps):
                return torch_structure(u, axis, seps, axis)
            a = kern().cpu().numpy().copy()
            b = kern().cpu().numpy().copy()
            t = route().cpu().numpy()
            same = np.array_equal(a.view(np.int64), b.view(np.int64))
            close = np.allclose(a, t, rtol=1e-9, atol=1e-9 * npts)
            ok &= same and close
            print('  axis %d, %s: two calls identical bits: %s; agrees with the torch route: %s' % (axis, label, same, close), flush=True)
            forms.append(('(k) axis %d, %s' % (axis, label), kern, 'k'))
            forms.append(('(t) axis %d, %s' % (axis, label), route, 't'))
    forms.append(('(d) gfft_probe_copy of the field', copy, 'd'))
    for _, f, _ in forms:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in forms]
    for r in range(REPS):                                # rotating: none always runs behind the same one
        for i in [(j + r) % len(forms) for j in range(len(forms))]:
            ts[i].append(timed(forms[i][1]))
    mins, meds = [min(t) for t in ts], [float(np.median(t)) for t in ts]
    ceiling = 2 * nbytes / mins[-1] / 1e6
    print('N = %d fp%d: physical block %s, m = %d, %.3f GB; copy (read + write) %.0f GB/s' % (N, 8 * size, ops.pshape, M, nbytes / 1e9, ceiling))
    for i, ((name, _, kind), lo, med) in enumerate(zip(forms, mins, meds)):
        extra = ''
        if kind == 'k':
            extra = '  torch / kernel = %.1f' % (mins[i + 1] / lo)
            if 'nsep = 1' in name:
                extra += '; one read at %.0f GB/s = %.2f of the copy' % (nbytes / lo / 1e6, nbytes / lo / 1e6 / ceiling)
        print('  %-34s min %.3f  median %.3f ms%s' % (name, lo, med, extra), flush=True)
    for i, (name, _, kind) in enumerate(forms):
        if kind == 'k':
            good = mins[i] <= mins[i + 1]
            ok &= good
            print('  gate 1: %s %.3f ms <= torch route %.3f ms: %s' % (name, mins[i], mins[i + 1], 'pass' if good else 'FAIL'))
    print('  gate 2 (identical bits, agreement with the torch route): see above; all gates: %s' % ('pass' if ok else 'FAIL'))
    fft.destroy()
    return 0 if ok else 1


def main():
    args = sys.argv[1:]
    if args and args[0] == '--child':
        sys.exit(child(args[1], int(args[2])))
    N = ([int(a) for a in args if not a.startswith('--')] or [256])[0]
    worst = 0
    for step in [['--child', dt, str(N)] for dt in ('d', 'f')]:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + step, timeout=240).returncode
        except subprocess.TimeoutExpired:
            print('step %s ran into its time limit: stopping' % step)
            sys.exit(124)
        if rc not in (0, 1):                             # 1: a gate failed; anything else: stop, start nothing more
            print('step %s ended with status %d: stopping' % (step, rc))
            sys.exit(rc if rc > 0 else 1)
        worst = max(worst, rc)
    sys.exit(worst)


if __name__ == '__main__':
    main()
