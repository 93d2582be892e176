#!/usr/bin/env python3
"""Developer probe: the particle-to-grid spread on the arrays of a real N^3 transform, fp64 and fp32, m = 3, P = 2^20 particles
uniform in the box, order 2 and order 4:
  (a) SpectralOps.spread (gfft_ps_spread + gfft_ps_spread_finish; scale_exp, acc and out given), the particles in random order;
  (b) the same with the particles sorted by cell index (sorted once on the host, outside the timing);
  (c) the same with every particle at ONE position: the contention case, recorded and not gated (5 rounds);
  (s) gfft_ps_spread alone, random order: the rate of the adds in added bytes per second (8 bytes per stencil point and
      component), beside the 1.3 TB/s the 32-bit float atomics of this chip reach at their best access shape;
  (t) the route a user has without the entry, order 2: torch index expressions and `index_add_` (float atomics, array-sized
      index and weight temporaries) -- per stencil point and component, and per stencil point with the components in one call;
  (f) gfft_ps_spread_finish alone (m = 3, clear on) against gfft_ps_scale_axes with m = 1 in place as its pointwise yardstick,
      both per byte moved;
  (d) gfft_probe_copy of 2 GiB (read + write): the same-run streaming ceiling;
rotating places in one process per precision, HIP events after a warm-up, minimum and median of the rounds.  Every precision is
a child process of its own under its own time limit; after a child that fails nothing more starts.
Gates (exit status 1 when one fails):
  1. (a) at order 2 does not exceed the minimum of the torch route (either form, either order of the particles);
  2. finish's minimum time per byte exceeds its yardstick's by no more than the yardstick's own spread (median / minimum).
usage: python tools/spread_probe.py [N]   (default 256).  SPREAD_PROBE_REPS sets the timed rounds (default 15)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = int(os.environ.get('SPREAD_PROBE_REPS', 15))
P = 1 << 20
M = 3


def timed(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def torch_spread(q, x, inv_dx, out, together):
    """order 2 over the whole periodic grid with index_add_: out = real [m][n0][n1][n2], zeroed here"""
    import torch
    n = out.shape[1:]
    flat = out.view(out.shape[0], -1)
    flat.zero_()
    w, idx = [], []
    for a in range(3):
        s = x[:, a] * inv_dx[a]
        i = torch.floor(s)
        t = s - i
        b = i.long()
        w.append([1.0 - t, t])
        idx.append([b % n[a], (b + 1) % n[a]])
    for j0 in range(2):
        for j1 in range(2):
            for j2 in range(2):
                at = (idx[0][j0] * n[1] + idx[1][j1]) * n[2] + idx[2][j2]
                wgt = w[0][j0] * w[1][j1] * w[2][j2]
                if together:
                    flat.index_add_(1, at, (wgt[None, :] * q.T).to(out.dtype))
                else:
                    for c in range(out.shape[0]):
                        flat[c].index_add_(0, at, (wgt * q[:, c]).to(out.dtype))
    return out


def child(dt, N):
    import numpy as np
    import torch
    from mpi4py_fft_amd import PFFT, _lib, comm, spectral
    L = _lib.lib()
    eng = _lib.engine()
    print(torch.cuda.get_device_name(0))
    src = torch.empty(1 << 27, dtype=torch.float64, device='cuda').normal_()          # 1 GiB read + 1 GiB written
    dst = torch.empty_like(src)
    st = _lib.current_stream()

    def copy():
        _lib.check(L.gfft_probe_copy(src.data_ptr(), dst.data_ptr(), src.numel() * 8, st))
    rdt, size = (torch.float64, 8) if dt == 'd' else (torch.float32, 4)
    fft = PFFT(comm.COMM_SELF, [N] * 3, dtype=dt)
    ops = spectral.SpectralOps(fft)
    npts, nmodes = int(np.prod(ops.pshape)), int(np.prod(ops.shape))
    rng = np.random.default_rng(3)
    x_h = rng.uniform(0.0, 2 * np.pi, (P, 3))
    q_h = rng.standard_normal((P, M))
    cell = np.floor(x_h * (N / (2 * np.pi))).astype(np.int64)
    order = np.argsort((cell[:, 0] * N + cell[:, 1]) * N + cell[:, 2], kind='stable')
    x_rand, x_sort = torch.as_tensor(x_h, device='cuda'), torch.as_tensor(x_h[order], device='cuda')
    x_one = torch.as_tensor(np.tile(x_h[:1], (P, 1)), device='cuda')
    q_rand, q_sort = torch.as_tensor(q_h, device='cuda'), torch.as_tensor(q_h[order], device='cuda')
    e = ops.spread_scale_exp(q_rand)
    out = torch.empty((M,) + ops.pshape, dtype=rdt, device='cuda')
    t_out = torch.empty((M,) + ops.pshape, dtype=rdt, device='cuda')
    acc = torch.zeros((M,) + ops.pshape, dtype=torch.int64, device='cuda')
    skipped = torch.zeros(1, dtype=torch.int64, device='cuda')
    f_hat = torch.randn(ops.shape, dtype=torch.complex128 if dt == 'd' else torch.complex64, device='cuda')
    bv = ops.bspline_vectors(4)
    factor = 1.0 / 2.0 ** e

    def spread(x, q, o):
        return lambda: ops.spread(q, x, order=o, out=out, scale_exp=e, acc=acc, skipped=skipped)

    def only(x, q, o):
        return lambda: eng.ps_spread(acc, M, ops.pshape, ops.pstart, ops._N, ops.inv_dx, x, q, P, o, e, skipped)
    fin_bytes = M * npts * (16 + size)
    added = lambda o: o ** 3 * M * 8 * P
    forms = [('(a) spread order 2, random', spread(x_rand, q_rand, 2), None),
             ('(b) spread order 2, sorted', spread(x_sort, q_sort, 2), None),
             ('(a) spread order 4, random', spread(x_rand, q_rand, 4), None),
             ('(b) spread order 4, sorted', spread(x_sort, q_sort, 4), None),
             ('(s) gfft_ps_spread alone order 2, random', only(x_rand, q_rand, 2), ('added', added(2))),
             ('(s) gfft_ps_spread alone order 4, random', only(x_rand, q_rand, 4), ('added', added(4))),
             ('(s) gfft_ps_spread alone order 2, sorted', only(x_sort, q_sort, 2), ('added', added(2))),
             ('(s) gfft_ps_spread alone order 4, sorted', only(x_sort, q_sort, 4), ('added', added(4))),
             ('(t) torch index_add_ per component, random', lambda: torch_spread(q_rand, x_rand, ops.inv_dx, t_out, False), None),
             ('(t) torch index_add_ per component, sorted', lambda: torch_spread(q_sort, x_sort, ops.inv_dx, t_out, False), None),
             ('(t) torch index_add_ components together, random', lambda: torch_spread(q_rand, x_rand, ops.inv_dx, t_out, True), None),
             ('(t) torch index_add_ components together, sorted', lambda: torch_spread(q_sort, x_sort, ops.inv_dx, t_out, True), None),
             ('(f) gfft_ps_spread_finish, m = 3, clear', lambda: eng.ps_spread_finish(out, acc, M * npts, factor, True, size), ('moved', fin_bytes)),
             ('(f) scale_axes, m = 1, in place (yardstick)', lambda: ops.scale_axes(f_hat, bv), ('moved', 2 * nmodes * 2 * size)),
             ('(d) gfft_probe_copy', copy, ('moved', 2 * src.numel() * 8))]
    contention = [('(c) spread order 2, one position', spread(x_one, q_rand, 2)), ('(c) spread order 4, one position', spread(x_one, q_rand, 4))]
    a = ops.spread(q_rand, x_rand, order=2, scale_exp=e).to(torch.float64)
    b = torch_spread(q_rand, x_rand, ops.inv_dx, t_out, False).to(torch.float64)
    tol = (1e-11 if dt == 'd' else 1e-4) * float(a.abs().max())
    assert float((a - b).abs().max()) <= tol, 'the torch route and the kernel disagree'
    for _, f, _ in forms:
        f()
    acc.zero_()                                          # ((s) leaves its adds in acc; (a), (b) and (f) clear it as the forms rotate, and the add wraps)
    torch.cuda.synchronize()
    ts = [[] for _ in forms]
    for r in range(REPS):                                # rotating: none always runs behind the same one
        for i in [(j + r) % len(forms) for j in range(len(forms))]:
            ts[i].append(timed(forms[i][1]))
    acc.zero_()
    tc = [[timed(f) for _ in range(6)][1:] for _, f in contention]
    mins, meds = [min(t) for t in ts], [float(np.median(t)) for t in ts]
    ceiling = forms[-1][2][1] / mins[-1] / 1e6
    print('N = %d fp%d: physical block %s, %d particles, m = %d, scale_exp %d; copy %.0f GB/s' % (N, 8 * size, ops.pshape, P, M, e, ceiling))
    for (name, _, info), lo, med in zip(forms, mins, meds):
        extra = ''
        if info is not None:
            extra = '  %.3f GB %s at %.0f GB/s' % (info[1] / 1e9, info[0], info[1] / lo / 1e6)
            if info[0] == 'moved':
                extra += ' = %.2f of the copy' % (info[1] / lo / 1e6 / ceiling)
        print('  %-50s min %.3f  median %.3f ms%s' % (name, lo, med, extra), flush=True)
    for (name, _), t in zip(contention, tc):
        print('  %-50s min %.3f  median %.3f ms  (not gated)' % (name, min(t), float(np.median(t))), flush=True)
    print('  (a) / (b): order 2 %.2f, order 4 %.2f' % (mins[0] / mins[1], mins[2] / mins[3]))
    ok = True
    gate = min(mins[8:12])
    good = mins[0] <= gate
    ok &= good
    print('  gate 1: %s %.3f ms <= torch route %.3f ms: %s' % (forms[0][0], mins[0], gate, 'pass' if good else 'FAIL'))
    per_byte = mins[12] / forms[12][2][1]
    yard, spread_y = mins[13] / forms[13][2][1], meds[13] / mins[13]
    good = per_byte <= yard * spread_y
    ok &= good
    print('  gate 2: finish %.4f ps per byte <= yardstick %.4f x its spread %.3f = %.4f: %s'
          % (per_byte * 1e9, yard * 1e9, spread_y, yard * spread_y * 1e9, 'pass' if good else 'FAIL'))
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
