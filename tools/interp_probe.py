#!/usr/bin/env python3
"""Developer probe: the B-spline interpolation on the arrays of a real N^3 transform, fp64 and fp32, m = 3, P = 2^20 particles:
  (a) SpectralOps.interpolate, order 2 and order 4, the particles in random order;
  (b) the same with the particles sorted by cell index (sorted once on the host, outside the timing);
  (c) the route a user has without the entry: torch index expressions for order 2 -- per axis the base cell, the weights and
      the wrapped indices, then eight gathers per component (what the example's fused=False path runs);
  (d) gfft_probe_copy of 2 GiB (read + write): the same-run streaming ceiling;
  (e) SpectralOps.scale_axes, m = 3, in place, against gfft_ps_gradient with m = 1 as its yardstick, both per byte moved;
alternating in one process per precision, HIP events after a warm-up, minimum and median of the rounds.  Every precision, and
every run of the example, is a child process of its own under its own time limit; after a child that fails nothing more starts.
Gates (exit status 1 when one fails):
  1. (a) and (b) at order 2 do not exceed (c)'s minimum;
  2. scale_axes' minimum time per byte exceeds its yardstick's by no more than the yardstick's own spread (median / minimum).
Reported beside them: the gather's rate against the line model (order^2 m lines of 128 bytes per particle), the ratio of (a) to
(b), and with --example the time of a step of examples/dns_taylor_green.py at N^3 with and without 2^20 tracers.
usage: python tools/interp_probe.py [--example] [N]   (default 256).  INTERP_PROBE_REPS sets the timed rounds (default 15)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = int(os.environ.get('INTERP_PROBE_REPS', 15))
P = 1 << 20
LINE = 128
BOX = None          # the default box [0, 2 pi)^3


def timed(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def torch_linear(field, x, inv_dx):
    """order 2 as index expressions over the whole periodic grid: the weights of the kernel, eight gathers per component"""
    import torch
    n = field.shape[1:]
    w, idx = [], []
    for a in range(3):
        s = x[:, a] * inv_dx[a]
        i = torch.floor(s)
        t = s - i
        b = i.long()
        w.append([1.0 - t, t])
        idx.append([b % n[a], (b + 1) % n[a]])
    out = torch.zeros((x.shape[0], field.shape[0]), dtype=torch.float64, device=x.device)
    for j0 in range(2):
        for j1 in range(2):
            for j2 in range(2):
                out += (w[0][j0] * w[1][j1] * w[2][j2])[:, None] * field[:, idx[0][j0], idx[1][j1], idx[2][j2]].T.to(torch.float64)
    return out


def child(dt, N):
    import numpy as np
    import torch
    from mpi4py_fft_amd import PFFT, _lib, comm, spectral
    L = _lib.lib()
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
    u = torch.randn((3,) + ops.pshape, dtype=rdt, device='cuda')
    rng = np.random.default_rng(3)
    x_h = rng.uniform(0.0, 2 * np.pi, (P, 3))
    cell = np.floor(x_h * (N / (2 * np.pi))).astype(np.int64)
    order = np.argsort((cell[:, 0] * N + cell[:, 1]) * N + cell[:, 2], kind='stable')
    x_rand, x_sort = torch.as_tensor(x_h, device='cuda'), torch.as_tensor(x_h[order], device='cuda')
    out = torch.empty((P, 3), dtype=torch.float64, device='cuda')
    f_hat = torch.randn((3,) + ops.shape, dtype=torch.complex128 if dt == 'd' else torch.complex64, device='cuda')
    g_out = torch.empty((3,) + ops.shape, dtype=f_hat.dtype, device='cuda')
    bv = ops.bspline_vectors(4)
    forms = [('(a) interpolate order 2, random', lambda: ops.interpolate(u, x_rand, order=2, out=out, reduce=False), 2),
             ('(b) interpolate order 2, sorted', lambda: ops.interpolate(u, x_sort, order=2, out=out, reduce=False), 2),
             ('(a) interpolate order 4, random', lambda: ops.interpolate(u, x_rand, order=4, out=out, reduce=False), 4),
             ('(b) interpolate order 4, sorted', lambda: ops.interpolate(u, x_sort, order=4, out=out, reduce=False), 4),
             ('(c) torch index expressions order 2, random', lambda: torch_linear(u, x_rand, ops.inv_dx), None),
             ('(c) torch index expressions order 2, sorted', lambda: torch_linear(u, x_sort, ops.inv_dx), None),
             ('(e) scale_axes, m = 3, in place', lambda: ops.scale_axes(f_hat, bv), 2 * 3 * nmodes * 2 * size),
             ('(e) gfft_ps_gradient, m = 1 (yardstick)', lambda: ops.gradient(f_hat[0], g_out), 4 * nmodes * 2 * size),
             ('(d) gfft_probe_copy', copy, 2 * src.numel() * 8)]
    check = torch_linear(u, x_rand[:1000], ops.inv_dx) - ops.interpolate(u, x_rand[:1000].contiguous(), order=2, reduce=False)
    assert float(check.abs().max()) <= 1e-12 * float(u.abs().max()), 'the torch route and the kernel disagree'
    for _, f, _ in forms:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in forms]
    for r in range(REPS):                                # rotating: none always runs behind the same one
        for i in [(j + r) % len(forms) for j in range(len(forms))]:
            ts[i].append(timed(forms[i][1]))
    mins, meds = [min(t) for t in ts], [float(np.median(t)) for t in ts]
    ceiling = forms[-1][2] / mins[-1] / 1e6
    print('N = %d fp%d: physical block %s, %d particles, m = 3; copy %.0f GB/s' % (N, 8 * size, ops.pshape, P, ceiling))
    for (name, _, info), lo, med in zip(forms, mins, meds):
        extra = ''
        if name.startswith('(a)') or name.startswith('(b)'):
            model = info * info * 3 * LINE               # order^2 rows of the stencil, m components, one line each
            extra = '  %.1f ns per 1000 particles; line model %d B per particle at %.0f GB/s = %.2f of the copy' % (
                lo * 1e6 / P * 1000, model, model * P / lo / 1e6, model * P / lo / 1e6 / ceiling)
        elif info is not None:
            extra = '  %.3f GB at %.0f GB/s = %.2f of the copy' % (info / 1e9, info / lo / 1e6, info / lo / 1e6 / ceiling)
        print('  %-46s min %.3f  median %.3f ms%s' % (name, lo, med, extra), flush=True)
    print('  (a) / (b): order 2 %.2f, order 4 %.2f' % (mins[0] / mins[1], mins[2] / mins[3]))
    ok = True
    gate = min(mins[4], mins[5])
    for i in (0, 1):
        good = mins[i] <= gate
        ok &= good
        print('  gate 1: %s %.3f ms <= torch route %.3f ms: %s' % (forms[i][0], mins[i], gate, 'pass' if good else 'FAIL'))
    per_byte = mins[6] / forms[6][2]
    yard, spread = mins[7] / forms[7][2], meds[7] / mins[7]
    good = per_byte <= yard * spread
    ok &= good
    print('  gate 2: scale_axes %.4f ps per byte <= yardstick %.4f x its spread %.3f = %.4f: %s'
          % (per_byte * 1e9, yard * 1e9, spread, yard * spread * 1e9, 'pass' if good else 'FAIL'))
    fft.destroy()
    return 0 if ok else 1


def example_child(N, with_particles):
    import importlib.util
    import torch
    from mpi4py_fft_amd import comm
    spec = importlib.util.spec_from_file_location('dns_taylor_green_probe', os.path.join(ROOT, 'examples', 'dns_taylor_green.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    M = N.bit_length() - 1
    for kw in ([dict(particles=(P, 2, 7)), dict(particles=(P, 4, 7))] if with_particles else [dict()]):
        ex.solve(comm.COMM_SELF, M=M, nsteps=1, **kw)                 # warm-up: plans, scratch
        torch.cuda.synchronize()
        ex.solve(comm.COMM_SELF, M=M, nsteps=5, verbose=True, **kw)
    return 0


def main():
    args = sys.argv[1:]
    if args and args[0] == '--child':
        sys.exit(child(args[1], int(args[2])))
    if args and args[0] == '--example-child':
        sys.exit(example_child(int(args[1]), args[2] == '1'))
    example = '--example' in args
    N = ([int(a) for a in args if not a.startswith('--')] or [256])[0]
    steps = [['--child', dt, str(N)] for dt in ('d', 'f')]
    if example:                                          # interleaved, every run a fresh process
        steps += [['--example-child', str(N), w] for w in ('0', '1', '0', '1')]
    worst = 0
    for step in steps:
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
