#!/usr/bin/env python3
"""Developer probe: the physical-space statistics of a real N^3 fp64 three-component field (u = [3][N][N][N] float64) as
  (a) gfft_ps_stats -- one read of u, 20 doubles out;
  (b) the torch expressions a user would write without it: abs, weighted component sum and amax for the CFL rate, the
      squared magnitude's amax, and per component amax, amin, sum and pow(2..4).sum -- a pass and often an array-sized
      temporary per quantity;
  (c) gfft_probe_copy of u's bytes (read + write: the same-run streaming ceiling; half of it is the read of (a)),
forms alternating in one process, HIP events, minimum of the rounds.   usage: python tools/stats_probe.py [N ...]
(default 512 1024).  STATS_PROBE_REPS sets the timed rounds (default 7); STATS_PROBE_ONLY=a runs form (a) alone (for a
counter pass under rocprofv3)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mpi4py_fft_amd import _lib

REPS = int(os.environ.get('STATS_PROBE_REPS', 7))
only = os.environ.get('STATS_PROBE_ONLY')


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    eng, L, st = _lib.engine(), _lib.lib(), _lib.current_stream()
    print(torch.cuda.get_device_name(0))
    for N in [int(a) for a in sys.argv[1:]] or [512, 1024]:
        count = N ** 3
        u = torch.empty((3, N, N, N), dtype=torch.float64, device='cuda')
        for c in range(3):                          # (component by component: normal_'s temporaries stay small)
            u[c].normal_()
        nbytes = u.numel() * 8
        inv = [N / (2 * np.pi), N / (4 * np.pi), N / (4 * np.pi)]
        out = torch.zeros(20, dtype=torch.float64, device='cuda')

        def form_a():
            eng.ps_stats(u, 3, count, inv, out, 8)

        form_a()
        torch.cuda.synchronize()
        got = out.clone()
        form_a()
        torch.cuda.synchronize()
        assert torch.equal(got, out), 'the statistics do not repeat bit for bit'
        if only == 'a':
            ta = [timed(form_a) for _ in range(REPS)]
            print('N = %d  (a) gfft_ps_stats: %s ms' % (N, ' '.join('%.3f' % t for t in ta)))
            continue
        out_b = torch.zeros_like(out)
        w = torch.tensor(inv, dtype=torch.float64, device='cuda')[:, None, None, None]

        def form_b():
            out_b[0] = (u.abs() * w).sum(0).amax()
            out_b[1] = (u * u).sum(0).amax()
            for c in range(3):
                x = u[c]
                o = 2 + 6 * c
                out_b[o] = x.amax()
                out_b[o + 1] = x.amin()
                out_b[o + 2] = x.sum()
                out_b[o + 3] = x.pow(2).sum()
                out_b[o + 4] = x.pow(3).sum()
                out_b[o + 5] = x.pow(4).sum()

        dst = torch.empty_like(u)

        def form_c():
            _lib.check(L.gfft_probe_copy(u.data_ptr(), dst.data_ptr(), nbytes, st))

        for f in (form_b, form_c):
            f()
        torch.cuda.synchronize()
        scale = torch.maximum(got.abs(), torch.tensor(float(count) ** 0.5, dtype=torch.float64, device='cuda'))
        err = float(((out_b - got).abs() / scale).max())
        ta, tb, tc = [], [], []
        for _ in range(REPS):
            ta.append(timed(form_a))
            tb.append(timed(form_b))
            tc.append(timed(form_c))
        a, b, c = min(ta), min(tb), min(tc)
        print('N = %d: u %.2f GB; (a) and (b) agree to %.1e (of max(|value|, sqrt(count)))' % (N, nbytes / 1e9, err))
        for name, ts in (('(a) gfft_ps_stats', ta), ('(b) torch expressions', tb), ('(c) gfft_probe_copy', tc)):
            print('  %-24s min %.3f  median %.3f ms   [%s]' % (name, min(ts), float(np.median(ts)), ' '.join('%.3f' % t for t in ts)))
        # the yardstick of DESIGN.md section 6: the copy moves 2 x nbytes, so HALF its time is "a copy of the same bytes"
        print('  (a) reads %.0f GB/s; (c) moves %.0f GB/s (read + write); copy of the same bytes = (c) / 2 = %.3f ms; '
              'kernel / copy = %.2f (the spectrum kernel: 1.41 at 512^3, 1.07-1.19 at 1024^3); (b) / (a) = %.1f x'
              % (nbytes / a / 1e6, 2 * nbytes / c / 1e6, c / 2, a / (c / 2), b / a), flush=True)
        del dst, u
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
