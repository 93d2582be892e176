#!/usr/bin/env python3
"""Developer probe: what the band forcing costs.  On the spectral block of a real N^3 transform ([3][N][N][N/2 + 1] complex,
fp64 and fp32):
  (a) gfft_ps_project -- the plain projection + viscous term, the yardstick: this kernel is what the forced one must match;
  (b) gfft_ps_project_forced, band (2, 4), the gain read from device memory -- the same nine component arrays, plus per mode
      two compares on |k|^2 and, for the few modes that pass them, the exact shell (fp64 square root and divide);
  (c) SpectralOps.forcing_gain(out=) -- the spectrum of shells 0..4 and gfft_ps_force_gain, once per time step,
(a) and (b) alternating in one process and swapping places every round (whichever always ran behind the other would
find a different cache), HIP events, minimum and median of the rounds.  (b) moves the bytes of (a): its minimum should not
exceed (a)'s minimum by more than (a)'s own spread in the run (median / minimum).
usage: python tools/forcing_probe.py [N ...]   (default 512).  FORCING_PROBE_REPS sets the timed rounds (default 16);
FORCING_PROBE_STEP=1 also runs examples/dns_taylor_green.py forced at M = log2 N (it prints its ms per RK4 step: the
denominator of (c)'s share of a step)."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mpi4py_fft_amd import PFFT, _lib, comm, spectral

REPS = int(os.environ.get('FORCING_PROBE_REPS', 16))
BAND = (2, 4)
BOX = (2 * np.pi, 4 * np.pi, 4 * np.pi)             # the example's box: dk = 1/2


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    eng = _lib.engine()
    print(torch.cuda.get_device_name(0))
    for N in [int(a) for a in sys.argv[1:]] or [512]:
        for dt in ('d', 'f'):
            fft = PFFT(comm.COMM_SELF, [N] * 3, dtype=dt)
            ops = spectral.SpectralOps(fft, BOX)
            prec = 8 if dt == 'd' else 4
            cdt = torch.complex128 if dt == 'd' else torch.complex64
            u = torch.empty((3,) + ops.shape, dtype=cdt, device='cuda')
            du = torch.empty_like(u)
            for t in (u, du):
                for c in range(3):                          # (component by component: normal_'s temporaries stay small)
                    torch.view_as_real(t[c]).normal_()
            nbytes = 3 * u.numel() * u.element_size()        # du read and written, u read
            gain = torch.zeros(2, dtype=torch.float64, device='cuda')

            def form_a():
                eng.ps_project(du, u, ops.K, ops.shape, 1e-3, prec)

            def form_b():
                eng.ps_project_forced(du, u, ops.K, ops.shape, 1e-3, ops.dk, BAND[0], BAND[1], 0.0, gain, prec)

            def form_c():
                ops.forcing_gain(u, 0.1, BAND, out=gain)

            for f in (form_c, form_a, form_b):               # (c) first: (b) reads the gain it writes
                f()
            torch.cuda.synchronize()
            g, ef = gain.cpu().tolist()
            ta, tb, tc = [], [], []
            for r in range(REPS):                            # (a) and (b) swap places every round: neither always runs second
                for ts, f in ((ta, form_a), (tb, form_b))[::1 if r % 2 == 0 else -1]:
                    ts.append(timed(f))
            for _ in range(REPS):
                tc.append(timed(form_c))
            a, b, c = min(ta), min(tb), min(tc)
            spread = float(np.median(ta)) / a
            print('N = %d fp%d: block %s, %.2f GB moved per projection; gain %.4e on band energy %.4e'
                  % (N, 8 * prec, ops.shape, nbytes / 1e9, g, ef))
            for name, ts in (('(a) gfft_ps_project', ta), ('(b) gfft_ps_project_forced', tb), ('(c) forcing_gain(out=)', tc)):
                print('  %-28s min %.3f  median %.3f ms   [%s]' % (name, min(ts), float(np.median(ts)), ' '.join('%.3f' % t for t in ts)))
            print('  (a) moves %.0f GB/s, (b) %.0f GB/s; (b) / (a) = %.4f against (a)\'s own spread median / min = %.4f: %s'
                  % (nbytes / a / 1e6, nbytes / b / 1e6, b / a, spread, 'within' if b / a <= spread else 'ABOVE'), flush=True)
            del u, du
            fft.destroy()
            torch.cuda.empty_cache()
        if os.environ.get('FORCING_PROBE_STEP') and N & (N - 1) == 0:
            spec = importlib.util.spec_from_file_location('dns_taylor_green_probe', os.path.join(ROOT, 'examples', 'dns_taylor_green.py'))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            M = N.bit_length() - 1
            mod.solve(comm.COMM_SELF, M=M, nsteps=5, verbose=True)
            mod.solve(comm.COMM_SELF, M=M, nsteps=5, verbose=True, forcing=(0.1, 2, 4), device_gain=True)
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
