#!/usr/bin/env python3
"""Developer probe: what the integrating factor costs the Runge-Kutta stage, on the spectral block of a real N^3 transform in
fp64, three components:
  (a) gfft_ps_rk_stage -- u = u0 + cb du, u1 += ca du: three loads and two stores per value, no wavenumbers;
  (b) gfft_ps_rk_stage_if with one nu (a velocity): the same bytes, three wavenumber lookups and one exp per mode;
  (c) gfft_ps_rk_stage_if with three different nu (three scalars): an exp per component;
      (b0) its last-stage form (u = None, all powers 0: no exp, three of the five streams) beside (a0), rk_stage's;
  (d) gfft_probe_copy of 2 GiB (read + write): the same-run streaming ceiling;
alternating in one process, HIP events after a warm-up, minimum and median of the rounds.  Reported: each form's achieved bytes
per second, its ratio to (d) and, the yardstick, to (a) -- both move 80 bytes per complex value.
usage: python tools/ifrk_probe.py [N ...]   (default 256).  IFRK_PROBE_REPS sets the timed rounds (default 15)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mpi4py_fft_amd import PFFT, _lib, comm, spectral

REPS = int(os.environ.get('IFRK_PROBE_REPS', 15))
BOX = (2 * np.pi, 4 * np.pi, 4 * np.pi)             # the example's box
NU = 0.000625
MIXED = [0.000625, 0.0025, 0.01]
H = 0.01


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    L = _lib.lib()
    print(torch.cuda.get_device_name(0))
    for N in [int(a) for a in sys.argv[1:]] or [256]:
        fft = PFFT(comm.COMM_SELF, [N] * 3, dtype='d')
        ops = spectral.SpectralOps(fft, BOX)
        nmodes = int(np.prod(ops.shape))
        src = torch.empty(1 << 28, dtype=torch.float64, device='cuda').normal_()
        dst = torch.empty_like(src)
        st = _lib.current_stream()

        def copy():
            _lib.check(L.gfft_probe_copy(src.data_ptr(), dst.data_ptr(), src.numel() * 8, st))
        cplx = lambda: torch.view_as_complex(torch.randn((3,) + ops.shape + (2,), dtype=torch.float64, device='cuda'))
        u, u0, u1, du = cplx(), cplx(), cplx(), cplx()
        keep = u1.clone()
        row = spectral.IFRK4[0]                           # powers 1, 1, 2, 2: E and E * E are both used
        full, tail = 5 * 3 * nmodes * 16, 3 * 3 * nmodes * 16
        eng = _lib.engine()
        forms = [('(a) gfft_ps_rk_stage', lambda: eng.ps_rk_stage(u, u0, u1, du, 6 * nmodes, row[0] * H, row[1] * H, 8), full),
                 ('(b) gfft_ps_rk_stage_if, one nu', lambda: ops.rk_stage_if(u, u0, u1, du, NU, row[0], row[1], row[2:], h=H), full),
                 ('(c) gfft_ps_rk_stage_if, three nu', lambda: ops.rk_stage_if(u, u0, u1, du, MIXED, row[0], row[1], row[2:], h=H), full),
                 ('(a0) gfft_ps_rk_stage, u = None', lambda: eng.ps_rk_stage(None, None, u1, du, 6 * nmodes, 0.0, H / 6, 8), tail),
                 ('(b0) gfft_ps_rk_stage_if, last stage', lambda: ops.rk_stage_if(None, None, u1, du, NU, 0.0, 1. / 6., (0, 0, 0, 0), h=H), tail),
                 ('(d) gfft_probe_copy', copy, 2 * src.numel() * 8)]
        for _, f, _ in forms:
            f()
        torch.cuda.synchronize()
        ts = [[] for _ in forms]
        for r in range(REPS):                            # rotating: none always runs behind the same one
            u1.copy_(keep)                               # (u1 is an accumulator: keep it finite over the rounds)
            for i in [(j + r) % len(forms) for j in range(len(forms))]:
                ts[i].append(timed(forms[i][1]))
        rate = [nbytes / min(t) / 1e6 for (_, _, nbytes), t in zip(forms, ts)]
        print('N = %d fp64, 3 components: spectral block %s, %d modes' % (N, ops.shape, nmodes))
        for (name, _, nbytes), t, r in zip(forms, ts, rate):
            print('  %-40s min %.3f  median %.3f ms  %.2f GB at %.0f GB/s = %.2f of the copy, %.2f of (a)'
                  % (name, min(t), float(np.median(t)), nbytes / 1e9, r, r / rate[-1], r / rate[0]))
        print('  one nu against gfft_ps_rk_stage: %.3f;  three nu: %.3f;  last stage against its rk_stage form: %.3f'
              % (rate[1] / rate[0], rate[2] / rate[0], rate[4] / rate[3]), flush=True)
        fft.destroy()


if __name__ == '__main__':
    main()
