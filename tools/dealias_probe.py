#!/usr/bin/env python3
"""Developer probe: what the dealiasing truncation costs, and what it saves.  On the spectral block of a real N^3 transform
([3][N][N][N/2 + 1] complex, fp64 and fp32):
  (a) gfft_ps_project -- the plain projection + viscous term, the yardstick: 9 component arrays, 3 stores + 6 loads per mode;
  (b) gfft_ps_project_dealiased with all-keep mask vectors and kcut = inf -- the same bytes plus three cached mask bytes per
      mode: what the predicate itself costs;
  (c) gfft_ps_project_dealiased with the 2/3 mask -- 3 stores everywhere, the 6 loads only on the kept modes (about 0.30 of
      an r2c block): the byte model says (3 + 6 kept) / 9 of (a);
the three alternating in one process and rotating places every round (whichever always ran behind another would find a
different cache), HIP events, minimum and median of the rounds.  Acceptance: neither (b)'s nor (c)'s minimum may exceed
(a)'s minimum by more than (a)'s own spread in the run (median / minimum) -- a kernel that skips loads must never cost more.
What (c) gains against the byte model is reported, not required.
usage: python tools/dealias_probe.py [N ...]   (default 512).  DEALIAS_PROBE_REPS sets the timed rounds (default 15)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mpi4py_fft_amd import PFFT, _lib, comm, spectral

REPS = int(os.environ.get('DEALIAS_PROBE_REPS', 15))
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
            ones = [torch.ones(n, dtype=torch.uint8, device='cuda') for n in ops.shape]
            m23 = ops.dealias_mask('2/3')
            kept = float(np.prod([float(m.sum().item()) / len(m) for m in m23[:3]]))
            model = (3 + 6 * kept) / 9

            def form_a():
                eng.ps_project(du, u, ops.K, ops.shape, 1e-3, prec)

            def form_b():
                eng.ps_project_dealiased(du, u, ops.K, ones, ops.shape, 1e-3, np.inf, None, prec)

            def form_c():
                eng.ps_project_dealiased(du, u, ops.K, m23[:3], ops.shape, 1e-3, np.inf, None, prec)

            forms = [form_a, form_b, form_c]
            for f in forms:
                f()
            torch.cuda.synchronize()
            ts = [[], [], []]
            for r in range(REPS):                            # the three rotate: none always runs behind the same one
                for i in [(j + r) % 3 for j in range(3)]:
                    ts[i].append(timed(forms[i]))
            a, b, c = (min(t) for t in ts)
            spread = float(np.median(ts[0])) / a
            print('N = %d fp%d: block %s, %.2f GB moved per plain projection; the 2/3 mask keeps %.4f of the modes: byte model %.3f'
                  % (N, 8 * prec, ops.shape, nbytes / 1e9, kept, model))
            for name, t in zip(('(a) gfft_ps_project', '(b) dealiased, all-keep vectors', '(c) dealiased, 2/3 mask'), ts):
                print('  %-32s min %.3f  median %.3f ms   [%s]' % (name, min(t), float(np.median(t)), ' '.join('%.3f' % x for x in t)))
            print('  (a) moves %.0f GB/s; (a)\'s own spread median / min = %.4f' % (nbytes / a / 1e6, spread))
            print('  (b) / (a) = %.4f: %s;  (c) / (a) = %.4f: %s, against the byte model %.3f (%.0f GB/s of the bytes it does move)'
                  % (b / a, 'within' if b / a <= spread else 'ABOVE', c / a, 'within' if c / a <= spread else 'ABOVE', model,
                     nbytes * model / c / 1e6), flush=True)
            del u, du
            fft.destroy()
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
