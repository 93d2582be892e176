#!/usr/bin/env python3
"""Developer probe: the pointwise work of the passive-scalar right-hand side, m = 1 and m = 3 scalars, on the arrays of a real
N^3 transform in fp64:
  (a) gfft_ps_scalar_flux -- 3 + m loads and 3 m stores per point of the physical block;
  (b) gfft_ps_scalar_rhs with a mean gradient, no mask -- 4 m + 3 complex loads and m stores per mode of the spectral block;
      (b') without the mean gradient (4 m loads), (b'') with the mean gradient and the 2/3 mask (loads on the kept modes only);
  (c) the same work as the array-sized torch expressions of examples/dns_taylor_green.py's fused=False path (the wavenumbers as
      three array-sized meshes, one temporary per operator);
  (d) gfft_probe_copy of 2 GiB (read + write): the same-run streaming ceiling;
alternating in one process, HIP events after a warm-up, minimum and median of the rounds.  Reported: each kernel's achieved
bytes per second against (d), and (a) + (b) against (c).
usage: python tools/scalar_probe.py [N ...]   (default 256).  SCALAR_PROBE_REPS sets the timed rounds (default 15)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mpi4py_fft_amd import PFFT, _lib, comm, spectral

REPS = int(os.environ.get('SCALAR_PROBE_REPS', 15))
BOX = (2 * np.pi, 4 * np.pi, 4 * np.pi)             # the example's box
KAPPA = [0.03, 0.01, 0.1]
GRAD = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.5, -0.5, 0.25]]


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
        pshape = ops.pshape
        npts, nmodes = int(np.prod(pshape)), int(np.prod(ops.shape))
        src = torch.empty(1 << 28, dtype=torch.float64, device='cuda').normal_()
        dst = torch.empty_like(src)
        st = _lib.current_stream()

        def copy():
            _lib.check(L.gfft_probe_copy(src.data_ptr(), dst.data_ptr(), src.numel() * 8, st))
        copy()
        torch.cuda.synchronize()
        K = torch.stack([torch.broadcast_to(k.reshape([-1 if i == j else 1 for j in range(3)]), ops.shape) for i, k in enumerate(ops.K)]).contiguous()
        K2 = (K * K).sum(0)
        mask = ops.dealias_mask('2/3')
        kept = float(np.prod([float(m.sum().item()) / len(m) for m in mask[:3]]))
        u = torch.randn((3,) + pshape, dtype=torch.float64, device='cuda')
        uh = torch.view_as_complex(torch.randn((3,) + ops.shape + (2,), dtype=torch.float64, device='cuda'))
        for m in (1, 3):
            th = torch.randn((m,) + pshape, dtype=torch.float64, device='cuda')
            ut = torch.empty((m, 3) + pshape, dtype=torch.float64, device='cuda')
            tht = torch.view_as_complex(torch.randn((m,) + ops.shape + (2,), dtype=torch.float64, device='cuda'))
            fh = torch.view_as_complex(torch.randn((m, 3) + ops.shape + (2,), dtype=torch.float64, device='cuda'))
            dth = torch.empty_like(tht)
            kap, G = KAPPA[:m], GRAD[:m]

            def torch_flux():
                for s in range(m):
                    for j in range(3):
                        torch.mul(u[j], th[s], out=ut[s, j])

            def torch_rhs():
                for s in range(m):
                    dth[s].zero_()
                    for j in range(3):
                        dth[s].sub_(1j * K[j] * fh[s, j])
                    dth[s].sub_(kap[s] * K2 * tht[s])
                    dth[s].sub_(G[s][0] * uh[0] + G[s][1] * uh[1] + G[s][2] * uh[2])
            forms = [('(a) gfft_ps_scalar_flux', lambda: spectral.scalar_flux(u, th, ut), (3 + 4 * m) * npts * 8),
                     ('(b) gfft_ps_scalar_rhs, mean gradient', lambda: ops.scalar_rhs(dth, fh, tht, kap, G, uh), (5 * m + 3) * nmodes * 16),
                     ("(b') gfft_ps_scalar_rhs, no gradient", lambda: ops.scalar_rhs(dth, fh, tht, kap), 5 * m * nmodes * 16),
                     ("(b'') gfft_ps_scalar_rhs, gradient, 2/3", lambda: ops.scalar_rhs(dth, fh, tht, kap, G, uh, dealias=mask),
                      (m + (4 * m + 3) * kept) * nmodes * 16),
                     ('(c1) torch flux', torch_flux, None), ('(c2) torch rhs', torch_rhs, None),
                     ('(d) gfft_probe_copy', copy, 2 * src.numel() * 8)]
            for _, f, _ in forms:
                f()
            torch.cuda.synchronize()
            ts = [[] for _ in forms]
            for r in range(REPS):                            # rotating: none always runs behind the same one
                for i in [(j + r) % len(forms) for j in range(len(forms))]:
                    ts[i].append(timed(forms[i][1]))
            best = [min(t) for t in ts]
            ceiling = forms[-1][2] / best[-1] / 1e6
            print('N = %d fp64, m = %d: physical block %s, spectral block %s; the 2/3 mask keeps %.4f of the modes' % (N, m, pshape, ops.shape, kept))
            for (name, _, nbytes), t in zip(forms, ts):
                rate = '' if nbytes is None else '  %.2f GB at %.0f GB/s = %.2f of the copy' % (nbytes / 1e9, nbytes / min(t) / 1e6, nbytes / min(t) / 1e6 / ceiling)
                print('  %-40s min %.3f  median %.3f ms%s' % (name, min(t), float(np.median(t)), rate))
            print('  fused (a) + (b) = %.3f ms against the torch expressions (c1) + (c2) = %.3f ms: %.2fx' %
                  (best[0] + best[1], best[4] + best[5], (best[4] + best[5]) / (best[0] + best[1])), flush=True)
            del th, ut, tht, fh, dth
            torch.cuda.empty_cache()
        fft.destroy()


if __name__ == '__main__':
    main()
