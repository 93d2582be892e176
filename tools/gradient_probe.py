#!/usr/bin/env python3
"""Developer probe: the two kernels of the velocity-gradient diagnostics on the arrays of a real N^3 transform, fp64 and fp32:
  (a) gfft_ps_gradient, m = 1 and m = 3 -- m complex loads and 3 m stores per mode of the spectral block;
  (b) gfft_ps_gradient_stats -- nine real loads per point of the physical block (the two reduction kernels together);
  (y1) gfft_ps_scalar_flux with three scalars and (y2) gfft_ps_stats of a three-component field: the yardsticks, a pointwise
      kernel with the load / store mix of (a) and the reduction whose structure (b) follows;
  (c) the same work as array-sized torch expressions: 1j * K[j] * f_hat[c] for (a) and, for (b), the expressions of
      examples/dns_taylor_green.py's fused=False path (fp64, m = 3 only);
  (d) gfft_probe_copy of 2 GiB (read + write): the same-run streaming ceiling;
alternating in one process, HIP events after a warm-up, minimum and median of the rounds.  Reported: each kernel's achieved
bytes per second against (d).
usage: python tools/gradient_probe.py [N ...]   (default 256).  GRADIENT_PROBE_REPS sets the timed rounds (default 15)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mpi4py_fft_amd import PFFT, _lib, comm, spectral

REPS = int(os.environ.get('GRADIENT_PROBE_REPS', 15))
BOX = (2 * np.pi, 4 * np.pi, 4 * np.pi)             # the example's box


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def torch_stats(a):
    at = a.transpose(0, 1)
    S = (a + at) / 2
    w = torch.stack([a[2][1] - a[1][2], a[0][2] - a[2][0], a[1][0] - a[0][1]])
    div = a[0][0] + a[1][1] + a[2][2]
    ss, ww = (S * S).sum((0, 1)), (w * w).sum(0)
    Q = (div * div - (a * at).sum((0, 1))) / 2
    R = -torch.linalg.det(a.permute(2, 3, 4, 0, 1))
    sss = torch.einsum('ijxyz,jkxyz,kixyz->xyz', S, S, S)
    wsw = torch.einsum('ixyz,ijxyz,jxyz->xyz', w, S, w)
    diag = torch.stack([a[0][0], a[1][1], a[2][2]])
    off = torch.stack([a[0][1], a[1][0], a[0][2], a[2][0], a[1][2], a[2][1]])
    return torch.stack([ss.max(), ww.max(), div.abs().max(), (div * div).sum(), ss.sum(), ww.sum(), (ss * ss).sum(), (ww * ww).sum(),
                        (ss * ww).sum(), Q.sum(), R.sum(), (Q * Q).sum(), (R * R).sum(), sss.sum(), wsw.sum(), (diag ** 2).sum(),
                        (diag ** 3).sum(), (diag ** 4).sum(), (off ** 2).sum(), (off ** 4).sum()])


def main():
    L = _lib.lib()
    print(torch.cuda.get_device_name(0))
    src = torch.empty(1 << 28, dtype=torch.float64, device='cuda').normal_()
    dst = torch.empty_like(src)
    st = _lib.current_stream()

    def copy():
        _lib.check(L.gfft_probe_copy(src.data_ptr(), dst.data_ptr(), src.numel() * 8, st))
    copy()
    torch.cuda.synchronize()
    for N in [int(a) for a in sys.argv[1:]] or [256]:
        for dt in ('d', 'f'):
            rdt, size = (torch.float64, 8) if dt == 'd' else (torch.float32, 4)
            fft = PFFT(comm.COMM_SELF, [N] * 3, dtype=dt)
            ops = spectral.SpectralOps(fft, BOX)
            pshape = ops.pshape
            npts, nmodes = int(np.prod(pshape)), int(np.prod(ops.shape))
            K = [k.reshape([-1 if i == j else 1 for j in range(3)]) for i, k in enumerate(ops.K)]
            fh = torch.view_as_complex(torch.randn((3,) + ops.shape + (2,), dtype=rdt, device='cuda'))
            gh = torch.empty((3, 3) + ops.shape, dtype=fh.dtype, device='cuda')
            A = torch.randn((3, 3) + pshape, dtype=rdt, device='cuda')
            u, ut = A[0], torch.empty((3, 3) + pshape, dtype=rdt, device='cuda')
            gs = torch.empty(_lib.PS_GRAD_NVAL, dtype=torch.float64, device='cuda')
            ss = torch.empty(_lib.PS_STATS_HEAD + 3 * _lib.PS_STATS_PER_COMP, dtype=torch.float64, device='cuda')

            def torch_gradient():
                for c in range(3):
                    for j in range(3):
                        torch.mul(fh[c], 1j * K[j], out=gh[c, j])
            forms = [('(a) gfft_ps_gradient, m = 1', lambda: ops.gradient(fh[0], gh[0]), 4 * nmodes * 2 * size),
                     ('(a) gfft_ps_gradient, m = 3', lambda: ops.gradient(fh, gh), 12 * nmodes * 2 * size),
                     ('(b) gfft_ps_gradient_stats', lambda: ops.gradient_stats(A, out=gs, reduce=False), 9 * npts * size),
                     ('(y1) gfft_ps_scalar_flux, m = 3', lambda: spectral.scalar_flux(u, A[1], ut), 15 * npts * size),
                     ('(y2) gfft_ps_stats, m = 3', lambda: ops.stats(u, out=ss, reduce=False), 3 * npts * size),
                     ('(c1) torch gradient, m = 3', torch_gradient, None)]
            if dt == 'd':
                forms.append(('(c2) torch gradient statistics', lambda: torch_stats(A), None))
            forms.append(('(d) gfft_probe_copy', copy, 2 * src.numel() * 8))
            for _, f, _ in forms:
                f()
            torch.cuda.synchronize()
            ts = [[] for _ in forms]
            for r in range(REPS):                            # rotating: none always runs behind the same one
                for i in [(j + r) % len(forms) for j in range(len(forms))]:
                    ts[i].append(timed(forms[i][1]))
            ceiling = forms[-1][2] / min(ts[-1]) / 1e6
            print('N = %d fp%d: physical block %s, spectral block %s' % (N, 8 * size, pshape, ops.shape))
            for (name, _, nbytes), t in zip(forms, ts):
                rate = '' if nbytes is None else '  %.2f GB at %.0f GB/s = %.2f of the copy' % (nbytes / 1e9, nbytes / min(t) / 1e6, nbytes / min(t) / 1e6 / ceiling)
                print('  %-40s min %.3f  median %.3f ms%s' % (name, min(t), float(np.median(t)), rate), flush=True)
            del fh, gh, A, u, ut
            torch.cuda.empty_cache()
            fft.destroy()


if __name__ == '__main__':
    main()
