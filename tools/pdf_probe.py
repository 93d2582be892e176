#!/usr/bin/env python3
"""Developer probe: the histogram kernels on the arrays of a real N^3 transform, fp64 and fp32:
  (a) gfft_ps_histogram, m = 3, 256 bins over +-4 sigma of a standard normal field;
  (b) the same on a constant field -- every lane on one counter, the worst case for the LDS adds;
  (c) gfft_ps_gradient_pdf on a random gradient tensor: Q alone (256 bins) and the joint (R, Q) table at 128 x 128;
  (y1) gfft_ps_stats on the field of (a) and (y2) gfft_ps_gradient_stats on the tensor of (c): the moment kernels that move the
      same bytes, the yardsticks of the issue ("more than about twice the moment kernel: find what bounds it");
  (d) the route a user has without these entries: torch.histc per component for (a) and, for (c), Q and R as array-sized torch
      expressions binned by torch.histc and by an index expression + torch.bincount (torch.histogramdd where the device has it);
  (e) gfft_probe_copy of 2 GiB (read + write): the same-run streaming ceiling;
alternating in one process, HIP events after a warm-up, minimum and median of the rounds.  Reported: each kernel's achieved
bytes per second against (e), and for the library's forms the time per call of eight calls between one pair of events (the
device's share: a single call also counts the host's time between the first event and the launch).
usage: python tools/pdf_probe.py [N ...]   (default 256).  PDF_PROBE_REPS sets the timed rounds (default 15); PDF_PROBE_TORCH=0
leaves (d) out."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mpi4py_fft_amd import PFFT, _lib, comm, spectral

REPS = int(os.environ.get('PDF_PROBE_REPS', 15))
TORCH_ROUTE = os.environ.get('PDF_PROBE_TORCH', '1') != '0'          # 0: leave the torch route (d) out, the kernels alone
BOX = (2 * np.pi, 4 * np.pi, 4 * np.pi)             # the example's box


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def torch_invariants(a):
    at = a.transpose(0, 1)
    div = a[0][0] + a[1][1] + a[2][2]
    Q = (div * div - (a * at).sum((0, 1))) / 2
    R = -torch.linalg.det(a.permute(2, 3, 4, 0, 1))
    return R, Q


def torch_joint(a, rr, qr, nb):
    R, Q = torch_invariants(a)
    bx = ((R - rr[0]) * (nb / (rr[1] - rr[0]))).floor().long()
    by = ((Q - qr[0]) * (nb / (qr[1] - qr[0]))).floor().long()
    inside = (bx >= 0) & (bx < nb) & (by >= 0) & (by < nb)
    return torch.bincount((bx * nb + by)[inside], minlength=nb * nb)


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
            npts = int(np.prod(pshape))
            A = torch.randn((3, 3) + pshape, dtype=rdt, device='cuda')
            u = A[0]
            flat = torch.full((3,) + pshape, 0.3, dtype=rdt, device='cuda')
            oh = torch.empty((3, 256 + 3), dtype=torch.int64, device='cuda')
            o1 = torch.empty(256 + 3, dtype=torch.int64, device='cuda')
            oj = torch.empty(128 * 128 + 2, dtype=torch.int64, device='cuda')
            gs = torch.empty(_lib.PS_GRAD_NVAL, dtype=torch.float64, device='cuda')
            ss = torch.empty(_lib.PS_STATS_HEAD + 3 * _lib.PS_STATS_PER_COMP, dtype=torch.float64, device='cuda')
            rr, qr = (-8.0, 8.0), (-8.0, 8.0)
            forms = [('(a) gfft_ps_histogram, m = 3, normal', lambda: ops.histogram(u, (-4.0, 4.0), 256, out=oh, reduce=False), 3 * npts * size),
                     ('(b) gfft_ps_histogram, m = 3, constant', lambda: ops.histogram(flat, (-4.0, 4.0), 256, out=oh, reduce=False), 3 * npts * size),
                     ('(y1) gfft_ps_stats, m = 3', lambda: ops.stats(u, out=ss, reduce=False), 3 * npts * size),
                     ('(c) gfft_ps_gradient_pdf, Q', lambda: ops.gradient_pdf(A, 'Q', range=qr, bins=256, out=o1, reduce=False), 9 * npts * size),
                     ('(c) gfft_ps_gradient_pdf, (R, Q) 128 x 128', lambda: ops.gradient_pdf(A, 'R', 'Q', range=(rr, qr), bins=128, out=oj, reduce=False), 9 * npts * size),
                     ('(y2) gfft_ps_gradient_stats', lambda: ops.gradient_stats(A, out=gs, reduce=False), 9 * npts * size),
                     ('(d) torch.histc x 3', lambda: [torch.histc(u[c], 256, -4.0, 4.0) for c in range(3)], None),
                     ('(d) torch Q + histc', lambda: torch.histc(torch_invariants(A)[1], 256, qr[0], qr[1]), None),
                     ('(d) torch R, Q + bincount', lambda: torch_joint(A, rr, qr, 128), None)]
            if not TORCH_ROUTE:
                forms = [f for f in forms if not f[0].startswith('(d)')]
            try:
                if not TORCH_ROUTE:
                    raise RuntimeError('skipped (PDF_PROBE_TORCH=0)')
                R_, Q_ = torch_invariants(A[:, :, :2])
                torch.histogramdd(torch.stack([R_.reshape(-1), Q_.reshape(-1)], 1), bins=[128, 128], range=[rr[0], rr[1], qr[0], qr[1]])
                forms.append(('(d) torch R, Q + histogramdd',
                              lambda: torch.histogramdd(torch.stack([t.reshape(-1) for t in torch_invariants(A)], 1), bins=[128, 128],
                                                        range=[rr[0], rr[1], qr[0], qr[1]]), None))
            except Exception as exc:          # (not implemented on the device in every torch)
                print('  torch.histogramdd on the device: %s' % str(exc).splitlines()[0][:100])
            forms.append(('(e) gfft_probe_copy', copy, 2 * src.numel() * 8))
            for _, f, _ in forms:
                f()
            torch.cuda.synchronize()
            ts = [[] for _ in forms]
            for r in range(REPS):                            # rotating: none always runs behind the same one
                for i in [(j + r) % len(forms) for j in range(len(forms))]:
                    ts[i].append(timed(forms[i][1]))
            # the library's forms once more, eight calls between one pair of events: the single call above includes what the host
            # spends between the first event and the launch (the queue is empty then), which differs from wrapper to wrapper
            b2b = [min(timed(lambda: [f() for _ in range(8)]) / 8 for _ in range(5)) if nbytes is not None else None
                   for _, f, nbytes in forms]
            ceiling = forms[-1][2] / min(ts[-1]) / 1e6
            print('N = %d fp%d: physical block %s; (R, Q) outside %d, Q outside %d of %d' % (N, 8 * size, pshape, int(oj[-2]), int(o1[256] + o1[257]), npts))
            for (name, _, nbytes), t, b in zip(forms, ts, b2b):
                rate = '' if nbytes is None else '  %.2f GB at %.0f GB/s = %.2f of the copy;  x 8 back to back %.3f ms each' % (
                    nbytes / 1e9, nbytes / min(t) / 1e6, nbytes / min(t) / 1e6 / ceiling, b)
                print('  %-46s min %.3f  median %.3f ms%s' % (name, min(t), float(np.median(t)), rate), flush=True)
            del A, u, flat
            torch.cuda.empty_cache()
            fft.destroy()


if __name__ == '__main__':
    main()
