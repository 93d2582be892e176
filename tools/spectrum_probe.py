#!/usr/bin/env python3
"""Developer probe: the shell spectrum of a real N^3 fp64 vector field (u_hat = [3][N][N][N/2+1] complex128) as
  (a) gfft_ps_spectrum -- one read of u_hat;
  (b) the torch expressions a user would write without it, with the bin and |k|^2 MESHES already built (array-sized,
      kept between calls: the favourable form) -- |u|^2, component sum, weight broadcast, two index_add_;
  (c) gfft_probe_copy of u_hat's bytes (read + write: the same-run streaming ceiling),
forms alternating in one process, HIP events.   usage: python tools/spectrum_probe.py [N ...]   (default 512 1024)
Then the two-field forms on the same u_hat and a second field v_hat, transfer (T) and helicity (H):
  (a') gfft_ps_cospectrum -- GFFT_PS_DOT reads u_hat and v_hat once, GFFT_PS_HELICITY reads u_hat once;
  (b') torch expressions with the same kept meshes -- Re u Re v + Im u Im v, component sum, weight broadcast, two
       index_add_; for helicity the curl 1j * (K x u_hat) is MATERIALISED first (three components written, read back);
  (c') gfft_probe_copy moving the bytes (a') reads: u_hat -> a buffer is read + write = the two fields of T; half of it for H.
SPECTRUM_PROBE_REPS sets the timed rounds (default 7).  SPECTRUM_PROBE_ONLY=a runs form (a) alone, =a2 the two (a') kernels alone (for a counter pass under rocprofv3)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mpi4py_fft_amd import _lib

REPS = int(os.environ.get('SPECTRUM_PROBE_REPS', 7))      # (the torch forms take seconds per call at 1024^3)
only = os.environ.get('SPECTRUM_PROBE_ONLY')


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def two_fields(N, u, K, w, dk, nbins, k2sq=None, bins=None):
    """(a'), (b'), (c') for the transfer (T: u_hat . v_hat) and the helicity (H: u_hat alone); meshes given = all forms"""
    eng, L, st = _lib.engine(), _lib.lib(), _lib.current_stream()
    shape, nbytes = tuple(u.shape[1:]), u.numel() * 16
    v = torch.empty_like(u)
    for c in range(3):
        torch.view_as_real(v[c]).normal_()
    out_t, out_h = (torch.zeros((2, nbins), dtype=torch.float64, device='cuda') for _ in range(2))

    def a_t():
        eng.ps_cospectrum(u, v, 3, _lib.PS_DOT, 1.0, K, w, shape, dk, nbins, out_t, 8)

    def a_h():
        eng.ps_cospectrum(u, None, 3, _lib.PS_HELICITY, 1.0, K, w, shape, dk, nbins, out_h, 8)

    forms = [("(a') cospectrum DOT", a_t), ("(a') cospectrum HELICITY", a_h)]
    if bins is not None:
        ob_t, ob_h = torch.zeros_like(out_t), torch.zeros_like(out_h)
        k0, k1, k2 = K[0][:, None, None], K[1][None, :, None], K[2][None, None, :]

        def binned(e, ob):
            e *= w
            ob.zero_()
            ob[0].index_add_(0, bins, e.reshape(-1))
            e *= k2sq
            ob[1].index_add_(0, bins, e.reshape(-1))

        def b_t():
            binned((u.real * v.real + u.imag * v.imag).sum(0), ob_t)

        def b_h():
            wh = torch.empty_like(u)                    # the stored curl
            wh[0] = 1j * (k1 * u[2] - k2 * u[1])
            wh[1] = 1j * (k2 * u[0] - k0 * u[2])
            wh[2] = 1j * (k0 * u[1] - k1 * u[0])
            binned((u.real * wh.real + u.imag * wh.imag).sum(0), ob_h)

        def c_t():
            _lib.check(L.gfft_probe_copy(u.data_ptr(), v2.data_ptr(), nbytes, st))

        def c_h():
            _lib.check(L.gfft_probe_copy(u.data_ptr(), v2.data_ptr(), nbytes // 2, st))

        v2 = torch.empty_like(u)
        forms += [("(b') torch T", b_t), ("(b') torch H, stored curl", b_h), ("(c') copy, bytes of T", c_t),
                  ("(c') copy, bytes of H", c_h)]
    for _, f in forms:
        f()
    torch.cuda.synchronize()
    times = [[] for _ in forms]
    for _ in range(REPS):
        for t, (_, f) in zip(times, forms):
            t.append(timed(f))
    print('N = %d, two fields: u_hat and v_hat %.2f GB each' % (N, nbytes / 1e9))
    for (name, _), ts in zip(forms, times):
        print('  %-28s min %.3f  median %.3f ms   [%s]' % (name, min(ts), float(np.median(ts)), ' '.join('%.3f' % t for t in ts)))
    if bins is not None:
        err = [float(((x - y).abs().max() / y.abs().max())) for x, y in ((ob_t, out_t), (ob_h, out_h))]
        m = [min(t) for t in times]
        print("  (a') and (b') agree to %.1e (T), %.1e (H) of the largest bin" % tuple(err))
        print("  T: (a') reads %.0f GB/s; (c') moves %.0f GB/s; (a') / (c') time = %.2f; (b') / (a') = %.1f x"
              % (2 * nbytes / m[0] / 1e6, 2 * nbytes / m[4] / 1e6, m[0] / m[4], m[2] / m[0]))
        print("  H: (a') reads %.0f GB/s; (c') moves %.0f GB/s; (a') / (c') time = %.2f; (b') / (a') = %.1f x"
              % (nbytes / m[1] / 1e6, nbytes / m[5] / 1e6, m[1] / m[5], m[3] / m[1]), flush=True)


def main():
    eng, L, st = _lib.engine(), _lib.lib(), _lib.current_stream()
    print(torch.cuda.get_device_name(0))
    for N in [int(a) for a in sys.argv[1:]] or [512, 1024]:
        H = N // 2 + 1
        shape = (N, N, H)
        u = torch.empty((3,) + shape, dtype=torch.complex128, device='cuda')
        for c in range(3):                          # (component by component: randn's temporaries stay small)
            torch.view_as_real(u[c]).normal_()
        nbytes = u.numel() * 16
        k = np.fft.fftfreq(N, 1. / N)
        K = [torch.as_tensor(k, device='cuda'), torch.as_tensor(k, device='cuda'),
             torch.as_tensor(np.fft.rfftfreq(N, 1. / N), device='cuda')]
        w = torch.full((H,), 2.0, dtype=torch.float64, device='cuda')
        w[0] = w[-1] = 1.0
        dk = 1.0
        nbins = int(np.floor(np.sqrt(3.0) * (N // 2) / dk + 0.5)) + 1
        out = torch.zeros((2, nbins), dtype=torch.float64, device='cuda')

        def form_a():
            eng.ps_spectrum(u, 3, K, w, shape, dk, nbins, out, 8)

        form_a()
        torch.cuda.synchronize()
        got = out.clone()
        ta, tb, tc = [], [], []
        if only == 'a2':
            two_fields(N, u, K, w, dk, nbins)
            continue
        if only == 'a':
            ta = [timed(form_a) for _ in range(REPS)]
            print('N = %d  (a) gfft_ps_spectrum: %s ms' % (N, ' '.join('%.3f' % t for t in ta)))
            continue
        k2sq = (K[0][:, None, None] ** 2 + K[1][None, :, None] ** 2) + K[2][None, None, :] ** 2
        bins = torch.floor(torch.sqrt(k2sq) / dk + 0.5).long().reshape(-1)
        out_b = torch.zeros_like(out)

        def form_b():
            e = (u.real ** 2 + u.imag ** 2).sum(0)
            e *= w
            e *= 0.5
            out_b.zero_()
            out_b[0].index_add_(0, bins, e.reshape(-1))
            e *= k2sq
            out_b[1].index_add_(0, bins, e.reshape(-1))

        dst = torch.empty_like(u)

        def form_c():
            _lib.check(L.gfft_probe_copy(u.data_ptr(), dst.data_ptr(), nbytes, st))

        for f in (form_b, form_c):
            f()
        torch.cuda.synchronize()
        err = float(((out_b - got).abs() / got.abs().clamp_min(1e-300)).max())
        for _ in range(REPS):
            ta.append(timed(form_a))
            tb.append(timed(form_b))
            tc.append(timed(form_c))
        a, b, c = min(ta), min(tb), min(tc)
        print('N = %d: u_hat %.2f GB, %d bins; (a) and (b) agree to %.1e' % (N, nbytes / 1e9, nbins, err))
        for name, ts in (('(a) gfft_ps_spectrum', ta), ('(b) torch expressions', tb), ('(c) gfft_probe_copy', tc)):
            print('  %-24s min %.3f  median %.3f ms   [%s]' % (name, min(ts), float(np.median(ts)), ' '.join('%.3f' % t for t in ts)))
        print('  (a) reads %.0f GB/s; (c) moves %.0f GB/s (read + write), i.e. %.0f GB/s each way; (a) read rate / (c) total rate = %.2f; '
              '(b) / (a) = %.1f x' % (nbytes / a / 1e6, 2 * nbytes / c / 1e6, nbytes / c / 1e6, (nbytes / a) / (2 * nbytes / c), b / a), flush=True)
        del dst
        two_fields(N, u, K, w, dk, nbins, k2sq, bins)
        del k2sq, bins, u
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
