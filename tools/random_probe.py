#!/usr/bin/env python3
"""Developer probe: random solenoidal fields on the spectral array of a real N^3 transform, fp64 and fp32, m = 3:
  (k) SpectralOps.random_solenoidal with a device amplitude table (gfft_ps_random_field: Philox, Box-Muller, projection, store);
  (r) SpectralOps.random_field end to end (fill, spectrum, the table on the host, scale_shells) -- wall-clock, it synchronises;
  (s) SpectralOps.scale_shells, m = 3, in place;
  (a) SpectralOps.scale_axes, m = 3, in place, shown beside (s): the separable multiplier it is the counterpart of;
  (t) the route a user has without the entry: torch.randn of the complex field, the projection and the amplitude as torch
      expressions over PREBUILT array-sized wavenumber meshes and shell indices (built outside the timing, and without the
      Hermitian symmetry the kernel gives: both in the route's favour);
  (z) a store-only fill of the field's bytes (Tensor.zero_): what the stores of (k) alone cost;
  (d) gfft_probe_copy of the field's bytes (read + write): the yardstick of (s);
rotating places in one process per precision, HIP events after a warm-up, minimum and median of the rounds.  Every precision is
a child process of its own under its own time limit; after a child that fails nothing more starts.
Gates (exit status 1 when one fails):
  1. (k) is not slower than (t), minimum against minimum;
  2. (s) per byte moved exceeds the copy's by no more than the copy's own spread (median / minimum), the rule scale_axes was held
     to against its yardstick (tools/interp_probe.py), in the same run.
usage: python tools/random_probe.py [N]   (default 256).  RANDOM_PROBE_REPS sets the timed rounds (default 15)."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = int(os.environ.get('RANDOM_PROBE_REPS', 15))


def timed(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def child(dt, N):
    import numpy as np
    import torch
    from mpi4py_fft_amd import PFFT, _lib, comm, spectral
    L = _lib.lib()
    print(torch.cuda.get_device_name(0))
    cdt, rdt, size = (torch.complex128, torch.float64, 8) if dt == 'd' else (torch.complex64, torch.float32, 4)
    fft = PFFT(comm.COMM_SELF, [N] * 3, dtype=dt)
    ops = spectral.SpectralOps(fft)
    nmodes = int(np.prod(ops.shape))
    nbytes = 3 * nmodes * 2 * size
    nb = ops.default_nbins()
    E = spectral.model_spectrum(ops.shells(nb), 'gaussian', 8.0, 1.0)
    amp = torch.as_tensor(np.sqrt(E)).to('cuda')
    u_hat = torch.zeros((3,) + ops.shape, dtype=cdt, device='cuda')
    dst = torch.empty_like(u_hat)
    bv = ops.bspline_vectors(4)
    st = _lib.current_stream()
    # what the torch route reads, built once outside the timing
    Km = torch.stack(torch.meshgrid(*ops.K, indexing='ij'))
    K2 = (Km * Km).sum(0)
    K_over_K2 = Km / torch.where(K2 == 0, torch.ones_like(K2), K2)
    shell = torch.floor(torch.sqrt(K2.to(torch.float64)) / ops.dk + 0.5).long().clamp_(max=nb - 1)
    amp_r = amp.to(rdt)
    ones = torch.ones(nb, dtype=torch.float64, device='cuda')          # (s) in place, round after round: the field stays what it is

    def route():
        G = torch.randn((3,) + ops.shape, dtype=cdt, device='cuda') * (2.0 ** 0.5)      # each part a standard normal
        G -= Km * (G * K_over_K2).sum(0)
        G *= amp_r[shell]
        return G

    def copy():
        _lib.check(L.gfft_probe_copy(u_hat.data_ptr(), dst.data_ptr(), nbytes, st))

    def end_to_end():
        t0 = time.perf_counter()
        ops.random_field(u_hat, E, seed=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    forms = [('(k) random_solenoidal, amp table', lambda: ops.random_solenoidal(u_hat, 1, 0, amp), None),
             ('(k) random_solenoidal, add', lambda: ops.random_solenoidal(u_hat, 1, 0, amp, add=True), None),
             ('(t) torch.randn + projection + amplitude', route, None),
             ('(z) store-only fill (zero_)', lambda: u_hat.zero_(), nbytes),
             ('(s) scale_shells, m = 3, in place', lambda: ops.scale_shells(u_hat, ones), 2 * nbytes),
             ('(a) scale_axes, m = 3, in place', lambda: ops.scale_axes(u_hat, bv), 2 * nbytes),
             ('(d) gfft_probe_copy (yardstick)', copy, 2 * nbytes)]
    a = ops.random_solenoidal(u_hat, 1, 0, amp).clone()
    same = bool((torch.view_as_real(ops.random_solenoidal(u_hat, 1, 0, amp)) == torch.view_as_real(a)).all())
    mean = float((a.abs() ** 2).sum(0).mean()) / float((amp[shell] ** 2).mean())
    print('  two calls identical: %s; mean sum_c |u_hat_c|^2 / mean amp^2 = %.3f (4 less the zeroed share)' % (same, mean))
    for _, f, _ in forms:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in forms]
    for r in range(REPS):                                # rotating: none always runs behind the same one
        for i in [(j + r) % len(forms) for j in range(len(forms))]:
            ts[i].append(timed(forms[i][1]))
    e2e = [end_to_end() for _ in range(5)]
    mins, meds = [min(t) for t in ts], [float(np.median(t)) for t in ts]
    ceiling = forms[-1][2] / mins[-1] / 1e6
    print('N = %d fp%d: spectral block %s, m = 3, %.3f GB; copy (read + write) %.0f GB/s' % (N, 8 * size, ops.shape, nbytes / 1e9, ceiling))
    for (name, _, info), lo, med in zip(forms, mins, meds):
        extra = ''
        if name.startswith('(k)'):
            extra = '  %.1f ps per mode; store-only fill / kernel = %.2f; torch / kernel = %.1f' % (lo * 1e9 / nmodes, mins[3] / lo, mins[2] / lo)
        elif info is not None:
            extra = '  %.3f GB at %.0f GB/s = %.2f of the copy' % (info / 1e9, info / lo / 1e6, info / lo / 1e6 / ceiling)
        print('  %-42s min %.3f  median %.3f ms%s' % (name, lo, med, extra), flush=True)
    print('  %-42s min %.3f  median %.3f ms (wall clock, synchronised; 5 runs)' % ('(r) random_field end to end', min(e2e), float(np.median(e2e))))
    ok = same
    good = mins[0] <= mins[2]
    ok &= good
    print('  gate 1: fill %.3f ms <= torch route %.3f ms: %s' % (mins[0], mins[2], 'pass' if good else 'FAIL'))
    per_byte, yard, spread = mins[4] / forms[4][2], mins[6] / forms[6][2], meds[6] / mins[6]
    good = per_byte <= yard * spread
    ok &= good
    print('  gate 2: scale_shells %.4f ps per byte <= copy %.4f x its spread %.3f = %.4f: %s   (scale_axes: %.4f)'
          % (per_byte * 1e9, yard * 1e9, spread, yard * spread * 1e9, 'pass' if good else 'FAIL', mins[5] / forms[5][2] * 1e9))
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
