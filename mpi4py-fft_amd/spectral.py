"""The pseudo-spectral caller either side of the transform path.

The reference's demo solver (examples/spectral_dns_solver.py:65-91) writes the steps between a
``backward`` and the next ``forward`` as numpy expressions over array-sized wavenumber meshes.  On
the device each of those steps is one HIP kernel (csrc/spectral.hip) that reads its operands once:

    curl(u_hat, out)            out = 1j * (K x u_hat)                     compute_curl, :76-80
    cross(a, b, out)            out = a x b  (physical space)              cross, :69-74
    project(du_hat, u_hat, nu)  P = sum(du*K/|K|^2); du -= P*K; du -= nu*|K|^2*u_hat      :88-90
    rk_stage(u, u0, u1, du, cb, ca)   u = u0 + cb*du;  u1 += ca*du         :112-116

and so are the diagnostics a DNS reads every few steps, which the reference leaves to the user:

    spectrum(u_hat)             E(k) and |k|^2 E(k) per shell of width dk, Hermitian-weighted, one read of u_hat
    energy(u_hat), enstrophy(u_hat)   their totals: <u.u>/2 and <|grad u|^2>/2
    cospectrum(a_hat, b_hat)    Re(conj(a_hat) . b_hat) per shell, signed, one read of each field
    transfer(u_hat, n_hat)      T(k) of the shell budget dE(k)/dt = T(k) - 2 nu k^2 E(k); flux(T) = the energy flux
    helicity_spectrum(u_hat), helicity(u_hat)   H(k) = Re(conj(u_hat) . (i K x u_hat)) without a stored curl; <u . curl u>

and the physical-space side of the same diagnostics, one read of a real field, bit for bit repeatable:

    stats(u)                    CFL rate max sum_c |u_c| N_c / L_c, max |u|^2, and per component max, min and the sums of
                                u, u^2, u^3, u^4; moments(stats, npoints) turns the sums into mean / variance / skewness /
                                flatness; a NaN in a sum is the blow-up signal
    cfl_rate(u), timestep(u, cfl, dt_max)   the advective limit dt <= cfl / rate, clamped; with out= a device double[2]
                                the step never leaves the device and rk_stage(..., dt=) reads it there, so a
                                CFL-controlled RK4 step can be captured into one HIP graph

and the term that keeps a flow from decaying, so that all of the above have a stationary state to describe:

    forcing_gain(u_hat, eps, band)   g = min(eps / (2 E_f), gain_max) with E_f the energy in shells blo..bhi (a partial sum of
                                `spectrum`): the gain of the linear band forcing f_hat = g u_hat that injects energy at the
                                rate eps; with out= a device double[2] it never leaves the device
    project(du_hat, u_hat, nu, force=(g, band))   the projection with du_hat += g u_hat in the band fused in behind it: no
                                extra pass; g a float or that device tensor, so a forced step replays from one HIP graph

and the truncation that keeps the quadratic term free of aliasing errors over a long run:

    dealias_mask(rule='2/3', kcut=None)   three per-axis byte vectors (the sparse form of a box mask, as K is of the wavenumber
                                mesh) and a spherical cut |k| <= kcut: rule '2/3' keeps integer wavenumber n_i iff 3 |n_i| < N_i
    project(du_hat, u_hat, nu, dealias=mask)   the projection (forced or not) with the truncation fused in: a truncated mode
                                is stored as +0 and none of its six operands is loaded -- fewer bytes than without, no extra pass
    dealias(field, mask)        the truncation alone, in place (the initial condition): stores to truncated modes, reads nothing

and the transport of passive scalars, d theta/dt + u . grad theta = kappa lap theta - G . u (G an imposed mean gradient), in
flux form -- u . grad theta = div(u theta) for solenoidal u: one backward and three forward transforms per scalar, as the
gradient form, and no stored gradient; up to four scalars (several Schmidt numbers) per call, the velocity read once for all:

    scalar_flux(u, theta, out)  out[s][c] = u[c] * theta[s] (physical space): 3 + m loads and 3 m stores per point
    scalar_rhs(dtheta_hat, flux_hat, theta_hat, kappa, mean_gradient, u_hat, dealias=mask)
                                dtheta_hat[s] = -i K . flux_hat[s] - kappa[s] |K|^2 theta_hat[s] - G[s] . u_hat, the truncation
                                fused in as in `project`; without a mean gradient u_hat is not read at all

    The scalar's diagnostics are the functions above: `spectrum(theta_hat)[0]` is the variance spectrum (sums to
    <theta^2>/2); the scalar dissipation is chi = 2 kappa <|grad theta|^2> = 2 * kappa * 2 * sum(spectrum(theta_hat)[1]);
    the scalar flux <u_c theta> is sum(cospectrum(u_hat[c], theta_hat)[0]); `stats(theta)` gives the extrema; `rk_stage`
    works on any count.

and the time integrator that survives a stiff linear term -- a well-resolved run's nu k_max^2, a scalar of low Schmidt number,
hyperviscosity: explicit RK4 is stable on the negative real axis only for lambda h <= 2.785, and `timestep` limits the step by
the advective rate alone.  With the integrating factor v = exp(nu |K|^2 t) u_hat the linear term is integrated exactly and only
the nonlinear term sees RK4:

    rk_stage_if(u, u0, u1, du, nu, cb, ca, powers, h= or dt=)
                                u = E^q0 u0 + cb h E^qd du (skipped when u is None);  u1 = E^q1 u1 + ca h E^qa du, with
                                E = exp(-nu |K|^2 h / 2) per mode and powers = (q0, qd, q1, qa) in {0, 1, 2}: the pass of `rk_stage`
                                and one exp per mode; nu a float (a velocity) or one per component (several scalars)
    IFRK4                       the four rows (cb, ca, q0, qd, q1, qa) of classical integrating-factor RK4: u0 and u1 start as copies
                                of u_hat, the right-hand sides come from `project(..., nu=0)` / `scalar_rhs(..., kappa=0)`, the
                                last row goes with u=None, and u1 ends as the new u_hat

and the small scales in physical space, where a DNS is validated -- everything that is a function of the velocity-gradient
tensor A_ij = d u_i / d x_j: the spectral gradient in one pass, nine backward transforms, and ONE read of A that reduces it:

    gradient(f_hat, out)        out[c][j] = 1j * K[j] * f_hat[c] for m <= 4 fields at once ([3][3] + spectral shape for a velocity,
                                [3] + spectral shape for a scalar): m loads and 3 m stores per mode.  K is applied as given, as
                                in `curl`: the derivative of a Nyquist column is not real, and the 2/3 mask removes those columns
    gradient_stats(A)           20 numbers from one read of the real [3][3] + physical shape tensor, bit for bit repeatable: the
                                maxima of S_ij S_ij, |w|^2 and |div u| and the sums of div^2, S_ij S_ij, |w|^2, their squares and
                                product, the invariants Q and R and their squares, S_ij S_jk S_ki, w_i S_ij w_j and the second
                                to fourth powers of the longitudinal and transverse derivatives (`_lib.GS_*` name the entries)
    gradient_moments(gs, npoints, nu)   turns them into dissipation, enstrophy, <Q>, <R>, derivative skewness and flatness,
                                the intermittency of dissipation and enstrophy, and the Betchov ratio <w S w> / (-4/3 <S S S>),
                                which is 1 for a solenoidal field that is resolved and alias-free

and the distributions those moments compress -- integer counts from one read, exact and additive over ranks:

    histogram(u, range, nbins)  per component of a real field the `nbins` bins of [lo, hi) and the counts below, above and NaN
    gradient_pdf(A, x, y, range, bins)   the histogram of one of ss, ww, div, Q, R, sss, wsw, or the joint histogram of two of
                                them -- gradient_pdf(A, 'R', 'Q', ...) is the teardrop --, the quantities formed per point
                                without fused multiply-adds so that the counts equal a numpy restatement exactly
    pdf(counts, range), joint_pdf(counts, ranges, bins)   bin centres, the density and the shares outside the range

and the two-point statistics in physical space -- the structure functions S_p(r) = <(u(x + r e_a) - u(x))^p>, of which only
p = 2 can be had from the transforms: the exact laws a run is validated against (4/5, 4/3, Yaglom) and the exponents and
increment flatness by which intermittency is reported; every separation from ONE read of the field:

    structure_functions(u, axis, seps, lcomp)   per separation and component the sums of d, ..., d^6, |d|, |d|^3 and d_l d^2 of
                                the increments along a grid axis this rank holds whole (m <= 4 components, up to 64
                                separations, axis <= 4096): whole lines staged once in LDS, the separations looped over them;
                                bit for bit repeatable, added over the ranks in rank order
    log_separations(N, per_octave)   1, 2, 3, 4, 6, 8, 12, ... <= N // 2
    structure_moments(sf, npoints, axis)   S_1 ... S_6, <|d|>, <|d|^3>, increment skewness and flatness, the mixed moment, and
                                which component is longitudinal

and the fields where no grid point is -- tracer particles, probes, a line or a plane that is not a grid plane: B-spline
interpolation (van Hinsberg et al. 2012), whose coefficients cost a spectral code one pointwise pass:

    scale_axes(f_hat, v, out)   f_hat * (v0[i0] * v1[i1]) * v2[i2]: any separable spectral multiplier as three per-axis vectors (the
                                sparse form again), in place or not; every part one multiply, bit for bit a numpy restatement
    bspline_vectors(order)      the three vectors of the order-4 prefilter 1 / ((2 + cos(2 pi n / N)) / 3); order 2 needs none
    interpolate(c, x, order)    the order-2 (trilinear) or order-4 (cubic) interpolant of m <= 4 real fields at double positions
                                [P][3], periodic, positions anywhere: order^2 lanes gather a particle's stencil and add it in a
                                fixed order (bit for bit repeatable); each rank adds the stencil points it owns and `reduce=`
                                adds the ranks -- no halo, no particle migration; a position that is not finite gives NaN
    spread(q, x, order)         its transpose, particle to grid: factor * sum_p w(x_p) q_p on this rank's block, every
                                contribution rounded once to 64-bit fixed point and added by an integer atomic, so the field
                                does not depend on the order of the adds, of the particles or on the cut into ranks, and a
                                numpy restatement gives the same bits; no rank reduction: the blocks are disjoint

and the way into homogeneous isotropic turbulence, which all of the above describe -- a random-phase, divergence-free field
with a prescribed E(k) (Rogallo 1981) and white-in-time forcing in a band (Eswaran & Pope 1988), from a counter-based
generator keyed by the global mode index: one pointwise pass, independent of the cut into ranks, Hermitian by construction:

    random_solenoidal(out, seed, stream, amp)   independent complex Gaussian modes of amplitude amp[shell], projected normal
                                to K; the mirror mode is bit for bit the conjugate, the r2c field the stored half of the c2c
                                field, the fp32 field the fp64 field rounded once; Nyquist indices and the mean are zero
    scale_shells(f_hat, table)  f_hat * table[shell]: the isotropic counterpart of `scale_axes` (sharp and Gaussian filters)
    random_field(out, E, seed)  the two together: a field whose shell spectrum equals E to rounding; returns the table
    model_spectrum(k, kind, k_peak, u_rms)   k^4 exp(-2 (k / k_p)^2) or k^4 / (1 + (k / k_p)^2)^(17/6), sum E = 3 u_rms^2 / 2
    white_noise_force(u_hat, work, step, eps, dt, band, seed)   u_hat += f, a fresh random band field with sum |f|^2 / 2 =
                                eps dt: the mean injection rate is eps whatever the flow does

Fields are ``newDistArray(fft, rank=1)`` arrays ([3][local shape]); the wavenumbers are three
per-axis device vectors (the sparse form of get_local_wavenumbermesh, :52-63).
"""
import collections
import math

import numpy as np
import torch

from . import _lib
from .array import DeviceArray


def local_wavenumbers(fft, L=None):
    """Per-axis wavenumber vectors of this rank's block of the spectral array, scaled by
    2 pi / L (examples/spectral_dns_solver.py:52-63): [k0, k1, k2] as 1-D device arrays."""
    s = fft.local_slice(True)
    N = fft.global_shape()
    real = np.dtype(fft.dtype(False)).kind == 'f'
    k = [np.fft.fftfreq(n, 1. / n) for n in N]
    if real:
        k[-1] = np.fft.rfftfreq(N[-1], 1. / N[-1])
    L = np.full(len(N), 2 * np.pi) if L is None else np.asarray(L, dtype=float)
    rdt = np.dtype(fft.dtype(True).char.lower())
    dev = fft.forward.output_array.device
    return [torch.as_tensor((ki[si].astype(int) * (2 * np.pi / L[i])).astype(rdt), device=dev)
            for i, (ki, si) in enumerate(zip(k, s))]


def hermitian_weights(fft):
    """How often each entry of this rank's block of spectral axis 2 counts in a sum over the FULL spectrum, as a 1-D
    device array of the transform's real precision.  A real transform stores half of the last axis (the convention
    of `local_wavenumbers`): the columns global k2 = 0 and, for even N2, k2 = N2/2 are their own mirror images and count
    once, every other column stands for itself and its conjugate and counts twice.  Complex transforms: all ones."""
    s = fft.local_slice(True)[-1]
    n = int(fft.global_shape()[-1])
    real = np.dtype(fft.dtype(False)).kind == 'f'
    k2 = np.arange(int(fft.global_shape(True)[-1]))[s]
    w = np.ones(len(k2))
    if real:
        w[(k2 != 0) & (2 * k2 != n)] = 2
    rdt = np.dtype(fft.dtype(True).char.lower())
    return torch.as_tensor(w.astype(rdt), device=fft.forward.output_array.device)


DealiasMask = collections.namedtuple('DealiasMask', 'm0 m1 m2 kcut')
DealiasMask.__doc__ = """What `SpectralOps.dealias_mask` returns: per-axis uint8 device vectors over this rank's spectral block (non-zero =
keep; None = the whole axis) and the spherical cut |k| <= kcut (inf: none)."""


def _t(a):
    return a.tensor if isinstance(a, DeviceArray) else a


_REAL, _COMPLEX = (torch.float32, torch.float64), (torch.complex64, torch.complex128)


def _operands(kinds, *fields):
    """(tensors, precision) of the operands of one pointwise kernel: all of ONE dtype among `kinds` and contiguous, which is
    what the kernel takes for granted -- it indexes every operand as it indexes the first.  None stays None."""
    ts = [None if f is None else _t(f) for f in fields]
    given = [t for t in ts if t is not None]
    assert all(isinstance(t, torch.Tensor) for t in given), 'the operands are device arrays or tensors'
    dtype = given[0].dtype
    assert dtype in kinds, dtype
    assert all(t.dtype == dtype for t in given), 'the operands differ in dtype: %s' % [t.dtype for t in given]
    assert all(t.is_contiguous() for t in given), 'an operand is not contiguous'
    return ts, (8 if dtype in (torch.float64, torch.complex128) else 4)


QUANTITIES = {'ss': _lib.PS_Q_SS, 'ww': _lib.PS_Q_WW, 'div': _lib.PS_Q_DIV, 'Q': _lib.PS_Q_Q, 'R': _lib.PS_Q_R,
              'sss': _lib.PS_Q_SSS, 'wsw': _lib.PS_Q_WSW}          # the x / y of SpectralOps.gradient_pdf


def _ranges(rng, m):
    """m (lo, hi) pairs of floats from one pair or m of them; what gfft_ps_histogram refuses is refused here
    (plain Python floats: these run between a caller's launches)"""
    rng = tuple(rng)
    if len(rng) == 2 and np.ndim(rng[0]) == 0 and np.ndim(rng[1]) == 0:
        rng = (rng,) * m
    assert len(rng) == m and all(np.ndim(r) == 1 and len(r) == 2 for r in rng), 'range = (lo, hi) or %d such pairs' % m
    out = [(float(lo), float(hi)) for lo, hi in rng]
    assert all(math.isfinite(lo) and math.isfinite(hi) and lo < hi and math.isfinite(hi - lo) for lo, hi in out), 'a range must be finite with lo < hi'
    return out


def _nbins(n, most, *ranges):
    """a bin count 1 ... most whose width w = n / (hi - lo) is finite on every range given"""
    assert isinstance(n, (int, np.integer)) and not isinstance(n, bool) and 1 <= n <= most, 'bins = 1 ... %d' % most
    assert all(math.isfinite(float(n) / (hi - lo)) for lo, hi in ranges), 'bins / (hi - lo) overflows'
    return int(n)


class SpectralOps:
    """The kernels that need wavenumbers, bound to one PFFT's local spectral shape and wavenumbers."""
    def __init__(self, fft, L=None):
        assert len(fft.global_shape()) == 3, 'vector calculus kernels are 3-D'
        self.K = local_wavenumbers(fft, L)
        self.shape = tuple(int(n) for n in fft.shape(True))
        self.W = hermitian_weights(fft)
        self.comms = [c for c in fft.subcomm if c.Get_size() > 1]
        # shell width and count from GLOBAL quantities: the same on every rank
        unit = 2 * np.pi / (np.full(3, 2 * np.pi) if L is None else np.asarray(L, dtype=float))
        self.dk = float(unit.min())
        self.kmax = float(np.sqrt(sum((int(n) // 2 * d) ** 2 for n, d in zip(fft.global_shape(), unit))))
        # the physical side (stats): this rank's block and the grid's N_i / L_i
        self.pshape = tuple(int(n) for n in fft.shape(False))
        self.inv_dx = [float(n) / float(l) for n, l in zip(fft.global_shape(), np.full(3, 2 * np.pi) if L is None else np.asarray(L, dtype=float))]
        self._stats_dev = None
        self._force_spec = None
        # what dealias_mask needs of the transform: global sizes, this rank's slice of the spectral axes, the device
        self._N = tuple(int(n) for n in fft.global_shape())
        self._gshape = tuple(int(n) for n in fft.global_shape(True))
        self._slice = tuple(fft.local_slice(True))
        self._real = np.dtype(fft.dtype(False)).kind == 'f'
        # what interpolate needs: where this rank's physical block starts in the periodic grid N
        self.pstart = tuple(int(sl.start or 0) for sl in fft.local_slice(False))
        # where spread counts skipped particles for a caller who passes no counter (so that such a call allocates nothing)
        self._spread_skipped = torch.zeros(1, dtype=torch.int64, device=self.K[0].device)

    def scale_axes(self, f_hat, v, out=None):
        """out = f_hat * g with g = (v[0][i0] * v[1][i1]) * v[2][i2]: a separable spectral multiplier in one pass.  f_hat is the
        spectral shape or [m] + spectral shape, m <= 4, complex, contiguous, of the transform's precision; v is a triple of real
        device vectors of that precision over this rank's spectral axes, or None for an axis that contributes no factor (no
        multiply by 1 is issued); out defaults to f_hat itself (in place) and otherwise has its shape and overlaps nothing.
        g is formed in the field's precision and each part of each value is one multiply by it: bit for bit a numpy
        restatement.  `bspline_vectors(4)` is the prefilter of `interpolate`; any separable filter -- Gaussian, box -- is
        three vectors through the same call.  Returns out.  Nothing synchronises or allocates."""
        t, ncomp, precision = self._field(f_hat)
        assert ncomp <= 4, 'at most 4 components per call'
        assert len(v) == 3, 'v = three per-axis vectors (or None)'
        rdt = torch.float64 if precision == 8 else torch.float32
        for vi, n in zip(v, self.shape):
            assert vi is None or (isinstance(vi, torch.Tensor) and vi.dtype == rdt and tuple(vi.shape) == (n,) and
                                  vi.is_contiguous()), 'a vector is a real tensor of the field\'s precision over its local axis'
        if out is None:
            out = f_hat
        to, no, po = self._field(out)
        assert (no, po) == (ncomp, precision) and to.dim() == t.dim(), 'out and f_hat differ in shape or precision'
        _lib.engine().ps_scale_axes(t, to, ncomp, tuple(v), self.shape, precision)
        return out

    def _shell_table(self, table, device, nbins=None):
        """a per-shell table (numpy array, sequence or tensor) as a contiguous device double[nbins]"""
        if isinstance(table, torch.Tensor):
            assert table.dtype == torch.float64 and table.dim() == 1 and table.is_contiguous(), 'a shell table is a contiguous double vector'
            assert table.device == device, 'the table and the field live on different devices'
            t = table
        else:
            a = np.ascontiguousarray(np.asarray(table, dtype=np.float64))
            assert a.ndim == 1, 'a shell table is a vector'
            t = torch.as_tensor(a).to(device)
        assert t.numel() >= 1 and (nbins is None or t.numel() == nbins), 'the table has one entry per shell'
        return t

    def random_solenoidal(self, out, seed, stream=0, amp=None, nbins=None, dk=None, add=False, project=True):
        """Fills `out` (add=True: adds to it) with random Fourier modes that make a REAL physical field: independent complex
        Gaussians of amplitude amp[b] per shell b = floor(|k| / dk + 1/2), projected onto the plane normal to K (project=True:
        a divergence-free velocity, out = [3] + spectral shape; E sum_c |u_hat_c|^2 = 4 amp^2 per mode) or left as they are
        (project=False: the spectral shape or [m] + it, m <= 4; E |u_hat_c|^2 = 2 amp^2).  One pointwise kernel
        (gfft_ps_random_field, include/gfft.h): a counter-based generator (Philox4x32-10) keyed by the GLOBAL mode index,
        `seed` (below 2^64) and `stream` (below 2^62; a step number, say), so
          * the field does not depend on how the ranks cut the array -- a 2-rank and an 8-rank run start from the same bits;
          * u_hat(-k) is bit for bit conj u_hat(k), in a c2c layout everywhere and in an r2c layout on its two self-mirrored
            planes, and the r2c field is the stored half of the c2c field;
          * the same call gives the same bits, and the fp32 field is the fp64 field rounded once (for equal wavenumbers).
        Stored as +0 (add=True: left untouched): the mean mode, every mode with a Nyquist index on any axis (K is not odd
        there, as `gradient` and `curl` document), shells b >= nbins and shells with amp[b] == 0.  amp is a numpy array, a
        device double tensor or None (every amplitude 1); nbins defaults to len(amp), else to `default_nbins(dk)`.  Returns
        out.  With amp a tensor or None nothing synchronises or allocates, so the call can be captured."""
        t, ncomp, precision = self._field(out)
        assert ncomp <= 4, 'at most 4 components per call'
        assert not project or (ncomp == 3 and t.dim() == 4), 'the projection needs a [3] + spectral shape field'
        seed, stream = int(seed), int(stream)
        assert 0 <= seed < 1 << 64 and 0 <= stream < 1 << 62, 'seed is below 2^64 and stream below 2^62'
        dk = self.dk if dk is None else float(dk)
        assert dk > 0 and np.isfinite(dk)
        tamp = None if amp is None else self._shell_table(amp, t.device, nbins)
        nbins = int(tamp.numel()) if tamp is not None else self.default_nbins(dk) if nbins is None else int(nbins)
        assert nbins >= 1
        start = [int(sl.start or 0) for sl in self._slice]
        N = list(self._N)
        _lib.engine().ps_random_field(t, ncomp, self.shape, start, N, self.K, project, dk, tamp, nbins, seed, stream, add, precision)
        return out

    def scale_shells(self, f_hat, table, out=None, dk=None):
        """out = f_hat * table[b], b = floor(|k| / dk + 1/2) the shell `spectrum` bins by: the isotropic counterpart of
        `scale_axes` in one pass -- a sharp or Gaussian LES filter, a rescale to an exact spectrum.  f_hat is the spectral shape
        or [m] + it, m <= 4; table is a numpy array or a device double tensor with one entry per shell, converted to the
        field's precision on the device; each part of each value is one multiply, bit for bit a numpy restatement.  A mode
        whose shell lies beyond the table is stored as +0 whatever it held.  out defaults to f_hat (in place) and otherwise
        has its shape and overlaps nothing.  Returns out.  With a tensor table nothing synchronises or allocates."""
        t, ncomp, precision = self._field(f_hat)
        assert ncomp <= 4, 'at most 4 components per call'
        dk = self.dk if dk is None else float(dk)
        assert dk > 0 and np.isfinite(dk)
        tab = self._shell_table(table, t.device)
        if out is None:
            out = f_hat
        to, no, po = self._field(out)
        assert (no, po) == (ncomp, precision) and to.dim() == t.dim(), 'out and f_hat differ in shape or precision'
        _lib.engine().ps_scale_shells(t, to, ncomp, self.K, dk, tab, int(tab.numel()), self.shape, precision)
        return out

    def random_field(self, out, E, seed, stream=0, dk=None):
        """A random solenoidal velocity whose shell spectrum IS `E` (Rogallo 1981): `random_solenoidal` at unit amplitude over
        len(E) shells, its `spectrum` (added over the ranks, the same bits on every rank), the table sqrt(E[b] / E_have[b])
        (0 where a shell holds no mode), and `scale_shells` in place with that table.  The spectrum of the result equals E
        to rounding in every shell that holds a mode; E of an empty shell (shell 0, or one beyond the grid) is unreachable
        and ignored.  out = [3] + spectral shape.  Synchronises (the spectrum is read on the host).  Returns the table."""
        E = np.asarray(E, dtype=np.float64)
        assert E.ndim == 1 and len(E) >= 1 and np.isfinite(E).all() and (E >= 0).all(), 'E = a finite, non-negative value per shell'
        nbins = len(E)
        self.random_solenoidal(out, seed, stream, None, nbins, dk)
        have = self.spectrum(out, nbins=nbins, dk=dk)[0]
        with np.errstate(divide='ignore', invalid='ignore'):
            table = np.where(have == 0, 0.0, np.sqrt(E / have))
        self.scale_shells(out, table, dk=dk)
        return table

    def white_noise_force(self, u_hat, work, step, eps, dt, band, seed):
        """One step of white-in-time random forcing in the shells band = (blo, bhi) (Eswaran & Pope 1988, without the
        Ornstein-Uhlenbeck memory): u_hat += f with f a fresh random solenoidal field in the band -- `random_solenoidal(work,
        seed, stream=step)`, an indicator amplitude -- scaled so that sum w |f|^2 / 2 = eps dt exactly.  The energy grows by
        eps dt + <u . f>, and the cross term has zero mean because f is independent of u: the mean injection rate is eps
        whatever the flow does.  `work` has u_hat's shape and is overwritten with the unscaled f.  The scale comes from the
        rank-reduced `spectrum(work)` on the host, so the call synchronises; a device-resident factor, which a captured step
        would need, is out of scope here.  Returns the factor sqrt(eps dt / E_f) (0 where the band holds no mode)."""
        blo, bhi = int(band[0]), int(band[1])
        eps, dt = float(eps), float(dt)
        assert 0 <= blo <= bhi and np.isfinite(eps) and eps >= 0 and np.isfinite(dt) and dt >= 0
        amp = np.zeros(bhi + 1)
        amp[blo:] = 1.0
        self.random_solenoidal(work, seed, stream=step, amp=amp)
        ef = float(self.spectrum(work, nbins=bhi + 1)[0][blo:].sum())
        factor = math.sqrt(eps * dt / ef) if ef > 0 else 0.0
        rk_stage(None, None, u_hat, work, 0.0, factor)
        return factor

    def bspline_vectors(self, order=4):
        """The prefilter of B-spline interpolation of `order` as three vectors for `scale_axes`, over this rank's spectral block,
        in the transform's precision, computed on the host in double: for order 4 entry n (global integer wavenumber) of axis
        i is 1 / ((2 + cos(2 pi n / N_i)) / 3) -- the reciprocal of the cubic B-spline's Fourier symbol, which lies in [1/3, 1]
        and is never zero; 1 at n = 0, 3 at the Nyquist index of an even axis.  order 2: (None, None, None) -- linear
        interpolation needs no prefilter.  Allocates three small device vectors: build them once."""
        assert order in (2, 4), 'order = 2 or 4'
        if order == 2:
            return (None, None, None)
        n = [np.fft.fftfreq(N, 1. / N) for N in self._N]
        if self._real:
            n[-1] = np.fft.rfftfreq(self._N[-1], 1. / self._N[-1])
        rdt = np.float64 if self.K[0].dtype == torch.float64 else np.float32
        dev = self.K[0].device
        return tuple(torch.as_tensor((1.0 / ((2.0 + np.cos(2 * np.pi * ni[sl].astype(int) / float(N))) / 3.0)).astype(rdt), device=dev)
                     for ni, N, sl in zip(n, self._N, self._slice))

    def interpolate(self, c, x, order=4, out=None, reduce=True):
        """The order-2 (trilinear) or order-4 (cubic B-spline) interpolant of real fields at particle positions: double [P][m],
        or [P] for a scalar field.  c is a contiguous real tensor or DistArray of shape fft.shape(False) or [m] + that shape,
        m <= 4, in the transform's precision; x is a contiguous double device tensor [P][3], THE SAME ON EVERY RANK (particles
        are replicated), in the units of L; positions need not lie in the box (the grid is periodic) and a NaN, an infinity
        or an |x| beyond 2^51 cells gives a NaN row.  For order 4, c must hold B-spline coefficients: the backward transform of
        `scale_axes(f_hat, bspline_vectors(4))`; order 2 reads the samples themselves.  The definition, operation by
        operation, is in include/gfft.h (gfft_ps_interp); values are converted to double first and summed in a fixed order:
        the result repeats bit for bit.

        Each rank adds the stencil points its block owns.  reduce=True adds the ranks' partial results on the host in rank
        order, one grid axis after the other (as `stats` does), so every rank holds identical bits; this synchronises and
        moves 8 P m bytes per rank through the host: priced for diagnostics and moderate P.  reduce=False only enqueues
        and returns the device tensor (`out`, a contiguous double tensor of the shape above, or a new one): on one rank the
        complete result, and with `out=` given capturable into a graph."""
        t, ncomp, precision = self._real_field(c)
        assert ncomp <= 4, 'at most 4 components per call'
        assert order in (2, 4), 'order = 2 or 4'
        assert isinstance(x, torch.Tensor) and x.dtype == torch.float64 and x.dim() == 2 and x.shape[1] == 3 and x.is_contiguous(), \
            'x is a contiguous double tensor [P][3]'
        assert x.device == t.device, 'x and the field live on different devices'
        P = int(x.shape[0])
        shape = (P,) if t.dim() == 3 else (P, ncomp)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=t.device)
        assert isinstance(out, torch.Tensor) and tuple(out.shape) == shape and out.dtype == torch.float64 and out.is_contiguous(), \
            (tuple(out.shape), shape)
        if min(self.pshape) == 0:                      # a rank without a block owns no stencil point
            out.zero_()
        else:
            _lib.engine().ps_interp(t, ncomp, self.pshape, self.pstart, self._N, self.inv_dx, x, P, order, out, precision)
        if not reduce:
            return out
        vals = out.cpu().numpy()                       # (waits for the kernel)
        _lib.check_async()
        for cm in self.comms:                          # one grid axis after the other: the same order on every rank
            parts = cm.allgather_obj(vals)
            vals = parts[0].copy()
            for p in parts[1:]:
                vals = vals + p
        return vals

    @staticmethod
    def spread_scale_exp(q):
        """The default `scale_exp` of `spread`: with S = max_c sum_p |q[p][c]| over the finite entries (one torch reduction; it
        synchronises), floor(log2(2^62 / S)) clamped to +-1000, and 0 for S = 0 -- the largest power of two at which no
        accumulator can leave int64, whatever the positions are."""
        a = q.abs()
        a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
        S = float(a.reshape(a.shape[0], -1).sum(dim=0).max()) if a.numel() else 0.0
        if S == 0.0:
            return 0
        if not math.isfinite(S):                       # (finite entries whose sum overflows)
            return -1000
        f, k = math.frexp(S)                           # S = f 2^k, 0.5 <= f < 1: floor(62 - k - log2 f), exactly
        return max(-1000, min(1000, 62 - k + (1 if f == 0.5 else 0)))

    def spread(self, q, x, order=4, out=None, scale_exp=None, factor=1.0, acc=None, skipped=None):
        """Particle to grid, the transpose of `interpolate`: out = this rank's block of factor * sum_p w(x_p) q_p with the
        order-2 (trilinear) or order-4 (cubic B-spline) weights of `interpolate`.  q is a contiguous double device tensor
        [P][m], m <= 4, or [P] for a scalar; x a contiguous double device tensor [P][3] as in `interpolate`; x and q are THE
        SAME ON EVERY RANK (particles are replicated).  out is a real tensor or DistArray of shape fft.shape(False) or [m] +
        that shape in the transform's precision (default: a new tensor); it is OVERWRITTEN.  Returns out.  There is no rank
        reduction: each rank deposits on the stencil points its block owns, the blocks are disjoint, and the distributed
        field is complete without a halo exchange.  A rank without a block zero-fills out and launches nothing.

        The sum is EXACT in the sense that matters for repeatability: each contribution w q 2^scale_exp is rounded once to a
        64-bit integer and added by an integer atomic (the definition, operation by operation: include/gfft.h,
        gfft_ps_spread), so the result does not depend on the order of the adds, on the order of the particles or on the
        number of ranks, and a numpy restatement reproduces it bit for bit.  acc is the int64 workspace [m] + the local
        physical shape (default: allocated and zeroed here); a caller's acc is ADDED TO and then cleared, so it is zeroed
        once by its owner and comes back zero.  The wrapper passes the one host quotient factor / 2^scale_exp to
        gfft_ps_spread_finish, which converts, multiplies and narrows once.

        scale_exp=None takes `spread_scale_exp(q)` (one reduction; it synchronises): weights are non-negative and sum to
        one, so no accumulator can leave int64, and a single contribution among 2^20 equal ones is resolved to about 2^-42
        of itself.  (A lone particle that carries all of a power-of-two S lands ON the 2^62 guard and is skipped: pass
        scale_exp one lower.)  A particle whose position is not finite or beyond 2^51 cells, or one of whose q 2^scale_exp is
        not finite or reaches 2^62, deposits nothing for any component; `skipped` (int64 [1], ADDED TO) counts them, the
        same on every rank that owns a block.  With scale_exp, acc and out all given nothing synchronises or allocates and the
        call can be captured into a graph.

        The adjoint chain: scale_axes(fft.forward(spread(q, x, 4)), bspline_vectors(4)) is the exact transpose of
        interpolate(fft.backward(scale_axes(f_hat, bspline_vectors(4))), x, 4) -- the type-1 / type-2 pair of a non-uniform
        transform, `scale_axes` being the deconvolution."""
        assert order in (2, 4), 'order = 2 or 4'
        assert isinstance(q, torch.Tensor) and q.dtype == torch.float64 and q.dim() in (1, 2) and q.is_contiguous(), \
            'q is a contiguous double tensor [P][m] or [P]'
        m = 1 if q.dim() == 1 else int(q.shape[1])
        assert 1 <= m <= 4, 'at most 4 components per call'
        P = int(q.shape[0])
        assert isinstance(x, torch.Tensor) and x.dtype == torch.float64 and tuple(x.shape) == (P, 3) and x.is_contiguous(), \
            'x is a contiguous double tensor [P][3], one row per row of q'
        assert x.device == q.device, 'x and q live on different devices'
        factor = float(factor)
        assert math.isfinite(factor), 'factor must be finite'
        rdt = self.K[0].dtype
        if out is None:
            out = torch.empty(self.pshape if q.dim() == 1 else (m,) + self.pshape, dtype=rdt, device=q.device)
        to, mo, precision = self._real_field(out)
        assert mo == m, 'out holds %d components, q %d' % (mo, m)
        assert to.device == q.device, 'out and q live on different devices'
        if acc is not None:
            assert isinstance(acc, torch.Tensor) and acc.dtype == torch.int64 and tuple(acc.shape) == (m,) + self.pshape and \
                acc.is_contiguous() and acc.device == q.device, 'acc is a contiguous int64 tensor [m] + the local physical shape'
        if skipped is not None:
            assert isinstance(skipped, torch.Tensor) and skipped.dtype == torch.int64 and tuple(skipped.shape) == (1,) and \
                skipped.device == q.device, 'skipped is an int64 tensor [1]'
        if scale_exp is None:
            scale_exp = self.spread_scale_exp(q)
        assert isinstance(scale_exp, (int, np.integer)) and not isinstance(scale_exp, bool) and abs(int(scale_exp)) <= 1000, \
            'scale_exp is an integer, |scale_exp| <= 1000'
        scale_exp = int(scale_exp)
        if min(self.pshape) == 0:                      # a rank without a block owns no stencil point
            to.zero_()
            return out
        if acc is None:
            acc = torch.zeros((m,) + self.pshape, dtype=torch.int64, device=q.device)
        eng = _lib.engine()
        eng.ps_spread(acc, m, self.pshape, self.pstart, self._N, self.inv_dx, x, q, P, order, scale_exp,
                      self._spread_skipped if skipped is None else skipped)
        eng.ps_spread_finish(to, acc, acc.numel(), factor / math.ldexp(1.0, scale_exp), True, precision)
        return out

    def _same_precision(self, precision):
        # the kernels read K (and W) in the field's precision: a field of the other one would get garbage wavenumbers
        assert precision == (8 if self.K[0].dtype == torch.float64 else 4), 'field and transform differ in precision'

    def curl(self, u_hat, out):
        """out = 1j * (K x u_hat); both [3] + spectral shape, complex, contiguous, of the transform's precision; out overlaps
        nothing.  K is applied as given.  Returns out."""
        assert tuple(u_hat.shape) == (3,) + self.shape == tuple(out.shape)
        (tu, to), precision = _operands(_COMPLEX, u_hat, out)
        self._same_precision(precision)
        _lib.engine().ps_curl(tu, to, self.K, self.shape, precision)
        return out

    def gradient(self, f_hat, out):
        """out[c][j] = 1j * K[j] * f_hat[c]: the spectral gradient of m <= 4 fields in one pass.  f_hat is [m] + spectral shape
        and out [m][3] + spectral shape (for m = 3 the layout of newDistArray(fft, rank=2): out[i][j] transforms back to
        A_ij = d u_i / d x_j), or, a scalar field, the spectral shape and [3] + spectral shape; contiguous, complex, of the
        transform's precision, out overlapping nothing.  Each part of each value is one multiply: the correctly rounded
        product, bit for bit.  K is applied as given (the convention of `curl`): a Nyquist column is not treated specially;
        the 2/3 mask removes it.  Returns out.  Nothing synchronises or allocates."""
        t, ncomp, precision = self._field(f_hat)
        assert ncomp <= 4, 'at most 4 components per call'
        to = _t(out)
        assert tuple(to.shape) == tuple(t.shape[:-3]) + (3,) + self.shape, (tuple(to.shape), tuple(t.shape))
        assert to.is_contiguous(), 'out is not contiguous'
        to, no, po = self._field(to.view((3 * ncomp,) + self.shape))
        assert (no, po) == (3 * ncomp, precision), 'out and f_hat differ in precision'
        _lib.engine().ps_gradient(t, to, ncomp, self.K, self.shape, precision)
        return out

    def gradient_stats(self, A, out=None, reduce=True):
        """Statistics of the velocity-gradient tensor in one read: float64 [20], indexed by `_lib.GS_*`,
            [0] max S_ij S_ij   [1] max |w|^2   [2] max |div u|          (S = (A + A^T) / 2, w = curl u, div u = tr A)
            [3] sum div^2   [4] sum S_ij S_ij   [5] sum |w|^2   [6] sum (S_ij S_ij)^2   [7] sum |w|^4   [8] sum S_ij S_ij |w|^2
            [9] sum Q   [10] sum R   [11] sum Q^2   [12] sum R^2         (Q = ((tr A)^2 - tr A^2) / 2, R = -det A)
            [13] sum S_ij S_jk S_ki   [14] sum w_i S_ij w_j
            [15 ... 17] sum_i A_ii^2, A_ii^3, A_ii^4   [18], [19] sum_{i != j} A_ij^2, A_ij^4
        (`gradient_moments` reads them; include/gfft.h has the exact expressions).  A is a contiguous real tensor or DistArray
        of shape [3][3] + fft.shape(False) in the transform's precision, A[i][j] = d u_i / d x_j: the nine backward transforms
        of `gradient(u_hat, .)`.  Every value is converted to double first.  A NaN in A[i][j] makes every sum that reads it NaN;
        the maxima follow fmax and skip it.

        `reduce` and `out` as in `stats`: reduce=True combines over the ranks of the grid on the host (entries 0 - 2 with
        np.maximum, the rest added in rank order, one grid axis after the other, so every rank holds identical bits), which
        synchronises; reduce=False only enqueues and returns the device tensor (`out`, a contiguous double tensor of 20
        entries, or a new one), so it can be captured after one call outside the capture.  The result repeats bit for bit from
        one call to the next."""
        t = _t(A)
        assert tuple(t.shape) == (3, 3) + self.pshape, (tuple(t.shape), self.pshape)
        assert t.is_contiguous() and t.dtype in (torch.float32, torch.float64), 'gradient_stats needs a contiguous real tensor'
        precision = 8 if t.dtype == torch.float64 else 4
        self._same_precision(precision)
        if out is None:
            out = torch.empty(_lib.PS_GRAD_NVAL, dtype=torch.float64, device=t.device)
        assert tuple(out.shape) == (_lib.PS_GRAD_NVAL,) and out.dtype == torch.float64 and out.is_contiguous()
        count = int(np.prod(self.pshape, dtype=np.int64))
        _lib.engine().ps_gradient_stats(t, count, out, precision)
        return self._reduce_gradient_stats(out) if reduce else out

    def _reduce_gradient_stats(self, out):
        """`_reduce_stats` for the layout of gradient_stats: maxima first, then sums"""
        vals = out.cpu().numpy()                       # (waits for the kernels)
        _lib.check_async()
        is_max = np.arange(len(vals)) < _lib.PS_GRAD_NMAX
        for c in self.comms:                           # one grid axis after the other: the same order on every rank
            parts = c.allgather_obj(vals)
            vals = parts[0].copy()
            for p in parts[1:]:
                vals = np.where(is_max, np.maximum(vals, p), vals + p)
        return vals

    def histogram(self, u, range, nbins, out=None, reduce=True):
        """Histograms of a real physical-space field in one read: int64 [m][nbins + 3] ([nbins + 3] for a scalar field) --
        per component the `nbins` bins of [lo, hi), then the counts below, above (hi itself included: the upper edge is
        exclusive) and NaN; every component adds up to the number of points.  u as for `stats`: [m] + fft.shape(False), m <= 4,
        or a scalar field of that shape; `range` is one (lo, hi) for all components or m pairs; nbins <= 4096.
        The bin rule (include/gfft.h), in double: t = (x - lo) * w with w = nbins / (hi - lo); bin int(t) for 0 <= t < nbins.
        Counts are exact: independent of order, the same from call to call and on any split over ranks.

        `reduce` and `out` as in `stats`: reduce=True adds the counts over the ranks of the grid on the host, one grid axis
        after the other (exact; every rank holds the same array), which synchronises; reduce=False only enqueues and returns
        the device tensor (`out`, a contiguous int64 tensor of the shape above, or a new one), so it can be captured after one
        call outside the capture.  `pdf(counts, range)` turns a row into a density.
        Pooled PDFs need no kernel of their own: the longitudinal-derivative PDF is histogram(A[i][i]) for i = 0, 1, 2 added,
        the transverse one the six off-diagonal slices added (A[i] is a [3] + shape field: one call per row, three ranges
        alike)."""
        t, ncomp, precision = self._real_field(u)
        assert ncomp <= 4, 'at most 4 components per call'
        ranges = _ranges(range, ncomp)
        nbins = _nbins(nbins, _lib.PS_PDF_MAX_BINS, *ranges)
        shape = (nbins + _lib.PS_PDF_TAIL,) if t.dim() == 3 else (ncomp, nbins + _lib.PS_PDF_TAIL)
        out = self._counts_out(out, shape, t.device)
        count = int(np.prod(self.pshape, dtype=np.int64))
        _lib.engine().ps_histogram(t, ncomp, count, [r[0] for r in ranges], [r[1] for r in ranges], nbins, out, precision)
        return self._reduce_counts(out) if reduce else out

    def gradient_pdf(self, A, x, y=None, range=None, bins=None, out=None, reduce=True):
        """The histogram of one, or the joint histogram of two, of the per-point quantities of `gradient_stats` in one read of
        A ([3][3] + fft.shape(False), as for `gradient_stats`): x and y among 'ss', 'ww', 'div', 'Q', 'R', 'sss', 'wsw'
        (S_ij S_ij, |w|^2, tr A, the invariants Q and R, S_ij S_jk S_ki, w_i S_ij w_j), evaluated in double with every
        operation rounded on its own (no fused multiply-add), so the counts equal a numpy restatement exactly.
        y=None: `range` = (lo, hi), `bins` an int <= 4096; int64 [bins + 3] laid out as one row of `histogram`.
        Otherwise `range` = ((xlo, xhi), (ylo, yhi)), `bins` an int (both axes) or a pair with nbx * nby <= 16384; int64
        [nbx * nby + 2]: bin bx * nby + by, then the points outside (either coordinate below or above its range), then those
        where either quantity is NaN (which wins over outside); `joint_pdf` reshapes and normalises it.  The bin rule, `reduce`
        and `out` are those of `histogram`.  gradient_pdf(A, 'R', 'Q', ...) is the teardrop."""
        t = _t(A)
        assert tuple(t.shape) == (3, 3) + self.pshape, (tuple(t.shape), self.pshape)
        assert t.is_contiguous() and t.dtype in (torch.float32, torch.float64), 'gradient_pdf needs a contiguous real tensor'
        precision = 8 if t.dtype == torch.float64 else 4
        self._same_precision(precision)
        assert x in QUANTITIES and (y is None or y in QUANTITIES), (x, y)
        assert range is not None and bins is not None, 'gradient_pdf needs range= and bins='
        if y is None:
            (xr,) = _ranges(range, 1)
            nbx, nby, qy, yr = _nbins(bins, _lib.PS_PDF_MAX_BINS, xr), 1, _lib.PS_Q_NONE, (0.0, 1.0)
            shape = (nbx + _lib.PS_PDF_TAIL,)
        else:
            assert len(range) == 2 and all(np.ndim(r) == 1 for r in range), 'range = ((xlo, xhi), (ylo, yhi))'
            xr, yr = _ranges(range, 2)
            assert np.ndim(bins) == 0 or len(bins) == 2, 'bins = an int or (nbx, nby)'
            bx, by = (bins, bins) if np.ndim(bins) == 0 else bins
            nbx, nby = _nbins(bx, _lib.PS_PDF_MAX_JOINT, xr), _nbins(by, _lib.PS_PDF_MAX_JOINT, yr)
            assert nbx * nby <= _lib.PS_PDF_MAX_JOINT, 'at most 16384 joint bins'
            qy = QUANTITIES[y]
            shape = (nbx * nby + 2,)
        out = self._counts_out(out, shape, t.device)
        count = int(np.prod(self.pshape, dtype=np.int64))
        _lib.engine().ps_gradient_pdf(t, count, QUANTITIES[x], xr, nbx, qy, yr, nby, out, precision)
        return self._reduce_counts(out) if reduce else out

    @staticmethod
    def _counts_out(out, shape, device):
        if out is None:
            out = torch.empty(shape, dtype=torch.int64, device=device)
        assert tuple(out.shape) == tuple(shape) and out.dtype == torch.int64 and out.is_contiguous(), (tuple(out.shape), shape)
        return out

    def _reduce_counts(self, out):
        """This rank's counts added over the ranks of the grid, on the host: exact, the same array on every rank"""
        counts = out.cpu().numpy()                     # (waits for the kernels)
        _lib.check_async()
        for c in self.comms:                           # one grid axis after the other
            counts = np.sum(c.allgather_obj(counts), axis=0, dtype=np.int64)
        return counts

    def dealias_mask(self, rule='2/3', kcut=None):
        """The kept set of `project(..., dealias=)` and `dealias` as a `DealiasMask` (m0, m1, m2, kcut): a mode is kept iff
        m0[i0] and m1[i1] and m2[i2] and |k| <= kcut.
        rule='2/3': global integer wavenumber n_i is kept iff 3 * |n_i| < N_i -- strictly: |n| <= 21 of N = 64, 15 of 48, 6 of
        21, never the Nyquist plane; with the looser |n| < 2/3 (N/2 + 1) the quadratic term keeps an O(1) aliasing error.
        Built from the fftfreq / rfftfreq integers and sliced by fft.local_slice(True), exactly as `local_wavenumbers`
        slices K.  rule=None: every axis whole (no vectors).  Or a sequence of three boolean arrays of the GLOBAL spectral
        axis lengths (None for a whole axis), sliced the same way.  kcut=None: no spherical cut.
        Allocates three small device vectors: build the mask once, outside anything that is captured."""
        kcut = np.inf if kcut is None else float(kcut)
        assert kcut >= 0, kcut
        if rule is None:
            return DealiasMask(None, None, None, kcut)
        if isinstance(rule, str):
            assert rule == '2/3', rule
            n = [np.fft.fftfreq(N, 1. / N) for N in self._N]
            if self._real:
                n[-1] = np.fft.rfftfreq(self._N[-1], 1. / self._N[-1])
            rule = [3 * np.abs(ni.astype(int)) < N for ni, N in zip(n, self._N)]
        assert len(rule) == 3, 'rule = three per-axis boolean arrays'
        dev = self.K[0].device
        m = []
        for r, g, sl in zip(rule, self._gshape, self._slice):
            if r is not None:
                r = np.asarray(r)
                assert r.shape == (g,), (r.shape, g)
                r = torch.as_tensor(np.ascontiguousarray(r[sl] != 0).astype(np.uint8), device=dev)
            m.append(r)
        return DealiasMask(m[0], m[1], m[2], kcut)

    def _mask(self, dealias):
        """((m0, m1, m2), kcut) of a `dealias=` argument, checked against this block"""
        assert len(dealias) == 4, 'dealias = (m0, m1, m2, kcut): see dealias_mask'
        m, kcut = tuple(dealias[:3]), dealias[3]
        kcut = np.inf if kcut is None else float(kcut)
        assert kcut >= 0, kcut
        for mi, n in zip(m, self.shape):
            assert mi is None or (isinstance(mi, torch.Tensor) and mi.dtype in (torch.uint8, torch.bool) and
                                  tuple(mi.shape) == (n,) and mi.is_contiguous()), 'a mask vector is a uint8 tensor over its local axis'
        return m, kcut

    def project(self, du_hat, u_hat, nu, force=None, dealias=None):
        """In place: pressure projection and viscous term of the Navier-Stokes right-hand side.
        force=(gain, (blo, bhi)) or (gain, (blo, bhi), dk): the same pass then adds gain * u_hat to du_hat in every mode
        whose shell floor(|k| / dk + 1/2) (the shells of `spectrum`; dk defaults as there) lies in blo..bhi -- linear band
        forcing, after the projection and the viscous term, not projected (solenoidal where u_hat is).  gain is a float
        or a device double tensor (contiguous, at least one element: `forcing_gain(out=)` writes one) whose element 0 the
        kernel reads when it runs; both are rounded to the field's precision once and give the same bits.  Outside the
        band the result is bit for bit that of force=None.
        dealias=a `dealias_mask()` (or any (m0, m1, m2, kcut)): the same pass also truncates -- a kept mode gets bit for bit
        the result without `dealias`, forced or not; a truncated mode becomes +0 whatever du_hat and u_hat hold there, and
        nothing of it is loaded.  du_hat and u_hat are complex, contiguous, of one dtype -- the transform's precision -- and
        do not overlap.  Nothing synchronises or allocates."""
        assert tuple(du_hat.shape) == (3,) + self.shape == tuple(u_hat.shape)
        (tdu, tu), precision = _operands(_COMPLEX, du_hat, u_hat)
        self._same_precision(precision)
        fargs = None if force is None else self._force(force)
        if dealias is not None:
            m, kcut = self._mask(dealias)
            _lib.engine().ps_project_dealiased(tdu, tu, self.K, m, self.shape, nu, kcut, fargs, precision)
        elif fargs is None:
            _lib.engine().ps_project(tdu, tu, self.K, self.shape, nu, precision)
        else:
            dk, blo, bhi, gain, tgain = fargs
            _lib.engine().ps_project_forced(tdu, tu, self.K, self.shape, nu, dk, blo, bhi, gain, tgain, precision)
        return du_hat

    def _force(self, force):
        """(dk, blo, bhi, gain, tgain) of a `force=` argument: tgain the device tensor that holds the gain, or None"""
        assert len(force) in (2, 3), 'force = (gain, (blo, bhi)) or (gain, (blo, bhi), dk)'
        gain, (blo, bhi) = force[0], force[1]
        dk = self.dk if len(force) == 2 or force[2] is None else float(force[2])
        assert dk > 0 and 0 <= int(blo) <= int(bhi)
        tgain = None
        if isinstance(gain, (torch.Tensor, DeviceArray)):
            tgain, gain = _t(gain), 0.0
            assert tgain.dtype == torch.float64 and tgain.numel() >= 1 and tgain.is_contiguous()
        else:
            assert np.isfinite(gain), gain
        return dk, int(blo), int(bhi), float(gain), tgain

    def dealias(self, field, mask):
        """In place: +0 to every mode of `field` ([m] + spectral shape or, a scalar field, the spectral shape) that `mask` (a
        `dealias_mask()`) does not keep; returns `field`.  Kept modes are neither read nor written: whatever they hold
        stays.  One kernel of stores; nothing synchronises or allocates."""
        t, ncomp, precision = self._field(field)
        m, kcut = self._mask(mask)
        _lib.engine().ps_dealias(t, ncomp, self.K, m, self.shape, kcut, precision)
        return field

    def scalar_rhs(self, dtheta_hat, flux_hat, theta_hat, kappa, mean_gradient=None, u_hat=None, dealias=None):
        """The right-hand side of m <= 4 passive scalars in flux form, one pass:
            dtheta_hat[s] = -1j * (K . flux_hat[s]) - kappa[s] * |K|^2 * theta_hat[s] - mean_gradient[s] . u_hat
        theta_hat and dtheta_hat are [m] + spectral shape or, one scalar, the spectral shape; flux_hat is the transform of
        `scalar_flux`'s output, [m][3] + spectral shape (or [3] + spectral shape).  kappa is a float or m floats, finite and
        >= 0.  mean_gradient is three floats shared by all scalars or m x 3 floats and requires u_hat ([3] + spectral
        shape); without it u_hat, if given, is not read.  dealias as in `project`: a kept mode gets bit for bit the result
        without it, a truncated mode becomes +0 and nothing of it is loaded.  dtheta_hat must not overlap an input.
        Returns dtheta_hat.  Nothing synchronises or allocates."""
        tth, ns, precision = self._field(theta_hat)
        td, nd, pd = self._field(dtheta_hat)
        assert ns <= 4, 'at most 4 scalars per call'
        assert (nd, pd) == (ns, precision) and td.dim() == tth.dim(), 'dtheta_hat and theta_hat differ in shape or precision'
        tf = _t(flux_hat)
        assert tuple(tf.shape) == tuple(tth.shape[:-3]) + (3,) + self.shape, (tuple(tf.shape), tuple(tth.shape))
        assert tf.is_contiguous(), 'flux_hat is not contiguous'
        tf, nf, pf = self._field(tf.view((3 * ns,) + self.shape))
        assert (nf, pf) == (3 * ns, precision), 'flux_hat and theta_hat differ in precision'
        kap = np.asarray(kappa, dtype=np.float64)
        kap = np.full(ns, float(kap)) if kap.ndim == 0 else kap
        assert kap.shape == (ns,) and np.isfinite(kap).all() and (kap >= 0).all(), kappa
        tu = grad = None
        if u_hat is not None:
            tu, nu_, pu = self._field(u_hat)
            assert (nu_, pu) == (3, precision) and tu.dim() == 4, 'u_hat is a three-component field of the same precision'
        if mean_gradient is not None:
            assert tu is not None, 'a mean gradient needs u_hat'
            grad = np.asarray(mean_gradient, dtype=np.float64)
            grad = np.tile(grad, (ns, 1)) if grad.shape == (3,) else grad
            assert grad.shape == (ns, 3) and np.isfinite(grad).all(), mean_gradient
        m, kcut = ((None, None, None), np.inf) if dealias is None else self._mask(dealias)
        _lib.engine().ps_scalar_rhs(td, tf, tth, tu, ns, kap, grad, self.K, m, self.shape, kcut, precision)
        return dtheta_hat

    def rk_stage_if(self, u, u0, u1, du, nu, cb, ca, powers, h=None, dt=None):
        """One Runge-Kutta stage with the integrating factor of the linear term -nu |K|^2 u, one pass over the four fields:
            u  = E^q0 * u0 + cb * h * E^qd * du        (skipped when u is None; u0 may then be None too)
            u1 = E^q1 * u1 + ca * h * E^qa * du
        with E = exp(-nu |K|^2 h / 2) per mode and powers = (q0, qd, q1, qa), each 0, 1 or 2 (E^2 is E * E, E^0 the constant
        1); `IFRK4` holds the four rows of the classical scheme.  The fields are [m] + spectral shape, m <= 4, or, a scalar
        field, the spectral shape; nu is a float or m floats, finite and >= 0 (all equal: one exp per mode).  Exactly one of
        h (a float) and dt (a device double tensor whose element 0 the kernel reads when it runs: `timestep(out=)` writes
        one) gives the step; both give the same bits for the same double.  With nu = 0 the result is bit for bit that of
        `rk_stage(u, u0, u1, du, cb * h, ca * h)`.  Returns u1.  Nothing synchronises or allocates."""
        t1, ncomp, precision = self._field(u1)
        td, nd, pd = self._field(du)
        assert ncomp <= 4, 'at most 4 components per call'
        assert (nd, pd) == (ncomp, precision) and td.dim() == t1.dim(), 'du and u1 differ in shape or precision'
        assert u is None or u0 is not None, 'u needs u0'
        both = []
        for f in (u, u0):
            t = None
            if f is not None:
                t, nf, pf = self._field(f)
                assert (nf, pf) == (ncomp, precision) and t.dim() == t1.dim(), 'the fields differ in shape or precision'
            both.append(t)
        tu, tu0 = both
        v = np.asarray(nu, dtype=np.float64)
        v = np.full(ncomp, float(v)) if v.ndim == 0 else v
        assert v.shape == (ncomp,) and np.isfinite(v).all() and (v >= 0).all(), nu
        powers = tuple(powers)
        assert len(powers) == 4 and all(int(q) == q and 0 <= q <= 2 for q in powers), powers
        assert (h is None) != (dt is None), 'exactly one of h and dt'
        tdt = None
        if dt is not None:
            tdt, h = _t(dt), 0.0
            assert tdt.dtype == torch.float64 and tdt.numel() >= 1 and tdt.is_contiguous()
        else:
            assert np.isfinite(h), h
        _lib.engine().ps_rk_stage_if(tu, tu0, t1, td, ncomp, v, self.K, self.shape, cb, ca, powers, float(h), tdt, precision)
        return u1

    def forcing_gain(self, u_hat, eps, band, gain_max=np.inf, dk=None, out=None):
        """The gain g of the band forcing f_hat = g u_hat (`project(..., force=(g, band))`) that injects energy at the rate
        eps: g = min(eps / (2 E_f), gain_max) with E_f = sum of E(k) over shells band = (blo, bhi) of `spectrum(u_hat)`,
        0 where E_f is zero or not finite; the injected power sum w Re(conj(u_hat) . g u_hat) = 2 g E_f is eps unless
        the clamp binds.
        out=None: on any grid, from the rank-reduced `spectrum(u_hat, nbins=bhi + 1, dk=dk)` (every rank holds the same
        bits) and `force_gain`; synchronises and returns (gain, E_f) as Python floats.
        out = a device double[2] tensor: one-rank grids only (no device-side reduction over ranks); enqueues the spectrum
        into a tensor this object keeps and then `gfft_ps_force_gain`, which writes the gain to out[0] and E_f to out[1];
        returns `out`.  Nothing synchronises or, after the first call with a band, allocates, so the call can be captured
        with the `project(..., force=(out, band))` calls that read the gain."""
        blo, bhi = int(band[0]), int(band[1])
        eps, gain_max = float(eps), float(gain_max)
        assert 0 <= blo <= bhi and np.isfinite(eps) and eps >= 0 and gain_max > 0
        if out is None:
            E = self.spectrum(u_hat, nbins=bhi + 1, dk=dk)
            return force_gain(E, (blo, bhi), eps, gain_max)
        assert not self.comms, 'the device path of forcing_gain needs a one-rank grid'
        assert tuple(out.shape) == (2,) and out.dtype == torch.float64 and out.is_contiguous()
        t = _t(u_hat)
        if self._force_spec is None or self._force_spec.device != t.device or self._force_spec.shape[1] != bhi + 1:
            self._force_spec = torch.empty((2, bhi + 1), dtype=torch.float64, device=t.device)
        self.spectrum(t, nbins=bhi + 1, dk=dk, out=self._force_spec, reduce=False)
        _lib.engine().ps_force_gain(self._force_spec, bhi + 1, blo, bhi, eps, gain_max, out)
        return out

    def default_nbins(self, dk=None):
        """Shells of width dk that hold every mode: floor(kmax / dk + 1/2) + 1 with the global largest |k|."""
        return int(np.floor(self.kmax / (self.dk if dk is None else dk) + 0.5)) + 1

    def shells(self, nbins, dk=None):
        """Centre of each shell: arange(nbins) * dk (shell b holds |k| in [(b - 1/2) dk, (b + 1/2) dk))."""
        return np.arange(nbins) * (self.dk if dk is None else dk)

    def spectrum(self, u_hat, nbins=None, dk=None, out=None, reduce=True):
        """Shell spectrum of a forward-normalised field: float64 [2][nbins],
            [0][b] = sum over shell b of 0.5 * w * sum_c |u_hat_c|^2        (E(k); sums to <u.u>/2)
            [1][b] = the same with each mode times |k|^2                     (sums to <|grad u|^2>/2)
        with b = floor(|k| / dk + 1/2) and w the `hermitian_weights`; modes with b >= nbins are dropped.  u_hat is
        [m] + spectral shape or, a scalar field, the spectral shape.  dk defaults to the smallest 2 pi / L_i, nbins to
        `default_nbins(dk)` (nothing dropped).  One kernel, one read of u_hat, no array-sized temporaries.

        reduce=True: the bins are added over the ranks of the PFFT's grid (allgather_obj, in rank order, so every rank
        holds bit-identical bins) and returned as a numpy array -- which SYNCHRONISES the stream and copies 16 nbins
        bytes to the host.  reduce=False: only this rank's kernel is enqueued, its device tensor (`out`, a contiguous
        double tensor of shape [2, nbins], or a new one) is returned; with `out=` given nothing allocates after the
        first call, so the call can be captured into a HIP graph.

        Bins repeat from one call to the next to rounding (a few units in the last place), not bit for bit: inside a
        workgroup the waves add to the shared histogram in the order they arrive.  Across workgroups and ranks the
        order is fixed."""
        t, ncomp, precision = self._field(u_hat)
        dk, nbins, out = self._bins(t, nbins, dk, out)
        _lib.engine().ps_spectrum(t, ncomp, self.K, self.W, self.shape, dk, nbins, out, precision)
        return self._reduce(out) if reduce else out

    def _field(self, u_hat):
        """(tensor, components, precision) of a spectral field: [m] + spectral shape or, a scalar field, the spectral shape"""
        t = _t(u_hat)
        if tuple(t.shape) == self.shape:
            ncomp = 1
        else:
            assert tuple(t.shape[1:]) == self.shape and t.dim() == 4, (tuple(t.shape), self.shape)
            ncomp = int(t.shape[0])
        assert t.is_contiguous() and t.dtype in (torch.complex64, torch.complex128)
        precision = 8 if t.dtype == torch.complex128 else 4
        self._same_precision(precision)
        return t, ncomp, precision

    def _bins(self, t, nbins, dk, out):
        """The defaults of a shell histogram and its device tensor: (dk, nbins, out)"""
        dk = self.dk if dk is None else float(dk)
        nbins = self.default_nbins(dk) if nbins is None else int(nbins)
        if out is None:
            out = torch.empty((2, nbins), dtype=torch.float64, device=t.device)
        assert tuple(out.shape) == (2, nbins) and out.dtype == torch.float64 and out.is_contiguous()
        return dk, nbins, out

    def _reduce(self, out):
        """This rank's bins added over the ranks of the grid, on the host: the same bits on every rank"""
        bins = out.cpu().numpy()                       # (waits for the kernel)
        _lib.check_async()
        for c in self.comms:                           # one grid axis after the other: the same order on every rank
            parts = c.allgather_obj(bins)
            bins = parts[0].copy()
            for p in parts[1:]:
                bins += p
        return bins

    def energy(self, u_hat):
        """<u.u>/2 over the whole box, from the spectral coefficients (synchronises: see `spectrum`)."""
        return float(self.spectrum(u_hat)[0].sum())

    def enstrophy(self, u_hat):
        """<|grad u|^2>/2 over the whole box = the enstrophy <|curl u|^2>/2 of a solenoidal field; the dissipation rate
        is 2 nu times it (synchronises: see `spectrum`)."""
        return float(self.spectrum(u_hat)[1].sum())

    def cospectrum(self, a_hat, b_hat, scale=1.0, nbins=None, dk=None, out=None, reduce=True):
        """Shell co-spectrum of two forward-normalised fields of the same shape and precision: float64 [2][nbins],
            [0][b] = sum over shell b of scale * w * sum_c Re(conj(a_hat_c) * b_hat_c)      (sums to scale * <a.b>)
            [1][b] = the same with each mode times |k|^2
        signed.  Shells, weights, shapes, defaults, `reduce` / `out` and repeatability are those of `spectrum`; one kernel,
        one read of each field, no array-sized temporaries.  a_hat may be b_hat: cospectrum(u, u, scale=0.5) equals
        spectrum(u) to rounding."""
        ta, ncomp, precision = self._field(a_hat)
        tb, mb, pb = self._field(b_hat)
        assert (ncomp, precision) == (mb, pb) and ta.dim() == tb.dim(), 'the two fields differ in shape or precision'
        dk, nbins, out = self._bins(ta, nbins, dk, out)
        _lib.engine().ps_cospectrum(ta, tb, ncomp, _lib.PS_DOT, scale, self.K, self.W, self.shape, dk, nbins, out, precision)
        return self._reduce(out) if reduce else out

    def transfer(self, u_hat, n_hat, nbins=None, dk=None, out=None, reduce=True):
        """Transfer spectrum: [0][b] = T(k) = sum w Re(conj(u_hat) . n_hat) with n_hat the projected nonlinear term, [1][b] =
        k^2 T(k).  The shell budget is dE(k)/dt = T(k) - 2 nu k^2 E(k) (row 1 of `spectrum`); sum T = 0 for a conservative
        nonlinear term, and `flux(T)` is the energy flux through each shell."""
        return self.cospectrum(u_hat, n_hat, 1.0, nbins, dk, out, reduce)

    def helicity_spectrum(self, u_hat, nbins=None, dk=None, out=None, reduce=True):
        """Helicity spectrum of a velocity field [3] + spectral shape: [0][b] = H(k) = sum w Re(conj(u_hat) . w_hat) with
        w_hat = 1j * (K x u_hat) formed in registers -- no curl is stored; sums to <u . curl u>.  [1][b] = k^2 H(k).
        Realizability: |H(k)| <= 2 k E(k) mode by mode.  Otherwise as `cospectrum`."""
        t, ncomp, precision = self._field(u_hat)
        assert ncomp == 3 and t.dim() == 4, 'helicity needs a three-component field'
        dk, nbins, out = self._bins(t, nbins, dk, out)
        _lib.engine().ps_cospectrum(t, None, 3, _lib.PS_HELICITY, 1.0, self.K, self.W, self.shape, dk, nbins, out, precision)
        return self._reduce(out) if reduce else out

    def helicity(self, u_hat):
        """Mean helicity <u . curl u> over the whole box (synchronises: see `spectrum`)."""
        return float(self.helicity_spectrum(u_hat)[0].sum())

    def stats(self, u, inv_dx=None, out=None, reduce=True):
        """Single-point statistics of a real physical-space field in one read: float64 [2 + 6 m],
            [0]          max over points of sum_c |u_c| * inv_dx[c]          (advective CFL rate: dt <= C / [0])
            [1]          max over points of sum_c u_c^2
            [2 + 6c + 0..5]   max u_c, min u_c, sum u_c, sum u_c^2, sum u_c^3, sum u_c^4      (`moments` reads the sums)
        u is a contiguous real tensor or DeviceArray of shape [m] + fft.shape(False), m <= 4, or a scalar field of that
        shape, in the transform's precision; every value is converted to double first.  inv_dx (m floats >= 0)
        defaults to N_i / L_i for m == 3 and to zeros otherwise.  A NaN anywhere in component c makes its four sums NaN
        (test those for a blow-up); max / min, [0] and [1] follow fmax / fmin and skip it.

        `reduce` and `out` as in `spectrum`: reduce=True combines over the ranks of the grid on the host (maxima with
        np.maximum, minima with np.minimum, sums added in rank order, one grid axis after the other, so every rank holds
        identical bits), which synchronises; reduce=False only enqueues and returns the device tensor (`out`, a
        contiguous double tensor of 2 + 6 m entries, or a new one), so it can be captured.  Unlike the spectrum the
        result repeats bit for bit from one call to the next: the summation order is fixed."""
        t, ncomp, precision = self._real_field(u)
        if inv_dx is None:
            inv_dx = self.inv_dx if ncomp == 3 else [0.0] * ncomp
        assert len(inv_dx) == ncomp
        nval = _lib.PS_STATS_HEAD + _lib.PS_STATS_PER_COMP * ncomp
        if out is None:
            out = torch.empty(nval, dtype=torch.float64, device=t.device)
        assert tuple(out.shape) == (nval,) and out.dtype == torch.float64 and out.is_contiguous()
        count = int(np.prod(self.pshape, dtype=np.int64))
        _lib.engine().ps_stats(t, ncomp, count, inv_dx, out, precision)
        return self._reduce_stats(out) if reduce else out

    def _real_field(self, u):
        """(tensor, components, precision) of a physical field: [m] + local physical shape or, a scalar field, that shape"""
        t = _t(u)
        if tuple(t.shape) == self.pshape:
            ncomp = 1
        else:
            assert tuple(t.shape[1:]) == self.pshape and t.dim() == 4, (tuple(t.shape), self.pshape)
            ncomp = int(t.shape[0])
        assert t.is_contiguous() and t.dtype in (torch.float32, torch.float64), 'stats needs a contiguous real field'
        precision = 8 if t.dtype == torch.float64 else 4
        self._same_precision(precision)
        return t, ncomp, precision

    def _reduce_stats(self, out):
        """This rank's statistics combined over the ranks of the grid, on the host: the same bits on every rank"""
        vals = out.cpu().numpy()                       # (waits for the kernels)
        _lib.check_async()
        head, per = _lib.PS_STATS_HEAD, _lib.PS_STATS_PER_COMP
        idx = np.arange(len(vals))
        is_max = (idx < head) | ((idx - head) % per == 0)
        is_min = (idx >= head) & ((idx - head) % per == 1)
        for c in self.comms:                           # one grid axis after the other: the same order on every rank
            parts = c.allgather_obj(vals)
            vals = parts[0].copy()
            for p in parts[1:]:
                vals = np.where(is_max, np.maximum(vals, p), np.where(is_min, np.minimum(vals, p), vals + p))
        return vals

    def cfl_rate(self, u):
        """max over the whole box of sum_c |u_c| N_c / L_c: an advective step is stable for dt <= C / cfl_rate
        (synchronises: see `stats`)."""
        return float(self.stats(u)[0])

    def timestep(self, u, cfl, dt_max, dt_min=0.0, out=None):
        """The CFL-limited step min(max(cfl / cfl_rate(u), dt_min), dt_max); dt_max where the rate is zero or not finite.
        out=None: on any grid, from the rank-reduced rate; synchronises and returns a Python float.
        out = a device double[2] tensor: one-rank grids only (no device-side reduction over ranks); enqueues the
        statistics into a tensor this object keeps and then `gfft_ps_timestep`, which writes the step to out[0] and adds
        it to out[1] (the running time); returns `out`.  Nothing synchronises or, after the first call, allocates, so
        the call can be captured with the `rk_stage(..., dt=out)` calls that read the step."""
        assert cfl > 0 and 0 <= dt_min <= dt_max and np.isfinite([cfl, dt_min, dt_max]).all()
        if out is None:
            return timestep_from_rate(self.cfl_rate(u), cfl, dt_max, dt_min)
        assert not self.comms, 'the device path of timestep needs a one-rank grid'
        assert tuple(out.shape) == (2,) and out.dtype == torch.float64 and out.is_contiguous()
        t, ncomp, _ = self._real_field(u)
        nval = _lib.PS_STATS_HEAD + _lib.PS_STATS_PER_COMP * 4
        if self._stats_dev is None or self._stats_dev.device != t.device:
            self._stats_dev = torch.empty(nval, dtype=torch.float64, device=t.device)
        st = self._stats_dev[:_lib.PS_STATS_HEAD + _lib.PS_STATS_PER_COMP * ncomp]
        self.stats(t, out=st, reduce=False)
        _lib.engine().ps_timestep(st, cfl, dt_min, dt_max, out)
        return out

    def whole_axes(self):
        """The axes of the physical grid that this rank holds whole: all three on one rank, 1 and 2 on a slab grid, 2 on a
        pencil grid."""
        return [a for a in range(3) if self.pshape[a] == self._N[a]]

    def structure_functions(self, u, axis, seps, lcomp=None, out=None, reduce=True):
        """The power sums of the increments d = u_c(x + r e_axis) - u_c(x) of a real physical-space field, for every
        separation r of `seps` (grid points, 0 <= r < N[axis], at most 64) from ONE read of the field: float64 [nsep][m][9],
        indexed by `_lib.SF_*`,
            [0 ... 5] sum d, d^2, d^3, d^4, d^5, d^6   [6] sum |d|   [7] sum |d|^3   [8] sum d_l d^2, d_l the increment of
        component `lcomp` at the same point (lcomp None: zeros).  With u a velocity and lcomp = axis, [axis][2] is the sum
        behind the 4/5 law, [8] summed over the components that behind the 4/3 law, and [8] of a scalar carried as a fourth
        component that behind Yaglom's law (`structure_moments` divides by the number of points and forms the ratios;
        include/gfft.h has the exact expressions).  u is as in `stats`: [m] + fft.shape(False), m <= 4, or a scalar field.
        Every value is converted to double first; a NaN reaches exactly the sums of its own component (and the [8] of every
        component if it lies in `lcomp`).

        The axis must be whole on this rank (`whole_axes`): all three axes on one rank, axes 1 and 2 on a slab grid, axis
        2 on a pencil grid, and at most 4096 points long.  Increments across rank boundaries need halos or a transposed copy
        of the field; that is not done here.

        `reduce` and `out` as in `stats`: reduce=True adds the ranks of the grid on the host in rank order, one grid axis
        after the other, so every rank holds identical bits, which synchronises; reduce=False only enqueues and returns the
        device tensor (`out`, a contiguous double tensor [nsep][m][9], or a new one), so it can be captured after one call
        outside the capture.  The result repeats bit for bit from one call to the next: the summation order is fixed."""
        t, ncomp, precision = self._real_field(u)
        axis = int(axis)
        assert 0 <= axis <= 2, axis
        assert self.pshape[axis] == self._N[axis], \
            'structure_functions needs an axis that is whole on this rank: axis %d is split, the whole axes of this grid are %s' % (
                axis, self.whole_axes())
        seps = [int(r) for r in seps]
        assert 1 <= len(seps) <= _lib.PS_SF_MAX_SEP, 'structure_functions takes 1 ... %d separations' % _lib.PS_SF_MAX_SEP
        assert all(0 <= r < self._N[axis] for r in seps), 'a separation must lie in [0, %d)' % self._N[axis]
        lcomp = -1 if lcomp is None else int(lcomp)
        assert -1 <= lcomp < ncomp, lcomp
        shape = (len(seps), ncomp, _lib.PS_SF_NVAL)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=t.device)
        assert tuple(out.shape) == shape and out.dtype == torch.float64 and out.is_contiguous()
        _lib.engine().ps_structure(t, ncomp, self.pshape, axis, seps, lcomp, out, precision)
        return self._reduce_sums(out) if reduce else out

    def _reduce_sums(self, out):
        """`_reduce_stats` for a table of sums only"""
        vals = out.cpu().numpy()                       # (waits for the kernels)
        _lib.check_async()
        for c in self.comms:                           # one grid axis after the other: the same order on every rank
            parts = c.allgather_obj(vals)
            vals = parts[0].copy()
            for p in parts[1:]:
                vals = vals + p
        return vals


# Classical RK4 on v = exp(lambda t) u_hat, lambda = nu |K|^2, written for u_hat itself; E = exp(-lambda h / 2).  Rows
# (cb, ca, q0, qd, q1, qa) of `SpectralOps.rk_stage_if`; u0 = u1 = u_n before row 1, which turns u1 into E^2 u_n; row 4 is
# called with u=None (its cb, q0 and qd do not enter the result) and leaves u_{n+1} in u1.
IFRK4 = ((1. / 2., 1. / 6., 1, 1, 2, 2),
         (1. / 2., 1. / 3., 1, 0, 0, 1),
         (1., 1. / 3., 2, 1, 0, 1),
         (0., 1. / 6., 0, 0, 0, 0))


def timestep_from_rate(rate, cfl, dt_max, dt_min=0.0):
    """The formula of `SpectralOps.timestep` and gfft_ps_timestep on a host float: cfl / rate clamped to
    [dt_min, dt_max]; dt_max for a rate that is zero, negative, infinite or NaN."""
    rate = float(rate)
    want = cfl / rate if (rate > 0 and np.isfinite(rate)) else dt_max
    return float(min(max(want, dt_min), dt_max))


def force_gain(E, band, eps, gain_max=np.inf):
    """The formula of `SpectralOps.forcing_gain` and gfft_ps_force_gain on host numbers, the same arithmetic in the same
    order: E_f = E[0][blo] + ... + E[0][bhi] added serially (E: [2][nbins] as `spectrum` returns it, or its row 0), gain =
    min(eps / (2 E_f), gain_max), 0 for an E_f that is zero, negative, infinite or NaN.  Returns (gain, E_f)."""
    E = np.asarray(E, dtype=np.float64)
    row = E[0] if E.ndim == 2 else E
    blo, bhi = int(band[0]), int(band[1])
    assert 0 <= blo <= bhi < len(row)
    ef = np.float64(0.0)
    for b in range(blo, bhi + 1):
        ef = ef + row[b]
    if not (ef > 0 and np.isfinite(ef)):
        return 0.0, float(ef)
    with np.errstate(over='ignore'):
        want = np.float64(eps) / (2.0 * ef)
    return float(min(want, np.float64(gain_max))), float(ef)


def moments(stats, npoints):
    """Single-point moments from `SpectralOps.stats` (rank-reduced) and the GLOBAL number of points: float64 [m][4] =
    per component the mean, the variance <(u - <u>)^2>, the skewness <(u - <u>)^3> / variance^(3/2) and the flatness
    <(u - <u>)^4> / variance^2 (3 for a Gaussian, 3/2 for a sine).  Host numpy."""
    s = np.asarray(stats, dtype=np.float64)
    s = s[_lib.PS_STATS_HEAD:].reshape(-1, _lib.PS_STATS_PER_COMP)
    n = float(npoints)
    m1, m2, m3, m4 = (s[:, j] / n for j in (2, 3, 4, 5))
    var = m2 - m1 * m1
    c3 = m3 - 3 * m1 * m2 + 2 * m1 ** 3
    c4 = m4 - 4 * m1 * m3 + 6 * m1 * m1 * m2 - 3 * m1 ** 4
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack([m1, var, c3 / var ** 1.5, c4 / (var * var)], axis=1)


GradientMoments = collections.namedtuple('GradientMoments', 'strain enstrophy Q R dissipation skewness flatness transverse_flatness '
                                         'dissipation_flatness enstrophy_flatness strain_enstrophy_correlation betchov div_rms')
GradientMoments.__doc__ = """What `gradient_moments` returns: strain = <S_ij S_ij>, enstrophy = <|w|^2> / 2, Q = <Q>, R = <R>,
dissipation = 2 nu <S_ij S_ij> (None without nu), skewness and flatness of the longitudinal derivatives d u_i / d x_i (averaged
over i), transverse_flatness of d u_i / d x_j, i != j, dissipation_flatness = <(S_ij S_ij)^2> / <S_ij S_ij>^2, enstrophy_flatness =
<|w|^4> / <|w|^2>^2, strain_enstrophy_correlation = <S_ij S_ij |w|^2> / (<S_ij S_ij> <|w|^2>), betchov = <w_i S_ij w_j> / (-4/3
<S_ij S_jk S_ki>) and div_rms = sqrt(<(div u)^2>)."""


def gradient_moments(gs, npoints, nu=None):
    """The small-scale statistics from `SpectralOps.gradient_stats` (rank-reduced) and the GLOBAL number of points, as a
    `GradientMoments`.  With S_n = gs[n] and n = npoints: skewness = (S16 / 3n) / (S15 / 3n)^(3/2), flatness = (S17 / 3n) /
    (S15 / 3n)^2 (3 for a Gaussian, 3/2 for a sine; the skewness of a turbulent field is about -0.5), transverse_flatness =
    (S19 / 6n) / (S18 / 6n)^2.  For a solenoidal, resolved, alias-free periodic field strain = enstrophy, Q = R = 0 and
    betchov = 1.  A ratio whose denominator vanishes is nan or inf, as in `moments`.  Host numpy."""
    s = np.asarray(gs, dtype=np.float64)
    assert s.shape == (_lib.PS_GRAD_NVAL,), s.shape
    n = float(npoints)
    ss, ww = s[_lib.GS_SS] / n, s[_lib.GS_WW] / n
    l2, l3, l4 = (s[i] / (3 * n) for i in (_lib.GS_LONG2, _lib.GS_LONG3, _lib.GS_LONG4))
    t2, t4 = s[_lib.GS_TRANS2] / (6 * n), s[_lib.GS_TRANS4] / (6 * n)
    with np.errstate(divide='ignore', invalid='ignore'):
        return GradientMoments(
            strain=float(ss), enstrophy=float(ww / 2), Q=float(s[_lib.GS_Q] / n), R=float(s[_lib.GS_R] / n),
            dissipation=None if nu is None else float(2 * nu * ss),
            skewness=float(l3 / l2 ** 1.5), flatness=float(l4 / (l2 * l2)), transverse_flatness=float(t4 / (t2 * t2)),
            dissipation_flatness=float((s[_lib.GS_SS2] / n) / (ss * ss)), enstrophy_flatness=float((s[_lib.GS_WW2] / n) / (ww * ww)),
            strain_enstrophy_correlation=float((s[_lib.GS_SSWW] / n) / (ss * ww)),
            betchov=float(np.float64(s[_lib.GS_WSW]) / (-4.0 / 3.0 * s[_lib.GS_SSS])), div_rms=float(np.sqrt(s[_lib.GS_DIV2] / n)))


def log_separations(N, per_octave=2):
    """The separations of a structure function on a periodic axis of N points: the increasing integers 1, 2, 3, 4, 6, 8, 12,
    ... <= N // 2: `per_octave` evenly spaced per factor of two, 2^k (1 + i / per_octave) for i < per_octave, rounded half up
    and deduplicated.  Plain Python integers."""
    N, per_octave = int(N), int(per_octave)
    assert per_octave >= 1
    top, out, octave = N // 2, [], 1
    while octave <= top:
        for i in range(per_octave):
            r = (2 * octave * (per_octave + i) + per_octave) // (2 * per_octave)       # floor(octave (1 + i / p) + 1 / 2)
            if r <= top and (not out or r > out[-1]):
                out.append(r)
        octave *= 2
    return out


StructureMoments = collections.namedtuple('StructureMoments', 'S abs1 abs3 skewness flatness mixed longitudinal transverse')
StructureMoments.__doc__ = """What `structure_moments` returns, every array [nsep][m] but S: S = [nsep][m][6], S[..., p - 1] = <d^p> for
p = 1 ... 6; abs1 = <|d|>, abs3 = <|d|^3>; skewness = S_3 / S_2^(3/2) and flatness = S_4 / S_2^2 of the increments (0 and 3 for a
Gaussian); mixed = <d_l d^2>; longitudinal = the index of the component along the axis and transverse = the others, or None
without an axis or with fewer than three components."""


def structure_moments(sf, npoints, axis=None):
    """The structure functions from `SpectralOps.structure_functions` (rank-reduced) and the GLOBAL number of points, as a
    `StructureMoments`.  With axis = a and m >= 3 component a is labelled longitudinal: S[k, a, 2] / (eps r_k) -> -4/5 in an
    inertial range, and mixed[k, :3].sum() / (eps r_k) -> -4/3 when the table was formed with lcomp = a.  A ratio whose
    denominator vanishes (r = 0) is nan or inf, as in `moments`.  Host numpy."""
    s = np.asarray(sf, dtype=np.float64)
    assert s.ndim == 3 and s.shape[2] == _lib.PS_SF_NVAL, s.shape
    m = s / float(npoints)
    S = m[..., _lib.SF_D1:_lib.SF_D6 + 1]
    s2 = S[..., 1]
    lon = tra = None
    if axis is not None and s.shape[1] >= 3:
        lon = int(axis)
        assert 0 <= lon <= 2, axis
        tra = [c for c in range(3) if c != lon]
    with np.errstate(divide='ignore', invalid='ignore'):
        return StructureMoments(S=S, abs1=m[..., _lib.SF_ABS1], abs3=m[..., _lib.SF_ABS3], skewness=S[..., 2] / s2 ** 1.5,
                                flatness=S[..., 3] / (s2 * s2), mixed=m[..., _lib.SF_MIX], longitudinal=lon, transverse=tra)


Pdf = collections.namedtuple('Pdf', 'centres density below above nan')
Pdf.__doc__ = """What `pdf` returns: the bin centres, the density counts / (n width) with n the number of non-NaN points, tails
included -- so the density integrates to the share of them that lies in the range --, and the counts below, above and NaN."""
JointPdf = collections.namedtuple('JointPdf', 'xcentres ycentres density outside nan')
JointPdf.__doc__ = """What `joint_pdf` returns: the bin centres of both axes, the density [nbx][nby] = counts / (n wx wy) with n the
number of non-NaN points, those outside included, and the counts outside and NaN."""


def pdf(counts, range):
    """A density from one row of `SpectralOps.histogram` or a 1-D `SpectralOps.gradient_pdf` (rank-reduced: int64 [nbins + 3])
    and its (lo, hi), as a `Pdf`.  Rows may be added first (a pooled PDF).  Host numpy; a row without a non-NaN point gives
    nan densities."""
    c = np.asarray(counts)
    assert c.ndim == 1 and len(c) > _lib.PS_PDF_TAIL and c.dtype.kind in 'iu', (c.shape, c.dtype)
    nbins = len(c) - _lib.PS_PDF_TAIL
    lo, hi = float(range[0]), float(range[1])
    width = (hi - lo) / nbins
    n = float(c[:nbins + 2].sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        density = c[:nbins] / (n * width)
    return Pdf(lo + (np.arange(nbins) + 0.5) * width, density, int(c[nbins]), int(c[nbins + 1]), int(c[nbins + 2]))


def joint_pdf(counts, ranges, bins):
    """A 2-D density from a joint `SpectralOps.gradient_pdf` (rank-reduced: int64 [nbx * nby + 2]), its ((xlo, xhi), (ylo, yhi))
    and its bins (an int or a pair), as a `JointPdf`.  Host numpy."""
    nbx, nby = (int(bins), int(bins)) if np.ndim(bins) == 0 else (int(bins[0]), int(bins[1]))
    c = np.asarray(counts)
    assert c.shape == (nbx * nby + 2,) and c.dtype.kind in 'iu', (c.shape, c.dtype, nbx, nby)
    (xlo, xhi), (ylo, yhi) = ((float(a), float(b)) for a, b in ranges)
    wx, wy = (xhi - xlo) / nbx, (yhi - ylo) / nby
    n = float(c[:nbx * nby + 1].sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        density = c[:nbx * nby].reshape(nbx, nby) / (n * wx * wy)
    return JointPdf(xlo + (np.arange(nbx) + 0.5) * wx, ylo + (np.arange(nby) + 0.5) * wy, density, int(c[nbx * nby]), int(c[nbx * nby + 1]))


def model_spectrum(k, kind, k_peak, u_rms):
    """A model E(k) on the shell centres `k` (`SpectralOps.shells`), the target of `SpectralOps.random_field`:
        'gaussian'   E ~ k^4 exp(-2 (k / k_peak)^2)                the usual start of decaying turbulence; peaks at k_peak
        'karman'     E ~ k^4 / (1 + (k / k_peak)^2)^(17/6)         von Karman: k^4 below k_peak, k^(-5/3) above
    normalised so that sum E = 3 u_rms^2 / 2 over the shells given (the sum `SpectralOps.energy` reports).  Host numpy."""
    k = np.asarray(k, dtype=np.float64)
    k_peak, u_rms = float(k_peak), float(u_rms)
    assert k.ndim == 1 and k_peak > 0 and u_rms >= 0 and (k >= 0).all()
    x = k / k_peak
    if kind == 'gaussian':
        E = k ** 4 * np.exp(-2.0 * x * x)
    elif kind == 'karman':
        E = k ** 4 / (1.0 + x * x) ** (17.0 / 6.0)
    else:
        raise AssertionError("kind = 'gaussian' or 'karman'")
    total = E.sum()
    assert total > 0, 'no shell carries energy'
    return E * (1.5 * u_rms * u_rms / total)


def flux(T):
    """Energy flux through the shells from a transfer spectrum `T` ([2][nbins] as `SpectralOps.transfer` returns it, or
    its row 0): Pi[b] = -sum_{j <= b} T[0][j], the energy leaving shells 0..b per unit time; the last entry is -sum T,
    zero for a conservative nonlinear term.  Host numpy."""
    T = np.asarray(T, dtype=np.float64)
    return -np.cumsum(T[0] if T.ndim == 2 else T)


def cross(a, b, out):
    """out = a x b for real fields of shape [3] + local physical shape: contiguous, of one precision, out overlapping
    neither input.  Returns out."""
    assert a.shape[0] == 3 and tuple(a.shape) == tuple(b.shape) == tuple(out.shape)
    (ta, tb, to), precision = _operands(_REAL, a, b, out)
    count = int(np.prod(a.shape[1:], dtype=np.int64))
    _lib.engine().ps_cross(ta, tb, to, count, precision)
    return out


def scalar_flux(u, theta, out):
    """out[s][c] = u[c] * theta[s]: the advective flux of m <= 4 scalars by one velocity, which is read once for all of them.
    u is a real field [3] + physical shape; theta is [m] + physical shape and out [m][3] + physical shape, or, for one
    scalar, the physical shape and [3] + physical shape; all contiguous, of one precision, out overlapping neither input.
    One multiply per value: the correctly rounded product.  Returns out."""
    tu, tt, to = _t(u), _t(theta), _t(out)
    pshape = tuple(tu.shape[1:])
    assert tu.shape[0] == 3 and tu.dim() >= 2 and tu.dtype in (torch.float32, torch.float64)
    lead = () if tuple(tt.shape) == pshape else (int(tt.shape[0]),)
    assert tuple(tt.shape) == lead + pshape and tuple(to.shape) == lead + (3,) + pshape, (tuple(tu.shape), tuple(tt.shape), tuple(to.shape))
    assert tu.dtype == tt.dtype == to.dtype and tu.is_contiguous() and tt.is_contiguous() and to.is_contiguous()
    ns = lead[0] if lead else 1
    assert 1 <= ns <= 4, 'at most 4 scalars per call'
    count = int(np.prod(pshape, dtype=np.int64))
    _lib.engine().ps_scalar_flux(tu, tt, to, ns, count, 8 if tu.dtype == torch.float64 else 4)
    return out


def rk_stage(u, u0, u1, du, cb, ca, dt=None):
    """u = u0 + cb*du (skipped when u is None); u1 += ca*du -- one pass over the four arrays.
    dt: a device double tensor; the coefficients are then cb * dt[0] and ca * dt[0], multiplied on the device (bit for
    bit the result of passing the host products), so a captured stage follows a step that `timestep(out=)` wrote.
    The fields have any one shape and one dtype, real or complex (a complex value is two reals to the kernel), and are
    contiguous; u needs u0 (u0 without u is not read); u and u1 overlap nothing else."""
    assert u is None or u0 is not None, 'u needs u0'
    (tu, tu0, tu1, tdu), precision = _operands(_REAL + _COMPLEX, u, u0, u1, du)
    assert all(t is None or tuple(t.shape) == tuple(tdu.shape) for t in (tu, tu0, tu1)), 'the fields differ in shape'
    count = int(tdu.numel()) * (2 if tdu.dtype in _COMPLEX else 1)
    if dt is not None:
        dt = _t(dt)
        assert dt.dtype == torch.float64 and dt.numel() >= 1 and dt.is_contiguous()
        _lib.engine().ps_rk_stage_dt(tu, tu0, tu1, tdu, count, cb, ca, dt, precision)
        return
    _lib.engine().ps_rk_stage(tu, tu0, tu1, tdu, count, cb, ca, precision)
