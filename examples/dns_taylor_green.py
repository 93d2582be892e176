"""Pseudo-spectral Navier-Stokes (Taylor-Green vortex, RK4) on MI355X: the realistic caller of the
PFFT hot path -- the device counterpart of the reference's examples/spectral_dns_solver.py, same
algorithm, same parameters, same known answer (kinetic energy 0.124953117517 after 10 steps at
64^3, examples/spectral_dns_solver.py:129).

The transforms are `PFFT.forward/backward` of this package, reading and writing the solver's own
device arrays in place.  The elementwise work between them runs either as the package's one-pass
kernels (`mpi4py_fft_amd.spectral`: curl, cross product, projection + viscous term, RK stage;
`fused=True`, default) or as torch expressions that transcribe the reference line by line
(`fused=False`, the A/B baseline: same answer, one temporary per operator).

`cfl=` turns the fixed step into a CFL-controlled one: every step takes dt = min(cfl / rate, dt) with rate = max
sum_c |u_c| N_c / L_c from `SpectralOps.timestep` (one read of U, which the step has in physical space anyway).  With
`device_dt=True` the step never visits the host: the statistics kernel, `gfft_ps_timestep` and the RK stages that read
dt from device memory are all enqueued, so the adaptive step replays from a HIP graph too (`graph=True`).

`forcing=(eps, blo, bhi)` keeps the flow from decaying: linear forcing f_hat = g U_hat in shells blo..bhi with the gain
g = eps / (2 E_band) of `SpectralOps.forcing_gain`, computed once per step from the U_hat the step starts from and held
over its four stages; the term rides in the projection kernel (`project(..., force=)`), no extra pass.  With
`device_gain=True` the gain stays in device memory, so the forced step replays from a HIP graph as well.

`dealias='2/3'` removes the aliasing error of the quadratic term: the initial U_hat is truncated by the 2/3 rule
(`SpectralOps.dealias` with `dealias_mask('2/3')`: integer wavenumber n_i kept iff 3 |n_i| < N_i) and every projection
carries the mask (`project(..., dealias=)`), so each right-hand side leaves truncated -- no extra pass, and fewer bytes than
without: a truncated mode is stored as zero and not loaded.  The Taylor-Green vortex over ten steps at 64^3 puts nothing
measurable beyond |n| = 21: the dealiased energy after 10 steps is 0.124953117516743 (DEALIASED_ENERGY below; measured on one
MI355X, there is no counterpart in the reference, which does not dealias), the undealiased run's value to all 15 digits.  A
forced run long enough to fill the spectrum is wrong without the truncation.

`scalar=(kappa, G)` carries a passive scalar along, d theta/dt + u . grad theta = kappa lap theta - G . u, in flux form: every
right-hand side adds one backward of theta_hat, `spectral.scalar_flux(U, Theta, UT)` on the U the step already has in physical
space, three forwards and `SpectralOps.scalar_rhs` (with the mean-gradient term and the step's dealiasing mask fused in); its
Runge-Kutta stages sit beside the velocity's and take the same step.  theta_0 = cos(x) sin(y / 2) cos(z / 2): zero mean, one
period of each axis of the box (2 pi, 4 pi, 4 pi).  After 10 steps at 64^3 with kappa = nu and G = (1, 0, 0) the variance
<theta^2> is SCALAR_VARIANCE below (measured on one MI355X; the reference has no scalar).

`integrator='ifrk4'` integrates the viscous and diffusive terms exactly (the integrating factor exp(nu |K|^2 t), classical RK4 on
the rest: `spectral.IFRK4`): every projection runs with nu = 0 and every scalar right-hand side with kappa = 0, and the stages are
`SpectralOps.rk_stage_if` with nu / kappa -- the same passes over the same bytes, and a step that nu k_max^2 (a well-resolved
run, a scalar of low Schmidt number) no longer limits.  Here nu |k|^2 dt is 2e-5 at the vortex's own wavenumber and 1e-2 at the
largest one, and the two integrators agree far below the
seventh digit: the energy after 10 steps at 64^3 is IF_ENERGY below (measured on one MI355X).

`gradients=True` reads the small scales of the final state: `SpectralOps.gradient(U_hat, .)` forms all nine i K_j U_hat_i in one pass,
nine backward transforms give A_ij = d u_i / d x_j, and `SpectralOps.gradient_stats` reduces one read of A to the 20 sums that
`spectral.gradient_moments` turns into dissipation, enstrophy, derivative skewness and flatness, <Q>, <R> and the Betchov ratio
<w S w> / (-4/3 <S S S>), which is 1 for a resolved, alias-free run.  The Taylor-Green vortex starts with zero skewness; after 10
steps at 64^3 with dealias='2/3' the longitudinal skewness is GRADIENT_SKEWNESS below (measured on one MI355X; the reference has
no such diagnostic).

`pdfs=True` (with `gradients=True`) adds the distributions those moments compress, from the same A: the joint histogram of the
invariants (R, Q) by `SpectralOps.gradient_pdf` on a plane scaled by <Q_w> = <|w|^2> / 4, and the PDF of the longitudinal
derivatives pooled over the three directions, three `SpectralOps.histogram` calls added; counts are integers, so one rank and
many give the same tables.  `solve(w, verbose=True, gradients=True, pdfs=True, dealias='2/3')` prints the shares of the four
(R, Q) quadrants.

`particles=(P, order, seed)` follows P tracers through the flow: positions uniform in the box, replicated on all ranks, advanced
by the same RK4 as the velocity -- every right-hand side interpolates the stage's velocity at the stage's positions with
`SpectralOps.interpolate`, for order 2 straight from the U the step already holds in physical space, for order 4 from B-spline
coefficients (`scale_axes(U_hat, bspline_vectors(4))` and three more backward transforms); the positions ride through
`spectral.rk_stage` beside the velocity's stages and are not wrapped (the interpolation is periodic).  After 10 steps at 64^3
with dealias='2/3' the coordinates of 1000 cubic tracers (seed 7) add up to PARTICLE_CHECK below (measured on one MI355X; the
reference has no particles).

`structure=(axis, per_octave)` (or `(axis, per_octave, every)`) reads the two-point statistics of the velocity along a grid axis
this rank holds whole: `SpectralOps.structure_functions(U, axis, spectral.log_separations(N, per_octave), lcomp=axis)` on the U the
step leaves in physical space -- one read of U for all separations -- and `spectral.structure_moments`.  Every `every` steps
(default: after the last step only) it prints the longitudinal S_2(r), the 4/5-law ratio -S_3L / (eps r) with eps = 2 nu sum k^2
E(k) from `SpectralOps.spectrum`, and the flatness of the longitudinal increment at the smallest separation.  The Taylor-Green
vortex at 64^3 after ten steps is a smooth laminar flow: the ratio is far from 4/5 and the flatness is that of a few Fourier
modes; the diagnostic is there for the forced runs this example grows into.  Off by default; it touches no other output.

  python examples/dns_taylor_green.py                         # 1 GPU
  torchrun --nproc-per-node 2 examples/dns_taylor_green.py    # one rank per GPU
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


DEALIASED_ENERGY = 0.124953117516743          # solve(dealias='2/3'), M = 6, 10 steps
SCALAR_VARIANCE = 0.126225641497587           # 'scalar_variance' of solve(scalar=(nu, (1, 0, 0))), M = 6, 10 steps
IF_ENERGY = 0.124953117516741                 # solve(integrator='ifrk4'), M = 6, 10 steps
GRADIENT_SKEWNESS = -0.064835990474654        # 'gradients'.skewness of solve(gradients=True, dealias='2/3'), M = 6, 10 steps
PARTICLE_CHECK = 15755.713888103239            # sum of 'particles' of solve(particles=(1000, 4, 7), dealias='2/3'), M = 6, 10 steps
PDF_BINS, PDF_R, PDF_Q, PDF_SIGMAS = 128, 4.0, 6.0, 6.0     # solve(pdfs=True): bins per axis; the (R, Q) plane in <Q_w>^(3/2), <Q_w>; the derivative range


def solve(world, M=6, nsteps=10, dt=0.01, nu=0.000625, verbose=False, fused=True, graph=False, spectrum=False,
          transfer=False, stats=None, cfl=None, device_dt=False, forcing=None, device_gain=False, dealias=None,
          scalar=None, integrator='rk4', gradients=False, pdfs=False, particles=None, structure=None, init=None):
    """Returns the kinetic energy after `nsteps`; with spectrum=True, (energy, E) where E is the shell spectrum
    `SpectralOps.spectrum` of the final U_hat: E[0] = E(k), E[1] = k^2 E(k), shells of width min(2 pi / L).
    With transfer=True (fused path), (energy, T) where T is `SpectralOps.transfer(U_hat, N_hat)` of the final state,
    N_hat the fused right-hand side evaluated with nu = 0 -- the projected nonlinear term alone: T[0] = T(k) of
    dE(k)/dt = T(k) - 2 nu k^2 E(k), T[1] = k^2 T(k); a dict passed as `stats` also receives 'nonlinear_energy'
    (`energy(N_hat)`) and 'helicity' (`helicity(U_hat)`).
    cfl: take dt = `SpectralOps.timestep(U, cfl, dt_max=dt)` at every step (fused path) instead of the fixed `dt`;
    device_dt=True keeps that step in device memory (one rank; needed under graph=True).  These paths take the final
    energy from `SpectralOps.stats`, sum_c S2_c / (2 N^3), and put the simulated 'time' into a dict passed as `stats`.
    forcing=(eps, blo, bhi) (fused path): every right-hand side adds g U_hat in shells blo..bhi, g = eps / (2 E_band) from
    `SpectralOps.forcing_gain` of the U_hat at the start of the step; device_gain=True computes it through `out=` and
    leaves it in device memory (one rank; needed under graph=True).  A dict passed as `stats` receives the last 'gain'
    and 'band_energy'.
    dealias='2/3': the initial U_hat and every right-hand side are truncated by the 2/3 rule -- on the fused path by
    `SpectralOps.dealias` and `project(..., dealias=)`, on the fused=False path by the same mask as an array-sized torch
    expression (the A/B baseline).
    scalar=(kappa, G): a passive scalar theta with diffusivity kappa and imposed mean gradient G (three floats, or None) is
    advanced with the velocity, theta_0 = cos(x) sin(y / 2) cos(z / 2) -- on the fused path by `spectral.scalar_flux` and
    `SpectralOps.scalar_rhs`, on the fused=False path by array-sized torch expressions (the A/B baseline).  A dict passed as
    `stats` receives 'scalar_variance' = <theta^2> (fused: 2 * sum(spectrum(T_hat)[0])) and 'scalar_flux' = the three
    <u_c theta> (fused: sum(cospectrum(U_hat[c], T_hat)[0])).  The velocity, and so the returned energy, is unchanged.
    integrator='ifrk4' (fused path): integrating-factor RK4 -- the right-hand sides are formed with nu = 0 and kappa = 0 and
    the stages are `SpectralOps.rk_stage_if` with nu / kappa, following `spectral.IFRK4`; it combines with every option
    above.  'rk4' (the default) is the explicit scheme.
    gradients=True: a dict passed as `stats` receives 'gradients', the `spectral.gradient_moments` (with nu) of the velocity-gradient
    tensor of the final state -- on the fused path from `SpectralOps.gradient`, nine backward transforms and
    `SpectralOps.gradient_stats`, on the fused=False path from array-sized torch expressions (the A/B baseline).  It reads the
    final U_hat only and combines with every option above; the diagnostic itself runs once, outside any captured step.
    pdfs=True (needs gradients=True and the fused path): the distributions behind those moments, from the same A -- a dict passed
    as `stats` receives 'pdfs', a dict with 'rq' (the `spectral.joint_pdf` of the invariants (R, Q) on +-PDF_R <Q_w>^(3/2) x
    +-PDF_Q <Q_w>, <Q_w> = <|w|^2> / 4 from the sums of `gradient_stats`, PDF_BINS^2 bins, by `SpectralOps.gradient_pdf`),
    'longitudinal' (the `spectral.pdf` of d u_i / d x_i pooled over i on +-PDF_SIGMAS standard deviations, PDF_BINS bins: three
    `SpectralOps.histogram` calls added), the int64 tables themselves ('rq_counts', 'longitudinal_counts'), their ranges
    ('rq_range', 'longitudinal_range') and 'quadrants', the shares of the in-range points in the four quarters of the table: (lower
    half of the R range, upper half of the Q range), (upper, upper), (lower, lower), (upper, lower).  The halves meet at 0 to
    within the rounding of the bin rule: a point with R or Q exactly 0 may count on either side.
    particles=(P, order, seed): P tracers, uniform in the box from np.random.default_rng(seed), the same on all ranks, in a
    double [P][3] tensor, advanced with the velocity: every right-hand side interpolates its stage's velocity at its stage's
    positions -- on the fused path by `SpectralOps.interpolate` (order 2 from U itself, order 4 from the coefficients that
    `SpectralOps.scale_axes` with `bspline_vectors(4)` and three backward transforms give; on one rank with reduce=False, so the
    step stays capturable), on the fused=False path by torch index expressions over the same weights (the A/B baseline) -- and
    the positions take the stages of `spectral.rk_stage` (dt= included) beside the velocity's.  Positions are not wrapped.
    A dict passed as `stats` receives 'particles' (numpy [P][3]) and 'particle_velocity' (the last interpolated velocities).
    The velocity, and so the returned energy, is unchanged.
    structure=(axis, per_octave) or (axis, per_octave, every) (fused path): the structure functions of the velocity along grid
    axis `axis` (whole on this rank: 1 or 2 on several ranks) at `spectral.log_separations(N, per_octave)`, every `every` steps
    (default nsteps: the final state only), from the U the step leaves in physical space.  A dict passed as `stats` receives
    'structure', a list with one dict per evaluation: 'step', 'r' (the separations in length units), 'moments' (the
    `spectral.structure_moments` with the longitudinal component labelled), 'eps' (2 nu sum k^2 E(k) of `SpectralOps.spectrum`)
    and 'four_fifths' (-S_3L / (eps r) per separation).  It reads U and U_hat only; every other output is unchanged.
    init=('random', seed, k_peak, u_rms) (fused path): start from `SpectralOps.random_field` -- a random-phase solenoidal field
    whose shell spectrum is `spectral.model_spectrum(..., 'gaussian', k_peak, u_rms)` exactly, the same on any number of ranks --
    instead of the Taylor-Green vortex (None, the default).
    forcing=('white', eps, blo, bhi) (fused path, not under graph=True: the scale is formed on the host): after every step
    `SpectralOps.white_noise_force` adds a fresh random solenoidal field in shells blo..bhi that carries exactly eps h of energy
    (stream = the step number, seed = init's seed or 0).  A dict passed as `stats` receives 'white_factor', the last scale."""
    from mpi4py_fft_amd import PFFT, _lib, newDistArray, spectral
    assert structure is None or fused, 'structure needs the fused path'
    assert init is None or (init[0] == 'random' and len(init) == 4 and fused), "init = None or ('random', seed, k_peak, u_rms) on the fused path"
    white = forcing is not None and forcing[0] == 'white'
    if white:
        assert fused and not graph and len(forcing) == 4, "forcing=('white', eps, blo, bhi) needs the fused path without graph=True"
        w_eps, w_band, w_seed = float(forcing[1]), (int(forcing[2]), int(forcing[3])), (int(init[1]) if init is not None else 0)
        w_step, w_factor = [0], [0.0]
        forcing = None
    assert not pdfs or (gradients and fused), 'pdfs needs gradients=True and the fused path'
    N = [2 ** M] * 3
    L = np.array([2 * np.pi, 4 * np.pi, 4 * np.pi])
    FFT = PFFT(world, N, collapse=False)                      # real input: r2c along axis 2
    dev = FFT.forward.input_array.device

    U = newDistArray(FFT, False, rank=1)                      # velocity, physical space
    U_hat = newDistArray(FFT, rank=1)                         # velocity, spectral space
    U_hat0, U_hat1, dU = (newDistArray(FFT, rank=1) for _ in range(3))
    curl = newDistArray(FFT, False, rank=1)

    # local mesh and wavenumbers (examples/spectral_dns_solver.py:44-63), moved to the device
    X = np.ogrid[FFT.local_slice(False)]
    X = [torch.as_tensor(np.broadcast_to(x * L[i] / N[i], FFT.shape(False)).copy(), device=dev)
         for i, x in enumerate(X)]
    s = FFT.local_slice()
    k = [np.fft.fftfreq(n, 1. / n).astype(int) for n in N[:-1]]
    k.append(np.fft.rfftfreq(N[-1], 1. / N[-1]).astype(int))
    Ks = np.meshgrid(*[ki[si] for ki, si in zip(k, s)], indexing='ij', sparse=True)
    Lp = 2 * np.pi / L
    K = torch.as_tensor(np.array([np.broadcast_to(kk * Lp[i], FFT.shape(True)) for i, kk in enumerate(Ks)]),
                        dtype=torch.float64, device=dev)
    K2 = (K * K).sum(0)
    K_over_K2 = K / torch.where(K2 == 0, torch.ones_like(K2), K2)

    u, uh, uh0, uh1, du, cu = (a.tensor for a in (U, U_hat, U_hat0, U_hat1, dU, curl))
    if scalar is not None:
        kappa, G = float(scalar[0]), (None if scalar[1] is None else tuple(float(g) for g in scalar[1]))
        Theta = newDistArray(FFT, False)                      # the scalar, physical space
        T_hat, T_hat0, T_hat1, dT = (newDistArray(FFT) for _ in range(4))
        th, tht, tht0, tht1, dth = (a.tensor for a in (Theta, T_hat, T_hat0, T_hat1, dT))
    if particles is not None:
        n_part, p_order, p_seed = int(particles[0]), int(particles[1]), particles[2]
        assert p_order in (2, 4), 'particles = (P, order, seed) with order 2 or 4'
        xp_start = np.random.default_rng(p_seed).uniform(0.0, 1.0, (n_part, 3)) * L
        Xp = torch.tensor(xp_start, dtype=torch.float64, device=dev)          # (a copy, also where the device is the host)
        Xp0, Xp1, dXp = (torch.zeros_like(Xp) for _ in range(3))          # the stage's start, the accumulator, the velocity at Xp
        one_rank = world.Get_size() == 1
        if p_order == 4:
            Coef = newDistArray(FFT, False, rank=1)               # B-spline coefficients of U
            C_hat = newDistArray(FFT, rank=1)
            # the prefilter per axis: 1 / ((2 + cos(2 pi n / N)) / 3) over this rank's spectral block
            bvec = [1.0 / ((2.0 + np.cos(2 * np.pi * ki[si] / float(n))) / 3.0) for ki, si, n in zip(k, s, N)]
    assert dealias in (None, '2/3'), dealias
    assert integrator in ('rk4', 'ifrk4') and (fused or integrator == 'rk4'), 'ifrk4 needs the fused path'
    ifrk = integrator == 'ifrk4'
    mask = None
    if dealias and not fused:
        # the 2/3 mask as an array: n_i kept iff 3 |n_i| < N_i
        keep = torch.as_tensor(np.logical_and.reduce(np.broadcast_arrays(*[3 * np.abs(kk) < n for kk, n in zip(Ks, N)])), device=dev)
    if fused:
        ops = spectral.SpectralOps(FFT, L)
        if dealias:
            mask = ops.dealias_mask(dealias)
        W_hat = newDistArray(FFT, rank=1)                     # i K x u_hat
        UxW = newDistArray(FFT, False, rank=1)                # u x curl u
        if scalar is not None:
            UT = newDistArray(FFT, False, rank=1)             # u theta
            UT_hat = newDistArray(FFT, rank=1)

        force = [None]                                        # project's force= of the current step
        if particles is not None and p_order == 4:
            bspl = ops.bspline_vectors(4)

        def compute_rhs_fused(nu=0.0 if ifrk else nu):
            for j in range(3):
                FFT.backward(U_hat[j], U[j])                  # kernels read U_hat[j], write U[j]
            ops.curl(U_hat, W_hat)
            for j in range(3):
                FFT.backward(W_hat[j], curl[j])
            spectral.cross(U, curl, UxW)
            for j in range(3):
                FFT.forward(UxW[j], dU[j])
            ops.project(dU, U_hat, nu, force=force[0], dealias=mask)
            if scalar is not None:                            # U is this stage's velocity in physical space already
                FFT.backward(T_hat, Theta)
                spectral.scalar_flux(U, Theta, UT)
                for j in range(3):
                    FFT.forward(UT[j], UT_hat[j])
                ops.scalar_rhs(dT, UT_hat, T_hat, 0.0 if ifrk else kappa, G, U_hat, dealias=mask)
            if particles is not None:                         # the stage's velocity at the stage's positions
                field = U
                if p_order == 4:
                    ops.scale_axes(U_hat, bspl, out=C_hat)
                    for j in range(3):
                        FFT.backward(C_hat[j], Coef[j])
                    field = Coef
                if one_rank:
                    ops.interpolate(field, Xp, order=p_order, out=dXp, reduce=False)          # enqueued, like everything else
                else:
                    dXp.copy_(torch.as_tensor(ops.interpolate(field, Xp, order=p_order)))    # each rank its points; added on the host

    def fwd(x, out):      # physical (torch expression) -> spectral slice `out`
        out.copy_(FFT.forward(x).tensor)

    def bwd(x, out):
        out.copy_(FFT.backward(x).tensor)

    def compute_rhs():
        for j in range(3):
            bwd(uh[j], u[j])
        bwd(1j * (K[0] * uh[1] - K[1] * uh[0]), cu[2])
        bwd(1j * (K[2] * uh[0] - K[0] * uh[2]), cu[1])
        bwd(1j * (K[1] * uh[2] - K[2] * uh[1]), cu[0])
        fwd(u[1] * cu[2] - u[2] * cu[1], du[0])
        fwd(u[2] * cu[0] - u[0] * cu[2], du[1])
        fwd(u[0] * cu[1] - u[1] * cu[0], du[2])
        p_hat = (du * K_over_K2).sum(0)
        du.sub_(p_hat * K)
        du.sub_(nu * K2 * uh)
        if dealias:
            du.masked_fill_(~keep, 0)
        if scalar is not None:
            bwd(tht, th)
            dth.zero_()
            for j in range(3):
                dth.sub_(1j * K[j] * FFT.forward(u[j] * th).tensor)
            dth.sub_(kappa * K2 * tht)
            if G is not None:
                dth.sub_(G[0] * uh[0] + G[1] * uh[1] + G[2] * uh[2])
            if dealias:
                dth.masked_fill_(~keep, 0)
        if particles is not None:
            field = u
            if p_order == 4:
                pre = torch.as_tensor(bvec[0][:, None, None] * bvec[1][None, :, None] * bvec[2][None, None, :], device=dev)
                field = torch.stack([FFT.backward(uh[j] * pre).tensor.clone() for j in range(3)])
            part = interp_torch(field)
            if world.Get_size() > 1:
                part = torch.as_tensor(sum(world.allgather_obj(part.cpu().numpy())), device=dev)
            dXp.copy_(part)

    def interp_torch(field):
        """this rank's share of the interpolant of field [3] + local shape at Xp as torch index expressions: per axis the
        base cell, the weights and the wrapped indices, then order^3 gathers per component"""
        start = [sl.start or 0 for sl in FFT.local_slice(False)]
        n = field.shape[1:]
        w, idx, ok = [], [], []
        for a in range(3):
            sa = Xp[:, a] * (N[a] / L[a])
            ia = torch.floor(sa)
            t = sa - ia
            r = 1.0 - t
            w.append([r, t] if p_order == 2 else
                     [r * r * r / 6.0, (3.0 * t * t * t - 6.0 * t * t + 4.0) / 6.0, (3.0 * r * r * r - 6.0 * r * r + 4.0) / 6.0, t * t * t / 6.0])
            b = ia.long() - (1 if p_order == 4 else 0)
            l = [(b + j) % N[a] - start[a] for j in range(p_order)]
            ok.append([(lj >= 0) & (lj < n[a]) for lj in l])
            idx.append([lj.clamp(0, n[a] - 1) for lj in l])
        out = torch.zeros_like(dXp)
        for j0 in range(p_order):
            for j1 in range(p_order):
                for j2 in range(p_order):
                    inside = ok[0][j0] & ok[1][j1] & ok[2][j2]
                    vals = field[:, idx[0][j0], idx[1][j1], idx[2][j2]].T.to(torch.float64)
                    out += torch.where(inside[:, None], (w[0][j0] * w[1][j1] * w[2][j2])[:, None] * vals, torch.zeros_like(vals))
        return out

    u[0] = torch.sin(X[0]) * torch.cos(X[1]) * torch.cos(X[2])
    u[1] = -torch.cos(X[0]) * torch.sin(X[1]) * torch.cos(X[2])
    u[2] = 0
    for i in range(3):
        fwd(u[i], uh[i])
    if init is not None:
        ops.random_field(U_hat, spectral.model_spectrum(ops.shells(ops.default_nbins()), 'gaussian', float(init[2]), float(init[3])),
                         seed=int(init[1]))
    if dealias and fused:
        ops.dealias(U_hat, mask)
    elif dealias:
        uh.masked_fill_(~keep, 0)
    if init is not None:                                      # U is what the first step's controller and diagnostics read
        for j in range(3):
            FFT.backward(U_hat[j], U[j])
    if scalar is not None:
        th.copy_(torch.cos(X[0]) * torch.sin(X[1] / 2) * torch.cos(X[2] / 2))
        fwd(th, tht)
        if dealias and fused:
            ops.dealias(T_hat, mask)
        elif dealias:
            tht.masked_fill_(~keep, 0)

    a = [1. / 6., 1. / 3., 1. / 3., 1. / 6.]
    b = [0.5, 0.5, 1.]
    adaptive = cfl is not None
    if adaptive:
        assert fused and (device_dt or not graph), 'a CFL-controlled step needs the fused path, and device_dt under a graph'
        sim_time = [0.0]
        if device_dt:
            dt_dev = torch.zeros(2, dtype=torch.float64, device=dev)      # [0] the step, [1] the running time
    forced = forcing is not None
    if forced:
        assert fused and (device_gain or not graph), 'forcing needs the fused path, and device_gain under a graph'
        f_eps, band = float(forcing[0]), (int(forcing[1]), int(forcing[2]))
        last_gain = [0.0, 0.0]                                # gain and band energy of the last step
        if device_gain:
            gain_dev = torch.zeros(2, dtype=torch.float64, device=dev)    # [0] the gain, [1] the band energy
            force[0] = (gain_dev, band)
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    t0 = time.time()
    def step():
        h = dt
        if forced and device_gain:
            ops.forcing_gain(U_hat, f_eps, band, out=gain_dev)   # enqueued, like the step below
        elif forced:
            last_gain[:] = ops.forcing_gain(U_hat, f_eps, band)
            force[0] = (last_gain[0], band)
        if adaptive and device_dt:
            ops.timestep(U, cfl, dt_max=dt, out=dt_dev)          # enqueued: nothing comes back to the host
        elif adaptive:
            h = ops.timestep(U, cfl, dt_max=dt)
            sim_time[0] += h
        uh0.copy_(uh)
        uh1.copy_(uh)
        if scalar is not None:
            tht0.copy_(tht)
            tht1.copy_(tht)
        if particles is not None:
            Xp0.copy_(Xp)
            Xp1.copy_(Xp)
        for rk in range(4):
            if ifrk:
                compute_rhs_fused()
                cb, ca = spectral.IFRK4[rk][:2]
                step_of = dict(dt=dt_dev) if adaptive and device_dt else dict(h=h)
                ops.rk_stage_if(U_hat if rk < 3 else None, U_hat0, U_hat1, dU, nu, cb, ca, spectral.IFRK4[rk][2:], **step_of)
                if scalar is not None:
                    ops.rk_stage_if(T_hat if rk < 3 else None, T_hat0, T_hat1, dT, kappa, cb, ca, spectral.IFRK4[rk][2:], **step_of)
            elif adaptive and device_dt:
                compute_rhs_fused()
                spectral.rk_stage(U_hat if rk < 3 else None, U_hat0, U_hat1, dU, b[rk] if rk < 3 else 0.0, a[rk], dt=dt_dev)
                if scalar is not None:
                    spectral.rk_stage(T_hat if rk < 3 else None, T_hat0, T_hat1, dT, b[rk] if rk < 3 else 0.0, a[rk], dt=dt_dev)
            elif fused:
                compute_rhs_fused()
                spectral.rk_stage(U_hat if rk < 3 else None, U_hat0, U_hat1, dU,
                                  b[rk] * h if rk < 3 else 0.0, a[rk] * h)
                if scalar is not None:
                    spectral.rk_stage(T_hat if rk < 3 else None, T_hat0, T_hat1, dT,
                                      b[rk] * h if rk < 3 else 0.0, a[rk] * h)
            else:
                compute_rhs()
                if rk < 3:
                    torch.add(uh0, du, alpha=b[rk] * dt, out=uh)
                uh1.add_(du, alpha=a[rk] * dt)
                if scalar is not None:
                    if rk < 3:
                        torch.add(tht0, dth, alpha=b[rk] * dt, out=tht)
                    tht1.add_(dth, alpha=a[rk] * dt)
            if particles is not None and fused:               # dXp is this stage's velocity at Xp: the stage the velocity took
                if adaptive and device_dt:
                    spectral.rk_stage(Xp if rk < 3 else None, Xp0, Xp1, dXp, b[rk] if rk < 3 else 0.0, a[rk], dt=dt_dev)
                else:
                    spectral.rk_stage(Xp if rk < 3 else None, Xp0, Xp1, dXp, b[rk] * h if rk < 3 else 0.0, a[rk] * h)
            elif particles is not None:
                if rk < 3:
                    torch.add(Xp0, dXp, alpha=b[rk] * dt, out=Xp)
                Xp1.add_(dXp, alpha=a[rk] * dt)
        uh.copy_(uh1)
        if white:                                             # dU is free between steps: the unscaled random band field
            w_factor[0] = ops.white_noise_force(U_hat, dU, w_step[0], w_eps, h, w_band, w_seed)
            w_step[0] += 1
        if particles is not None:
            Xp.copy_(Xp1)
        if scalar is not None:
            tht.copy_(tht1)
        for i in range(3):
            if fused:
                FFT.backward(U_hat[i], U[i])
            else:
                bwd(uh[i], u[i])

    sf_log = []

    def structure_diag(n):
        """after step n (1-based): the structure functions of U along the chosen axis, when the interval says so"""
        if structure is None:
            return
        axis, per_octave = int(structure[0]), int(structure[1])
        every = int(structure[2]) if len(structure) > 2 else nsteps
        if n % every and n != nsteps:
            return
        seps = spectral.log_separations(N[axis], per_octave)
        sf = ops.structure_functions(U, axis, seps, lcomp=axis)              # rank-reduced; one read of U for all separations
        mo = spectral.structure_moments(sf, N[0] * N[1] * N[2], axis=axis)
        eps = 2.0 * nu * float(ops.spectrum(U_hat)[1].sum())
        r = np.array(seps) * (L[axis] / N[axis])
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = -mo.S[:, axis, 2] / (eps * r)
        sf_log.append(dict(step=n, r=r, moments=mo, eps=eps, four_fifths=ratio))
        if verbose and world.Get_rank() == 0:
            print('  structure functions along axis %d after step %d: eps = %.6e, flatness of the longitudinal increment at r = %.4f: %.4f'
                  % (axis, n, eps, r[0], mo.flatness[0, axis]))
            for k in range(len(seps)):
                print('    r = %8.4f  S_2L = %.6e  -S_3L / (eps r) = % .4e' % (r[k], mo.S[k, axis, 1], ratio[k]))

    if graph:
        # One RK4 step is ~130 small kernels at 64^3: launch bound.  Every kernel of this package
        # is enqueued on torch's current stream and nothing allocates or synchronises after the
        # first execution, so the step can be captured into a HIP graph and replayed.
        assert fused and world.Get_size() == 1 and dev.type == 'cuda'
        keep = uh.clone()
        keep_t = tht.clone() if scalar is not None else None
        keep_u = u.clone() if adaptive else None     # the adaptive step READS U: the warm-up must not leave its own there
        keep_x = Xp.clone() if particles is not None else None
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            step()                               # warm-up on the capture stream: scratch, tables
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        uh.copy_(keep)
        if scalar is not None:
            tht.copy_(keep_t)
        if particles is not None:
            Xp.copy_(keep_x)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        uh.copy_(keep)
        if scalar is not None:
            tht.copy_(keep_t)
        if particles is not None:
            Xp.copy_(keep_x)
        if adaptive:
            u.copy_(keep_u)
            dt_dev.zero_()
        torch.cuda.synchronize()
        t0 = time.time()
        for n in range(nsteps):
            g.replay()
            structure_diag(n + 1)
    else:
        for n in range(nsteps):
            step()
            structure_diag(n + 1)
    if structure is not None and stats is not None:
        stats.update(structure=sf_log)
    if white and stats is not None:
        stats.update(white_factor=w_factor[0])
    if adaptive:
        st = ops.stats(U)                                     # rank-reduced; one read of U, no temporaries
        energy = float(sum(st[2 + 6 * c + 3] for c in range(3))) / (2.0 * N[0] * N[1] * N[2])
        if device_dt:
            sim_time[0] = float(dt_dev[1].item())
        if stats is not None:
            stats.update(time=sim_time[0])
    else:
        energy = sum(world.allgather_obj(float((u * u).sum().item()))) / N[0] / N[1] / N[2] / 2
    if forced:
        if device_gain:
            last_gain[:] = gain_dev.cpu().tolist()
        if stats is not None:
            stats.update(gain=last_gain[0], band_energy=last_gain[1])
    if scalar is not None:
        if fused:
            variance = 2.0 * float(ops.spectrum(T_hat)[0].sum())
            sflux = [float(ops.cospectrum(U_hat[c], T_hat)[0].sum()) for c in range(3)]
        else:
            bwd(tht, th)
            npts = float(N[0] * N[1] * N[2])
            variance = sum(world.allgather_obj(float((th * th).sum().item()))) / npts
            sflux = [sum(world.allgather_obj(float((u[c] * th).sum().item()))) / npts for c in range(3)]
        if stats is not None:
            stats.update(scalar_variance=variance, scalar_flux=sflux)
    if particles is not None:
        xp_h, vp_h = Xp.cpu().numpy(), dXp.cpu().numpy()
        if stats is not None:
            stats.update(particles=xp_h, particle_velocity=vp_h)
    elapsed = time.time() - t0
    if verbose and world.Get_rank() == 0:
        print('%d^3, %d steps, %s pointwise path: %.3f s (%.2f ms per RK4 step), energy = %.12f'
              % (N[0], nsteps, ('fused-kernel' if fused else 'torch-expression') + (' + HIP graph replay' if graph else '')
                 + (', dealiased (%s)' % dealias if dealias else '') + (', integrating factor' if ifrk else ''), elapsed,
                 elapsed / nsteps * 1e3, energy))
        if adaptive:
            print('  CFL %g (%s dt): simulated time %.6f in %d steps' % (cfl, 'device' if device_dt else 'host', sim_time[0], nsteps))
        if forced:
            print('  forcing shells %d..%d at eps = %g (%s gain): last gain %.6f on band energy %.6f -> injecting %.6f'
                  % (band + (f_eps, 'device' if device_gain else 'host', last_gain[0], last_gain[1], 2 * last_gain[0] * last_gain[1])))
    if scalar is not None and verbose and world.Get_rank() == 0:
        print('  scalar (kappa = %g, G = %s): variance %.15f, flux <u theta> = (%.6e, %.6e, %.6e)' % ((kappa, G, variance) + tuple(sflux)))
    if particles is not None and verbose and world.Get_rank() == 0:
        print('  %d tracers, order %d: sum of coordinates %.12f, mean |v| %.6f, largest displacement %.6f'
              % (n_part, p_order, xp_h.sum(), np.sqrt((vp_h * vp_h).sum(axis=1)).mean() if n_part else 0.0,
                 np.abs(xp_h - xp_start).max() if n_part else 0.0))
    if gradients:
        npts = N[0] * N[1] * N[2]
        if fused:
            A_hat, A = newDistArray(FFT, rank=2), newDistArray(FFT, False, rank=2)
            ops.gradient(U_hat, A_hat)                        # all nine i K_j U_hat_i in one pass
            for i in range(3):
                for j in range(3):
                    FFT.backward(A_hat[i][j], A[i][j])
            gs = ops.gradient_stats(A)                        # rank-reduced; one read of A, no temporaries
        else:
            a = torch.empty((3, 3) + tuple(u.shape[1:]), dtype=u.dtype, device=dev)
            for i in range(3):
                for j in range(3):
                    bwd(1j * K[j] * uh[i], a[i][j])
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
            local = [ss.max(), ww.max(), div.abs().max(), (div * div).sum(), ss.sum(), ww.sum(), (ss * ss).sum(), (ww * ww).sum(),
                     (ss * ww).sum(), Q.sum(), R.sum(), (Q * Q).sum(), (R * R).sum(), sss.sum(), wsw.sum(), (diag ** 2).sum(),
                     (diag ** 3).sum(), (diag ** 4).sum(), (off ** 2).sum(), (off ** 4).sum()]
            parts = world.allgather_obj([float(x.item()) for x in local])
            gs = np.array([max(q[n] for q in parts) if n < 3 else sum(q[n] for q in parts) for n in range(20)])
        gm = spectral.gradient_moments(gs, npts, nu)
        if stats is not None:
            stats.update(gradients=gm)
        if verbose and world.Get_rank() == 0:
            print('  gradients: dissipation %.9e, enstrophy %.9e, skewness %.6e, flatness %.6f, Betchov ratio %.12f, rms div %.1e'
                  % (gm.dissipation, gm.enstrophy, gm.skewness, gm.flatness, gm.betchov, gm.div_rms))
        if pdfs:
            qw = float(gs[_lib.GS_WW]) / npts / 4.0           # <Q_w> = <|w|^2> / 4: the scale of the (R, Q) plane
            rq_range = ((-PDF_R * qw ** 1.5, PDF_R * qw ** 1.5), (-PDF_Q * qw, PDF_Q * qw))
            rq = ops.gradient_pdf(A, 'R', 'Q', range=rq_range, bins=PDF_BINS)          # rank-reduced; one read of A
            sigma = float(np.sqrt(gs[_lib.GS_LONG2] / (3.0 * npts)))                   # of d u_i / d x_i, pooled over i
            lrange = (-PDF_SIGMAS * sigma, PDF_SIGMAS * sigma)
            lcounts = sum(ops.histogram(A[i][i], lrange, PDF_BINS) for i in range(3))  # counts add: the pooled PDF
            table = rq[:PDF_BINS * PDF_BINS].reshape(PDF_BINS, PDF_BINS)
            h = PDF_BINS // 2                                  # bins below h: the lower half of a range (0 itself: bin h or h - 1, as t rounds)
            inside = max(int(table.sum()), 1)
            quadrants = tuple(float(q.sum()) / inside for q in (table[:h, h:], table[h:, h:], table[:h, :h], table[h:, :h]))
            if stats is not None:
                stats.update(pdfs=dict(rq=spectral.joint_pdf(rq, rq_range, PDF_BINS), rq_counts=rq, rq_range=rq_range,
                                       longitudinal=spectral.pdf(lcounts, lrange), longitudinal_counts=lcounts,
                                       longitudinal_range=lrange, quadrants=quadrants))
            if verbose and world.Get_rank() == 0:
                print('  (R, Q) table by halves of its ranges: R lower, Q upper %.4f;  R upper, Q upper %.4f;  R lower, Q lower %.4f;  R upper, Q lower %.4f  (%d of %d points outside)'
                      % (quadrants + (int(rq[-2]), npts)))
    if transfer:
        assert fused and not spectrum
        compute_rhs_fused(0.0)                                # dU = N_hat: no viscous term
        T = ops.transfer(U_hat, dU)
        if stats is not None:
            stats.update(nonlinear_energy=ops.energy(dU), helicity=ops.helicity(U_hat))
        if verbose and world.Get_rank() == 0:
            print('  transfer: sum T = %.3e, max |T| = %.3e, max |flux| = %.3e'
                  % (T[0].sum(), np.abs(T[0]).max(), np.abs(spectral.flux(T)).max()))
        FFT.destroy()
        return energy, T
    if spectrum:
        E = spectral.SpectralOps(FFT, L).spectrum(U_hat)
        if verbose and world.Get_rank() == 0:
            print('  from U_hat: energy = %.12f, enstrophy = %.12f, %d shells' % (E[0].sum(), E[1].sum(), E.shape[1]))
        FFT.destroy()
        return energy, E
    FFT.destroy()
    return energy


if __name__ == '__main__':
    from mpi4py_fft_amd import comm, spectral
    w = comm.init_distributed()
    e = solve(w, verbose=True)
    assert round(e - 0.124953117517, 7) == 0, e
    e = solve(w, verbose=True, fused=False)
    assert round(e - 0.124953117517, 7) == 0, e
    e, E = solve(w, verbose=True, spectrum=True)
    assert round(E[0].sum() - 0.124953117517, 7) == 0, E[0].sum()
    st = {}
    e, T = solve(w, verbose=True, transfer=True, stats=st)
    if w.Get_rank() == 0:
        print('  sum T = %.3e, max |Pi| = %.3e, mean helicity = %.3e (the Taylor-Green vortex has none)'
              % (T[0].sum(), np.abs(spectral.flux(T)).max(), st['helicity']))
    assert abs(T[0].sum()) <= 1e-10 * np.sqrt(e * st['nonlinear_energy']) and abs(st['helicity']) <= 1e-10 * e
    st = {}
    ea = solve(w, verbose=True, cfl=0.05, stats=st)          # CFL-controlled: about 0.004 per step instead of 0.01
    assert 0.124953117517 < ea < 0.125 and 0 < st['time'] < 0.1, (ea, st)
    if w.Get_size() == 1:
        e = solve(w, verbose=True, graph=True)
        assert round(e - 0.124953117517, 7) == 0, e
        eg = solve(w, verbose=True, graph=True, cfl=0.05, device_dt=True)
        assert eg == ea, (eg, ea)                            # the device-side step is the same arithmetic
    st = {}
    ef = solve(w, verbose=True, forcing=(0.1, 3, 3), stats=st)    # forced at the Taylor-Green shell: 0.1 x 10 x 0.01 goes in
    if w.Get_rank() == 0:
        print('  forced: energy %.9f against %.9f unforced: injected rate %.4f of eps = 0.1'
              % (ef, e, (ef - 0.124953117517) / (10 * 0.01)))
    assert 0.09 <= (ef - 0.124953117517) / (10 * 0.01) <= 0.11 and abs(2 * st['gain'] * st['band_energy'] - 0.1) <= 1e-12, (ef, st)
    if w.Get_size() == 1:
        sg = {}
        eg = solve(w, verbose=True, graph=True, forcing=(0.1, 3, 3), device_gain=True, stats=sg)
        assert abs(eg - ef) <= 1e-12 and abs(sg['gain'] - st['gain']) <= 1e-12 * st['gain'], (eg, ef, sg, st)
    ed = solve(w, verbose=True, dealias='2/3')               # 2/3-rule dealiasing fused into the projection
    eb = solve(w, verbose=True, dealias='2/3', fused=False)
    if w.Get_rank() == 0:
        print('  dealiased: energy %.12f (torch-expression baseline %.12f) against %.12f aliased' % (ed, eb, e))
    assert abs(ed - eb) <= 1e-10 and abs(ed - DEALIASED_ENERGY) <= 1e-9, (ed, eb)
    if w.Get_size() == 1:
        eg = solve(w, verbose=True, dealias='2/3', graph=True)
        assert abs(eg - ed) <= 1e-12, (eg, ed)
    ss, sb = {}, {}
    es = solve(w, verbose=True, scalar=(0.000625, (1, 0, 0)), stats=ss)      # a passive scalar against a mean gradient, kappa = nu
    eb = solve(w, verbose=True, scalar=(0.000625, (1, 0, 0)), stats=sb, fused=False)
    assert round(es - 0.124953117517, 7) == 0 and round(eb - 0.124953117517, 7) == 0, (es, eb)      # the scalar is passive
    assert abs(ss['scalar_variance'] - sb['scalar_variance']) <= 1e-10 * sb['scalar_variance'], (ss, sb)
    assert abs(ss['scalar_variance'] - SCALAR_VARIANCE) <= 1e-9 * SCALAR_VARIANCE, (ss, SCALAR_VARIANCE)
    assert max(abs(x - y) for x, y in zip(ss['scalar_flux'], sb['scalar_flux'])) <= 1e-10, (ss, sb)
    if w.Get_size() == 1:
        sg = {}
        solve(w, verbose=True, scalar=(0.000625, (1, 0, 0)), stats=sg, graph=True)
        assert abs(sg['scalar_variance'] - ss['scalar_variance']) <= 1e-12 * ss['scalar_variance'], (sg, ss)
    ei = solve(w, verbose=True, integrator='ifrk4')          # the viscous term exact, RK4 on the rest
    assert round(ei - 0.124953117517, 7) == 0 and abs(ei - IF_ENERGY) <= 1e-9, (ei, IF_ENERGY)
    si = {}
    es = solve(w, verbose=True, integrator='ifrk4', scalar=(0.000625, (1, 0, 0)), dealias='2/3', forcing=(0.1, 3, 3), stats=si)
    if w.Get_rank() == 0:
        print('  ifrk4, forced, dealiased, with a scalar: energy %.12f, scalar variance %.15f' % (es, si['scalar_variance']))
    assert 0.09 <= (es - 0.124953117517) / (10 * 0.01) <= 0.11, es
    si = {}
    solve(w, verbose=True, integrator='ifrk4', scalar=(0.000625, (1, 0, 0)), stats=si)
    assert abs(si['scalar_variance'] - SCALAR_VARIANCE) <= 1e-6 * SCALAR_VARIANCE, (si, SCALAR_VARIANCE)
    eia = solve(w, verbose=True, integrator='ifrk4', cfl=0.05)
    assert abs(eia - ea) <= 1e-7, (eia, ea)
    if w.Get_size() == 1:
        eg = solve(w, verbose=True, integrator='ifrk4', graph=True)
        assert abs(eg - ei) <= 1e-12, (eg, ei)
        eg = solve(w, verbose=True, integrator='ifrk4', graph=True, cfl=0.05, device_dt=True)
        assert eg == eia, (eg, eia)                          # the device-side step is the same arithmetic
    sf, sb = {}, {}
    solve(w, verbose=True, gradients=True, dealias='2/3', stats=sf)          # the small scales of the final state
    solve(w, verbose=True, gradients=True, dealias='2/3', stats=sb, fused=False)
    gf, gb = sf['gradients'], sb['gradients']
    assert abs(gf.skewness - gb.skewness) <= 1e-10 * abs(gf.skewness) and abs(gf.dissipation - gb.dissipation) <= 1e-10 * gf.dissipation, (gf, gb)
    assert abs(gf.skewness - GRADIENT_SKEWNESS) <= 1e-9 * abs(GRADIENT_SKEWNESS) and abs(gf.betchov - 1) <= 1e-9, (gf, GRADIENT_SKEWNESS)
    assert abs(gf.strain - gf.enstrophy) <= 1e-12 * gf.strain and gf.div_rms <= 1e-12, gf
    sp, sq = {}, {}
    ep = solve(w, verbose=True, particles=(1000, 4, 7), dealias='2/3', stats=sp)      # tracers: cubic B-splines
    solve(w, verbose=True, particles=(1000, 2, 7), dealias='2/3', stats=sq)           # ... and trilinear
    assert abs(ep - DEALIASED_ENERGY) <= 1e-9, ep                                     # tracers are passive
    assert abs(sp['particles'].sum() - PARTICLE_CHECK) <= 1e-9 * PARTICLE_CHECK, (sp['particles'].sum(), PARTICLE_CHECK)
    assert np.abs(sp['particles'] - sq['particles']).max() <= 1e-3, np.abs(sp['particles'] - sq['particles']).max()
    if w.Get_size() == 1:
        sg = {}
        solve(w, verbose=True, particles=(1000, 4, 7), dealias='2/3', stats=sg, graph=True)
        assert np.array_equal(sg['particles'], sp['particles'])
    ss = {}
    es = solve(w, verbose=True, structure=(2, 2), dealias='2/3', stats=ss)            # two-point statistics along z: one read of U
    assert abs(es - DEALIASED_ENERGY) <= 1e-9 and len(ss['structure']) == 1, (es, ss)
    mo = ss['structure'][0]['moments']
    # (the vortex is 2 pi-periodic in z in a box of 4 pi: at the largest separation, N / 2 points = 2 pi, the increments vanish to rounding)
    assert mo.longitudinal == 2 and np.all(mo.S[:-1, :2, 1] > 0) and np.all(np.isfinite(ss['structure'][0]['four_fifths'])), mo
    if len(sys.argv) > 1:                       # e.g. `dns_taylor_green.py 8` for 256^3 timings
        for f in (True, False):
            solve(w, M=int(sys.argv[1]), nsteps=5, verbose=True, fused=f)
        solve(w, M=int(sys.argv[1]), nsteps=5, verbose=True, cfl=0.5)
