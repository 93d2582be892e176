// The pseudo-spectral layer either side of the transform path: the gfft_ps_* entry points of include/gfft.h (at the end of
// the file), their launchers and their kernels, each one pass over its operands.
//   * pointwise (the reference's examples/spectral_dns_solver.py:65-91 does these with numpy expressions, one temporary per
//     operator): i K x u_hat, u x w, pressure projection + viscous term (with a band forcing and the dealiasing
//     truncation fused in where asked for), the truncation on its own, the Runge-Kutta stage update (plain, and with the integrating factor of the
//     viscous term), the time-step controller and the forcing gain; for passive
//     scalars the flux u theta and the right-hand side -i K . (u theta)^ - kappa |K|^2 theta^ - G . u^.  HBM-bound elementwise work: 16 bytes per lane, grid-stride, wavenumbers from three per-axis vectors instead
//     of three array-sized meshes (the reference's K is a (3, n0, n1, n2) float array: 1.5x the velocity);
//   * reductions, sharing one launch geometry (sp_geometry) and the stream's scratch for their per-workgroup slabs: shell sums
//     binned by |k| (ps_shell_kernel: E(k), co-spectra, helicity), physical-space statistics (ps_stats_kernel) and the
//     statistics of the velocity-gradient tensor (ps_gradient_stats_kernel, behind the pointwise ps_gradient_kernel: i K_j f_hat);
//   * histograms over the same geometry: integer counts in a workgroup's LDS table (ps_histogram_kernel: the components of a
//     real field; ps_gradient_pdf_kernel: one or two of the gradient invariants per point), summed to int64 by pd_sum_kernel;
//   * a field where no grid point is: ps_scale_axes_kernel (pointwise: a separable spectral multiplier, the B-spline prefilter)
//     and ps_interp_kernel (a gather: order^2 lanes per particle, trilinear or cubic B-spline, periodic, block by block);
//   * its transpose, particle to grid: ps_spread_kernel (a scatter with the same weights, every contribution rounded once to
//     64-bit fixed point and added by an integer atomic: order-independent to the last bit) and ps_spread_finish_kernel
//     (pointwise: the integers to reals, and the accumulator cleared);
//   * two-point statistics: ps_structure_kernel (the power sums of the increments along a grid axis at up to 64 separations:
//     tiles of whole lines staged once in LDS, the separations looped over the staged tile; fixed-order sums, sf_reduce_kernel).
#include "../../include/gfft.h"
#include "gfft_internal.h"

#include <cmath>
#include <limits>

namespace gfft {

namespace {

constexpr int PS_THREADS = 256;

inline int ps_grid(int64_t count) {
  const int64_t b = (count + PS_THREADS - 1) / PS_THREADS;
  return (int)(b < 16384 ? (b > 0 ? b : 1) : 16384);
}

// out = i (K x u): out0 = i (k1 u2 - k2 u1), out1 = i (k2 u0 - k0 u2), out2 = i (k0 u1 - k1 u0)
template <typename real>
__global__ void __launch_bounds__(PS_THREADS)
ps_curl_kernel(const cx<real> *__restrict__ u, cx<real> *__restrict__ out, const real *__restrict__ k0,
               const real *__restrict__ k1, const real *__restrict__ k2, int64_t n1, int64_t n2, int64_t count) {
  for (int64_t e = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; e < count; e += (int64_t)gridDim.x * PS_THREADS) {
    const int64_t row = e / n2;
    const real kz = k2[e - row * n2];
    const int64_t i0 = row / n1;
    const real ky = k1[row - i0 * n1], kx = k0[i0];
    const cx<real> a = u[e], b = u[e + count], c = u[e + 2 * count];
    const cx<real> w0 = {ky * c.x - kz * b.x, ky * c.y - kz * b.y};
    const cx<real> w1 = {kz * a.x - kx * c.x, kz * a.y - kx * c.y};
    const cx<real> w2 = {kx * b.x - ky * a.x, kx * b.y - ky * a.y};
    out[e] = {-w0.y, w0.x};
    out[e + count] = {-w1.y, w1.x};
    out[e + 2 * count] = {-w2.y, w2.x};
  }
}

// out = a x b on real 3-vectors stored as [3][count]
template <typename real>
__global__ void __launch_bounds__(PS_THREADS)
ps_cross_kernel(const real *__restrict__ a, const real *__restrict__ b, real *__restrict__ out, int64_t count) {
  for (int64_t e = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; e < count; e += (int64_t)gridDim.x * PS_THREADS) {
    const real a0 = a[e], a1 = a[e + count], a2 = a[e + 2 * count];
    const real b0 = b[e], b1 = b[e + count], b2 = b[e + 2 * count];
    out[e] = a1 * b2 - a2 * b1;
    out[e + count] = a2 * b0 - a0 * b2;
    out[e + 2 * count] = a0 * b1 - a1 * b0;
  }
}

// The shell of a mode: b = floor(|k| / dk + 0.5), in double from wavenumbers converted to double first (k2sq = |k|^2).  The
// ONE definition: ps_shell_kernel bins by it and the forced ps_project_kernel forces by it, so the band that is forced is
// the band whose energy the spectrum reports.  Integer-valued, or NaN for a NaN wavenumber (which compares false everywhere).
__device__ __forceinline__ double ps_k2sq(double kx, double ky, double kz) { return (kx * kx + ky * ky) + kz * kz; }

__device__ __forceinline__ double ps_shell_of(double kx, double ky, double kz, double dk, double &k2sq) {
  k2sq = ps_k2sq(kx, ky, kz);
  return floor(sqrt(k2sq) / dk + 0.5);
}

// What ps_project_kernel does to a mode after the projection and the viscous term.  A launch passes an argument pack `A`
// by value; arg.bind<real>() turns it, once per lane and before the loop, into the functor applied to every mode.
// gfft_ps_project: nothing.
struct ps_no_force {
  template <typename real> __device__ __forceinline__ ps_no_force bind() const { return *this; }
  template <typename real>
  __device__ __forceinline__ void operator()(real, real, real, real, const cx<real> &, const cx<real> &, const cx<real> &,
                                             cx<real> &, cx<real> &, cx<real> &) const {}
};

// gfft_ps_project_forced: du_c += g u_c for the modes whose shell lies in [blo, bhi].  The exact shell costs an fp64 square
// root and an fp64 divide; it is evaluated only where |k|^2 -- the `kk` the projection has already formed, in the field's
// precision -- lies in [lo2, hi2], bounds the host computes once (ps_band_bounds) so that no mode of the band fails them.
// Everywhere else the test is two compares, and the mode leaves exactly as gfft_ps_project leaves it.
template <typename real>
struct ps_band_force {
  real g, lo2, hi2;
  double dk, blo, bhi;
  __device__ __forceinline__ void operator()(real kx, real ky, real kz, real kk, const cx<real> &u0, const cx<real> &u1,
                                             const cx<real> &u2, cx<real> &d0, cx<real> &d1, cx<real> &d2) const {
    if (kk >= lo2 && kk <= hi2) {
      double k2sq;
      const double sh = ps_shell_of((double)kx, (double)ky, (double)kz, dk, k2sq);
      if (sh >= blo && sh <= bhi) {
        d0.x += g * u0.x; d0.y += g * u0.y;
        d1.x += g * u1.x; d1.y += g * u1.y;
        d2.x += g * u2.x; d2.y += g * u2.y;
      }
    }
  }
};

// g = (real)gain[0] where `gain` is given (read when the kernel runs: a captured launch follows what ps_force_gain_kernel
// wrote in front of it), else (real)gain_val -- the one conversion either way, so the same double gives the same bits.
// lo2 / hi2 arrive as doubles already representable in `real` (ps_band_bounds rounds them outwards).
struct ps_band_args {
  double dk;
  int blo, bhi;
  double lo2, hi2, gain_val;
  const double *gain;
  template <typename real> __device__ __forceinline__ ps_band_force<real> bind() const {
    return {(real)(gain ? gain[0] : gain_val), (real)lo2, (real)hi2, dk, (double)blo, (double)bhi};
  }
};

// Which modes ps_project_kernel and ps_dealias_kernel keep (dealiasing): a launch passes a predicate `M` by value.  It has two
// halves so that a kernel can put other work between them: load() fetches what the predicate needs of a mode beside its
// wavenumbers, kept() decides from that and the wavenumbers.
// gfft_ps_project, gfft_ps_project_forced: every mode; nothing is loaded or evaluated.
struct ps_keep_all {
  static constexpr bool always = true;
  struct bytes {};
  __device__ __forceinline__ bytes load(int64_t, int64_t, int64_t) const { return {}; }
  template <typename real> __device__ __forceinline__ bool kept(const bytes &, real, real, real) const { return true; }
};

// gfft_ps_project_dealiased, gfft_ps_dealias: mode (i0, i1, i2) is kept iff m0[i0] && m1[i1] && m2[i2] (a box mask in the
// sparse form of the wavenumbers: one byte per axis entry, a null vector keeps its whole axis) and |k|^2 <= kcut2, |k|^2 being
// ps_k2sq -- the double the spectrum bins by -- and kcut2 = kcut * kcut formed once on the host; the edge is inclusive and a
// NaN wavenumber fails it.  kcut2 = +inf: no spherical cut, and cuts() -- the same in every lane, so a scalar branch -- keeps
// its conversions and multiplies out of the loop.  The three bytes are loaded together, not short-circuited: two or three
// cached loads in flight cost less than branches between them.
struct ps_keep_mask {
  static constexpr bool always = false;
  const unsigned char *m0, *m1, *m2;
  double kcut2;
  struct bytes { unsigned a, b, c; };
  __device__ __forceinline__ bytes load(int64_t i0, int64_t i1, int64_t i2) const {
    return {m0 ? m0[i0] : 1u, m1 ? m1[i1] : 1u, m2 ? m2[i2] : 1u};
  }
  __device__ __forceinline__ bool cuts() const { return kcut2 < (double)INFINITY; }
  template <typename real> __device__ __forceinline__ bool kept(const bytes &m, real kx, real ky, real kz) const {
    bool k = (m.a != 0) & (m.b != 0) & (m.c != 0);
    if (cuts()) k = k & (ps_k2sq((double)kx, (double)ky, (double)kz) <= kcut2);
    return k;
  }
};

// what ps_project_kernel looks up for a mode before it touches the fields: its wavenumbers and the predicate's bytes
template <typename real, typename M> struct ps_mode { real kx, ky, kz; typename M::bytes m; };

template <typename real, typename M>
__device__ __forceinline__ ps_mode<real, M> ps_mode_of(int64_t e, int64_t n1, int64_t n2, const real *__restrict__ k0,
                                                       const real *__restrict__ k1, const real *__restrict__ k2, const M &keep) {
  const int64_t row = e / n2;
  const int64_t i2 = e - row * n2;
  const real kz = k2[i2];
  const int64_t i0 = row / n1;
  const int64_t i1 = row - i0 * n1;
  const real ky = k1[i1], kx = k0[i0];
  return {kx, ky, kz, keep.load(i0, i1, i2)};
}

// p = sum_i du_i k_i / |k|^2 (|k|^2 = 0 -> 1);  du_j -= k_j p;  du_j -= nu |k|^2 u_j;  then the mode's forcing, if any (A).
// One pass over nine component arrays either way: pointwise, grid-stride, no LDS, no atomics.
// With a keep-predicate M other than ps_keep_all the pass also dealiases: the predicate is evaluated from the three
// wavenumber lookups and the mask bytes BEFORE any load of du or u; a truncated mode loads nothing, stores +0 to its three
// du components (whatever du and u hold there, NaN included) and is done; a kept mode runs the same body as without a
// predicate.  Kept and truncated lanes share waves; whole rows and planes outside the box are waves that issue stores alone.
// The field loads of a mode can only be issued once its lookups have come back; so that the two latencies do not add up in
// every grid-stride step, the lookups of a lane's NEXT mode are issued in front of the field loads of the current one and
// are back, with those, before its stores.
// (Registers: in the list above ps_stats_kernel.)
template <typename real, typename A, typename M = ps_keep_all>
__global__ void __launch_bounds__(PS_THREADS)
ps_project_kernel(cx<real> *__restrict__ du, const cx<real> *__restrict__ u, const real *__restrict__ k0,
                  const real *__restrict__ k1, const real *__restrict__ k2, int64_t n1, int64_t n2,
                  int64_t count, real nu, A arg, M keep) {
  const auto force = arg.template bind<real>();
  const int64_t first = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * PS_THREADS;
  [[maybe_unused]] ps_mode<real, M> ahead = {};           // the lookups of the lane's next mode
  if constexpr (!M::always)
    if (first < count) ahead = ps_mode_of(first, n1, n2, k0, k1, k2, keep);
  for (int64_t e = first; e < count; e += stride) {
    const ps_mode<real, M> m = M::always ? ps_mode_of(e, n1, n2, k0, k1, k2, keep) : ahead;          // (a constant condition)
    const real kx = m.kx, ky = m.ky, kz = m.kz;
    if constexpr (!M::always) {
      if (e + stride < count) ahead = ps_mode_of(e + stride, n1, n2, k0, k1, k2, keep);
      if (!keep.kept(m.m, kx, ky, kz)) {
        du[e] = {(real)0, (real)0};
        du[e + count] = {(real)0, (real)0};
        du[e + 2 * count] = {(real)0, (real)0};
        continue;
      }
    }
    const real kk = kx * kx + ky * ky + kz * kz;
    const real inv = (real)1 / (kk == (real)0 ? (real)1 : kk);
    cx<real> d0 = du[e], d1 = du[e + count], d2 = du[e + 2 * count];
    const cx<real> u0 = u[e], u1 = u[e + count], u2 = u[e + 2 * count];
    const real px = d0.x * (kx * inv) + d1.x * (ky * inv) + d2.x * (kz * inv);
    const real py = d0.y * (kx * inv) + d1.y * (ky * inv) + d2.y * (kz * inv);
    const real v = nu * kk;
    d0.x -= px * kx;  d0.y -= py * kx;
    d1.x -= px * ky;  d1.y -= py * ky;
    d2.x -= px * kz;  d2.y -= py * kz;
    d0.x -= v * u0.x; d0.y -= v * u0.y;
    d1.x -= v * u1.x; d1.y -= v * u1.y;
    d2.x -= v * u2.x; d2.y -= v * u2.y;
    force(kx, ky, kz, kk, u0, u1, u2, d0, d1, d2);
    du[e] = d0;
    du[e + count] = d1;
    du[e + 2 * count] = d2;
  }
}

// The truncation on its own, in place on f = [ncomp][count]: +0 to every component of every mode that `keep` (above) does
// not keep.  Kept modes are neither read nor written -- no element of the field is read at all, so whatever a kept mode
// holds (a NaN, a -0, a denormal) stays --, and the wavenumbers are looked up only where there is a spherical cut.
// Pointwise, grid-stride, a lane's mode is its flat index; stores only: 16 ncomp bytes per truncated mode.
template <typename real>
__global__ void __launch_bounds__(PS_THREADS)
ps_dealias_kernel(cx<real> *__restrict__ f, int ncomp, const real *__restrict__ k0, const real *__restrict__ k1,
                  const real *__restrict__ k2, int64_t n1, int64_t n2, int64_t count, ps_keep_mask keep) {
  for (int64_t e = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; e < count; e += (int64_t)gridDim.x * PS_THREADS) {
    const int64_t row = e / n2;
    const int64_t i2 = e - row * n2;
    const int64_t i0 = row / n1;
    const int64_t i1 = row - i0 * n1;
    const ps_keep_mask::bytes m = keep.load(i0, i1, i2);
    real kx = 0, ky = 0, kz = 0;
    if (keep.cuts()) { kx = k0[i0]; ky = k1[i1]; kz = k2[i2]; }
    if (!keep.kept(m, kx, ky, kz))
      for (int c = 0; c < ncomp; ++c) f[e + c * count] = {(real)0, (real)0};
  }
}

// Runge-Kutta stage on `count` real scalars: u = u0 + cb du (if u != null); u1 += ca du
template <typename real>
__device__ __forceinline__ void ps_rk_body(real *__restrict__ u, const real *__restrict__ u0, real *__restrict__ u1,
                                           const real *__restrict__ du, int64_t count, real cb, real ca) {
  for (int64_t e = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; e < count; e += (int64_t)gridDim.x * PS_THREADS) {
    const real d = du[e];
    if (u) u[e] = u0[e] + cb * d;
    u1[e] += ca * d;
  }
}

template <typename real>
__global__ void __launch_bounds__(PS_THREADS)
ps_rk_kernel(real *__restrict__ u, const real *__restrict__ u0, real *__restrict__ u1, const real *__restrict__ du,
             int64_t count, real cb, real ca) {
  ps_rk_body(u, u0, u1, du, count, cb, ca);
}

// The same stage with the time step read from device memory: coefficients cb dt[0] and ca dt[0], the products formed in
// double and rounded to the field's precision exactly as the host path rounds (real)(cb * dt) -- the same body, so the
// result is bit for bit that of ps_rk_kernel with host-multiplied coefficients.  A captured graph replays with whatever
// dt[0] holds at that moment.
template <typename real>
__global__ void __launch_bounds__(PS_THREADS)
ps_rk_dt_kernel(real *__restrict__ u, const real *__restrict__ u0, real *__restrict__ u1, const real *__restrict__ du,
                int64_t count, double cb, double ca, const double *__restrict__ dt) {
  const double h = dt[0];
  ps_rk_body(u, u0, u1, du, count, (real)(cb * h), (real)(ca * h));
}

// ---- integrating-factor Runge-Kutta stage: the linear term -nu |K|^2 u integrated exactly ---------------------------------
// With v = exp(nu |K|^2 t) u_hat only the nonlinear term sees RK4, so nu k_max^2 h no longer limits the step.  Per mode and
// component c of a complex field [ncomp][count], kk = |k|^2 as ps_project_kernel forms it in the field's precision:
//   E = exp(-(((real)nu_c kk) hh)), hh = (real)(h / 2);   E^2 = E * E;   E^0 = the constant 1
//   u  = E^q0 u0 + (cbh E^qd) du   (skipped when u is null);   u1 = E^q1 u1 + (cah E^qa) du,   cbh = (real)(cb h), cah = (real)(ca h)
// each update one explicit fused multiply-add on a rounded product, per real part: fma(cbh E^qd, du, E^q0 u0).  With nu = 0
// every power is exactly 1 and these are the multiply-adds the compiler makes of ps_rk_body's u0 + cb d and u1 += ca d: the
// same bits.  The powers q in {0, 1, 2} are the same in every lane (selects between 1, E and E * E); a call whose powers
// are all 0 -- the last stage of IFRK4 -- evaluates no exp.  A zero mode stays zero; a factor that underflows to 0 is the
// correct result; E^0 is 1 whatever E is.
// UNIFORM (every nu_c equal: a velocity): one exp per mode for all components; otherwise one per component (several scalars
// of different Schmidt numbers in one call).  The components are taken in turn, three loads and two stores of 16 bytes
// (8 in fp32) each: the 80 bytes per complex value of ps_rk_kernel, plus three cached wavenumber lookups per mode.
// Pointwise, grid-stride, a lane's mode is its flat index; no LDS, no atomics.  (Registers: in the list above ps_stats_kernel.)
constexpr int IF_MAX_COMP = 4;

struct ps_if_nu { double v[IF_MAX_COMP]; };          // by value in the launch, as st_scale
struct ps_if_pow { int q0, qd, q1, qa; };

template <typename real> struct ps_if_step { real hh, cbh, cah; };

// The step of a launch: h = dt[0] where `dt` is given (read when the kernel runs: a captured launch follows what
// ps_timestep_kernel wrote in front of it), else h_val; the three products are formed in double and rounded once either way,
// so the same double gives the same bits.
struct ps_if_args {
  double cb, ca, h_val;
  const double *dt;
  template <typename real> __device__ __forceinline__ ps_if_step<real> bind() const {
    const double h = dt ? dt[0] : h_val;
    return {(real)(0.5 * h), (real)(cb * h), (real)(ca * h)};
  }
};

__device__ __forceinline__ float ps_exp(float x) { return expf(x); }
__device__ __forceinline__ double ps_exp(double x) { return exp(x); }
__device__ __forceinline__ float ps_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double ps_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename real>
__device__ __forceinline__ real ps_if_power(int q, real e, real e2) { return q == 0 ? (real)1 : q == 1 ? e : e2; }

template <typename real, bool UNIFORM>
__global__ void __launch_bounds__(PS_THREADS)
ps_rk_if_kernel(cx<real> *__restrict__ u, const cx<real> *__restrict__ u0, cx<real> *__restrict__ u1,
                const cx<real> *__restrict__ du, int ncomp, const real *__restrict__ k0, const real *__restrict__ k1,
                const real *__restrict__ k2, int64_t n1, int64_t n2, int64_t count, ps_if_nu nu, ps_if_pow q, ps_if_args arg) {
  const ps_if_step<real> st = arg.template bind<real>();
  const bool decays = (u && (q.q0 | q.qd)) || (q.q1 | q.qa);          // some power is not 0: the same in every lane
  for (int64_t e = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; e < count; e += (int64_t)gridDim.x * PS_THREADS) {
    real kk = 0;
    if (decays) {
      const ps_mode<real, ps_keep_all> m = ps_mode_of(e, n1, n2, k0, k1, k2, ps_keep_all());
      kk = m.kx * m.kx + m.ky * m.ky + m.kz * m.kz;
    }
    real f0 = 1, cd = st.cbh, f1 = 1, ad = st.cah;
    for (int c = 0; c < ncomp; ++c) {
      if (decays && (!UNIFORM || c == 0)) {
        const real E = ps_exp(-(((real)nu.v[c] * kk) * st.hh));
        const real E2 = E * E;
        f0 = ps_if_power(q.q0, E, E2);
        cd = st.cbh * ps_if_power(q.qd, E, E2);
        f1 = ps_if_power(q.q1, E, E2);
        ad = st.cah * ps_if_power(q.qa, E, E2);
      }
      const int64_t i = e + c * count;
      const cx<real> d = du[i], a = u1[i];
      if (u) {
        const cx<real> b = u0[i];
        u[i] = {ps_fma(cd, d.x, f0 * b.x), ps_fma(cd, d.y, f0 * b.y)};
      }
      u1[i] = {ps_fma(ad, d.x, f1 * a.x), ps_fma(ad, d.y, f1 * a.y)};
    }
  }
}

// dt[0] = clamp(cfl / stats[0], dt_min, dt_max) (dt_max where the rate is zero or not finite); dt[1] += dt[0]
__global__ void ps_timestep_kernel(const double *__restrict__ stats, double cfl, double dt_min, double dt_max,
                                   double *__restrict__ dt) {
  if (blockIdx.x || threadIdx.x) return;
  const double r = stats[0];
  const double want = (r > 0.0 && isfinite(r)) ? cfl / r : dt_max;
  const double h = fmin(fmax(want, dt_min), dt_max);
  dt[0] = h;
  dt[1] += h;
}

// E_f = spec[blo] + ... + spec[bhi] (row 0 of gfft_ps_spectrum's bins), added serially in that order;
// gain[0] = min(eps / (2 E_f), gain_max) (0 where E_f is zero, negative or not finite); gain[1] = E_f
__global__ void ps_force_gain_kernel(const double *__restrict__ spec, int blo, int bhi, double eps, double gain_max,
                                     double *__restrict__ gain) {
  if (blockIdx.x || threadIdx.x) return;
  double ef = 0.0;
  for (int b = blo; b <= bhi; ++b) ef += spec[b];
  gain[0] = (ef > 0.0 && isfinite(ef)) ? fmin(eps / (2.0 * ef), gain_max) : 0.0;
  gain[1] = ef;
}

// ---- shell sums: a per-mode value c and |k|^2 c binned by |k|, one read of each field ----------------------------------
// out[0][b] += e, out[1][b] += |k|^2 e with e = (scale w2[i2]) c and b = floor(|k| / dk + 0.5), all in double (the inputs
// are converted before any arithmetic; c may be negative: sp_wave_add and the slab sum never look at a sign).  c per mode:
//   SP_NORM      sum_comp |a_c|^2 -- at scale = 0.5 the spectrum E(k); three loads in flight for a vector field.
//                Internal: gfft_ps_spectrum passes it, gfft_ps_cospectrum refuses it like any unknown op
//   SP_DOT       sum_comp (Re a_c Re b_c + Im a_c Im b_c); the 2 x 3 loads of a vector mode are in flight together; a == b is allowed
//   SP_HELICITY  Re(conj(a) . (i K x a)) = 2 K . (Re a x Im a): three components of `a` alone, the curl is never stored
// The array is cut into contiguous chunks of flat modes, one per workgroup:
// local rows are often shorter than a wave (11 entries in the tests, N / 2P on pencils), so a lane's mode is its flat
// index, never its place in a row, and every lane looks up its own row's k0^2 + k1^2 (two cached reads).  The workgroup
// walks its chunk 256 x V modes at a time, carrying (i0, i1, i2) of the step's first mode along with 32-bit divisions
// instead of dividing a 64-bit flat index per mode.
// Shell adds: neighbouring lanes mostly hold the same shell, so each row of 16 lanes first sums its runs of equal bins
// (DPP row shifts, no LDS traffic); the last lane of a run adds the run to the workgroup's LDS histogram with the native
// fp64 LDS add.  The histogram goes to this workgroup's slab of the stream's scratch, and ps_spectrum_sum_kernel adds
// the slabs in workgroup order -- no floating-point atomics on global memory.  (Within a workgroup the waves' LDS adds
// land in arrival order: bins repeat to rounding, not bit for bit, from one launch to the next.)
// Cost per mode beside its 16 x ncomp bytes (8 x ncomp in fp32): two 32-bit divisions, an fp64 square root and an fp64
// divide, 16 DPP moves and, per run of equal shells in a row of 16 lanes, two LDS adds.  A three-component fp64 field
// has the most bytes per mode to hide that behind; a one-component fp32 field has a sixth of them and is the first
// candidate for being bound by the arithmetic instead of HBM.  tools/spectrum_probe.py measures the fp64 vector case.
// Bytes per mode double against SP_NORM for SP_DOT while the arithmetic beside them grows by three multiply-adds per
// component: of the suspects listed above, contention of the shell adds and the square root / divide weigh the same per
// mode and so half as much per byte.
constexpr int SP_MAX_WG = 2048;          // workgroups (= slabs) of one launch: 8 per CU
constexpr int SP_MAX_BINS = 4096;        // 2 x 4096 doubles = 64 KiB of LDS, what a workgroup gets without opting in to more
enum { SP_DOT = GFFT_PS_DOT, SP_HELICITY = GFFT_PS_HELICITY, SP_NORM };

template <int CTRL>
__device__ __forceinline__ double sp_dpp(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// one step of the segmented sum: take lane - D's partial sums if that lane belongs to this lane's run
template <int D>
__device__ __forceinline__ void sp_step(int lane, int start, double &e, double &f) {
  const double te = sp_dpp<0x110 + D>(e), tf = sp_dpp<0x110 + D>(f);      // row_shr:D
  if (lane - D >= start) { e += te; f += tf; }
}

// Adds (e, k2sq e) of every lane to bin b of the workgroup's histogram; b < 0 = nothing to add.  All 64 lanes call it.
__device__ __forceinline__ void sp_wave_add(double *hist, int nbins, int b, double e, double f) {
  const int lane = threadIdx.x & 63;
  const int prev = __builtin_amdgcn_mov_dpp(b, 0x111, 0xf, 0xf, false);
  const bool head = (lane & 15) == 0 || prev != b;                         // first lane of a run (runs end with their row of 16)
  const unsigned long long heads = __ballot(head);
  const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
  sp_step<1>(lane, start, e, f);
  sp_step<2>(lane, start, e, f);
  sp_step<4>(lane, start, e, f);
  sp_step<8>(lane, start, e, f);
  const bool tail = (lane & 15) == 15 || ((heads >> 1) >> lane) & 1;
  if (tail && b >= 0) {
    atomicAdd(&hist[b], e);
    atomicAdd(&hist[nbins + b], f);
  }
}

// the V modes one lane loads at once: 16 bytes, or 8 (fp32, V = 1)
template <typename real, int V> struct alignas(sizeof(cx<real>) * V) sp_load { cx<real> m[V]; };

template <typename real, int V>
__device__ __forceinline__ void sp_acc(double (&s)[V], const sp_load<real, V> &v) {
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const double x = v.m[j].x, y = v.m[j].y;          // converted before squaring
    s[j] += x * x + y * y;
  }
}

template <typename real, int V>
__device__ __forceinline__ void sp_acc_dot(double (&s)[V], const sp_load<real, V> &a, const sp_load<real, V> &b) {
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const double ar = a.m[j].x, ai = a.m[j].y, br = b.m[j].x, bi = b.m[j].y;          // converted before multiplying
    s[j] += ar * br + ai * bi;
  }
}

// V = modes per lane and load: 1 (16 B in fp64, 8 B in fp32 when a field that is read is not 16-B aligned) or 2 (fp32, 16 B)
template <typename real, int V, int OP>
__global__ void __launch_bounds__(PS_THREADS)
ps_shell_kernel(const cx<real> *__restrict__ fa, const cx<real> *__restrict__ fb, int ncomp, double scale,
                const real *__restrict__ k0, const real *__restrict__ k1, const real *__restrict__ k2,
                const real *__restrict__ w2, uint32_t n1, uint32_t n2, int64_t count, int64_t chunk, double dk,
                int nbins, double *__restrict__ slabs) {
  extern __shared__ double sp_hist[];
  for (int i = threadIdx.x; i < 2 * nbins; i += PS_THREADS) sp_hist[i] = 0.0;
  __syncthreads();
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < count ? begin + chunk : count;
  // (i0, i1, i2) of the first mode of the current step, uniform over the workgroup
  const int64_t row0 = begin / n2;
  uint32_t c0 = (uint32_t)(begin - row0 * n2);
  int64_t p0 = row0 / n1;
  uint32_t r0 = (uint32_t)(row0 - p0 * n1);
  for (int64_t base = begin; base < end; base += PS_THREADS * V) {
    const int64_t e0 = base + (int64_t)threadIdx.x * V;
    // this lane's first mode: at most (n2 + 256 V) / n2 rows and as many planes further on
    uint32_t c = c0 + threadIdx.x * V;
    uint32_t q = c / n2;
    uint32_t i2 = c - q * n2;
    q += r0;
    const uint32_t pq = q / n1;
    uint32_t i1 = q - pq * n1;
    int64_t i0 = p0 + pq;
    int b[V];
    double en[V], kk[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { b[j] = -1; en[j] = 0.0; kk[j] = 0.0; }
    if (e0 < end) {                                      // (count and chunk are multiples of V when V == 2: all V or none)
      double s[V];
#pragma unroll
      for (int j = 0; j < V; ++j) s[j] = 0.0;
      // components `count` modes apart
      const sp_load<real, V> *pa = reinterpret_cast<const sp_load<real, V> *>(fa + e0);
      const int64_t comp = count / V;
      [[maybe_unused]] sp_load<real, V> h0, h1, h2;      // SP_HELICITY: the three components, used once the wavenumbers are known
      if constexpr (OP == SP_NORM) {
        int cc = 0;
        for (; cc + 3 <= ncomp; cc += 3, pa += 3 * comp) {
          const sp_load<real, V> v0 = pa[0], v1 = pa[comp], v2 = pa[2 * comp];
          sp_acc(s, v0);
          sp_acc(s, v1);
          sp_acc(s, v2);
        }
        for (; cc < ncomp; ++cc, pa += comp) sp_acc(s, *pa);
      } else if constexpr (OP == SP_DOT) {
        const sp_load<real, V> *pb = reinterpret_cast<const sp_load<real, V> *>(fb + e0);
        int cc = 0;
        for (; cc + 3 <= ncomp; cc += 3, pa += 3 * comp, pb += 3 * comp) {
          const sp_load<real, V> a0 = pa[0], a1 = pa[comp], a2 = pa[2 * comp];
          const sp_load<real, V> b0 = pb[0], b1 = pb[comp], b2 = pb[2 * comp];
          sp_acc_dot(s, a0, b0);
          sp_acc_dot(s, a1, b1);
          sp_acc_dot(s, a2, b2);
        }
        for (; cc < ncomp; ++cc, pa += comp, pb += comp) {
          const sp_load<real, V> a0 = *pa, b0 = *pb;
          sp_acc_dot(s, a0, b0);
        }
      } else {
        h0 = pa[0];
        h1 = pa[comp];
        h2 = pa[2 * comp];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double kx = k0[i0], ky = k1[i1], kz = k2[i2];
        double k2sq;
        const double sh = ps_shell_of(kx, ky, kz, dk, k2sq);
        const double w = w2 ? (double)w2[i2] : 1.0;
        b[j] = sh < (double)nbins ? (int)sh : -1;       // (a NaN wavenumber drops the mode too)
        if constexpr (OP == SP_HELICITY) {
          const double x0 = h0.m[j].x, x1 = h1.m[j].x, x2 = h2.m[j].x;              // Re a
          const double y0 = h0.m[j].y, y1 = h1.m[j].y, y2 = h2.m[j].y;              // Im a
          s[j] = 2.0 * ((kx * (x1 * y2 - x2 * y1) + ky * (x2 * y0 - x0 * y2)) + kz * (x0 * y1 - x1 * y0));
        }
        en[j] = (scale * w) * s[j];
        kk[j] = k2sq * en[j];
        if (++i2 == n2) {                                // the pair's second mode may start the next row
          i2 = 0;
          if (++i1 == n1) { i1 = 0; ++i0; }
        }
      }
    }
    if (V == 2) {
      // the pair's modes are neighbours along i2: same shell almost always; otherwise the second goes in on its own
      if (b[V - 1] == b[0]) { en[0] += en[V - 1]; kk[0] += kk[V - 1]; }
      else if (b[V - 1] >= 0) { atomicAdd(&sp_hist[b[V - 1]], en[V - 1]); atomicAdd(&sp_hist[nbins + b[V - 1]], kk[V - 1]); }
    }
    sp_wave_add(sp_hist, nbins, b[0], en[0], kk[0]);
    // advance the step's first mode by 256 V
    c = c0 + PS_THREADS * V;
    q = c / n2;
    c0 = c - q * n2;
    q += r0;
    const uint32_t pn = q / n1;
    r0 = q - pn * n1;
    p0 += pn;
  }
  __syncthreads();
  double *slab = slabs + (int64_t)blockIdx.x * 2 * nbins;
  for (int i = threadIdx.x; i < 2 * nbins; i += PS_THREADS) slab[i] = sp_hist[i];
}

// out[i] = sum over the workgroups' slabs, in workgroup order (nwg == 0: an empty block, zeros).  One thread per output walks
// the slabs serially, eight loads in flight: at most 2048 x 16 nbins bytes, nothing beside u_hat at 1024^3, but a
// latency-bound tail on small arrays -- unmeasured; a fixed-order tree over more threads is the remedy if it shows.
__global__ void __launch_bounds__(PS_THREADS)
ps_spectrum_sum_kernel(const double *__restrict__ slabs, int nwg, int n, double *__restrict__ out) {
  const int i = blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
#pragma unroll 8
  for (int w = 0; w < nwg; ++w) s += slabs[(int64_t)w * n + i];
  out[i] = s;
}

// ---- physical-space statistics: CFL rate, extrema and the first four power sums, one read of u --------------------------
// u = [NC][count] reals, components `count` apart.  NVAL = 2 + 6 NC doubles, every value converted before any arithmetic:
//   [0] max over points of sum_c |u_c| inv_dx[c]      [1] max over points of sum_c u_c^2
//   [2 + 6c + 0..5] max u_c, min u_c, sum u_c, sum u_c^2, sum (u u) u, sum (u u)(u u)
// Geometry (that of the shell kernels): 256-lane workgroups, at most SP_MAX_WG, each owning one contiguous chunk of whole
// steps of 256 V points; a lane loads 16 bytes per component (V = 2 in fp64, 4 in fp32; V = 1 where count % V != 0 or
// the base is not 16-byte aligned), the NC loads of a point in flight together.  NC is a template parameter so that the
// NVAL accumulators of a lane are registers (an array indexed by a runtime component would live in scratch memory).
// Summation order -- fixed, so the result repeats bit for bit for the same array, count and alignment:
//   1. a lane combines its own points in index order (the V of a load, then step after step);
//   2. the 64 lanes of a wave by the butterfly lane ^ 32, 16, 8, 4, 2, 1 (both partners form the same a + b);
//   3. the 4 waves of a workgroup through LDS, in wave order; the result goes to slot [value][workgroup] of the slabs;
//   4. st_reduce_kernel, one workgroup per value: lane t combines slabs t, t + 256, ... in that order, then 2. and 3.
// No floating-point atomics.  Sums propagate a NaN (the blow-up signal); max / min are fmax / fmin and ignore it, so
// [0] and [1] skip a point whose rate or square is NaN.
// Cost per value beside its bytes: a conversion and 11 fp64 operations; no divide, no square root, no LDS in the loop.
// Registers (hipcc -O3, gfx950; no instantiation spills or uses scratch): ps_stats_kernel<double, 2, 3> 70 VGPRs,
// <float, 4, 3> 70, <double, 2, 4> 90, <float, 4, 4> 98 (the largest), <double, 1, 3> 62, <float, 1, 3> 58;
// st_reduce_kernel 12, ps_rk_dt_kernel 14 / 10 (double / float), ps_timestep_kernel 13;
// ps_project_kernel<double / float, ps_band_args> (the forced projection) 64 / 50 against 58 / 42 unforced, ps_force_gain_kernel 12;
// ps_project_kernel<double / float, ., ps_keep_mask> (the dealiased projection) 70 / 50 unforced and 76 / 60 forced -- the
// next mode's lookups are live across the body: 7 and 6 waves per SIMD in fp64, 8 in fp32 --, ps_dealias_kernel 24 / 23.
// ps_scalar_flux_kernel<double, 2, NS = 1 ... 4> 28, 44, 58, 58 and <float, 4, NS> 28, 44, 58, 60; one element per lane: 16 ... 54;
// ps_scalar_rhs_kernel<double / float, NS, mean gradient?, mask?>, every instantiation 8 waves per SIMD but <double, 2, yes, no>:
//   NS = 1: 36 / 26 plain, 48 / 38 with the gradient, 48 / 34 masked, 60 / 46 with both;   NS = 2: 56 / 40, 66 / 56 (7 waves in
//   fp64), 52 / 50, 64 / 56;   NS = 3 and 4 (the scalars in turn): 40 / 26, 52 / 34, 46 / 36, 60 / 42.
// ps_rk_if_kernel<double / float, UNIFORM> 72 / 44 (7 and 8 waves per SIMD), <double / float, per component> 60 / 30 (8 waves).
// ps_gradient_kernel<double, NC = 1 ... 4> 40, 50, 66, 64 (7 waves per SIMD at NC = 3, else 8) and <float, NC> 28, 40, 48, 54;
// ps_gradient_stats_kernel<double, 2> 112 and <float, 4> 128 (4 waves per SIMD), <double, 1> 90, <float, 1> 90 (5 waves); gs_reduce_kernel 11.
// ps_histogram_kernel<double, 2, NC = 1 ... 4> 54, 58, 60, 64 and <float, 4, NC> the same (8 waves per SIMD), one element per lane 54 ... 64;
// ps_gradient_pdf_kernel<double, 2, 1-D / joint> 78 / 84 (6 / 5 waves per SIMD) and <float, 4, .> 92 / 98 (5 / 4 waves), <., 1, .> 58 / 62 (8 waves);
// pd_sum_kernel 48 (8 waves).
// ps_structure_kernel<double, 2, NC = 1 ... 4> 56, 76, 96, 117 and <float, 4, NC> 56, 76, 94, 116 (8, 6, 5, 4 waves per SIMD by registers;
// its LDS tile allows 2 workgroups = 2 waves per SIMD), one element per staging load 54 / 74 / 94 / 115 and 54 / 74 / 94 / 114; sf_reduce_kernel 9.
constexpr int ST_MAX_COMP = 4;
constexpr int ST_HEAD = GFFT_PS_STATS_HEAD, ST_PER_COMP = GFFT_PS_STATS_PER_COMP;
enum { ST_MAX0 = 0, ST_MAX = 1, ST_MIN = 2, ST_SUM = 3 };

struct st_scale { double v[ST_MAX_COMP]; };          // inv_dx, by value in the launch

__host__ __device__ constexpr int st_kind(int i) {
  return i < ST_HEAD ? ST_MAX0 : (i - ST_HEAD) % ST_PER_COMP == 0 ? ST_MAX : (i - ST_HEAD) % ST_PER_COMP == 1 ? ST_MIN : ST_SUM;
}

__device__ __forceinline__ double st_identity(int kind) {
  return kind == ST_MAX ? -INFINITY : kind == ST_MIN ? INFINITY : 0.0;
}

__device__ __forceinline__ double st_combine(int kind, double a, double b) {
  return kind == ST_SUM ? a + b : kind == ST_MIN ? fmin(a, b) : fmax(a, b);
}

// step 2 of the order: afterwards every lane of the wave holds the wave's value
__device__ __forceinline__ double st_wave(int kind, double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = st_combine(kind, v, __shfl_xor(v, off));
  return v;
}

// the V points one lane loads from one component: 16 bytes, or one scalar
template <typename real, int V> struct alignas(sizeof(real) * V) st_load { real m[V]; };

template <typename real, int V, int NC>
__global__ void __launch_bounds__(PS_THREADS)
ps_stats_kernel(const real *__restrict__ u, int64_t count, int64_t chunk, st_scale inv, double *__restrict__ slabs) {
  constexpr int NVAL = ST_HEAD + ST_PER_COMP * NC;
  __shared__ double st_part[PS_THREADS / 64][NVAL];
  double val[NVAL];
#pragma unroll
  for (int i = 0; i < NVAL; ++i) val[i] = st_identity(st_kind(i));
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < count ? begin + chunk : count;
  // (count and chunk are multiples of V: a lane has all V points of a load or none)
  for (int64_t e0 = begin + (int64_t)threadIdx.x * V; e0 < end; e0 += PS_THREADS * V) {
    st_load<real, V> v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = *reinterpret_cast<const st_load<real, V> *>(u + c * count + e0);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      double rate = 0.0, sq = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const double x = v[c].m[j];                    // converted before any arithmetic
        const double xx = x * x;
        double *a = val + ST_HEAD + ST_PER_COMP * c;
        rate += fabs(x) * inv.v[c];
        sq += xx;
        a[0] = fmax(a[0], x);
        a[1] = fmin(a[1], x);
        a[2] += x;
        a[3] += xx;
        a[4] += xx * x;
        a[5] += xx * xx;
      }
      val[0] = fmax(val[0], rate);
      val[1] = fmax(val[1], sq);
    }
  }
#pragma unroll
  for (int i = 0; i < NVAL; ++i) {
    const double w = st_wave(st_kind(i), val[i]);
    if ((threadIdx.x & 63) == 0) st_part[threadIdx.x >> 6][i] = w;
  }
  __syncthreads();
  if (threadIdx.x < NVAL) {
    const int i = threadIdx.x, kind = st_kind(i);
    double r = st_part[0][i];
    for (int w = 1; w < PS_THREADS / 64; ++w) r = st_combine(kind, r, st_part[w][i]);
    slabs[(int64_t)i * SP_MAX_WG + blockIdx.x] = r;
  }
}

// out[i] = the nwg workgroup values of slot i combined in the fixed order above; workgroup i of the launch owns value i
// (nwg == 0, an empty block: the identities 0, -inf, +inf, 0).  At most 8 dependent loads per lane, not 2048.
// (KIND: the kind map of the caller's values -- st_kind here, gs_kind for the gradient statistics)
// (stride: the slots of one value in the slabs -- SP_MAX_WG, or what ps_structure_kernel's launch used)
template <int (*KIND)(int)>
__device__ __forceinline__ void st_reduce_value(const double *__restrict__ slabs, int nwg, double *__restrict__ out,
                                                int stride = SP_MAX_WG) {
  __shared__ double part[PS_THREADS / 64];
  const int i = blockIdx.x, kind = KIND(i);
  double r = st_identity(kind);
  for (int w = threadIdx.x; w < nwg; w += PS_THREADS) r = st_combine(kind, r, slabs[(int64_t)i * stride + w]);
  r = st_wave(kind, r);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    r = part[0];
    for (int w = 1; w < PS_THREADS / 64; ++w) r = st_combine(kind, r, part[w]);
    out[i] = r;
  }
}

__global__ void __launch_bounds__(PS_THREADS)
st_reduce_kernel(const double *__restrict__ slabs, int nwg, double *__restrict__ out) {
  st_reduce_value<st_kind>(slabs, nwg, out);
}

// ---- passive scalars: d theta / dt + div(u theta) = kappa lap theta - G . u, NS <= SC_MAX scalars per launch --------------
// The flux form (u . grad theta = div(u theta) for solenoidal u) costs the four transforms per scalar of the gradient form
// and stores no gradient; its pointwise work is the two kernels below.  NS is a template parameter, as NC is of
// ps_stats_kernel, so that nothing is indexed at run time; the velocity is read ONCE for all NS scalars.
// (Registers: in the list above ps_stats_kernel.)
// Measured on one MI355X (tools/scalar_probe.py, 256^3 fp64, HIP events after a warm-up, minimum of 15 rounds), achieved bytes
// per second against gfft_probe_copy in the same run (6.08 TB/s), one scalar / three scalars:
//   ps_scalar_flux_kernel                      5.52 / 5.11 TB/s = 0.91 / 0.84 of the copy
//   ps_scalar_rhs_kernel, mean gradient        4.55 / 4.80 TB/s = 0.75 / 0.79      without it 5.02 / 4.95 = 0.83 / 0.81
//   ps_scalar_rhs_kernel, gradient + 2/3 mask  4.24 / 4.41 TB/s = 0.70 / 0.73 of the bytes it does move, in 0.41 / 0.45 of the
//                                              unmasked pass's time
// flux + rhs take 0.41 / 0.90 ms against 1.37 / 4.16 ms for the array-sized torch expressions of the example: 3.4x / 4.6x.
// The right-hand side sits a fifth to a quarter below the copy -- 8 to 19 streams per lane against the copy's two; not tuned.
constexpr int SC_MAX = 4;

// flux[s][c][e] = u[c][e] * theta[s][e]: one multiply, so the correctly rounded product.  3 + NS loads and 3 NS stores per
// point, V points (16 bytes, or one scalar: ps_lane_width) per lane, load and store; grid-stride.  flux overlaps no input.
template <typename real, int V, int NS>
__global__ void __launch_bounds__(PS_THREADS)
ps_scalar_flux_kernel(const real *__restrict__ u, const real *__restrict__ theta, real *__restrict__ flux, int64_t count) {
  using vec = st_load<real, V>;
  const int64_t nvec = count / V;                        // (count is a multiple of V)
  for (int64_t i = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * PS_THREADS) {
    const int64_t e = i * V;
    vec a[3], t[NS];
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = *reinterpret_cast<const vec *>(u + c * count + e);
#pragma unroll
    for (int s = 0; s < NS; ++s) t[s] = *reinterpret_cast<const vec *>(theta + s * count + e);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        vec f;
#pragma unroll
        for (int j = 0; j < V; ++j) f.m[j] = a[c].m[j] * t[s].m[j];
        *reinterpret_cast<vec *>(flux + (s * 3 + c) * count + e) = f;
      }
    }
  }
}

struct sc_coef { double kappa[SC_MAX], grad[SC_MAX][3]; };          // by value in the launch, as st_scale

// Per mode and scalar s, in the field's precision, kk = |k|^2 as ps_project_kernel forms it:
//   a = kx F[s][0] + ky F[s][1] + kz F[s][2];   d[s] = -i a - (kappa[s] kk) theta[s] - (G[s][0] u0 + G[s][1] u1 + G[s][2] u2)
// F = flux [NS][3][count], theta and d = [NS][count], u = [3][count]; d overlaps no input.  The mean-gradient term is the
// instantiation MG: without it u is not a kernel operand that is ever loaded; with it u is loaded once per mode for all
// NS scalars.  One pass: 4 NS (+ 3) complex loads and NS stores per mode.  One or two scalars are unrolled, their loads in
// flight together; three and four are processed in turn (a loop over s: four loads in flight, kappa[s] and G[s] scalar loads
// from the launch's arguments) -- unrolled, the masked instantiations of three and four scalars ran out of scalar registers
// for the 16 + 3 + 4 array bases and the coefficients and spilled them; in turn every instantiation keeps 7 or 8 waves per SIMD.
// The keep-predicate M, its evaluation before any load of the mode, the +0 stores of a truncated mode and the look-ahead of
// the lane's next mode are those of ps_project_kernel, for the reasons given there.
template <typename real, int NS, bool MG, typename M>
__global__ void __launch_bounds__(PS_THREADS)
ps_scalar_rhs_kernel(cx<real> *__restrict__ d, const cx<real> *__restrict__ flux, const cx<real> *__restrict__ theta,
                     const cx<real> *__restrict__ u, const real *__restrict__ k0, const real *__restrict__ k1,
                     const real *__restrict__ k2, int64_t n1, int64_t n2, int64_t count, sc_coef coef, M keep) {
  constexpr int TURNS = NS <= 2 ? NS : 1;                 // the unroll count of the loop over the scalars
  const int64_t first = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * PS_THREADS;
  [[maybe_unused]] ps_mode<real, M> ahead = {};           // the lookups of the lane's next mode
  if constexpr (!M::always)
    if (first < count) ahead = ps_mode_of(first, n1, n2, k0, k1, k2, keep);
  for (int64_t e = first; e < count; e += stride) {
    const ps_mode<real, M> m = M::always ? ps_mode_of(e, n1, n2, k0, k1, k2, keep) : ahead;          // (a constant condition)
    const real kx = m.kx, ky = m.ky, kz = m.kz;
    if constexpr (!M::always) {
      if (e + stride < count) ahead = ps_mode_of(e + stride, n1, n2, k0, k1, k2, keep);
      if (!keep.kept(m.m, kx, ky, kz)) {
#pragma unroll
        for (int s = 0; s < NS; ++s) d[e + s * count] = {(real)0, (real)0};
        continue;
      }
    }
    const real kk = kx * kx + ky * ky + kz * kz;
    [[maybe_unused]] cx<real> u0, u1, u2;                // held in registers over the scalars
    if constexpr (MG) { u0 = u[e]; u1 = u[e + count]; u2 = u[e + 2 * count]; }
#pragma unroll TURNS
    for (int s = 0; s < NS; ++s) {
      const cx<real> *__restrict__ f = flux + e + 3 * s * count;
      const cx<real> f0 = f[0], f1 = f[count], f2 = f[2 * count], th = theta[e + s * count];
      const real ax = kx * f0.x + ky * f1.x + kz * f2.x;
      const real ay = kx * f0.y + ky * f1.y + kz * f2.y;
      const real v = (real)coef.kappa[s] * kk;
      cx<real> r = {ay - v * th.x, -ax - v * th.y};
      if constexpr (MG) {
        const real g0 = (real)coef.grad[s][0], g1 = (real)coef.grad[s][1], g2 = (real)coef.grad[s][2];
        r.x -= g0 * u0.x + g1 * u1.x + g2 * u2.x;
        r.y -= g0 * u0.y + g1 * u1.y + g2 * u2.y;
      }
      d[e + s * count] = r;
    }
  }
}

// ---- the velocity-gradient tensor: A_ij = d u_i / d x_j in spectral space, and one read of it in physical space --------------
// out[c][j][e] = i k_j f[c][e] = {-(k_j f.y), k_j f.x}: one multiply per part, so the correctly rounded product, the sign of
// a zero included.  f = [NC][count] modes, out = [NC][3][count]; NC loads and 3 NC stores per mode and the three cached
// wavenumber lookups of ps_curl_kernel, a lane's mode its flat index, grid-stride; out overlaps nothing.  K is applied as given (the
// convention of ps_curl_kernel): nothing special happens in a Nyquist column, which the 2/3 mask removes.  NC is a template
// parameter as NS is of ps_scalar_flux_kernel; all NC <= 4 loads of a mode are in flight together.  (Registers: in the list above ps_stats_kernel.)
// A single field (NC = 1) takes TWO modes per lane and step, a grid stride apart, both loads in flight before the first
// store: with one 16-byte load per lane the fp64 form was bound by latency, not bytes -- 3.49 TB/s = 0.62 of the copy, two
// tenths below its yardstick, its median a quarter above its minimum --; with two it runs level with it (below).
// Measured on one MI355X (tools/gradient_probe.py, 256^3, HIP events after a warm-up, minimum of 15 rounds), achieved bytes per
// second against gfft_probe_copy in the same run (6.04 TB/s), fp64 / fp32:
//   ps_gradient_kernel, one field      4.89 / 4.94 TB/s = 0.81 / 0.82 of the copy
//   ps_gradient_kernel, three fields   4.91 / 5.25 TB/s = 0.81 / 0.87                (ps_scalar_flux_kernel, three scalars, same run: 0.80 / 0.86)
//   ps_gradient_stats_kernel + reduce  4.18 / 3.70 TB/s = 0.69 / 0.61                (ps_stats_kernel, three components, same run: 0.61 / 0.54)
// 0.33 ms against 0.48 ms for the nine torch products of a velocity, 0.29 ms against 124 ms for the 20 numbers as torch expressions.
template <typename real, int NC>
__global__ void __launch_bounds__(PS_THREADS)
ps_gradient_kernel(const cx<real> *__restrict__ f, cx<real> *__restrict__ out, const real *__restrict__ k0,
                   const real *__restrict__ k1, const real *__restrict__ k2, int64_t n1, int64_t n2, int64_t count) {
  constexpr int U = NC == 1 ? 2 : 1;          // modes per lane and step: a single field has two loads in flight, not one
  const int64_t stride = (int64_t)gridDim.x * PS_THREADS;
  for (int64_t e0 = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; e0 < count; e0 += U * stride) {
    real kx[U], ky[U], kz[U];
    cx<real> v[U][NC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e = e0 + u * stride;
      if (e < count) {
        const int64_t row = e / n2;
        kz[u] = k2[e - row * n2];
        const int64_t i0 = row / n1;
        ky[u] = k1[row - i0 * n1];
        kx[u] = k0[i0];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[u][c] = f[e + c * count];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e = e0 + u * stride;
      if (e < count) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          cx<real> *__restrict__ o = out + e + 3 * c * count;
          o[0] = {-(kx[u] * v[u][c].y), kx[u] * v[u][c].x};
          o[count] = {-(ky[u] * v[u][c].y), ky[u] * v[u][c].x};
          o[2 * count] = {-(kz[u] * v[u][c].y), kz[u] * v[u][c].x};
        }
      }
    }
  }
}

// A = [3][3][count] reals, a_ij = A[3 i + j] converted to double before any arithmetic.  The GS_NVAL = 20 values, their
// expressions and associations: include/gfft.h (gfft_ps_gradient_stats).  Geometry, summation order (steps 1 - 4), NaN
// behaviour and scratch are those of ps_stats_kernel: 16 bytes per lane and component (V = 2 in fp64, 4 in fp32; V = 1 where
// count % V != 0 or the base is not 16-byte aligned), the nine loads of a step in flight together, the V points of a load
// processed in turn; slot [value][workgroup] of the slabs, then gs_reduce_kernel.  Values 0 - 2 are maxima of non-negative
// numbers with the identity 0 (ST_MAX0), the rest sums: an empty block gives zeros.
// Cost per point beside its 72 bytes (36 in fp32): nine conversions and about 110 fp64 operations -- ten times what
// ps_stats_kernel does per value, 1.5 (fp64) and 3 (fp32) operations per byte of HBM traffic.  Measured (above
// ps_gradient_kernel): it runs at the rate of ps_stats_kernel all the same, the arithmetic hidden behind the loads.
// Registers (in the list above ps_stats_kernel): 20 accumulators (40 VGPRs) and 9 V loaded values (36) leave room for one
// point's temporaries only if the V points are taken IN TURN.  Left to itself the scheduler interleaves them -- 166 VGPRs in
// fp64 and 256 in fp32, 3 and 2 waves per SIMD --, so a scheduling barrier closes every point, and an empty asm on each loaded
// value keeps the conversions of the later points from being hoisted over it: 112 and 128 VGPRs, 4 waves per SIMD.
constexpr int GS_NVAL = GFFT_PS_GRAD_NVAL, GS_NMAX = 3;
static_assert(GS_NVAL <= ST_HEAD + ST_PER_COMP * ST_MAX_COMP, "the slabs fit the scratch that gfft_ps_stats asks for");

__host__ __device__ constexpr int gs_kind(int i) { return i < GS_NMAX ? ST_MAX0 : ST_SUM; }

// one point: a[3 i + j] = A_ij
__device__ __forceinline__ void gs_point(double (&val)[GS_NVAL], const double (&a)[9]) {
  const double a00 = a[0], a01 = a[1], a02 = a[2], a10 = a[3], a11 = a[4], a12 = a[5], a20 = a[6], a21 = a[7], a22 = a[8];
  const double div = (a00 + a11) + a22;
  const double s01 = 0.5 * (a01 + a10), s02 = 0.5 * (a02 + a20), s12 = 0.5 * (a12 + a21);
  const double w0 = a21 - a12, w1 = a02 - a20, w2 = a10 - a01;
  const double q00 = a00 * a00, q11 = a11 * a11, q22 = a22 * a22;
  const double d2 = (q00 + q11) + q22;
  const double p01 = s01 * s01, p02 = s02 * s02, p12 = s12 * s12;
  const double ss = d2 + 2.0 * ((p01 + p02) + p12);
  const double ww = (w0 * w0 + w1 * w1) + w2 * w2;
  const double Q = 0.5 * (div * div - (d2 + 2.0 * ((a01 * a10 + a02 * a20) + a12 * a21)));
  const double R = -((a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20)) + a02 * (a10 * a21 - a11 * a20));
  const double d3 = (a00 * q00 + a11 * q11) + a22 * q22;
  const double sss = (d3 + 3.0 * ((a00 * (p01 + p02) + a11 * (p01 + p12)) + a22 * (p02 + p12))) + 6.0 * ((s01 * s02) * s12);
  const double wsw = ((a00 * (w0 * w0) + a11 * (w1 * w1)) + a22 * (w2 * w2)) +
                     2.0 * ((s01 * (w0 * w1) + s02 * (w0 * w2)) + s12 * (w1 * w2));
  const double o01 = a01 * a01, o10 = a10 * a10, o02 = a02 * a02, o20 = a20 * a20, o12 = a12 * a12, o21 = a21 * a21;
  val[0] = fmax(val[0], ss);
  val[1] = fmax(val[1], ww);
  val[2] = fmax(val[2], fabs(div));
  val[3] += div * div;
  val[4] += ss;
  val[5] += ww;
  val[6] += ss * ss;
  val[7] += ww * ww;
  val[8] += ss * ww;
  val[9] += Q;
  val[10] += R;
  val[11] += Q * Q;
  val[12] += R * R;
  val[13] += sss;
  val[14] += wsw;
  val[15] += d2;
  val[16] += d3;
  val[17] += (q00 * q00 + q11 * q11) + q22 * q22;
  val[18] += ((o01 + o10) + (o02 + o20)) + (o12 + o21);
  val[19] += ((o01 * o01 + o10 * o10) + (o02 * o02 + o20 * o20)) + (o12 * o12 + o21 * o21);
}

template <typename real, int V>
__global__ void __launch_bounds__(PS_THREADS)
ps_gradient_stats_kernel(const real *__restrict__ A, int64_t count, int64_t chunk, double *__restrict__ slabs) {
  __shared__ double gs_part[PS_THREADS / 64][GS_NVAL];
  double val[GS_NVAL];
#pragma unroll
  for (int i = 0; i < GS_NVAL; ++i) val[i] = st_identity(gs_kind(i));
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < count ? begin + chunk : count;
  // (count and chunk are multiples of V: a lane has all V points of a load or none)
  for (int64_t e0 = begin + (int64_t)threadIdx.x * V; e0 < end; e0 += PS_THREADS * V) {
    st_load<real, V> v[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) v[c] = *reinterpret_cast<const st_load<real, V> *>(A + c * count + e0);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      double a[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        real x = v[c].m[j];
        asm volatile("" : "+v"(x));                                    // (keeps the conversions of a later point behind the barrier)
        a[c] = x;                                                      // converted before any arithmetic
      }
      gs_point(val, a);
      __builtin_amdgcn_sched_barrier(0);                               // one point after the other: see above
    }
  }
#pragma unroll
  for (int i = 0; i < GS_NVAL; ++i) {
    const double w = st_wave(gs_kind(i), val[i]);
    if ((threadIdx.x & 63) == 0) gs_part[threadIdx.x >> 6][i] = w;
  }
  __syncthreads();
  if (threadIdx.x < GS_NVAL) {
    const int i = threadIdx.x, kind = gs_kind(i);
    double r = gs_part[0][i];
    for (int w = 1; w < PS_THREADS / 64; ++w) r = st_combine(kind, r, gs_part[w][i]);
    slabs[(int64_t)i * SP_MAX_WG + blockIdx.x] = r;
  }
}

// st_reduce_kernel's step 4 with the kind map of the gradient statistics: workgroup i owns value i; nwg == 0, an empty block:
// the identities, all 0
__global__ void __launch_bounds__(PS_THREADS)
gs_reduce_kernel(const double *__restrict__ slabs, int nwg, double *__restrict__ out) {
  st_reduce_value<gs_kind>(slabs, nwg, out);
}

// ---- one-pass PDFs: histograms of a real field and (joint) histograms of the gradient invariants -------------------------
// Counts are integers: the result is exact, independent of arrival order, bit for bit repeatable and additive over ranks.
// The bin rule (include/gfft.h), for x converted to double before any arithmetic and w = (double)nbins / (hi - lo) formed ONCE
// on the host:  t = (x - lo) * w;  x NaN -> the NaN slot;  t < 0 -> below;  t >= nbins -> above (+inf and a value within
// rounding of hi included: the upper edge is exclusive);  otherwise bin (int)t.  A subtraction followed by a multiply cannot
// be contracted: one defined sequence of IEEE operations.  pd_bin returns the slot: 0 ... nbins - 1, nbins (below),
// nbins + 1 (above), nbins + 2 (NaN) -- a bin index is < nbins by the comparison itself, never by a clamp.
// Geometry: that of ps_stats_kernel (256 lanes, one contiguous chunk of whole steps of 256 V points per workgroup, 16 bytes
// per lane and component; V = 1 where count % V != 0 or the base is not 16-byte aligned), except that a table beyond
// 4096 counters takes fewer workgroups (pd_max_wg: 512 at the 16384 counters of a 128 x 128 joint table -- two 64 KiB
// tables are resident per CU, and the slabs stay a fortieth of the bytes of A at 256^3 instead of a tenth).
// Counting: the bins are 32-bit counters in the workgroup's LDS table, bumped by no-return LDS integer adds (ds_add_u32);
// the tails (below / above / NaN, or outside / NaN of a joint table) are lane registers, combined once at the end through
// the then idle table.  A workgroup counts at most its chunk, which the entry points keep below 2^32 points
// (GFFT_ERR_UNSUPPORTED beyond: count >= 2^32 x pd_max_wg, 2^41 points at the fewest workgroups).
// Workgroup tables go to slabs [workgroup][counters + tails] in the stream's scratch (at most 2048 x (4096 + 12) or 512 x
// (16384 + 2) 32-bit words, 32.1 MiB: a quarter of the 128 MiB gfft_ps_spectrum asks for at ITS bin limit; at equal bins a
// four-component table asks for the spectrum's 32768 nbins bytes plus 96 KiB of tails) and pd_sum_kernel adds them to int64
// and OVERWRITES d_out.  Chosen over 64-bit atomics on d_out behind a
// zeroing step: the slab route is the one the shell sums already take (one scratch, no memset node in a captured graph),
// its cost is a fixed number of streamed bytes, and 2048 workgroups hitting the 259 words of a small table with device-scope
// atomics is exactly the same-address traffic the LDS table exists to avoid.  No floating-point atomics anywhere.
// Per-point quantities of the gradient PDFs: gp_quantity, the expressions of gs_point with FMA contraction switched OFF, so
// each is exactly the IEEE double sequence written in gfft.h (what tests/gradient_ref.pointwise computes); only the
// quantities named by the call are evaluated (a workgroup-uniform switch per point), A is read once, all nine components.
// Measured on one MI355X (tools/pdf_probe.py, 256^3, HIP events after a warm-up, minimum of 15 rounds; in brackets eight
// calls back to back between one pair of events, per call -- a single call also pays what the host spends between the
// first event and the launch), fp64 / fp32, the copy of the same run at 5.90 TB/s:
//   (a) histogram, m = 3, 256 bins, normal field   0.157 / 0.111 ms (0.113 / 0.078)      gfft_ps_stats, same array:          0.097 / 0.060 ms (0.081 / 0.054)
//   (b) the same, constant field (worst case)      0.226 / 0.220 ms (0.207 / 0.207)
//   (c) gradient_pdf, Q, 256 bins                  0.263 / 0.156 ms (0.246 / 0.150)      gfft_ps_gradient_stats, same array: 0.217 / 0.125 ms (0.211 / 0.120)
//   (c) gradient_pdf, (R, Q), 128 x 128            0.242 / 0.139 ms (0.227 / 0.131)
//   (d) torch on the device: histc x 3 43.2 / 0.35 ms; Q as expressions + histc 19.5 / 2.6 ms; R, Q + an index expression +
//       bincount 4.9 / 3.6 ms (torch.histogramdd has no device kernel)
// (a) is 1.4 x the moment kernel back to back (1.6 - 1.9 x as single calls), (c) 1.1 - 1.25 x.  What bounded the first
// form was not the counting: pd_sum_kernel walked 2048 slabs with 8 loads in flight per lane, 75 us whatever the precision
// ((a) 0.201 / 0.161 ms then, (c) Q 0.306 / 0.200); see its comment.
// Contention: the LDS adds of lanes that hit one counter serialise, (b) against (a).  Both remedies were built, measured in
// the same probe (kernels alone, fp64 / fp32; the plain add in that run (a) 0.136 / 0.102, (b) 0.229 / 0.228) and taken out again:
//   a copy of the table per wave (tables up to 4096 counters), added up at the flush
//              (a) 0.139 / 0.108  (b) 0.251 / 0.251 -- the conflict is between the lanes of one wave, not between waves: no gain
//   runs of equal bins within a row of 16 lanes counted by their last lane (the scheme of sp_wave_add; a DPP move, a ballot, a subtraction)
//              (a) 0.139 / 0.119  (b) 0.139 / 0.117 -- the worst case falls to the common one, which pays 2 / 17 % for it;
//              (c) is unchanged either way (one add per point beside ~100 fp64 operations)
// Kept: one add per lane and value -- (b) is the recorded worst case, a field of one value, and stays within 2.6 x (fp64)
// and 4 x (fp32) of the moment kernel; a real PDF's peak holds a few per cent of the points.  The merge is the one to take
// up again if a caller's fields are mostly constant (DESIGN_HISTORY.md 6g).
constexpr int PD_MAX_BINS = 4096, PD_MAX_COUNTERS = 16384;          // 64 KiB of 32-bit counters: the LDS a workgroup gets without opting in
constexpr int PD_MAX_TAILS = GFFT_PS_PDF_TAIL * ST_MAX_COMP;        // 12: the table is never allocated smaller than this
static_assert(PD_MAX_BINS == SP_MAX_BINS && PD_MAX_COUNTERS * sizeof(uint32_t) == 2 * SP_MAX_BINS * sizeof(double), "the LDS of the shell kernels");

struct pd_ranges { double lo[ST_MAX_COMP], w[ST_MAX_COMP]; };       // by value in the launch

__device__ __forceinline__ int pd_bin(double x, double lo, double w, int nbins) {
  const double t = (x - lo) * w;
  return x != x ? nbins + 2 : t < 0.0 ? nbins : t >= (double)nbins ? nbins + 1 : (int)t;
}

// the words of LDS a table of ncounters takes
__host__ __device__ constexpr int pd_words(int ncounters) { return ncounters > PD_MAX_TAILS ? ncounters : PD_MAX_TAILS; }

// the table (ncounters words) to this workgroup's slab, then the NT tails of the lanes behind it
template <int NT>
__device__ __forceinline__ void pd_flush(uint32_t *__restrict__ tab, int ncounters, const uint32_t (&tail)[NT],
                                         uint32_t *__restrict__ slabs) {
  __syncthreads();
  uint32_t *slab = slabs + (int64_t)blockIdx.x * (ncounters + NT);
  for (int i = threadIdx.x; i < ncounters; i += PS_THREADS) slab[i] = tab[i];
  __syncthreads();
  if (threadIdx.x < NT) tab[threadIdx.x] = 0;          // (the table holds at least PD_MAX_TAILS words)
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NT; ++i)
    if (tail[i]) atomicAdd(&tab[i], tail[i]);
  __syncthreads();
  if (threadIdx.x < NT) slab[ncounters + threadIdx.x] = tab[threadIdx.x];
}

// u = [NC][count] reals; table [NC][nbins], tails [NC][below, above, NaN]
template <typename real, int V, int NC>
__global__ void __launch_bounds__(PS_THREADS)
ps_histogram_kernel(const real *__restrict__ u, int64_t count, int64_t chunk, pd_ranges rg, int nbins, uint32_t *__restrict__ slabs) {
  extern __shared__ uint32_t pd_table[];
  const int ncounters = NC * nbins;
  for (int i = threadIdx.x; i < pd_words(ncounters); i += PS_THREADS) pd_table[i] = 0;
  __syncthreads();
  uint32_t tail[GFFT_PS_PDF_TAIL * NC];
#pragma unroll
  for (int i = 0; i < GFFT_PS_PDF_TAIL * NC; ++i) tail[i] = 0;
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < count ? begin + chunk : count;
  // (count and chunk are multiples of V: a lane has all V points of a load or none)
  for (int64_t e0 = begin + (int64_t)threadIdx.x * V; e0 < end; e0 += PS_THREADS * V) {
    st_load<real, V> v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = *reinterpret_cast<const st_load<real, V> *>(u + c * count + e0);
#pragma unroll
    for (int j = 0; j < V; ++j) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const double x = v[c].m[j];                    // converted before any arithmetic
        const int b = pd_bin(x, rg.lo[c], rg.w[c], nbins);
        if (b < nbins) atomicAdd(&pd_table[c * nbins + b], 1u);
        tail[3 * c + 0] += b == nbins;
        tail[3 * c + 1] += b == nbins + 1;
        tail[3 * c + 2] += b == nbins + 2;
      }
    }
  }
  pd_flush(pd_table, ncounters, tail, slabs);
}

// One quantity of one point, a[3 i + j] = A_ij: the expressions and associations of gs_point (include/gfft.h), every
// operation rounded on its own -- contraction is off in this function, and stays off where it is inlined.
__device__ __forceinline__ double gp_quantity(int q, const double (&a)[9]) {
#pragma clang fp contract(off)
  const double a00 = a[0], a01 = a[1], a02 = a[2], a10 = a[3], a11 = a[4], a12 = a[5], a20 = a[6], a21 = a[7], a22 = a[8];
  switch (q) {
    case GFFT_PS_Q_DIV:
      return (a00 + a11) + a22;
    case GFFT_PS_Q_WW: {
      const double w0 = a21 - a12, w1 = a02 - a20, w2 = a10 - a01;
      return (w0 * w0 + w1 * w1) + w2 * w2;
    }
    case GFFT_PS_Q_Q: {
      const double div = (a00 + a11) + a22;
      const double d2 = (a00 * a00 + a11 * a11) + a22 * a22;
      return 0.5 * (div * div - (d2 + 2.0 * ((a01 * a10 + a02 * a20) + a12 * a21)));
    }
    case GFFT_PS_Q_R:
      return -((a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20)) + a02 * (a10 * a21 - a11 * a20));
    default:
      break;
  }
  const double s01 = 0.5 * (a01 + a10), s02 = 0.5 * (a02 + a20), s12 = 0.5 * (a12 + a21);
  const double p01 = s01 * s01, p02 = s02 * s02, p12 = s12 * s12;
  const double q00 = a00 * a00, q11 = a11 * a11, q22 = a22 * a22;
  if (q == GFFT_PS_Q_SS) return ((q00 + q11) + q22) + 2.0 * ((p01 + p02) + p12);
  if (q == GFFT_PS_Q_SSS) {
    const double d3 = (a00 * q00 + a11 * q11) + a22 * q22;
    return (d3 + 3.0 * ((a00 * (p01 + p02) + a11 * (p01 + p12)) + a22 * (p02 + p12))) + 6.0 * ((s01 * s02) * s12);
  }
  const double w0 = a21 - a12, w1 = a02 - a20, w2 = a10 - a01;          // GFFT_PS_Q_WSW
  return ((a00 * (w0 * w0) + a11 * (w1 * w1)) + a22 * (w2 * w2)) + 2.0 * ((s01 * (w0 * w1) + s02 * (w0 * w2)) + s12 * (w1 * w2));
}

// A = [3][3][count] reals.  JOINT: table [nbx][nby], tails [outside, NaN] (NaN wins); else table [nbx], tails [below, above, NaN]
struct gp_axis { int q; double lo, w; int nbins; };

template <typename real, int V, bool JOINT>
__global__ void __launch_bounds__(PS_THREADS)
ps_gradient_pdf_kernel(const real *__restrict__ A, int64_t count, int64_t chunk, gp_axis ax, gp_axis ay, uint32_t *__restrict__ slabs) {
  extern __shared__ uint32_t pd_table[];
  constexpr int NT = JOINT ? 2 : GFFT_PS_PDF_TAIL;
  const int ncounters = JOINT ? ax.nbins * ay.nbins : ax.nbins;
  for (int i = threadIdx.x; i < pd_words(ncounters); i += PS_THREADS) pd_table[i] = 0;
  __syncthreads();
  uint32_t tail[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) tail[i] = 0;
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < count ? begin + chunk : count;
  // (count and chunk are multiples of V: a lane has all V points of a load or none)
  for (int64_t e0 = begin + (int64_t)threadIdx.x * V; e0 < end; e0 += PS_THREADS * V) {
    st_load<real, V> v[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) v[c] = *reinterpret_cast<const st_load<real, V> *>(A + c * count + e0);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      double a[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) a[c] = v[c].m[j];            // converted before any arithmetic
      const int bx = pd_bin(gp_quantity(ax.q, a), ax.lo, ax.w, ax.nbins);
      if constexpr (JOINT) {
        const int by = pd_bin(gp_quantity(ay.q, a), ay.lo, ay.w, ay.nbins);
        const bool nan = bx == ax.nbins + 2 || by == ay.nbins + 2;
        const bool in = bx < ax.nbins && by < ay.nbins;
        if (in) atomicAdd(&pd_table[bx * ay.nbins + by], 1u);
        tail[0] += !in && !nan;
        tail[1] += nan;
      } else {
        if (bx < ax.nbins) atomicAdd(&pd_table[bx], 1u);
        tail[0] += bx == ax.nbins;
        tail[1] += bx == ax.nbins + 1;
        tail[2] += bx == ax.nbins + 2;
      }
    }
  }
  pd_flush(pd_table, ncounters, tail, slabs);
}

// The slabs [nwg][nrow * rowlen + nrow * ntail] added over the workgroups into out = int64 [nrow][rowlen + ntail], OVERWRITTEN
// (nwg == 0, an empty block: zeros).  A workgroup owns 16 outputs; its sixteen rows of 16 lanes take every sixteenth slab each
// (64 contiguous bytes per row and slab), sixteen loads in flight, and meet in LDS: 128 loads per lane in 8 rounds at 2048
// slabs.  This kernel is latency, not bytes (6 MiB of slabs for a 3 x 256 table): with 32 outputs x 8 rows and eight loads in
// flight (32 rounds) it cost 75 us at 256^3, as much as the counting itself -- measured, tools/pdf_probe.py, the difference
// to gfft_ps_stats being the same 75 us in fp64 and fp32.  Integer sums: the order does not matter.
constexpr int PD_SUM_OUT = 16, PD_SUM_ROWS = PS_THREADS / PD_SUM_OUT;
__global__ void __launch_bounds__(PS_THREADS)
pd_sum_kernel(const uint32_t *__restrict__ slabs, int nwg, int nrow, int rowlen, int ntail, int64_t *__restrict__ out) {
  __shared__ unsigned long long part[PD_SUM_ROWS][PD_SUM_OUT];
  const int n = nrow * (rowlen + ntail), table = nrow * rowlen;
  const int o = threadIdx.x % PD_SUM_OUT, r = threadIdx.x / PD_SUM_OUT;
  const int i = blockIdx.x * PD_SUM_OUT + o;
  unsigned long long s = 0;
  if (i < n) {
#pragma unroll 16
    for (int w = r; w < nwg; w += PD_SUM_ROWS) s += slabs[(int64_t)w * n + i];
  }
  part[r][o] = s;
  __syncthreads();
  if (r == 0 && i < n) {
    for (int k = 1; k < PD_SUM_ROWS; ++k) s += part[k][o];
    const int row = i < table ? i / rowlen : (i - table) / ntail;
    const int col = i < table ? i - row * rowlen : rowlen + (i - table) - row * ntail;
    out[(int64_t)row * (rowlen + ntail) + col] = (int64_t)s;
  }
}

// ---- the fields where no grid point is: a separable spectral multiplier and the B-spline gather ----------------------------
// out[c][e] = f[c][e] * g with g = (v0[i0] * v1[i1]) * v2[i2] formed in the field's precision; a null vector contributes no
// factor (no multiply by 1), all three null: a copy.  Each part of each value is ONE multiply by g, and g at most two: a
// defined sequence of single multiplies with nothing to contract, so any host restates it bit for bit.  The B-spline
// prefilter of gfft_ps_interp is one such g (SpectralOps.bspline_vectors); a Gaussian or a box filter is another.
// NC loads and NC stores per mode in the mould of ps_gradient_kernel (a lane's mode its flat index, the three cached vector
// lookups of ps_curl_kernel, grid-stride); V modes per lane: 16 bytes per load and store -- one mode in fp64, two in fp32
// where n2 is even (a pair then shares its row) and both bases are 16-byte aligned, else one.  A lane reads all its values
// before it stores any, and no other lane touches them: out may BE f (in place); any other overlap is the caller's error.
// (Registers, hipcc -O3, gfx950: ps_scale_axes_kernel<double, 1, NC = 1 ... 4> 21, 26, 42, 40 VGPRs; <float, 2, NC> 23, 24, 29, 34;
// <float, 1, NC> 21, 21, 26, 27 -- 8 waves per SIMD, no scratch.)
constexpr int SA_MAX_COMP = 4;

template <typename real, int V, int NC>
__global__ void __launch_bounds__(PS_THREADS)
ps_scale_axes_kernel(cx<real> *out, const cx<real> *f, const real *__restrict__ v0, const real *__restrict__ v1,
                     const real *__restrict__ v2, int64_t n1, int64_t n2, int64_t count) {
  using vec = st_load<real, 2 * V>;
  const int64_t nvec = count / V;                        // (count is a multiple of V)
  for (int64_t i = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * PS_THREADS) {
    const int64_t e = i * V;
    const int64_t row = e / n2, i2 = e - row * n2;
    const int64_t i0 = row / n1;
    bool has = false;
    real g01 = 0;
    if (v0) { g01 = v0[i0]; has = true; }
    if (v1) { const real b = v1[row - i0 * n1]; g01 = has ? g01 * b : b; has = true; }
    real g[V];
#pragma unroll
    for (int j = 0; j < V; ++j) g[j] = v2 ? (has ? g01 * v2[i2 + j] : v2[i2 + j]) : g01;
    const bool any = has || v2;
    vec a[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = *reinterpret_cast<const vec *>(f + c * count + e);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      vec o = a[c];
      if (any) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          o.m[2 * j] = a[c].m[2 * j] * g[j];
          o.m[2 * j + 1] = a[c].m[2 * j + 1] * g[j];
        }
      }
      *reinterpret_cast<vec *>(out + c * count + e) = o;
    }
  }
}

// gfft_ps_interp: trilinear (ORDER 2) or cubic B-spline (ORDER 4) interpolation of NC <= 4 real fields at np positions; the
// definition, operation by operation, is in include/gfft.h.  A GROUP of ORDER^2 lanes (4 or 16: whole groups per wave) serves
// one particle: lane (j0, j1) of the group owns one row of the stencil and loads its ORDER last-axis values for every
// component -- ORDER NC independent loads per lane, ORDER^2 NC lines in flight per particle --, forms its partial sum in
// double in the order j2 = 0, 1, ..., and the group adds the partial sums by the butterfly lane ^ ORDER^2 / 2, ..., 2, 1 (both
// partners form the same a + b): one fixed order, so the result repeats bit for bit.  Every lane of a group derives the same
// base cell and fraction from the same position (redundant arithmetic instead of a broadcast).  Groups stride over the
// particles; lane 0 of a group stores its NC results.  No atomics, no LDS, nothing between workgroups.
//
// What keeps every load inside the block, whatever the position holds:
//   1. s = x * inv_dx passes !(fabs(s) < 2^51) -> the particle's results are NaN and the group loads NOTHING.  This comes
//      BEFORE the conversion to an integer: NaN, +-inf and anything without a fraction never reach it.
//   2. otherwise floor(s) is an integer of magnitude <= 2^51, exact in int64, and b + j cannot overflow;
//   3. ip_wrap brings it to g in [0, N) by the integer remainder, made non-negative; ip_next steps g + 1 with the wrap, which
//      is (b + j) mod N for every j (also where N < ORDER: the stencil wraps onto itself);
//   4. l = g - start is tested 0 <= l < n on all three axes, per element, and ONLY a point that passed is added.  The index of
//      a load is SELECTED between two values: the sum of three tested l's, inside [0, n0 n1 n2) of its component, and the
//      constant 0 -- element 0 of the component, which exists because every n >= 1 (the entry point refuses less) -- for a
//      point outside the block, whose value is then dropped.  The select instead of a branch keeps the ORDER NC loads of a
//      lane independent and in flight together: with a branch around each load the compiler waited for one load before it
//      issued the next (a wait per load in the assembly), and the random-order gather ran at the latency of ORDER loads in turn.
// A particle none of whose points lies in the block gets +0.0 (the sum of nothing).
// (Registers, hipcc -O3, gfx950: ps_interp_kernel<double, NC = 1 ... 4, ORDER 4> 38, 48, 54, 64 VGPRs and <float, NC, 4> 36, 38, 42,
// 50; <double, NC, ORDER 2> 36, 36, 35, 44 and <float, NC, 2> 36, 36, 38, 44: every instantiation 8 waves per SIMD, none spills or
// uses scratch.)
constexpr int IP_MAX_COMP = 4;
struct ip_dims { int64_t n[3], start[3], N[3]; double inv_dx[3]; };          // by value in the launch

__device__ __forceinline__ int64_t ip_wrap(int64_t b, int64_t N) {
  if (b >= 0 && b < N) return b;                         // a particle inside the box: no division
  const int64_t r = b % N;
  return r < 0 ? r + N : r;
}

__device__ __forceinline__ int64_t ip_next(int64_t g, int64_t N) { return g + 1 == N ? 0 : g + 1; }

// weight j of the stencil at fraction t in [0, 1] (j is a lane's own index: selected, never indexed)
template <int ORDER>
__device__ __forceinline__ double ip_weight(int j, double t) {
  const double r = 1.0 - t;
  if (ORDER == 2) return j == 0 ? r : t;
  const double sixth = 1.0 / 6.0;
  const double wa = ((r * r) * r) * sixth, wd = ((t * t) * t) * sixth;
  const double wb = ((t * t) * (3.0 * t - 6.0) + 4.0) * sixth, wc = ((r * r) * (3.0 * r - 6.0) + 4.0) * sixth;
  return j == 0 ? wa : j == 1 ? wb : j == 2 ? wc : wd;
}

template <typename real, int NC, int ORDER>
__global__ void __launch_bounds__(PS_THREADS)
ps_interp_kernel(const real *__restrict__ c, ip_dims d, const double *__restrict__ x, int64_t np, double *__restrict__ out) {
  constexpr int G = ORDER * ORDER;                       // lanes per particle
  const int lane = threadIdx.x % G, j0 = lane / ORDER, j1 = lane % ORDER;
  const int64_t cnt = d.n[0] * d.n[1] * d.n[2];
  const int64_t stride = (int64_t)gridDim.x * (PS_THREADS / G);
  for (int64_t p = (int64_t)blockIdx.x * (PS_THREADS / G) + threadIdx.x / G; p < np; p += stride) {
    const double s0 = x[3 * p] * d.inv_dx[0], s1 = x[3 * p + 1] * d.inv_dx[1], s2 = x[3 * p + 2] * d.inv_dx[2];
    const double lim = 2251799813685248.0;               // 2^51
    const bool good = fabs(s0) < lim && fabs(s1) < lim && fabs(s2) < lim;          // (false for a NaN)
    double acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = 0.0;
    if (good) {                                          // (the same on every lane of the group)
      const double f0 = floor(s0), f1 = floor(s1), f2 = floor(s2);
      const double w01 = ip_weight<ORDER>(j0, s0 - f0) * ip_weight<ORDER>(j1, s1 - f1);
      const double t2 = s2 - f2;
      const int64_t shift = ORDER == 4 ? 1 : 0;
      int64_t g0 = ip_wrap((int64_t)f0 - shift, d.N[0]), g1 = ip_wrap((int64_t)f1 - shift, d.N[1]);
      int64_t g2 = ip_wrap((int64_t)f2 - shift, d.N[2]);
#pragma unroll
      for (int j = 1; j < ORDER; ++j) {
        if (j <= j0) g0 = ip_next(g0, d.N[0]);
        if (j <= j1) g1 = ip_next(g1, d.N[1]);
      }
      const int64_t l0 = g0 - d.start[0], l1 = g1 - d.start[1];
      const bool row_in = l0 >= 0 && l0 < d.n[0] && l1 >= 0 && l1 < d.n[1];
      const int64_t base = row_in ? (l0 * d.n[1] + l1) * d.n[2] : 0;
      bool in[ORDER];
      real v[NC][ORDER];
#pragma unroll
      for (int j = 0; j < ORDER; ++j) {
        const int64_t l2 = g2 - d.start[2];
        in[j] = row_in && l2 >= 0 && l2 < d.n[2];
        const int64_t at = in[j] ? base + l2 : 0;        // tested, or element 0 of the component (n >= 1: it exists); see 4.
#pragma unroll
        for (int k = 0; k < NC; ++k) v[k][j] = c[k * cnt + at];
        g2 = ip_next(g2, d.N[2]);
      }
#pragma unroll
      for (int j = 0; j < ORDER; ++j) {
        const double w = w01 * ip_weight<ORDER>(j, t2);
#pragma unroll
        for (int k = 0; k < NC; ++k)
          if (in[j]) acc[k] += w * (double)v[k][j];
      }
    }
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) {
#pragma unroll
      for (int k = 0; k < NC; ++k) acc[k] += __shfl_xor(acc[k], off);
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < NC; ++k) out[p * NC + k] = good ? acc[k] : (double)NAN;
    }
  }
}

// ---- particle to grid: the transpose of the gather, in 64-bit fixed point ------------------------------------------------
// gfft_ps_spread: every particle adds ((w0 w1) w2) (q 2^scale_exp), rounded ONCE to an integer, to the ORDER^3 stencil points of
// each of its NC <= 4 components; the definition, operation by operation, is in include/gfft.h.  The adds are 64-bit INTEGER
// atomics (atomicAdd on unsigned long long, result unused: one no-return global_atomic_add_x2 each, agent scope, no
// compare-and-swap loop), and integer addition is associative: the accumulator does not depend on the order of the adds, of
// the particles or on the cut into blocks, and a host restates it bit for bit.  No floating-point atomic, no LDS, no scratch.
// Contraction is OFF in this kernel and in spr_weight: each product, sum and difference of the definition is rounded on its own
// (the only fused operations in the assembly belong to the conversions between double and int64).
// A GROUP of ORDER^2 lanes (4 or 16) serves one particle, groups stride over the particles (the geometry of ps_interp_kernel).
// Lane (j1, j2) of the group, j2 fastest, loops over j0: the ORDER lanes of a stencil row add to ORDER consecutive 8-byte words
// -- 16 or 32 contiguous bytes where the row does not wrap --, ORDER NC adds per lane.  Measured against the mapping of
// ps_interp_kernel (lane (j0, j1) looping over j2: 64 lanes of a wave instruction in 64 different rows), 256^3, 2^20 particles in
// random order, m = 3: 0.66 against 1.12 ms (order 2) and 2.94 against 8.61 ms (order 4); that mapping was taken out.
// What keeps every add inside the block is what keeps ps_interp_kernel's loads there: the 2^51 guard BEFORE the conversion to
// an integer, ip_wrap / ip_next, and the block test 0 <= l < n on all three axes per point; a point outside the block is
// skipped by a branch (an add has no value to drop).  The guard on u = q 2^scale_exp (|u| < 2^62) keeps the conversion of w u
// (0 <= w <= 1) inside int64.  A skipped particle is counted once, by lane 0 of its group.
// (Registers, hipcc -O3, gfx950: ps_spread_kernel<NC = 1 ... 4, ORDER 4> 37, 40, 42, 46 VGPRs, <NC, ORDER 2> 35, 37, 37, 41: 8 waves per SIMD;
// ps_spread_finish_kernel at most 26; none spills or uses scratch, none uses LDS.)
constexpr int SPR_MAX_COMP = 4;

template <int ORDER>
__device__ __forceinline__ double spr_weight(int j, double t) {
#pragma clang fp contract(off)
  const double r = 1.0 - t;
  if (ORDER == 2) return j == 0 ? r : t;
  const double sixth = 1.0 / 6.0;
  const double wa = ((r * r) * r) * sixth, wd = ((t * t) * t) * sixth;
  const double wb = ((t * t) * (3.0 * t - 6.0) + 4.0) * sixth, wc = ((r * r) * (3.0 * r - 6.0) + 4.0) * sixth;
  return j == 0 ? wa : j == 1 ? wb : j == 2 ? wc : wd;
}

template <int NC, int ORDER>
__global__ void __launch_bounds__(PS_THREADS)
ps_spread_kernel(unsigned long long *acc, ip_dims d, const double *__restrict__ x, const double *__restrict__ q, int64_t np,
                 double scale, unsigned long long *skipped) {
#pragma clang fp contract(off)
  constexpr int G = ORDER * ORDER;                       // lanes per particle
  const int lane = threadIdx.x % G, j1 = lane / ORDER, j2 = lane % ORDER;
  const int64_t cnt = d.n[0] * d.n[1] * d.n[2];
  const int64_t stride = (int64_t)gridDim.x * (PS_THREADS / G);
  for (int64_t p = (int64_t)blockIdx.x * (PS_THREADS / G) + threadIdx.x / G; p < np; p += stride) {
    const double s0 = x[3 * p] * d.inv_dx[0], s1 = x[3 * p + 1] * d.inv_dx[1], s2 = x[3 * p + 2] * d.inv_dx[2];
    const double lim = 2251799813685248.0;               // 2^51
    bool good = fabs(s0) < lim && fabs(s1) < lim && fabs(s2) < lim;          // (false for a NaN)
    double u[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      u[k] = q[p * NC + k] * scale;
      good = good && fabs(u[k]) < 4611686018427387904.0;          // 2^62
    }
    if (!good) {                                         // (the same on every lane of the group; before any block test)
      if (lane == 0) atomicAdd(skipped, 1ull);
      continue;
    }
    const double f0 = floor(s0), f1 = floor(s1), f2 = floor(s2);
    const double t0 = s0 - f0;
    const int64_t shift = ORDER == 4 ? 1 : 0;
    int64_t g0 = ip_wrap((int64_t)f0 - shift, d.N[0]), g1 = ip_wrap((int64_t)f1 - shift, d.N[1]);
    int64_t g2 = ip_wrap((int64_t)f2 - shift, d.N[2]);
#pragma unroll
    for (int j = 1; j < ORDER; ++j) {
      if (j <= j1) g1 = ip_next(g1, d.N[1]);
      if (j <= j2) g2 = ip_next(g2, d.N[2]);
    }
    const int64_t l1 = g1 - d.start[1], l2 = g2 - d.start[2];
    const bool row_in = l1 >= 0 && l1 < d.n[1] && l2 >= 0 && l2 < d.n[2];
    const double w1 = spr_weight<ORDER>(j1, s1 - f1), w2 = spr_weight<ORDER>(j2, s2 - f2);
#pragma unroll
    for (int j = 0; j < ORDER; ++j) {
      const int64_t l0 = g0 - d.start[0];
      const double w = (spr_weight<ORDER>(j, t0) * w1) * w2;
      if (row_in && l0 >= 0 && l0 < d.n[0]) {            // every index below is tested: inside [0, cnt) of its component
        const int64_t at = (l0 * d.n[1] + l1) * d.n[2] + l2;
#pragma unroll
        for (int k = 0; k < NC; ++k) atomicAdd(acc + k * cnt + at, (unsigned long long)__double2ll_rn(w * u[k]));
      }
      g0 = ip_next(g0, d.N[0]);
    }
  }
}

// out[i] = (real)((double)acc[i] * factor), then acc[i] = 0 where `clear`: one conversion, one multiply, for fp32 one
// narrowing.  Pointwise, grid-stride; V values per lane: 16 bytes of out (2 doubles, 4 floats) from 16-byte loads of acc where
// both bases are 16-byte aligned, else one.  The count % V values behind the last whole vector go to the first lanes of the grid.
template <typename real, int V>
__global__ void __launch_bounds__(PS_THREADS)
ps_spread_finish_kernel(real *__restrict__ out, int64_t *__restrict__ acc, int64_t count, double factor, int clear) {
  const int64_t nvec = count / V, gid = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if constexpr (V > 1) {
    using pair = st_load<int64_t, 2>;
    for (int64_t i = gid; i < nvec; i += (int64_t)gridDim.x * PS_THREADS) {
      const int64_t e = i * V;
      pair a[V / 2];
#pragma unroll
      for (int j = 0; j < V / 2; ++j) a[j] = *reinterpret_cast<const pair *>(acc + e + 2 * j);
      st_load<real, V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.m[j] = (real)((double)a[j / 2].m[j % 2] * factor);
      *reinterpret_cast<st_load<real, V> *>(out + e) = o;
      if (clear) {
        pair z;
        z.m[0] = z.m[1] = 0;
#pragma unroll
        for (int j = 0; j < V / 2; ++j) *reinterpret_cast<pair *>(acc + e + 2 * j) = z;
      }
    }
  }
  const int64_t first = V > 1 ? nvec * V + gid : gid, step = V > 1 ? count : (int64_t)gridDim.x * PS_THREADS;
  for (int64_t i = first; i < count; i += step) {        // V > 1: at most V - 1 values, one lane each
    out[i] = (real)((double)acc[i] * factor);
    if (clear) acc[i] = 0;
  }
}

// ---- random fields: a counter-based generator keyed by the GLOBAL mode index ------------------------------------------------
// gfft_ps_random_field; the definition, operation by operation, is in include/gfft.h.  A mode's value is a function of its
// global index, the seed and the stream alone: not of the block it lies in, of the lane that forms it or of the precision
// before the one rounding at the store.  A mode and its mirror draw from the SAME counter (the smaller of their two linear
// indices) and the wavenumbers enter only through products of two of them, so the mirror's value is bit for bit the conjugate.
// Pointwise, grid-stride over the block, a lane's modes V neighbours along i2 (16 bytes per store: one mode in fp64, two in
// fp32 where n2 is even and the base is 16-byte aligned, else one); no LDS, no atomics, no scratch.  Everything between the
// Philox words and the store is double, and the projection is compiled without contraction: one defined sequence of roundings
// in every instantiation, so the fp32 field is the fp64 field rounded once.
// Without `project` the components are taken in turn (ncomp at run time, one log / sqrt / sincospi chain live); with it the
// three of a mode are live together.  The launch is capped at RF_MAX_WG workgroups, 8 per CU: the arithmetic, not the stores,
// is what a lane spends its time on, so a lane walks several modes rather than the grid growing with the block.
// (Registers, hipcc -O3, gfx950: ps_random_field_kernel<double, 1, projected / plain> 66 / 78 VGPRs, <float, 1, .> 66 / 78,
// <float, 2, .> 98 / 92 -- 7 / 6 and 4 / 5 waves per SIMD; no instantiation uses scratch or spills a VGPR; the projected ones park 42 to 57
// scalar registers in lanes of a VGPR.  ps_scale_shells_kernel<double, 1, NC = 1 ... 4> 26, 28, 30, 34, <float, 2, NC> 32, 32, 38, 44,
// <float, 1, NC> 26, 28, 26, 26: 8 waves per SIMD.)
constexpr int RF_MAX_COMP = 4;
constexpr int RF_MAX_WG = 2048;

struct rf_dims { int64_t n1, n2, s0, s1, s2, N0, N1, N2; };          // block rows, block offset, global grid

// counter words 2 and 3 without the component, and the key
struct rf_key { uint32_t s_lo, s_hi4, k0, k1; };

// Philox4x32-10 (Salmon et al. 2011): ten rounds, the key bumped between them
__device__ __forceinline__ void rf_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// 52 bits of (hi, lo) as the centre of one of 2^52 equal cells of (0, 1): exact, never 0 or 1
__device__ __forceinline__ double rf_uniform(uint32_t lo, uint32_t hi) {
  return ((double)((((uint64_t)hi << 32) | lo) >> 12) + 0.5) * 0x1p-52;
}

// what a lane knows of a mode before it draws: whether it is stored as zero, whether it is the mirror of its pair, the
// pair's counter, its wavenumbers and |k|^2 in double, and its amplitude
struct rf_mode { bool zero, mirror; uint32_t c_lo, c_hi; double kx, ky, kz, kk, a; };

template <typename real>
__device__ __forceinline__ rf_mode rf_mode_of(int64_t e, const rf_dims &d, const real *__restrict__ k0, const real *__restrict__ k1,
                                              const real *__restrict__ k2, double dk, const double *__restrict__ amp, int nbins) {
  const int64_t row = e / d.n2;
  const int64_t i2 = e - row * d.n2;
  const int64_t i0 = row / d.n1;
  const int64_t i1 = row - i0 * d.n1;
  const uint64_t g0 = d.s0 + i0, g1 = d.s1 + i1, g2 = d.s2 + i2;
  const uint64_t m0 = g0 ? d.N0 - g0 : 0, m1 = g1 ? d.N1 - g1 : 0, m2 = g2 ? d.N2 - g2 : 0;
  const uint64_t lg = (g0 * d.N1 + g1) * d.N2 + g2, lm = (m0 * d.N1 + m1) * d.N2 + m2;
  const uint64_t c = lm < lg ? lm : lg;
  rf_mode m;
  m.mirror = lm < lg;
  m.c_lo = (uint32_t)c;
  m.c_hi = (uint32_t)(c >> 32);
  m.zero = (g0 | g1 | g2) == 0 || 2 * g0 == (uint64_t)d.N0 || 2 * g1 == (uint64_t)d.N1 || 2 * g2 == (uint64_t)d.N2;
  m.kx = m.ky = m.kz = m.kk = 0.0;
  m.a = 1.0;
  if (!m.zero) {
    m.kx = (double)k0[i0], m.ky = (double)k1[i1], m.kz = (double)k2[i2];
    const double sh = ps_shell_of(m.kx, m.ky, m.kz, dk, m.kk);
    if (!(sh < (double)nbins)) m.zero = true;            // (a NaN shell too)
    else if (amp) {
      m.a = amp[(int)sh];
      if (m.a == 0.0) m.zero = true;
    }
  }
  return m;
}

// the complex standard normal pair of (mode, component): Box-Muller on the two uniforms of one Philox call
__device__ __forceinline__ void rf_gauss(const rf_mode &m, const rf_key &key, int comp, double &gr, double &gi) {
  uint32_t r[4];
  rf_philox(m.c_lo, m.c_hi, key.s_lo, key.s_hi4 | (uint32_t)comp, key.k0, key.k1, r);
  const double u1 = rf_uniform(r[0], r[1]), u2 = rf_uniform(r[2], r[3]);
  const double rho = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(2.0 * u2, &s, &c);
  gr = rho * c;
  gi = rho * s;
}

// G <- G - K (K . G) / |K|^2 on one part (real or imaginary) of the three components, in double, nothing contracted
__device__ __forceinline__ void rf_project(const rf_mode &m, double &a, double &b, double &c) {
#pragma clang fp contract(off)
  const double kk = m.kk == 0.0 ? 1.0 : m.kk;
  const double p = ((m.kx * a + m.ky * b) + m.kz * c) / kk;
  a = a - m.kx * p;
  b = b - m.ky * p;
  c = c - m.kz * p;
}

// the store of V neighbouring modes of one component: `v` holds (re, im) per mode in double, already scaled and conjugated
template <typename real, int V>
__device__ __forceinline__ void rf_store(cx<real> *p, const double (&v)[2 * V], const bool (&zero)[V], bool any, bool add) {
  using vec = st_load<real, 2 * V>;
  vec o;
  if (add) {
    if (!any) return;                                    // every mode of the vector is a zeroed one: untouched
    o = *reinterpret_cast<const vec *>(p);
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (!zero[j]) {
        o.m[2 * j] = o.m[2 * j] + (real)v[2 * j];
        o.m[2 * j + 1] = o.m[2 * j + 1] + (real)v[2 * j + 1];
      }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o.m[2 * j] = zero[j] ? (real)0 : (real)v[2 * j];
      o.m[2 * j + 1] = zero[j] ? (real)0 : (real)v[2 * j + 1];
    }
  }
  *reinterpret_cast<vec *>(p) = o;
}

template <typename real, int V, bool PROJECT>
__global__ void __launch_bounds__(PS_THREADS)
ps_random_field_kernel(cx<real> *__restrict__ out, int ncomp, rf_dims d, const real *__restrict__ k0, const real *__restrict__ k1,
                       const real *__restrict__ k2, double dk, const double *__restrict__ amp, int nbins, rf_key key, int add,
                       int64_t count) {
  const int64_t nvec = count / V;                        // (count is a multiple of V)
  for (int64_t i = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * PS_THREADS) {
    const int64_t e = i * V;
    rf_mode m[V];
    bool zero[V], any = false;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      m[j] = rf_mode_of(e + j, d, k0, k1, k2, dk, amp, nbins);
      zero[j] = m[j].zero;
      any = any || !zero[j];
    }
    if constexpr (PROJECT) {
      double v[3][2 * V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        double gr[3] = {0.0, 0.0, 0.0}, gi[3] = {0.0, 0.0, 0.0};
        if (!zero[j]) {
#pragma unroll
          for (int c = 0; c < 3; ++c) rf_gauss(m[j], key, c, gr[c], gi[c]);
          rf_project(m[j], gr[0], gr[1], gr[2]);
          rf_project(m[j], gi[0], gi[1], gi[2]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v[c][2 * j] = gr[c] * m[j].a;
          v[c][2 * j + 1] = m[j].mirror ? -(gi[c] * m[j].a) : gi[c] * m[j].a;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) rf_store<real, V>(out + c * count + e, v[c], zero, any, add != 0);
    } else {
#pragma unroll 1
      for (int c = 0; c < ncomp; ++c) {
        double v[2 * V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          double gr = 0.0, gi = 0.0;
          if (!zero[j]) rf_gauss(m[j], key, c, gr, gi);
          v[2 * j] = gr * m[j].a;
          v[2 * j + 1] = m[j].mirror ? -(gi * m[j].a) : gi * m[j].a;
        }
        rf_store<real, V>(out + c * count + e, v, zero, any, add != 0);
      }
    }
  }
}

// gfft_ps_scale_shells: out[c][e] = f[c][e] * (real)tab[b], b the shell of ps_shell_of; +0 where b >= nbins (a NaN shell too).
// The isotropic counterpart of ps_scale_axes_kernel and in its mould: V modes per lane and 16 bytes per load and store, a
// lane reads all its values before it stores any (out may BE f).  A vector whose modes are all dropped is not loaded.
template <typename real, int V, int NC>
__global__ void __launch_bounds__(PS_THREADS)
ps_scale_shells_kernel(cx<real> *out, const cx<real> *f, const real *__restrict__ k0, const real *__restrict__ k1,
                       const real *__restrict__ k2, double dk, const double *__restrict__ tab, int nbins, int64_t n1, int64_t n2,
                       int64_t count) {
  using vec = st_load<real, 2 * V>;
  const int64_t nvec = count / V;                        // (count is a multiple of V)
  for (int64_t i = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * PS_THREADS) {
    const int64_t e = i * V;
    const int64_t row = e / n2, i2 = e - row * n2;
    const int64_t i0 = row / n1;
    const double kx = (double)k0[i0], ky = (double)k1[row - i0 * n1];
    real g[V];
    bool keep[V], any = false;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      double kk;
      const double sh = ps_shell_of(kx, ky, (double)k2[i2 + j], dk, kk);
      keep[j] = sh < (double)nbins;
      g[j] = keep[j] ? (real)tab[(int)sh] : (real)0;
      any = any || keep[j];
    }
    vec a[NC] = {};
    if (any) {
#pragma unroll
      for (int c = 0; c < NC; ++c) a[c] = *reinterpret_cast<const vec *>(f + c * count + e);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      vec o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        o.m[2 * j] = keep[j] ? a[c].m[2 * j] * g[j] : (real)0;
        o.m[2 * j + 1] = keep[j] ? a[c].m[2 * j + 1] * g[j] : (real)0;
      }
      *reinterpret_cast<vec *>(out + c * count + e) = o;
    }
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
// f(real()) with the element type of `precision`: a launcher names its kernel and arguments once
template <typename F>
hipError_t by_precision(int precision, F &&f) { return precision == GFFT_F64 ? f(double()) : f(float()); }

// `kern` on `grid` workgroups of 256 lanes, the arguments converted to its parameter types (void * to typed pointers, double to real)
template <typename... P, typename... A>
hipError_t ps_launch(void (*kern)(P...), int grid, size_t lds, hipStream_t s, A... args) {
  hipLaunchKernelGGL(kern, dim3(grid), dim3(PS_THREADS), lds, s, static_cast<P>(args)...);
  return hipGetLastError();
}

// a grid-stride kernel over `count` elements (none: nothing to launch)
template <typename K, typename... A>
hipError_t ps_pointwise(K kern, int64_t count, hipStream_t s, A... args) {
  return count ? ps_launch(kern, ps_grid(count), 0, s, args...) : hipSuccess;
}

hipError_t launch_ps_curl(const void *u, void *out, const void *k0, const void *k1, const void *k2, int64_t n0,
                          int64_t n1, int64_t n2, int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  return by_precision(
      precision, [&](auto r) { return ps_pointwise(ps_curl_kernel<decltype(r)>, count, s, u, out, k0, k1, k2, n1, n2, count); });
}

hipError_t launch_ps_cross(const void *a, const void *b, void *out, int64_t count, int precision, hipStream_t s) {
  return by_precision(precision, [&](auto r) { return ps_pointwise(ps_cross_kernel<decltype(r)>, count, s, a, b, out, count); });
}

hipError_t launch_ps_project(void *du, const void *u, const void *k0, const void *k1, const void *k2, int64_t n0,
                             int64_t n1, int64_t n2, double nu, int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  return by_precision(
      precision, [&](auto r) { return ps_pointwise(ps_project_kernel<decltype(r), ps_no_force>, count, s, du, u, k0, k1, k2, n1, n2, count, nu, ps_no_force(), ps_keep_all()); });
}

// The pre-filter of ps_band_force: lo2 <= kk <= hi2 for every mode whose exact shell lies in [blo, bhi], kk being |k|^2 as
// ps_project_kernel forms it in the field's precision.  In real numbers the band is (blo - 1/2) dk <= |k| < (bhi + 1/2) dk.
// Against that, relative to |k|^2:
//   * the exact test's own double arithmetic (three squares, two adds, sqrt, divide, + 0.5) moves its edges by < 8 x 2^-53;
//   * kk (three products and two adds of non-negative terms, contracted or not) is off by < 3 ulp of `real`: 3 eps;
//   * the squares formed here in double: < 4 x 2^-53.
// Both bounds are widened by 16 eps (eps = 2^-23 or 2^-52: more than four times the sum above) and then rounded OUTWARDS
// to `real`, so the conversion in the kernel is exact.  Below 16 x the smallest normal number kk may have lost bits to
// underflow: the lower bound gives way to 0 there.  An overflowing upper bound is +inf.  (An overflowing or NaN kk fails
// the pre-filter; its mode lies beyond every finite hi2, or has a NaN shell.)
struct ps_band { double lo2, hi2; };

template <typename real>
ps_band ps_band_bounds(double dk, int blo, int bhi) {
  const double m = 16.0 * (double)std::numeric_limits<real>::epsilon();
  const double lo = blo > 0 ? ((double)blo - 0.5) * dk : 0.0, hi = ((double)bhi + 0.5) * dk;
  double lo2 = lo * lo * (1.0 - m), hi2 = hi * hi * (1.0 + m);
  if (!(lo2 >= 16.0 * (double)std::numeric_limits<real>::min())) lo2 = 0.0;
  real l = (real)lo2, h = (real)hi2;
  if ((double)l > lo2) l = std::nextafter(l, (real)0);
  if ((double)h < hi2) h = std::nextafter(h, std::numeric_limits<real>::infinity());
  return {(double)l, (double)h};
}

hipError_t launch_ps_project_forced(void *du, const void *u, const void *k0, const void *k1, const void *k2, int64_t n0,
                                    int64_t n1, int64_t n2, double nu, double dk, int blo, int bhi, double gain,
                                    const double *d_gain, int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  return by_precision(precision, [&](auto r) {
    const ps_band b = ps_band_bounds<decltype(r)>(dk, blo, bhi);
    return ps_pointwise(ps_project_kernel<decltype(r), ps_band_args>, count, s, du, u, k0, k1, k2, n1, n2, count, nu,
                        ps_band_args{dk, blo, bhi, b.lo2, b.hi2, gain, d_gain}, ps_keep_all());
  });
}

// the projection, forced (the band arguments as above) or not, with the truncation `keep` fused in
hipError_t launch_ps_project_dealiased(void *du, const void *u, const void *k0, const void *k1, const void *k2, int64_t n0,
                                       int64_t n1, int64_t n2, double nu, ps_keep_mask keep, bool forced, double dk, int blo,
                                       int bhi, double gain, const double *d_gain, int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  return by_precision(precision, [&](auto r) {
    using real = decltype(r);
    if (!forced)
      return ps_pointwise(ps_project_kernel<real, ps_no_force, ps_keep_mask>, count, s, du, u, k0, k1, k2, n1, n2, count, nu,
                          ps_no_force(), keep);
    const ps_band b = ps_band_bounds<real>(dk, blo, bhi);
    return ps_pointwise(ps_project_kernel<real, ps_band_args, ps_keep_mask>, count, s, du, u, k0, k1, k2, n1, n2, count, nu,
                        ps_band_args{dk, blo, bhi, b.lo2, b.hi2, gain, d_gain}, keep);
  });
}

hipError_t launch_ps_dealias(void *f, int ncomp, const void *k0, const void *k1, const void *k2, int64_t n0, int64_t n1,
                             int64_t n2, ps_keep_mask keep, int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  return by_precision(
      precision, [&](auto r) { return ps_pointwise(ps_dealias_kernel<decltype(r)>, count, s, f, ncomp, k0, k1, k2, n1, n2, count, keep); });
}

hipError_t launch_ps_force_gain(const double *spec, int blo, int bhi, double eps, double gain_max, double *gain, hipStream_t s) {
  hipLaunchKernelGGL(ps_force_gain_kernel, dim3(1), dim3(64), 0, s, spec, blo, bhi, eps, gain_max, gain);
  return hipGetLastError();
}

hipError_t launch_ps_rk(void *u, const void *u0, void *u1, const void *du, int64_t count, double cb, double ca,
                        int precision, hipStream_t s) {
  return by_precision(
      precision, [&](auto r) { return ps_pointwise(ps_rk_kernel<decltype(r)>, count, s, u, u0, u1, du, count, cb, ca); });
}

hipError_t launch_ps_rk_dt(void *u, const void *u0, void *u1, const void *du, int64_t count, double cb, double ca,
                           const double *dt, int precision, hipStream_t s) {
  return by_precision(
      precision, [&](auto r) { return ps_pointwise(ps_rk_dt_kernel<decltype(r)>, count, s, u, u0, u1, du, count, cb, ca, dt); });
}

// 1 <= ncomp <= IF_MAX_COMP; every nu equal: the instantiation with one exp per mode
hipError_t launch_ps_rk_if(void *u, const void *u0, void *u1, const void *du, int ncomp, const ps_if_nu &nu, const void *k0,
                           const void *k1, const void *k2, int64_t n0, int64_t n1, int64_t n2, ps_if_pow q, ps_if_args arg,
                           int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  bool uniform = true;
  for (int c = 1; c < ncomp; ++c) uniform = uniform && nu.v[c] == nu.v[0];
  return by_precision(precision, [&](auto r) {
    using real = decltype(r);
    return ps_pointwise(uniform ? ps_rk_if_kernel<real, true> : ps_rk_if_kernel<real, false>, count, s, u, u0, u1, du, ncomp, k0,
                        k1, k2, n1, n2, count, nu, q, arg);
  });
}

hipError_t launch_ps_timestep(const double *stats, double cfl, double dt_min, double dt_max, double *dt, hipStream_t s) {
  hipLaunchKernelGGL(ps_timestep_kernel, dim3(1), dim3(64), 0, s, stats, cfl, dt_min, dt_max, dt);
  return hipGetLastError();
}

// elements per lane and load: `wide` (those of 16 bytes) where they divide `count` and every base is 16-byte aligned, else one
inline int ps_lane_width(int64_t count, int wide, bool aligned16) { return (count % wide == 0 && aligned16) ? wide : 1; }

// launch geometry of the reductions: V elements per lane and load, one contiguous chunk of whole steps of 256 V per workgroup
struct sp_geom { int V; int64_t chunk; int nwg; };

// wide = the elements of a 16-byte load (shell kernels: 1 or 2 modes; ps_stats: 2 or 4 reals), taken by ps_lane_width: where
// they divide `count` and every component of every field that is read starts 16-byte aligned; else one element per lane
sp_geom sp_geometry(int64_t count, int wide, bool aligned16) {
  sp_geom g;
  g.V = ps_lane_width(count, wide, aligned16);
  const int64_t step = (int64_t)PS_THREADS * g.V;
  g.chunk = (count + SP_MAX_WG - 1) / SP_MAX_WG;
  g.chunk = (g.chunk + step - 1) / step * step;
  g.nwg = count ? (int)((count + g.chunk - 1) / g.chunk) : 0;
  return g;
}

constexpr size_t ST_SCRATCH_BYTES = (size_t)SP_MAX_WG * (ST_HEAD + ST_PER_COMP * ST_MAX_COMP) * sizeof(double);

template <typename real, int V>
auto st_kernel(int ncomp) {
  return ncomp == 1 ? ps_stats_kernel<real, V, 1> : ncomp == 2 ? ps_stats_kernel<real, V, 2>
       : ncomp == 3 ? ps_stats_kernel<real, V, 3> : ps_stats_kernel<real, V, 4>;
}

// 1 <= ncomp <= ST_MAX_COMP; `slabs` = ST_SCRATCH_BYTES of stream-ordered scratch
hipError_t launch_ps_stats(const void *u, int ncomp, int64_t count, const double *inv_dx, double *out, double *slabs,
                           int precision, hipStream_t s) {
  const sp_geom g = sp_geometry(count, 16 / precision, (uintptr_t)u % 16 == 0);
  st_scale inv = {};
  for (int c = 0; c < ncomp; ++c) inv.v[c] = inv_dx[c];
  const hipError_t e = !g.nwg ? hipSuccess : by_precision(precision, [&](auto r) {
    using real = decltype(r);
    constexpr int W = 16 / sizeof(real);
    return ps_launch(g.V == W ? st_kernel<real, W>(ncomp) : st_kernel<real, 1>(ncomp), g.nwg, 0, s, u, count, g.chunk, inv, slabs);
  });
  if (e != hipSuccess) return e;
  return ps_launch(st_reduce_kernel, ST_HEAD + ST_PER_COMP * ncomp, 0, s, slabs, g.nwg, out);
}

template <typename real, int V>
auto sp_kernel(int op) {
  return op == SP_NORM ? ps_shell_kernel<real, V, SP_NORM>
       : op == SP_HELICITY ? ps_shell_kernel<real, V, SP_HELICITY> : ps_shell_kernel<real, V, SP_DOT>;
}

// op: SP_NORM / SP_DOT / SP_HELICITY (b is read by SP_DOT alone); `slabs` = SP_MAX_WG x 2 nbins doubles of stream-ordered scratch
hipError_t launch_ps_shell(const void *a, const void *b, int ncomp, int op, double scale, const void *k0, const void *k1,
                           const void *k2, const void *w2, int64_t n0, int64_t n1, int64_t n2, double dk, int nbins,
                           double *out, double *slabs, int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  const bool aligned = (uintptr_t)a % 16 == 0 && (op != SP_DOT || (uintptr_t)b % 16 == 0);
  const sp_geom g = sp_geometry(count, 8 / precision, aligned);
  const hipError_t e = !g.nwg ? hipSuccess : by_precision(precision, [&](auto r) {
    using real = decltype(r);
    constexpr int W = 16 / sizeof(cx<real>);
    return ps_launch(g.V == W ? sp_kernel<real, W>(op) : sp_kernel<real, 1>(op), g.nwg, (size_t)2 * nbins * sizeof(double), s, a, b,
                     ncomp, scale, k0, k1, k2, w2, n1, n2, count, g.chunk, dk, nbins, slabs);
  });
  if (e != hipSuccess) return e;
  return ps_launch(ps_spectrum_sum_kernel, (2 * nbins + PS_THREADS - 1) / PS_THREADS, 0, s, slabs, g.nwg, 2 * nbins, out);
}

template <typename real, int V>
auto sc_flux_kernel(int ns) {
  return ns == 1 ? ps_scalar_flux_kernel<real, V, 1> : ns == 2 ? ps_scalar_flux_kernel<real, V, 2>
       : ns == 3 ? ps_scalar_flux_kernel<real, V, 3> : ps_scalar_flux_kernel<real, V, 4>;
}

// 1 <= ns <= SC_MAX; the lane width is that of launch_ps_stats, over all three bases
hipError_t launch_ps_scalar_flux(const void *u, const void *theta, void *flux, int ns, int64_t count, int precision, hipStream_t s) {
  const bool aligned = (uintptr_t)u % 16 == 0 && (uintptr_t)theta % 16 == 0 && (uintptr_t)flux % 16 == 0;
  const int V = ps_lane_width(count, 16 / precision, aligned);
  return by_precision(precision, [&](auto r) {
    using real = decltype(r);
    constexpr int W = 16 / sizeof(real);
    return ps_pointwise(V == W ? sc_flux_kernel<real, W>(ns) : sc_flux_kernel<real, 1>(ns), count / V, s, u, theta, flux, count);
  });
}

template <typename real, bool MG, typename M>
auto sc_rhs_kernel(int ns) {
  return ns == 1 ? ps_scalar_rhs_kernel<real, 1, MG, M> : ns == 2 ? ps_scalar_rhs_kernel<real, 2, MG, M>
       : ns == 3 ? ps_scalar_rhs_kernel<real, 3, MG, M> : ps_scalar_rhs_kernel<real, 4, MG, M>;
}

// 1 <= ns <= SC_MAX; u is read iff `mean_gradient`; masked = false: the ps_keep_all instantiation, `keep` is not looked at
hipError_t launch_ps_scalar_rhs(void *d, const void *flux, const void *theta, const void *u, int ns, const sc_coef &coef,
                                bool mean_gradient, const void *k0, const void *k1, const void *k2, int64_t n0, int64_t n1,
                                int64_t n2, bool masked, ps_keep_mask keep, int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  return by_precision(precision, [&](auto r) {
    using real = decltype(r);
    auto go = [&](auto kern, auto pred) { return ps_pointwise(kern, count, s, d, flux, theta, u, k0, k1, k2, n1, n2, count, coef, pred); };
    if (masked)
      return mean_gradient ? go(sc_rhs_kernel<real, true, ps_keep_mask>(ns), keep) : go(sc_rhs_kernel<real, false, ps_keep_mask>(ns), keep);
    return mean_gradient ? go(sc_rhs_kernel<real, true, ps_keep_all>(ns), ps_keep_all()) : go(sc_rhs_kernel<real, false, ps_keep_all>(ns), ps_keep_all());
  });
}

template <typename real>
auto gr_kernel(int nc) {
  return nc == 1 ? ps_gradient_kernel<real, 1> : nc == 2 ? ps_gradient_kernel<real, 2>
       : nc == 3 ? ps_gradient_kernel<real, 3> : ps_gradient_kernel<real, 4>;
}

// 1 <= ncomp <= GR_MAX_COMP
constexpr int GR_MAX_COMP = 4;
hipError_t launch_ps_gradient(const void *f, void *out, int ncomp, const void *k0, const void *k1, const void *k2, int64_t n0,
                              int64_t n1, int64_t n2, int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  const int64_t lanes = ncomp == 1 ? (count + 1) / 2 : count;          // a single field: two modes per lane and step
  return by_precision(
      precision, [&](auto r) { return ps_pointwise(gr_kernel<decltype(r)>(ncomp), lanes, s, f, out, k0, k1, k2, n1, n2, count); });
}

template <typename real, int V>
auto sa_kernel(int nc) {
  return nc == 1 ? ps_scale_axes_kernel<real, V, 1> : nc == 2 ? ps_scale_axes_kernel<real, V, 2>
       : nc == 3 ? ps_scale_axes_kernel<real, V, 3> : ps_scale_axes_kernel<real, V, 4>;
}

// 1 <= ncomp <= SA_MAX_COMP; out == f or no overlap
hipError_t launch_ps_scale_axes(void *out, const void *f, int ncomp, const void *v0, const void *v1, const void *v2, int64_t n0,
                                int64_t n1, int64_t n2, int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  const bool pair = precision == GFFT_F32 && n2 % 2 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)f % 16 == 0;
  if (pair) return ps_pointwise(sa_kernel<float, 2>(ncomp), count / 2, s, out, f, v0, v1, v2, n1, n2, count);
  return by_precision(
      precision, [&](auto r) { return ps_pointwise(sa_kernel<decltype(r), 1>(ncomp), count, s, out, f, v0, v1, v2, n1, n2, count); });
}

template <typename real, int ORDER>
auto ip_kernel(int nc) {
  return nc == 1 ? ps_interp_kernel<real, 1, ORDER> : nc == 2 ? ps_interp_kernel<real, 2, ORDER>
       : nc == 3 ? ps_interp_kernel<real, 3, ORDER> : ps_interp_kernel<real, 4, ORDER>;
}

// 1 <= ncomp <= IP_MAX_COMP, order 2 or 4, d checked by the caller; ORDER^2 lanes per particle, so np * ORDER^2 lanes
hipError_t launch_ps_interp(const void *c, int ncomp, const ip_dims &d, const double *x, int64_t np, int order, double *out,
                            int precision, hipStream_t s) {
  return by_precision(precision, [&](auto r) {
    using real = decltype(r);
    return ps_pointwise(order == 4 ? ip_kernel<real, 4>(ncomp) : ip_kernel<real, 2>(ncomp), np * order * order, s, c, d, x, np, out);
  });
}

template <int ORDER>
auto spr_kernel(int nc) {
  return nc == 1 ? ps_spread_kernel<1, ORDER> : nc == 2 ? ps_spread_kernel<2, ORDER> : nc == 3 ? ps_spread_kernel<3, ORDER> : ps_spread_kernel<4, ORDER>;
}

// 1 <= ncomp <= SPR_MAX_COMP, order 2 or 4, d checked by the caller; the geometry of launch_ps_interp: np * ORDER^2 lanes
hipError_t launch_ps_spread(int64_t *acc, int ncomp, const ip_dims &d, const double *x, const double *q, int64_t np, int order,
                            double scale, int64_t *skipped, hipStream_t s) {
  return ps_pointwise(order == 4 ? spr_kernel<4>(ncomp) : spr_kernel<2>(ncomp), np * order * order, s, (void *)acc, d, x, q, np, scale,
                      (void *)skipped);
}

hipError_t launch_ps_spread_finish(void *out, int64_t *acc, int64_t count, double factor, int clear, int precision, hipStream_t s) {
  const bool wide = (uintptr_t)out % 16 == 0 && (uintptr_t)acc % 16 == 0;
  return by_precision(precision, [&](auto r) {
    using real = decltype(r);
    constexpr int V = 16 / (int)sizeof(real);
    if (wide) return ps_pointwise(ps_spread_finish_kernel<real, V>, (count + V - 1) / V, s, out, acc, count, factor, clear);
    return ps_pointwise(ps_spread_finish_kernel<real, 1>, count, s, out, acc, count, factor, clear);
  });
}

// the geometry of launch_ps_stats over the one base A; `slabs` = ST_SCRATCH_BYTES of stream-ordered scratch
hipError_t launch_ps_gradient_stats(const void *A, int64_t count, double *out, double *slabs, int precision, hipStream_t s) {
  const sp_geom g = sp_geometry(count, 16 / precision, (uintptr_t)A % 16 == 0);
  const hipError_t e = !g.nwg ? hipSuccess : by_precision(precision, [&](auto r) {
    using real = decltype(r);
    constexpr int W = 16 / sizeof(real);
    return ps_launch(g.V == W ? ps_gradient_stats_kernel<real, W> : ps_gradient_stats_kernel<real, 1>, g.nwg, 0, s, A, count,
                     g.chunk, slabs);
  });
  if (e != hipSuccess) return e;
  return ps_launch(gs_reduce_kernel, GS_NVAL, 0, s, slabs, g.nwg, out);
}

// ---- the PDFs: geometry, scratch and launchers ----
// workgroups (= slabs) of a table of `ncounters` 32-bit words: SP_MAX_WG up to 4096 words, then in inverse proportion (512 at 16384)
inline int pd_max_wg(int ncounters) { return ncounters <= 4096 ? SP_MAX_WG : (int)((int64_t)SP_MAX_WG * 4096 / ncounters); }

// sp_geometry with that many workgroups at most
sp_geom pd_geometry(int64_t count, int wide, bool aligned16, int max_wg) {
  sp_geom g;
  g.V = ps_lane_width(count, wide, aligned16);
  const int64_t step = (int64_t)PS_THREADS * g.V;
  g.chunk = (count + max_wg - 1) / max_wg;          // (count passed pd_chunk_fits: nothing overflows)
  g.chunk = (g.chunk + step - 1) / step * step;
  g.nwg = count ? (int)((count + g.chunk - 1) / g.chunk) : 0;
  return g;
}

// a workgroup's 32-bit counters hold its chunk: whole steps of at most 1024 points
inline bool pd_chunk_fits(int64_t count, int max_wg) { return count / max_wg + 1 + 1024 < ((int64_t)1 << 32); }

inline size_t pd_scratch_bytes(int ncounters, int ntails) { return (size_t)pd_max_wg(ncounters) * (ncounters + ntails) * sizeof(uint32_t); }

inline size_t pd_lds_bytes(int ncounters) { return (size_t)pd_words(ncounters) * sizeof(uint32_t); }

template <typename real, int V>
auto pd_hist_kernel(int ncomp) {
  return ncomp == 1 ? ps_histogram_kernel<real, V, 1> : ncomp == 2 ? ps_histogram_kernel<real, V, 2>
       : ncomp == 3 ? ps_histogram_kernel<real, V, 3> : ps_histogram_kernel<real, V, 4>;
}

// 1 <= ncomp <= ST_MAX_COMP, ncomp * nbins <= PD_MAX_COUNTERS; `slabs` = pd_scratch_bytes(ncomp nbins, 3 ncomp) of stream-ordered scratch
hipError_t launch_ps_histogram(const void *u, int ncomp, int64_t count, const pd_ranges &rg, int nbins, int64_t *out,
                               uint32_t *slabs, int precision, hipStream_t s) {
  const int ncounters = ncomp * nbins;
  const sp_geom g = pd_geometry(count, 16 / precision, (uintptr_t)u % 16 == 0, pd_max_wg(ncounters));
  const hipError_t e = !g.nwg ? hipSuccess : by_precision(precision, [&](auto r) {
    using real = decltype(r);
    constexpr int W = 16 / sizeof(real);
    return ps_launch(g.V == W ? pd_hist_kernel<real, W>(ncomp) : pd_hist_kernel<real, 1>(ncomp), g.nwg, pd_lds_bytes(ncounters), s,
                     u, count, g.chunk, rg, nbins, slabs);
  });
  if (e != hipSuccess) return e;
  const int n = ncomp * (nbins + GFFT_PS_PDF_TAIL);
  return ps_launch(pd_sum_kernel, (n + PD_SUM_OUT - 1) / PD_SUM_OUT, 0, s, slabs, g.nwg, ncomp, nbins, (int)GFFT_PS_PDF_TAIL, out);
}

// ay.q == GFFT_PS_Q_NONE: the 1-D table of ax; `slabs` = pd_scratch_bytes(counters, 3 or 2)
hipError_t launch_ps_gradient_pdf(const void *A, int64_t count, const gp_axis &ax, const gp_axis &ay, int64_t *out,
                                  uint32_t *slabs, int precision, hipStream_t s) {
  const bool joint = ay.q != GFFT_PS_Q_NONE;
  const int ncounters = joint ? ax.nbins * ay.nbins : ax.nbins, ntail = joint ? 2 : (int)GFFT_PS_PDF_TAIL;
  const sp_geom g = pd_geometry(count, 16 / precision, (uintptr_t)A % 16 == 0, pd_max_wg(ncounters));
  const hipError_t e = !g.nwg ? hipSuccess : by_precision(precision, [&](auto r) {
    using real = decltype(r);
    constexpr int W = 16 / sizeof(real);
    auto go = [&](auto kern) { return ps_launch(kern, g.nwg, pd_lds_bytes(ncounters), s, A, count, g.chunk, ax, ay, slabs); };
    if (joint) return g.V == W ? go(ps_gradient_pdf_kernel<real, W, true>) : go(ps_gradient_pdf_kernel<real, 1, true>);
    return g.V == W ? go(ps_gradient_pdf_kernel<real, W, false>) : go(ps_gradient_pdf_kernel<real, 1, false>);
  });
  if (e != hipSuccess) return e;
  return ps_launch(pd_sum_kernel, (ncounters + ntail + PD_SUM_OUT - 1) / PD_SUM_OUT, 0, s, slabs, g.nwg, 1, ncounters, ntail, out);
}

// lo < hi, both finite, hi - lo finite; w = nbins / (hi - lo), formed here once, finite
inline bool pd_range(double lo, double hi, int nbins, double &w) {
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return false;
  const double span = hi - lo;
  if (!std::isfinite(span)) return false;
  w = (double)nbins / span;
  return std::isfinite(w);
}

// gfft_ps_spectrum and gfft_ps_cospectrum behind their own argument checks (`bad`); fn names the caller in the messages.
// Arguments first: a bad call is refused without a device, like gfft_plan_create
int ps_shell(const char *fn, bool bad, const void *d_a_hat, const void *d_b_hat, int ncomp, int op, double scale,
             const void *d_k0, const void *d_k1, const void *d_k2, const void *d_w2, int64_t n0, int64_t n1, int64_t n2,
             double dk, int nbins, double *d_out, int precision, void *stream) {
  if (bad || !d_a_hat || !d_k0 || !d_k1 || !d_k2 || !d_out || ncomp < 1 || nbins < 1 || !(dk > 0) || n0 < 0 || n1 < 0 || n2 < 0 ||
      (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, std::string(fn) + ": bad argument");
  static_assert(SP_MAX_BINS == 4096, "the message names the limit");
  if (nbins > SP_MAX_BINS) return fail(GFFT_ERR_UNSUPPORTED, std::string(fn) + ": more than 4096 bins");
  if (n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30))
    return fail(GFFT_ERR_UNSUPPORTED, std::string(fn) + ": axis longer than 2^30");
  int rc = check_device();
  if (rc) return rc;
  // the workgroups' partial histograms live in the stream's shared scratch: allocated by the first call, so later
  // calls -- captured ones included -- allocate nothing
  void *slabs = nullptr;
  rc = scratch_get((hipStream_t)stream, (size_t)SP_MAX_WG * 2 * nbins * sizeof(double), &slabs);
  if (rc) return rc;
  HIP_TRY(launch_ps_shell(d_a_hat, d_b_hat, ncomp, op, scale, d_k0, d_k1, d_k2, d_w2, n0, n1, n2, dk, nbins, d_out,
                          static_cast<double *>(slabs), precision, (hipStream_t)stream));
  return GFFT_OK;
}

// ---- structure functions: the power sums of the increments u(x + r e_axis) - u(x), every separation from one read of u -----
// Definition, summation order and properties: include/gfft.h (gfft_ps_structure).  A workgroup takes tiles of WHOLE lines of
// `axis`, all NC components, staged once in LDS in the field's precision; the separations are the OUTER loop over the staged
// tile, so the field leaves HBM once per call and every partner is an LDS read.  Tiles (sf_geometry):
//   axis 2      W consecutive lines -- one contiguous run of W L elements per component, LDS point p = its offset in the run;
//   axis 0, 1   for one index of the axes in front, W = 2^w <= 256 adjacent columns of the axes behind: L rows of W
//               contiguous elements, LDS point p = row W + column (a ragged last tile leaves its missing columns unused).
// Either way consecutive lanes read consecutive LDS words for x and, but for the one place where the line wraps, for its
// partner: no bank conflicts.  A lane walks p = lane, lane + 256, ... and carries its index along the axis with it
// (+ 256 mod L, or + 256 / W): no division in the loop, and the partner is p + ((i + s) mod L - i) x (1 or W), the wrap an
// integer compare on an index < 2 L.  A tile holds SF_TILE_BYTES (two workgroups per CU) or one line if that is longer,
// fewer where the block is small (sf_geometry), never fewer than SF_MIN_POINTS points: the reduction after each separation
// is paid per tile.  As 9 NC plain butterflies it cost more than the tile's arithmetic (256^3, m = 3, fp64, 14 separations:
// 2.29 ms); sf_wave_sums forms the same sums with a fifth of the exchanges (0.95 ms).  NC is a template parameter so that the
// 9 NC accumulators of a lane are registers; the per-separation results accumulate in LDS (nsep x 9 NC doubles), thread v
// owning value v, and go to slot [k][c][value][workgroup] of the slabs at the end; sf_reduce_kernel is st_reduce_value over
// all nsep x 9 NC values.  At most sf_max_wg workgroups (512 = the two per CU that fit; fewer beyond 1024 values per
// workgroup: the slabs stay within 4 MiB); they take the tiles t = w, w + nwg, ...
// Measured (tools/structure_probe.py; 256^3, m = 3): one separation reads the field at 0.40 - 0.53 (fp64) and
// 0.31 - 0.35 (fp32) of the copy's rate (2 waves per SIMD; staging and arithmetic overlap only between the two workgroups of a
// CU); at 14 separations the pass (1.0 - 1.1 ms in fp64) is bound by the fp64 arithmetic and the LDS reads at that occupancy,
// not by HBM.  Tiles of 32 KiB on 1024 workgroups and of 48 KiB on 768 were measured too (the kernel alone, back to back): no
// faster at 14 separations (0.98 - 1.14 and 0.95 - 0.97 ms against 0.87 - 0.95), and the smaller tile's 32-byte rows along
// axis 0 and 1 cost 70 % at one separation.
// (Registers: in the list above ps_stats_kernel; no instantiation spills or uses scratch.)
constexpr int SF_NVAL = GFFT_PS_SF_NVAL, SF_MAX_COMP = 4, SF_MAX_SEP = GFFT_PS_SF_MAX_SEP, SF_MAX_AXIS = GFFT_PS_SF_MAX_AXIS;
constexpr int SF_TILE_BYTES = 64 * 1024, SF_MIN_POINTS = 1024;
constexpr int SF_MAX_WG = 512, SF_SLAB_VALUES = 1024;
constexpr size_t SF_MAX_LDS = 156 * 1024;            // dynamic; 2 x 4 x 36 doubles of static LDS beside it
static_assert((size_t)SF_MAX_AXIS * SF_MAX_COMP * sizeof(double) + (size_t)SF_MAX_SEP * SF_MAX_COMP * SF_NVAL * sizeof(double) <= SF_MAX_LDS,
              "the longest line of four doubles and the running sums fit");

struct sf_seps { int32_t v[SF_MAX_SEP]; };           // by value in the launch

struct sf_geom {
  int L;               // n[axis]
  int rows;            // 0: axis 2, a tile is one contiguous run; 1: axis 0 or 1, a tile is L rows of W columns
  int V;               // elements per staging load: those of 16 bytes, or 1
  int W;               // lines (axis 2) or columns (axis 0, 1: a power of two) of a full tile
  int row_shift;       // staging: point p lies in row p >> row_shift (axis 2: one row, shift 30)
  int pstride;         // LDS points between components (a multiple of 4)
  int istride;         // LDS points between neighbours along the axis: 1 or W
  int istep;           // a lane's index along the axis grows by this (mod L) per step of 256 points
  int nwg;
  int64_t nb;          // axis 0, 1: column tiles per index of the axes in front
  int64_t lines;       // axis 2: lines of the block; axis 0, 1: columns per index of the axes in front
  int64_t row_stride;  // axis 0, 1: elements between neighbours along the axis
  int64_t count;       // elements between components
  int64_t ntiles;
  size_t lds;
};

inline int sf_max_wg(int nvalues) {
  return nvalues <= SF_SLAB_VALUES ? SF_MAX_WG : (int)((int64_t)SF_MAX_WG * SF_SLAB_VALUES / nvalues);
}

sf_geom sf_geometry(const int64_t n[3], int axis, int ncomp, int nsep, int precision, bool aligned16) {
  sf_geom g = {};
  g.L = (int)n[axis];
  g.count = n[0] * n[1] * n[2];
  if (!g.count) return g;
  const int wide = 16 / precision, max_wg = sf_max_wg(nsep * ncomp * SF_NVAL);
  const int64_t cap = SF_TILE_BYTES / (ncomp * precision);      // points per component in SF_TILE_BYTES
  int64_t points;
  if (axis == 2) {
    const int64_t lines = n[0] * n[1];
    // a small block: no more lines than hand every workgroup a tile, but SF_MIN_POINTS points; always one whole line
    const int64_t spread = (lines + max_wg - 1) / max_wg, least = (SF_MIN_POINTS + g.L - 1) / g.L;
    int64_t W = cap / g.L;
    if (W > (spread > least ? spread : least)) W = spread > least ? spread : least;
    if (W > lines) W = lines;
    if (W < 1) W = 1;
    g.V = ps_lane_width(g.L, wide, aligned16);
    g.rows = 0, g.W = (int)W, g.row_shift = 30, g.istride = 1, g.istep = PS_THREADS % g.L;
    g.nb = 1, g.lines = lines, g.row_stride = 0;
    g.ntiles = (lines + W - 1) / W;
    points = W * g.L;
  } else {
    const int64_t inner = axis == 1 ? n[2] : n[1] * n[2], outer = axis == 1 ? n[0] : 1;
    int W = PS_THREADS, lg = 8;
    while (W > 1 && ((int64_t)W * g.L > cap || W / 2 >= inner)) W >>= 1, --lg;
    while (W > 16 && (int64_t)(W / 2) * g.L >= SF_MIN_POINTS && outer * ((inner + W - 1) / W) < max_wg) W >>= 1, --lg;
    g.V = W >= wide ? ps_lane_width(inner, wide, aligned16) : 1;
    g.rows = 1, g.W = W, g.row_shift = lg, g.istride = W, g.istep = PS_THREADS / W;
    g.nb = (inner + W - 1) / W, g.lines = inner, g.row_stride = inner;
    g.ntiles = outer * g.nb;
    points = (int64_t)W * g.L;
  }
  g.pstride = (int)((points + 3) & ~(int64_t)3);
  g.nwg = (int)(g.ntiles < max_wg ? g.ntiles : max_wg);
  g.lds = (size_t)ncomp * g.pstride * precision + (size_t)nsep * ncomp * SF_NVAL * sizeof(double);
  return g;
}

__host__ __device__ constexpr int sf_kind(int) { return ST_SUM; }

// The butterfly of st_wave for N sums at once.  At the step with the partner lane ^ m a lane keeps the half of its values that
// bit m of its number selects and hands the partner the other half: what a lane forms is own + partner's, the very a + b both
// partners of the plain butterfly form, so every sum is the plain butterfly's to the last bit -- but N values padded to
// P = 2^p cost about P exchanges, not 6 N (27 values: 32 against 162).  sf_fold: one such step over the LIVE values left, H of
// them kept; afterwards v[0] is the value number `idx` of the lane, summed over the masks taken so far.
template <int H, int LIVE, int N>
__device__ __forceinline__ void sf_fold(double (&v)[N], int lane, int m, int &idx) {
  if constexpr (H >= 1) {
    constexpr int KEPT = LIVE < H ? LIVE : H;
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int j = 0; j < KEPT; ++j) {
      const double hi = j + H < LIVE ? v[j + H] : 0.0;
      const double keep = up ? hi : v[j], give = up ? v[j] : hi;
      v[j] = keep + __shfl_xor(give, m);
    }
    if (up) idx += H;
    sf_fold<H / 2, KEPT, N>(v, lane, m >> 1, idx);
  }
}

// the wave's sums of v[0 ... N - 1]: afterwards value number `idx` (if < N) stands in every lane that returns it -- the lanes
// that differ only in the bits `low` -- summed by lane ^ 32, 16, 8, 4, 2, 1 in that order
template <int N>
__device__ __forceinline__ double sf_wave_sums(double (&v)[N], int lane, int &idx, int &low) {
  constexpr int P = N <= 16 ? 16 : N <= 32 ? 32 : 64;
  static_assert(N <= 64, "one value per lane at the most");
  idx = 0;
  sf_fold<P / 2, N, N>(v, lane, 32, idx);
  double r = v[0];
#pragma unroll
  for (int m = 32 / P; m >= 1; m >>= 1) r += __shfl_xor(r, m);
  low = 64 / P - 1;
  return r;
}

template <typename real, int V, int NC>
__global__ void __launch_bounds__(PS_THREADS)
ps_structure_kernel(const real *__restrict__ u, sf_geom g, sf_seps seps, int nsep, int lcomp, double *__restrict__ slabs) {
  constexpr int NVAL = SF_NVAL * NC;
  extern __shared__ __attribute__((aligned(16))) unsigned char sf_lds[];
  __shared__ double sf_part[2][PS_THREADS / 64][NVAL];
  real *tile = reinterpret_cast<real *>(sf_lds);                                   // [NC][pstride]
  double *acc = reinterpret_cast<double *>(sf_lds + (size_t)NC * g.pstride * sizeof(real));   // [nsep][NVAL], thread v owns value v
  const int tid = threadIdx.x, L = g.L, ps = g.pstride;
  const bool rows = g.rows != 0;                             // axis 0 or 1
  const int rmask = (1 << g.row_shift) - 1;
  const int i0 = rows ? tid >> g.row_shift : tid % L;        // the lane's first index along the axis, the same in every tile
  for (int i = tid; i < nsep * NVAL; i += PS_THREADS) acc[i] = 0.0;
  for (int64_t t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    // the tile: its first element, its valid columns per staging row, its LDS points
    int64_t base;
    int ncol, plimit;
    if (rows) {
      const int64_t o = t / g.nb, j0 = (t - o * g.nb) * g.W;
      base = o * L * g.row_stride + j0;
      ncol = (int)(g.lines - j0 < g.W ? g.lines - j0 : g.W);
      plimit = L << g.row_shift;
    } else {
      const int64_t l0 = t * g.W;
      base = l0 * L;
      ncol = (int)(g.lines - l0 < g.W ? g.lines - l0 : g.W) * L;
      plimit = ncol;
    }
    const int cmask = rows ? rmask : 0, cvalid = rows ? ncol : 1;      // point p is one of the block iff (p & cmask) < cvalid
    __syncthreads();                                         // the tile before is done with
    for (int p = tid * V; p < plimit; p += PS_THREADS * V) {
      const int row = p >> g.row_shift, col = p & rmask;
      if (col < ncol) {                                      // (ncol, col and every base are multiples of V: all V or none)
        const real *src = u + base + row * g.row_stride + col;
#pragma unroll
        for (int c = 0; c < NC; ++c)
          *reinterpret_cast<st_load<real, V> *>(tile + c * ps + p) = *reinterpret_cast<const st_load<real, V> *>(src + c * g.count);
      }
    }
    __syncthreads();
    for (int k = 0; k < nsep; ++k) {
      const int s = seps.v[k];
      double val[NVAL];
#pragma unroll
      for (int i = 0; i < NVAL; ++i) val[i] = 0.0;
      int ia = i0;
      for (int p = tid; p < plimit; p += PS_THREADS) {
        if ((p & cmask) < cvalid) {
          int ib = ia + s;
          if (ib >= L) ib -= L;                              // the integer wrap: 0 <= ia, s < L
          const int q = p + (ib - ia) * g.istride;
          double d[NC], dl = 0.0;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const double a = tile[c * ps + p], b = tile[c * ps + q];       // converted before any arithmetic
            d[c] = b - a;
            if (c == lcomp) dl = d[c];
          }
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            double *v = val + SF_NVAL * c;
            const double d1 = d[c], d2 = d1 * d1, d3 = d2 * d1, d4 = d2 * d2, ad = fabs(d1);
            v[GFFT_PS_SF_D1] += d1;
            v[GFFT_PS_SF_D2] += d2;
            v[GFFT_PS_SF_D3] += d3;
            v[GFFT_PS_SF_D4] += d4;
            v[GFFT_PS_SF_D5] += d4 * d1;
            v[GFFT_PS_SF_D6] += d3 * d3;
            v[GFFT_PS_SF_ABS1] += ad;
            v[GFFT_PS_SF_ABS3] += d2 * ad;
            if (lcomp >= 0) v[GFFT_PS_SF_MIX] += dl * d2;
          }
        }
        ia += g.istep;
        if (ia >= L) ia -= L;
      }
      double(&part)[PS_THREADS / 64][NVAL] = sf_part[k & 1];   // two buffers: one barrier per separation
      int slot, low;
      const double w = sf_wave_sums(val, tid & 63, slot, low);
      if (slot < NVAL && (tid & low) == 0) part[tid >> 6][slot] = w;
      __syncthreads();
      if (tid < NVAL) {
        double r = part[0][tid];
        for (int w = 1; w < PS_THREADS / 64; ++w) r += part[w][tid];
        acc[k * NVAL + tid] += r;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < nsep * NVAL; i += PS_THREADS) slabs[(int64_t)i * gridDim.x + blockIdx.x] = acc[i];
}

__global__ void __launch_bounds__(PS_THREADS)
sf_reduce_kernel(const double *__restrict__ slabs, int nwg, double *__restrict__ out) {
  st_reduce_value<sf_kind>(slabs, nwg, out, nwg);
}

inline size_t sf_scratch_bytes(int nvalues) { return (size_t)sf_max_wg(nvalues) * nvalues * sizeof(double); }

template <typename real, int V, int NC>
hipError_t sf_launch(const void *u, const sf_geom &g, const sf_seps &seps, int nsep, int lcomp, double *slabs, hipStream_t s) {
  // beyond 64 KiB of dynamic LDS a kernel has to be told once per device
  static bool attr_set[kMaxDevices] = {};
  const int dev = current_device();
  if (g.lds > 48 * 1024 && !attr_set[dev]) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ps_structure_kernel<real, V, NC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)SF_MAX_LDS);
    if (e != hipSuccess) return e;
    attr_set[dev] = true;
  }
  return ps_launch(ps_structure_kernel<real, V, NC>, g.nwg, g.lds, s, u, g, seps, nsep, lcomp, slabs);
}

template <typename real, int V>
hipError_t sf_launch_nc(int ncomp, const void *u, const sf_geom &g, const sf_seps &seps, int nsep, int lcomp, double *slabs, hipStream_t s) {
  return ncomp == 1 ? sf_launch<real, V, 1>(u, g, seps, nsep, lcomp, slabs, s)
       : ncomp == 2 ? sf_launch<real, V, 2>(u, g, seps, nsep, lcomp, slabs, s)
       : ncomp == 3 ? sf_launch<real, V, 3>(u, g, seps, nsep, lcomp, slabs, s)
                    : sf_launch<real, V, 4>(u, g, seps, nsep, lcomp, slabs, s);
}

// 1 <= ncomp <= SF_MAX_COMP, 1 <= nsep <= SF_MAX_SEP, 0 <= sep < n[axis] <= SF_MAX_AXIS; `slabs` = sf_scratch_bytes of stream-ordered scratch
hipError_t launch_ps_structure(const void *u, int ncomp, const int64_t n[3], int axis, const sf_seps &seps, int nsep, int lcomp,
                               double *out, double *slabs, int precision, hipStream_t s) {
  const sf_geom g = sf_geometry(n, axis, ncomp, nsep, precision, (uintptr_t)u % 16 == 0);
  const hipError_t e = !g.nwg ? hipSuccess : by_precision(precision, [&](auto r) {
    using real = decltype(r);
    constexpr int W = 16 / sizeof(real);
    return g.V == W ? sf_launch_nc<real, W>(ncomp, u, g, seps, nsep, lcomp, slabs, s)
                    : sf_launch_nc<real, 1>(ncomp, u, g, seps, nsep, lcomp, slabs, s);
  });
  if (e != hipSuccess) return e;
  return ps_launch(sf_reduce_kernel, nsep * ncomp * SF_NVAL, 0, s, slabs, g.nwg, out);
}

// the grid of ps_random_field_kernel: a lane per vector of modes up to RF_MAX_WG workgroups, grid-stride beyond
inline int rf_grid(int64_t nvec) {
  const int64_t b = (nvec + PS_THREADS - 1) / PS_THREADS;
  return (int)(b < RF_MAX_WG ? b : RF_MAX_WG);
}

// 1 <= ncomp <= RF_MAX_COMP (3 with project), the block inside the grid N; checked by the caller
hipError_t launch_ps_random_field(void *out, int ncomp, const rf_dims &d, int64_t count, const void *k0, const void *k1, const void *k2,
                                  int project, double dk, const double *amp, int nbins, const rf_key &key, int add, int precision,
                                  hipStream_t s) {
  if (!count) return hipSuccess;
  const bool pair = precision == GFFT_F32 && d.n2 % 2 == 0 && (uintptr_t)out % 16 == 0;
  auto go = [&](auto kern, int64_t nvec) {
    return ps_launch(kern, rf_grid(nvec), 0, s, out, ncomp, d, k0, k1, k2, dk, amp, nbins, key, add, count);
  };
  if (pair) return project ? go(ps_random_field_kernel<float, 2, true>, count / 2) : go(ps_random_field_kernel<float, 2, false>, count / 2);
  return by_precision(precision, [&](auto r) {
    using real = decltype(r);
    return project ? go(ps_random_field_kernel<real, 1, true>, count) : go(ps_random_field_kernel<real, 1, false>, count);
  });
}

template <typename real, int V>
auto ss_kernel(int nc) {
  return nc == 1 ? ps_scale_shells_kernel<real, V, 1> : nc == 2 ? ps_scale_shells_kernel<real, V, 2>
       : nc == 3 ? ps_scale_shells_kernel<real, V, 3> : ps_scale_shells_kernel<real, V, 4>;
}

// 1 <= ncomp <= SA_MAX_COMP; out == f or no overlap; the geometry of launch_ps_scale_axes
hipError_t launch_ps_scale_shells(void *out, const void *f, int ncomp, const void *k0, const void *k1, const void *k2, double dk,
                                  const double *tab, int nbins, int64_t n0, int64_t n1, int64_t n2, int precision, hipStream_t s) {
  const int64_t count = n0 * n1 * n2;
  const bool pair = precision == GFFT_F32 && n2 % 2 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)f % 16 == 0;
  if (pair) return ps_pointwise(ss_kernel<float, 2>(ncomp), count / 2, s, out, f, k0, k1, k2, dk, tab, nbins, n1, n2, count);
  return by_precision(precision, [&](auto r) {
    return ps_pointwise(ss_kernel<decltype(r), 1>(ncomp), count, s, out, f, k0, k1, k2, dk, tab, nbins, n1, n2, count);
  });
}

}  // namespace

}  // namespace gfft

// ---- C ABI (include/gfft.h) --------------------------------------------------------------------------------------------
using namespace gfft;

extern "C" {

int gfft_ps_curl(const void *d_u_hat, void *d_out, const void *d_k0, const void *d_k1, const void *d_k2,
                 int64_t n0, int64_t n1, int64_t n2, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_u_hat || !d_out || !d_k0 || !d_k1 || !d_k2 || n0 < 0 || n1 < 0 || n2 < 0 || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_curl: bad argument");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_curl(d_u_hat, d_out, d_k0, d_k1, d_k2, n0, n1, n2, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_cross(const void *d_a, const void *d_b, void *d_out, int64_t count, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_a || !d_b || !d_out || count < 0 || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_cross: bad argument");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_cross(d_a, d_b, d_out, count, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_project(void *d_du_hat, const void *d_u_hat, const void *d_k0, const void *d_k1, const void *d_k2,
                    int64_t n0, int64_t n1, int64_t n2, double nu, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_du_hat || !d_u_hat || !d_k0 || !d_k1 || !d_k2 || n0 < 0 || n1 < 0 || n2 < 0 || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_project: bad argument");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_project(d_du_hat, d_u_hat, d_k0, d_k1, d_k2, n0, n1, n2, nu, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_rk_stage(void *d_u, const void *d_u0, void *d_u1, const void *d_du, int64_t count, double cb,
                     double ca, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if ((d_u && !d_u0) || !d_u1 || !d_du || count < 0 || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_rk_stage: bad argument");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_rk(d_u, d_u0, d_u1, d_du, count, cb, ca, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_spectrum(const void *d_u_hat, int ncomp, const void *d_k0, const void *d_k1, const void *d_k2,
                     const void *d_w2, int64_t n0, int64_t n1, int64_t n2, double dk, int nbins, double *d_out,
                     int precision, void *stream) {
  return ps_shell("gfft_ps_spectrum", false, d_u_hat, nullptr, ncomp, SP_NORM, 0.5, d_k0, d_k1, d_k2, d_w2, n0, n1, n2, dk,
                  nbins, d_out, precision, stream);
}

int gfft_ps_cospectrum(const void *d_a_hat, const void *d_b_hat, int ncomp, int op, double scale, const void *d_k0,
                       const void *d_k1, const void *d_k2, const void *d_w2, int64_t n0, int64_t n1, int64_t n2, double dk,
                       int nbins, double *d_out, int precision, void *stream) {
  const bool bad = (op != GFFT_PS_DOT && op != GFFT_PS_HELICITY) || (op == GFFT_PS_DOT && !d_b_hat) ||
                   (op == GFFT_PS_HELICITY && ncomp != 3) || !std::isfinite(scale);
  return ps_shell("gfft_ps_cospectrum", bad, d_a_hat, d_b_hat, ncomp, op, scale, d_k0, d_k1, d_k2, d_w2, n0, n1, n2, dk,
                  nbins, d_out, precision, stream);
}

int gfft_ps_stats(const void *d_u, int ncomp, int64_t count, const double *inv_dx, double *d_out, int precision,
                  void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_u || !inv_dx || !d_out || ncomp < 1 || count < 0 || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_stats: bad argument");
  static_assert(ST_MAX_COMP == 4, "the message names the limit");
  if (ncomp > ST_MAX_COMP) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_stats: more than 4 components");
  for (int c = 0; c < ncomp; ++c)
    if (!std::isfinite(inv_dx[c]) || inv_dx[c] < 0) return fail(GFFT_ERR_INVALID, "gfft_ps_stats: inv_dx must be finite and >= 0");
  int rc = check_device();
  if (rc) return rc;
  // the workgroups' partial results live in the stream's shared scratch: the first call allocates, later ones only enqueue
  void *slabs = nullptr;
  rc = scratch_get((hipStream_t)stream, ST_SCRATCH_BYTES, &slabs);
  if (rc) return rc;
  HIP_TRY(launch_ps_stats(d_u, ncomp, count, inv_dx, d_out, static_cast<double *>(slabs), precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_timestep(const double *d_stats, double cfl, double dt_min, double dt_max, double *d_dt, void *stream) {
  if (!d_stats || !d_dt || !std::isfinite(cfl) || !std::isfinite(dt_min) || !std::isfinite(dt_max) || !(cfl > 0) ||
      !(dt_min >= 0) || !(dt_min <= dt_max))
    return fail(GFFT_ERR_INVALID, "gfft_ps_timestep: bad argument");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_timestep(d_stats, cfl, dt_min, dt_max, d_dt, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_rk_stage_dt(void *d_u, const void *d_u0, void *d_u1, const void *d_du, int64_t count, double cb, double ca,
                        const double *d_dt, int precision, void *stream) {
  if ((d_u && !d_u0) || !d_u1 || !d_du || !d_dt || count < 0 || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_rk_stage_dt: bad argument");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_rk_dt(d_u, d_u0, d_u1, d_du, count, cb, ca, d_dt, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_rk_stage_if(void *d_u, const void *d_u0, void *d_u1, const void *d_du, int ncomp, const double *nu, const void *d_k0,
                        const void *d_k1, const void *d_k2, int64_t n0, int64_t n1, int64_t n2, double cb, double ca, int q0,
                        int qd, int q1, int qa, double h, const double *d_dt, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  const auto power = [](int q) { return q >= 0 && q <= 2; };
  if ((d_u && !d_u0) || !d_u1 || !d_du || !nu || !d_k0 || !d_k1 || !d_k2 || ncomp < 1 || n0 < 0 || n1 < 0 || n2 < 0 ||
      !power(q0) || !power(qd) || !power(q1) || !power(qa) || (!d_dt && !std::isfinite(h)) ||
      (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_rk_stage_if: bad argument");
  static_assert(IF_MAX_COMP == 4, "the message names the limit");
  if (ncomp > IF_MAX_COMP) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_rk_stage_if: more than 4 components");
  ps_if_nu v = {};
  for (int c = 0; c < ncomp; ++c) {
    if (!std::isfinite(nu[c]) || nu[c] < 0) return fail(GFFT_ERR_INVALID, "gfft_ps_rk_stage_if: nu must be finite and >= 0");
    v.v[c] = nu[c];
  }
  if (n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30))
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_rk_stage_if: axis longer than 2^30");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_rk_if(d_u, d_u0, d_u1, d_du, ncomp, v, d_k0, d_k1, d_k2, n0, n1, n2, ps_if_pow{q0, qd, q1, qa},
                          ps_if_args{cb, ca, h, d_dt}, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_force_gain(const double *d_spec, int nbins, int blo, int bhi, double eps, double gain_max, double *d_gain,
                       void *stream) {
  if (!d_spec || !d_gain || nbins < 1 || blo < 0 || bhi < blo || bhi >= nbins || !std::isfinite(eps) || !(eps >= 0) ||
      !(gain_max > 0))
    return fail(GFFT_ERR_INVALID, "gfft_ps_force_gain: bad argument");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_force_gain(d_spec, blo, bhi, eps, gain_max, d_gain, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_project_forced(void *d_du_hat, const void *d_u_hat, const void *d_k0, const void *d_k1, const void *d_k2,
                           int64_t n0, int64_t n1, int64_t n2, double nu, double dk, int blo, int bhi, double gain,
                           const double *d_gain, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_du_hat || !d_u_hat || !d_k0 || !d_k1 || !d_k2 || n0 < 0 || n1 < 0 || n2 < 0 || !(dk > 0) || blo < 0 || bhi < blo ||
      (!d_gain && !std::isfinite(gain)) || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_project_forced: bad argument");
  if (n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30))
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_project_forced: axis longer than 2^30");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_project_forced(d_du_hat, d_u_hat, d_k0, d_k1, d_k2, n0, n1, n2, nu, dk, blo, bhi, gain, d_gain, precision,
                                   (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_project_dealiased(void *d_du_hat, const void *d_u_hat, const void *d_k0, const void *d_k1, const void *d_k2,
                              const unsigned char *d_m0, const unsigned char *d_m1, const unsigned char *d_m2,
                              int64_t n0, int64_t n1, int64_t n2, double nu, double kcut,
                              int forced, double dk, int blo, int bhi, double gain, const double *d_gain,
                              int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum; the band arguments are looked at only where they are used)
  if (!d_du_hat || !d_u_hat || !d_k0 || !d_k1 || !d_k2 || n0 < 0 || n1 < 0 || n2 < 0 || !(kcut >= 0) ||
      (forced && (!(dk > 0) || blo < 0 || bhi < blo || (!d_gain && !std::isfinite(gain)))) ||
      (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_project_dealiased: bad argument");
  if (n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30))
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_project_dealiased: axis longer than 2^30");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_project_dealiased(d_du_hat, d_u_hat, d_k0, d_k1, d_k2, n0, n1, n2, nu, ps_keep_mask{d_m0, d_m1, d_m2, kcut * kcut},
                                      forced != 0, dk, blo, bhi, gain, d_gain, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_dealias(void *d_field, int ncomp, const void *d_k0, const void *d_k1, const void *d_k2,
                    const unsigned char *d_m0, const unsigned char *d_m1, const unsigned char *d_m2,
                    int64_t n0, int64_t n1, int64_t n2, double kcut, int precision, void *stream) {
  // (arguments first; the wavenumbers are read only for a spherical cut)
  if (!d_field || ncomp < 1 || n0 < 0 || n1 < 0 || n2 < 0 || !(kcut >= 0) ||
      (std::isfinite(kcut) && (!d_k0 || !d_k1 || !d_k2)) || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_dealias: bad argument");
  if (n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30))
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_dealias: axis longer than 2^30");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_dealias(d_field, ncomp, d_k0, d_k1, d_k2, n0, n1, n2, ps_keep_mask{d_m0, d_m1, d_m2, kcut * kcut}, precision,
                            (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_scalar_flux(const void *d_u, const void *d_theta, void *d_flux, int nscalar, int64_t count, int precision,
                        void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_u || !d_theta || !d_flux || nscalar < 1 || count < 0 || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_scalar_flux: bad argument");
  static_assert(SC_MAX == 4, "the message names the limit");
  if (nscalar > SC_MAX) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_scalar_flux: more than 4 scalars");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_scalar_flux(d_u, d_theta, d_flux, nscalar, count, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_scalar_rhs(void *d_dtheta_hat, const void *d_flux_hat, const void *d_theta_hat, const void *d_u_hat, int nscalar,
                       const double *kappa, const double *grad, const void *d_k0, const void *d_k1, const void *d_k2,
                       const unsigned char *d_m0, const unsigned char *d_m1, const unsigned char *d_m2,
                       int64_t n0, int64_t n1, int64_t n2, double kcut, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_dtheta_hat || !d_flux_hat || !d_theta_hat || !d_k0 || !d_k1 || !d_k2 || n0 < 0 || n1 < 0 || n2 < 0 || !(kcut >= 0) ||
      nscalar < 1 || !kappa || (grad && !d_u_hat) || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_scalar_rhs: bad argument");
  static_assert(SC_MAX == 4, "the message names the limit");
  if (nscalar > SC_MAX) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_scalar_rhs: more than 4 scalars");
  sc_coef coef = {};
  for (int s = 0; s < nscalar; ++s) {
    if (!std::isfinite(kappa[s]) || kappa[s] < 0) return fail(GFFT_ERR_INVALID, "gfft_ps_scalar_rhs: kappa must be finite and >= 0");
    coef.kappa[s] = kappa[s];
    for (int c = 0; grad && c < 3; ++c) {
      if (!std::isfinite(grad[3 * s + c])) return fail(GFFT_ERR_INVALID, "gfft_ps_scalar_rhs: grad must be finite");
      coef.grad[s][c] = grad[3 * s + c];
    }
  }
  if (n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30))
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_scalar_rhs: axis longer than 2^30");
  if (int rc = check_device()) return rc;
  const bool masked = d_m0 || d_m1 || d_m2 || kcut < (double)INFINITY;
  HIP_TRY(launch_ps_scalar_rhs(d_dtheta_hat, d_flux_hat, d_theta_hat, d_u_hat, nscalar, coef, grad != nullptr, d_k0, d_k1, d_k2,
                               n0, n1, n2, masked, ps_keep_mask{d_m0, d_m1, d_m2, kcut * kcut}, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_gradient(const void *d_f_hat, void *d_out, int ncomp, const void *d_k0, const void *d_k1, const void *d_k2,
                     int64_t n0, int64_t n1, int64_t n2, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_f_hat || !d_out || !d_k0 || !d_k1 || !d_k2 || ncomp < 1 || n0 < 0 || n1 < 0 || n2 < 0 ||
      (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_gradient: bad argument");
  static_assert(GR_MAX_COMP == 4, "the message names the limit");
  if (ncomp > GR_MAX_COMP) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_gradient: more than 4 components");
  if (n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30))
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_gradient: axis longer than 2^30");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_gradient(d_f_hat, d_out, ncomp, d_k0, d_k1, d_k2, n0, n1, n2, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_gradient_stats(const void *d_A, int64_t count, double *d_out, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_A || !d_out || count < 0 || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_gradient_stats: bad argument");
  int rc = check_device();
  if (rc) return rc;
  // the slabs of gfft_ps_stats, and no more of the stream's scratch than it asks for: the first call allocates, later ones only enqueue
  void *slabs = nullptr;
  rc = scratch_get((hipStream_t)stream, ST_SCRATCH_BYTES, &slabs);
  if (rc) return rc;
  HIP_TRY(launch_ps_gradient_stats(d_A, count, d_out, static_cast<double *>(slabs), precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_structure(const void *d_u, int ncomp, const int64_t n[3], int axis, int nsep, const int32_t *sep, int lcomp,
                      double *d_out, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_u || !n || !sep || !d_out || ncomp < 1 || nsep < 1 || axis < 0 || axis > 2 || n[0] < 0 || n[1] < 0 || n[2] < 0 ||
      lcomp < -1 || lcomp >= ncomp || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_structure: bad argument");
  static_assert(SF_MAX_COMP == 4 && SF_MAX_SEP == 64 && SF_MAX_AXIS == 4096, "the messages name the limits");
  if (ncomp > SF_MAX_COMP) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_structure: more than 4 components");
  if (nsep > SF_MAX_SEP) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_structure: more than 64 separations");
  sf_seps seps = {};
  for (int k = 0; k < nsep; ++k) {
    if (sep[k] < 0 || sep[k] >= n[axis]) return fail(GFFT_ERR_INVALID, "gfft_ps_structure: a separation must lie in [0, n[axis])");
    seps.v[k] = sep[k];
  }
  if (n[axis] > SF_MAX_AXIS) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_structure: axis longer than 4096 (a workgroup stages whole lines)");
  if ((double)n[0] * (double)n[1] * (double)n[2] > 0x1p40) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_structure: more than 2^40 points");
  int rc = check_device();
  if (rc) return rc;
  // the workgroups' sums live in the stream's shared scratch: the first call allocates, later ones only enqueue
  void *slabs = nullptr;
  rc = scratch_get((hipStream_t)stream, sf_scratch_bytes(nsep * ncomp * SF_NVAL), &slabs);
  if (rc) return rc;
  HIP_TRY(launch_ps_structure(d_u, ncomp, n, axis, seps, nsep, lcomp, d_out, static_cast<double *>(slabs), precision,
                              (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_histogram(const void *d_u, int ncomp, int64_t count, const double *lo, const double *hi, int nbins, int64_t *d_out,
                      int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_u || !lo || !hi || !d_out || ncomp < 1 || count < 0 || nbins < 1 || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_histogram: bad argument");
  static_assert(ST_MAX_COMP == 4 && PD_MAX_BINS == 4096, "the messages name the limits");
  if (ncomp > ST_MAX_COMP) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_histogram: more than 4 components");
  pd_ranges rg = {};
  for (int c = 0; c < ncomp; ++c) {
    rg.lo[c] = lo[c];
    if (!pd_range(lo[c], hi[c], nbins, rg.w[c])) return fail(GFFT_ERR_INVALID, "gfft_ps_histogram: a range must be finite with lo < hi");
  }
  if (nbins > PD_MAX_BINS) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_histogram: more than 4096 bins");
  const int ncounters = ncomp * nbins, ntails = GFFT_PS_PDF_TAIL * ncomp;
  if (!pd_chunk_fits(count, pd_max_wg(ncounters))) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_histogram: more than 2^32 points per workgroup");
  int rc = check_device();
  if (rc) return rc;
  // the workgroups' tables live in the stream's shared scratch: the first call allocates, later ones only enqueue
  void *slabs = nullptr;
  rc = scratch_get((hipStream_t)stream, pd_scratch_bytes(ncounters, ntails), &slabs);
  if (rc) return rc;
  HIP_TRY(launch_ps_histogram(d_u, ncomp, count, rg, nbins, d_out, static_cast<uint32_t *>(slabs), precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_gradient_pdf(const void *d_A, int64_t count, int qx, double xlo, double xhi, int nbx, int qy, double ylo, double yhi,
                         int nby, int64_t *d_out, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  const bool joint = qy != GFFT_PS_Q_NONE;
  if (!d_A || !d_out || count < 0 || nbx < 1 || nby < 1 || qx < 0 || qx >= GFFT_PS_Q_COUNT || qy < GFFT_PS_Q_NONE ||
      qy >= GFFT_PS_Q_COUNT || (!joint && nby != 1) || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_gradient_pdf: bad argument");
  gp_axis ax = {qx, xlo, 0.0, nbx}, ay = {qy, 0.0, 1.0, 1};
  if (!pd_range(xlo, xhi, nbx, ax.w)) return fail(GFFT_ERR_INVALID, "gfft_ps_gradient_pdf: a range must be finite with lo < hi");
  if (joint) {
    ay = {qy, ylo, 0.0, nby};
    if (!pd_range(ylo, yhi, nby, ay.w)) return fail(GFFT_ERR_INVALID, "gfft_ps_gradient_pdf: a range must be finite with lo < hi");
  }
  static_assert(PD_MAX_BINS == 4096 && PD_MAX_COUNTERS == 16384, "the messages name the limits");
  if (!joint && nbx > PD_MAX_BINS) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_gradient_pdf: more than 4096 bins");
  if (joint && (int64_t)nbx * nby > PD_MAX_COUNTERS) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_gradient_pdf: more than 16384 joint bins");
  const int ncounters = joint ? nbx * nby : nbx, ntails = joint ? 2 : (int)GFFT_PS_PDF_TAIL;
  if (!pd_chunk_fits(count, pd_max_wg(ncounters))) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_gradient_pdf: more than 2^32 points per workgroup");
  int rc = check_device();
  if (rc) return rc;
  void *slabs = nullptr;
  rc = scratch_get((hipStream_t)stream, pd_scratch_bytes(ncounters, ntails), &slabs);
  if (rc) return rc;
  HIP_TRY(launch_ps_gradient_pdf(d_A, count, ax, ay, d_out, static_cast<uint32_t *>(slabs), precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_scale_axes(void *d_out, const void *d_f_hat, int ncomp, const void *d_v0, const void *d_v1, const void *d_v2,
                       int64_t n0, int64_t n1, int64_t n2, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum; a null vector is legal: that axis contributes no factor)
  if (!d_out || !d_f_hat || ncomp < 1 || n0 < 0 || n1 < 0 || n2 < 0 || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_scale_axes: bad argument");
  static_assert(SA_MAX_COMP == 4, "the message names the limit");
  if (ncomp > SA_MAX_COMP) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_scale_axes: more than 4 components");
  if (n0 > ((int64_t)1 << 30) || n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30))
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_scale_axes: axis longer than 2^30");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_scale_axes(d_out, d_f_hat, ncomp, d_v0, d_v1, d_v2, n0, n1, n2, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_scale_shells(void *d_out, const void *d_f_hat, int ncomp, const void *d_k0, const void *d_k1, const void *d_k2, double dk,
                         const double *d_tab, int nbins, int64_t n0, int64_t n1, int64_t n2, int precision, void *stream) {
  // (arguments first, as in gfft_ps_scale_axes)
  if (!d_out || !d_f_hat || !d_k0 || !d_k1 || !d_k2 || !d_tab || ncomp < 1 || nbins < 1 || !(dk > 0) || n0 < 0 || n1 < 0 || n2 < 0 ||
      (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_scale_shells: bad argument");
  static_assert(SA_MAX_COMP == 4, "the message names the limit");
  if (ncomp > SA_MAX_COMP) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_scale_shells: more than 4 components");
  if (n0 > ((int64_t)1 << 30) || n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30))
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_scale_shells: axis longer than 2^30");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_scale_shells(d_out, d_f_hat, ncomp, d_k0, d_k1, d_k2, dk, d_tab, nbins, n0, n1, n2, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_random_field(void *d_out, int ncomp, const int64_t n[3], const int64_t start[3], const int64_t N[3], const void *d_k0,
                         const void *d_k1, const void *d_k2, int project, double dk, const double *d_amp, int nbins, uint64_t seed,
                         uint64_t stream_id, int add, int precision, void *stream) {
  // (arguments first, as in gfft_ps_interp; d_amp may be NULL: every amplitude 1)
  if (!d_out || !n || !start || !N || !d_k0 || !d_k1 || !d_k2 || nbins < 1 || !(dk > 0) || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_random_field: bad argument");
  static_assert(RF_MAX_COMP == 4, "the message names the limit");
  if (ncomp < 1 || ncomp > RF_MAX_COMP) return fail(GFFT_ERR_INVALID, "gfft_ps_random_field: ncomp must be 1 ... 4");
  if (project && ncomp != 3) return fail(GFFT_ERR_INVALID, "gfft_ps_random_field: the projection needs 3 components");
  if (stream_id >> 62) return fail(GFFT_ERR_INVALID, "gfft_ps_random_field: stream_id must be below 2^62");
  for (int a = 0; a < 3; ++a)
    if (n[a] < 0 || N[a] < 1 || start[a] < 0 || start[a] > N[a] || n[a] > N[a] - start[a])
      return fail(GFFT_ERR_INVALID, "gfft_ps_random_field: a block needs n >= 0, N >= 1 and 0 <= start, start + n <= N");
  if (n[1] > ((int64_t)1 << 30) || n[2] > ((int64_t)1 << 30))
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_random_field: axis longer than 2^30");
  // the linear index of a mode of the full grid and c * count + e of the block both stay far inside 64 bits
  if ((double)N[0] * (double)N[1] * (double)N[2] > 0x1p60)
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_random_field: a grid of more than 2^60 points");
  if (int rc = check_device()) return rc;
  const rf_dims d = {n[1], n[2], start[0], start[1], start[2], N[0], N[1], N[2]};
  const rf_key key = {(uint32_t)stream_id, (uint32_t)(stream_id >> 32) << 2, (uint32_t)seed, (uint32_t)(seed >> 32)};
  HIP_TRY(launch_ps_random_field(d_out, ncomp, d, n[0] * n[1] * n[2], d_k0, d_k1, d_k2, project != 0, dk, d_amp, nbins, key, add,
                                 precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_interp(const void *d_c, int ncomp, const int64_t n[3], const int64_t start[3], const int64_t N[3],
                   const double inv_dx[3], const double *d_x, int64_t np, int order, double *d_out, int precision, void *stream) {
  // (arguments first, as in gfft_ps_spectrum)
  if (!d_c || !n || !start || !N || !inv_dx || !d_x || !d_out || ncomp < 1 || np < 0 ||
      (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_interp: bad argument");
  if (order != 2 && order != 4) return fail(GFFT_ERR_INVALID, "gfft_ps_interp: order must be 2 or 4");
  ip_dims d;
  for (int a = 0; a < 3; ++a) {
    if (n[a] < 1 || N[a] < 1 || start[a] < 0 || start[a] > N[a] || n[a] > N[a] - start[a])
      return fail(GFFT_ERR_INVALID, "gfft_ps_interp: a block needs n >= 1, N >= 1 and 0 <= start, start + n <= N");
    if (!std::isfinite(inv_dx[a]) || !(inv_dx[a] > 0)) return fail(GFFT_ERR_INVALID, "gfft_ps_interp: inv_dx must be finite and > 0");
    d.n[a] = n[a], d.start[a] = start[a], d.N[a] = N[a], d.inv_dx[a] = inv_dx[a];
  }
  static_assert(IP_MAX_COMP == 4, "the message names the limit");
  if (ncomp > IP_MAX_COMP) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_interp: more than 4 components");
  // an axis of 2^40 cells and a block of 2^60 values: the flat index of a load and b + j stay far inside int64
  if (N[0] > ((int64_t)1 << 40) || N[1] > ((int64_t)1 << 40) || N[2] > ((int64_t)1 << 40) ||
      (double)n[0] * (double)n[1] * (double)n[2] > 0x1p60)
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_interp: block too large");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_interp(d_c, ncomp, d, d_x, np, order, d_out, precision, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_spread(int64_t *d_acc, int ncomp, const int64_t n[3], const int64_t start[3], const int64_t N[3], const double inv_dx[3],
                   const double *d_x, const double *d_q, int64_t np, int order, int scale_exp, int64_t *d_skipped, void *stream) {
  // (arguments first, as in gfft_ps_interp, whose block refusals and size limits these are)
  if (!d_acc || !n || !start || !N || !inv_dx || !d_x || !d_q || !d_skipped || ncomp < 1 || np < 0)
    return fail(GFFT_ERR_INVALID, "gfft_ps_spread: bad argument");
  if (order != 2 && order != 4) return fail(GFFT_ERR_INVALID, "gfft_ps_spread: order must be 2 or 4");
  if (scale_exp < -1000 || scale_exp > 1000) return fail(GFFT_ERR_INVALID, "gfft_ps_spread: |scale_exp| must not exceed 1000");
  ip_dims d;
  for (int a = 0; a < 3; ++a) {
    if (n[a] < 1 || N[a] < 1 || start[a] < 0 || start[a] > N[a] || n[a] > N[a] - start[a])
      return fail(GFFT_ERR_INVALID, "gfft_ps_spread: a block needs n >= 1, N >= 1 and 0 <= start, start + n <= N");
    if (!std::isfinite(inv_dx[a]) || !(inv_dx[a] > 0)) return fail(GFFT_ERR_INVALID, "gfft_ps_spread: inv_dx must be finite and > 0");
    d.n[a] = n[a], d.start[a] = start[a], d.N[a] = N[a], d.inv_dx[a] = inv_dx[a];
  }
  static_assert(SPR_MAX_COMP == 4, "the message names the limit");
  if (ncomp > SPR_MAX_COMP) return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_spread: more than 4 components");
  if (N[0] > ((int64_t)1 << 40) || N[1] > ((int64_t)1 << 40) || N[2] > ((int64_t)1 << 40) ||
      (double)n[0] * (double)n[1] * (double)n[2] > 0x1p60)
    return fail(GFFT_ERR_UNSUPPORTED, "gfft_ps_spread: block too large");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_spread(d_acc, ncomp, d, d_x, d_q, np, order, std::ldexp(1.0, scale_exp), d_skipped, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_ps_spread_finish(void *d_out, int64_t *d_acc, int64_t count, double factor, int clear, int precision, void *stream) {
  if (!d_out || !d_acc || count < 0 || !std::isfinite(factor) || (precision != GFFT_F32 && precision != GFFT_F64))
    return fail(GFFT_ERR_INVALID, "gfft_ps_spread_finish: bad argument");
  if (int rc = check_device()) return rc;
  HIP_TRY(launch_ps_spread_finish(d_out, d_acc, count, factor, clear, precision, (hipStream_t)stream));
  return GFFT_OK;
}

}  // extern "C"
