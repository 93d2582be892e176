"""Reference for the four base kernels of the pseudo-spectral layer (TEST INFRASTRUCTURE): gfft_ps_curl, gfft_ps_cross,
gfft_ps_project and gfft_ps_rk_stage, evaluated by numpy in np.longdouble from the SAME rounded inputs the device gets.

    curl       out = i (k x u):   out_a = i (k_b u_c - k_c u_b), (a, b, c) cyclic
    cross      out = a x b:       out_a = a_b b_c - a_c b_b
    projected  p = (sum_i d_i k_i) / |k|^2 (|k|^2 = 0 taken as 1);   out_j = d_j - k_j p - nu |k|^2 u_j
    rk_stage   u = u0 + cb du;   u1 = u1 + ca du

The wavenumbers are the per-axis vectors of the block IN THE FIELD'S PRECISION (what the kernel reads), widened; they are not
recomputed in float64.  nu, cb and ca are the doubles passed to the call.  A complex field is handled as its two real parts
(`parts`: a trailing axis of length 2): every one of these operations acts on the real and the imaginary parts separately --
the wavenumbers and coefficients are real, and the factor i of the curl only swaps the parts and negates one --, so a NaN in
one part of one input stays in that part of the outputs it feeds, here as on the device.  Every function returns real
long-double arrays; `join` makes complex numbers of a parts array.

np.longdouble is the x87 80-bit format where these tests run (64-bit significand, eps = 2^-63); the reference's own
rounding, a dozen roundings of 2^-64 S, is 2^-12 of the fp64 bounds below and is neglected.  Where np.longdouble is only a
double the fp64 comparisons lose that margin (the bounds leave 2.5 of 8 and 0.5 ... 1 of 2 eps S); the fp32 ones lose nothing.

Bounds, per real scalar, with eps = 2^-23 or 2^-52 (cases.EPS) and u = eps / 2 the unit roundoff.  They are derived from the
kernels' operation order (csrc/spectral.hip), not measured.  A fused multiply-add removes roundings and adds none, so the
counts hold for any contraction the compiler chooses.  Each count is the number of factors (1 + delta), |delta| <= u, that
multiply one term of the exact result; second-order terms (11 u)^2 / 2 are below 2^-40 of the first-order ones.

  curl, cross:  |got - ref| <= 2 eps S,  S = |k_b||u_c| + |k_c||u_b|  (cross: |a_b||b_c| + |a_c||b_b|), on the part that
      feeds the output part.  fl(fl(x y) - fl(z w)): each term is rounded once as a product and once in the subtraction:
      2 unit roundoffs = 1 eps S.  (Counting the three operations of an output gives 3; no term sees more than 2 of them.)
  rk_stage:     |got - ref| <= 2 eps S,  S = |u0| + |cb||du| for u and |u1| + |ca||du| for u1.  The term cb du sees the
      conversion of the double cb to the field's precision, the product and the add: 3; u0 sees the add: 1.  At most
      3 unit roundoffs = 1.5 eps S.
  projection:   |got - ref| <= 8 eps S_j,  S_j = |d_j| + |k_j| (sum_i |d_i||k_i|) / |k|^2 + |nu| |k|^2 |u_j|.
      The kernel forms  kk = (kx kx + ky ky) + kz kz;  inv = 1 / kk;  p = (d_0 (kx inv) + d_1 (ky inv)) + d_2 (kz inv);
      d_j -= p k_j;  v = (real)nu kk;  d_j -= v u_j.  Factors (1 + delta) on each quantity:
          kk            3   (a square and two adds on its first term; all terms are >= 0, so this is relative to kk itself)
          inv           4   (+ the division)
          k_i inv       5
          d_i (k_i inv) 6
          p             8   (two adds on its first two terms), relative to sum_i |d_i||k_i| / |k|^2
          p k_j         9
          v             5   (conversion of nu, kk, the product);   v u_j  6
          d_j - p k_j       1 more on both: d_j 1, the projection term 10
          ... - v u_j       1 more on all three: d_j 2, the projection term 11, the viscous term 7
      At most 11 unit roundoffs = 5.5 eps S_j; the bound asked for is 8 eps S_j.  At |k|^2 = 0 every k_j is 0, the two
      subtracted terms are exact zeros and d_j comes back in value (the sign of a zero may change).
  divergence (nu = 0):  sum_j k_j ref_j = 0 exactly where |k|^2 > 0 and every k_j is 0 elsewhere, so
      |sum_j k_j got_j| = |sum_j k_j (got_j - ref_j)| <= 8 eps sum_j |k_j| S_j  (`divergence`, `divergence_size`): evaluated
      from the device's output alone.

An unfused numpy emulation of the operation order (tests/test_vector_host.py) reaches 1.9 eps S for the projection, 0.9 eps S for
curl and cross, 1.0 eps S for the stage and 0.11 of the divergence bound at the test shapes: measurements beside the
derivation, not its source.
"""
import numpy as np

LD = np.longdouble

C_CURL = C_CROSS = C_RK = 2.0           # |got - ref| <= C eps S
C_PROJECT = 8.0


def parts(z):
    """The real scalars of a field in long double: a complex array gets a trailing axis (re, im), a real one stays as it is"""
    z = np.asarray(z)
    if z.dtype.kind == 'c':
        return np.stack([z.real.astype(LD), z.imag.astype(LD)], axis=-1)
    return z.astype(LD)


def join(p):
    """complex long double from a parts array"""
    out = np.empty(p.shape[:-1], dtype=np.clongdouble)
    out.real, out.imag = p[..., 0], p[..., 1]
    return out


def _mesh(k, trailing):
    """the three wavenumber vectors, widened, broadcastable over [n0][n1][n2] + a parts axis if `trailing`"""
    tail = (None,) * trailing
    k = [np.asarray(ki).astype(LD) for ki in k]
    return (k[0][(slice(None), None, None) + tail], k[1][(None, slice(None), None) + tail],
            k[2][(None, None, slice(None)) + tail])


def _cross_terms(a, b):
    """((x, y) per output component) with out = x - y: the two products of each component of a x b"""
    return [(a[1] * b[2], a[2] * b[1]), (a[2] * b[0], a[0] * b[2]), (a[0] * b[1], a[1] * b[0])]


def cross(a, b):
    """a x b of real fields [3] + shape"""
    return np.array([x - y for x, y in _cross_terms(parts(a), parts(b))])


def cross_size(a, b):
    return np.array([x + y for x, y in _cross_terms(np.abs(parts(a)), np.abs(parts(b)))])


def curl(u_hat, k):
    """i (k x u_hat) as parts [3] + block + [2]: with w = k x u taken part by part, (re, im) of the result is (-w.im, w.re)"""
    w = np.array([x - y for x, y in _cross_terms(_mesh(k, 1), parts(u_hat))])
    return np.stack([-w[..., 1], w[..., 0]], axis=-1)


def curl_size(u_hat, k):
    """S of `curl`, laid out as its result: the real part of an output is fed by the imaginary parts of u_hat and vice versa"""
    s = np.array([x + y for x, y in _cross_terms([np.abs(m) for m in _mesh(k, 1)], np.abs(parts(u_hat)))])
    return np.stack([s[..., 1], s[..., 0]], axis=-1)


def projected(du, u_hat, k, nu):
    """du - k (du . k) / |k|^2 - nu |k|^2 u_hat as parts [3] + block + [2]"""
    d, u, K = parts(du), parts(u_hat), _mesh(k, 1)
    kk = K[0] * K[0] + K[1] * K[1] + K[2] * K[2]
    p = (d[0] * K[0] + d[1] * K[1] + d[2] * K[2]) / np.where(kk == 0, LD(1), kk)
    v = LD(float(nu)) * kk
    return np.array([d[j] - K[j] * p - v * u[j] for j in range(3)])


def projected_size(du, u_hat, k, nu):
    d, u, K = np.abs(parts(du)), np.abs(parts(u_hat)), [np.abs(m) for m in _mesh(k, 1)]
    kk = K[0] * K[0] + K[1] * K[1] + K[2] * K[2]
    p = (d[0] * K[0] + d[1] * K[1] + d[2] * K[2]) / np.where(kk == 0, LD(1), kk)
    v = LD(abs(float(nu))) * kk
    return np.array([d[j] + K[j] * p + v * u[j] for j in range(3)])


def divergence(got, k):
    """sum_j k_j got_j per mode and part, in long double, from a result alone: block + [2]"""
    g, K = parts(got), _mesh(k, 1)
    return K[0] * g[0] + K[1] * g[1] + K[2] * g[2]


def divergence_size(du, k):
    """sum_j |k_j| S_j with S_j of the projection at nu = 0: what the divergence of a projected field may be off zero by, over
    C_PROJECT eps"""
    S, K = projected_size(du, np.zeros_like(du), k, 0.0), [np.abs(m) for m in _mesh(k, 1)]
    return K[0] * S[0] + K[1] * S[1] + K[2] * S[2]


def rk_stage(u0, u1, du, cb, ca):
    """(u0 + cb du, u1 + ca du), real scalar by real scalar; the first is None where u0 is"""
    d = parts(du)
    return (None if u0 is None else parts(u0) + LD(float(cb)) * d), parts(u1) + LD(float(ca)) * d


def rk_size(u0, u1, du, cb, ca):
    d = np.abs(parts(du))
    return (None if u0 is None else np.abs(parts(u0)) + LD(abs(float(cb))) * d), np.abs(parts(u1)) + LD(abs(float(ca))) * d


def ratio(got, ref, S, c, eps):
    """|got - ref| / (c eps S) per real scalar, `got` in the precision under test.  NaN where the reference is NaN -- and the
    caller asserts that `got` has its NaNs exactly there; where S = 0 the result is exact: 0 if got == ref, else inf."""
    g = parts(got)
    assert g.shape == ref.shape == S.shape, (g.shape, ref.shape, S.shape)
    err = np.abs(g - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(S > 0, err / (LD(c * eps) * S), np.where(err == 0, LD(0), LD(np.inf)))
    return np.where(np.isnan(ref), LD(np.nan), r)


def assert_within(got, ref, S, c, eps, what):
    """Every element within c eps S of the reference, NaN where and only where the reference has one; prints and returns the
    worst ratio"""
    g = parts(got)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(g), nan), (what, 'NaNs differ from the reference', int(np.isnan(g).sum()), int(nan.sum()))
    r = ratio(got, ref, S, c, eps)[~nan]
    worst = float(r.max()) if r.size else 0.0
    print('%s: worst / bound = %.3f' % (what, worst))
    assert worst <= 1.0, (what, 'worst / bound', worst, int((r > 1).sum()), 'of', r.size)
    return worst
