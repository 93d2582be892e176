"""numpy restatement of gfft_ps_random_field and gfft_ps_scale_shells (include/gfft.h), the reference of tests/test_random_host.py
and tests/test_gpu_random_field.py.

Philox4x32-10 runs on uint64 arrays (every word masked to 32 bits); the two uniforms of a call are exact doubles; everything
behind them -- log, sqrt, cos / sin of 2 pi u, the projection, the amplitude -- is np.longdouble (64-bit mantissa here), so
the reference's own error, a few 2^-64, is a thousandth of the bound's unit.

THE BOUND.  u = 2^-53, the unit roundoff of a double; an error of 1 ulp is at most 2 u relative.  Per part (real or
imaginary) of one component of one mode, with G the unprojected Gaussian vector of the mode (all components, both parts):

    rho = sqrt(-2 log u1)   log within 1 ulp (the device library's documented limit): 2 u relative on log u1, so after the
                            exact factor -2 and the square root u relative on rho; the square root's own limit of 1 ulp adds
                            2 u:                                                                              3 u |rho|
    cos / sin (pi x)        sincospi within 2 ulp:                                                            4 u |cos|
    rho * cos               one rounding:                                                                     1 u |G part|
                            so a part of G carries at most 8 u |part|, and the vector at most 8 u ||G||_2
    projection              in exact arithmetic a contraction of that error:                                  8 u ||G||_2
                            its own roundings: the dot product K . G (three products, two sums: at most 3 u |K| ||G||),
                            |K|^2 (all terms positive: 3 u relative) and the quotient (1 u) put p = K . G / |K|^2 within
                            7 u ||G|| / |K|; times k_j: 7 u ||G||; that product's rounding and the subtraction's, each at
                            most 1 u ||G||:                                                                   9 u ||G||_2
    times amp[b]            one rounding:                                                                     1 u |value|
    the reference           long double throughout:                                                          < 1 u

    |got - ref| <= C u amp ||G||_2  with  C = 8 + 9 + 1 + 1 = 19, taken as BOUND_C = 20

(without the projection 10 suffices; one constant serves both).  The conjugation of a mirror mode is exact.  In fp32 the one
rounding at the store adds 2^-24 |ref|.  An index, stream, component or mirror mistake gives differences of order amp ||G||.
"""
import numpy as np

LD = np.longdouble
BOUND_C = 20
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32(ctr, key):
    """Philox4x32-10 on uint64 arrays holding 32-bit words: ctr = four arrays (or ints), key = two; returns four arrays"""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) & MASK for x in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return c


def uniform(lo, hi):
    """(((hi << 32 | lo) >> 12) + 0.5) 2^-52 as exact doubles"""
    return ((((hi << np.uint64(32)) | lo) >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52


def wavenumbers(N, r2c, L=None, dtype=np.float64):
    """the three full wavenumber vectors of a spectral array over the physical grid N, as SpectralOps builds them"""
    L = (2 * np.pi,) * 3 if L is None else L
    k = [np.fft.fftfreq(n, 1. / n) for n in N]
    if r2c:
        k[2] = np.fft.rfftfreq(N[2], 1. / N[2])
    return [(ki.astype(int) * (2 * np.pi / Li)).astype(dtype) for ki, Li in zip(k, L)]


def shell_of(kx, ky, kz, dk):
    """b = floor(|k| / dk + 0.5) in double from wavenumbers converted to double first: the ONE shell definition"""
    kx, ky, kz = (np.asarray(a, dtype=np.float64) for a in (kx, ky, kz))
    return np.floor(np.sqrt((kx * kx + ky * ky) + kz * kz) / dk + 0.5)


def random_field(n, start, N, K, seed, stream, ncomp=3, project=True, dk=1.0, amp=None, nbins=1 << 30):
    """(field, zeroed, gnorm): the block start .. start + n of the field over the grid N as complex long double
    [ncomp] + n; which modes are stored as zero; amp ||G||_2 per mode (what the bound multiplies).  K = the BLOCK's three
    wavenumber vectors."""
    assert 0 <= stream < 1 << 62 and 1 <= ncomp <= 4 and (not project or ncomp == 3)
    g = np.meshgrid(*[np.arange(s, s + m, dtype=np.uint64) for s, m in zip(start, n)], indexing='ij')
    Nu = [np.uint64(x) for x in N]
    m = [np.where(gi == 0, np.uint64(0), Ni - gi) for gi, Ni in zip(g, Nu)]
    lin = lambda q: (q[0] * Nu[1] + q[1]) * Nu[2] + q[2]
    lg, lm = lin(g), lin(m)
    c = np.minimum(lg, lm)
    mirror = lm < lg
    zero = (lg == 0) | (2 * g[0] == Nu[0]) | (2 * g[1] == Nu[1]) | (2 * g[2] == Nu[2])
    k = np.meshgrid(*[np.asarray(ki, dtype=np.float64) for ki in K], indexing='ij')
    with np.errstate(invalid='ignore'):
        b = shell_of(k[0], k[1], k[2], dk)
    zero |= ~(b < nbins)
    bi = np.where(zero, 0, b).astype(np.int64)
    a = np.ones(lg.shape) if amp is None else np.asarray(amp, dtype=np.float64)[bi]
    zero |= a == 0
    G = np.zeros((ncomp,) + lg.shape, dtype=np.clongdouble)
    for comp in range(ncomp):
        r = philox4x32((c & MASK, c >> np.uint64(32), np.uint64(stream & 0xFFFFFFFF), np.uint64(((stream >> 32) << 2) | comp)),
                       (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)))
        u1, u2 = uniform(r[0], r[1]).astype(LD), uniform(r[2], r[3]).astype(LD)
        rho = np.sqrt(-2 * np.log(u1))
        ang = 8 * np.arctan(LD(1))                                               # 2 pi in long double
        G[comp] = rho * np.cos(ang * u2) + 1j * (rho * np.sin(ang * u2))
    gnorm = np.sqrt((np.abs(G) ** 2).sum(axis=0)).astype(np.float64) * np.abs(a)
    if project:
        kl = [ki.astype(LD) for ki in k]
        kk = kl[0] * kl[0] + kl[1] * kl[1] + kl[2] * kl[2]
        kk = np.where(kk == 0, LD(1), kk)
        p = (kl[0] * G[0] + kl[1] * G[1] + kl[2] * G[2]) / kk
        G = np.stack([G[j] - kl[j] * p for j in range(3)])
    G = G * a.astype(LD)
    G = np.where(mirror[None], np.conj(G), G)
    G = np.where(zero[None], np.clongdouble(0), G)
    return G, zero, np.where(zero, 0.0, gnorm)


def full_field(N, r2c, seed, stream, **kw):
    """the whole spectral array over the grid N (r2c: the stored half of the last axis) with L = 2 pi"""
    n = (N[0], N[1], N[2] // 2 + 1 if r2c else N[2])
    return random_field(n, (0, 0, 0), N, wavenumbers(N, r2c), seed, stream, **kw)


def bound(ref, gnorm, fp32=False):
    """per part: BOUND_C 2^-53 amp ||G||_2 (+ 2^-24 |ref| for the one rounding to float), broadcast over the components"""
    base = BOUND_C * 2.0 ** -53 * gnorm[None]
    if not fp32:
        return base, base
    return base + 2.0 ** -24 * np.abs(ref.real).astype(np.float64), base + 2.0 ** -24 * np.abs(ref.imag).astype(np.float64)


def worst_share(got, ref, gnorm, fp32=False):
    """max over the parts of |got - ref| / bound (0 where both are 0); a zeroed mode must be exactly zero"""
    br, bi = bound(ref, gnorm, fp32)
    er = np.abs(got.real.astype(LD) - ref.real).astype(np.float64)
    ei = np.abs(got.imag.astype(LD) - ref.imag).astype(np.float64)
    zero = gnorm == 0
    assert not er[:, zero].any() and not ei[:, zero].any(), 'a zeroed mode is not zero'
    keep = ~zero
    return float(max((er[:, keep] / br[:, keep]).max(initial=0.0), (ei[:, keep] / bi[:, keep]).max(initial=0.0)))


def scale_shells(f, K, tab, dk):
    """f [ncomp, n0, n1, n2] complex64 / complex128 times (real)tab[b] per part, +0 where b >= len(tab): the same bits as the
    kernel.  K = the block's wavenumber vectors in the field's precision."""
    f = np.asarray(f)
    rdt = np.float32 if f.dtype == np.complex64 else np.float64
    k = np.meshgrid(*[np.asarray(ki, dtype=np.float64) for ki in K], indexing='ij')
    with np.errstate(invalid='ignore'):
        b = shell_of(k[0], k[1], k[2], dk)
    keep = b < len(tab)
    g = np.asarray(tab, dtype=np.float64).astype(rdt)[np.where(keep, b, 0).astype(np.int64)]
    out = np.zeros_like(f)
    with np.errstate(invalid='ignore', over='ignore'):
        re, im = f.real * g[None], f.imag * g[None]
    out.real = np.where(keep[None], re, rdt(0))
    out.imag = np.where(keep[None], im, rdt(0))
    return out


def spectrum(f, K, w2, dk, nbins):
    """E(b) = sum over shell b of 0.5 w2[i2] sum_c |f_c|^2 in double, the host twin of SpectralOps.spectrum's row 0"""
    k = np.meshgrid(*[np.asarray(ki, dtype=np.float64) for ki in K], indexing='ij')
    b = shell_of(k[0], k[1], k[2], dk)
    e = 0.5 * np.asarray(w2, dtype=np.float64)[None, None, :] * (np.abs(np.asarray(f).astype(np.complex128)) ** 2).sum(axis=0)
    keep = b < nbins
    return np.bincount(b[keep].astype(np.int64), weights=e[keep], minlength=nbins)[:nbins]


def shell_table(E_target, E_have):
    """sqrt(E_target / E_have) per shell, 0 where E_have == 0: the table of SpectralOps.random_field"""
    E_target, E_have = np.asarray(E_target, dtype=np.float64), np.asarray(E_have, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(E_have == 0, 0.0, np.sqrt(E_target / E_have))
