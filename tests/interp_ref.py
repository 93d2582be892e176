"""numpy restatement of gfft_ps_scale_axes, SpectralOps.bspline_vectors and gfft_ps_interp (include/gfft.h), the reference of
tests/test_interp_host.py and tests/test_gpu_interp.py.

`interp` follows the definition operation by operation: s = x * inv_dx in double, the 2^51 guard, floor, one rounded
subtraction, the weights, the integer wrap, the block test, and the sum over the contributing points in the serial order
(j0, j1, j2).  The positions' arithmetic (s, floor, t) is always double -- it is part of the definition --; the weights, the
products and the sum are formed in `acc`: np.float64 for the serial double sum, np.longdouble for the reference that the
device's (differently ordered, possibly contracted) double sum is measured against.  Beside the result it returns
M_p = sum |w0 w1 w2 c| per particle and component, the scale of the rounding bound (order^3 + 64) 2^-53 M_p."""
import numpy as np

LIMIT = 2.0 ** 51
EPS = 2.0 ** -53


def scale_axes(f, v):
    """out[c][i0][i1][i2] = f[c][i0][i1][i2] * ((v0[i0] * v1[i1]) * v2[i2]) in the field's real type, the real and the imaginary
    part one multiply each; an axis whose vector is None contributes no factor; all None: a copy.  f: complex [..., n0, n1, n2]."""
    f = np.ascontiguousarray(f)
    rdt = np.float64 if f.dtype == np.complex128 else np.float32
    assert f.dtype in (np.complex128, np.complex64)
    g = None
    for axis, vi in enumerate(v):
        if vi is None:
            continue
        vi = np.asarray(vi)
        assert vi.dtype == rdt and vi.shape == (f.shape[-3 + axis],)
        shape = [1, 1, 1]
        shape[axis] = len(vi)
        vi = vi.reshape(shape)
        with np.errstate(all='ignore'):
            g = vi if g is None else (g * vi).astype(rdt)
    if g is None:
        return f.copy()
    out = np.empty_like(f)
    parts, oparts = f.view(rdt).reshape(f.shape + (2,)), out.view(rdt).reshape(f.shape + (2,))
    with np.errstate(all='ignore'):
        oparts[...] = parts * np.broadcast_to(g, f.shape[-3:])[..., None]
    return out


def bspline_vectors(N, order, real=True, slices=None, dtype=np.float64):
    """The three per-axis vectors of the order-4 prefilter over the spectral axes of a transform of global shape N (the last
    axis halved for a real transform), entry n (integer wavenumber) 1 / ((2 + cos(2 pi n / N_i)) / 3), computed in double and
    rounded to `dtype`; order 2: three Nones."""
    if order == 2:
        return (None, None, None)
    assert order == 4
    n = [np.fft.fftfreq(Ni, 1. / Ni) for Ni in N]
    if real:
        n[-1] = np.fft.rfftfreq(N[-1], 1. / N[-1])
    slices = slices or (slice(None),) * 3
    return tuple((1.0 / ((2.0 + np.cos(2 * np.pi * ni[sl].astype(int) / float(Ni))) / 3.0)).astype(dtype) for ni, Ni, sl in zip(n, N, slices))


def weights(t, order, acc=np.float64):
    """[order] arrays of weights at fractions t (an array in [0, 1]), formed in `acc`"""
    t = np.asarray(t).astype(acc)
    r = 1 - t
    if order == 2:
        return [r, t]
    six, three, four = acc(6), acc(3), acc(4)
    return [r * r * r / six, (three * t * t * t - six * t * t + four) / six, (three * r * r * r - six * r * r + four) / six, t * t * t / six]


def interp(c, x, inv_dx, order, N=None, start=(0, 0, 0), acc=np.longdouble):
    """(out [P][m], M [P][m]) in `acc`: this block's share of the interpolant of c = real [m][n0][n1][n2] (any float dtype;
    converted to double exactly) at x = double [P][3], and M = sum |w0 w1 w2 c| over the contributing points.  N defaults to
    the block's shape (the whole periodic grid); start is the block's first cell."""
    c = np.asarray(c)
    assert c.ndim == 4 and order in (2, 4)
    m, n = c.shape[0], c.shape[1:]
    N = tuple(int(v) for v in (n if N is None else N))
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    P = len(x)
    cd = c.astype(np.float64).astype(acc)
    with np.errstate(all='ignore'):
        s = x * np.asarray(inv_dx, dtype=np.float64)[None, :]                 # one multiply per axis, in double
        good = (np.abs(s) < LIMIT).all(axis=1)                            # (False for a NaN)
    sg = np.where(good[:, None], s, 0.0)
    i = np.floor(sg)
    t = sg - i                                                            # one rounded subtraction, in double
    base = i.astype(np.int64) - (1 if order == 4 else 0)
    w = [weights(t[:, a], order, acc) for a in range(3)]
    g = [[(base[:, a] + j) % N[a] for j in range(order)] for a in range(3)]           # numpy's %: non-negative for N > 0
    l = [[g[a][j] - int(start[a]) for j in range(order)] for a in range(3)]
    ok = [[(l[a][j] >= 0) & (l[a][j] < n[a]) for j in range(order)] for a in range(3)]
    out, M = np.zeros((P, m), dtype=acc), np.zeros((P, m), dtype=acc)
    with np.errstate(all='ignore'):
        for j0 in range(order):
            for j1 in range(order):
                w01 = w[0][j0] * w[1][j1]
                for j2 in range(order):
                    inside = ok[0][j0] & ok[1][j1] & ok[2][j2] & good
                    idx = np.flatnonzero(inside)
                    if not len(idx):
                        continue
                    vals = cd[:, l[0][j0][idx], l[1][j1][idx], l[2][j2][idx]].T           # [k][m]
                    term = (w01[idx] * w[2][j2][idx])[:, None] * vals
                    out[idx] += term
                    M[idx] += np.abs(term)
    out[~good] = np.nan
    M[~good] = np.nan
    return out, M


def bound(M, order, extra=0):
    """(order^3 + 64 + extra) 2^-53 M: what a double sum in any order, with any contraction, may differ from the exact one"""
    return (order ** 3 + 64 + extra) * EPS * np.asarray(M, dtype=np.float64)


def smooth_field(X, Y, Z):
    """f = sin x cos 2y cos z + cos(3x + y) sin z / 2 on [0, 2 pi)^3: the field of the convergence table"""
    return np.sin(X) * np.cos(2 * Y) * np.cos(Z) + 0.5 * np.cos(3 * X + Y) * np.sin(Z)


def convergence_points():
    """the 400 points of the convergence table: uniform in [-10, 20)^3, seed 5"""
    return np.random.default_rng(5).uniform(-10.0, 20.0, (400, 3))


def grid_samples(N):
    """smooth_field on the N^3 grid of [0, 2 pi)^3, double [N][N][N]"""
    ax = np.arange(N) * (2 * np.pi / N)
    return smooth_field(ax[:, None, None], ax[None, :, None], ax[None, None, :])


def coefficients(samples, order):
    """The B-spline coefficients of real samples [..., n0, n1, n2] by numpy's FFT: rfftn, the prefilter through `scale_axes`,
    irfftn -- the host twin of forward / scale_axes(bspline_vectors) / backward.  order 2: the samples themselves."""
    if order == 2:
        return np.array(samples, dtype=np.float64)
    N = samples.shape[-3:]
    fh = np.fft.rfftn(samples, axes=(-3, -2, -1))
    return np.fft.irfftn(scale_axes(fh, bspline_vectors(N, 4)), s=N, axes=(-3, -2, -1))
