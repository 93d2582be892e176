"""numpy restatement of gfft_ps_spread and gfft_ps_spread_finish (include/gfft.h), the reference of tests/test_spread_host.py
and tests/test_gpu_spread.py.

`spread_int` follows the definition operation by operation, every operation a numpy ufunc of its own (so nothing is contracted):
s = x * inv_dx, u = q * 2^scale_exp, the two guards, floor, one rounded subtraction, the weights in the header's sequence, the
integer wrap, the block test, k = rint(((w0 * w1) * w2) * u) and np.add.at on int64, which wraps modulo 2^64 as the device's
add does.  The integers it returns are what the device must hold, EXACTLY.  Beside them it returns, per point and component,
the number of contributions n_l, the sum with long-double weights and products (in units of q) and M_l = sum |w q|: the
fixed-point value acc 2^-scale_exp lies within n_l 2^-(scale_exp + 1) + 16 * 2^-53 M_l of that sum -- half a unit per add, plus
the roundings of three weights (at most 4 operations each: <= 12 eps together, eps = 2^-53), two products and one more product
with u (3 eps), to first order 15 eps, 16 with the second-order terms."""
import numpy as np

LIMIT = 2.0 ** 51
QLIMIT = 2.0 ** 62
EPS = 2.0 ** -53


def weights(t, order):
    """[order] double arrays: the header's sequence, one rounding per operation"""
    t = np.asarray(t, dtype=np.float64)
    r = 1.0 - t
    if order == 2:
        return [r, t]
    sixth = 1.0 / 6.0
    return [((r * r) * r) * sixth, ((t * t) * (3.0 * t - 6.0) + 4.0) * sixth, ((r * r) * (3.0 * r - 6.0) + 4.0) * sixth, ((t * t) * t) * sixth]


def _long_weights(t, order):
    t = np.asarray(t, dtype=np.float64).astype(np.longdouble)
    r = 1 - t
    if order == 2:
        return [r, t]
    six, three, four = np.longdouble(6), np.longdouble(3), np.longdouble(4)
    return [r * r * r / six, (three * t * t * t - six * t * t + four) / six, (three * r * r * r - six * r * r + four) / six, t * t * t / six]


def spread_int(q, x, inv_dx, order, N, start, n, scale_exp, exact=True, acc=None):
    """(acc int64 [m] + n, skipped, count int64 n, exact [m] + n long double, M [m] + n long double) for q = double [P][m] (or [P]),
    x = double [P][3], the block start .. start + n of the periodic grid N.  acc, if given, is ADDED TO (a copy is returned).
    exact=False skips the long-double sums (None, None): the integers alone, for large P."""
    assert order in (2, 4) and abs(int(scale_exp)) <= 1000
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    P = len(x)
    q = np.asarray(q, dtype=np.float64)
    q = q.reshape(P, 1) if q.ndim == 1 else q
    assert q.ndim == 2 and len(q) == P
    m = q.shape[1]
    N, start, n = (tuple(int(v) for v in t) for t in (N, start, n))
    cnt = int(np.prod(n))
    acc = np.zeros((m,) + n, dtype=np.int64) if acc is None else np.array(acc, dtype=np.int64).reshape((m,) + n)
    flat_acc = acc.reshape(m, cnt)
    count = np.zeros(cnt, dtype=np.int64)
    ex = np.zeros((m, cnt), dtype=np.longdouble) if exact else None
    M = np.zeros((m, cnt), dtype=np.longdouble) if exact else None
    with np.errstate(all='ignore'):
        s = x * np.asarray(inv_dx, dtype=np.float64)[None, :]                 # one multiply per axis
        u = q * np.ldexp(1.0, int(scale_exp))                                 # one multiply per component
        good = (np.abs(s) < LIMIT).all(axis=1) & (np.abs(u) < QLIMIT).all(axis=1)          # (False for a NaN)
    skipped = int(P - good.sum())
    sg = np.where(good[:, None], s, 0.0)
    i = np.floor(sg)
    t = sg - i                                                            # one rounded subtraction
    base = i.astype(np.int64) - (1 if order == 4 else 0)
    w = [weights(t[:, a], order) for a in range(3)]
    wl = [_long_weights(t[:, a], order) for a in range(3)] if exact else None
    g = [[(base[:, a] + j) % N[a] for j in range(order)] for a in range(3)]           # numpy's %: non-negative for N > 0
    l = [[g[a][j] - start[a] for j in range(order)] for a in range(3)]
    ok = [[(l[a][j] >= 0) & (l[a][j] < n[a]) for j in range(order)] for a in range(3)]
    ql = q.astype(np.longdouble) if exact else None
    for j0 in range(order):
        for j1 in range(order):
            for j2 in range(order):
                idx = np.flatnonzero(ok[0][j0] & ok[1][j1] & ok[2][j2] & good)
                if not len(idx):
                    continue
                at = (l[0][j0][idx] * n[1] + l[1][j1][idx]) * n[2] + l[2][j2][idx]
                ww = (w[0][j0][idx] * w[1][j1][idx]) * w[2][j2][idx]
                np.add.at(count, at, 1)
                for c in range(m):
                    np.add.at(flat_acc[c], at, np.rint(ww * u[idx, c]).astype(np.int64))          # (rint: ties to even)
                    if exact:
                        term = wl[0][j0][idx] * wl[1][j1][idx] * wl[2][j2][idx] * ql[idx, c]
                        np.add.at(ex[c], at, term)
                        np.add.at(M[c], at, np.abs(term))
    shape = (m,) + n
    return acc, skipped, count.reshape(n), (ex.reshape(shape) if exact else None), (M.reshape(shape) if exact else None)


def finish(acc, factor, dtype):
    """out = (dtype)((double)acc * factor): one conversion, one multiply, one narrowing"""
    with np.errstate(all='ignore'):
        return (np.asarray(acc, dtype=np.int64).astype(np.float64) * np.float64(factor)).astype(dtype)


def bound(count, M, scale_exp):
    """n_l 2^-(scale_exp + 1) + 16 * 2^-53 M_l, in long double, broadcast over the components"""
    return np.asarray(count, dtype=np.longdouble)[None] * np.ldexp(np.longdouble(1), -(int(scale_exp) + 1)) + 16 * EPS * np.asarray(M, dtype=np.longdouble)


def default_scale_exp(q):
    """floor(log2(2^62 / S)), S = max_c sum_p |q[p][c]| over the finite entries, clamped to +-1000; 0 for S = 0: by trial, not by
    the wrapper's frexp: the largest e with S * 2^e <= 2^62"""
    q = np.asarray(q, dtype=np.float64)
    q = q.reshape(len(q), 1) if q.ndim == 1 else q
    a = np.where(np.isfinite(q), np.abs(q), 0.0)
    S = float(a.sum(axis=0).max()) if a.size else 0.0
    if S == 0.0:
        return 0
    if not np.isfinite(S):
        return -1000
    e = -1000
    while e < 1000 and np.ldexp(np.longdouble(S), e + 1) <= np.ldexp(np.longdouble(1), 62):
        e += 1
    return e
