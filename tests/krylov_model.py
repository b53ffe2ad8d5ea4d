"""numpy model of the Krylov kernels of dedflow_amd/csrc (k_blas.hip, k_cgs.hip, k_cgs_block.hip): one function per
launcher, with the launcher's argument meaning, on host arrays.  Test infrastructure only: no GPU, no import of the library.

Matrices are flat column-major arrays with a leading dimension, as the launchers take them: column j of the basis is
Q[j * ldq : j * ldq + n], column j of the Hessenberg matrix is H[j * ldh : ...].  In-place arguments are modified in
place.  Every function takes a `dtype`:

  np.longdouble  the high-precision runs (64-bit significand on x86),
  np.float64     the device's own format (the GMRES loop of the CPU test, the order-independence check),
  np.int64       the exact tier: inputs are small integers, every product and partial sum is an integer below 2**53,
                 so a float64 kernel must reproduce the result bit for bit in any reduction order.  Where a kernel
                 scales by a power of two (1 / nrm, dyadic alpha coefficients) the integer part is done in int64 and
                 the exact scaling in float64.

`order` (reductions only) fixes the summation order for the order-independence check: a callable that maps a length
to an index array over the reduced axis, which is then summed strictly left to right; `peak` (a one-element list)
receives the largest intermediate met.  `col_order` does the same for the column loop of an update.
"""
import numpy as np

U = 2.0 ** -53  # unit roundoff of float64
HAVE_EXTENDED = bool(np.finfo(np.longdouble).eps < 2e-19)
EXTENDED_REASON = "np.longdouble has no 64-bit significand on this host (eps = %g)" % np.finfo(np.longdouble).eps


def _conv(a, dtype):
    a = np.asarray(a)
    if dtype == np.int64:
        r = a.astype(np.int64)
        assert np.array_equal(r, a), "exact tier needs integer input"
        return r
    return a.astype(dtype)


def _note(peak, *vals):
    if peak is not None:
        for v in vals:
            v = np.asarray(v)
            if v.size:
                peak[0] = max(peak[0], float(np.abs(v).max()))


def _sum(terms, dtype, order=None, peak=None):
    """sum of a 1-D array of terms; strict left-to-right in `order` when one is given.  Like every accumulator of
    the kernels the sum starts from +0.0, so that a lone -0.0 term gives +0.0"""
    if order is None:
        return dtype(0) + terms.sum(dtype=dtype)
    c = np.cumsum(np.concatenate([np.zeros(1, terms.dtype), terms[order(terms.size)]]), dtype=dtype)
    _note(peak, terms, c)
    return c[-1]


def _col(Q, j, ld, n):
    return Q[j * ld: j * ld + n]


# ---- reductions and the fused CGS pair -----------------------------------------------------------------------------
def ddot(n, x, y, dtype, order=None, peak=None):
    return _sum(_conv(x[:n], dtype) * _conv(y[:n], dtype), dtype, order, peak)


def dnrm2_sq(n, x, dtype, order=None, peak=None):
    """sum(x*x); dfl_dnrm2 returns its square root"""
    return ddot(n, x, x, dtype, order, peak)


def cgs_dots(n, ncol, Q, ldq, w, dtype, order=None, peak=None):
    """h[j] = Q[:, j] . w"""
    wv = _conv(w[:n], dtype)
    h = np.zeros(ncol, dtype)
    for j in range(ncol):
        h[j] = _sum(_conv(_col(Q, j, ldq, n), dtype) * wv, dtype, order, peak)
    return h


def cgs_update(n, ncol, Q, ldq, h, w, dtype, order=None, col_order=None, peak=None):
    """w - Q h and sum(w*w) of the result (the launcher takes the square root when asked to)"""
    acc = _conv(w[:n], dtype).copy()
    hv = _conv(h[:ncol], dtype)
    for j in (range(ncol) if col_order is None else col_order(ncol)):
        t = _conv(_col(Q, j, ldq, n), dtype) * hv[j]
        acc -= t
        _note(peak, t, acc)
    return acc, _sum(acc * acc, dtype, order, peak)


def gemv_n(n, ncol, Q, ldq, c, dtype, col_order=None, peak=None):
    """y = Q[:, 0:ncol] c"""
    acc = np.zeros(n, dtype)
    cv = _conv(c[:ncol], dtype)
    for j in (range(ncol) if col_order is None else col_order(ncol)):
        t = _conv(_col(Q, j, ldq, n), dtype) * cv[j]
        acc += t
        _note(peak, t, acc)
    return acc


def scal_inv(n, scale, x, dtype):
    """x * (1 / scale): the reciprocal first, as scal_inv_dev does"""
    if dtype == np.int64:  # exact tier: a power-of-two scale
        s = 1.0 / float(scale)
        assert np.frexp(s)[0] == 0.5
        return _conv(x[:n], np.int64).astype(np.float64) * s
    return _conv(x[:n], dtype) * (dtype(1) / dtype(scale))


# ---- the Givens step -------------------------------------------------------------------------------------------------
def drotg(a, b, dtype):
    """drotg_dev: returns (r, z, c, s) for the pair (a, b)"""
    one, zero = dtype(1), dtype(0)
    roe = a if abs(a) > abs(b) else b
    scale = abs(a) + abs(b)
    if scale == 0:
        return zero, zero, one, zero
    ta, tb = a / scale, b / scale
    r = scale * np.sqrt(ta * ta + tb * tb)
    if roe < 0:
        r = -r
    c, s = a / r, b / r
    z = one
    if abs(a) > abs(b):
        z = s
    if abs(b) >= abs(a) and c != 0:
        z = one / c
    return r, z, c, s


def givens_step(it, nrm, H, ldh, gv, beta, res_hist, dtype=np.float64):
    """givens_step_block on column `it` of H (in place): H[it+1, it] = nrm, the earlier rotations, drotg, the
    residual recurrence.  All arrays are of `dtype` already."""
    col = H[it * ldh: it * ldh + it + 2]
    col[it + 1] = nrm
    for i in range(it):
        c, s = gv[2 * i], gv[2 * i + 1]
        x, y = col[i], col[i + 1]
        col[i] = c * x + s * y
        col[i + 1] = c * y - s * x
    r, _, gc, gs = drotg(col[it], col[it + 1], dtype)
    col[it] = r
    gv[2 * it], gv[2 * it + 1] = gc, gs
    col[it + 1] = 0
    b0 = beta[it]
    beta[it + 1] = -gs * b0
    beta[it] = b0 * gc
    if res_hist is not None:
        res_hist[it] = abs(beta[it + 1])


def pythagoras_norm(h, ww, dtype):
    """(nrm, flag) of gmres_givens_pythagoras_kernel: r = ww - sum h_j^2 summed left to right, flag when r < 1e-6 ww,
    r clamped at 0.  The flag is the kernel's float64 decision in every dtype."""
    hv = _conv(h, dtype)
    hh = dtype(0)
    for v in hv:
        hh = hh + v * v
    ww = _conv(ww, dtype)[()]
    r = ww - hh
    flag = int(float(r) < 1e-6 * float(ww))
    if r < 0:
        r = dtype(0)
    if dtype == np.int64:
        return np.sqrt(np.float64(r)), flag
    return np.sqrt(r), flag


def update_pc_givens(nrows, N, ncol, Q, ldq, hraw, w, dinv33, dinv1, z, z4, it, H, ldh, gv, beta, res_hist, dtype):
    """cgs_update_pc_kernel: w -= Q h on the owned rows (3 velocity rows and the pressure row of nodes 0..nrows-1),
    w *= 1/nrm, z = M^-1 w (3x3 block in the kernel's A[0],A[3],A[6] order, scalar pressure), z4 interleaved, column
    copy and Givens step.  w, z, z4 (float64 arrays, or None for z4) and H, gv, beta, res_hist are updated in place;
    returns (nrm, flag).  dtype int64: integer update, exact power-of-two scaling and Jacobi sums in float64."""
    nrm, flag = pythagoras_norm(hraw[:ncol], hraw[ncol], dtype)
    wt = np.float64 if dtype == np.int64 else dtype
    hv = _conv(hraw[:ncol], dtype)
    i = np.arange(nrows)
    rows = np.concatenate([3 * i, 3 * i + 1, 3 * i + 2, 3 * N + i])
    acc = _conv(w[rows], dtype)
    for j in range(ncol):
        acc = acc - _conv(Q[j * ldq + rows], dtype) * hv[j]
    s = wt(1) / wt(nrm)
    if dtype == np.int64:
        assert np.frexp(float(s))[0] == 0.5, "exact tier needs nrm = 2**k"
    acc = acc.astype(wt) * s
    a0, a1, a2, ap = acc[:nrows], acc[nrows:2 * nrows], acc[2 * nrows:3 * nrows], acc[3 * nrows:]
    A = _conv(dinv33[:9 * nrows], wt).reshape(nrows, 9)
    z0 = A[:, 0] * a0 + A[:, 3] * a1 + A[:, 6] * a2
    z1 = A[:, 1] * a0 + A[:, 4] * a1 + A[:, 7] * a2
    z2 = A[:, 2] * a0 + A[:, 5] * a1 + A[:, 8] * a2
    zp = ap * _conv(dinv1[:nrows], wt)
    w[rows] = acc
    z[rows] = np.concatenate([z0, z1, z2, zp])
    if z4 is not None:
        z4[:4 * nrows] = np.stack([z0, z1, z2, zp], axis=1).reshape(-1)
    H[it * ldh: it * ldh + ncol] = hraw[:ncol]
    givens_step(it, H.dtype.type(nrm), H, ldh, gv, beta, res_hist, H.dtype.type)
    return nrm, flag


def trsv_upper(m, H, ldh, beta, dtype):
    """y with H[0:m, 0:m] y = beta[0:m], column-oriented back substitution as gmres_trsv_kernel runs it"""
    b = _conv(beta[:m], dtype).copy()
    for i in range(m - 1, -1, -1):
        col = _conv(H[i * ldh: i * ldh + i + 1], dtype)
        b[i] = b[i] / col[i]
        b[:i] -= col[:i] * b[i]
    return b


# ---- the Newton driver's state algebra ------------------------------------------------------------------------------
def norms4(N, F, dtype, order=None, peak=None):
    """sums of squares of the u, p, phi, T segments of a 6N vector (the launcher takes square roots when asked to)"""
    out = np.zeros(4, dtype)
    for seg, (b, ln) in enumerate(((0, 3 * N), (3 * N, N), (4 * N, N), (5 * N, N))):
        v = _conv(F[b: b + ln], dtype)
        out[seg] = _sum(v * v, dtype, order, peak)
    return out


def _dyadic(c, dtype):
    """coefficient for the exact tier: integers after scaling by 4 (0.25, 0.5, 2 and their like)"""
    if dtype == np.int64:
        k = int(round(c * 4))
        assert k == c * 4
        return np.int64(k)
    return dtype(c)


def _undyadic(v, dtype, power):
    return v.astype(np.float64) / 4.0 ** power if dtype == np.int64 else v


def alpha_states(N, wgold, dwgold, dwg, f1_0, f1_1, f2_0, f2_1, xg, dtype, want_nodep=False, want_nodexu=False):
    """alpha_states_kernel: returns (wgalpha, dwgalpha, nodep or None, nodexu or None); the pressure slot [3N, 4N)
    takes dwgalpha = dwg and wgalpha = 0"""
    o, d0, d1 = _conv(wgold[:6 * N], dtype), _conv(dwgold[:6 * N], dtype), _conv(dwg[:6 * N], dtype)
    one = np.int64(4) if dtype == np.int64 else dtype(1)
    d = _undyadic(_dyadic(f1_1, dtype) * d1 + _dyadic(f1_0, dtype) * d0, dtype, 1)
    w = _undyadic(_dyadic(f2_1, dtype) * d1 + _dyadic(f2_0, dtype) * d0 + one * o, dtype, 1)
    p = slice(3 * N, 4 * N)
    d[p] = d1[p]
    w[p] = 0
    nodep = nodexu = None
    if want_nodep:
        x = _conv(xg[:3 * N], dtype).astype(w.dtype).reshape(N, 3)
        seg = lambda a, k: a[(2 + k) * N: (3 + k) * N]
        nodep = np.zeros((N, 16), w.dtype)
        nodep[:, 0:3] = x
        nodep[:, 3:6] = w[:3 * N].reshape(N, 3)
        nodep[:, 6], nodep[:, 7] = seg(w, 2), seg(w, 3)
        nodep[:, 8:11] = d[:3 * N].reshape(N, 3)
        nodep[:, 11], nodep[:, 12], nodep[:, 13] = seg(d, 1), seg(d, 2), seg(d, 3)
        if want_nodexu:
            nodexu = np.zeros((N, 8), w.dtype)
            nodexu[:, 0:6] = nodep[:, 0:6]
            nodexu = nodexu.reshape(-1)
        nodep = nodep.reshape(-1)
    return w, d, nodep, nodexu


def alpha_predict(N, fac, dwg, dtype):
    """dwg * fac except the pressure slot"""
    d = _conv(dwg[:6 * N], dtype)
    r = _undyadic(_dyadic(fac, dtype) * d, dtype, 1)
    r[3 * N: 4 * N] = d[3 * N: 4 * N]
    return r


def alpha_correct(N, c0, c1, wgold, dwgold, dwg, dtype):
    """(wgold + c0 dwgold + c1 dwg except the pressure slot, dwgold = dwg on all slots)"""
    o, d0, d1 = _conv(wgold[:6 * N], dtype), _conv(dwgold[:6 * N], dtype), _conv(dwg[:6 * N], dtype)
    one = np.int64(4) if dtype == np.int64 else dtype(1)
    w = _undyadic(_dyadic(c1, dtype) * d1 + _dyadic(c0, dtype) * d0 + one * o, dtype, 1)
    w[3 * N: 4 * N] = o[3 * N: 4 * N]
    return w, (d1.astype(np.float64) if dtype == np.int64 else d1.copy())


# ---- Tier A input generators (shared by the device tests and the CPU check of their exactness) ----------------------
def gen_cgs(seed, n, ncol, ldq):
    """integer basis in [-3, 3] (gaps of ldq > n left at 0 for the caller to fill), w in [-4, 4], coefficients in
    [-3, 3] drawn independently of the dots"""
    rng = np.random.default_rng(seed)
    Q = np.zeros(ncol * ldq)
    for j in range(ncol):
        Q[j * ldq: j * ldq + n] = rng.integers(-3, 4, size=n)
    w = rng.integers(-4, 5, size=n).astype(np.float64)
    h = rng.integers(-3, 4, size=ncol).astype(np.float64)
    return Q, w, h


def gen_pc(seed, nrows, N, ncol, ldq, k):
    """owned rows of Q / w as gen_cgs, integer Jacobi blocks in [-2, 2], hraw = [h, sum(h*h) + 4**k]"""
    rng = np.random.default_rng(seed)
    i = np.arange(nrows)
    rows = np.concatenate([3 * i, 3 * i + 1, 3 * i + 2, 3 * N + i])
    Qv = rng.integers(-3, 4, size=(ncol, rows.size)).astype(np.float64)
    wv = rng.integers(-4, 5, size=rows.size).astype(np.float64)
    h = rng.integers(-3, 4, size=ncol).astype(np.float64)
    hraw = np.concatenate([h, [np.sum(h * h) + 4.0 ** k]])
    dinv33 = rng.integers(-2, 3, size=9 * nrows).astype(np.float64)
    dinv1 = rng.integers(-2, 3, size=nrows).astype(np.float64)
    return rows, Qv, wv, hraw, dinv33, dinv1


def gen_states(seed, N, count):
    """`count` integer 6N state vectors in [-8, 8]"""
    rng = np.random.default_rng(seed)
    return [rng.integers(-8, 9, size=6 * N).astype(np.float64) for _ in range(count)]


# The covering list of the CGS family: (n, ncol, ldq - n, pointer offset in doubles).  Every value of every axis meets
# both alignments and both stride parities (n + pad even / odd) at least once; the two largest n stay at ncol <= 9.
CGS_N = (1, 2, 3, 255, 1023, 1024, 1025, 2047, 2048, 2049, 20014, 20015, 256 * 2048 + 7, 2097152 + 2049)
CGS_NCOL = (1, 7, 8, 9, 37, 128, 129, 200)
CGS_PAD = (0, 1, 5)


def _pad_for(n, parity, alt):
    """a pad from CGS_PAD that makes the stride n + pad even (parity 0) or odd (1); 1 and 5 alternate"""
    if ((n + 0) & 1) == parity:
        return 0
    return 5 if alt else 1


def cgs_cases():
    cases = []
    quad = ((0, 0), (0, 1), (1, 0), (1, 1))  # (pointer offset, stride parity)
    for k, n in enumerate(CGS_N):  # every n
        ncols = CGS_NCOL if n < 100000 else (1, 7, 8, 9)
        for q, (off, par) in enumerate(quad):
            cases.append((n, ncols[(k + 3 * q) % len(ncols)], _pad_for(n, par, (k + q) & 1), off))
    mid = (2049, 20014, 20015, 1025, 2048, 255, 1024, 3)
    for k, c in enumerate(CGS_NCOL):  # every ncol
        for q, (off, par) in enumerate(quad):
            n = mid[(k + q) % len(mid)]
            cases.append((n, c, _pad_for(n, par, (k + q + 1) & 1), off))
    for pad in CGS_PAD:  # every pad: n even and odd give both parities
        for n in (2047, 2048):
            for off in (0, 1):
                cases.append((n, 9, pad, off))
    out, seen = [], set()
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out
