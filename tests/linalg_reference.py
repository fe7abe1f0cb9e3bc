"""Plain long-double reference of the dense float64 primitives (Cholesky, triangular solve,
triangular inverse, GEMM) and the inputs of their tests.  Inputs are taken as the exact float64
values they hold; every product and every sum is ``np.longdouble`` (x87 extended: 64
significand bits).  It imports nothing of everest_amd and knows nothing of the kernels' tiling,
blocking or summation order.

Every checker returns a ``Check(ratio, err, scale)``: the largest componentwise ratio of the
error to the scale it is judged against (the sum of the absolute values of the same terms, so
that a small element cannot hide behind a large one), and the absolute error and the scale at
the element where that ratio is attained.  Where the scale is zero the error must be exactly
zero (the ratio is 0 then, ``inf`` otherwise); a NaN in the checked result gives a NaN ratio,
which fails every ``<=``.

The bars of the tests, with u = 2^-53 and gamma(k) = k u / (1 - k u), are first-order bounds of
Higham, *Accuracy and Stability of Numerical Algorithms* (2nd ed.), valid for any summation
order:

    Cholesky            chol_residual  <= gamma(n + 1)     Thm 10.3
    triangular solve    trsm_residual  <= gamma(n)         Thm 8.5
    triangular inverse  tri_inv_error  <= n u              sec. 14.2-14.3 (forward bound)
    GEMM                gemm_error     <= gamma(K + 3)     K products, alpha, beta, the add

The module also holds the seeded input builders (``spectrum``, ``rbf_clustered``, ``graded``) and
the case lists shared by the CPU test (which asserts that LAPACK stays under a quarter of each
bar on them) and the GPU test (which evaluates the device on them).
"""
from __future__ import annotations

import collections
import functools

import numpy as np
import torch

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise RuntimeError(f"linalg_reference needs an extended long double (>= 63 mantissa bits); this platform's "
                       f"np.longdouble has {np.finfo(LD).nmant}: the reference would be no more precise than "
                       "the float64 results it judges")

U = LD(2) ** -53

Check = collections.namedtuple("Check", "ratio err scale")


def gamma(k: int):
    return k * U / (1 - k * U)


def _ld(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=LD)


def _check(err, scale) -> Check:
    """Largest err / scale over the elements (err, scale >= 0, same shape)."""
    err, scale = np.asarray(err, dtype=LD), np.asarray(scale, dtype=LD)
    if err.size == 0:
        return Check(LD(0), LD(0), LD(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, err / np.where(scale > 0, scale, LD(1)), np.where(err == 0, LD(0), LD(np.inf)))
    ratio = np.where(np.isnan(err) | np.isnan(scale), LD(np.nan), ratio)
    if np.isnan(ratio).any():
        at = int(np.argmax(np.isnan(ratio)))
    else:
        at = int(np.argmax(ratio))
    return Check(ratio.flat[at], err.flat[at], scale.flat[at])


_BS = 128


def _tril_product(A, B):
    """A @ B for lower-triangular A, B by blocks (only the blocks that are not zero)."""
    n = A.shape[0]
    C = np.zeros((n, n), dtype=LD)
    for i0 in range(0, n, _BS):
        i1 = min(n, i0 + _BS)
        for j0 in range(0, i1, _BS):
            j1 = min(n, j0 + _BS)
            C[i0:i1, j0:j1] = A[i0:i1, j0:i1] @ B[j0:i1, j0:j1]
    return np.tril(C)


def _gram_lower(L, rows=None):
    """(L L^T)[rows] for a lower-triangular L; without rows, the lower triangle by blocks."""
    if rows is not None:
        return L[rows] @ L.T
    n = L.shape[0]
    C = np.zeros((n, n), dtype=LD)
    for i0 in range(0, n, _BS):
        i1 = min(n, i0 + _BS)
        for j0 in range(0, i1, _BS):
            j1 = min(n, j0 + _BS)
            C[i0:i1, j0:j1] = L[i0:i1, :j1] @ L[j0:j1, :j1].T
    return C


def symmetrise_lower(A):
    """The symmetric matrix whose lower triangle is A's (the strict upper triangle is not read)."""
    lo = np.tril(_ld(A))
    return lo + np.tril(lo, -1).T


def chol_residual(A_lower, L, rows=None) -> Check:
    """max_ij |(L L^T - A)_ij| / (|L| |L^T|)_ij, A symmetrised from its lower triangle, L taken
    as given (a non-zero upper triangle enters the product).  rows: check these rows only."""
    A, L = symmetrise_lower(A_lower), _ld(L)
    if rows is None:
        if not np.all(np.triu(L, 1) == 0):   # not lower triangular (or NaN above): the full product
            return _check(np.abs(L @ L.T - A), np.abs(L) @ np.abs(L).T)
        m = np.tril(np.ones(A.shape, dtype=bool))   # symmetric: the lower triangle is every element
        return _check(np.abs(_gram_lower(L) - A)[m], _gram_lower(np.abs(L))[m])
    rows = np.asarray(rows, dtype=np.int64)
    return _check(np.abs(_gram_lower(L, rows) - A[rows]), _gram_lower(np.abs(L), rows))


def trsm_residual(L, X, B, transpose: bool) -> Check:
    """max |op(L) X - B| / (|op(L)| |X|), op(L) = L^T if transpose (L's lower triangle)."""
    T, X, B = np.tril(_ld(L)), _ld(X), _ld(B)
    if transpose:
        T = T.T
    return _check(np.abs(T @ X - B), np.abs(T) @ np.abs(X))


def tri_inv_ld(L):
    """L^-1 of the lower triangle of L by row-wise forward substitution in long double:
    X[i, :i+1] = (e_i - L[i, :i] X[:i, :i+1]) / L[i, i]."""
    T = np.tril(_ld(L))
    n = T.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        row = -(T[i, :i] @ X[:i, :i + 1]) if i else np.zeros(1, dtype=LD)
        row[i] += 1
        X[i, :i + 1] = row / T[i, i]
    return X


def tri_inv_scale(L, Xr):
    """|Xr| |L| |Xr|, the scale of the forward bound of a triangular inverse."""
    aX = np.abs(Xr)
    return _tril_product(_tril_product(aX, np.abs(np.tril(_ld(L)))), aX)


def tri_inv_error(L, X, ref=None):
    """(Check of max |X - Xr| / (|Xr| |L| |Xr|) over the lower triangle, whether triu(X, 1) is
    exactly zero), Xr = tri_inv_ld(L).  ref: a precomputed (Xr, scale) pair of this L."""
    X = _ld(X)
    Xr, S = ref if ref is not None else tri_inv_reference(L)
    m = np.tril(np.ones(X.shape, dtype=bool))
    upper_zero = bool(np.all(X[~m] == 0))
    return _check(np.abs(X - Xr)[m], S[m]), upper_zero


def tri_inv_reference(L):
    Xr = tri_inv_ld(L)
    return Xr, tri_inv_scale(L, Xr)


def gemm_reference(alpha, opA, opB, beta, C0):
    """(alpha opA opB + beta C0, |alpha| |opA| |opB| + |beta| |C0|); C0 does not enter when
    beta == 0 (it may hold NaN)."""
    a, b = _ld(opA), _ld(opB)
    al, be = LD(alpha), LD(beta)
    R, S = al * (a @ b), np.abs(al) * (np.abs(a) @ np.abs(b))
    if beta != 0:
        c0 = _ld(C0)
        R, S = R + be * c0, S + np.abs(be) * np.abs(c0)
    return R, S


def gemm_error(alpha, opA, opB, beta, C0, C) -> Check:
    """max |C - (alpha opA opB + beta C0)| / (|alpha| |opA| |opB| + |beta| |C0|)."""
    R, S = gemm_reference(alpha, opA, opB, beta, C0)
    return _check(np.abs(_ld(C) - R), S)


# ---------------------------------------------------------------------------------------
# input builders (seeded, float64 tensors)
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spectrum(n: int, k: float, seed: int):
    rng = np.random.default_rng([n, int(k), seed, 1])
    j = np.arange(n, dtype=LD)
    C = np.cos(LD(np.pi) * (j[:, None] + LD(0.5)) * j[None, :] / n) * np.sqrt(LD(2) / n)   # DCT-II
    C[:, 0] /= np.sqrt(LD(2))
    Q = C[rng.permutation(n)] * rng.choice([-1.0, 1.0], size=n).astype(LD)[:, None]
    d = np.logspace(0, -k, n)[rng.permutation(n)].astype(LD)
    A = ((Q * d) @ Q.T).astype(np.float64)
    return 0.5 * (A + A.T)


def spectrum(n: int, k: float, seed: int = 0) -> torch.Tensor:
    """Q diag(logspace(0, -k, n)) Q^T, symmetrised: condition 10^k.  Q is an orthogonal cosine
    transform with seeded row order and signs (the eigenvalues in seeded order), and the product
    is formed in long double and rounded once, so that every platform builds the same float64
    matrix (a LAPACK QR and a BLAS product differ in the last bits from one CPU to the next,
    which is enough to move a ratio measured on an ill-conditioned input)."""
    return torch.from_numpy(_spectrum(n, k, seed).copy())


def rbf_clustered(n: int, noise: float, seed: int = 0) -> torch.Tensor:
    """RBF kernel matrix (lengthscale 0.3) of 2-D points, three quarters uniform on the unit
    square and one quarter uniform in [0.4, 0.41]^2 (near-duplicate rows), plus noise I."""
    rng = np.random.default_rng([n, seed, 2])
    nc = n // 4
    P = np.concatenate([rng.uniform(size=(n - nc, 2)), rng.uniform(0.4, 0.41, size=(nc, 2))])
    P = P[rng.permutation(n)]
    # the kernel in long double, rounded once: the same float64 matrix whatever exp the
    # platform's numpy dispatches to
    P = P.astype(LD)
    d2 = sum(((P[:, None, k] - P[None, :, k]) / LD(0.3)) ** 2 for k in range(2))
    return torch.from_numpy(np.exp(-d2 / 2).astype(np.float64) + noise * np.eye(n))


def graded(n: int, seed: int = 0) -> torch.Tensor:
    """D spectrum(n, 6) D with D = diag(10^+-6) in shuffled order: entries over 24 decades."""
    rng = np.random.default_rng([n, seed, 3])
    d = 10.0 ** np.where(rng.permutation(n) % 2 == 0, 6.0, -6.0)
    A = spectrum(n, 6, seed).numpy() * d[:, None] * d[None, :]
    return torch.from_numpy(0.5 * (A + A.T))


# ---------------------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------------------
CHOL_SMALL_N = (1, 2, 3, 15, 16, 17, 63, 64, 65, 129, 193)
CHOL_MID_N = (512, 513)
CHOL_BIG_N = 1025
CHOL_CLASSES = {"small": ("spectrum8", "rbf1e-6", "graded"), "mid": ("spectrum10", "rbf1e-4"), "big": ("rbf1e-4",)}


# With n <= 3 the whole factorisation makes a handful of roundings, and one correctly rounded
# operation already takes a large share of the bound: a_11 = 1 + 1e-6 of rbf_clustered has
# fl(sqrt(a_11)) at 0.90 gamma(2), graded(1) = 1e12 has the exact root 1e6 whose correctly rounded
# reciprocal is 0.41 u off, and which way the few roundings of a 2 x 2 or 3 x 3 factor fall
# depends on the last bit of the input.  No float64 algorithm can promise a quarter of the bar
# there, so the CPU test holds LAPACK to the bar itself for n <= 3 and to the quarter from n = 15 on.
QUARTER_FROM_N = 15


def chol_inputs(n: int) -> torch.Tensor:
    """The batch of test (a) at size n (the classes' names: chol_classes(n))."""
    if n == CHOL_BIG_N:
        return torch.stack([rbf_clustered(n, 1e-4)])
    if n in CHOL_MID_N:
        return torch.stack([spectrum(n, 10), rbf_clustered(n, 1e-4)])
    return torch.stack([spectrum(n, 8), rbf_clustered(n, 1e-6), graded(n)])


def chol_classes(n: int):
    return CHOL_CLASSES["big" if n == CHOL_BIG_N else "mid" if n in CHOL_MID_N else "small"]


def residual_rows(n: int, count: int = 96):
    """First and last row of every 64-block, filled up to count with seeded random rows."""
    rows = sorted({r for b in range(0, n, 64) for r in (b, min(n, b + 64) - 1)})
    rng = np.random.default_rng(n)
    rest = [int(r) for r in rng.permutation(n) if int(r) not in set(rows)]
    return np.array(sorted(rows + rest[:max(0, count - len(rows))]), dtype=np.int64)


# (d): (n, nrhs) without and with the transpose
TRSM_N_CASES = [(1, 1), (15, 17), (16, 16), (17, 15), (63, 65), (64, 1), (64, 16), (65, 17), (65, 65), (511, 15),
                (512, 1), (512, 17), (513, 16), (513, 65)]
TRSM_T_CASES = [(1, 1), (63, 17), (64, 64), (65, 65), (513, 130)]


def trsm_inputs(n: int, nrhs: int):
    """L (2 x n x n: the LAPACK factors of spectrum(n, 8) and graded(n)) and B (2 x n x nrhs,
    standard normal with the columns scaled by logspace(-8, 8, nrhs))."""
    L = torch.linalg.cholesky(torch.stack([spectrum(n, 8), graded(n)]))
    g = torch.Generator().manual_seed(1000 * n + nrhs)
    B = torch.randn(2, n, nrhs, generator=g, dtype=torch.float64) * torch.logspace(-8, 8, nrhs, dtype=torch.float64)
    return L, B


def well_conditioned(n: int, seed: int = 0) -> torch.Tensor:
    """G G^T / n + I."""
    g = torch.Generator().manual_seed(7 * n + seed)
    G = torch.randn(n, n, generator=g, dtype=torch.float64)
    return G @ G.T / n + torch.eye(n, dtype=torch.float64)


def gemm_operands(M: int, N: int, K: int, batch: int, ta: bool, tb: bool, seed: int = 0, batch_a=None, batch_b=None):
    """A, B, C0 as stored (A batch x K x M if ta, B batch x N x K if tb), standard normal with
    the rows of op(A) and the columns of op(B) scaled by 10^U(-6, 6).  batch_a / batch_b = 1: a
    broadcast operand."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + 101 * seed + 2 * int(ta) + int(tb))
    ba, bb = batch if batch_a is None else batch_a, batch if batch_b is None else batch_b
    A = torch.randn(ba, M, K, generator=g, dtype=torch.float64)
    B = torch.randn(bb, K, N, generator=g, dtype=torch.float64)
    A = A * 10.0 ** (12.0 * torch.rand(ba, M, 1, generator=g, dtype=torch.float64) - 6.0)
    B = B * 10.0 ** (12.0 * torch.rand(bb, 1, N, generator=g, dtype=torch.float64) - 6.0)
    C0 = torch.randn(batch, M, N, generator=g, dtype=torch.float64)
    if K == 1:
        # outer product: operands rounded to 24 bits, so that a b is exact and the add of
        # a b + c is the only rounding a correct algorithm makes (the two roundings of an
        # inexact product and the add would take half of gamma(4) on their own)
        A, B = A.float().double(), B.float().double()
    if ta:
        A = A.transpose(1, 2).contiguous()
    if tb:
        B = B.transpose(1, 2).contiguous()
    return A, B, C0


TRANSPOSE_PAIRS = [(False, False), (True, False), (False, True), (True, True)]
GEMM_SPLIT_K = (255, 256, 257, 1152, 1153, 4096, 4097)
GEMM_PARITY = [(33, 64, 64), (64, 33, 64), (64, 64, 33)]
GEMM_STRIDED = [(33, 65, 257), (64, 64, 64)]
# every (M, N, K, batch, transA, transB, alpha, beta) of the GPU GEMM tests (the CPU test runs torch's
# matmul on them)
_AB = (1.5, -0.5)
GEMM_SHAPES = ([(512, 1, 512, 5, ta, False) + _AB for ta in (False, True)]
               + [(130, 130, 1, 1, False, True, 1.0, 0.0), (513, 513, 1, 1, False, True, 1.0, 1.0)]
               + [(32, 32, K, 1, ta, False) + _AB for K in GEMM_SPLIT_K for ta in (False, True)]
               + [(64, 64, K, 1, False, True) + _AB for K in GEMM_SPLIT_K]
               + [(70, 33, 40, 1, False, False, 1.5, 0.0), (32, 32, 1152, 1, False, False, 1.5, 0.0),
                  (32, 32, 1152, 1, False, True, 1.5, 0.0)]
               + [(M, N, K, 1, ta, tb) + _AB for M, N, K in GEMM_PARITY + GEMM_STRIDED for ta, tb in TRANSPOSE_PAIRS])


def op(X: torch.Tensor, t: bool) -> torch.Tensor:
    return X.transpose(-1, -2) if t else X
