"""Plain numpy reference of the GP gradient, MLL-term and posterior-finalize device entry points
(evr_kernel_cross_grad, evr_kernel_lengthscale_grad, evr_gp_mll_terms, evr_gp_posterior_finalize),
written from the formulas alone: explicit differences (no quadratic expansion), one output at a
time, the normalised inputs in float64 and from there every element and every sum in
``np.longdouble`` (x87 extended where the platform has it,
plain double otherwise).  It imports nothing of everest_amd and knows nothing of the kernels'
tiling or summation order.

    u       = (x - shift) * scale             absent shift / scale: identity
    diff_k  = (u2_k - u1_k) / ls_bk
    d2      = sum_k diff_k^2
    dscale  = RBF -exp(-d2/2); Matern: 0 where d2 < 1e-30 (GPyTorch's clamp_min kills the
              gradient there), nu = 1/2: -exp(-r)/r, 3/2: -3 exp(-sqrt3 r),
              5/2: -(5/3)(1 + sqrt5 r) exp(-sqrt5 r), r = sqrt(d2)

Every function returns, next to its result, the sum of the absolute values of the same terms:
the scale an error bar is taken against, so that cancellation cannot hide behind it.

The module also holds the inputs of the MLL-chain tests (``mll_case``): the CPU test asserts
their conditioning, the GPU test evaluates them.
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
RBF, MATERN05, MATERN15, MATERN25 = 0, 1, 2, 3


def _ld(a):
    return None if a is None else np.asarray(a, dtype=LD)


def normalise(X, shift=None, scale=None):
    """u = (x - shift) * scale in float64, the inputs' own format (a float64 subtraction and a
    float64 product, as the oracle's Normalize does): rows that normalise to the same float64
    point are at distance exactly zero.  Everything after it is long double."""
    u = np.asarray(X, dtype=np.float64)
    if shift is not None:
        u = u - np.asarray(shift, dtype=np.float64)
    if scale is not None:
        u = u * np.asarray(scale, dtype=np.float64)
    return _ld(u)


def dscale(kind: int, d2):
    """(dk/dd2) * 2 of the family: dk/du2_k = dscale * diff_k / ls_k."""
    d2 = _ld(d2)
    if kind == RBF:
        return -np.exp(-d2 / 2)
    dead = d2 < LD(1e-30)
    r = np.sqrt(np.where(dead, LD(1), d2))
    if kind == MATERN05:
        v = -np.exp(-r) / r
    elif kind == MATERN15:
        s3 = np.sqrt(LD(3))
        v = -3 * np.exp(-s3 * r)
    elif kind == MATERN25:
        s5 = np.sqrt(LD(5))
        v = -(LD(5) / 3) * (1 + s5 * r) * np.exp(-s5 * r)
    else:
        raise ValueError(f"kernel kind {kind}")
    return np.where(dead, LD(0), v)


def _kinds(kinds, B):
    if np.isscalar(kinds):
        return [int(kinds)] * B
    kinds = [int(k) for k in kinds]
    if len(kinds) != B:
        raise ValueError(f"{len(kinds)} kinds for {B} outputs")
    return kinds


def cross_grad(X1, X2, ls, G, kinds, shift1=None, scale1=None, shift2=None, scale2=None, outputscale=None,
               row_chunk: int = 64):
    """dX2[c,k] = scale2_k sum_b sum_i G[b,i,c] os_b dscale_b(d2) diff_k / ls_bk and S[c,k], the
    sum of the absolute values of the same terms.  X1 n1 x d, X2 n2 x d, ls B x d, G B x n1 x n2."""
    u1, u2 = normalise(X1, shift1, scale1), normalise(X2, shift2, scale2)
    ls, G = _ld(ls), _ld(G)
    B, d = ls.shape
    n1, n2 = u1.shape[0], u2.shape[0]
    kinds = _kinds(kinds, B)
    os_ = np.ones(B, dtype=LD) if outputscale is None else _ld(outputscale)
    out = np.zeros((n2, d), dtype=LD)
    S = np.zeros((n2, d), dtype=LD)
    for b in range(B):
        for i0 in range(0, n1, row_chunk):
            diff = (u2[None, :, :] - u1[i0:i0 + row_chunk, None, :]) / ls[b]          # rows x n2 x d
            d2 = (diff * diff).sum(-1)
            w = G[b, i0:i0 + row_chunk] * os_[b] * dscale(kinds[b], d2)             # rows x n2
            term = w[:, :, None] * diff / ls[b]
            out += term.sum(0)
            S += np.abs(term).sum(0)
    if scale2 is not None:
        sc = _ld(scale2)
        out, S = out * sc, S * np.abs(sc)
    return out, S


def lengthscale_grad(X, ls, W, kinds, row_chunk: int = 32):
    """g[b,k] = sum_i sum_j W[b,i,j] (-dscale_b(d2) diff_k^2 / ls_bk) and S[b,k].  W is taken as
    given (not symmetrised)."""
    u, ls, W = _ld(X), _ld(ls), _ld(W)
    B, d = ls.shape
    n = u.shape[0]
    kinds = _kinds(kinds, B)
    g = np.zeros((B, d), dtype=LD)
    S = np.zeros((B, d), dtype=LD)
    for b in range(B):
        for i0 in range(0, n, row_chunk):
            diff = (u[None, :, :] - u[i0:i0 + row_chunk, None, :]) / ls[b]            # rows x n x d
            sq = diff * diff
            w = -W[b, i0:i0 + row_chunk] * dscale(kinds[b], sq.sum(-1))             # rows x n
            term = w[:, :, None] * sq / ls[b]
            g[b] += term.sum((0, 1))
            S[b] += np.abs(term).sum((0, 1))
    return g, S


def mll_terms(L, Linv, r, alpha):
    """[2 sum log L_ii, r.alpha, ||Linv||_F^2, sum alpha, sum alpha^2] per output (B x 5) and
    the matching absolute sums."""
    L, Linv, r, alpha = _ld(L), _ld(Linv), _ld(r), _ld(alpha)
    lg = np.log(np.diagonal(L, axis1=-2, axis2=-1))
    sq = (Linv * Linv).sum((-2, -1))
    a2 = (alpha * alpha).sum(-1)
    out = np.stack([2 * lg.sum(-1), (r * alpha).sum(-1), sq, alpha.sum(-1), a2], -1)
    S = np.stack([2 * np.abs(lg).sum(-1), np.abs(r * alpha).sum(-1), sq, np.abs(alpha).sum(-1), a2], -1)
    return out, S


def posterior_finalize(R, c, ym, ys, kxx, noise=None):
    """R: B x (n + 1) x nt (rows 0..n-1: L^-1 K_*, row n: alpha^T K_*).  Returns
    mean = ym + ys (c + R[n]), var = ys^2 (kxx - sum_{i<n} R[i]^2 [+ noise]), and sum_{i<n} R[i]^2."""
    R, c, ym, ys, kxx = _ld(R), _ld(c), _ld(ym), _ld(ys), _ld(kxx)
    ss = (R[:, :-1] * R[:, :-1]).sum(1)                                               # B x nt
    mean = ym[:, None] + ys[:, None] * (c[:, None] + R[:, -1])
    v = kxx[:, None] - ss
    if noise is not None:
        v = v + _ld(noise)[:, None]
    return mean, ys[:, None] ** 2 * v, ss


# ---------------------------------------------------------------------------------------
# inputs of the MLL-chain tests
# ---------------------------------------------------------------------------------------
NOISES = (1e-2, 5e-2, 0.2)
CONSTANTS = (0.0, 0.1, -0.2)
# (n, d, kinds) of the op-by-op chain, of the plan (B = 3), and the many-output plan case
MLL_CHAIN_CASES = [(97, 1, (0, 3)), (97, 8, (0, 1, 2, 3)), (97, 9, (0, 3)), (129, 16, (0, 3)),
                   (129, 17, (0, 1, 2, 3)), (129, 33, (0, 3)), (65, 64, (0, 3))]
MLL_PLAN_CASES = [(97, 8), (129, 17), (64, 16), (33, 33)]
MLL_PLAN_KINDS = (0, 1, 2, 3)
MLL_MANY = (8, 1, 52)          # n, d, B (RBF)


def inv_softplus(y):
    y = np.asarray(y, dtype=np.float64)
    return y + np.log(-np.expm1(-y))


def mll_case(n: int, d: int, B: int):
    """X (n x d, unit cube), Ys (B x n: a smooth function of X plus 0.05 noise, standardised with
    the unbiased std) and the raw parameter vectors xs (B x (d + 2): noise, constant, raw
    lengthscales with softplus(raw) uniform in [0.3 sqrt d, 1.2 sqrt d])."""
    rng = np.random.default_rng(1000 * n + 10 * d + B)
    X = rng.uniform(size=(n, d))
    Ys = np.empty((B, n))
    xs = np.empty((B, d + 2))
    for b in range(B):
        w = rng.normal(size=d) / math.sqrt(d)
        y = np.sin(3.0 * (X @ w) + 0.7 * b) + ((X - 0.5) ** 2).mean(1) + 0.05 * rng.normal(size=n)
        Ys[b] = (y - y.mean()) / y.std(ddof=1)
        ls = rng.uniform(0.3, 1.2, d) * math.sqrt(d)
        xs[b] = np.r_[NOISES[b % 3], CONSTANTS[b % 3], inv_softplus(ls)]
    return X, Ys, xs


def kernel_value(kind: int, d2):
    """k(d2) of the family in float64 (GPyTorch's forms; Matern distance clamped at 1e-30)."""
    d2 = np.asarray(d2, dtype=np.float64)
    if kind == RBF:
        return np.exp(-0.5 * d2)
    r = np.sqrt(np.maximum(d2, 1e-30))
    if kind == MATERN05:
        return np.exp(-r)
    if kind == MATERN15:
        return (1 + math.sqrt(3) * r) * np.exp(-math.sqrt(3) * r)
    return (1 + math.sqrt(5) * r + 5.0 / 3.0 * d2) * np.exp(-math.sqrt(5) * r)


def train_matrix(X, ls, noise, kind):
    """K + noise I in float64 by explicit differences."""
    diff = (X[:, None, :] - X[None, :, :]) / ls
    return kernel_value(kind, (diff * diff).sum(-1)) + noise * np.eye(X.shape[0])
