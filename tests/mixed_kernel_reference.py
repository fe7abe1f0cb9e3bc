"""Plain numpy reference of the mixed continuous / categorical kernel entry points
(evr_mixed_kernel_matrix, evr_mixed_kernel_param_grad), written from the formulas alone: explicit
differences, one member at a time, the inputs in float64 and from there every element and every
sum in ``np.longdouble`` (x87 extended where the platform has it, plain double otherwise).  It
imports nothing of everest_amd and knows nothing of the kernels' tiling or summation order.

    K(x, x') = s_sum (k_c(r1) + s_cat h1) + s_prod k_c(r2) h2
    r_t^2 = sum_k ((xc_k - xc'_k) / ls_t,k)^2                         t = 1, 2
    h_t   = exp(-(1 / nc) sum_f [c_f != c'_f] / lam_t,f)
    params = [ls1 (dc) | ls2 (dc) | lam1 (nc) | lam2 (nc) | s_sum | s_cat | s_prod]      P = 2 dc + 2 nc + 3

k_c: RBF exp(-r^2 / 2) or Matern 1/2, 3/2, 5/2 in r = sqrt(max(r^2, 1e-30)); its lengthscale
derivative is -dscale(r^2) diff_k^2 / ls_k with gp_kernel_reference.dscale (zero where
r^2 < 1e-30: GPyTorch's clamp_min kills the gradient there).

``param_grad`` returns, next to each sum, the sum of the absolute values of the same terms: the
scale an error bar is taken against, so that cancellation cannot hide behind it.

The module also holds the inputs of the mixed-GP tests (``kernel_case``, ``mll_case``,
``posterior_case``, ``fit_case``): the CPU test asserts their conditioning, the GPU tests evaluate them.
"""
from __future__ import annotations

import math

import numpy as np

from tests.gp_kernel_reference import LD, MATERN05, MATERN15, MATERN25, RBF, dscale, inv_softplus

__all__ = ["LD", "RBF", "MATERN05", "MATERN15", "MATERN25", "n_params", "split_params", "kvalue", "kernel_matrix",
           "param_grad", "kxx", "kernel_case", "mll_case", "posterior_case", "fit_case"]


def n_params(dc: int, nc: int) -> int:
    return 2 * dc + 2 * nc + 3


def split_params(p, dc: int, nc: int):
    """(ls1, ls2, lam1, lam2, s_sum, s_cat, s_prod) of one member's parameter vector."""
    if p.shape[-1] != n_params(dc, nc):
        raise ValueError(f"{p.shape[-1]} parameters for dc = {dc}, nc = {nc}")
    return (p[:dc], p[dc:2 * dc], p[2 * dc:2 * dc + nc], p[2 * dc + nc:2 * dc + 2 * nc], p[-3], p[-2], p[-1])


def kxx(params):
    """k(x, x) = s_sum (1 + s_cat) + s_prod per member."""
    p = np.atleast_2d(np.asarray(params, dtype=np.float64))
    return p[:, -3] * (1.0 + p[:, -2]) + p[:, -1]


def kvalue(kind: int, d2):
    """k_c(r^2) of the family in long double (Matern distance clamped at 1e-30)."""
    d2 = np.asarray(d2, dtype=LD)
    if kind == RBF:
        return np.exp(-d2 / 2)
    r = np.sqrt(np.maximum(d2, LD(1e-30)))
    if kind == MATERN05:
        return np.exp(-r)
    if kind == MATERN15:
        s3 = np.sqrt(LD(3))
        return (1 + s3 * r) * np.exp(-s3 * r)
    if kind == MATERN25:
        s5 = np.sqrt(LD(5))
        return (1 + s5 * r + LD(5) / 3 * d2) * np.exp(-s5 * r)
    raise ValueError(f"kernel kind {kind}")


def _pieces(u1, c1, u2, c2, ls, lam):
    """Scaled squared differences (n1 x n2 x dc), r^2, the mismatch indicators (n1 x n2 x nc) and h."""
    diff = (u1[:, None, :] - u2[None, :, :]) / ls
    sq = diff * diff
    ne = (c1[:, None, :] != c2[None, :, :]).astype(LD)
    h = np.exp(-(ne / lam).sum(-1) / LD(c1.shape[1]))
    return sq, sq.sum(-1), ne, h


def kernel_matrix(Xc1, C1, Xc2, C2, params, kind: int, row_chunk: int = 64):
    """K (B x n1 x n2, long double).  params: B x P."""
    u1, u2 = np.asarray(Xc1, dtype=np.float64).astype(LD), np.asarray(Xc2, dtype=np.float64).astype(LD)
    c1, c2 = np.asarray(C1), np.asarray(C2)
    params = np.atleast_2d(np.asarray(params, dtype=np.float64)).astype(LD)
    dc, nc = u1.shape[1], c1.shape[1]
    K = np.empty((params.shape[0], u1.shape[0], u2.shape[0]), dtype=LD)
    for b, p in enumerate(params):
        ls1, ls2, lam1, lam2, s_sum, s_cat, s_prod = split_params(p, dc, nc)
        for i0 in range(0, u1.shape[0], row_chunk):
            sl = slice(i0, i0 + row_chunk)
            _, d21, _, h1 = _pieces(u1[sl], c1[sl], u2, c2, ls1, lam1)
            _, d22, _, h2 = _pieces(u1[sl], c1[sl], u2, c2, ls2, lam2)
            K[b, sl] = s_sum * (kvalue(kind, d21) + s_cat * h1) + s_prod * kvalue(kind, d22) * h2
    return K


def param_grad(Xc, C, params, W, kind: int, row_chunk: int = 32):
    """g[b, p] = sum_ij W[b, i, j] dK_b[i, j] / dparams_p and S[b, p], the sum of the absolute values
    of the same terms (B x P each, long double).  W (B x n x n) is taken as given (not symmetrised)."""
    u, c = np.asarray(Xc, dtype=np.float64).astype(LD), np.asarray(C)
    params = np.atleast_2d(np.asarray(params, dtype=np.float64)).astype(LD)
    W = np.asarray(W, dtype=np.float64).astype(LD)
    n, dc = u.shape
    nc = c.shape[1]
    B, P = params.shape
    g, S = np.zeros((B, P), dtype=LD), np.zeros((B, P), dtype=LD)

    def add(b, p0, term):      # term: rows x n (one parameter) or rows x n x m (m consecutive ones)
        term = term.reshape(term.shape[0], term.shape[1], -1)
        g[b, p0:p0 + term.shape[2]] += term.sum((0, 1))
        S[b, p0:p0 + term.shape[2]] += np.abs(term).sum((0, 1))

    for b, p in enumerate(params):
        ls1, ls2, lam1, lam2, s_sum, s_cat, s_prod = split_params(p, dc, nc)
        for i0 in range(0, n, row_chunk):
            sl = slice(i0, i0 + row_chunk)
            w = W[b, sl]
            sq1, d21, ne, h1 = _pieces(u[sl], c[sl], u, c, ls1, lam1)
            sq2, d22, _, h2 = _pieces(u[sl], c[sl], u, c, ls2, lam2)
            k1, k2 = kvalue(kind, d21), kvalue(kind, d22)
            add(b, 0, (w * s_sum * -dscale(kind, d21))[:, :, None] * sq1 / ls1)
            add(b, dc, (w * s_prod * h2 * -dscale(kind, d22))[:, :, None] * sq2 / ls2)
            add(b, 2 * dc, (w * s_sum * s_cat * h1)[:, :, None] * ne / (nc * lam1 * lam1))
            add(b, 2 * dc + nc, (w * s_prod * k2 * h2)[:, :, None] * ne / (nc * lam2 * lam2))
            add(b, P - 3, w * (k1 + s_cat * h1))
            add(b, P - 2, w * s_sum * h1)
            add(b, P - 1, w * k2 * h2)
    return g, S


# ---------------------------------------------------------------------------------------
# inputs of the tests
# ---------------------------------------------------------------------------------------
NOISES = (1e-2, 5e-2, 0.2)
CONSTANTS = (0.1, -0.2, 0.3)
FAMILIES = (RBF, MATERN05, MATERN15, MATERN25)


def cardinalities(nc: int):
    """2, 3, 4, 5, 2, ... levels per categorical feature."""
    return np.array([2 + f % 4 for f in range(nc)])


def _points(rng, n, dc, nc):
    return rng.uniform(size=(n, dc)), rng.integers(0, cardinalities(nc), size=(n, nc)).astype(np.int32)


def _params(rng, B, dc, nc):
    """B parameter vectors: lengthscales in [0.3 sqrt dc, 1.2 sqrt dc], lam in [0.3, 2], scales in [0.5, 2]."""
    return np.concatenate([rng.uniform(0.3, 1.2, (B, 2 * dc)) * math.sqrt(dc), rng.uniform(0.3, 2.0, (B, 2 * nc)),
                           rng.uniform(0.5, 2.0, (B, 3))], axis=1)


def kernel_case(n1: int, n2: int, dc: int, nc: int, B: int):
    """(Xc1, C1, Xc2, C2, params): points in the unit cube with 2..5 levels per categorical feature.
    Row 0 of the second set is row 0 of the first (zero distance, equal in every category); from
    two rows on, row 1 of the second set is row 0 of the first with every category changed, and row
    1 of the first set is its row 0 again with every category kept (a duplicated row: zero distance
    off the diagonal of K(X1, X1)), and from three rows on its row 2 is row 0 with every category
    changed."""
    rng = np.random.default_rng(100000 * n1 + 1000 * n2 + 10 * dc + nc)
    Xc1, C1 = _points(rng, n1, dc, nc)
    Xc2, C2 = _points(rng, n2, dc, nc)
    if n1 > 1:
        Xc1[1], C1[1] = Xc1[0], C1[0]
    if n1 > 2:      # and once more with every category changed
        Xc1[2], C1[2] = Xc1[0], (C1[0] + 1) % cardinalities(nc)
    Xc2[0], C2[0] = Xc1[0], C1[0]
    if n2 > 1:
        Xc2[1], C2[1] = Xc1[0], (C1[0] + 1) % cardinalities(nc)
    return Xc1, C1, Xc2, C2, _params(rng, B, dc, nc)


def mll_case(n: int, dc: int, nc: int, member: int = 0):
    """Inputs of the MLL tests: Xc (n x dc), C (n x nc), y (a smooth function of Xc plus per-category
    offsets plus 0.05 noise, standardised with the unbiased std), the parameter vector p (P), the
    noise and the constant (nonzero, cycling with ``member``)."""
    rng = np.random.default_rng(1000 * n + 10 * dc + nc)
    Xc, C = _points(rng, n, dc, nc)
    w = rng.normal(size=dc) / math.sqrt(dc)
    off = rng.normal(size=(nc, 5))
    y = np.sin(3.0 * (Xc @ w)) + ((Xc - 0.5) ** 2).mean(1) + off[np.arange(nc), C].sum(1) + 0.05 * rng.normal(size=n)
    y = (y - y.mean()) / y.std(ddof=1)
    return Xc, C, y, _params(rng, 1, dc, nc)[0], NOISES[member % 3], CONSTANTS[member % 3]


MLL_CASES = [(n, dc, nc) for n in (31, 80) for dc in (2, 9) for nc in (1, 3)]
MIN_LAM = 1e-6


def raw_of(p, dc: int, nc: int, noise: float, constant: float, ard: bool = True):
    """The optimiser's vector [noise, constant, raw ls1, raw ls2, raw lam1, raw lam2, raw scales] whose
    transformed values (softplus; lam = 1e-6 + softplus) are p.  ard=False: one raw lengthscale per
    continuous kernel, the first of p's."""
    p = np.asarray(p, dtype=np.float64)
    ls = p[:2 * dc].reshape(2, dc)
    ls = ls if ard else ls[:, :1]
    return np.concatenate([[noise, constant], inv_softplus(ls.reshape(-1)),
                           inv_softplus(p[2 * dc:2 * dc + 2 * nc] - MIN_LAM), inv_softplus(p[-3:])])


def posterior_case():
    """The posterior test's inputs: the n = 80, dc = 9, nc = 3 MLL case as the fitted model (raw
    targets with mean 1.5 and std 2.5), and 50 test points of which rows 0..3 are training rows
    7, 19, 40 and 79."""
    Xc, C, y, p, noise, const = mll_case(80, 9, 3)
    rng = np.random.default_rng(5)
    Xt, Ct = _points(rng, 50, 9, 3)
    rows = [7, 19, 40, 79]
    Xt[:4], Ct[:4] = Xc[rows], C[rows]
    return dict(Xc=Xc, C=C, y_raw=1.5 + 2.5 * y, p=p, noise=noise, constant=const, Xt=Xt, Ct=Ct)


# the fit test's data seed (tests/test_mixed_kernel_reference.py asserts that two CPU fits from the
# start and from the start moved by 1e-8 end within the test's slack of each other at this seed)
FIT_SEED = 3


def fit_case(seed: int = FIT_SEED, n: int = 60):
    """n points with two continuous inputs and two categorical ones of three levels each; y has a
    strong categorical offset (tests/test_gpu_categorical.py _exps)."""
    rng = np.random.default_rng(seed)
    Xc = rng.uniform(size=(n, 2))
    C = rng.integers(0, 3, size=(n, 2)).astype(np.int32)
    off0, off1 = np.array([0.0, 0.5, -0.4]), np.array([0.2, 9.0, -0.1])
    y = (Xc[:, 0] - 0.3) ** 2 + (Xc[:, 1] - 0.6) ** 2 + off0[C[:, 0]] + off1[C[:, 1]]
    return Xc, C, y
