"""References of the scaled kernel k = sigma^2 k_base (ScaleKernel around RBF / Matérn), written
from the formulas alone; imports nothing of everest_amd.

* ``outputscale_grad``: sum_ij W_ij k_base(x_i, x_j) in long double, with the sum of the absolute
  values of the same terms (the scale its error bar is taken against), next to
  tests/gp_kernel_reference.lengthscale_grad (whose result times sigma^2 is the scaled kernel's
  lengthscale piece).
* ``mll_value``: oracle.gp.mll_value restated with sigma^2 = softplus(raw) on the kernel and an
  optional prior on sigma^2, as a differentiable CPU torch scalar, for autograd.
* ``scaled_case``: gp_kernel_reference.mll_case with a raw outputscale appended to each x.
* ``posterior``: mean and variance (with observation noise) of the scaled, unfolded GP in
  physical units, in any numpy float type.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import gp as ogp
from tests import gp_kernel_reference as ref

LD = np.longdouble
OUTPUTSCALES = (0.05, math.log(2.0), 7.0)


def kernel_value_ld(kind: int, d2):
    """k_base(d2) in long double (GPyTorch's forms; Matérn distance clamped at 1e-30)."""
    d2 = np.asarray(d2, dtype=LD)
    if kind == ref.RBF:
        return np.exp(-d2 / 2)
    r = np.sqrt(np.maximum(d2, LD(1e-30)))
    if kind == ref.MATERN05:
        return np.exp(-r)
    if kind == ref.MATERN15:
        s = np.sqrt(LD(3)) * r
        return (1 + s) * np.exp(-s)
    s = np.sqrt(LD(5)) * r
    return (1 + s + LD(5) / 3 * d2) * np.exp(-s)


def outputscale_grad(X, ls, W, kinds, row_chunk: int = 32):
    """g[b] = sum_i sum_j W[b,i,j] k_base_b(x_i, x_j) and S[b], the sum of the absolute terms."""
    u, ls, W = np.asarray(X, dtype=LD), np.asarray(ls, dtype=LD), np.asarray(W, dtype=LD)
    B = ls.shape[0]
    n = u.shape[0]
    kinds = [int(kinds)] * B if np.isscalar(kinds) else [int(k) for k in kinds]
    g, S = np.zeros(B, dtype=LD), np.zeros(B, dtype=LD)
    for b in range(B):
        for i0 in range(0, n, row_chunk):
            diff = (u[None, :, :] - u[i0:i0 + row_chunk, None, :]) / ls[b]
            term = W[b, i0:i0 + row_chunk] * kernel_value_ld(kinds[b], (diff * diff).sum(-1))
            g[b] += term.sum()
            S[b] += np.abs(term).sum()
    return g, S


def _logpdf(prior, x):
    """log density of ("lognormal" | "gamma" | "normal", a, b) at the torch scalar / tensor x."""
    fam, a, b = prior
    if fam == "lognormal":
        lx = torch.log(x)
        return -lx - math.log(b) - 0.5 * math.log(2 * math.pi) - 0.5 * ((lx - a) / b) ** 2
    if fam == "gamma":
        return a * math.log(b) - math.lgamma(a) + (a - 1) * torch.log(x) - b * x
    return -0.5 * math.log(2 * math.pi * b * b) - 0.5 * ((x - a) / b) ** 2


def mll_value(X, y, x, d, kind, ls_prior, noise_prior, os_prior):
    """[log N(y | c, sigma^2 k_base + s2 I) + log p(ls) + log p(s2) + log p(sigma^2)] / n for
    x = [noise, constant, raw ls (d), raw sigma^2] (a torch vector), priors as (family, a, b) or None."""
    noise, const, ls, os_ = x[0], x[1], ogp.softplus(x[2:2 + d]), ogp.softplus(x[2 + d])
    n = X.shape[0]
    K = os_ * ogp.kernel_matrix(X, X, ls, kind) + noise * torch.eye(n, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    r = (y - const).unsqueeze(-1)
    a = torch.cholesky_solve(r, L)
    ll = -0.5 * (r * a).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * math.log(2 * math.pi)
    if ls_prior is not None:
        ll = ll + _logpdf(ls_prior, ls).sum()
    if noise_prior is not None:
        ll = ll + _logpdf(noise_prior, noise)
    if os_prior is not None:
        ll = ll + _logpdf(os_prior, os_)
    return ll / n


def mll_value_and_grad(X, y, x, d, kind, ls_prior, noise_prior, os_prior):
    t = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    v = mll_value(torch.tensor(X), torch.tensor(y), t, d, kind, ls_prior, noise_prior, os_prior)
    v.backward()
    return v.item(), t.grad.numpy().copy()


def scaled_case(n: int, d: int, B: int):
    """mll_case(n, d, B) with softplus(raw outputscale) = OUTPUTSCALES[b % 3] appended to each x."""
    X, Ys, xs = ref.mll_case(n, d, B)
    raw = ref.inv_softplus(np.array([OUTPUTSCALES[b % 3] for b in range(B)]))
    return X, Ys, np.concatenate([xs, raw[:, None]], 1)


def posterior(Xn, y, Xtn, ls, noise, const, os_, y_mean, y_std, kind, dtype):
    """Mean and variance with observation noise of the scaled GP at the normalised points Xtn, in
    physical units, every step in ``dtype`` (solves by Cholesky-free elimination: np.linalg.solve
    does not take long double, so a plain Gaussian elimination with partial pivoting is used)."""
    f = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    Xn, y, Xtn, ls = f(Xn), f(y), f(Xtn), f(ls)
    noise, const, os_, y_mean, y_std = (dtype(v) for v in (noise, const, os_, y_mean, y_std))

    def k(A, B):
        diff = (A[:, None, :] - B[None, :, :]) / ls
        d2 = (diff * diff).sum(-1)
        if kind == ref.RBF:
            return np.exp(-d2 / 2)
        r = np.sqrt(np.maximum(d2, dtype(1e-30)))
        if kind == ref.MATERN05:
            return np.exp(-r)
        if kind == ref.MATERN15:
            s = np.sqrt(dtype(3)) * r
            return (1 + s) * np.exp(-s)
        s = np.sqrt(dtype(5)) * r
        return (1 + s + dtype(5) / 3 * d2) * np.exp(-s)

    n = Xn.shape[0]
    K = os_ * k(Xn, Xn) + noise * np.eye(n, dtype=dtype)
    Ks = os_ * k(Xn, Xtn)
    rhs = np.concatenate([((y - y_mean) / y_std - const)[:, None], Ks], 1)
    sol = _solve(K, rhs)
    mean = const + Ks.T @ sol[:, 0]
    var = os_ - (Ks * sol[:, 1:]).sum(0) + noise
    return y_mean + y_std * mean, y_std * y_std * var


def _solve(A, Bm):
    A, Bm = A.copy(), Bm.copy()
    n = A.shape[0]
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]], Bm[[c, p]] = A[[p, c]], Bm[[p, c]]
        f = A[c + 1:, c] / A[c, c]
        A[c + 1:] -= f[:, None] * A[c]
        Bm[c + 1:] -= f[:, None] * Bm[c]
    for c in range(n - 1, -1, -1):
        Bm[c] = (Bm[c] - A[c, c + 1:] @ Bm[c + 1:]) / A[c, c]
    return Bm
