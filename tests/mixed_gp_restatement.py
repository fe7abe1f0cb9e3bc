"""Torch float64 restatement of the mixed GP on the CPU ([upstream] BoTorch MixedSingleTaskGP as
the issue specifies it; BoTorch is not installed), differentiated by autograd: the kernel, the
exact MLL / n with the hyperpriors, the Cholesky posterior and the scipy L-BFGS-B fit.  Written
the way GPyTorch forms the kernel (inputs divided by the lengthscales first, then distances),
independent of tests/mixed_kernel_reference.py and of everest_amd.

Raw vector: x = [noise, constant, raw ls1, raw ls2, raw lam1 (nc), raw lam2 (nc), raw s_sum,
raw s_cat, raw s_prod]; ls = softplus(raw) (dc values per kernel, or one with ard=False),
lam = 1e-6 + softplus(raw), scales = softplus(raw).  Priors: (family, p1, p2) tuples, "gamma"
(concentration, rate) or "lognormal" (loc, scale), on both lengthscale sets and on the noise.
"""
from __future__ import annotations

import math

import numpy as np
import torch

MIN_LAM = 1e-6
MIN_NOISE = 1e-6
NOISE0 = 1e-3


def continuous_kernel(A: torch.Tensor, Bm: torch.Tensor, ls: torch.Tensor, kind: int) -> torch.Tensor:
    a, b = A / ls, Bm / ls
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    if kind == 0:
        return torch.exp(-0.5 * d2)
    r = d2.clamp_min(1e-30).sqrt()
    if kind == 1:
        return torch.exp(-r)
    if kind == 2:
        return (1 + math.sqrt(3) * r) * torch.exp(-math.sqrt(3) * r)
    return (1 + math.sqrt(5) * r + 5.0 / 3.0 * r ** 2) * torch.exp(-math.sqrt(5) * r)


def categorical_kernel(C1: torch.Tensor, C2: torch.Tensor, lam: torch.Tensor) -> torch.Tensor:
    ne = (C1[:, None, :] != C2[None, :, :]).to(torch.float64)
    return torch.exp(-(ne / lam).mean(-1))


def kernel(Xc1, C1, Xc2, C2, p: torch.Tensor, kind: int) -> torch.Tensor:
    """K (n1 x n2) of one member's parameter vector p (2 dc + 2 nc + 3)."""
    dc, nc = Xc1.shape[1], C1.shape[1]
    ls1, ls2, lam1, lam2 = p[:dc], p[dc:2 * dc], p[2 * dc:2 * dc + nc], p[2 * dc + nc:2 * dc + 2 * nc]
    s_sum, s_cat, s_prod = p[-3], p[-2], p[-1]
    return (s_sum * (continuous_kernel(Xc1, Xc2, ls1, kind) + s_cat * categorical_kernel(C1, C2, lam1))
            + s_prod * continuous_kernel(Xc1, Xc2, ls2, kind) * categorical_kernel(C1, C2, lam2))


def params_of(x: torch.Tensor, dc: int, nc: int, ard: bool = True) -> torch.Tensor:
    """The kernel's parameter vector (2 dc + 2 nc + 3) of the raw vector x."""
    sp = torch.nn.functional.softplus
    nls = dc if ard else 1
    raw = x[2:]
    ls = sp(raw[:2 * nls]).reshape(2, nls).expand(2, dc).reshape(-1)
    lam = MIN_LAM + sp(raw[2 * nls:2 * nls + 2 * nc])
    return torch.cat([ls, lam, sp(raw[2 * nls + 2 * nc:])])


def log_prior(prior, v: torch.Tensor) -> torch.Tensor:
    if prior is None:
        return v.new_zeros(())
    fam, a, b = prior
    if fam == "gamma":
        return (a * math.log(b) - math.lgamma(a) + (a - 1) * torch.log(v) - b * v).sum()
    if fam == "lognormal":
        lv = torch.log(v)
        return (-lv - math.log(b) - 0.5 * math.log(2 * math.pi) - 0.5 * ((lv - a) / b) ** 2).sum()
    raise ValueError(fam)


def mll(x: torch.Tensor, Xc, C, y, kind: int, ls_prior, noise_prior, ard: bool = True) -> torch.Tensor:
    """(MLL + sum log prior) / n at the raw vector x (constant mean, standardised targets y)."""
    n, dc = Xc.shape
    nc = C.shape[1]
    p = params_of(x, dc, nc, ard)
    K = kernel(Xc, C, Xc, C, p, kind) + x[0] * torch.eye(n, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    r = (y - x[1]).unsqueeze(-1)
    alpha = torch.cholesky_solve(r, L)
    ll = -0.5 * (r * alpha).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * math.log(2 * math.pi)
    nls = dc if ard else 1
    ls = p[:2 * dc].reshape(2, dc)[:, :nls]          # the lengthscales as parameters: one per kernel without ARD
    return (ll + log_prior(ls_prior, ls) + log_prior(noise_prior, x[0])) / n


def mll_value_and_grad(x: np.ndarray, Xc, C, y, kind, ls_prior, noise_prior, ard=True):
    t = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    v = mll(t, torch.as_tensor(Xc), torch.as_tensor(C), torch.as_tensor(y), kind, ls_prior, noise_prior, ard)
    v.backward()
    return v.item(), t.grad.numpy().copy()


def posterior(Xc, C, y_raw, p, noise, constant, Xt, Ct, kind, observation_noise=True):
    """Posterior mean and variance in raw target units by the Cholesky of K + noise I."""
    Xc, C, Xt, Ct = (torch.as_tensor(a) for a in (Xc, C, Xt, Ct))
    y_raw = torch.as_tensor(y_raw)
    ym, ys = y_raw.mean(), y_raw.std()
    p = torch.as_tensor(p)
    n = Xc.shape[0]
    L = torch.linalg.cholesky(kernel(Xc, C, Xc, C, p, kind) + noise * torch.eye(n, dtype=torch.float64))
    Ks = kernel(Xc, C, Xt, Ct, p, kind)
    alpha = torch.cholesky_solve(((y_raw - ym) / ys - constant).unsqueeze(-1), L)
    V = torch.linalg.solve_triangular(L, Ks, upper=False)
    var = p[-3] * (1 + p[-2]) + p[-1] - (V * V).sum(0) + (noise if observation_noise else 0.0)
    return (ym + ys * (constant + (Ks * alpha).sum(0))).numpy(), (ys ** 2 * var).numpy(), float(ym), float(ys)


def start(dc: int, nc: int, ard: bool = True) -> np.ndarray:
    x0 = np.zeros(2 + 2 * (dc if ard else 1) + 2 * nc + 3)
    x0[0] = NOISE0
    return x0


def fit(Xc, C, y, kind, ls_prior, noise_prior, ard=True, x0=None, options=None):
    """scipy L-BFGS-B on -mll from x0 (default: the start point), noise >= 1e-6.  Returns the raw
    vector found."""
    from scipy.optimize import minimize

    x0 = start(Xc.shape[1], C.shape[1], ard) if x0 is None else np.asarray(x0, dtype=np.float64)

    def f(x):
        v, g = mll_value_and_grad(x, Xc, C, y, kind, ls_prior, noise_prior, ard)
        return -v, -g

    res = minimize(f, x0, jac=True, method="L-BFGS-B", bounds=[(MIN_NOISE, None)] + [(None, None)] * (len(x0) - 1),
                   options=options or {})
    return res.x
