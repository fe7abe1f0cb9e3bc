"""Torch-CPU float64 restatement of the negative integrated posterior variance
(everest_amd.acquisition.QNegIntPosVar, nipv.hip), by two routes.

``direct``      conditions each output's GP on [Xn; X_c] with one dense (n + q) Cholesky and
                averages the posterior variance over the integration points.  It shares nothing
                with the device's algebra; gradients come from autograd.
``schur_route`` is the device's own route in torch: the explicit L^-1 of the training block, the
                Schur complement A of the candidate block and the Gram trace tr(A^-1 G) / N.

Both take raw inputs with the model's normalisation bounds ``lo`` / ``hi``; kernels are k(x, x) = 1
(standardised units), ``coef_j = w_j^2 ys_j^2`` carries the weights and output scales.

The error of ``schur_route`` against ``direct`` is the yardstick the device tests derive their
bounds from (``bounds``): the device differs from ``schur_route`` only in summation order and FMA
contraction."""
import math

import torch

RBF, MATERN05, MATERN15, MATERN25 = 0, 1, 2, 3
EPS = 2.220446049250313e-16


def kernel(x1: torch.Tensor, x2: torch.Tensor, ls: torch.Tensor, kind: int) -> torch.Tensor:
    """k(x1, x2) for normalised inputs; Matern distances clamp d^2 at 1e-30 like GPyTorch."""
    df = (x1[:, None, :] - x2[None, :, :]) / ls
    d2 = (df * df).sum(-1)
    if kind == RBF:
        return torch.exp(-0.5 * d2)
    r = torch.sqrt(torch.clamp(d2, min=1e-30))
    if kind == MATERN05:
        return torch.exp(-r)
    if kind == MATERN15:
        s = math.sqrt(3.0) * r
        return (1.0 + s) * torch.exp(-s)
    s = math.sqrt(5.0) * r
    return (1.0 + s + (5.0 / 3.0) * d2) * torch.exp(-s)


def _t(a):
    return torch.as_tensor(a, dtype=torch.float64)


def _norm(X, lo, hi):
    return (X - lo) / (hi - lo)


def direct(Xn, P, Xc, ls, noise, kinds, coef, lo=None, hi=None) -> torch.Tensor:
    """acq of ONE candidate Xc (q x d raw): - sum_j coef_j mean_p var_j(p | Xn, Xc).  Xn: n x d
    normalised training rows; P (N x d) and Xc raw; ls B x d; noise, coef: B."""
    Xn, P, Xc, ls = _t(Xn), _t(P), Xc if isinstance(Xc, torch.Tensor) else _t(Xc), _t(ls)
    d = Xn.shape[1]
    lo = torch.zeros(d, dtype=torch.float64) if lo is None else _t(lo)
    hi = torch.ones(d, dtype=torch.float64) if hi is None else _t(hi)
    Z = torch.cat([Xn, _norm(Xc, lo, hi)], 0)
    Pn = _norm(P, lo, hi)
    acq = Xc.new_zeros(())
    for j, kind in enumerate(kinds):
        K = kernel(Z, Z, ls[j], kind) + float(noise[j]) * torch.eye(Z.shape[0], dtype=torch.float64)
        L = torch.linalg.cholesky(K)
        v = torch.linalg.solve_triangular(L, kernel(Z, Pn, ls[j], kind), upper=False)
        var = 1.0 - (v * v).sum(0)
        acq = acq - float(coef[j]) * var.mean()
    return acq


def schur_route(Xn, P, Xc, ls, noise, kinds, coef, lo=None, hi=None) -> torch.Tensor:
    """The same value by the device's algebra (explicit L^-1, Schur complement, Gram trace)."""
    Xn, P, Xc, ls = _t(Xn), _t(P), Xc if isinstance(Xc, torch.Tensor) else _t(Xc), _t(ls)
    n, d = Xn.shape
    lo = torch.zeros(d, dtype=torch.float64) if lo is None else _t(lo)
    hi = torch.ones(d, dtype=torch.float64) if hi is None else _t(hi)
    Xq, Pn = _norm(Xc, lo, hi), _norm(P, lo, hi)
    N, q = Pn.shape[0], Xq.shape[0]
    acq = Xc.new_zeros(())
    eye = torch.eye(n, dtype=torch.float64)
    for j, kind in enumerate(kinds):
        L = torch.linalg.cholesky(kernel(Xn, Xn, ls[j], kind) + float(noise[j]) * eye)
        Linv = torch.linalg.solve_triangular(L, eye, upper=False)
        Vp = Linv @ kernel(Xn, Pn, ls[j], kind)
        v0 = (1.0 - (Vp * Vp).sum(0)).mean()
        Vx = Linv @ kernel(Xn, Xq, ls[j], kind)
        C = kernel(Pn, Xq, ls[j], kind) - Vp.T @ Vx
        Kqq = kernel(Xq, Xq, ls[j], kind)
        Kqq = Kqq - torch.diag(torch.diagonal(Kqq)) + torch.eye(q, dtype=torch.float64)     # k(x, x) = 1
        A = Kqq - Vx.T @ Vx + float(noise[j]) * torch.eye(q, dtype=torch.float64)
        G = C.T @ C
        tr = torch.trace(torch.cholesky_solve(G, torch.linalg.cholesky(A)))
        acq = acq - float(coef[j]) * (v0 - tr / N)
    return acq


def batch(route, Xn, P, X, ls, noise, kinds, coef, lo=None, hi=None, grad=True, gout=None):
    """Values (b) and gradients (b x q x d, of sum_c gout_c acq_c) of ``route`` over the candidates
    X (b x q x d raw)."""
    X = _t(X).clone().requires_grad_(grad)
    vals = torch.stack([route(Xn, P, X[c], ls, noise, kinds, coef, lo, hi) for c in range(X.shape[0])])
    if not grad:
        return vals.detach(), None
    w = torch.ones_like(vals) if gout is None else _t(gout)
    (g,) = torch.autograd.grad((vals * w).sum(), X)
    return vals.detach(), g


def value_error(a, ref) -> float:
    """Largest relative error of the values a against ref."""
    a, ref = _t(a), _t(ref)
    return float(((a - ref).abs() / ref.abs()).max())


def row_error(g, ref) -> float:
    """Largest row-relative error of gradients: per candidate (one row of b), the largest absolute
    difference over its q x d entries relative to the largest reference entry of that row."""
    g, ref = _t(g).reshape(ref.shape[0], -1), _t(ref).reshape(ref.shape[0], -1)
    return float(((g - ref).abs().max(1).values / ref.abs().max(1).values).max())


def bounds(e_val: float, e_grad: float, coef) -> tuple:
    """The device's bounds from the CPU error e of schur_route against direct:
    max(8 e, 64 * 2.2e-16 * sum_j coef_j).  The factor 8 covers summation order and FMA
    contraction, the only differences between schur_route and the kernel; the floor is the rounding
    of N differences of O(1) terms."""
    floor = 64.0 * EPS * float(_t(coef).sum())
    return max(8.0 * e_val, floor), max(8.0 * e_grad, floor)
