"""CPU references of the mixed GP inside the single-objective acquisition chain — TEST
INFRASTRUCTURE ONLY, importing nothing of everest_amd.

``cross_grad``: numpy long double, the explicit sum of the mixed cross-covariance X-gradient
(the formula of include/everest_amd.h, evr_mixed_kernel_cross_grad), with the sum of the absolute
values of the summed terms beside it (the scale of the error bar).

``MixedModels``: torch float64 with autograd, m mixed members on shared training inputs, built
from tests/mixed_gp_restatement.kernel: the split of raw transformed rows (continuous columns
normalised, arg-max codes — no gradient through the codes), the joint posterior mean /
covariance at a joint batch, and from them
  qEI / qLogEI:   plain Cholesky of the q x q covariance, samples mean + L z, then the scan of
                  tests/nei_reference.scan (one output) or tests/sobo_reference.scan;
  qNEI / qLogNEI: ONE Cholesky of the joint covariance over [baseline; new points] with base
                  samples [z_base; z_new] — what [upstream] sample_cached_cholesky equals when no
                  jitter is applied, and independent of the device's split operator
                  M = [L^-1; G; H^T; alpha^T].
Every Cholesky here is un-jittered (torch.linalg.cholesky_ex): ``ok`` reports whether each one
succeeded, the tests assert it.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import mixed_gp_restatement as mr
from tests.gp_kernel_reference import LD, dscale

F64 = torch.float64


# ---------------------------------------------------------------------------------------
# X-gradient of K(train, candidates): explicit sum in long double
# ---------------------------------------------------------------------------------------
def cross_grad(Xc, C, X2c, C2, params, G, kind: int):
    """(g, S), rows x dc each: g[j, k] = sum_b sum_i G[b, i, j] (s_sum k_c'(r1^2) / ls1_k^2
    + s_prod h2 k_c'(r2^2) / ls2_k^2) (x2_jk - x1_ik), S the sum of the absolute values of the same
    (b, i, part) terms.  k_c' = dscale (zero where r^2 < 1e-30)."""
    u1, u2 = np.asarray(Xc, np.float64).astype(LD), np.asarray(X2c, np.float64).astype(LD)
    c1, c2 = np.asarray(C), np.asarray(C2)
    params = np.atleast_2d(np.asarray(params, np.float64)).astype(LD)
    G = np.asarray(G, np.float64).astype(LD)
    dc, nc = u1.shape[1], c1.shape[1]
    g = np.zeros((u2.shape[0], dc), dtype=LD)
    S = np.zeros_like(g)
    diff = u2[None, :, :] - u1[:, None, :]                      # n x rows x dc
    ne = (c1[:, None, :] != c2[None, :, :]).astype(LD)
    for b, p in enumerate(params):
        ls1, ls2, lam2 = p[:dc], p[dc:2 * dc], p[2 * dc + nc:2 * dc + 2 * nc]
        s_sum, s_prod = p[-3], p[-1]
        d21 = ((diff / ls1) ** 2).sum(-1)
        d22 = ((diff / ls2) ** 2).sum(-1)
        h2 = np.exp(-(ne / lam2).sum(-1) / LD(nc))
        t1 = (G[b] * s_sum * dscale(kind, d21))[:, :, None] * diff / (ls1 * ls1)
        t2 = (G[b] * s_prod * h2 * dscale(kind, d22))[:, :, None] * diff / (ls2 * ls2)
        g += t1.sum(0) + t2.sum(0)
        S += np.abs(t1).sum(0) + np.abs(t2).sum(0)
    return g, S


# ---------------------------------------------------------------------------------------
# the mixed members and their joint posterior
# ---------------------------------------------------------------------------------------
class MixedModels:
    """m members sharing the training inputs.  Xc n x dc (normalised), C n x nc, Y n x m raw
    targets, params m x P, noise / const / ym / ys (m): the hyperparameters and the standardisation
    the device model was given.  lo / hi (d), cont_cols (dc), cat_blocks (nc index arrays): the
    layout of the raw transformed row."""

    def __init__(self, Xc, C, Y, params, noise, const, ym, ys, kind, lo, hi, cont_cols, cat_blocks):
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
        self.Xc, self.C = t(Xc), torch.as_tensor(np.asarray(C)).long()
        self.params, self.noise, self.const, self.ym, self.ys = t(params), t(noise), t(const), t(ym), t(ys)
        self.kind, self.m, self.n = int(kind), len(noise), self.Xc.shape[0]
        self.lo, self.hi = t(lo), t(hi)
        self.cont = torch.as_tensor(np.asarray(cont_cols)).long()
        self.blocks = [torch.as_tensor(np.asarray(b)).long() for b in cat_blocks]
        Ys = (t(Y) - self.ym) / self.ys                                  # n x m standardised
        self.L, self.alpha = [], []
        eye = torch.eye(self.n, dtype=F64)
        for j in range(self.m):
            K = mr.kernel(self.Xc, self.C, self.Xc, self.C, self.params[j], self.kind) + self.noise[j] * eye
            L = torch.linalg.cholesky(K)
            self.L.append(L)
            self.alpha.append(torch.cholesky_solve((Ys[:, j] - self.const[j]).unsqueeze(-1), L)[:, 0])

    def split(self, X):
        """Raw rows (... x d) -> (Xc ... x dc, differentiable; C ... x nc codes)."""
        Xc = (X[..., self.cont] - self.lo[self.cont]) / (self.hi[self.cont] - self.lo[self.cont])
        C = torch.stack([X[..., blk].detach().argmax(-1) for blk in self.blocks], -1)
        return Xc, C

    def joint_posterior(self, X):
        """X: k x d raw rows -> (mean k x m, cov m x k x k), noise-free, original units."""
        Xc, C = self.split(X)
        means, covs = [], []
        for j in range(self.m):
            p = self.params[j]
            Ks = mr.kernel(self.Xc, self.C, Xc, C, p, self.kind)         # n x k
            V = torch.linalg.solve_triangular(self.L[j], Ks, upper=False)
            Kss = mr.kernel(Xc, C, Xc, C, p, self.kind)
            means.append(self.ym[j] + self.ys[j] * (self.const[j] + Ks.T @ self.alpha[j]))
            covs.append(self.ys[j] ** 2 * (Kss - V.T @ V))
        return torch.stack(means, -1), torch.stack(covs, 0)

    def samples(self, X, z_new, Xb=None, z_base=None):
        """Joint samples of the batches X (b x q x d): (Y S x b x q x m, Y_base S x nb x m | None,
        ok).  z_new S x q x m; with a baseline Xb (nb x d raw rows) and z_base (S x nb x m) the draw is
        the one Cholesky over [baseline; new points].  ok: every un-jittered Cholesky succeeded."""
        nb = 0 if Xb is None else Xb.shape[0]
        out, ok, Yb = [], True, None
        for c in range(X.shape[0]):
            Xj = X[c] if nb == 0 else torch.cat([Xb, X[c]], 0)
            z = z_new if nb == 0 else torch.cat([z_base, z_new], 1)      # S x (nb + q) x m
            mean, cov = self.joint_posterior(Xj)
            cov = 0.5 * (cov + cov.transpose(-1, -2))
            L, info = torch.linalg.cholesky_ex(cov)
            ok = ok and bool((info == 0).all())
            Y = mean.unsqueeze(0) + torch.einsum("jik,skj->sij", L, z)   # S x (nb + q) x m
            out.append(Y[:, nb:])
            if nb and Yb is None:
                Yb = Y[:, :nb].detach()
        return torch.stack(out, 1), Yb, ok
