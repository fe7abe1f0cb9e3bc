"""CPU restatement (torch float64, autograd-capable) of the single-objective improvement
acquisitions SoboStrategy builds (bofire/strategies/predictives/sobo.py:51-90): qNEI,
qLogNEI (its default) and qLogEI — TEST INFRASTRUCTURE ONLY, composed from oracle.qnehvi:
``joint_posterior``, ``QNEHVI.samples`` (the cached-Cholesky draw), ``fatplus``, ``fatmax``,
``logmeanexp`` — plus ``prune_inferior_points``.

BoTorch is not importable offline, so the constants (TAU_RELU = 1e-6, TAU_MAX = 1e-2,
fatmax alpha = 2) and forms restate [upstream] botorch.acquisition.logei and
botorch.utils.safe_math and are parity-unpinned against it."""
from __future__ import annotations

import math
from typing import Optional

import torch

from oracle import qnehvi as oq
from oracle.gp import psd_safe_cholesky

TAU_RELU = 1e-6   # botorch.acquisition.logei.TAU_RELU
TAU_MAX = 1e-2    # botorch.acquisition.logei.TAU_MAX


def prune_inferior_points(obj: torch.Tensor, max_frac: float = 1.0) -> torch.Tensor:
    """[upstream] botorch.acquisition.utils.prune_inferior_points on drawn objective values
    obj (S' x n): the rows that are the arg-max of at least one draw (sorted indices); more
    than ceil(max_frac n) of them are cut to the most probable ones."""
    n = obj.shape[1]
    probs = torch.bincount(obj.argmax(dim=1), minlength=n).to(torch.float64) / obj.shape[0]
    idx = probs.nonzero().view(-1)
    max_points = math.ceil(max_frac * n)
    if idx.shape[0] > max_points:
        idx = torch.sort(probs, stable=True, descending=True).indices[:max_points]
    return idx.sort().values


def prune_rows(models, Xb: torch.Tensor, a: float, b: float, z_prune: torch.Tensor) -> torch.Tensor:
    """Kept rows of the baseline Xb (n x d, normalized) under the joint draws z_prune
    (S' x n x 1) of its posterior (psd_safe_cholesky, 3 tries)."""
    mean, cov = oq.joint_posterior(models, Xb)                  # n x 1, 1 x n x n
    L, _ = psd_safe_cholesky(cov)
    Y = mean.unsqueeze(0) + torch.einsum("jik,skj->sij", L, z_prune)
    return prune_inferior_points(a * Y[..., 0] + b)


def scan(g: torch.Tensor, best: torch.Tensor, log: bool, tau_relu: float = TAU_RELU,
         tau_max: float = TAU_MAX) -> torch.Tensor:
    """The improvement scan: g (S x b x q objective samples), best (S incumbents, or one) ->
    plain: mean_s max_i (g - best_s)_+;  log: logmeanexp_s fatmax_i(log fatplus(g - best_s))."""
    imp = g - best.reshape(-1, 1, 1)
    if not log:
        return imp.clamp_min(0.0).max(-1).values.mean(0)
    li = oq.fatplus(imp, tau_relu).log()
    return oq.logmeanexp(oq.fatmax(li, dim=-1, tau=tau_max), dim=0)


class NEI:
    """qNEI (log = False) / qLogNEI (log = True) over one output with g = a y + b.  Xb: the
    (pruned) baseline, normalized; z_base S x nb x 1, z_new S x q_tot x 1; ``best`` overrides
    the per-sample incumbent max_k g(Y_base[s, k]); X_pending (normalized) joins every
    candidate's joint batch (concatenate_pending_points).  An empty baseline samples the plain
    joint posterior (what sample_cached_cholesky reduces to)."""

    def __init__(self, models, Xb: torch.Tensor, a: float, b: float, z_base: torch.Tensor, z_new: torch.Tensor,
                 log: bool = False, tau_relu: float = TAU_RELU, tau_max: float = TAU_MAX,
                 best: Optional[torch.Tensor] = None, X_pending: Optional[torch.Tensor] = None):
        self.models, self.a, self.b, self.z_new = models, float(a), float(b), z_new
        self.log, self.tau_relu, self.tau_max, self.X_pending = log, tau_relu, tau_max, X_pending
        self.orc = None
        if Xb.shape[0] > 0:
            obj = oq.Objective(torch.tensor([self.a], dtype=torch.float64), torch.tensor([self.b], dtype=torch.float64))
            self.orc = oq.QNEHVI(models, Xb, obj, torch.tensor([-math.inf], dtype=torch.float64), z_base, z_new,
                                 cells=[])
            self.best = self.orc.base_obj[..., 0].amax(dim=1)        # S
        if best is not None:
            self.best = best

    def samples(self, X: torch.Tensor) -> torch.Tensor:
        """X: b x q x d -> S x b x q."""
        if self.orc is not None:
            return self.orc.samples(X)[..., 0]
        mean, cov = oq.joint_posterior(self.models, X)             # b x q x 1, b x 1 x q x q
        L, _ = psd_safe_cholesky(cov[..., 0, :, :], max_tries=6)
        return mean[..., 0].unsqueeze(0) + torch.einsum("bqk,sk->sbq", L, self.z_new[..., 0])

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        if self.X_pending is not None:
            X = torch.cat([X, self.X_pending.unsqueeze(0).expand(X.shape[0], *self.X_pending.shape)], -2)
        g = self.a * self.samples(X) + self.b
        return scan(g, self.best, self.log, self.tau_relu, self.tau_max)


def log_ei(models, X: torch.Tensor, best_f: float, z: torch.Tensor, a: float, b: float, log: bool = True,
           tau_relu: float = TAU_RELU, tau_max: float = TAU_MAX, X_pending: Optional[torch.Tensor] = None):
    """qLogEI (log = False: qEI) over plain joint samples: X b x q x d, z S x q_tot."""
    nei = NEI(models, X.new_zeros(0, X.shape[-1]), a, b, z.new_zeros(z.shape[0], 0, 1), z.unsqueeze(-1), log=log,
              tau_relu=tau_relu, tau_max=tau_max, best=torch.tensor([float(best_f)], dtype=torch.float64),
              X_pending=X_pending)
    return nei.forward(X)
