"""CPU restatement (torch float64, autograd-capable) of the qSR / qUCB / qPI acquisitions
SoboStrategy / AdditiveSoboStrategy build (bofire/strategies/predictives/sobo.py:42-222 with
botorch.py:726-750) — TEST INFRASTRUCTURE ONLY, composed from tests/sobo_reference.py and
oracle.qnehvi (``joint_posterior``, ``OutputConstraints``).

BoTorch is not importable offline, so these forms restate from memory, parity-unpinned:
  [upstream] ConstrainedMCObjective / apply_constraints:  r = (u + M) W - M,
      W = exp(sum_e logsigmoid(-c_e / eta_e)) (plain sigmoid), r = u without constraints;
  [upstream] get_infeasible_cost:  M = -min(0, min_x u(mu(x) - 6 sigma(x)));
  [upstream] qSimpleRegret:  mean_s max_i r;
  [upstream] qUpperConfidenceBound:  mean_s max_i (rbar + sqrt(beta pi / 2) |r - rbar|), rbar = mean_s r;
  [upstream] qProbabilityOfImprovement with SampleReducingMCAcquisitionFunction._apply_constraints:
      mean_s max_i [ sigmoid((u - best_f) / tau) W ]."""
from __future__ import annotations

import math
from typing import Optional

import torch

from oracle import qnehvi as oq
from oracle.gp import psd_safe_cholesky
from tests import sobo_reference as sr

SR, UCB, PI = "SR", "UCB", "PI"


def reward(Y: torch.Tensor, utility: sr.Utility, cons: Optional[oq.OutputConstraints], M: float) -> torch.Tensor:
    """Y: ... x m -> r (...): add M, multiply by the soft indicators, subtract M again."""
    u = utility(Y)
    if cons is None:
        return u
    return u.add(M).mul(cons.weight(Y)).sub(M)


def scan(Y: torch.Tensor, utility: sr.Utility, cons: Optional[oq.OutputConstraints], mode: str, beta: float = 0.2,
         tau: float = 1e-3, best_f=None, M: float = 0.0) -> torch.Tensor:
    """Y: S x b x q x m joint samples -> acq (b)."""
    if mode == PI:
        v = torch.sigmoid((utility(Y) - best_f) / tau)
        if cons is not None:
            v = v * cons.weight(Y)
        return v.max(-1).values.mean(0)
    r = reward(Y, utility, cons, M)
    if mode == UCB:
        mean = r.mean(0)
        r = mean + math.sqrt(beta * math.pi / 2.0) * (r - mean).abs()
    return r.max(-1).values.mean(0)


def infeasible_cost(models, X: torch.Tensor, utility: sr.Utility) -> float:
    """M over the rows of X (normalised inputs): noise-free posterior moments per output."""
    return float((-sr.lower_bound(models, X, utility)).clamp_min(0.0))


class Reward:
    """The full chain: plain joint samples y = mu + chol(Sigma_qq) z per output (z_new S x q_tot x
    m), pending points joined to every candidate's batch, then ``scan``."""

    def __init__(self, models, utility: sr.Utility, cons, z_new: torch.Tensor, mode: str, beta: float = 0.2,
                 tau: float = 1e-3, best_f=None, M: float = 0.0, X_pending=None):
        self.models, self.utility, self.cons, self.z_new = models, utility, cons, z_new
        self.mode, self.beta, self.tau, self.best_f, self.M, self.X_pending = mode, beta, tau, best_f, M, X_pending

    def samples(self, X):
        mean, cov = oq.joint_posterior(self.models, X)              # b x q x m, b x m x q x q
        L, _ = psd_safe_cholesky(cov, max_tries=6)
        return mean.unsqueeze(0) + torch.einsum("bjqk,skj->sbqj", L, self.z_new)

    def forward(self, X):
        if self.X_pending is not None:
            X = torch.cat([X, self.X_pending.unsqueeze(0).expand(X.shape[0], *self.X_pending.shape)], -2)
        return scan(self.samples(X), self.utility, self.cons, self.mode, self.beta, self.tau, self.best_f, self.M)
