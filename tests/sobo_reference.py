"""CPU restatement (torch float64, autograd-capable) of the scalarised, output-constrained
single-objective acquisitions SoboStrategy / AdditiveSoboStrategy build
(bofire/strategies/predictives/sobo.py:42-222) — TEST INFRASTRUCTURE ONLY, composed from
oracle.qnehvi: ``QNEHVI(..., cells=[]).samples`` (the cached-Cholesky draw, S x b x q x m),
``joint_posterior``, ``fatplus``, ``fatmax``, ``logmeanexp``, ``log_feasibility`` (log_fatmoid)
and ``OutputConstraints``.

The term callables are written in the reference's own form (bofire/utils/torch_tools.py:
384-450), e.g. MinimizeSigmoid as ``1 - 1/(1+exp(-s(y-tp)))``.

BoTorch is not importable offline, so these forms restate [upstream]
SampleReducingMCAcquisitionFunction._apply_constraints, compute_best_feasible_objective,
_estimate_objective_lower_bound (the mean - 6 sigma fallback) and prune_inferior_points with
constraints from memory and are parity-unpinned against it."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from oracle import qnehvi as oq
from oracle.gp import psd_safe_cholesky
from tests.nei_reference import TAU_MAX, TAU_RELU, prune_inferior_points

AFFINE, CLOSE_TO_TARGET, SIGMOID, TARGET = 0, 1, 2, 3


@dataclass
class Utility:
    """u(y) = sum_t w_t g_t(y[..., out_t]); terms: (out, kind, w, p0, p1, p2).  SIGMOID with
    p0 > 0 is MaximizeSigmoid (steepness p0, tp p1), with p0 < 0 MinimizeSigmoid (steepness -p0);
    TARGET: steepness p0, target p1, tolerance p2."""
    terms: Sequence[tuple]

    @staticmethod
    def term(kind, p0, p1, p2, y):
        if kind == AFFINE:
            return y * p0 + p1
        if kind == CLOSE_TO_TARGET:
            return -1.0 * (torch.abs(y - p0) ** p1)
        if kind == SIGMOID:
            if p0 >= 0:
                return 1.0 / (1.0 + torch.exp(-1.0 * p0 * (y - p1)))
            return 1.0 - 1.0 / (1.0 + torch.exp(-1.0 * (-p0) * (y - p1)))
        return (1.0 / (1.0 + torch.exp(-1 * p0 * (y - (p1 - p2))))
                * (1.0 - 1.0 / (1.0 + torch.exp(-1.0 * p0 * (y - (p1 + p2))))))

    def __call__(self, Y):
        return sum(w * self.term(k, p0, p1, p2, Y[..., o]) for o, k, w, p0, p1, p2 in self.terms)


def constraints_of(cons) -> Optional[oq.OutputConstraints]:
    """[(out, sign, thr, eta)] -> oracle OutputConstraints (None when empty)."""
    if not cons:
        return None
    return oq.OutputConstraints([c[0] for c in cons], [c[1] for c in cons], [c[2] for c in cons],
                                [c[3] for c in cons])


def scan(Y: torch.Tensor, utility: Utility, cons: Optional[oq.OutputConstraints], best: torch.Tensor, log: bool,
         tau_relu: float = TAU_RELU, tau_max: float = TAU_MAX) -> torch.Tensor:
    """Y: S x b x q x m joint samples, best: S incumbents or one -> acq (b).  The feasibility
    weighs every (sample, point) before the reduction over q: multiplied in plain mode,
    added in log mode ([upstream] _apply_constraints)."""
    imp = utility(Y) - best.reshape(-1, 1, 1)
    if not log:
        v = imp.clamp_min(0.0)
        if cons is not None:
            v = v * cons.weight(Y)
        return v.max(-1).values.mean(0)
    li = oq.fatplus(imp, tau_relu).log()
    if cons is not None:
        li = li + oq.log_feasibility(cons, Y, fat=True)
    return oq.logmeanexp(oq.fatmax(li, dim=-1, tau=tau_max), dim=0)


def lower_bound(models, Xb: torch.Tensor, utility: Utility) -> torch.Tensor:
    """[upstream] _estimate_objective_lower_bound: min_k u(mu(x_k) - 6 sigma(x_k)) over the rows
    of Xb (noise-free posterior moments per output, original units)."""
    mean, cov = oq.joint_posterior(models, Xb)                      # n x m, m x n x n
    sigma = torch.diagonal(cov, dim1=-2, dim2=-1).clamp_min(0.0).sqrt().transpose(-1, -2)
    return utility(mean - 6.0 * sigma).min()


def best_feasible(u: torch.Tensor, feas: torch.Tensor, fallback) -> torch.Tensor:
    """[upstream] compute_best_feasible_objective on u, feas (... x n): max_k where(feas, u, iv),
    iv = -inf when every leading entry has a feasible row, else ``fallback()``."""
    iv = u.new_tensor(-math.inf) if bool(feas.any(-1).all()) else fallback()
    return torch.where(feas, u, iv).amax(-1)


def _feasible(cons, Y):
    return torch.ones(Y.shape[:-1], dtype=torch.bool) if cons is None else cons.feasible(Y)


def prune_rows(models, Xb: torch.Tensor, utility: Utility, cons, z_prune: torch.Tensor) -> torch.Tensor:
    """Kept rows of the baseline Xb (n x d) under the joint draws z_prune (S' x n x m):
    infeasible draws take the lower bound before the arg-max count."""
    mean, cov = oq.joint_posterior(models, Xb)
    L, _ = psd_safe_cholesky(cov)
    Y = mean.unsqueeze(0) + torch.einsum("jik,skj->sij", L, z_prune)
    u, feas = utility(Y), _feasible(cons, Y)
    if not bool(feas.all()):
        u = torch.where(feas, u, lower_bound(models, Xb, utility))
    return prune_inferior_points(u)


class SoboNEI:
    """Constrained / scalarised qNEI (log = False) / qLogNEI (log = True) over m outputs.  Xb: the
    (pruned) baseline; z_base S x nb x m, z_new S x q_tot x m; ``best`` overrides the per-sample
    incumbent; X_pending joins every candidate's joint batch.  An empty baseline samples the
    plain joint posterior (qEI / qLogEI with a scalar ``best``)."""

    def __init__(self, models, Xb, utility: Utility, cons, z_base, z_new, log=False, tau_relu=TAU_RELU,
                 tau_max=TAU_MAX, best=None, X_pending=None):
        self.models, self.utility, self.cons, self.z_new = models, utility, cons, z_new
        self.log, self.tau_relu, self.tau_max, self.X_pending = log, tau_relu, tau_max, X_pending
        self.orc = None
        m = len(models)
        if Xb.shape[0] > 0:
            self.orc = oq.QNEHVI(models, Xb, lambda y: y, torch.full((m,), -math.inf, dtype=torch.float64), z_base,
                                 z_new, cells=[])
            Yb = self.orc.base_obj                                   # S x nb x m model outputs
            self.best = best_feasible(utility(Yb), _feasible(cons, Yb), lambda: lower_bound(models, Xb, utility))
        if best is not None:
            self.best = best

    def samples(self, X):
        """X: b x q x d -> S x b x q x m."""
        if self.orc is not None:
            return self.orc.samples(X)
        mean, cov = oq.joint_posterior(self.models, X)              # b x q x m, b x m x q x q
        L, _ = psd_safe_cholesky(cov, max_tries=6)
        return mean.unsqueeze(0) + torch.einsum("bjqk,skj->sbqj", L, self.z_new)

    def forward(self, X):
        if self.X_pending is not None:
            X = torch.cat([X, self.X_pending.unsqueeze(0).expand(X.shape[0], *self.X_pending.shape)], -2)
        return scan(self.samples(X), self.utility, self.cons, self.best, self.log, self.tau_relu, self.tau_max)


def best_f(models, X_train: torch.Tensor, utility: Utility, cons) -> torch.Tensor:
    """qEI / qLogEI's scalar incumbent: the rule of ``best_feasible`` on the posterior means at
    X_train."""
    mean, _ = oq.joint_posterior(models, X_train)
    return best_feasible(utility(mean), _feasible(cons, mean), lambda: lower_bound(models, X_train, utility))
