"""CPU restatement (torch float64, autograd-capable) of qParEGO's utility — TEST INFRASTRUCTURE
ONLY.

``Chebyshev`` is the augmented Chebyshev utility u = min_k (A_k g_k + B_k) + alpha sum_k (...)
with the call signature of ``sobo_reference.Utility``, so ``sr.scan``, ``sr.SoboNEI``,
``sr.best_f`` and ``sr.prune_rows`` take it unchanged.

``botorch_scalarization`` restates [upstream] botorch.utils.multi_objective.scalarization.
get_chebyshev_scalarization in BoTorch's own form (``normalize`` to the bounds of Y, the -1
shift of the minimised columns, max-plus-sum of the negated products, negated) and
``terms_from_botorch`` reads the (A_k, B_k) of the device table off it.  BoTorch is not
importable offline, so the form is written from memory and parity-unpinned against it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import torch

from tests.sobo_reference import AFFINE, CLOSE_TO_TARGET, Utility


@dataclass
class Chebyshev:
    """terms: (out, kind, p0, p1, A, B), kind AFFINE or CLOSE_TO_TARGET."""
    terms: Sequence[tuple]
    alpha: float

    def term_values(self, Y):
        for _, k, *_ in self.terms:
            assert k in (AFFINE, CLOSE_TO_TARGET)
        return torch.stack([A * Utility.term(k, p0, p1, 0.0, Y[..., o]) + B for o, k, p0, p1, A, B in self.terms], -1)

    def __call__(self, Y):
        t = self.term_values(Y)
        return t.min(-1).values + self.alpha * t.sum(-1)


def botorch_scalarization(weights: torch.Tensor, Y: torch.Tensor, alpha: float = 0.05):
    """get_chebyshev_scalarization(weights, Y, alpha): returns (obj, products) — obj(Y) is the
    scalarisation (to be maximised), products(Y) the per-objective weighted values whose
    minimum and sum it combines."""
    minimize = weights < 0
    if Y.shape[-2] == 1:
        Y_bounds = torch.cat([Y, Y + 1], dim=0)
    else:
        Y_bounds = torch.stack([Y.min(dim=-2).values, Y.max(dim=-2).values])

    def normalized(Y):
        Yn = (Y - Y_bounds[0]) / (Y_bounds[1] - Y_bounds[0])       # botorch.utils.transforms.normalize
        Yn = Yn.clone()
        Yn[..., minimize] = Yn[..., minimize] - 1                   # minimised columns to [-1, 0]
        return Yn

    def chebyshev_obj(Y):
        product = weights * Y
        return product.max(dim=-1).values + alpha * product.sum(dim=-1)

    def obj(Y):
        return -1 * chebyshev_obj(-normalized(Y))

    def products(Y):
        return -1 * (weights * -normalized(Y))

    return obj, products


def terms_from_botorch(w, mask, z):
    """[(A_k, B_k)] such that products(g * mask)_k = A_k g_k + B_k for the scalarisation with
    weights w * mask over Y = z (rows x K, masked objective values)."""
    w, mask, z = (torch.as_tensor(v, dtype=torch.float64) for v in (w, mask, z))
    _, products = botorch_scalarization(w * mask, z.reshape(-1, w.numel()))
    K = w.numel()
    t0 = products(torch.zeros(1, K, dtype=torch.float64) * mask)[0]
    t1 = products(torch.ones(1, K, dtype=torch.float64) * mask)[0]
    return [(float(t1[k] - t0[k]), float(t0[k])) for k in range(K)]
