"""CPU restatement (torch float64, autograd-capable) of the multiplicative and
multiplicative-additive utilities — TEST INFRASTRUCTURE ONLY.

``Product`` is u = prod_k g_k ** w_k * (1 + sum_a g_a w_a) with the call signature of
``sobo_reference.Utility``, so ``sr.scan``, ``sr.SoboNEI``, ``sr.best_f`` and ``sr.prune_rows``
take it unchanged.  It is written in the reference's own form
(bofire/utils/torch_tools.py:662-675 and 794-804): ``val = val * c ** w`` in list order from
tensor(1.0), the bracket from tensor(1.0) by ``+ c * w``, then the product of the two.  ``**`` is
torch.pow(tensor, float), whose backward is w * pow(g, w - 1) (masked to 0 for w == 0 only), so
autograd gives the slopes of an exactly zero factor.

``dev_layout`` turns joint samples into the layout the scans take."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Sequence

import torch

from tests.sobo_reference import Utility


@dataclass
class Product:
    """factors / addends: (out, kind, w, p0, p1, p2) with the kinds of ``sobo_reference``."""
    factors: Sequence[tuple]
    addends: Sequence[tuple] = field(default_factory=tuple)

    def __call__(self, Y):
        additive_objective = torch.tensor(1.0, dtype=torch.float64)
        for o, k, w, p0, p1, p2 in self.addends:
            additive_objective = additive_objective + Utility.term(k, p0, p1, p2, Y[..., o]) * w
        multiplicative_objective = torch.tensor(1.0, dtype=torch.float64)
        for o, k, w, p0, p1, p2 in self.factors:
            multiplicative_objective = multiplicative_objective * Utility.term(k, p0, p1, p2, Y[..., o]) ** w
        return multiplicative_objective * additive_objective


def dev_layout(Y):
    """Joint samples S x b x q x m -> the scans' S x m x (b*q)."""
    S, b, q, m = Y.shape
    return Y.permute(0, 3, 1, 2).reshape(S, m, b * q).contiguous()
