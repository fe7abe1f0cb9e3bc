"""CPU reference of the q = 1 hypervolume improvement and its gradient — TEST
INFRASTRUCTURE ONLY — built from the oracle alone (oracle.multiobjective: Pareto filter,
local-upper-bound cells, clipped-length products, autograd), sharing nothing with the device
chain (box_device.hip, cells_kd.hip, hvi.hip), plus the front and candidate builders of the
scan-level tests.

Fronts are S x n x m in maximisation space with the reference point at -1.1 (objective
values in (-1.1, 0) dominate it)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from oracle import multiobjective as omo

REF = -1.1
N_EDGE = 5            # fixed edge rows of candidates(): rows 1..5
TIE_ROWS = (4, 5)     # of which these two sit on a gradient discontinuity (values only)


# ---------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------
def cells_of(front, ref) -> torch.Tensor:
    """Oracle cells (2 x C x m) of the region above ref not dominated by front (n x m)."""
    ref = torch.as_tensor(np.asarray(ref, dtype=np.float64))
    P = omo.pareto_above_ref(torch.as_tensor(np.asarray(front, dtype=np.float64)), ref)
    return omo.nondominated_cells(P, ref)


def hvi_cells(front, ref, Y, cells: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """front n x m, ref m, Y b x m -> (HVI (b), dHVI/dY (b x m)) in torch float64: the
    oracle's cells and clipped-length products, the gradient by autograd."""
    if cells is None:
        cells = cells_of(front, ref)
    y = torch.tensor(np.asarray(Y, dtype=np.float64), requires_grad=True)
    v = omo.hvi_from_cells(y, cells)
    v.sum().backward()
    return v.detach(), y.grad


def hvi_slicing(front, ref, y, hv_front: Optional[float] = None) -> float:
    """HV(front + {y}) - HV(front) by recursive slicing: no box decomposition involved
    (hv_front: HV(front) when the caller already has it)."""
    front = np.asarray(front, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(1, -1)
    if hv_front is None:
        hv_front = omo.hv_slicing(front, ref)
    return omo.hv_slicing(np.concatenate([front, y], 0), ref) - hv_front


def term_scales(cells: torch.Tensor, Y) -> Tuple[torch.Tensor, torch.Tensor]:
    """Largest single summand per candidate of the value sum (b) and of any gradient
    component's sum (b): the scale of the absolute part of the rounding bound."""
    lo, hi = cells[0], cells[1]
    y = torch.as_tensor(np.asarray(Y, dtype=np.float64))
    L = (torch.minimum(y.unsqueeze(-2), hi) - lo).clamp_min(0.0)       # b x C x m
    m = L.shape[-1]
    vt = L.prod(-1).amax(-1)
    gt = torch.zeros_like(vt)
    for j in range(m):
        keep = [k for k in range(m) if k != j]
        gt = torch.maximum(gt, (L[..., keep].prod(-1) if keep else torch.ones_like(vt).unsqueeze(-1)).amax(-1))
    return vt, gt


class Reference:
    """Sample-averaged reference of one state over its widest batch: fronts S x n x m,
    Y S x b x m (each sample's own candidates).  acq (b) = mean_s HVI_s; dG S x m x b =
    dHVI_s/dY / S (times gout[c] in grad()); batches b' < b are the first b' columns.
    ``c_max`` is the largest per-sample cell count, ``vterm`` / ``gterm`` (S x b) the
    largest summands (term_scales)."""

    def __init__(self, fronts: np.ndarray, ref, Y: np.ndarray):
        S, b, m = Y.shape
        self.S, self.b, self.m = S, b, m
        self.sval = torch.empty(S, b, dtype=torch.float64)
        self.dG = torch.empty(S, m, b, dtype=torch.float64)
        self.vterm = torch.empty(S, b, dtype=torch.float64)
        self.gterm = torch.empty(S, b, dtype=torch.float64)
        self.counts = []
        for s in range(S):
            cells = cells_of(fronts[s], ref)
            self.counts.append(int(cells.shape[1]))
            v, g = hvi_cells(fronts[s], ref, Y[s], cells)
            self.sval[s] = v
            self.dG[s] = g.T / S
            self.vterm[s], self.gterm[s] = term_scales(cells, Y[s])
        self.c_max = max(self.counts)
        self.acq = self.sval.mean(0)

    def grad(self, b: int, gout: Optional[torch.Tensor] = None) -> torch.Tensor:
        g = self.dG[:, :, :b]
        return g if gout is None else g * gout.reshape(1, 1, b)


def rounding_factor(c_max: int, m: int) -> float:
    """Every summand is a product of m nonnegative clipped lengths, so neither sum cancels:
    two correctly rounded evaluations of a sum of C such terms differ by at most about
    2 (C + m) 2^-53 relative; the tests allow twice that."""
    return 4.0 * (c_max + m) * 2.0 ** -53


# ---------------------------------------------------------------------------------------
# front builders
# ---------------------------------------------------------------------------------------
def sphere(S: int, n: int, m: int, seed: int) -> np.ndarray:
    """Points on a jittered positive orthant shell, negated (tests/test_gpu_box_device._front)."""
    rng = np.random.default_rng(seed)
    X = np.abs(rng.normal(size=(S, n, m)))
    X /= np.linalg.norm(X, axis=-1, keepdims=True)
    X *= 1 + 0.1 * rng.uniform(size=(S, n, 1))
    return -X


def staircase(S: int, n: int, m: int, j0: int, j1: int, seed: int) -> np.ndarray:
    """A two-objective trade-off in objectives j0, j1 (strictly increasing against strictly
    decreasing, irregular steps, rows shuffled), every other objective constant at -0.5: all
    n points are nondominated while the cell count stays O(n)."""
    rng = np.random.default_rng(seed)
    X = np.full((S, n, m), -0.5)
    for s in range(S):
        up = -1.0 + 0.9 * (np.arange(n) + rng.uniform(0.1, 0.9, size=n)) / n
        down = -1.0 + 0.9 * (np.arange(n) + rng.uniform(0.1, 0.9, size=n))[::-1] / n
        perm = rng.permutation(n)
        X[s, :, j0] = up[perm]
        X[s, :, j1] = down[perm]
    return X


def with_dominated(front: np.ndarray, n_total: int, seed: int = 0) -> np.ndarray:
    """front S x n x m padded to n_total rows with copies of front points shifted worse by
    0.05..0.5 in every objective (dominated; some fall below the reference point)."""
    S, n, m = front.shape
    rng = np.random.default_rng(seed)
    k = n_total - n
    if k <= 0:
        return front.copy()
    src = rng.integers(0, n, size=(S, k))
    pad = np.take_along_axis(front, src[:, :, None], axis=1) - rng.uniform(0.05, 0.5, size=(S, k, m))
    return np.concatenate([front, pad], axis=1)


# ---------------------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------------------
def candidates(front: np.ndarray, ref, b: int, seed: int) -> Tuple[np.ndarray, List[int]]:
    """b candidate objective rows for one sample's front (n x m), and the tie rows among them.

    Row 0 and every row from 6 on are random points around the front (even rows improve on a
    front point in every objective, odd rows scatter both ways).  Rows 1..5 are fixed edges:
      1  better than the whole front but below ref in exactly one objective   (HVI = 0)
      2  dominated by a front point                                           (HVI = 0)
      3  dominating the whole front
      4  equal to a front point                                               (tie row)
      5  better than two front points except for one coordinate exactly equal to a front
         point's coordinate, i.e. on a cell bound                             (tie row)
    On the tie rows the value is continuous and the gradient is not: they are held on values
    only (TIE_ROWS).  A batch shorter than 6 rows is a prefix of the same list."""
    front = np.asarray(front, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    n, m = front.shape
    rng = np.random.default_rng(seed)
    P = omo.pareto_above_ref(torch.as_tensor(front), torch.as_tensor(ref)).numpy()
    assert P.shape[0] >= 2, "candidates() needs two Pareto points above ref"
    top = front.max(0)
    rows = []
    for r in range(max(b, N_EDGE + 1)):
        p = P[rng.integers(P.shape[0])]
        z = rng.normal(size=m)
        rows.append(p + (0.02 + 0.1 * np.abs(z) if r % 2 == 0 else 0.12 * z))
    j = int(rng.integers(m))
    rows[1] = top + 0.05
    rows[1][j] = ref[j] - 0.01
    inner = P[np.argmax((P - ref).min(1))]
    rows[2] = inner - 0.5 * (inner - ref).min() * rng.uniform(0.1, 0.9, size=m)
    rows[3] = top + 0.05
    rows[4] = P[rng.integers(P.shape[0])].copy()
    ia, ib = rng.choice(P.shape[0], size=2, replace=False)
    rows[5] = np.maximum(P[ia], P[ib]) + 0.03
    rows[5][j] = P[ib][j]
    Y = np.stack(rows[:b], 0)
    return Y, [r for r in TIE_ROWS if r < b]


def batch(fronts: np.ndarray, ref, b: int, seed: int) -> Tuple[np.ndarray, List[int]]:
    """candidates() per sample: Y S x b x m and the tie rows (the same rows in every sample)."""
    out = [candidates(fronts[s], ref, b, seed + 7919 * s) for s in range(fronts.shape[0])]
    return np.stack([y for y, _ in out], 0), out[0][1]
