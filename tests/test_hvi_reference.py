"""The scan-level HVI reference (tests/hvi_reference.py) against an evaluation that uses no
box decomposition at all — hypervolume by recursive slicing, HV(P + {y}) - HV(P) — and its
autograd gradient against a central difference, so that neither is taken on trust by the
GPU tests that compare the device scans with it."""
import numpy as np
import pytest
import torch

from oracle import multiobjective as omo
from tests import hvi_reference as hr

ROWS = (0, 3, 5, 7)     # improving random, dominating the front, on a cell bound (tie row), scattered random


def _front(kind, n, m, seed):
    if kind == "sphere":
        return hr.sphere(1, n, m, seed)[0]
    return hr.staircase(1, n, m, 0, m - 1, seed)[0]


@pytest.mark.parametrize("kind", ["sphere", "staircase"])
@pytest.mark.parametrize("n", [8, 12, 16])
@pytest.mark.parametrize("m", [2, 5, 6, 7, 8])
def test_hvi_cells_equals_slicing(m, n, kind):
    """1e-12 relative on the improvement and nothing on top: where the scattered random row is
    dominated, both sides are exactly 0 (slicing adds no slab for a dominated point).  Worst
    measured 3.7e-13 (m = 2, n = 16, sphere), every other case at most 3.9e-14."""
    front = _front(kind, n, m, seed=10 * m + n)
    ref = hr.REF * np.ones(m)
    Y, ties = hr.candidates(front, ref, 8, seed=m + n)
    assert ties == [4, 5]
    Y = Y[list(ROWS)]
    v, _ = hr.hvi_cells(front, ref, Y)
    worst = 0.0
    hv0 = omo.hv_slicing(front, ref)
    for c in range(len(ROWS)):
        sl = hr.hvi_slicing(front, ref, Y[c], hv0)
        tol = 1e-12 * abs(sl)
        worst = max(worst, abs(v[c].item() - sl) / max(abs(sl), 1e-300))
        assert abs(v[c].item() - sl) <= tol, (c, v[c].item(), sl)
    assert v[1] > 0 and v[0] > 0            # the dominating and the improving row do improve
    print(f"hvi_cells vs slicing m={m} n={n} {kind}: worst relative error {worst:.3e}")


def test_edge_rows_have_the_values_they_are_built_for():
    front = hr.sphere(1, 12, 4, seed=1)[0]
    ref = hr.REF * np.ones(4)
    Y, ties = hr.candidates(front, ref, 9, seed=2)
    v, g = hr.hvi_cells(front, ref, Y)
    assert v[1] == 0 and (g[1] == 0).all()                       # below ref in one objective
    assert ((Y[1] < ref).sum() == 1)
    assert v[2] == 0 and (g[2] == 0).all()                       # dominated
    assert (front >= Y[2]).all(1).any()
    assert (Y[3] > front).all() and v[3] > v[[0, 1, 2, 4, 5]].max()
    assert v[4] == 0 and (front == Y[4]).all(1).any()            # on a front point
    assert v[5] > 0 and (front == Y[5]).any()                    # on a cell bound
    # dominating row: HVI = volume of its box minus the front's hypervolume
    hv = omo.hv_slicing(front, ref)
    assert abs(v[3].item() - (np.prod(Y[3] - ref) - hv)) < 1e-13


@pytest.mark.parametrize("m,kind", [(3, "sphere"), (6, "sphere"), (8, "staircase")])
def test_hvi_cells_gradient_equals_central_difference(m, kind):
    """Autograd of the reference on two non-tie candidates against central differences of its
    own value (h = 1e-6: truncation 0 — the value is multilinear in y inside a cell
    arrangement — and rounding about 2^-53 HVI / h ~ 1e-10)."""
    front = _front(kind, 12, m, seed=3 + m)
    ref = hr.REF * np.ones(m)
    Y, _ = hr.candidates(front, ref, 8, seed=m)
    Y = Y[[0, 6]]
    cells = hr.cells_of(front, ref)
    v, g = hr.hvi_cells(front, ref, Y, cells)
    assert (v > 0).all()
    h = 1e-6
    for c in range(2):
        for j in range(m):
            e = np.zeros(m)
            e[j] = h
            vp, _ = hr.hvi_cells(front, ref, Y[c:c + 1] + e, cells)
            vm, _ = hr.hvi_cells(front, ref, Y[c:c + 1] - e, cells)
            fd = (vp.item() - vm.item()) / (2 * h)
            assert abs(fd - g[c, j].item()) <= 1e-8 * max(1.0, abs(fd)), (c, j, fd, g[c, j].item())


def test_reference_layout_and_builders():
    """Reference averages over samples in the (S, m, b) layout with dG divided by S; the
    builders give what they promise (all staircase points nondominated, padding dominated)."""
    S, n, m, b = 3, 10, 3, 9
    fr = hr.sphere(S, n, m, seed=4)
    ref = hr.REF * np.ones(m)
    Y, ties = hr.batch(fr, ref, b, seed=5)
    R = hr.Reference(fr, ref, Y)
    assert R.dG.shape == (S, m, b) and R.acq.shape == (b,)
    v1, g1 = hr.hvi_cells(fr[1], ref, Y[1])
    assert torch.equal(R.sval[1], v1) and torch.equal(R.dG[1], g1.T / S)
    assert torch.allclose(R.acq, R.sval.sum(0) / S, rtol=1e-15)
    gout = torch.linspace(0.5, 2.0, 7, dtype=torch.float64)
    assert torch.equal(R.grad(7, gout), R.dG[:, :, :7] * gout)
    assert (R.vterm <= R.sval + 1e-300).all() and (R.vterm[:, 3] > 0).all()
    st = hr.staircase(2, 40, 5, 1, 3, seed=6)
    nd = omo.is_non_dominated(torch.as_tensor(st))
    assert nd.all() and (st[:, :, [0, 2, 4]] == -0.5).all()
    pad = hr.with_dominated(fr, 50, seed=7)
    assert pad.shape == (S, 50, m) and np.array_equal(pad[:, :n], fr)
    nd = omo.is_non_dominated(torch.as_tensor(pad))
    assert not nd[:, n:].any()
    # padding leaves the Pareto set, hence the reference, unchanged
    v2, _ = hr.hvi_cells(pad[1], ref, Y[1])
    assert torch.equal(v1, v2)
