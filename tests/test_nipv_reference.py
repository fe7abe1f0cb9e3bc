"""tests/nipv_reference.py on the CPU: ``direct`` against the 40-digit truth of
tests/golden/nipv_truth.json (tests/golden/make_nipv_truth.py), ``schur_route`` against ``direct``,
and known answers of the negative integrated posterior variance.

Bound against the truth: 1e-10 relative.  The (n + q) x (n + q) system has 2-norm condition
<= (n + q) / noise = 8e4 on the truth states, so float64 holds its solution to about
8e4 * 2.2e-16 = 2e-11 relative; the values are O(1) combinations of those solutions."""
import json
import os

import numpy as np
import pytest
import torch

from tests import nipv_reference as nr

T = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "nipv_truth.json")))


def _coef():
    return [(w * s) ** 2 for w, s in zip(T["w"], T["ys"])]


@pytest.mark.parametrize("state", [0, 1])
@pytest.mark.parametrize("cand", range(5))
@pytest.mark.parametrize("route", [nr.direct, nr.schur_route], ids=["direct", "schur"])
def test_routes_match_truth(state, cand, route):
    st = T["states"][state]
    got = float(route(T["Xn"], T["P"], T["candidates"][cand], T["ls"], st["noise"], T["kinds"], _coef()))
    want = float(st["acq"][cand])
    assert len(st["acq"][cand].lstrip("-0.")) >= 39
    assert abs(got - want) <= 1e-10 * abs(want), (got, want)


def _state(seed, n, N, d, kinds, noise=1e-3):
    rng = np.random.default_rng(seed)
    B = len(kinds)
    return dict(Xn=rng.uniform(size=(n, d)), P=rng.uniform(size=(N, d)), ls=rng.uniform(0.3, 1.0, size=(B, d)),
                noise=[noise] * B, kinds=kinds, coef=list(rng.uniform(0.2, 2.0, size=B)))


def _acq(route, s, Xc):
    return float(route(s["Xn"], s["P"], Xc, s["ls"], s["noise"], s["kinds"], s["coef"]))


def test_schur_route_matches_direct_with_gradients():
    s = _state(1, 40, 33, 3, [nr.RBF, nr.MATERN25, nr.MATERN15], noise=1e-4)
    X = np.random.default_rng(2).uniform(size=(4, 3, 3))
    lo, hi = np.array([-1.0, 0.0, 2.0]), np.array([1.0, 0.5, 4.0])
    Xr = lo + (hi - lo) * X
    Pr = lo + (hi - lo) * s["P"]
    gout = np.array([1.0, -2.0, 0.5, 3.0])
    args = (s["Xn"], Pr, Xr, s["ls"], s["noise"], s["kinds"], s["coef"], lo, hi)
    v0, g0 = nr.batch(nr.direct, *args, gout=gout)
    v1, g1 = nr.batch(nr.schur_route, *args, gout=gout)
    assert nr.value_error(v1, v0) <= 1e-11
    assert nr.row_error(g1, g0) <= 1e-9


def test_far_candidate_changes_nothing():
    """A candidate far from everything: C = 0, so acq = - sum_j coef_j v0_j, the variance integrated
    without the candidate."""
    s = _state(3, 12, 9, 2, [nr.RBF, nr.MATERN25])
    far = np.array([[400.0, -300.0]])
    want = 0.0
    for j, kind in enumerate(s["kinds"]):
        Xn, P, ls = (torch.tensor(s[k]) for k in ("Xn", "P", "ls"))
        K = nr.kernel(Xn, Xn, ls[j], kind) + s["noise"][j] * torch.eye(12, dtype=torch.float64)
        kp = nr.kernel(Xn, P, ls[j], kind)
        var = 1.0 - (kp * torch.linalg.solve(K, kp)).sum(0)
        want -= s["coef"][j] * float(var.mean())
    for route in (nr.direct, nr.schur_route):
        assert _acq(route, s, far) == pytest.approx(want, rel=1e-12)


@pytest.mark.parametrize("kind", [nr.RBF, nr.MATERN25])
def test_one_point_at_the_integration_point(kind):
    """N = 1, q = 1, x = p: observing p with noise s2 leaves var = v s2 / (v + s2), v the prior
    posterior variance at p."""
    s = _state(4, 7, 1, 2, [kind], noise=1e-2)
    Xn, P, ls = (torch.tensor(s[k]) for k in ("Xn", "P", "ls"))
    K = nr.kernel(Xn, Xn, ls[0], kind) + 1e-2 * torch.eye(7, dtype=torch.float64)
    kp = nr.kernel(Xn, P, ls[0], kind)
    v = float(1.0 - (kp * torch.linalg.solve(K, kp)).sum())
    want = -s["coef"][0] * v * 1e-2 / (v + 1e-2)
    for route in (nr.direct, nr.schur_route):
        assert _acq(route, s, s["P"]) == pytest.approx(want, rel=1e-11)


def test_more_points_never_hurt_and_order_does_not_matter():
    s = _state(5, 15, 20, 3, [nr.MATERN25, nr.RBF])
    X = np.random.default_rng(6).uniform(size=(4, 3))
    for route in (nr.direct, nr.schur_route):
        vals = [_acq(route, s, X[:k]) for k in range(1, 5)]
        assert all(b >= a for a, b in zip(vals, vals[1:])), vals     # acq(X u {x'}) >= acq(X)
        assert vals[-1] < 0.0
        perm = _acq(route, s, X[[2, 0, 3, 1]])
        assert perm == pytest.approx(vals[-1], rel=1e-12)
