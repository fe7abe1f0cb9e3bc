"""ActiveLearningStrategy end to end on the MI355X: tell / ask / calc_acquisition through
strategies.map, against the independent ``direct`` route of tests/nipv_reference.py on the
strategy's own integration points.

Domains: 2 continuous inputs, 1 output or 2 outputs with ``weights``, 8 told rows;
n_mc_samples = 64, num_restarts = 4, num_raw_samples = 64.  Values are held to the measured bound of
tests/test_gpu_nipv.py: max(8 e, 64 * 2.2e-16 * sum_j coef_j), e the CPU error of ``schur_route``
against ``direct`` on the same state."""
import numpy as np
import pandas as pd
import pytest
import torch

import everest_amd.data_models as dm
from everest_amd import strategies
from everest_amd.acquisition import QNegIntPosVar
from tests import nipv_reference as nr

pytestmark = pytest.mark.gpu

KEYS = ["x1", "x2"]
WEIGHTS = {"y0": 0.4, "y1": 1.7}


def _domain(n_out, constrained=False):
    inputs = dm.Inputs(features=[dm.ContinuousInput(key="x1", bounds=(-1.0, 2.0)),
                                 dm.ContinuousInput(key="x2", bounds=(0.0, 0.5))])
    outs = dm.Outputs(features=[dm.ContinuousOutput(key=f"y{i}", objective=dm.MaximizeObjective(w=1.0))
                                for i in range(n_out)])
    cons = []
    if constrained:     # x1 + 2 x2 <= 1.5
        cons = [dm.LinearInequalityConstraint(features=KEYS, coefficients=[1.0, 2.0], rhs=1.5)]
    return dm.Domain(inputs=inputs, outputs=outs, constraints=dm.Constraints(constraints=cons))


def _experiments(dom, n_out):
    X = strategies.map(dm.RandomStrategy(domain=dom, seed=17)).ask(8)[KEYS]
    X["y0"] = np.sin(3.0 * X["x1"]) + 4.0 * X["x2"] ** 2
    if n_out == 2:
        X["y1"] = 10.0 * np.cos(5.0 * X["x2"]) * X["x1"]
    for i in range(n_out):
        X[f"valid_y{i}"] = 1
    return X


def _strategy(n_out, constrained=False, seed=5, **kw):
    dom = _domain(n_out, constrained)
    af = dm.qNegIntPosVar(n_mc_samples=64, weights=WEIGHTS if n_out == 2 else None)
    s = strategies.map(dm.ActiveLearningStrategy(domain=dom, seed=seed, acquisition_function=af, num_restarts=4,
                                                 num_raw_samples=64), **kw)
    s.tell(_experiments(dom, n_out))
    return s


@pytest.fixture(scope="module")
def strat():
    return {1: _strategy(1), 2: _strategy(2)}


def _columns(n_out):
    return KEYS + [f"y{i}_{t}" for t in ("pred", "sd", "des") for i in range(n_out)]


def _host_model(s):
    """The fitted model's numbers on the host, for the CPU routes."""
    gp = s.model
    c = lambda t: t.cpu().numpy()  # noqa: E731
    w = np.ones(1) if gp.B == 1 else np.array([WEIGHTS[k] for k in s.model.output_keys])
    return dict(Xn=c(gp.Xn), ls=c(gp.ls), noise=c(gp.noise), kinds=list(gp.kinds), coef=(w * c(gp.ys)) ** 2,
                lo=c(gp.lo), hi=c(gp.hi))


def _routes(s, P, X3):
    m = _host_model(s)
    args = (m["Xn"], P, X3, m["ls"], m["noise"], m["kinds"], m["coef"], m["lo"], m["hi"])
    v_d, _ = nr.batch(nr.direct, *args, grad=False)
    v_s, _ = nr.batch(nr.schur_route, *args, grad=False)
    return v_d, nr.bounds(nr.value_error(v_s, v_d), 0.0, m["coef"])[0]


@pytest.mark.parametrize("n_out", [1, 2])
@pytest.mark.parametrize("q", [1, 2])
def test_ask_returns_the_reference_columns_and_beats_raw_samples(strat, n_out, q):
    s = strat[n_out]
    cand = s.ask(q)
    assert len(cand) == q and sorted(cand.columns) == sorted(_columns(n_out))
    acqf = s.last_acqf
    assert type(acqf) is QNegIntPosVar and acqf.n_pending == 0
    assert tuple(acqf.mc_points.shape) == (64, 2) and acqf.log_acqf is False and acqf.supports_plan is False
    assert acqf.nonnegative is False
    lo, hi = np.array([-1.0, 0.0]), np.array([2.0, 0.5])
    xv = cand[KEYS].values
    assert ((xv >= lo) & (xv <= hi)).all()
    # the returned batch scores at least what every raw sample of a 64-point Sobol set scores
    sob = torch.quasirandom.SobolEngine(2 * q, scramble=True, seed=1).draw(64).to(torch.float64).reshape(64, q, 2)
    raw = torch.as_tensor(lo) + torch.as_tensor(hi - lo) * sob
    vals = acqf.forward(raw.to(acqf.dev)).cpu().numpy()
    best = float(acqf.forward(torch.as_tensor(xv, device=acqf.dev).unsqueeze(0)).item())
    assert best == pytest.approx(float(np.ravel(s.last_ask_stats.best_value)[0]), rel=1e-9)
    print(f"active learning ask({q}), {n_out} outputs: candidate {best:.6e}, best raw sample {vals.max():.6e}")
    assert best >= vals.max()


@pytest.mark.parametrize("n_out", [1, 2])
def test_calc_acquisition_equals_direct(strat, n_out):
    s = strat[n_out]
    X = strategies.map(dm.RandomStrategy(domain=s.domain, seed=23)).ask(6)[KEYS]
    single = s.calc_acquisition(X)
    P = s.last_acqf.mc_points.cpu().numpy()
    v_d, tol = _routes(s, P, X.values[:, None, :])
    err = nr.value_error(single, v_d)
    print(f"active learning calc_acquisition, {n_out} outputs: dev_val={err:.3e} bound={tol:.3e}")
    assert single.shape == (6,) and err <= tol
    joint = s.calc_acquisition(X.iloc[:3], combined=True)
    v_j, tol_j = _routes(s, s.last_acqf.mc_points.cpu().numpy(), X.values[None, :3, :])
    assert joint.shape == (1,) and nr.value_error(joint, v_j) <= tol_j


def test_weights_follow_the_output_keys(strat):
    s = strat[2]
    s.calc_acquisition(pd.DataFrame([[0.0, 0.2]], columns=KEYS))
    a = s.last_acqf
    assert list(a.weights) == [WEIGHTS[k] for k in s.model.output_keys]          # by key, not normalised
    want = (torch.as_tensor(a.weights, device=a.dev) * s.model.ys) ** 2
    assert torch.allclose(a.coef, want, rtol=4 * nr.EPS, atol=0.0)
    assert strat[1]._output_weights() is None                                   # one output: no transform


def test_same_seed_gives_the_same_ask():
    a, b = _strategy(1, seed=9), _strategy(1, seed=9)
    ca, cb = a.ask(2), b.ask(2)
    assert np.array_equal(ca[KEYS].values, cb[KEYS].values)
    assert torch.equal(a.last_acqf.mc_points, b.last_acqf.mc_points)
    c = _strategy(1, seed=10)
    c.ask(2)
    assert not torch.equal(a.last_acqf.mc_points, c.last_acqf.mc_points)


def test_mc_points_hook_fixes_the_integration_points():
    P = np.random.default_rng(0).uniform([-1.0, 0.0], [2.0, 0.5], size=(7, 2))
    s = _strategy(1, mc_points=P)
    g0 = s.gen.get_state()
    s.calc_acquisition(pd.DataFrame([[0.5, 0.1]], columns=KEYS))
    assert np.array_equal(s.last_acqf.mc_points.cpu().numpy(), P)
    assert not s.gen.get_state().equal(g0)          # the seed is still the first draw


def test_linear_inequality_is_respected():
    s = _strategy(1, constrained=True)
    cand = s.ask(1)
    P = s.last_acqf.mc_points.cpu().numpy()
    assert P.shape == (64, 2) and (P[:, 0] + 2.0 * P[:, 1] <= 1.5 + 1e-9).all()
    x = cand[KEYS].values
    assert (x[:, 0] + 2.0 * x[:, 1] <= 1.5 + 1e-6).all()
    assert s.last_ask_stats is not None


def test_pending_candidates_enter_the_next_ask():
    s = _strategy(2)
    c1 = s.ask(1, add_pending=True)
    assert s.num_candidates == 1 and s.last_acqf.n_pending == 0
    c2 = s.ask(1, add_pending=True)
    assert s.last_acqf.n_pending == 1 and s.num_candidates == 2
    assert torch.equal(s.last_acqf.X_pending.cpu(), torch.as_tensor(c1[KEYS].values))
    assert np.abs(c2[KEYS].values - c1[KEYS].values).max() > 1e-3


def test_joint_batch_limit(strat):
    s = strat[1]
    with pytest.raises(ValueError, match="12"):
        s.ask(13)
    s.set_candidates(pd.DataFrame(np.random.default_rng(0).uniform([-1.0, 0.0], [2.0, 0.5], size=(10, 2)),
                                  columns=KEYS))
    try:
        with pytest.raises(ValueError, match="12"):
            s.ask(3)                                   # 3 new + 10 pending = 13
    finally:
        s.reset_candidates()
