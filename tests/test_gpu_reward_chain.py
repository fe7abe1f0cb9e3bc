"""QSoboSR / QSoboUCB / QSoboPI on the MI355X: the full chain (forward_backward through
evr_qreward_eval) against tests/reward_reference.py on the same base samples — infeasible cost,
incumbent, values and gradients — and torch autograd through torch.ops.everest_amd.qreward_*.

State: 25 points, d = 4, DTLZ2(dim=4, num_objectives=2), Matern-2.5 (that of
tests/test_gpu_sobo_constrained.py, rebuilt here), S = 128, 12 candidates.  f_0 is Minimize
throughout; f_1 carries
  (a) MinimizeSigmoid with tp at the median of the observed f_1 (mixed feasibility),
  (b) a TargetObjective (two constraints on one output);
  (u) is the single-output model on f_0 alone with no constraint (m = 1, one affine term).

Tolerances are the project's bars for the plain variants of this chain (tests/test_gpu_nei.py):
values rtol 1e-6 / atol 1e-10, gradients rtol 1e-5 / atol 1e-8.  Every candidate is held."""
import numpy as np
import pytest
import torch

import everest_amd.data_models as dm
from everest_amd import ops, strategies
from everest_amd.benchmarks import DTLZ2
from oracle import gp as ogp
from tests import reward_reference as rr
from tests import sobo_reference as sr

pytestmark = pytest.mark.gpu

S = 128
MODES = {"SR": (rr.SR, {}), "UCB": (rr.UCB, {"beta": 0.2}), "PI": (rr.PI, {"tau": 1e-3})}


def _domain(bench, f1_objective=None):
    feats = [dm.ContinuousOutput(key="f_0", objective=dm.MinimizeObjective(w=1.0))]
    if f1_objective is not None:
        feats.append(dm.ContinuousOutput(key="f_1", objective=f1_objective))
    return dm.Domain(inputs=bench.domain.inputs, outputs=dm.Outputs(features=feats))


def _strategy(dom, exps):
    keys = dom.outputs.get_keys()
    specs = [dm.SingleTaskGPSurrogate(inputs=dom.inputs, outputs=dm.Outputs(features=[dom.outputs.get_by_key(k)]),
                                      kernel=dm.MaternKernel(nu=2.5)) for k in keys]
    s = strategies.map(dm.SoboStrategy(domain=dom, seed=3, surrogate_specs=dm.BotorchSurrogates(surrogates=specs),
                                       num_raw_samples=64, num_restarts=2))
    s.tell(exps[dom.inputs.get_keys() + keys + ["valid_" + k for k in keys]])
    return s


def _oracle_models(s):
    models = []
    for sur in s.surrogates.surrogates:
        st = sur.state
        models.append(ogp.GPState(X=torch.tensor(st["X"]), y=torch.tensor((st["y"] - st["y_mean"]) / st["y_std"]),
                                  lengthscale=torch.tensor(st["lengthscale"]), noise=st["noise"],
                                  constant=st["constant"], y_mean=st["y_mean"], y_std=st["y_std"],
                                  kind=ogp.MATERN25))
    return models


@pytest.fixture(scope="module")
def state():
    bench = DTLZ2(dim=4, num_objectives=2)
    rnd = strategies.map(dm.RandomStrategy(domain=bench.domain, seed=11))
    exps = bench.f(rnd.ask(25), return_complete=True)
    f1 = exps["f_1"].values
    objs = {"a": dm.MinimizeSigmoidObjective(w=1.0, steepness=4.0, tp=float(np.median(f1))),
            "b": dm.TargetObjective(w=1.0, target_value=float(np.median(f1)), tolerance=0.15, steepness=6.0)}
    s2 = _strategy(_domain(bench, objs["a"]), exps)
    s1 = _strategy(_domain(bench), exps)
    assert list(s2.model.output_keys) == ["f_0", "f_1"] and list(s1.model.output_keys) == ["f_0"]
    out = {}
    for v, obj in objs.items():
        terms, cons = strategies.sobo_objective_spec(_domain(bench, obj).outputs, ["f_0", "f_1"])
        assert len(terms) == 1 and len(cons) == (2 if v == "b" else 1)
        out[v] = dict(s=s2, models=_oracle_models(s2), terms=terms, cons=cons, m=2)
    terms, cons = strategies.sobo_objective_spec(_domain(bench).outputs, ["f_0"])
    assert terms == [(0, ops.OBJ_AFFINE, 1.0, -1.0, 0.0, 0.0)] and cons == []
    out["u"] = dict(s=s1, models=_oracle_models(s1), terms=terms, cons=cons, m=1)
    X_train, _ = s2.get_acqf_input_tensors()
    # the points of the infeasible cost: X_train and 128 more (the strategy draws them from a RandomStrategy)
    X_cost = np.concatenate([X_train, np.random.default_rng(2).uniform(size=(128, 4))], 0)
    for v, st in out.items():
        st["X_train"] = X_train
        util = sr.Utility(st["terms"])
        st["M_ref"] = rr.infeasible_cost(st["models"], torch.tensor(X_cost), util)
        mean, var = st["s"].model.posterior(torch.tensor(X_cost, device="cuda"))
        from everest_amd.acquisition import get_infeasible_cost
        st["M"] = get_infeasible_cost(ops.SoboSpec(st["m"], st["terms"], st["cons"]), mean, var)
    return out


def _build(st, mode_name, npend, rng):
    from everest_amd.acquisition import QSoboPI, QSoboSR, QSoboUCB

    spec = ops.SoboSpec(st["m"], st["terms"], st["cons"])
    Xp = rng.uniform(size=(npend, 4)) if npend else None
    gp, X_train = st["s"].model, st["X_train"]
    M = st["M"] if st["cons"] else 0.0
    if mode_name == "SR":
        return QSoboSR(gp, X_train, spec, S=S, seed=9, X_pending_raw=Xp, infeasible_cost=M), Xp
    if mode_name == "UCB":
        return QSoboUCB(gp, X_train, spec, beta=0.2, S=S, seed=9, X_pending_raw=Xp, infeasible_cost=M), Xp
    return QSoboPI(gp, X_train, spec, tau=1e-3, S=S, seed=9, X_pending_raw=Xp), Xp


def test_infeasible_cost_matches_restatement(state):
    for v, st in state.items():
        print(f"variant {v}: M device {st['M']:.12e}, restatement {st['M_ref']:.12e}")
        assert st["M"] >= 0.0
        assert np.isclose(st["M"], st["M_ref"], rtol=1e-6, atol=1e-10)
    assert state["a"]["M"] > 0.0          # f_0 >= 0 is minimised: u(mu - 6 sigma) goes below zero


@pytest.mark.parametrize("q,npend", [(1, 0), (3, 0), (2, 1)])
@pytest.mark.parametrize("mode_name", list(MODES))
@pytest.mark.parametrize("variant", ["a", "b", "u"])
def test_full_chain_matches_restatement(state, variant, mode_name, q, npend):
    st = state[variant]
    rng = np.random.default_rng(q * 10 + npend)
    acqf, Xp = _build(st, mode_name, npend, rng)
    mode, kw = MODES[mode_name]
    m, qq = st["m"], q + npend
    util, oc = sr.Utility(st["terms"]), sr.constraints_of(st["cons"])
    z_new = acqf._zq(qq).cpu().reshape(S, qq, m)
    best = None
    if mode == rr.PI:
        best = sr.best_f(st["models"], torch.tensor(st["X_train"]), util, oc).reshape(1)
        print(f"{mode_name} {variant}: best_f device {acqf.best_f:.12e}, restatement {float(best):.12e}")
        assert torch.allclose(acqf.best.cpu(), best, rtol=1e-6, atol=1e-10)
    assert acqf.supports_plan is False and acqf.log_acqf is False
    assert getattr(acqf, "nonnegative", True) is (mode == rr.PI)
    M = st["M"] if st["cons"] else 0.0      # checked against the restatement's own in the test above
    ref_acq = rr.Reward(st["models"], util, oc, z_new, mode, best_f=best, M=M,
                        X_pending=None if Xp is None else torch.tensor(Xp), **kw)
    Xc = rng.uniform(size=(12, q, 4))
    x = torch.tensor(Xc, requires_grad=True)
    ref = ref_acq.forward(x)
    ref.sum().backward()
    acq, dX = acqf.forward_backward(torch.tensor(Xc, device="cuda"))
    acq, dX, r, gr = acq.cpu(), dX.cpu().reshape(12, q, 4), ref.detach(), x.grad
    assert torch.isfinite(acq).all() and torch.isfinite(dX).all()
    assert torch.equal(acqf.forward(torch.tensor(Xc, device="cuda")).cpu(), acq)
    print(f"{mode_name} {variant} q={q} npend={npend}: max |d acq| {float((acq - r).abs().max()):.3e} "
          f"(acq in [{float(r.min()):.3e}, {float(r.max()):.3e}]), max |d grad| {float((dX - gr).abs().max()):.3e} "
          f"(max |grad| {float(gr.abs().max()):.3e})")
    assert torch.allclose(acq, r, rtol=1e-6, atol=1e-10)
    assert torch.allclose(dX, gr, rtol=1e-5, atol=1e-8)


def test_autograd_equals_forward_backward(state):
    rng = np.random.default_rng(4)
    for variant, mode_name, q, npend in (("a", "SR", 2, 0), ("b", "UCB", 1, 1), ("u", "UCB", 3, 0), ("a", "PI", 2, 1)):
        acqf, _ = _build(state[variant], mode_name, npend, rng)
        Xc = torch.tensor(rng.uniform(size=(7, q, 4)), device="cuda")
        acq, dX = acqf.forward_backward(Xc)
        x = Xc.clone().requires_grad_(True)
        out = acqf(x)
        out.sum().backward()
        assert torch.equal(out.detach(), acq) and torch.equal(x.grad, dX), mode_name
        w = torch.tensor(rng.uniform(0.5, 2.0, size=7), device="cuda")
        x2 = Xc.clone().requires_grad_(True)
        (acqf(x2) * w).sum().backward()
        assert torch.equal(x2.grad, dX * w.view(-1, 1, 1)), mode_name
        a2, g2 = acqf.forward_backward(Xc)
        assert torch.equal(a2, acq) and torch.equal(g2, dX), mode_name       # bitwise reproducible


def test_classes_refuse_bad_parameters(state):
    from everest_amd.acquisition import QSoboPI, QSoboSR, QSoboUCB

    st = state["a"]
    spec = ops.SoboSpec(2, st["terms"], st["cons"])
    gp, X_train = st["s"].model, st["X_train"]
    with pytest.raises(ValueError):
        QSoboUCB(gp, X_train, spec, beta=-0.1, S=S)
    with pytest.raises(ValueError):
        QSoboPI(gp, X_train, spec, tau=0.0, S=S)
    with pytest.raises(ValueError):
        QSoboSR(gp, X_train, spec, S=S, infeasible_cost=-1.0)
