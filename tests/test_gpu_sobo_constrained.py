"""Output-constrained / scalarised single-objective acquisitions on the MI355X: the full chain
(QSoboNEI / QSoboLogNEI / QSoboLogEI forward_backward through evr_qsobo_eval) against
tests/sobo_reference.py on the same base samples — baseline rows, incumbents, values and
gradients — torch autograd, and SoboStrategy / AdditiveSoboStrategy end to end.

State: 25 points, d = 4, DTLZ2(dim=4, num_objectives=2), Matern-2.5 (test_gpu_nei._sobo_strategy
with both outputs kept), S = 128, 12 candidates.  f_0 is Minimize throughout; f_1 carries
  (a) MinimizeSigmoid with tp at the median of the observed f_1 (mixed feasibility),
  (b) a TargetObjective (two constraints on one output),
  (c) MinimizeSigmoid with tp below every observed value and every baseline draw: no sample has a
      feasible row, so the incumbent is the mean - 6 sigma fallback.

Tolerances are the project's bars for this chain (tests/test_gpu_nei.py): plain values rtol
1e-6 / atol 1e-10 and gradients rtol 1e-5 / atol 1e-8; log variants 5e-6 absolute in log space
and 1e-3 relative gradients per candidate.  Every candidate is held."""
import numpy as np
import pytest
import torch

import everest_amd.data_models as dm
from everest_amd import ops, strategies
from everest_amd.benchmarks import DTLZ2
from oracle import gp as ogp
from oracle import qnehvi as oq
from tests import sobo_reference as sr

pytestmark = pytest.mark.gpu

S = 128


def _domain(bench, f1_objective, f0_objective=None):
    f0 = f0_objective or dm.MinimizeObjective(w=1.0)
    return dm.Domain(inputs=bench.domain.inputs,
                     outputs=dm.Outputs(features=[dm.ContinuousOutput(key="f_0", objective=f0),
                                                  dm.ContinuousOutput(key="f_1", objective=f1_objective)]))


def _experiments(bench, seed=11):
    rnd = strategies.map(dm.RandomStrategy(domain=bench.domain, seed=seed))
    return bench.f(rnd.ask(25), return_complete=True)


def _strategy(cls, dom, exps, **kw):
    specs = [dm.SingleTaskGPSurrogate(inputs=dom.inputs, outputs=dm.Outputs(features=[dom.outputs.get_by_key(k)]),
                                      kernel=dm.MaternKernel(nu=2.5)) for k in ("f_0", "f_1")]
    s = strategies.map(cls(domain=dom, seed=3, surrogate_specs=dm.BotorchSurrogates(surrogates=specs),
                           num_raw_samples=64, num_restarts=2, **kw))
    s.tell(exps[dom.inputs.get_keys() + ["f_0", "f_1", "valid_f_0", "valid_f_1"]])
    return s


def _variants(f1):
    return {"a": dm.MinimizeSigmoidObjective(w=1.0, steepness=4.0, tp=float(np.median(f1))),
            "b": dm.TargetObjective(w=1.0, target_value=float(np.median(f1)), tolerance=0.15, steepness=6.0),
            "c": dm.MinimizeSigmoidObjective(w=1.0, steepness=2.0, tp=float(np.min(f1)) - 3.0)}


@pytest.fixture(scope="module")
def state():
    bench = DTLZ2(dim=4, num_objectives=2)
    exps = _experiments(bench)
    objs = _variants(exps["f_1"].values)
    s = _strategy(dm.SoboStrategy, _domain(bench, objs["a"]), exps)
    assert list(s.model.output_keys) == ["f_0", "f_1"]
    models = []
    for sur in s.surrogates.surrogates:
        st = sur.state
        models.append(ogp.GPState(X=torch.tensor(st["X"]), y=torch.tensor((st["y"] - st["y_mean"]) / st["y_std"]),
                                  lengthscale=torch.tensor(st["lengthscale"]), noise=st["noise"],
                                  constant=st["constant"], y_mean=st["y_mean"], y_std=st["y_std"],
                                  kind=ogp.MATERN25))
    X_train, _ = s.get_acqf_input_tensors()
    z_prune = oq.base_samples(2048, X_train.shape[0], 2, 5)
    specs, kept = {}, {}
    for v, obj in objs.items():
        terms, cons = strategies.sobo_objective_spec(_domain(bench, obj).outputs, ["f_0", "f_1"])
        assert len(terms) == 1 and len(cons) == (2 if v == "b" else 1)
        specs[v] = (terms, cons)
        kept[v] = sr.prune_rows(models, torch.tensor(X_train), sr.Utility(terms), sr.constraints_of(cons), z_prune)
    return dict(s=s, models=models, X_train=X_train, z_prune=z_prune, specs=specs, kept=kept, bench=bench, exps=exps)


def _build(state, variant, name, npend, prune, rng):
    from everest_amd.acquisition import QSoboLogEI, QSoboLogNEI, QSoboNEI

    s, X_train = state["s"], state["X_train"]
    spec = ops.SoboSpec(2, *state["specs"][variant])
    Xp = rng.uniform(size=(npend, 4)) if npend else None
    if name in ("QSoboLogEI", "QSoboEI"):
        return QSoboLogEI(s.model, X_train, spec, S=S, seed=9, X_pending_raw=Xp, log=name == "QSoboLogEI"), Xp
    cls = QSoboNEI if name == "QSoboNEI" else QSoboLogNEI
    return cls(s.model, s.model.X_raw, X_train, spec, S=S, sampler_seed=9, prune_baseline=prune,
               z_prune=state["z_prune"], X_pending_raw=Xp), Xp


def _restatement(state, variant, acqf, name, qq, Xp):
    models = state["models"]
    terms, cons = state["specs"][variant]
    util, oc = sr.Utility(terms), sr.constraints_of(cons)
    z_new = acqf._zq(qq).cpu().reshape(S, qq, 2)
    Xpt = None if Xp is None else torch.tensor(Xp)
    log = name in ("QSoboLogNEI", "QSoboLogEI")
    if name in ("QSoboLogEI", "QSoboEI"):
        X_train = torch.tensor(state["X_train"])
        best = sr.best_f(models, X_train, util, oc).reshape(1)
        return sr.SoboNEI(models, X_train.new_zeros(0, 4), util, oc, z_new.new_zeros(S, 0, 2), z_new, log=log,
                          best=best, X_pending=Xpt)
    Xb = torch.tensor(np.asarray(state["s"].model.X_raw)[acqf.base_rows])
    return sr.SoboNEI(models, Xb, util, oc, acqf.z_base_host(), z_new, log=log, X_pending=Xpt)


@pytest.mark.parametrize("q,npend", [(1, 0), (3, 0), (2, 1)])
@pytest.mark.parametrize("name,prune", [("QSoboNEI", True), ("QSoboNEI", False), ("QSoboLogNEI", True),
                                        ("QSoboLogNEI", False), ("QSoboLogEI", False), ("QSoboEI", False)])
@pytest.mark.parametrize("variant", ["a", "b", "c"])
def test_full_chain_matches_restatement(state, variant, name, prune, q, npend):
    rng = np.random.default_rng(q * 10 + npend)
    acqf, Xp = _build(state, variant, name, npend, prune, rng)
    X_train = state["X_train"]
    nei = _restatement(state, variant, acqf, name, q + npend, Xp)
    if name in ("QSoboNEI", "QSoboLogNEI"):
        want = state["kept"][variant].numpy() if prune else np.arange(X_train.shape[0])
        assert np.array_equal(np.sort(acqf.base_rows), want)
        Yb = nei.orc.base_obj
        feas_rows = sr._feasible(nei.cons, Yb).any(-1)
        if variant == "c":
            assert not bool(feas_rows.any())          # the mean - 6 sigma fallback is what runs
            assert torch.isfinite(nei.best).all() and bool((nei.best == nei.best[0]).all())
    elif variant == "c":
        mean, _ = oq.joint_posterior(state["models"], torch.tensor(X_train))
        assert not bool(sr._feasible(nei.cons, mean).any())
    assert acqf.best.shape == nei.best.shape
    print(f"{name} {variant} prune={prune}: max |d best| {float((acqf.best.cpu() - nei.best).abs().max()):.3e}")
    assert torch.allclose(acqf.best.cpu(), nei.best, rtol=1e-6, atol=1e-10)
    Xc = rng.uniform(size=(12, q, 4))
    x = torch.tensor(Xc, requires_grad=True)
    ref = nei.forward(x)
    ref.sum().backward()
    acq, dX = acqf.forward_backward(torch.tensor(Xc, device="cuda"))
    acq, dX, r, gr = acq.cpu(), dX.cpu().reshape(12, q, 4), ref.detach(), x.grad
    assert torch.isfinite(acq).all() and torch.isfinite(dX).all()
    assert torch.equal(acqf.forward(torch.tensor(Xc, device="cuda")).cpu(), acq)
    if name in ("QSoboNEI", "QSoboEI"):
        print(f"{name} {variant} prune={prune} q={q} npend={npend}: max |d acq| {float((acq - r).abs().max()):.3e} "
              f"(max acq {float(r.max()):.3e}), max |d grad| {float((dX - gr).abs().max()):.3e}")
        assert torch.allclose(acq, r, rtol=1e-6, atol=1e-10)
        assert torch.allclose(dX, gr, rtol=1e-5, atol=1e-8)
    else:
        err = (acq - r).abs()
        row = (dX - gr).abs().amax((1, 2)) / gr.abs().amax((1, 2)).clamp_min(1e-300)
        print(f"{name} {variant} prune={prune} q={q} npend={npend}: max |d log| {float(err.max()):.3e}, "
              f"max relative gradient error {float(row.max()):.3e}")
        assert (err <= 5e-6).all(), err
        assert (row <= 1e-3).all(), row


def test_autograd_equals_forward_backward(state):
    rng = np.random.default_rng(4)
    for variant, name, q, npend in (("a", "QSoboNEI", 2, 0), ("b", "QSoboLogNEI", 1, 1), ("c", "QSoboLogEI", 2, 1)):
        acqf, _ = _build(state, variant, name, npend, True, rng)
        Xc = torch.tensor(rng.uniform(size=(7, q, 4)), device="cuda")
        acq, dX = acqf.forward_backward(Xc)
        x = Xc.clone().requires_grad_(True)
        out = acqf(x)
        out.sum().backward()
        assert torch.equal(out.detach(), acq) and torch.equal(x.grad, dX), name
        w = torch.tensor(rng.uniform(0.5, 2.0, size=7), device="cuda")
        x2 = Xc.clone().requires_grad_(True)
        (acqf(x2) * w).sum().backward()
        _, dXw = acqf.forward_backward(Xc, gout=w)
        # autograd scales the saved unit gradient by the incoming weights: one product, bit for bit
        assert torch.equal(x2.grad, dX * w.view(-1, 1, 1)), name
        # The gout route carries w through the whole backward chain instead, so it agrees with the
        # scaled unit gradient up to the chain's rounding only.  An element of these gradients is a
        # sum of ~1e3 sample terms that cancel to ~1e-3 of their absolute sum in the smallest
        # elements, so two orders of rounding differ by about 1e3 * 1e3 * 2^-53 ~ 1e-10 relative
        # there (seeds 4 to 11 give up to 1.9e-10; the former rtol 1e-12 held at this seed alone and
        # failed at 7 of the 8 others).  rtol 1e-9 with no absolute floor: a weight or a term wrong
        # by more than that fails
        assert torch.allclose(dXw, x2.grad, rtol=1e-9, atol=1e-300), name
        a2, g2 = acqf.forward_backward(Xc)
        assert torch.equal(a2, acq) and torch.equal(g2, dX), name       # bitwise reproducible


def test_models_on_different_row_sets_are_refused(state):
    from everest_amd.acquisition import QSoboLogEI

    gp = state["s"].model
    spec = ops.SoboSpec(2, *state["specs"]["a"])
    old = gp.mask
    gp.mask = torch.ones(2, gp.n, dtype=torch.float64, device=gp.device)
    try:
        with pytest.raises(NotImplementedError):
            QSoboLogEI(gp, state["X_train"], spec, S=S)
    finally:
        gp.mask = old


# ---------------------------------------------------------------------------------------
# strategies
# ---------------------------------------------------------------------------------------
def _run_strategy(s, dom, want):
    keys = dom.inputs.get_keys()

    def check(cand, q):
        assert len(cand) == q
        xv = cand[keys].values
        assert ((xv >= 0.0) & (xv <= 1.0)).all()
        acqf, st = s.last_acqf, s.last_ask_stats
        assert type(acqf) is want
        x0 = torch.tensor(np.asarray(st.init_X).reshape(2, q, 4), device="cuda")
        v0 = acqf.forward(x0).cpu()
        vc = acqf.forward(torch.tensor(s._transform(cand).reshape(1, q, 4), device="cuda")).cpu()
        assert torch.isfinite(vc).all() and float(vc[0]) >= float(v0.max()), (vc, v0)

    check(s.ask(1), 1)
    c2 = s.ask(2)
    check(c2, 2)
    c1 = s.ask(1, add_pending=True)
    check(c1, 1)
    assert s.candidates is not None and len(s.candidates) == 1
    c3 = s.ask(1)
    check(c3, 1)
    assert s.last_acqf.n_pending == 1 and not np.allclose(c1[keys].values, c3[keys].values)
    single = s.calc_acquisition(c2[keys])
    joint = s.calc_acquisition(c2[keys], combined=True)
    assert single.shape == (2,) and joint.shape == (1,) and np.isfinite(single).all() and np.isfinite(joint).all()


@pytest.mark.parametrize("af", [None, "qEI"])
def test_sobo_strategy_with_output_constraint(state, af):
    from everest_amd.acquisition import QSoboLogEI, QSoboLogNEI

    bench, exps = state["bench"], state["exps"]
    dom = _domain(bench, _variants(exps["f_1"].values)["a"])
    s = _strategy(dm.SoboStrategy, dom, exps, **({} if af is None else {"acquisition_function": getattr(dm, af)()}))
    _run_strategy(s, dom, QSoboLogNEI if af is None else QSoboLogEI)
    assert s.last_acqf.log_acqf is (af is None)
    assert s.last_acqf.spec.terms == [(0, ops.OBJ_AFFINE, 1.0, -1.0, 0.0, 0.0)] and len(s.last_acqf.spec.constraints) == 1


@pytest.mark.parametrize("use_output_constraints", [True, False])
def test_additive_sobo_strategy(state, use_output_constraints):
    from everest_amd.acquisition import QSoboLogNEI

    bench, exps = state["bench"], state["exps"]
    f1 = dm.MinimizeSigmoidObjective(w=0.5, steepness=4.0, tp=float(np.median(exps["f_1"].values)))
    dom = _domain(bench, f1)
    s = _strategy(dm.AdditiveSoboStrategy, dom, exps, use_output_constraints=use_output_constraints)
    _run_strategy(s, dom, QSoboLogNEI)
    spec = s.last_acqf.spec
    if use_output_constraints:
        assert [t[:3] for t in spec.terms] == [(0, ops.OBJ_AFFINE, 1.0)] and len(spec.constraints) == 1
    else:
        assert [t[:3] for t in spec.terms] == [(0, ops.OBJ_AFFINE, 1.0), (1, ops.OBJ_SIGMOID, 0.5)]
        assert spec.constraints == []


def test_single_output_unconstrained_domain_keeps_qlognei(state):
    from everest_amd.acquisition import QLogNEI

    bench, exps = state["bench"], state["exps"]
    dom = dm.Domain(inputs=bench.domain.inputs,
                    outputs=dm.Outputs(features=[dm.ContinuousOutput(key="f_0",
                                                                      objective=dm.MinimizeObjective(w=1.0))]))
    spec = dm.SingleTaskGPSurrogate(inputs=dom.inputs, outputs=dom.outputs, kernel=dm.MaternKernel(nu=2.5))
    s = strategies.map(dm.SoboStrategy(domain=dom, seed=3, surrogate_specs=dm.BotorchSurrogates(surrogates=[spec]),
                                       num_raw_samples=64, num_restarts=2))
    s.tell(exps[dom.inputs.get_keys() + ["f_0", "valid_f_0"]])
    assert len(s.ask(1)) == 1 and type(s.last_acqf) is QLogNEI
