"""qParEGO on the MI355X: the full chain (QParegoNEI / QParegoLogNEI / QParegoLogEI
forward_backward through evr_qparego_eval) against tests/sobo_reference.py with the Chebyshev
utility of tests/parego_reference.py on the same base samples — baseline rows, incumbents, values
and gradients — torch autograd, and QparegoStrategy end to end.

State: 25 points, d = 4, DTLZ2(dim=4, num_objectives=3), Matern-2.5, S = 128, 12 candidates
(the experiments of test_gpu_sobo_constrained).  f_0 is Minimize, f_1 Maximize ("max") or
CloseToTarget ("ctt"), f_2 MinimizeSigmoid with tp at the median of the observed f_2: one output
is a constraint.  The scalarisation weights are fixed (0.35, 0.65).

Tolerances are the project's bars for this chain (tests/test_gpu_nei.py): plain values rtol
1e-6 / atol 1e-10 and gradients rtol 1e-5 / atol 1e-8; log variants 5e-6 absolute in log space
and 1e-3 relative gradients per candidate.  Every candidate is held."""
import numpy as np
import pandas as pd
import pytest
import torch

import everest_amd.data_models as dm
from everest_amd import ops, strategies
from everest_amd.acquisition import QParegoLogEI, QParegoLogNEI, QParegoNEI
from everest_amd.benchmarks import DTLZ2
from oracle import gp as ogp
from oracle import qnehvi as oq
from tests import parego_reference as pr
from tests import sobo_reference as sr
from tests.test_gpu_sobo_constrained import S, _experiments

pytestmark = pytest.mark.gpu

KEYS = ["f_0", "f_1", "f_2"]
WEIGHTS = (0.35, 0.65)


def _f1(variant, f1):
    if variant == "max":
        return dm.MaximizeObjective(w=1.0)
    return dm.CloseToTargetObjective(w=1.0, target_value=float(np.median(f1)), exponent=2.0)


def _domain(bench, exps, variant, constrained=True):
    f2 = dm.MinimizeSigmoidObjective(w=1.0, steepness=4.0, tp=float(np.median(exps["f_2"].values)))
    objs = [dm.MinimizeObjective(w=1.0), _f1(variant, exps["f_1"].values), f2 if constrained else None]
    return dm.Domain(inputs=bench.domain.inputs,
                     outputs=dm.Outputs(features=[dm.ContinuousOutput(key=k, objective=o) for k, o in zip(KEYS, objs)]))


def _strategy(dom, exps, seed=3, weights=WEIGHTS, **kw):
    specs = [dm.SingleTaskGPSurrogate(inputs=dom.inputs, outputs=dm.Outputs(features=[dom.outputs.get_by_key(k)]),
                                      kernel=dm.MaternKernel(nu=2.5)) for k in KEYS]
    s = strategies.map(dm.QparegoStrategy(domain=dom, seed=seed, surrogate_specs=dm.BotorchSurrogates(surrogates=specs),
                                          num_raw_samples=64, num_restarts=2, maxiter=100, **kw), weights=weights)
    s.tell(exps[dom.inputs.get_keys() + KEYS + [f"valid_{k}" for k in KEYS]])
    return s


@pytest.fixture(scope="module")
def state():
    bench = DTLZ2(dim=4, num_objectives=3)
    exps = _experiments(bench)
    s = _strategy(_domain(bench, exps, "max"), exps)
    assert list(s.model.output_keys) == KEYS
    models = []
    for sur in s.surrogates.surrogates:
        st = sur.state
        models.append(ogp.GPState(X=torch.tensor(st["X"]), y=torch.tensor((st["y"] - st["y_mean"]) / st["y_std"]),
                                  lengthscale=torch.tensor(st["lengthscale"]), noise=st["noise"],
                                  constant=st["constant"], y_mean=st["y_mean"], y_std=st["y_std"],
                                  kind=ogp.MATERN25))
    X_train, _ = s.get_acqf_input_tensors()
    z_prune = oq.base_samples(2048, X_train.shape[0], 3, 5)
    specs, kept = {}, {}
    for v in ("max", "ctt"):
        s.domain = _domain(bench, exps, v)             # the same fitted models, the variant's objectives
        spec = s._parego_spec()
        assert len(spec.terms) == 2 and len(spec.constraints) == 1 and spec.alpha == 0.05
        specs[v] = spec
        kept[v] = sr.prune_rows(models, torch.tensor(X_train), pr.Chebyshev(spec.terms, spec.alpha),
                                sr.constraints_of(spec.constraints), z_prune)
    s.domain = _domain(bench, exps, "max")
    return dict(s=s, models=models, X_train=X_train, z_prune=z_prune, specs=specs, kept=kept, bench=bench, exps=exps)


LOG_NAMES = ("QParegoLogNEI", "QParegoLogEI")
EI_NAMES = ("QParegoLogEI", "QParegoEI")


def _build(state, variant, name, npend, prune, rng):
    s, X_train, spec = state["s"], state["X_train"], state["specs"][variant]
    Xp = rng.uniform(size=(npend, 4)) if npend else None
    if name in EI_NAMES:
        return QParegoLogEI(s.model, X_train, spec, S=S, seed=9, X_pending_raw=Xp, log=name == "QParegoLogEI"), Xp
    cls = QParegoNEI if name == "QParegoNEI" else QParegoLogNEI
    return cls(s.model, s.model.X_raw, X_train, spec, S=S, sampler_seed=9, prune_baseline=prune,
               z_prune=state["z_prune"], X_pending_raw=Xp), Xp


def _restatement(state, variant, acqf, name, qq, Xp):
    models, spec = state["models"], state["specs"][variant]
    util, oc = pr.Chebyshev(spec.terms, spec.alpha), sr.constraints_of(spec.constraints)
    z_new = acqf._zq(qq).cpu().reshape(S, qq, 3)
    Xpt = None if Xp is None else torch.tensor(Xp)
    log = name in LOG_NAMES
    if name in EI_NAMES:
        X_train = torch.tensor(state["X_train"])
        best = sr.best_f(models, X_train, util, oc).reshape(1)
        return sr.SoboNEI(models, X_train.new_zeros(0, 4), util, oc, z_new.new_zeros(S, 0, 3), z_new, log=log,
                          best=best, X_pending=Xpt)
    Xb = torch.tensor(np.asarray(state["s"].model.X_raw)[acqf.base_rows])
    return sr.SoboNEI(models, Xb, util, oc, acqf.z_base_host(), z_new, log=log, X_pending=Xpt)


@pytest.mark.parametrize("q,npend", [(1, 0), (1, 2), (3, 0)])
@pytest.mark.parametrize("name,prune", [("QParegoNEI", True), ("QParegoNEI", False), ("QParegoLogNEI", True),
                                        ("QParegoLogEI", False), ("QParegoEI", False)])
@pytest.mark.parametrize("variant", ["max", "ctt"])
def test_full_chain_matches_restatement(state, variant, name, prune, q, npend):
    rng = np.random.default_rng(q * 10 + npend)
    acqf, Xp = _build(state, variant, name, npend, prune, rng)
    X_train = state["X_train"]
    nei = _restatement(state, variant, acqf, name, q + npend, Xp)
    if name not in EI_NAMES:
        want = state["kept"][variant].numpy() if prune else np.arange(X_train.shape[0])
        assert np.array_equal(np.sort(acqf.base_rows), want)
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
    if name not in LOG_NAMES:
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
    for variant, name, q, npend in (("max", "QParegoNEI", 2, 0), ("ctt", "QParegoLogNEI", 1, 1),
                                    ("max", "QParegoLogEI", 2, 1)):
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
        assert torch.allclose(x2.grad, dXw, rtol=1e-12, atol=1e-300), name
        a2, g2 = acqf.forward_backward(Xc)
        assert torch.equal(a2, acq) and torch.equal(g2, dX), name       # bitwise reproducible


def test_acquisitions_need_a_parego_spec(state):
    s = state["s"]
    sobo = ops.SoboSpec(3, [(0, ops.OBJ_AFFINE, 1.0, -1.0, 0.0, 0.0)])
    with pytest.raises(TypeError):
        QParegoLogEI(s.model, state["X_train"], sobo, S=S)
    with pytest.raises(TypeError):
        QParegoNEI(s.model, s.model.X_raw, state["X_train"], sobo, S=S)


# ---------------------------------------------------------------------------------------
# strategy
# ---------------------------------------------------------------------------------------
def test_ask_runs_the_acquisition_list(state):
    bench, exps = state["bench"], state["exps"]
    dom = _domain(bench, exps, "max")
    keys = dom.inputs.get_keys()
    s = _strategy(dom, exps, weights=None)
    gen0 = s.gen.get_state()
    pend = s.ask(1, add_pending=True)                       # the strategy's own pending candidate
    assert len(pend) == 1 and s.num_candidates == 1 and type(s.last_acqf) is QParegoNEI
    gen1 = s.gen.get_state()
    cand = s.ask(3)
    assert len(cand) == 3
    want_cols = keys + [f"{k}_{t}" for t in ("pred", "sd", "des") for k in KEYS]
    assert sorted(cand.columns) == sorted(want_cols)
    xv = cand[keys].values
    assert ((xv >= 0.0) & (xv <= 1.0)).all()
    w = s.last_weights
    assert w.shape == (2,) and (w > 0).all() and abs(w.sum() - 1.0) < 1e-15
    acqfs = s.last_acqfs
    assert len(acqfs) == 3 and s.last_acqf is acqfs[2] and all(type(a) is QParegoNEI for a in acqfs)
    # round 0 sees the strategy's pending candidate, round i > 0 only the i earlier winners
    assert np.array_equal(acqfs[0].X_pending.cpu().numpy(), pend[keys].values)
    for i in (1, 2):
        assert acqfs[i].n_pending == i
        assert np.array_equal(acqfs[i].X_pending.cpu().numpy(), xv[:i])
    assert all(a.spec is acqfs[0].spec for a in acqfs) and len(acqfs[0].spec.constraints) == 1
    vals = s.last_ask_stats.best_value
    assert len(vals) == 3 and np.isfinite(vals).all()
    for i, a in enumerate(acqfs):                           # each round's value is its acquisition at its winner
        v = float(a.forward(torch.tensor(xv[i:i + 1].reshape(1, 1, 4), device="cuda")).cpu()[0])
        assert abs(v - vals[i]) <= 1e-9 * max(1.0, abs(v))
    # calc_acquisition from the same generator state: acquisition 0 of that ask
    s.gen.set_state(gen1)
    got = s.calc_acquisition(cand[keys])
    assert np.array_equal(got, acqfs[0].forward(torch.tensor(xv.reshape(3, 1, 4), device="cuda")).cpu().numpy())
    # a fresh strategy with the same seed repeats both asks bit for bit
    s2 = _strategy(dom, exps, weights=None)
    assert s2.gen.get_state().equal(gen0)
    p2 = s2.ask(1, add_pending=True)
    c2 = s2.ask(3)
    assert np.array_equal(p2[keys].values, pend[keys].values) and np.array_equal(c2[keys].values, xv)
    assert np.array_equal(s2.last_weights, w)


@pytest.mark.parametrize("af", ["qLogNEI", "qLogEI", "qEI"])
def test_other_acquisitions_and_no_constraint(state, af):
    """Without a sigmoid / target output no constraint is derived; the other acquisition kinds."""
    bench, exps = state["bench"], state["exps"]
    dom = _domain(bench, exps, "ctt", constrained=False)
    s = _strategy(dom, exps, acquisition_function=getattr(dm, af)(n_mc_samples=128))
    cand = s.ask(2)
    assert len(cand) == 2
    a = s.last_acqf
    assert type(a) is (QParegoLogNEI if af == "qLogNEI" else QParegoLogEI) and a.log_acqf is (af != "qEI")
    assert a.spec.constraints == [] and [t[1] for t in a.spec.terms] == [ops.OBJ_AFFINE, ops.OBJ_CLOSE_TO_TARGET]
    assert a.n_pending == 1 and np.array_equal(a.X_pending.cpu().numpy(), cand[dom.inputs.get_keys()].values[:1])


def test_limit_on_the_joint_batch(state):
    s = state["s"]
    with pytest.raises(ValueError, match="12"):
        s.ask(13)
    s.set_candidates(pd.DataFrame(np.random.default_rng(0).uniform(size=(12, 4)), columns=s.domain.inputs.get_keys()))
    try:
        with pytest.raises(ValueError, match="12"):
            s.ask(1)
    finally:
        s.reset_candidates()


def test_exhaustive_categorical_domain():
    """Two category combinations: every round runs optimize_acqf_mixed (q = 1)."""
    inputs = dm.Inputs(features=[dm.ContinuousInput(key="x0", bounds=(0, 1)), dm.ContinuousInput(key="x1", bounds=(0, 1)),
                                 dm.CategoricalInput(key="c0", categories=["a", "b"])])
    outputs = dm.Outputs(features=[dm.ContinuousOutput(key="y0", objective=dm.MinimizeObjective(w=1.0)),
                                   dm.ContinuousOutput(key="y1", objective=dm.MaximizeObjective(w=1.0))])
    dom = dm.Domain(inputs=inputs, outputs=outputs)
    X = strategies.map(dm.RandomStrategy(domain=dom, seed=2)).ask(30)
    off = X["c0"].map({"a": 0.0, "b": 0.3})
    exps = pd.concat([X, pd.DataFrame({"y0": (X["x0"] - 0.3) ** 2 + (X["x1"] - 0.6) ** 2 + off,
                                       "y1": np.sin(3.0 * X["x0"]) + X["x1"] - off, "valid_y0": 1, "valid_y1": 1})],
                     axis=1)
    specs = [dm.SingleTaskGPSurrogate(inputs=dom.inputs, outputs=dm.Outputs(features=[outputs.get_by_key(k)]),
                                      kernel=dm.MaternKernel(nu=2.5)) for k in ("y0", "y1")]
    s = strategies.map(dm.QparegoStrategy(domain=dom, seed=4, surrogate_specs=dm.BotorchSurrogates(surrogates=specs),
                                          categorical_method="EXHAUSTIVE", num_raw_samples=64, num_restarts=2,
                                          maxiter=100, acquisition_function=dm.qNEI(n_mc_samples=128)))
    s.tell(exps)
    assert len(s.get_categorical_combinations()) == 2
    c = s.ask(2)
    assert len(c) == 2 and set(c["c0"]) <= {"a", "b"}
    Xt = s._transform(c)
    assert set(np.unique(Xt[:, 2:])) <= {0.0, 1.0}                  # exact one-hot
    assert len(s.last_ask_stats.mixed_values) == 2 and len(s.last_ask_stats.best_value) == 2
    assert s.last_acqfs[1].n_pending == 1 and np.array_equal(s.last_acqfs[1].X_pending.cpu().numpy(), Xt[:1])
