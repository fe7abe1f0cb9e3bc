"""GPU: the single-objective strategies end to end on the mixed GP, on the domain of
tests/test_gpu_categorical.py (two continuous inputs, two categoricals, one forbidden level,
n = 30): SoboStrategy without surrogate_specs — the reference's default configuration for such a
domain — with qLogNEI, qLogEI, qEI and qUCB, an AdditiveSoboStrategy with two outputs and a
QparegoStrategy; and the refusals of what stays stationary-only."""
import numpy as np
import pandas as pd
import pytest
import torch

import everest_amd.data_models as dm
from everest_amd import strategies, surrogates
from everest_amd.gp import MixedGPBatch

pytestmark = pytest.mark.gpu


def _domain(n_out=1):
    cont = [dm.ContinuousInput(key="x0", bounds=(0, 1)), dm.ContinuousInput(key="x1", bounds=(0, 1))]
    cats = [dm.CategoricalInput(key="c0", categories=["a", "b", "c"]),
            dm.CategoricalInput(key="c1", categories=["u", "v", "w"], allowed=[True, False, True])]
    outs = [dm.ContinuousOutput(key="y", objective=dm.MinimizeObjective(w=1.0)),
            dm.ContinuousOutput(key="z", objective=dm.MaximizeObjective(w=1.0))][:n_out]
    return dm.Domain(inputs=dm.Inputs(features=cont + cats), outputs=dm.Outputs(features=outs))


def _exps(dom, n=30):
    X = strategies.map(dm.RandomStrategy(domain=dom, seed=2)).ask(n)
    off = {"a": 0.0, "b": 0.5, "c": -0.4, "u": 0.2, "v": 9.0, "w": -0.1}
    y = (X["x0"] - 0.3) ** 2 + (X["x1"] - 0.6) ** 2 + X["c0"].map(off) + X["c1"].map(off)
    cols = {"y": y, "valid_y": 1}
    if len(dom.outputs.features) > 1:
        cols.update(z=np.sin(3 * X["x0"]) + X["x1"] * X["c0"].map(off), valid_z=1)
    return pd.concat([X, pd.DataFrame(cols)], axis=1)


def _check_rows(s, c):
    for k in range(len(c)):
        assert c["c0"].iloc[k] in ("a", "b", "c") and c["c1"].iloc[k] in ("u", "w")    # never the forbidden one
    X = s._transform(c)
    assert set(np.unique(X[:, 2:])) <= {0.0, 1.0} and np.all(X[:, 2:5].sum(1) == 1) and np.all(X[:, 5:].sum(1) == 1)
    return X


@pytest.fixture(scope="module")
def fitted():
    """The frame and a stand-alone default mixed surrogate fitted on it (predict's yardstick)."""
    dom = _domain()
    exps = _exps(dom)
    alone = surrogates.map(dm.MixedSingleTaskGPSurrogate(inputs=dom.inputs, outputs=dom.outputs))
    alone.fit(exps)
    return dom, exps, alone


@pytest.mark.parametrize("af", [dm.qLogNEI(), dm.qLogEI(), dm.qEI(), dm.qUCB()], ids=lambda a: type(a).__name__)
def test_sobo_without_specs_runs_on_the_mixed_model(fitted, af):
    dom, exps, alone = fitted
    s = strategies.map(dm.SoboStrategy(domain=dom, acquisition_function=af, seed=4, num_raw_samples=64,
                                       num_restarts=2))
    assert [type(m) for m in s.surrogate_specs.mixed_surrogates] == [dm.MixedSingleTaskGPSurrogate]
    s.tell(exps)
    assert isinstance(s.model, MixedGPBatch)
    # predict: the stand-alone surrogate fitted on the same frame
    own, ref = s.predict(exps), alone.predict(exps)
    y_std = alone.state["y_std"]
    assert np.abs(own["y_pred"].values - ref["y_pred"].values).max() <= 1e-10 * y_std
    assert np.abs(own["y_sd"].values - ref["y_sd"].values).max() <= 1e-10 * y_std
    assert len(s.get_categorical_combinations()) == 6
    c = s.ask(1)
    X = _check_rows(s, c)
    st = s.last_ask_stats
    assert len(st.mixed_values) == 6 and st.best_value == max(st.mixed_values)
    v = float(s.last_acqf.forward(torch.as_tensor(X, dtype=torch.float64, device="cuda")).cpu()[0])
    assert abs(v - st.best_value) <= 1e-9 * max(1.0, abs(v))
    c2 = s.ask(2)
    assert len(c2) == 2
    X2 = _check_rows(s, c2)
    assert not np.allclose(X2[0], X2[1])
    st = s.last_ask_stats       # the sequential greedy's last round; best_value holds both rounds' values
    assert len(st.mixed_values) == 6 and len(st.best_value) == 2 and st.best_value[-1] == max(st.mixed_values)
    assert all(np.isfinite(st.best_value))


def test_additive_sobo_two_outputs(fitted):
    dom = _domain(2)
    exps = _exps(dom)
    s = strategies.map(dm.AdditiveSoboStrategy(domain=dom, seed=4, num_raw_samples=64, num_restarts=2))
    assert [type(m) for m in s.surrogate_specs.mixed_surrogates] == [dm.MixedSingleTaskGPSurrogate] * 2
    s.tell(exps)
    assert isinstance(s.model, MixedGPBatch) and s.model.B == 2
    _check_rows(s, s.ask(1))
    st = s.last_ask_stats
    assert len(st.mixed_values) == 6 and st.best_value == max(st.mixed_values)


def test_qparego(fitted):
    dom = _domain(2)
    s = strategies.map(dm.QparegoStrategy(domain=dom, seed=4, num_raw_samples=64, num_restarts=2))
    s.tell(_exps(dom))
    assert isinstance(s.model, MixedGPBatch) and s.model.B == 2
    _check_rows(s, s.ask(1))


def test_mixed_and_one_hot_specs_together_raise(fitted):
    dom = _domain(2)
    y, z = dom.outputs.features
    specs = dm.BotorchSurrogates(
        mixed_surrogates=[dm.MixedSingleTaskGPSurrogate(inputs=dom.inputs, outputs=dm.Outputs(features=[y]))],
        surrogates=[dm.SingleTaskGPSurrogate(inputs=dom.inputs, outputs=dm.Outputs(features=[z]))])
    s = strategies.map(dm.AdditiveSoboStrategy(domain=dom, seed=4, surrogate_specs=specs, num_raw_samples=64,
                                               num_restarts=2))
    with pytest.raises(NotImplementedError, match="together"):
        s.tell(_exps(dom))


def test_mixed_members_on_different_rows_raise(fitted):
    dom = _domain(2)
    exps = _exps(dom)
    exps.loc[exps.index[:3], "valid_z"] = 0
    s = strategies.map(dm.AdditiveSoboStrategy(domain=dom, seed=4, num_raw_samples=64, num_restarts=2))
    with pytest.raises(NotImplementedError, match="different row sets"):
        s.tell(exps)


def test_a_mixed_spec_over_a_subset_of_the_inputs_raises(fitted):
    """The chain splits candidate rows of the domain's layout with the surrogate's column map: a
    surrogate over other inputs than the domain's is refused, not read under the wrong map."""
    dom = _domain()
    sub = dm.Inputs(features=[f for f in dom.inputs.get().features if f.key != "x1"])
    specs = dm.BotorchSurrogates(mixed_surrogates=[dm.MixedSingleTaskGPSurrogate(inputs=sub, outputs=dom.outputs)])
    s = strategies.map(dm.SoboStrategy(domain=dom, seed=4, surrogate_specs=specs, num_raw_samples=64, num_restarts=2))
    with pytest.raises(NotImplementedError, match="subset or another order"):
        s.tell(_exps(dom))
