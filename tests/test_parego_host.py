"""QparegoStrategy on the host — no device: the data model against golden vectors of the
REFERENCE's own data model (tests/golden/make_parego_golden.py: bofire/data_models/strategies/
predictives/qparego.py), preprocess_experiments_any_valid_output, the simplex weights and their
place in the seed order, and the (A, B) table of the device scan against the restatement of
BoTorch's Chebyshev scalarisation (tests/parego_reference.py) and a hand-computed answer."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch
from pydantic import TypeAdapter, ValidationError

import everest_amd.data_models as dm
from everest_amd import ops, strategies
from everest_amd.data_models.domain import AnyObjective
from tests import parego_reference as pr

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "parego_datamodels.json")))
_OBJ = TypeAdapter(AnyObjective)
_ANY = TypeAdapter(dm.AnyStrategy)


def _domain(objectives):
    """The maker's domain: inputs x1, x2 in [0, 1], outputs y0, y1, ... with the given objectives."""
    inputs = dm.Inputs(features=[dm.ContinuousInput(key=k, bounds=(0, 1)) for k in ("x1", "x2")])
    feats = [dm.ContinuousOutput(key=f"y{i}", objective=o) for i, o in enumerate(objectives)]
    return dm.Domain(inputs=inputs, outputs=dm.Outputs(features=feats))


def _objectives(dumps):
    return [None if d is None else _OBJ.validate_python(d) for d in dumps]


def _case(name):
    return _objectives(next(v for v in G["validators"] if v["name"] == name)["objectives"])


# ---------------------------------------------------------------------------------------
# data model
# ---------------------------------------------------------------------------------------
def test_default_dumps_match_reference():
    two = _case("min_max")
    built = {"QparegoStrategy": dm.QparegoStrategy(domain=_domain(two)),
             "QparegoStrategy_qLogEI": dm.QparegoStrategy(domain=_domain(two), seed=7,
                                                          acquisition_function=dm.qLogEI(n_mc_samples=128))}
    for name, s in built.items():
        want, got = G["defaults"][name], json.loads(s.model_dump_json())
        shared = set(got) & set(want)
        assert {"type", "acquisition_function", "num_restarts", "num_raw_samples", "maxiter", "batch_limit", "seed",
                "categorical_method"} <= shared, name
        for k in sorted(shared):
            assert got[k] == want[k], (name, k)
    assert isinstance(built["QparegoStrategy"].acquisition_function, dm.qNEI)
    with pytest.raises(ValidationError):
        dm.QparegoStrategy(domain=_domain(two), acquisition_function=dm.qNEHVI())


@pytest.mark.parametrize("case", G["validators"], ids=lambda c: c["name"])
def test_domain_validators_match_reference(case):
    dom = _domain(_objectives(case["objectives"]))
    if case["QparegoStrategy"]:
        assert dm.QparegoStrategy(domain=dom).type == "QparegoStrategy"
    else:
        with pytest.raises(ValidationError):
            dm.QparegoStrategy(domain=dom)


def test_json_round_trip_and_strategy_map():
    s = dm.QparegoStrategy(domain=_domain(_case("min_max_all_constrained_kinds")), seed=5,
                           acquisition_function=dm.qLogNEI(prune_baseline=False))
    back = _ANY.validate_json(s.model_dump_json())
    assert type(back) is dm.QparegoStrategy and back.model_dump() == s.model_dump()
    assert strategies.STRATEGY_MAP[dm.QparegoStrategy] is strategies.QparegoStrategy
    assert type(strategies.map(s)) is strategies.QparegoStrategy


def test_preprocess_experiments_any_valid_output():
    outputs = _domain(_case("min_max")).outputs
    nan = np.nan
    df = pd.DataFrame({"x1": np.arange(6.0), "y0": [1.0, nan, 3.0, nan, 5.0, 6.0], "y1": [1.0, 2.0, nan, nan, 5.0, 6.0],
                       "valid_y0": [1, 1, 1, 1, 0, 0], "valid_y1": [1, 1, 1, 1, 0, 1]}, index=list("abcdef"))
    # a: both, b: y1 only, c: y0 only, d: none observed, e: both invalid, f: y1 valid
    got = outputs.preprocess_experiments_any_valid_output(df)
    assert list(got.index) == ["a", "b", "c", "f"]
    assert got.equals(df.loc[["a", "b", "c", "f"]])
    assert list(outputs.preprocess_experiments_all_valid_outputs(df).index) == ["a"]


# ---------------------------------------------------------------------------------------
# weights, table, utility
# ---------------------------------------------------------------------------------------
def _host_strategy(objectives, preds: np.ndarray, seed=3, weights=None, af=None):
    """A QparegoStrategy whose model is replaced by fixed posterior means (rows x outputs): the
    host derivation (_parego_spec, the seed draws) runs without a device."""
    dom = _domain(objectives)
    kw = {} if af is None else {"acquisition_function": af}
    s = strategies.map(dm.QparegoStrategy(domain=dom, seed=seed, **kw), weights=weights)
    keys = dom.outputs.get_keys()
    n = preds.shape[0]
    exp = pd.DataFrame({"x1": np.linspace(0.1, 0.9, n), "x2": np.linspace(0.9, 0.1, n)})
    for j, k in enumerate(keys):
        exp[k], exp[f"valid_{k}"] = preds[:, j], 1
    s._experiments = exp
    s.is_fitted = True
    s.model = SimpleNamespace(output_keys=list(keys))
    s.predict = lambda df: pd.DataFrame({f"{k}_pred": preds[:len(df), j] for j, k in enumerate(keys)}, index=df.index)
    return s


def test_simplex_weights_and_seed_order():
    for K in (2, 3, 5):
        for seed in (1, 2, 3):
            w = strategies.sample_simplex_weights(K, torch.Generator().manual_seed(seed))
            assert w.shape == (K,) and (w >= 0).all() and abs(w.sum() - 1.0) < 1e-15
    objectives = [dm.MinimizeObjective(w=1.0), dm.MaximizeObjective(w=1.0),
                  dm.CloseToTargetObjective(w=1.0, target_value=0.4, exponent=2.0)]
    preds = np.random.default_rng(0).normal(size=(6, 3))
    for af, nseeds in ((dm.qNEI(), 2), (dm.qNEI(prune_baseline=False), 1), (dm.qLogEI(), 1)):
        s = _host_strategy(objectives, preds, seed=11, af=af)
        spec = s._parego_spec()
        seeds = [s._draw_acqf_seeds() for _ in range(2)]
        gen = torch.Generator().manual_seed(11)            # the strategy's stream, replayed by hand
        r = torch.sort(torch.rand(2, dtype=torch.float64, generator=gen)).values
        want_w = np.diff(np.concatenate([[0.0], r.numpy(), [1.0]]))
        assert np.array_equal(s.last_weights, want_w)       # the weights are the FIRST draw
        want = [int(torch.randint(0, 1000000, (1,), generator=gen).item()) for _ in range(2 * nseeds)]
        if isinstance(af, dm.qNEI):                         # (prune seed | 0 when not pruning, sampler seed)
            assert all(len(sd) == 2 and (af.prune_baseline or sd[0] == 0) for sd in seeds)
            drawn = [x for sd in seeds for x in (sd if af.prune_baseline else sd[1:])]
        else:
            drawn = [x for sd in seeds for x in sd]
        assert drawn == want, (af, seeds, want)
        assert spec.alpha == 0.05 and len(spec.terms) == 3
    # the hook overrides the draw and consumes nothing
    s = _host_strategy(objectives, preds, seed=11, weights=[0.2, 0.3, 0.5])
    s._parego_spec()
    assert np.array_equal(s.last_weights, [0.2, 0.3, 0.5])
    assert s.gen.get_state().equal(torch.Generator().manual_seed(11).get_state())


@pytest.mark.parametrize("n_rows", [1, 7])
def test_table_matches_botorch_form(n_rows):
    """Mixed Maximize / Minimize / CloseToTarget (+ a sigmoid output that becomes a constraint)."""
    objectives = [dm.MaximizeObjective(w=1.0, bounds=(-1, 3)), dm.MinimizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5),
                  dm.MinimizeObjective(w=1.0), dm.CloseToTargetObjective(w=1.0, target_value=0.4, exponent=2.0)]
    rng = np.random.default_rng(n_rows)
    preds = rng.normal(size=(n_rows, 4))
    w = np.array([0.5, 0.2, 0.3])
    s = _host_strategy(objectives, preds, weights=w)
    spec = s._parego_spec()
    keys = ["y0", "y2", "y3"]
    assert [t[0] for t in spec.terms] == [0, 2, 3]
    assert [t[1] for t in spec.terms] == [ops.OBJ_AFFINE, ops.OBJ_AFFINE, ops.OBJ_CLOSE_TO_TARGET]
    assert spec.constraints == [(1, 1.0, 0.5, 0.5)]          # present because a sigmoid output exists
    mask = strategies.get_ref_point_mask(s.domain)
    assert mask.tolist() == [1.0, -1.0, -1.0]
    g = np.stack([np.asarray(s.domain.outputs.get_by_key(k).objective(preds[:, j]), dtype=np.float64)
                  for k, j in zip(keys, (0, 2, 3))], -1)
    want = pr.terms_from_botorch(w, mask, g * mask)
    for (_, _, _, _, A, B), (wa, wb) in zip(spec.terms, want):
        assert A == pytest.approx(wa, rel=1e-12, abs=1e-14) and B == pytest.approx(wb, rel=1e-12, abs=1e-14)
    # the whole utility against BoTorch's callable on fresh model outputs
    Y = rng.normal(size=(50, 4))
    gY = np.stack([np.asarray(s.domain.outputs.get_by_key(k).objective(Y[:, j]), dtype=np.float64)
                   for k, j in zip(keys, (0, 2, 3))], -1)
    obj, _ = pr.botorch_scalarization(torch.tensor(w * mask), torch.tensor(g * mask))
    np.testing.assert_allclose(spec.utility(Y), obj(torch.tensor(gY * mask)).numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(spec.utility(torch.tensor(Y)).numpy(), spec.utility(Y), rtol=0, atol=1e-15)
    cheb = pr.Chebyshev(spec.terms, spec.alpha)
    np.testing.assert_allclose(cheb(torch.tensor(Y)).numpy(), spec.utility(Y), rtol=1e-13, atol=1e-14)
    # without the sigmoid output no constraint is derived
    s2 = _host_strategy([objectives[0], objectives[2], objectives[3]], preds[:, [0, 2, 3]], weights=w)
    assert s2._parego_spec().constraints == []


def test_known_answer():
    """weights (0.25, 0.75); objective 0 maximised over [0, 2], objective 1 minimised over [1, 3]."""
    # masked objective values z = mask * g: a minimised output's z is the output itself
    ab = strategies.chebyshev_terms([0.25, 0.75], [1.0, -1.0], [[0.0, 1.0], [2.0, 3.0]], ["a", "b"])
    assert ab == [(0.125, 0.0), (0.375, 1.125)]
    spec = ops.ParegoSpec(2, [(0, ops.OBJ_AFFINE, 1.0, 0.0, *ab[0]), (1, ops.OBJ_AFFINE, -1.0, 0.0, *ab[1])], 0.05)
    # g = (1, -2): model outputs y = (1, 2); t = (0.125, 0.375), u = 0.125 + 0.05 * 0.5
    assert float(spec.utility(np.array([1.0, 2.0]))) == 0.15
    assert float(spec.utility(torch.tensor([1.0, 2.0], dtype=torch.float64))) == 0.15


def test_zero_range_and_bad_weights_raise():
    with pytest.raises(ValueError, match="`b`"):
        strategies.chebyshev_terms([0.25, 0.75], [1.0, -1.0], [[0.0, -3.0], [2.0, -3.0]], ["a", "b"])
    with pytest.raises(ValueError, match="not positive"):
        strategies.chebyshev_terms([0.0, 1.0], [1.0, -1.0], [[0.0, -3.0], [2.0, -1.0]], ["a", "b"])
    # one row: hi = lo + 1, never a zero range
    assert strategies.chebyshev_terms([0.5, 0.5], [1.0, 1.0], [[2.0, 3.0]], ["a", "b"]) == [(0.5, -1.0), (0.5, -1.5)]
    objectives = [dm.MinimizeObjective(w=1.0), dm.MaximizeObjective(w=1.0)]
    preds = np.array([[1.0, 2.0], [1.0, 3.0], [1.0, 4.0]])
    with pytest.raises(ValueError, match="y0"):
        _host_strategy(objectives, preds)._parego_spec()
    with pytest.raises(ValueError, match="expected 2"):
        _host_strategy(objectives, preds, weights=[1.0])._parego_spec()


def test_exact_tie_takes_the_first_term():
    """t_0 == t_1 exactly: the value by hand, and the first arg-min rule of the backward."""
    spec = ops.ParegoSpec(3, [(0, ops.OBJ_AFFINE, 1.0, 0.0, 0.5, 0.25), (2, ops.OBJ_AFFINE, 2.0, 0.0, 0.25, 0.25),
                              (1, ops.OBJ_AFFINE, 1.0, 0.0, 1.0, 0.0)], 0.125)
    y = np.array([1.0, 4.0, 1.0])                   # t = (0.75, 0.75, 4.0)
    assert spec.term_values(y).tolist() == [0.75, 0.75, 4.0]
    assert float(spec.utility(y)) == 0.75 + 0.125 * 5.5
    assert spec.term_slopes(y).tolist() == [1.125, 0.125, 0.125]
    assert spec.term_slopes(np.array([1.0, 0.75, 1.0])).tolist() == [1.125, 0.125, 0.125]     # three-way tie
    assert spec.term_slopes(np.array([1.5, 4.0, 1.0])).tolist() == [0.125, 1.125, 0.125]


def test_spec_refuses_bad_tables():
    ok = [(0, ops.OBJ_AFFINE, 1.0, 0.0, 1.0, 0.0), (1, ops.OBJ_AFFINE, 1.0, 0.0, 1.0, 0.0)]
    with pytest.raises(ValueError):
        ops.ParegoSpec(2, ok[:1], 0.05)
    with pytest.raises(ValueError):
        ops.ParegoSpec(2, [ok[0], (1, ops.OBJ_SIGMOID, 1.0, 0.0, 1.0, 0.0)], 0.05)
    with pytest.raises(ValueError):
        ops.ParegoSpec(2, [ok[0], (1, ops.OBJ_AFFINE, 1.0, 0.0, 0.0, 0.0)], 0.05)
    with pytest.raises(ValueError):
        ops.ParegoSpec(2, ok, -0.1)
    with pytest.raises(ValueError):
        ops.ParegoSpec(2, [ok[0], (2, ops.OBJ_AFFINE, 1.0, 0.0, 1.0, 0.0)], 0.05)
