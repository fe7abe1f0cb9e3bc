"""MultiplicativeSoboStrategy and MultiplicativeAdditiveSoboStrategy on the host — no device: the
data models against golden vectors of the REFERENCE's own data models
(tests/golden/make_mult_sobo_golden.py: bofire/data_models/strategies/predictives/sobo.py:78-135),
``mult_objective_spec`` against the list / split the golden file restates from
bofire/utils/torch_tools.py:598-659 and 770-792, ``ops.MultSpec.utility`` against the restatement
in the reference's own form (tests/mult_reference.Product), hand-computed answers and the closed
forms of the slopes."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch
from pydantic import TypeAdapter, ValidationError

import everest_amd.data_models as dm
from everest_amd import ops, strategies
from everest_amd.data_models.domain import AnyObjective
from tests import mult_reference as mr
from tests import sobo_reference as sr

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "mult_sobo_datamodels.json")))
_OBJ = TypeAdapter(AnyObjective)
_ANY = TypeAdapter(dm.AnyStrategy)
MSG_TWO = "Multiplicative SOBO strategy requires at least 2 outputs with objectives. Consider SOBO strategy instead."
MSG_W = "Weight transformation to (1, inf) requires w>=1e-8 . Violated by feature y1."
A, C, SG, T = ops.OBJ_AFFINE, ops.OBJ_CLOSE_TO_TARGET, ops.OBJ_SIGMOID, ops.OBJ_TARGET


def _domain(objectives):
    """The maker's domain: inputs x1, x2 in [0, 1], outputs y0, y1, ... with the given objectives."""
    inputs = dm.Inputs(features=[dm.ContinuousInput(key=k, bounds=(0, 1)) for k in ("x1", "x2")])
    feats = [dm.ContinuousOutput(key=f"y{i}", objective=o) for i, o in enumerate(objectives)]
    return dm.Domain(inputs=inputs, outputs=dm.Outputs(features=feats))


def _objectives(dumps):
    return [None if d is None else _OBJ.validate_python(d) for d in dumps]


def _case(name):
    return next(c for c in G["cases"] if c["name"] == name)


def _experiments(n_out, n=6, seed=0):
    rng = np.random.default_rng(seed)
    exp = pd.DataFrame({"x1": np.linspace(0.1, 0.9, n), "x2": np.linspace(0.9, 0.1, n)})
    for j in range(n_out):
        exp[f"y{j}"], exp[f"valid_y{j}"] = rng.uniform(0.2, 1.5, size=n), 1
    return exp


# ---------------------------------------------------------------------------------------
# data models
# ---------------------------------------------------------------------------------------
def test_default_dumps_match_reference():
    two = _objectives(_case("two")["objectives"])
    built = {"MultiplicativeSoboStrategy": dm.MultiplicativeSoboStrategy(domain=_domain(two)),
             "MultiplicativeAdditiveSoboStrategy": dm.MultiplicativeAdditiveSoboStrategy(domain=_domain(two)),
             "MultiplicativeAdditiveSoboStrategy_y1": dm.MultiplicativeAdditiveSoboStrategy(
                 domain=_domain(two), seed=7, additive_features=["y1"], use_output_constraints=False)}
    for name, s in built.items():
        want, got = G["defaults"][name], json.loads(s.model_dump_json())
        shared = set(got) & set(want)
        need = {"type", "acquisition_function", "num_restarts", "num_raw_samples", "maxiter", "batch_limit", "seed",
                "categorical_method"}
        if name != "MultiplicativeSoboStrategy":
            need |= {"use_output_constraints", "additive_features"}
        assert need <= shared, name
        for k in sorted(shared):
            assert got[k] == want[k], (name, k)
    assert isinstance(built["MultiplicativeSoboStrategy"].acquisition_function, dm.qLogNEI)
    plain = built["MultiplicativeAdditiveSoboStrategy"]
    assert plain.use_output_constraints is True and plain.additive_features == []
    assert "use_output_constraints" not in json.loads(built["MultiplicativeSoboStrategy"].model_dump_json())


@pytest.mark.parametrize("case", G["cases"], ids=lambda c: c["name"])
def test_validators_match_reference(case):
    dom = _domain(_objectives(case["objectives"]))
    for cls, kw in ((dm.MultiplicativeSoboStrategy, {}),
                    (dm.MultiplicativeAdditiveSoboStrategy, {"additive_features": case["additive_features"]})):
        want = case[cls.__name__]
        if want["accepts"]:
            assert cls(domain=dom, **kw).type == cls.__name__
            continue
        with pytest.raises(ValueError) as err:
            cls(domain=dom, **kw)
        if want["is_value_error"]:
            # the reference's message is inside its pydantic report; the same sentence is inside ours
            sentence = next(m for m in (MSG_TWO, "is not an output feature of the domain.") if m in want["message"])
            assert isinstance(err.value, ValidationError) and sentence in str(err.value)
            for f in kw.get("additive_features", []):
                if f not in dom.outputs.get_keys():
                    assert f"Feature {f} is not an output feature of the domain." in str(err.value)
        else:
            # deviation: the reference's weight check dies with a TypeError while building its
            # pydantic.ValidationError; here it is the ValueError it means, with its message
            assert want["exception"] == "TypeError" and case["name"] == "tiny_weight"
            assert MSG_W in str(err.value)


def test_single_objective_is_accepted_by_the_additive_model_only():
    dom = _domain([dm.MaximizeObjective(w=1.0)])
    assert dm.MultiplicativeAdditiveSoboStrategy(domain=dom).type == "MultiplicativeAdditiveSoboStrategy"
    with pytest.raises(ValidationError, match="Multiplicative SOBO strategy requires at least 2 outputs"):
        dm.MultiplicativeSoboStrategy(domain=dom)


def test_json_round_trip_and_strategy_map():
    objs = _objectives(_case("all_kinds")["objectives"])
    for s, cls in ((dm.MultiplicativeSoboStrategy(domain=_domain(objs), seed=5,
                                                  acquisition_function=dm.qLogEI(n_mc_samples=64)),
                    strategies.MultiplicativeSoboStrategy),
                   (dm.MultiplicativeAdditiveSoboStrategy(domain=_domain(objs), seed=5, additive_features=["y4"]),
                    strategies.MultiplicativeAdditiveSoboStrategy)):
        back = _ANY.validate_json(s.model_dump_json())
        assert type(back) is type(s) and back.model_dump() == s.model_dump()
        assert strategies.MULT_STRATEGY_MAP[type(s)] is cls
        mapped = strategies.map(s)
        assert type(mapped) is cls and isinstance(mapped, strategies.SoboStrategy)
    assert strategies.map(back).additive_features == ["y4"]


# ---------------------------------------------------------------------------------------
# mult_objective_spec
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G["cases"], ids=lambda c: c["name"])
def test_mult_objective_spec_matches_reference_split(case):
    objs = _objectives(case["objectives"])
    outputs = _domain(objs).outputs
    keys = outputs.get_keys()
    exp = _experiments(len(objs))
    for want, kw in ((case["multiplicative"], dict(exclude_constraints=False)),
                     (case["multiplicative_additive"], dict(exclude_constraints=True,
                                                            additive_features=case["additive_features"]))):
        if want is None:                                   # every objective constrained: min([]) upstream
            with pytest.raises(ValueError, match="no objective is left"):
                strategies.mult_objective_spec(outputs, keys, exp, **kw)
            continue
        factors, addends = strategies.mult_objective_spec(outputs, keys, exp, **kw)
        assert [[keys[t[0]], t[2]] for t in factors] == want["factors"]         # the weights to the bit
        assert [[keys[t[0]], t[2]] for t in addends] == want["addends"]
        for t in factors + addends:                        # the callable: sobo_term's row
            obj = objs[int(keys[t[0]][1:])]
            x = exp[keys[t[0]]].values
            assert t == strategies.sobo_term(obj, t[0], t[2], x)
        assert min(t[2] for t in factors + addends) == 1.0                       # the smallest weight: exactly 1
        ops.MultSpec(len(keys), factors, addends)          # the device table takes it


def test_constrained_outputs_vanish_from_the_additive_utility():
    """A sigmoid output has no effect on MultiplicativeAdditive — named additive or not — and is a
    factor of Multiplicative; the remaining weights are normalised without it."""
    objs = _objectives(_case("sigmoid")["objectives"])
    outputs = _domain(objs).outputs
    keys = outputs.get_keys()
    for additive in (["y2"], ["y1", "y2"]):
        factors, addends = strategies.mult_objective_spec(outputs, keys, None, additive_features=additive,
                                                          exclude_constraints=True)
        assert [t[0] for t in factors] == [0] and [t[0] for t in addends] == [2]
        assert factors[0][2] == 1.0 and addends[0][2] == 0.9 / 0.6
    factors, addends = strategies.mult_objective_spec(outputs, keys, None)
    assert [t[:2] for t in factors] == [(0, A), (1, SG), (2, A)] and addends == []
    assert factors[1][2] == 1.0 and factors[2][2] == 0.9 / 0.2


def test_moving_sigmoid_factor_adapts_to_the_experiments():
    objs = [dm.MaximizeObjective(w=1.0), dm.MovingMaximizeSigmoidObjective(w=0.5, steepness=1.5, tp=-0.3)]
    outputs = _domain(objs).outputs
    keys = outputs.get_keys()
    for seed in (1, 2):
        exp = _experiments(2, seed=seed)
        exp.loc[0, "valid_y1"] = 0                          # an invalid row does not count
        exp.loc[0, "y1"] = 100.0
        factors, _ = strategies.mult_objective_spec(outputs, keys, exp)
        assert factors[1] == (1, SG, 1.0, 1.5, float(exp["y1"].values[1:].max()) - 0.3, 0.0)
        assert factors[0][2] == 2.0
    with pytest.raises(ValueError, match="experiments"):
        strategies.mult_objective_spec(outputs, keys, None)


# ---------------------------------------------------------------------------------------
# MultSpec
# ---------------------------------------------------------------------------------------
FACTORS = [(0, A, 1.0, 0.7, 0.2, 0.0), (1, SG, 2.5, 1.5, 0.2, 0.0), (2, T, 1.5, 2.0, 0.4, 1.5), (3, C, 2.0, 0.4, 1.5, 0.0)]
ADDENDS = [(4, SG, 0.5, -2.0, 0.3, 0.0), (1, A, 0.25, 1.1, -0.2, 0.0)]


@pytest.mark.parametrize("factors,addends", [(FACTORS, ADDENDS), (FACTORS[:2], []), ([], ADDENDS)])
def test_utility_matches_the_reference_form(factors, addends):
    spec, prod = ops.MultSpec(5, factors, addends), mr.Product(factors, addends)
    Y = torch.tensor(np.random.default_rng(1).uniform(-2.0, 2.0, size=(7, 3, 2, 5)))
    want = prod(Y)
    assert torch.isfinite(want).all()
    assert torch.allclose(spec.utility(Y), want, rtol=1e-13, atol=0.0)
    got = spec.utility(Y.numpy())
    assert isinstance(got, np.ndarray) and np.allclose(got, want.numpy(), rtol=1e-13, atol=0.0)
    assert spec.constraints == [] and spec.m_model == 5 and spec.terms == spec.factors + spec.addends
    assert bool(spec.feasible(Y).all()) and bool(spec.feasible(Y.numpy()).all())


def test_known_answer_and_closed_form_slopes():
    """Weights 0.25 / 0.5 / 1.0 normalise to 1 / 2 / 4; factors 0.5 and 2.0, addend 3.0:
    u = 0.5 * 2 ** 2 * (1 + 4 * 3) = 26."""
    case = _case("known_answer")
    outputs = _domain(_objectives(case["objectives"])).outputs
    factors, addends = strategies.mult_objective_spec(outputs, outputs.get_keys(), None, additive_features=["y2"],
                                                      exclude_constraints=True)
    assert [t[2] for t in factors] == [1.0, 2.0] and [t[2] for t in addends] == [4.0]
    spec, prod = ops.MultSpec(3, factors, addends), mr.Product(factors, addends)
    y = torch.tensor([0.5, 2.0, 3.0], dtype=torch.float64, requires_grad=True)      # Maximize: g = y
    u = prod(y)
    u.backward()
    assert float(u.detach()) == 26.0 and float(spec.utility(y.detach())) == 26.0 and float(spec.utility(y.detach().numpy())) == 26.0
    # d u / d g_k = w_k pow(g_k, w_k - 1) prod_{s != k} g_s ** w_s A;  d u / d g_a = w_a P
    assert y.grad.tolist() == [1.0 * 4.0 * 13.0, 2.0 * 2.0 * 0.5 * 13.0, 4.0 * 2.0]


def test_exact_zero_factor_slopes():
    """0 ** 1 * 3 ** 2 * (1 + 0.5 * 3): the slope with respect to the zero factor is the product of
    the others (22.5), every other slope 0; a zero factor of weight 2 has slope 0 itself."""
    factors, addends = [(0, A, 1.0, 1.0, 0.0, 0.0), (1, A, 2.0, 1.0, 0.0, 0.0)], [(2, A, 0.5, 1.0, 0.0, 0.0)]
    prod = mr.Product(factors, addends)
    y = torch.tensor([0.0, 3.0, 3.0], dtype=torch.float64, requires_grad=True)
    prod(y).backward()
    assert y.grad.tolist() == [22.5, 0.0, 0.0]
    y = torch.tensor([2.0, 0.0, 3.0], dtype=torch.float64, requires_grad=True)
    prod(y).backward()
    assert y.grad.tolist() == [0.0, 0.0, 0.0]


def test_pow_is_c_pow():
    neg = torch.tensor([-2.0], dtype=torch.float64)
    for w, want in ((1.5, float("nan")), (3.0, -8.0)):
        spec, prod = ops.MultSpec(1, [(0, A, w, 1.0, 0.0, 0.0)]), mr.Product([(0, A, w, 1.0, 0.0, 0.0)])
        with np.errstate(invalid="ignore"):
            got = [float(prod(neg)), float(spec.utility(neg)), float(spec.utility(neg.numpy()))]
        assert all(np.isnan(g) for g in got) if np.isnan(want) else got == [want] * 3


def test_multspec_refuses_bad_tables():
    row = (0, A, 1.0, 1.0, 0.0, 0.0)
    ops.MultSpec(2, [row]), ops.MultSpec(2, [], [row]), ops.MultSpec(2, [row] * 4, [row] * 4)
    bad = [dict(factors=[], addends=[]),                                     # no term
           dict(factors=[row] * 5, addends=[row] * 4),                       # nine terms
           dict(factors=[(2, A, 1.0, 1.0, 0.0, 0.0)]),                       # an output outside the model
           dict(factors=[row], addends=[(-1, A, 1.0, 1.0, 0.0, 0.0)]),
           dict(factors=[(0, 4, 1.0, 1.0, 0.0, 0.0)]),                       # an unknown kind
           dict(factors=[row], addends=[(0, -1, 1.0, 1.0, 0.0, 0.0)]),
           dict(factors=[(0, A, 0.99, 1.0, 0.0, 0.0)]),                      # a factor's weight below 1
           dict(factors=[(0, A, float("nan"), 1.0, 0.0, 0.0)]),
           dict(factors=[(0, A, float("inf"), 1.0, 0.0, 0.0)]),
           dict(factors=[row], addends=[(0, A, float("inf"), 1.0, 0.0, 0.0)])]
    for kw in bad:
        with pytest.raises(ValueError, match="mult scan"):
            ops.MultSpec(2, **{"addends": (), **kw})
    ops.MultSpec(2, [row], [(1, A, -0.5, 1.0, 0.0, 0.0)])                    # an addend's weight is free


# ---------------------------------------------------------------------------------------
# strategies
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("af", [dm.qSR(), dm.qUCB(), dm.qPI()], ids=lambda a: type(a).__name__)
def test_reward_acquisitions_are_refused(af):
    two = _objectives(_case("two")["objectives"])
    for data_model in (dm.MultiplicativeSoboStrategy(domain=_domain(two), acquisition_function=af),
                       dm.MultiplicativeAdditiveSoboStrategy(domain=_domain(two), acquisition_function=af,
                                                             additive_features=["y1"])):
        s = strategies.map(data_model)
        with pytest.raises(NotImplementedError) as err:
            s._get_acqfs(1)
        for name in ("qLogNEI", "qNEI", "qLogEI", "qEI"):
            assert name in str(err.value)


def test_acquisition_classes_insist_on_a_multspec():
    from everest_amd.acquisition import QMultLogEI, QMultLogNEI, QMultNEI, QSoboLogEI, QSoboNEI
    assert issubclass(QMultNEI, QSoboNEI) and issubclass(QMultLogNEI, QMultNEI) and issubclass(QMultLogEI, QSoboLogEI)
    sobo = ops.SoboSpec(2, [(0, A, 1.0, 1.0, 0.0, 0.0)])
    for cls, args in ((QMultNEI, (None, None, None, sobo)), (QMultLogNEI, (None, None, None, sobo)),
                      (QMultLogEI, (None, None, sobo))):
        with pytest.raises(TypeError, match="MultSpec"):
            cls(*args)
    assert sr.AFFINE == A and sr.TARGET == T
