"""Generate tests/golden/mult_sobo_datamodels.json by importing the REFERENCE's own data models.

Run where the reference checkout is available (it never travels with this repository):
    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mult_sobo_golden.py
The strategy data models are imported DIRECTLY (bofire.data_models.strategies.predictives.sobo):
that module imports without BoTorch, bofire.data_models.strategies.api and bofire.utils.torch_tools
do not.  Writes inputs + expected outputs only:
  - the default dumps of MultiplicativeSoboStrategy and MultiplicativeAdditiveSoboStrategy (domain
    and surrogate specs left out),
  - a validator table: which output sets / additive features each data model accepts, and the
    exception type and message where it does not,
  - per case, the list that _callables_and_weights (bofire/utils/torch_tools.py:598-659) keeps
    (walk outputs.get() in order, skip outputs without an objective and, with exclude_constraints,
    those with a ConstrainedObjective, divide the weights by the smallest) and the split of
    get_multiplicative_additive_objective (:770-792) by additive_features — a few lines of plain
    Python over the reference's data models, restated here because torch_tools itself does not
    import offline.
"""
import json
import os

from bofire.data_models.domain.api import Domain, Inputs, Outputs
from bofire.data_models.features.api import ContinuousInput, ContinuousOutput
from bofire.data_models.objectives.api import (CloseToTargetObjective, ConstrainedObjective, MaximizeObjective,
                                               MaximizeSigmoidObjective, MinimizeObjective, MinimizeSigmoidObjective,
                                               MovingMaximizeSigmoidObjective, TargetObjective)
from bofire.data_models.strategies.predictives.sobo import (MultiplicativeAdditiveSoboStrategy,
                                                            MultiplicativeSoboStrategy)

out = {}

INPUTS = Inputs(features=[ContinuousInput(key="x1", bounds=[0, 1]), ContinuousInput(key="x2", bounds=[0, 1])])


def domain(objectives):
    return Domain(inputs=INPUTS, outputs=Outputs(features=[ContinuousOutput(key=f"y{i}", objective=o)
                                                           for i, o in enumerate(objectives)]))


def dump(s):
    d = json.loads(s.model_dump_json())
    return {k: v for k, v in d.items() if k not in ("domain", "surrogate_specs")}


two = [MaximizeObjective(w=1.0), MinimizeObjective(w=0.5)]
out["defaults"] = {
    "MultiplicativeSoboStrategy": dump(MultiplicativeSoboStrategy(domain=domain(two))),
    "MultiplicativeAdditiveSoboStrategy": dump(MultiplicativeAdditiveSoboStrategy(domain=domain(two))),
    "MultiplicativeAdditiveSoboStrategy_y1": dump(MultiplicativeAdditiveSoboStrategy(domain=domain(two), seed=7,
                                                                                     additive_features=["y1"],
                                                                                     use_output_constraints=False)),
}

# name -> (objectives, additive features)
cases = {
    "one": ([MaximizeObjective(w=1.0)], []),
    "two": (two, []),
    "two_additive": (two, ["y1"]),
    "tiny_weight": ([MaximizeObjective(w=1.0), MinimizeObjective(w=1e-9)], []),
    "unknown_additive": (two, ["nope"]),
    "input_as_additive": (two, ["x1"]),
    "known_answer": ([MaximizeObjective(w=0.25), MaximizeObjective(w=0.5), MaximizeObjective(w=1.0)], ["y2"]),
    "with_none": ([MaximizeObjective(w=0.8), None, CloseToTargetObjective(w=0.4, target_value=0.4, exponent=2.0)],
                  ["y2"]),
    # a sigmoid output: a factor of the multiplicative utility, nothing in the multiplicative-additive one
    "sigmoid": ([MaximizeObjective(w=0.6), MaximizeSigmoidObjective(w=0.2, steepness=2.0, tp=0.5),
                 MinimizeObjective(w=0.9)], ["y2"]),
    "sigmoid_named_additive": ([MaximizeObjective(w=0.6), MaximizeSigmoidObjective(w=0.2, steepness=2.0, tp=0.5),
                                MinimizeObjective(w=0.9)], ["y1", "y2"]),
    "all_kinds": ([MaximizeObjective(w=0.5), MinimizeSigmoidObjective(w=0.25, steepness=2.0, tp=0.5),
                   TargetObjective(w=1.0, target_value=0.8, tolerance=0.6, steepness=4.0),
                   MovingMaximizeSigmoidObjective(w=0.75, steepness=1.5, tp=-0.3),
                   CloseToTargetObjective(w=0.3, target_value=0.4, exponent=2.0)], ["y4"]),
    "all_constrained": ([MaximizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5),
                         TargetObjective(w=0.5, target_value=0.8, tolerance=0.6, steepness=4.0)], []),
    "all_additive": (two, ["y0", "y1"]),
}


def verdict(cls, objectives, **kw):
    try:
        cls(domain=domain(objectives), **kw)
        return {"accepts": True}
    except Exception as e:  # the reference's weight check raises a TypeError, not a ValidationError
        return {"accepts": False, "exception": type(e).__name__, "is_value_error": isinstance(e, ValueError),
                "message": str(e)}


def listed(outputs, exclude_constraints):
    """_callables_and_weights: keys and normalised weights."""
    keys, weights = [], []
    for feat in outputs.get():
        if feat.objective is None:
            continue
        if exclude_constraints and isinstance(feat.objective, ConstrainedObjective):
            continue
        keys.append(feat.key)
        weights.append(feat.objective.w)
    if not weights:
        return None                     # the reference fails in min([])
    min_w = min(weights)
    return keys, [w / min_w for w in weights]


def split(outputs, exclude_constraints, additive_features):
    kw = listed(outputs, exclude_constraints)
    if kw is None:
        return None
    fac = [[k, w] for k, w in zip(*kw) if k not in additive_features]
    add = [[k, w] for k, w in zip(*kw) if k in additive_features]
    return {"factors": fac, "addends": add}


rows = []
for name, (objectives, additive) in cases.items():
    row = {"name": name, "objectives": [None if o is None else json.loads(o.model_dump_json()) for o in objectives],
           "additive_features": additive,
           "MultiplicativeSoboStrategy": verdict(MultiplicativeSoboStrategy, objectives),
           "MultiplicativeAdditiveSoboStrategy": verdict(MultiplicativeAdditiveSoboStrategy, objectives,
                                                         additive_features=additive)}
    outputs = domain(objectives).outputs
    # the multiplicative utility lists every objective and has no addends; the multiplicative-additive
    # one keeps the function's default exclude_constraints=True
    row["multiplicative"] = split(outputs, False, [])
    row["multiplicative_additive"] = split(outputs, True, additive)
    rows.append(row)
out["cases"] = rows

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mult_sobo_datamodels.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
print("wrote", path)
