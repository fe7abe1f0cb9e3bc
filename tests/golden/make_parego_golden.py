"""Generate tests/golden/parego_datamodels.json by importing the REFERENCE's own data model.

Run where the reference checkout is available (it never travels with this repository):
    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_parego_golden.py
The strategy data model is imported DIRECTLY (bofire.data_models.strategies.predictives.qparego):
that module imports without BoTorch, bofire.data_models.strategies.api does not.
Writes inputs + expected outputs only:
  - the default dump of QparegoStrategy and one with a non-default acquisition (domain and
    surrogate specs left out),
  - which of a handful of output sets the objective / multi-objective validators accept.
"""
import json
import os

from bofire.data_models.acquisition_functions.api import qLogEI
from bofire.data_models.domain.api import Domain, Inputs, Outputs
from bofire.data_models.features.api import ContinuousInput, ContinuousOutput
from bofire.data_models.objectives.api import (CloseToTargetObjective, MaximizeObjective, MaximizeSigmoidObjective,
                                               MinimizeObjective, MinimizeSigmoidObjective,
                                               MovingMaximizeSigmoidObjective, TargetObjective)
from bofire.data_models.strategies.predictives.qparego import QparegoStrategy

out = {}

INPUTS = Inputs(features=[ContinuousInput(key="x1", bounds=[0, 1]), ContinuousInput(key="x2", bounds=[0, 1])])


def domain(objectives):
    return Domain(inputs=INPUTS, outputs=Outputs(features=[ContinuousOutput(key=f"y{i}", objective=o)
                                                           for i, o in enumerate(objectives)]))


def dump(s):
    d = json.loads(s.model_dump_json())
    return {k: v for k, v in d.items() if k not in ("domain", "surrogate_specs")}


two = [MinimizeObjective(w=1.0), MaximizeObjective(w=1.0)]
out["defaults"] = {
    "QparegoStrategy": dump(QparegoStrategy(domain=domain(two))),
    "QparegoStrategy_qLogEI": dump(QparegoStrategy(domain=domain(two), acquisition_function=qLogEI(n_mc_samples=128),
                                                   seed=7)),
}

sets = {
    "min_max": two,
    "min_ctt": [MinimizeObjective(w=1.0), CloseToTargetObjective(w=1.0, target_value=0.4, exponent=2.0)],
    "min_max_all_constrained_kinds": [MinimizeObjective(w=1.0), MaximizeObjective(w=1.0),
                                      TargetObjective(w=1.0, target_value=0.8, tolerance=0.6, steepness=4.0),
                                      MinimizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5),
                                      MaximizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5)],
    "min_max_none": [MinimizeObjective(w=1.0), MaximizeObjective(w=1.0), None],
    # rejected: one scalarised objective only
    "min": [MinimizeObjective(w=1.0)],
    "min_minsig": [MinimizeObjective(w=1.0), MinimizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5)],
    # rejected: a weight != 1
    "min_max_weight": [MinimizeObjective(w=1.0), MaximizeObjective(w=0.5)],
    # rejected: an objective type outside the allowed six
    "min_max_movingsig": [MinimizeObjective(w=1.0), MaximizeObjective(w=1.0),
                          MovingMaximizeSigmoidObjective(w=1.0, steepness=1.5, tp=-0.3)],
}


def accepts(objectives):
    try:
        QparegoStrategy(domain=domain(objectives))
        return True
    except ValueError:
        return False


out["validators"] = [{"name": k, "objectives": [None if o is None else json.loads(o.model_dump_json()) for o in v],
                      "QparegoStrategy": accepts(v)} for k, v in sets.items()]

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "parego_datamodels.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
print("wrote", path)
