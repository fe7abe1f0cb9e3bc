"""Generate tests/golden/sobo_datamodels.json by importing the REFERENCE's own data models.

Run where the reference checkout is available (it never travels with this repository):
    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sobo_golden.py
The strategy data models are imported DIRECTLY (bofire.data_models.strategies.predictives.sobo):
that module imports without BoTorch, bofire.data_models.strategies.api does not.
Writes inputs + expected outputs only:
  - the default dumps of SoboStrategy / AdditiveSoboStrategy (domain and surrogate specs left out),
  - the sigmoid / target objective __call__ values on a small grid,
  - which of a handful of output sets each strategy's domain validator accepts.
"""
import json
import os

import numpy as np

from bofire.data_models.acquisition_functions.api import qEI, qLogEI, qLogNEI, qNEI
from bofire.data_models.domain.api import Domain, Inputs, Outputs
from bofire.data_models.features.api import ContinuousInput, ContinuousOutput
from bofire.data_models.objectives.api import (CloseToTargetObjective, MaximizeObjective, MaximizeSigmoidObjective,
                                               MinimizeObjective, MinimizeSigmoidObjective,
                                               MovingMaximizeSigmoidObjective, TargetObjective)
from bofire.data_models.strategies.predictives.sobo import AdditiveSoboStrategy, SoboStrategy

out = {}

INPUTS = Inputs(features=[ContinuousInput(key="x1", bounds=[0, 1]), ContinuousInput(key="x2", bounds=[0, 1])])


def domain(objectives):
    return Domain(inputs=INPUTS, outputs=Outputs(features=[ContinuousOutput(key=f"y{i}", objective=o)
                                                           for i, o in enumerate(objectives)]))


def dump(s):
    d = json.loads(s.model_dump_json())
    return {k: v for k, v in d.items() if k not in ("domain", "surrogate_specs")}


two = [MinimizeObjective(w=1.0), MinimizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5)]
out["defaults"] = {
    "SoboStrategy": dump(SoboStrategy(domain=domain(two))),
    "AdditiveSoboStrategy": dump(AdditiveSoboStrategy(domain=domain(two))),
    "AdditiveSoboStrategy_absorbed": dump(AdditiveSoboStrategy(domain=domain(two), use_output_constraints=False,
                                                               acquisition_function=qEI(n_mc_samples=128))),
    "acquisition_functions": [json.loads(a.model_dump_json()) for a in (qLogNEI(), qNEI(), qLogEI(), qEI())],
}

# objective __call__ values (bofire/data_models/objectives/sigmoid.py, target.py)
y = np.linspace(-3.0, 4.0, 15)
x_adapt = np.array([0.2, 1.4, -0.5])
objs = [
    MaximizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5),
    MinimizeSigmoidObjective(w=0.5, steepness=3.0, tp=-0.25),
    MovingMaximizeSigmoidObjective(w=1.0, steepness=1.5, tp=-0.3),
    TargetObjective(w=0.7, target_value=0.8, tolerance=0.6, steepness=4.0),
    TargetObjective(w=1.0, target_value=-1.0, tolerance=0.0, steepness=1.0),
    MaximizeObjective(w=0.4, bounds=[-1, 3]),
    MinimizeObjective(w=1.0),
    CloseToTargetObjective(w=0.3, target_value=0.4, exponent=2.0),
]
out["objective_calls"] = {
    "y": y.tolist(), "x_adapt": x_adapt.tolist(),
    "cases": [{"objective": json.loads(o.model_dump_json()),
               "values": np.asarray(o(y, x_adapt), dtype=np.float64).tolist()} for o in objs],
}

# domain validators
sets = {
    "min": [MinimizeObjective(w=1.0)],
    "min_min": [MinimizeObjective(w=1.0), MinimizeObjective(w=1.0)],
    "min_minsig": two,
    "min_target_maxsig": [MinimizeObjective(w=1.0),
                          TargetObjective(w=1.0, target_value=0.8, tolerance=0.6, steepness=4.0),
                          MaximizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5)],
    "maxsig": [MaximizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5)],
    "maxsig_minsig": [MaximizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5),
                      MinimizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5)],
    "min_none": [MinimizeObjective(w=1.0), None],
    "min_max_ctt": [MinimizeObjective(w=1.0), MaximizeObjective(w=1.0),
                    CloseToTargetObjective(w=1.0, target_value=0.4, exponent=2.0)],
    "min_min_none": [MinimizeObjective(w=1.0), MinimizeObjective(w=0.5), None],
}


def accepts(cls, objectives):
    try:
        cls(domain=domain(objectives))
        return True
    except ValueError:
        return False


out["validators"] = [{"name": k, "objectives": [None if o is None else json.loads(o.model_dump_json()) for o in v],
                      "SoboStrategy": accepts(SoboStrategy, v),
                      "AdditiveSoboStrategy": accepts(AdditiveSoboStrategy, v)} for k, v in sets.items()]

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sobo_datamodels.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
print("wrote", path)
