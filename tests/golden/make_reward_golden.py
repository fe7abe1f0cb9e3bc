"""Generate tests/golden/reward_datamodels.json by importing the REFERENCE's own data models.

Run where the reference checkout is available (it never travels with this repository):
    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reward_golden.py
bofire.data_models.acquisition_functions.api and bofire.data_models.strategies.predictives.sobo
import without BoTorch.  Writes inputs + expected outputs only:
  - the default dumps of qSR / qUCB / qPI and of SoboStrategy / AdditiveSoboStrategy carrying each
    (domain and surrogate specs left out),
  - which values of beta, tau and n_mc_samples validate.
"""
import json
import os

from bofire.data_models.acquisition_functions.api import qPI, qSR, qUCB
from bofire.data_models.domain.api import Domain, Inputs, Outputs
from bofire.data_models.features.api import ContinuousInput, ContinuousOutput
from bofire.data_models.objectives.api import MinimizeObjective, MinimizeSigmoidObjective
from bofire.data_models.strategies.predictives.sobo import AdditiveSoboStrategy, SoboStrategy

out = {}

INPUTS = Inputs(features=[ContinuousInput(key="x1", bounds=[0, 1]), ContinuousInput(key="x2", bounds=[0, 1])])
two = [MinimizeObjective(w=1.0), MinimizeSigmoidObjective(w=1.0, steepness=2.0, tp=0.5)]
DOMAIN = Domain(inputs=INPUTS, outputs=Outputs(features=[ContinuousOutput(key=f"y{i}", objective=o)
                                                         for i, o in enumerate(two)]))
ACQFS = {"qSR": qSR, "qUCB": qUCB, "qPI": qPI}


def dump(s):
    d = json.loads(s.model_dump_json())
    return {k: v for k, v in d.items() if k not in ("domain", "surrogate_specs")}


out["acquisition_functions"] = [json.loads(cls().model_dump_json()) for cls in ACQFS.values()]
out["strategies"] = {
    f"{scls.__name__}_{name}": dump(scls(domain=DOMAIN, acquisition_function=cls()))
    for scls in (SoboStrategy, AdditiveSoboStrategy) for name, cls in ACQFS.items()
}


def accepts(cls, **kw):
    try:
        cls(**kw)
        return True
    except ValueError:
        return False


out["validation"] = (
    [{"type": "qUCB", "kwargs": {"beta": b}, "valid": accepts(qUCB, beta=b)} for b in (-0.1, 0.0, 0.2)]
    + [{"type": "qPI", "kwargs": {"tau": t}, "valid": accepts(qPI, tau=t)} for t in (0.0, 1e-3)]
    + [{"type": name, "kwargs": {"n_mc_samples": n}, "valid": accepts(cls, n_mc_samples=n)}
       for name, cls in ACQFS.items() for n in (96, 128)]
)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reward_datamodels.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
print("wrote", path)
