"""Generate tests/golden/dot_surrogates.json by importing the REFERENCE's own data models.

Run where the reference checkout is available (it never travels with this repository):
    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dot_surrogate_golden.py
The surrogate data models are imported DIRECTLY (bofire.data_models.surrogates.linear / polynomial):
those modules import without BoTorch.  Writes expected outputs only: the full dumps of
``LinearSurrogate(inputs, outputs)`` and ``PolynomialSurrogate.from_power(3, inputs, outputs)``.
"""
import json
import os

from bofire.data_models.domain.api import Inputs, Outputs
from bofire.data_models.features.api import ContinuousInput, ContinuousOutput
from bofire.data_models.surrogates.linear import LinearSurrogate
from bofire.data_models.surrogates.polynomial import PolynomialSurrogate

inputs = Inputs(features=[ContinuousInput(key="a", bounds=(0, 40)), ContinuousInput(key="b", bounds=(20, 60))])
outputs = Outputs(features=[ContinuousOutput(key="c")])

out = {
    "LinearSurrogate": json.loads(LinearSurrogate(inputs=inputs, outputs=outputs).model_dump_json()),
    "PolynomialSurrogate_from_power_3": json.loads(PolynomialSurrogate.from_power(3, inputs=inputs,
                                                                                  outputs=outputs).model_dump_json()),
}

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dot_surrogates.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
print("wrote", path)
