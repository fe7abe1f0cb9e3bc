"""Generate tests/golden/scale_kernel.json by importing the REFERENCE's own data models.

Run where the reference checkout is available (it never travels with this repository):
    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_scale_kernel_golden.py
Writes expected outputs only: the dumps of the ``ScaleKernel`` specs the reference's users store
(the pre-Hvarfner default ``ScaleKernel(MaternKernel(2.5))`` with the THREESIX and the MBO priors, an
RBF base without an outputscale prior), of a ``SingleTaskGPSurrogate`` around the first, and of the
four prior factories.
"""
import json
import os

from bofire.data_models.domain.api import Inputs, Outputs
from bofire.data_models.features.api import ContinuousInput, ContinuousOutput
from bofire.data_models.kernels.api import MaternKernel, RBFKernel, ScaleKernel
from bofire.data_models.priors.api import (MBO_LENGTHCALE_PRIOR, MBO_NOISE_PRIOR, MBO_OUTPUTSCALE_PRIOR,
                                           THREESIX_LENGTHSCALE_PRIOR, THREESIX_NOISE_PRIOR, THREESIX_SCALE_PRIOR)
from bofire.data_models.surrogates.single_task_gp import SingleTaskGPSurrogate

inputs = Inputs(features=[ContinuousInput(key="a", bounds=(0, 40)), ContinuousInput(key="b", bounds=(20, 60))])
outputs = Outputs(features=[ContinuousOutput(key="c")])
threesix = ScaleKernel(base_kernel=MaternKernel(ard=True, nu=2.5, lengthscale_prior=THREESIX_LENGTHSCALE_PRIOR()),
                       outputscale_prior=THREESIX_SCALE_PRIOR())
mbo = ScaleKernel(base_kernel=MaternKernel(ard=True, nu=2.5, lengthscale_prior=MBO_LENGTHCALE_PRIOR()),
                  outputscale_prior=MBO_OUTPUTSCALE_PRIOR())
rbf = ScaleKernel(base_kernel=RBFKernel(ard=True))
dump = lambda m: json.loads(m.model_dump_json())  # noqa: E731

out = {
    "kernels": {"threesix": dump(threesix), "mbo": dump(mbo), "rbf_no_prior": dump(rbf)},
    "priors": {"THREESIX_SCALE_PRIOR": dump(THREESIX_SCALE_PRIOR()), "MBO_LENGTHCALE_PRIOR": dump(MBO_LENGTHCALE_PRIOR()),
               "MBO_NOISE_PRIOR": dump(MBO_NOISE_PRIOR()), "MBO_OUTPUTSCALE_PRIOR": dump(MBO_OUTPUTSCALE_PRIOR())},
    "SingleTaskGPSurrogate": dump(SingleTaskGPSurrogate(inputs=inputs, outputs=outputs, kernel=threesix,
                                                        noise_prior=THREESIX_NOISE_PRIOR())),
}

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scale_kernel.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
print("wrote", path)
