"""Writes tests/golden/reference_active_learning.json from the reference's importable data model
module bofire.data_models.strategies.predictives.active_learning (the reference tree on
PYTHONPATH, PYTHONDONTWRITEBYTECODE=1):

    python tests/golden/make_reference_active_learning.py

Data only: the pydantic field names (all, and those the strategy declares beside its
BotorchStrategy base), the ``type`` strings and the defaults of the acquisition."""
import json
import os

from bofire.data_models.acquisition_functions.api import qNegIntPosVar
from bofire.data_models.strategies.predictives.active_learning import ActiveLearningStrategy
from bofire.data_models.strategies.predictives.botorch import BotorchStrategy


def main():
    acq = qNegIntPosVar()
    out = {
        "source": "generated from the reference's data model module",
        "strategy_type": ActiveLearningStrategy.model_fields["type"].default,
        "strategy_fields": sorted(ActiveLearningStrategy.model_fields),
        # what the strategy declares itself, beside its BotorchStrategy base
        "strategy_own_fields": sorted(k for k, f in ActiveLearningStrategy.model_fields.items()
                                      if k not in BotorchStrategy.model_fields
                                      or f.annotation != BotorchStrategy.model_fields[k].annotation),
        "acquisition_type": acq.type,
        "acquisition_fields": sorted(type(acq).model_fields),
        "acquisition_defaults": {"n_mc_samples": acq.n_mc_samples, "weights": acq.weights},
    }
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_active_learning.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
