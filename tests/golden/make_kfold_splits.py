"""Generate tests/golden/kfold_splits.json from scikit-learn: the (train, test) index lists of
``sklearn.model_selection.KFold(n_splits=k, shuffle=True, random_state=seed)`` on n rows — the
splitter bofire/surrogates/trainable.py:327 uses — for the (n, k, seed) cases below.
everest_amd.surrogates.kfold_indices restates it in numpy (no scikit-learn on the GPU host);
tests/test_cross_validation_host.py compares the two.

Run where scikit-learn is installed:
    python tests/golden/make_kfold_splits.py
"""
import json
import os

import numpy as np
import sklearn
from sklearn.model_selection import KFold

CASES = [(13, 4, 0), (12, 3, 7), (9, 9, 1), (70, 5, 42), (2, 2, 3), (23, 4, 3), (5, 2, 11)]

out = {"sklearn": sklearn.__version__, "cases": []}
for n, k, seed in CASES:
    folds = [{"train": tr.tolist(), "test": te.tolist()}
             for tr, te in KFold(n_splits=k, shuffle=True, random_state=seed).split(np.zeros((n, 1)))]
    out["cases"].append({"n": n, "k": k, "seed": seed, "folds": folds})

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kfold_splits.json")
with open(path, "w") as f:
    json.dump(out, f, separators=(",", ":"))
    f.write("\n")
print(f"wrote {path}: {len(CASES)} cases")
