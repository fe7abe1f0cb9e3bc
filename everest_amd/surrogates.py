"""Functional surrogates on the device — mirrors bofire/surrogates/{single_task_gp,botorch,
surrogate,trainable,botorch_surrogates}.py for ``SingleTaskGPSurrogate``, and
bofire/surrogates/mixed_single_task_gp.py for ``MixedSingleTaskGPSurrogate``; ``LinearSurrogate``
and ``PolynomialSurrogate`` (SingleTaskGP with a dot-product kernel in the reference) share
``DotProductGPSurrogate``.

The fitted model (transformed training inputs, targets, hyperparameters, Normalize bounds,
kernel family) is the wire format of ``dumps()/loads()`` — a versioned JSON + base64(npz)
blob instead of the reference's base64 BoTorch pickle (bofire/surrogates/botorch.py:66-77),
which cannot be produced without BoTorch.
"""
from __future__ import annotations

import base64
import copy
import io
import json
import math
import os
import warnings
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import pandas as pd
import torch

from . import data_models as dm
from .data_models.models import (CategoricalEncodingEnum, DimensionalityScaledLogNormalPrior, GammaPrior,
                                  LogNormalPrior, MaternKernel, NormalPrior, RBFKernel, ScalerEnum)
from .diagnostics import CvResult, CvResults
from .gp import GPBatch, GPHyper, fit_single, fold_outputscale, standardize_params

KIND_BY_NU = {0.5: 1, 1.5: 2, 2.5: 3}
# feature types a cross-validation can be stratified by (of the reference's DiscreteInput,
# CategoricalInput, CategoricalOutput and ContinuousOutput, the ones this build has)
_STRATIFIABLE = (dm.CategoricalInput, dm.ContinuousOutput)


def check_valid_nfolds(folds: int, n: int) -> int:
    """The number of folds to run on n experiments (trainable.py:270-295): -1 is leave-one-out,
    more folds than experiments falls back to it with a warning."""
    if n == 0:
        raise ValueError("Experiments is empty.")
    if folds > n:
        warnings.warn(f"Training data only has {n} experiments, which is less than folds, fallback to LOOCV.")
        return n
    if folds == -1:
        return n
    if folds < 2:
        raise ValueError("Folds must be -1 for LOO, or > 1.")
    return folds


def kfold_indices(n: int, k: int, random_state: Optional[int] = None) -> List[Tuple[np.ndarray, np.ndarray]]:
    """(train, test) index arrays of ``sklearn.model_selection.KFold(k, shuffle=True,
    random_state=random_state).split`` on n rows, restated in numpy: one shuffle of range(n)
    by RandomState(random_state), cut into consecutive slices of n // k rows (one more in the
    first n % k); a fold's test rows are its slice, sorted, its train rows the others, ascending."""
    idx = np.arange(n)
    np.random.RandomState(random_state).shuffle(idx)
    sizes = np.full(k, n // k, dtype=int)
    sizes[:n % k] += 1
    out, start = [], 0
    for size in sizes:
        held = np.zeros(n, dtype=bool)
        held[idx[start:start + size]] = True
        out.append((np.flatnonzero(~held), np.flatnonzero(held)))
        start += size
    return out


def cv_splits(experiments: pd.DataFrame, folds: int, random_state: Optional[int] = None,
              stratified_feature: Optional[str] = None, group_split_column: Optional[str] = None):
    """The folds' (train, test) row positions (trainable.py:297-339): stratified K-fold when a
    feature is named, else group shuffle splits when a group column is, else shuffled K-fold."""
    if stratified_feature is None and group_split_column is None:
        return kfold_indices(len(experiments), folds, random_state)
    try:
        from sklearn.model_selection import GroupShuffleSplit, StratifiedKFold
    except ImportError as e:
        raise NotImplementedError("stratified and group splits need the scikit-learn package (sklearn), "
                                  "which is not installed") from e
    if stratified_feature is not None:
        cv = StratifiedKFold(n_splits=folds, shuffle=True, random_state=random_state)
        return list(cv.split(experiments.drop([stratified_feature], axis=1), experiments[stratified_feature]))
    cv = GroupShuffleSplit(n_splits=folds, random_state=random_state)
    return list(cv.split(experiments, groups=experiments[group_split_column]))


def device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("everest_amd surrogates run on the MI355X only (no HIP device visible)")
    return torch.device("cuda", torch.cuda.current_device())


def kernel_kind(kernel) -> int:
    """bofire/kernels/mapper.py:31-69."""
    if isinstance(kernel, RBFKernel):
        return 0
    if isinstance(kernel, MaternKernel):
        return KIND_BY_NU[kernel.nu]
    raise NotImplementedError(f"kernel {type(kernel).__name__} is out of scope for the MI355X build")


def unwrap_scale(kernel):
    """(base kernel, scaled, outputscale prior spec) of a SingleTaskGPSurrogate kernel: a
    ScaleKernel gives its base kernel (family and lengthscale prior come from it) and a fitted
    outputscale (bofire/kernels/mapper.py: gpytorch ScaleKernel(base, outputscale_prior))."""
    if isinstance(kernel, dm.ScaleKernel):
        return kernel.base_kernel, True, map_prior(kernel.outputscale_prior, 1)
    return kernel, False, None


def map_prior(prior, d: int) -> Optional[Tuple[str, float, float]]:
    """bofire/priors/mapper.py:9-63 -> (family, p1, p2)."""
    if prior is None:
        return None
    if isinstance(prior, DimensionalityScaledLogNormalPrior):
        return ("lognormal", prior.loc + math.log(d) * prior.loc_scaling,
                (prior.scale ** 2 + math.log(d) * prior.scale_scaling) ** 0.5)
    if isinstance(prior, LogNormalPrior):
        return ("lognormal", float(prior.loc), float(prior.scale))
    if isinstance(prior, GammaPrior):
        return ("gamma", float(prior.concentration), float(prior.rate))
    if isinstance(prior, NormalPrior):
        return ("normal", float(prior.loc), float(prior.scale))
    raise NotImplementedError(type(prior).__name__)


def run_cross_validation(surrogate_, fit_folds: Callable, experiments: pd.DataFrame, folds: int = -1,
                         include_X: bool = False, include_labcodes: bool = False,
                         random_state: Optional[int] = None, stratified_feature: Optional[str] = None,
                         group_split_column: Optional[str] = None, hooks: Optional[Dict[str, Callable]] = None,
                         hook_kwargs: Optional[Dict[str, Dict[str, Any]]] = None
                         ) -> Tuple[CvResults, CvResults, Dict[str, list]]:
    """The argument checks, split, result and hook code of ``cross_validate``
    (bofire/surrogates/trainable.py:79-339), shared by the surrogate classes.
    ``fit_folds(experiments, splits)`` returns, per fold, (surrogate getter, {"train" / "test":
    predictions}) on the rows valid for the surrogate's output."""
    if include_labcodes and "labcode" not in experiments.columns:
        raise ValueError("No labcodes available for the provided experiments.")
    if len(surrogate_.outputs) > 1:
        raise NotImplementedError("Cross validation not implemented for multi-output models")
    if stratified_feature is not None:
        if stratified_feature not in surrogate_.inputs.get_keys() + surrogate_.outputs.get_keys():
            raise ValueError("The feature to be stratified is not in the model inputs or outputs")
        feats = surrogate_.inputs if stratified_feature in surrogate_.inputs.get_keys() else surrogate_.outputs
        if not isinstance(feats.get_by_key(stratified_feature), _STRATIFIABLE):
            raise ValueError("The feature to be stratified needs to be a DiscreteInput, CategoricalInput, "
                             "CategoricalOutput, or ContinuousOutput")
    if group_split_column is not None:
        if group_split_column not in experiments.columns:
            raise ValueError(f"Group split column {group_split_column} is not present in the experiments.")
        ngroups = experiments[group_split_column].nunique(dropna=False)
        if ngroups < folds:
            raise ValueError(f"Number of unique groups {ngroups} is less than the number of folds {folds}.")
    experiments = surrogate_._preprocess_experiments(experiments)
    folds = check_valid_nfolds(folds, len(experiments))
    splits = cv_splits(experiments, folds, random_state, stratified_feature, group_split_column)
    hooks, hook_kwargs = hooks or {}, hook_kwargs or {}
    key, in_keys = surrogate_.output_key, surrogate_.inputs.get_keys()
    fitted = fit_folds(experiments, splits)
    train_results, test_results, hook_results = [], [], {name: [] for name in hooks}
    for (tr, te), (surrogate, pred) in zip(splits, fitted):
        rows = {"train": experiments.iloc[tr], "test": experiments.iloc[te]}
        for part, out in (("train", train_results), ("test", test_results)):
            df = rows[part]
            out.append(CvResult(key=key, observed=df[key], predicted=pred[part][f"{key}_pred"],
                                standard_deviation=pred[part][f"{key}_sd"],
                                X=df[in_keys] if include_X else None,
                                labcodes=df["labcode"] if include_labcodes else None))
        fold_model = surrogate() if hooks else None      # built only when a hook asks for it
        for name, hook in hooks.items():
            hook_results[name].append(hook(surrogate=fold_model, X_train=rows["train"][in_keys],
                                           y_train=rows["train"][[key]], X_test=rows["test"][in_keys],
                                           y_test=rows["test"][[key]], **hook_kwargs.get(name, {})))
    return CvResults(train_results), CvResults(test_results), hook_results


def cv_sequential(surrogate_, experiments: pd.DataFrame, splits):
    """Per fold (surrogate getter, {"train" / "test": predictions}): one fit after another, a
    fresh copy of the surrogate per fold."""
    key, in_keys = surrogate_.output_key, surrogate_.inputs.get_keys()
    out = []
    for tr, te in splits:
        sur = copy.copy(surrogate_)
        sur._fit(experiments.iloc[tr][in_keys], experiments.iloc[tr][[key]])
        out.append((lambda s=sur: s, {"train": sur.predict(experiments.iloc[tr][in_keys]),
                                      "test": sur.predict(experiments.iloc[te][in_keys])}))
    return out


class SingleTaskGPSurrogate:
    """Exact GP surrogate for one output (bofire/surrogates/single_task_gp.py:23-71)."""

    def __init__(self, data_model: dm.SingleTaskGPSurrogate):
        self.data_model = data_model
        self.inputs = data_model.inputs
        self.outputs = data_model.outputs
        self.kernel = data_model.kernel
        self.noise_prior = data_model.noise_prior
        self.scaler = data_model.scaler
        self.output_scaler = data_model.output_scaler
        self.input_preprocessing_specs = {k: v.value if hasattr(v, "value") else v
                                          for k, v in data_model.input_preprocessing_specs.items()}
        self.state: Optional[dict] = None
        self.gp: Optional[GPBatch] = None
        if data_model.dump is not None:
            self.loads(data_model.dump)

    @property
    def is_fitted(self) -> bool:
        return self.state is not None

    @property
    def output_key(self) -> str:
        return self.outputs.get_keys()[0]

    # ---- transforms ----------------------------------------------------------------
    def _bounds(self, X: pd.DataFrame) -> Tuple[np.ndarray, np.ndarray]:
        """Normalize bounds on the continuous columns (get_scaler, bofire/surrogates/utils.py:103-164);
        one-hot columns keep [0, 1] (identity)."""
        f2i, _ = self.inputs._transform_info(self.input_preprocessing_specs)
        d = sum(len(v) for v in f2i.values())
        lo, hi = np.zeros(d), np.ones(d)
        if self.scaler == ScalerEnum.NORMALIZE:
            for feat in self.inputs.get(dm.ContinuousInput).features:
                (l,), (u,) = feat.get_bounds(values=X[feat.key])
                j = f2i[feat.key][0]
                lo[j], hi[j] = l, (u if u > l else l + 1.0)
        elif self.scaler != ScalerEnum.IDENTITY:
            raise NotImplementedError("InputStandardize is out of scope for the MI355X build")
        return lo, hi

    def transform_inputs(self, X: pd.DataFrame) -> np.ndarray:
        return self.inputs.transform(X, self.input_preprocessing_specs).values.astype(np.float64)

    # ---- fit -------------------------------------------------------------------------
    def fit(self, experiments: pd.DataFrame, options: Optional[dict] = None):
        """TrainableSurrogate.fit (bofire/surrogates/trainable.py:24-42): valid rows of this output."""
        X, Y = self._fit_data(experiments)
        self._fit(X, Y, options)

    def _preprocess_experiments(self, experiments: pd.DataFrame) -> pd.DataFrame:
        """The rows valid for this output (bofire/surrogates/trainable.py:44-66), all columns."""
        key = self.output_key
        df = experiments
        if f"valid_{key}" in df:
            df = df[df[f"valid_{key}"] > 0]
        return df.dropna(subset=[key])

    def _fit_data(self, experiments: pd.DataFrame):
        key = self.output_key
        df = self._preprocess_experiments(experiments)
        return df[self.inputs.get_keys()], df[[key]]

    def _fit_problem(self, X: pd.DataFrame, Y: pd.DataFrame) -> dict:
        """Everything the MLL fit needs: transformed inputs, bounds, targets, kernel, priors."""
        Xt = self.transform_inputs(X)
        lo, hi = self._bounds(X)
        base, scaled, os_prior = unwrap_scale(self.kernel)
        return dict(Xt=Xt, lo=lo, hi=hi, y=Y.values[:, 0].astype(np.float64), kind=kernel_kind(base),
                    ls_prior=map_prior(getattr(base, "lengthscale_prior", None), Xt.shape[1]),
                    noise_prior=map_prior(self.noise_prior, 1),
                    standardize=self.output_scaler == ScalerEnum.STANDARDIZE,
                    scaled=scaled, os_prior=os_prior)

    def _fit(self, X: pd.DataFrame, Y: pd.DataFrame, options: Optional[dict] = None):
        pb = self._fit_problem(X, Y)
        Xn = torch.as_tensor((pb["Xt"] - pb["lo"]) / (pb["hi"] - pb["lo"]), dtype=torch.float64, device=device())
        hyp = fit_single(Xn, pb["y"], pb["kind"], pb["ls_prior"], pb["noise_prior"], standardize=pb["standardize"],
                         options=options, outputscale_prior=pb["os_prior"], scaled=pb["scaled"])
        self._set_state(pb["Xt"], pb["y"], pb["lo"], pb["hi"], pb["kind"], hyp)

    def _set_state(self, Xt, y, lo, hi, kind, hyp: GPHyper):
        self.state = dict(X=np.asarray(Xt), y=np.asarray(y), lo=np.asarray(lo), hi=np.asarray(hi), kind=int(kind),
                          lengthscale=np.asarray(hyp.lengthscale), noise=float(hyp.noise),
                          constant=float(hyp.constant), y_mean=float(hyp.y_mean), y_std=float(hyp.y_std))
        if hyp.outputscale is not None:      # a ScaleKernel fit: sigma^2 as fitted, the others unfolded
            self.state["outputscale"] = float(hyp.outputscale)
        self.gp = self._build_gp()

    def fitted_hyper(self) -> GPHyper:
        """The hyperparameters as fitted (a ScaleKernel's outputscale apart)."""
        s = self.state
        return GPHyper(lengthscale=s["lengthscale"], noise=s["noise"], constant=s["constant"], y_mean=s["y_mean"],
                       y_std=s["y_std"], outputscale=s.get("outputscale"))

    def hyper(self) -> GPHyper:
        """The device model's hyperparameters: a fitted outputscale folded into noise, constant and
        y_std (gp.fold_outputscale: exactly the same GP), so nothing downstream knows about it."""
        return fold_outputscale(self.fitted_hyper())

    def _build_gp(self) -> GPBatch:
        s = self.state
        dev = device()
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
        Xn = t((s["X"] - s["lo"]) / (s["hi"] - s["lo"]))
        return GPBatch(Xn, t(s["y"][:, None]), [self.hyper()], s["kind"], t(s["lo"]), t(s["hi"]))

    # ---- predict ----------------------------------------------------------------------
    def predict(self, experiments: pd.DataFrame) -> pd.DataFrame:
        """Surrogate.predict (bofire/surrogates/surrogate.py:39-67): posterior(observation_noise=True)."""
        if not self.is_fitted:
            raise ValueError("Model is not fitted/available yet.")
        Xt = self.transform_inputs(experiments[self.inputs.get_keys()])
        mean, var = self.gp.posterior(torch.as_tensor(Xt, dtype=torch.float64, device=self.gp.device),
                                      observation_noise=True)
        key = self.output_key
        return pd.DataFrame({f"{key}_pred": mean[0].cpu().numpy(), f"{key}_sd": np.sqrt(var[0].cpu().numpy())},
                            index=experiments.index)

    # ---- cross-validation --------------------------------------------------------------
    def cross_validate(self, experiments: pd.DataFrame, folds: int = -1, include_X: bool = False,
                       include_labcodes: bool = False, random_state: Optional[int] = None,
                       stratified_feature: Optional[str] = None, group_split_column: Optional[str] = None,
                       hooks: Optional[Dict[str, Callable]] = None,
                       hook_kwargs: Optional[Dict[str, Dict[str, Any]]] = None
                       ) -> Tuple[CvResults, CvResults, Dict[str, list]]:
        """TrainableSurrogate.cross_validate (bofire/surrogates/trainable.py:79-339): K-fold (or,
        folds = -1, leave-one-out) cross-validation on the rows valid for this output.  Returns
        the folds' train results, their test results, and per hook the list of its return
        values (a hook is called once per fold as ``hook(surrogate=, X_train=, y_train=,
        X_test=, y_test=, **hook_kwargs[name])`` with a surrogate fitted on that fold).

        Every fold is its own fit on its own rows, with its own Normalize bounds and Standardize
        statistics, as in the reference's loop of ``_fit`` calls — but the folds are fitted in
        lock-step (gp.fit_folds: one L-BFGS-B per fold, one member MLL plan launch per round) and
        predicted by one masked GPBatch posterior over all rows (fold j is output j, its mask
        its train rows, its bounds folded into its lengthscales as in
        BotorchSurrogates.compatibilize).  EVR_CV_LOCKSTEP=0 runs the plain sequential loop
        (a fresh surrogate per fold: ``_fit``, then ``predict`` twice).

        Unlike the reference, which leaves the last fold's model in ``self``, this surrogate's own
        fitted state is left as it was.  Plain K-fold splits are those of
        ``sklearn.model_selection.KFold(shuffle=True, random_state=random_state)`` (kfold_indices);
        ``stratified_feature`` and ``group_split_column`` need scikit-learn."""
        lockstep = os.environ.get("EVR_CV_LOCKSTEP", "1") != "0"
        return run_cross_validation(self, self._cv_lockstep if lockstep else self._cv_sequential, experiments,
                                    folds, include_X, include_labcodes, random_state, stratified_feature,
                                    group_split_column, hooks, hook_kwargs)

    def _cv_sequential(self, experiments: pd.DataFrame, splits):
        """Per fold (surrogate getter, {"train" / "test": predictions}): one fit after another."""
        return cv_sequential(self, experiments, splits)

    def _cv_lockstep(self, experiments: pd.DataFrame, splits):
        """_cv_sequential's result with all folds fitted in lock-step and predicted together."""
        from .gp import fit_folds, member_chunks

        key, in_keys = self.output_key, self.inputs.get_keys()
        pb = self._fit_problem(experiments[in_keys], experiments[[key]])
        Xt, y, lo0, hi0 = pb["Xt"], pb["y"], pb["lo"], pb["hi"]
        n, d = Xt.shape
        B, nmax = len(splits), max(len(tr) for tr, _ in splits)
        bounds = [self._bounds(experiments.iloc[tr][in_keys]) for tr, _ in splits]
        Xb, Yb = np.zeros((B, nmax, d)), np.zeros((B, nmax))
        for j, ((tr, _), (lo, hi)) in enumerate(zip(splits, bounds)):
            Xb[j, :len(tr)] = (Xt[tr] - lo) / (hi - lo)
            Yb[j, :len(tr)] = y[tr]
        dev = device()
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
        hyps = fit_folds(t(Xb), Yb, [len(tr) for tr, _ in splits], pb["kind"], pb["ls_prior"], pb["noise_prior"],
                         pb["standardize"], outputscale_prior=pb["os_prior"], scaled=pb["scaled"])
        Xall, Xn_all = t(Xt), t((Xt - lo0) / (hi0 - lo0))
        out = []
        for ch in member_chunks(B, nmax, d):
            mask = np.zeros((len(ch), n), dtype=bool)
            folded = []
            for k, j in enumerate(ch):
                mask[k, splits[j][0]] = True
                lo, hi = bounds[j]
                h = fold_outputscale(hyps[j])
                # the fold's Normalize bounds folded into its lengthscales: the stationary kernels
                # see (x - x') / ((hi - lo) ls) only
                folded.append(GPHyper(lengthscale=np.asarray(h.lengthscale) * ((hi - lo) / (hi0 - lo0)), noise=h.noise,
                                      constant=h.constant, y_mean=h.y_mean, y_std=h.y_std))
            gp = GPBatch(Xn_all, t(np.repeat(y[:, None], len(ch), 1)), folded, pb["kind"],
                         t(lo0), t(hi0), mask=mask)
            mean, var = gp.posterior(Xall, observation_noise=True)
            mean, sd = mean.cpu().numpy(), np.sqrt(var.cpu().numpy())
            for k, j in enumerate(ch):
                tr, te = splits[j]
                pred = {part: pd.DataFrame({f"{key}_pred": mean[k, rows], f"{key}_sd": sd[k, rows]},
                                           index=experiments.index[rows])
                        for part, rows in (("train", tr), ("test", te))}

                def surrogate(j=j, tr=tr):
                    sur = copy.copy(self)
                    sur._set_state(Xt[tr], y[tr], *bounds[j], pb["kind"], hyps[j])
                    return sur

                out.append((surrogate, pred))
        return out

    # ---- dump / load ------------------------------------------------------------------
    def dumps(self) -> str:
        if not self.is_fitted:
            raise ValueError("Model is not fitted/available yet.")
        buf = io.BytesIO()
        s = self.state
        np.savez(buf, X=s["X"], y=s["y"], lo=s["lo"], hi=s["hi"], lengthscale=s["lengthscale"])
        meta = {"format": "everest_amd.SingleTaskGP/1", "kind": s["kind"], "noise": s["noise"],
                "constant": s["constant"], "y_mean": s["y_mean"], "y_std": s["y_std"],
                "arrays": base64.b64encode(buf.getvalue()).decode()}
        if "outputscale" in s:       # optional key, last: a dump without a scale is what it was
            meta["outputscale"] = s["outputscale"]
        return base64.b64encode(json.dumps(meta).encode()).decode()

    def loads(self, data: str):
        meta = json.loads(base64.b64decode(data.encode()).decode())
        if meta.get("format") != "everest_amd.SingleTaskGP/1":
            raise ValueError("unknown surrogate dump format (BoTorch pickles cannot be loaded without BoTorch)")
        arr = np.load(io.BytesIO(base64.b64decode(meta["arrays"])), allow_pickle=False)
        hyp = GPHyper(lengthscale=arr["lengthscale"], noise=meta["noise"], constant=meta["constant"],
                      y_mean=meta["y_mean"], y_std=meta["y_std"], outputscale=meta.get("outputscale"))
        self._set_state(arr["X"], arr["y"], arr["lo"], arr["hi"], meta["kind"], hyp)


class MixedSingleTaskGPSurrogate:
    """Mixed continuous / categorical exact GP for one output
    (bofire/surrogates/mixed_single_task_gp.py:27-112 on [upstream] BoTorch MixedSingleTaskGP;
    the model is restated in gp.py).  The transformed (one-hot) row is split on the host into the
    continuous columns, normalised with the bounds of get_scaler as SingleTaskGPSurrogate does,
    and one category code per categorical feature: the arg-max of its one-hot block, the first
    on ties ([upstream] OneHotToNumeric).  Needs at least one continuous and one categorical
    input; up to 32 continuous columns and 8 categorical features."""

    FORMAT = "everest_amd.MixedSingleTaskGP/1"

    def __init__(self, data_model: dm.MixedSingleTaskGPSurrogate):
        self.data_model = data_model
        self.inputs = data_model.inputs
        self.outputs = data_model.outputs
        self.continuous_kernel = data_model.continuous_kernel
        self.categorical_kernel = data_model.categorical_kernel
        self.noise_prior = data_model.noise_prior
        self.scaler = data_model.scaler
        self.output_scaler = data_model.output_scaler
        self.input_preprocessing_specs = {k: v.value if hasattr(v, "value") else v
                                          for k, v in data_model.input_preprocessing_specs.items()}
        f2i, _ = self.inputs._transform_info(self.input_preprocessing_specs)
        cat_keys = [k for k in self.inputs.get_keys(dm.CategoricalInput)
                    if self.input_preprocessing_specs.get(k) == CategoricalEncodingEnum.ONE_HOT.value]
        self._cat_blocks = [np.asarray(f2i[k]) for k in cat_keys]
        self._cont_cols = np.asarray([j for k in self.inputs.get_keys() if k not in cat_keys for j in f2i[k]],
                                     dtype=np.int64)
        if len(self._cont_cols) < 1 or len(self._cat_blocks) < 1:
            raise ValueError("MixedSingleTaskGPSurrogate needs at least one continuous and one categorical input")
        self.state: Optional[dict] = None
        self.gp = None
        if data_model.dump is not None:
            self.loads(data_model.dump)

    @property
    def is_fitted(self) -> bool:
        return self.state is not None

    @property
    def output_key(self) -> str:
        return self.outputs.get_keys()[0]

    # ---- transforms ----------------------------------------------------------------
    _bounds = SingleTaskGPSurrogate._bounds
    transform_inputs = SingleTaskGPSurrogate.transform_inputs
    _preprocess_experiments = SingleTaskGPSurrogate._preprocess_experiments
    _fit_data = SingleTaskGPSurrogate._fit_data

    def split_inputs(self, Xt: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(Xc, C) of transformed rows: the normalised continuous columns (n x dc) and the int32
        category codes (n x nc).  lo / hi: the Normalize bounds of all transformed columns."""
        cc = self._cont_cols
        Xc = (Xt[:, cc] - lo[cc]) / (hi[cc] - lo[cc])
        C = np.stack([np.argmax(Xt[:, blk], axis=1) for blk in self._cat_blocks], axis=1).astype(np.int32)
        return np.ascontiguousarray(Xc), np.ascontiguousarray(C)

    # ---- fit -------------------------------------------------------------------------
    def fit(self, experiments: pd.DataFrame, options: Optional[dict] = None):
        """TrainableSurrogate.fit (bofire/surrogates/trainable.py:24-42): valid rows of this output."""
        X, Y = self._fit_data(experiments)
        self._fit(X, Y, options)

    def _fit(self, X: pd.DataFrame, Y: pd.DataFrame, options: Optional[dict] = None):
        from .gp import fit_mixed

        Xt = self.transform_inputs(X)
        lo, hi = self._bounds(X)
        y = Y.values[:, 0].astype(np.float64)
        Xc, C = self.split_inputs(Xt, lo, hi)
        dev = device()
        kernel = self.continuous_kernel
        kind = kernel_kind(kernel)
        hyp = fit_mixed(torch.as_tensor(Xc, device=dev), torch.as_tensor(C, device=dev), y, kind,
                        map_prior(getattr(kernel, "lengthscale_prior", None), Xc.shape[1]),
                        map_prior(self.noise_prior, 1), ard=kernel.ard, options=options,
                        standardize=self.output_scaler == ScalerEnum.STANDARDIZE)
        self._set_state(Xt, y, lo, hi, kind, hyp)

    def _set_state(self, Xt, y, lo, hi, kind, hyp):
        self.state = dict(X=np.asarray(Xt), y=np.asarray(y), lo=np.asarray(lo), hi=np.asarray(hi), kind=int(kind),
                          params=np.asarray(hyp.params, dtype=np.float64), noise=float(hyp.noise),
                          constant=float(hyp.constant), y_mean=float(hyp.y_mean), y_std=float(hyp.y_std))
        self.gp = self._build_gp()

    def hyper(self):
        from .gp import MixedGPHyper

        s = self.state
        return MixedGPHyper(params=s["params"], noise=s["noise"], constant=s["constant"], y_mean=s["y_mean"],
                            y_std=s["y_std"])

    def _build_gp(self):
        from .gp import MixedGPBatch

        s = self.state
        dev = device()
        Xc, C = self.split_inputs(s["X"], s["lo"], s["hi"])
        gp = MixedGPBatch(torch.as_tensor(Xc, device=dev), torch.as_tensor(C, device=dev),
                          torch.as_tensor(s["y"][:, None], dtype=torch.float64, device=dev), [self.hyper()],
                          s["kind"])
        return gp.set_layout(s["lo"], s["hi"], self._cont_cols, self._cat_blocks)

    # ---- predict ----------------------------------------------------------------------
    def predict(self, experiments: pd.DataFrame) -> pd.DataFrame:
        """Surrogate.predict (bofire/surrogates/surrogate.py:39-67): posterior(observation_noise=True)."""
        if not self.is_fitted:
            raise ValueError("Model is not fitted/available yet.")
        Xt = self.transform_inputs(experiments[self.inputs.get_keys()])
        Xc, C = self.split_inputs(Xt, self.state["lo"], self.state["hi"])
        dev = self.gp.device
        mean, var = self.gp.posterior(torch.as_tensor(Xc, device=dev), torch.as_tensor(C, device=dev),
                                      observation_noise=True)
        key = self.output_key
        return pd.DataFrame({f"{key}_pred": mean[0].cpu().numpy(), f"{key}_sd": np.sqrt(var[0].cpu().numpy())},
                            index=experiments.index)

    # ---- cross-validation --------------------------------------------------------------
    def cross_validate(self, experiments: pd.DataFrame, folds: int = -1, include_X: bool = False,
                       include_labcodes: bool = False, random_state: Optional[int] = None,
                       stratified_feature: Optional[str] = None, group_split_column: Optional[str] = None,
                       hooks: Optional[Dict[str, Callable]] = None,
                       hook_kwargs: Optional[Dict[str, Dict[str, Any]]] = None
                       ) -> Tuple[CvResults, CvResults, Dict[str, list]]:
        """TrainableSurrogate.cross_validate (bofire/surrogates/trainable.py:79-339), arguments and
        return value as SingleTaskGPSurrogate.cross_validate: the plain sequential loop, a fresh
        surrogate per fold.  This surrogate's own fitted state is left as it was."""
        return run_cross_validation(self, lambda ex, splits: cv_sequential(self, ex, splits), experiments, folds,
                                    include_X, include_labcodes, random_state, stratified_feature,
                                    group_split_column, hooks, hook_kwargs)

    # ---- dump / load ------------------------------------------------------------------
    def dumps(self) -> str:
        if not self.is_fitted:
            raise ValueError("Model is not fitted/available yet.")
        buf = io.BytesIO()
        s = self.state
        np.savez(buf, X=s["X"], y=s["y"], lo=s["lo"], hi=s["hi"], params=s["params"])
        meta = {"format": self.FORMAT, "kind": s["kind"], "noise": s["noise"], "constant": s["constant"],
                "y_mean": s["y_mean"], "y_std": s["y_std"], "arrays": base64.b64encode(buf.getvalue()).decode()}
        return base64.b64encode(json.dumps(meta).encode()).decode()

    def loads(self, data: str):
        from .gp import MixedGPHyper

        meta = json.loads(base64.b64decode(data.encode()).decode())
        if meta.get("format") != self.FORMAT:
            raise ValueError(f"not a {self.FORMAT} dump (format {meta.get('format')!r})")
        arr = np.load(io.BytesIO(base64.b64decode(meta["arrays"])), allow_pickle=False)
        hyp = MixedGPHyper(params=arr["params"], noise=meta["noise"], constant=meta["constant"],
                           y_mean=meta["y_mean"], y_std=meta["y_std"])
        self._set_state(arr["X"], arr["y"], arr["lo"], arr["hi"], meta["kind"], hyp)


class DotProductGPSurrogate:
    """Exact GP with a dot-product kernel for one output: the device side of ``LinearSurrogate``
    (k = v <x, x'>) and ``PolynomialSurrogate`` (k = (<x, x'> + c)^p, 1 <= p <= 8), which the
    reference maps onto SingleTaskGPSurrogate with a gpytorch LinearKernel / PolynomialKernel
    (bofire/surrogates/mapper.py; the model is restated in gp.py).  Inputs are transformed and
    normalised as SingleTaskGPSurrogate does."""

    FORMAT = "everest_amd.DotProductGP/1"

    def __init__(self, data_model):
        from .gp import check_dot_power

        self.data_model = data_model
        self.inputs = data_model.inputs
        self.outputs = data_model.outputs
        self.kernel = data_model.kernel
        if self.kernel.features is not None:
            raise NotImplementedError("kernel.features (a kernel on a subset of the inputs) is out of scope for the "
                                      "MI355X build")
        if isinstance(self.kernel, dm.LinearKernel):
            self.power, self.theta_prior = 0, self.kernel.variance_prior
        else:
            if self.kernel.power < 1:
                raise NotImplementedError(f"PolynomialKernel power must be an integer 1 <= p <= 8 on the device, "
                                          f"got {self.kernel.power}")
            self.power, self.theta_prior = check_dot_power(self.kernel.power), self.kernel.offset_prior
        self.noise_prior = data_model.noise_prior
        self.scaler = data_model.scaler
        self.output_scaler = data_model.output_scaler
        self.input_preprocessing_specs = {k: v.value if hasattr(v, "value") else v
                                          for k, v in data_model.input_preprocessing_specs.items()}
        self.state: Optional[dict] = None
        self.gp = None
        if data_model.dump is not None:
            self.loads(data_model.dump)

    @property
    def is_fitted(self) -> bool:
        return self.state is not None

    @property
    def output_key(self) -> str:
        return self.outputs.get_keys()[0]

    # ---- transforms ----------------------------------------------------------------
    _bounds = SingleTaskGPSurrogate._bounds
    transform_inputs = SingleTaskGPSurrogate.transform_inputs
    _preprocess_experiments = SingleTaskGPSurrogate._preprocess_experiments
    _fit_data = SingleTaskGPSurrogate._fit_data

    # ---- fit -------------------------------------------------------------------------
    def fit(self, experiments: pd.DataFrame, options: Optional[dict] = None):
        """TrainableSurrogate.fit (bofire/surrogates/trainable.py:24-42): valid rows of this output."""
        X, Y = self._fit_data(experiments)
        self._fit(X, Y, options)

    def _fit(self, X: pd.DataFrame, Y: pd.DataFrame, options: Optional[dict] = None):
        from .gp import fit_dot

        Xt = self.transform_inputs(X)
        lo, hi = self._bounds(X)
        y = Y.values[:, 0].astype(np.float64)
        Xn = torch.as_tensor((Xt - lo) / (hi - lo), dtype=torch.float64, device=device())
        hyp = fit_dot(Xn, y, self.power, map_prior(self.theta_prior, 1), map_prior(self.noise_prior, 1),
                      options=options, standardize=self.output_scaler == ScalerEnum.STANDARDIZE)
        self._set_state(Xt, y, lo, hi, hyp)

    def _set_state(self, Xt, y, lo, hi, hyp):
        self.state = dict(X=np.asarray(Xt), y=np.asarray(y), lo=np.asarray(lo), hi=np.asarray(hi),
                          power=int(hyp.power), theta=float(hyp.theta), noise=float(hyp.noise),
                          constant=float(hyp.constant), y_mean=float(hyp.y_mean), y_std=float(hyp.y_std))
        self.gp = self._build_gp()

    def hyper(self):
        from .gp import DotGPHyper

        s = self.state
        return DotGPHyper(power=s["power"], theta=s["theta"], noise=s["noise"], constant=s["constant"],
                          y_mean=s["y_mean"], y_std=s["y_std"])

    def _build_gp(self):
        from .gp import DotGPBatch

        s = self.state
        dev = device()
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
        Xn = t((s["X"] - s["lo"]) / (s["hi"] - s["lo"]))
        return DotGPBatch(Xn, t(s["y"][:, None]), [self.hyper()], t(s["lo"]), t(s["hi"]))

    # ---- predict ----------------------------------------------------------------------
    def predict(self, experiments: pd.DataFrame) -> pd.DataFrame:
        """Surrogate.predict (bofire/surrogates/surrogate.py:39-67): posterior(observation_noise=True)."""
        if not self.is_fitted:
            raise ValueError("Model is not fitted/available yet.")
        Xt = self.transform_inputs(experiments[self.inputs.get_keys()])
        mean, var = self.gp.posterior(torch.as_tensor(Xt, dtype=torch.float64, device=self.gp.device),
                                      observation_noise=True)
        key = self.output_key
        return pd.DataFrame({f"{key}_pred": mean[0].cpu().numpy(), f"{key}_sd": np.sqrt(var[0].cpu().numpy())},
                            index=experiments.index)

    # ---- cross-validation --------------------------------------------------------------
    def cross_validate(self, experiments: pd.DataFrame, folds: int = -1, include_X: bool = False,
                       include_labcodes: bool = False, random_state: Optional[int] = None,
                       stratified_feature: Optional[str] = None, group_split_column: Optional[str] = None,
                       hooks: Optional[Dict[str, Callable]] = None,
                       hook_kwargs: Optional[Dict[str, Dict[str, Any]]] = None
                       ) -> Tuple[CvResults, CvResults, Dict[str, list]]:
        """TrainableSurrogate.cross_validate (bofire/surrogates/trainable.py:79-339), arguments and
        return value as SingleTaskGPSurrogate.cross_validate: the plain sequential loop, a fresh
        surrogate per fold.  This surrogate's own fitted state is left as it was."""
        return run_cross_validation(self, lambda ex, splits: cv_sequential(self, ex, splits), experiments, folds,
                                    include_X, include_labcodes, random_state, stratified_feature,
                                    group_split_column, hooks, hook_kwargs)

    # ---- dump / load ------------------------------------------------------------------
    def dumps(self) -> str:
        if not self.is_fitted:
            raise ValueError("Model is not fitted/available yet.")
        buf = io.BytesIO()
        s = self.state
        np.savez(buf, X=s["X"], y=s["y"], lo=s["lo"], hi=s["hi"])
        meta = {"format": self.FORMAT, "power": s["power"], "theta": s["theta"], "noise": s["noise"],
                "constant": s["constant"], "y_mean": s["y_mean"], "y_std": s["y_std"],
                "arrays": base64.b64encode(buf.getvalue()).decode()}
        return base64.b64encode(json.dumps(meta).encode()).decode()

    def loads(self, data: str):
        from .gp import DotGPHyper

        try:
            meta = json.loads(base64.b64decode(data.encode()).decode())
        except Exception as e:
            raise ValueError(f"not a {self.FORMAT} dump") from e
        if not isinstance(meta, dict) or meta.get("format") != self.FORMAT:
            raise ValueError(f"not a {self.FORMAT} dump (format "
                             f"{meta.get('format') if isinstance(meta, dict) else None!r})")
        if int(meta["power"]) != self.power:
            raise ValueError(f"dump of a power-{meta['power']} model does not fit this surrogate's kernel "
                             f"(power {self.power})")
        arr = np.load(io.BytesIO(base64.b64decode(meta["arrays"])), allow_pickle=False)
        hyp = DotGPHyper(power=int(meta["power"]), theta=meta["theta"], noise=meta["noise"],
                         constant=meta["constant"], y_mean=meta["y_mean"], y_std=meta["y_std"])
        self._set_state(arr["X"], arr["y"], arr["lo"], arr["hi"], hyp)


class BotorchSurrogates:
    """bofire/surrogates/botorch_surrogates.py:19-128."""

    def __init__(self, data_model: dm.BotorchSurrogates):
        self.surrogates = [map(s) for s in data_model.all_surrogates]

    def fit(self, experiments: pd.DataFrame):
        """Fits the per-output GPs (independent problems, as in the reference's sequential
        loop, bofire/surrogates/botorch_surrogates.py).  Outputs observed on the same rows with
        the same kernel, priors and scalers (the usual case) are fitted in lock-step by
        gp.fit_batch: one L-BFGS-B per output, one batched MLL launch chain per round.  Others
        run concurrently, one host thread and one HIP stream per output (EVR_FIT_THREADS=1:
        sequentially); EVR_FIT_BATCH=0 disables the lock-step fit."""
        import os
        from concurrent.futures import ThreadPoolExecutor

        from .gp import fit_batch

        # mixed members: one after another (their MLL runs op by op, there is no lock-step plan)
        for s in self.surrogates:
            if isinstance(s, MixedSingleTaskGPSurrogate):
                s.fit(experiments)
        rest = [s for s in self.surrogates if not isinstance(s, MixedSingleTaskGPSurrogate)]
        if not rest:
            return
        if os.environ.get("EVR_FIT_BATCH", "1") != "0" and len(rest) > 1 and torch.cuda.is_available():
            probs = [(s, s._fit_problem(*s._fit_data(experiments))) for s in rest]
            groups = {}
            for s, pb in probs:
                key = (pb["Xt"].shape, pb["Xt"].tobytes(), pb["lo"].tobytes(), pb["hi"].tobytes(), pb["kind"],
                       pb["ls_prior"], pb["noise_prior"], pb["standardize"], pb["scaled"], pb["os_prior"])
                groups.setdefault(key, []).append((s, pb))
            rest = []
            for members in groups.values():
                if len(members) == 1:
                    rest.append(members[0][0])
                    continue
                pb0 = members[0][1]
                Xn = torch.as_tensor((pb0["Xt"] - pb0["lo"]) / (pb0["hi"] - pb0["lo"]), dtype=torch.float64,
                                     device=device())
                hyps = fit_batch(Xn, np.stack([pb["y"] for _, pb in members], 1), pb0["kind"], pb0["ls_prior"],
                                 pb0["noise_prior"], standardize=pb0["standardize"],
                                 outputscale_prior=pb0["os_prior"], scaled=pb0["scaled"])
                for (s, pb), h in zip(members, hyps):
                    s._set_state(pb["Xt"], pb["y"], pb["lo"], pb["hi"], pb["kind"], h)
            if not rest:
                return

        workers = int(os.environ.get("EVR_FIT_THREADS", "0") or 0) or len(rest)
        if workers <= 1 or len(rest) <= 1 or not torch.cuda.is_available():
            for s in rest:
                s.fit(experiments)
            return
        dev = device()

        def run(s):
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                s.fit(experiments)
            stream.synchronize()

        with ThreadPoolExecutor(max_workers=min(workers, len(rest))) as ex:
            for f in [ex.submit(run, s) for s in rest]:
                f.result()

    def compatibilize(self, inputs, outputs) -> GPBatch:
        """One batched device model over the outputs in domain order — the ModelListGP of
        bofire/surrogates/botorch_surrogates.py:79-128.  Outputs may be fitted on different
        rows (each surrogate trains on the rows where its output is valid,
        bofire/surrogates/trainable.py:44-66) and with different kernel families: the batch
        holds the union of the training rows with a per-output row mask and a per-output
        family (gp.GPBatch), and each output's Normalize bounds are folded into its
        lengthscales (the stationary kernels see (x - x') / ((hi - lo) ls) only), so every
        member is exactly its own GP."""
        by_key = {s.output_key: s for s in self.surrogates}
        order = [k for k in outputs.get_keys() if k in by_key]
        ss = [by_key[k] for k in order]
        for k, s in zip(order, ss):
            if not s.is_fitted:
                raise ValueError(f"Surrogate for output feature {k} not fitted.")
        n_mixed = sum(isinstance(s, MixedSingleTaskGPSurrogate) for s in ss)
        if n_mixed == len(ss):
            return self._compatibilize_mixed(order, ss, inputs)
        if n_mixed:
            raise NotImplementedError("MixedSingleTaskGPSurrogate and SingleTaskGPSurrogate specs together: one "
                                      "device model holds either mixed or stationary members, not both")
        d = ss[0].state["X"].shape[1]
        if any(s.state["X"].shape[1] != d for s in ss):
            raise NotImplementedError("surrogates over different input subsets are out of scope for the MI355X build")
        X_all, rows = union_rows([s.state["X"] for s in ss])
        n, B = X_all.shape[0], len(ss)
        mask = np.zeros((B, n), dtype=bool)
        Y = np.zeros((n, B))
        for j, (s, r) in enumerate(zip(ss, rows)):
            mask[j, r] = True
            Y[r, j] = s.state["y"]
        s0 = ss[0].state
        lo, hi = np.asarray(s0["lo"], dtype=np.float64), np.asarray(s0["hi"], dtype=np.float64)
        hypers = []
        for s in ss:
            h = s.hyper()
            st = s.state
            if not (np.array_equal(st["lo"], lo) and np.array_equal(st["hi"], hi)):
                h.lengthscale = np.asarray(h.lengthscale) * ((st["hi"] - st["lo"]) / (hi - lo))
            hypers.append(h)
        dev = device()
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
        gp = GPBatch(t((X_all - lo) / (hi - lo)), t(Y), hypers, [s.state["kind"] for s in ss], t(lo), t(hi),
                     mask=mask)
        gp.output_keys = order
        gp.X_raw = X_all
        gp.rows = rows
        return gp

    @staticmethod
    def _compatibilize_mixed(order, ss, inputs):
        """Every surrogate mixed: one gp.MixedGPBatch of B members.  The members share their inputs
        (Xc, C), so they must have been trained on the same rows, with the same continuous kernel
        family and the same Normalize bounds — and over the strategy's own inputs: the chain splits
        candidate rows of ``inputs``' transformed layout with the members' column map."""
        from .gp import MixedGPBatch

        s0 = ss[0]
        st0 = s0.state
        for s in ss:
            own, _ = s.inputs._transform_info(s.input_preprocessing_specs)
            dom, _ = inputs._transform_info(s.input_preprocessing_specs)
            if (list(s.inputs.get_keys()) != list(inputs.get_keys())
                    or any(list(own[k]) != list(dom[k]) for k in inputs.get_keys())):
                raise NotImplementedError("a mixed surrogate over a subset or another order of the domain's inputs "
                                          "is not supported: candidate rows are split with the surrogate's column "
                                          "map")
        for s in ss[1:]:
            st = s.state
            if st["X"].shape != st0["X"].shape or not np.array_equal(st["X"], st0["X"]):
                raise NotImplementedError("mixed surrogates trained on different row sets are not supported (the "
                                          "members of the mixed device model share their training inputs)")
            if st["kind"] != st0["kind"]:
                raise NotImplementedError("mixed surrogates with different continuous kernel families are not "
                                          "supported in one device model")
            if not (np.array_equal(st["lo"], st0["lo"]) and np.array_equal(st["hi"], st0["hi"])
                    and np.array_equal(s._cont_cols, s0._cont_cols)
                    and len(s._cat_blocks) == len(s0._cat_blocks)
                    and all(np.array_equal(a, b) for a, b in zip(s._cat_blocks, s0._cat_blocks))):
                raise NotImplementedError("mixed surrogates with different Normalize bounds or input layouts are "
                                          "not supported in one device model")
        dev = device()
        Xc, C = s0.split_inputs(st0["X"], st0["lo"], st0["hi"])
        Y = np.stack([s.state["y"] for s in ss], 1)
        gp = MixedGPBatch(torch.as_tensor(Xc, device=dev), torch.as_tensor(C, device=dev),
                          torch.as_tensor(Y, dtype=torch.float64, device=dev), [s.hyper() for s in ss], st0["kind"])
        gp.set_layout(st0["lo"], st0["hi"], s0._cont_cols, s0._cat_blocks)
        gp.output_keys = order
        gp.X_raw = np.asarray(st0["X"], dtype=np.float64)
        gp.rows = [np.arange(gp.n) for _ in ss]
        return gp


def union_rows(Xs):
    """Union of the training-row multisets of several outputs, first output's rows first in
    their order, then each later output's rows that no earlier row of equal value (unused by
    that output) covers.  Returns (X_union, [row indices of output j's rows])."""
    out, index, per = [], {}, []
    for X in Xs:
        X = np.asarray(X, dtype=np.float64)
        used = {}
        ids = np.empty(X.shape[0], dtype=np.int64)
        for i, row in enumerate(X):
            key = row.tobytes()
            lst = index.setdefault(key, [])
            k = used.get(key, 0)
            if k == len(lst):
                lst.append(len(out))
                out.append(row)
            ids[i] = lst[k]
            used[key] = k + 1
        per.append(ids)
    return np.asarray(out, dtype=np.float64).reshape(-1, Xs[0].shape[1]), per


def map(data_model):
    """bofire/surrogates/mapper.py:21-44 (SingleTaskGPSurrogate, MixedSingleTaskGPSurrogate, and
    LinearSurrogate / PolynomialSurrogate, which share DotProductGPSurrogate)."""
    if isinstance(data_model, dm.SingleTaskGPSurrogate):
        return SingleTaskGPSurrogate(data_model)
    if isinstance(data_model, (dm.LinearSurrogate, dm.PolynomialSurrogate)):
        return DotProductGPSurrogate(data_model)
    if isinstance(data_model, dm.MixedSingleTaskGPSurrogate):
        return MixedSingleTaskGPSurrogate(data_model)
    if isinstance(data_model, dm.BotorchSurrogates):
        return BotorchSurrogates(data_model)
    raise NotImplementedError(f"{type(data_model).__name__} is out of scope for the MI355X build")
