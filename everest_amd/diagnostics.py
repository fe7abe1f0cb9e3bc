"""Cross-validation results and their regression metrics — the containers
``SingleTaskGPSurrogate.cross_validate`` returns (bofire/surrogates/diagnostics.py: ``CvResult``,
``CvResults`` and the seven regression metrics), over numpy / scipy.stats only.

UQ metrics, classification metrics and ``CrossValidationValues`` are out of scope.
"""
from __future__ import annotations

import warnings
from enum import Enum
from typing import Optional, Sequence

import numpy as np
import pandas as pd


class RegressionMetricsEnum(Enum):
    """bofire/data_models/enum.py RegressionMetricsEnum."""
    R2 = "R2"
    MAE = "MAE"
    MSD = "MSD"
    MAPE = "MAPE"
    PEARSON = "PEARSON"
    SPEARMAN = "SPEARMAN"
    FISHER = "FISHER"


def _mae(observed: np.ndarray, predicted: np.ndarray) -> float:
    return float(np.mean(np.abs(observed - predicted)))


def _msd(observed: np.ndarray, predicted: np.ndarray) -> float:
    return float(np.mean((observed - predicted) ** 2))


def _r2(observed: np.ndarray, predicted: np.ndarray) -> float:
    """Coefficient of determination 1 - SS_res / SS_tot; constant observations give 1 for exact
    predictions and 0 otherwise (the convention of sklearn.metrics.r2_score)."""
    res = float(np.sum((observed - predicted) ** 2))
    tot = float(np.sum((observed - np.mean(observed)) ** 2))
    if tot == 0.0:
        return 1.0 if res == 0.0 else 0.0
    return 1.0 - res / tot


def _mape(observed: np.ndarray, predicted: np.ndarray) -> float:
    """mean |o - p| / max(|o|, eps): a fraction, not a percentage, and finite at o = 0."""
    return float(np.mean(np.abs(observed - predicted) / np.maximum(np.abs(observed), np.finfo(np.float64).eps)))


def _pearson(observed: np.ndarray, predicted: np.ndarray) -> float:
    from scipy.stats import pearsonr

    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")     # constant input: rho is NaN, which is the answer
        return float(pearsonr(predicted, observed)[0])


def _spearman(observed: np.ndarray, predicted: np.ndarray) -> float:
    from scipy.stats import spearmanr

    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(spearmanr(predicted, observed)[0])


def _fisher(observed: np.ndarray, predicted: np.ndarray) -> float:
    """p value of Fisher's exact test (one-sided) that the model tells the top half of the
    observations from the bottom half: the 2 x 2 table counts how many of the n // 2 largest
    predictions are among the n // 2 largest observations.  Small p: it can."""
    from scipy.stats import fisher_exact

    n, half = len(observed), len(observed) // 2
    top_obs = set(np.argsort(observed)[n - half:].tolist())
    top_pred = set(np.argsort(predicted)[n - half:].tolist())
    both = len(top_obs & top_pred)
    miss = half - both
    table = np.array([[both, miss], [miss, (n - half) - miss]])
    return float(fisher_exact(table, alternative="greater")[1])


METRICS = {RegressionMetricsEnum.MAE: _mae, RegressionMetricsEnum.MSD: _msd, RegressionMetricsEnum.R2: _r2,
           RegressionMetricsEnum.MAPE: _mape, RegressionMetricsEnum.PEARSON: _pearson,
           RegressionMetricsEnum.SPEARMAN: _spearman, RegressionMetricsEnum.FISHER: _fisher}
DEFAULT_METRICS = (RegressionMetricsEnum.MAE, RegressionMetricsEnum.MSD, RegressionMetricsEnum.R2,
                   RegressionMetricsEnum.MAPE, RegressionMetricsEnum.PEARSON, RegressionMetricsEnum.SPEARMAN,
                   RegressionMetricsEnum.FISHER)


def _numeric(s: pd.Series) -> bool:
    return pd.api.types.is_numeric_dtype(s) and not pd.api.types.is_bool_dtype(s)


class CvResult:
    """One fold: observed and predicted values of output ``key``, optionally the predictive
    standard deviation, the labcodes and the inputs of the same rows."""

    OPTIONAL = ("standard_deviation", "labcodes", "X")

    def __init__(self, key: str, observed: pd.Series, predicted: pd.Series,
                 standard_deviation: Optional[pd.Series] = None, labcodes: Optional[pd.Series] = None,
                 X: Optional[pd.DataFrame] = None):
        for name, s in (("observed", observed), ("predicted", predicted), ("standard_deviation", standard_deviation)):
            if s is not None and not _numeric(s):
                raise ValueError(f"Not all values of {name} are numerical")
        n = len(predicted)
        if len(observed) != n:
            raise ValueError(f"Predicted values has length {n} whereas observed has length {len(observed)}")
        for name, v in (("standard_deviation", standard_deviation), ("labcodes", labcodes), ("X", X)):
            if v is not None and len(v) != n:
                raise ValueError(f"Predicted values has length {n} whereas {name} has length {len(v)}")
        self.key = key
        self.observed = observed
        self.predicted = predicted
        self.standard_deviation = standard_deviation
        self.labcodes = labcodes
        self.X = X

    @property
    def n_samples(self) -> int:
        return len(self.observed)

    def get_metric(self, metric: RegressionMetricsEnum) -> float:
        if self.n_samples == 1:
            warnings.warn("Metric cannot be calculated for only one sample. Null value will be returned")
            return float("nan")
        return METRICS[RegressionMetricsEnum(metric)](np.asarray(self.observed.values, dtype=np.float64),
                                                      np.asarray(self.predicted.values, dtype=np.float64))


class CvResults:
    """All folds of one cross-validation run (at least two, of the same output, and either all
    or none of them carrying each optional field)."""

    def __init__(self, results: Sequence[CvResult]):
        results = list(results)
        if len(results) < 2:
            raise ValueError("`results` sequence has to contain at least two elements.")
        first = results[0]
        if any(r.key != first.key for r in results):
            raise ValueError("`CvResult` objects do not match.")
        for field in CvResult.OPTIONAL:
            if len({getattr(r, field) is None for r in results}) > 1:
                raise ValueError(f"Either all or none `CvResult` objects contain {field}.")
        if first.X is not None and any(sorted(r.X.columns) != sorted(first.X.columns) for r in results):
            raise ValueError("Columns of X do not match.")
        self.results = results

    def __len__(self) -> int:
        return len(self.results)

    def __iter__(self):
        return iter(self.results)

    def __getitem__(self, i) -> CvResult:
        return self.results[i]

    @property
    def key(self) -> str:
        return self.results[0].key

    @property
    def is_loo(self) -> bool:
        """Leave-one-out: every fold holds exactly one sample."""
        return all(r.n_samples == 1 for r in self.results)

    def _combine_folds(self) -> CvResult:
        """The folds' rows as one CvResult, in fold order, re-indexed 0..N-1."""
        def cat(field):
            parts = [getattr(r, field) for r in self.results]
            return None if parts[0] is None else pd.concat(parts, ignore_index=True)

        return CvResult(key=self.key, observed=cat("observed"), predicted=cat("predicted"),
                        standard_deviation=cat("standard_deviation"), labcodes=cat("labcodes"), X=cat("X"))

    def get_metric(self, metric: RegressionMetricsEnum, combine_folds: bool = True) -> pd.Series:
        """One value over the combined folds (``combine_folds``, and always for LOO, whose
        one-sample folds have no metric of their own), else one value per fold."""
        metric = RegressionMetricsEnum(metric)
        if combine_folds or self.is_loo:
            return pd.Series(self._combine_folds().get_metric(metric), name=metric.name)
        return pd.Series([r.get_metric(metric) for r in self.results], name=metric.name)

    def get_metrics(self, metrics: Sequence[RegressionMetricsEnum] = DEFAULT_METRICS,
                    combine_folds: bool = True) -> pd.DataFrame:
        return pd.concat([self.get_metric(m, combine_folds) for m in metrics], axis=1)
