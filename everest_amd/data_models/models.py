"""Kernel, prior, surrogate, acquisition-function and strategy data models on the
GP/qNEHVI path (same names, defaults and ``type`` tags as BoFire):

* kernels  — bofire/data_models/kernels/continuous.py:12-30
* priors   — bofire/data_models/priors/{normal,gamma,api}.py
* surrogate — bofire/data_models/surrogates/single_task_gp.py:106-128,
  trainable_botorch.py:9-30, botorch_surrogates.py
* strategies — bofire/data_models/strategies/predictives/{botorch,qehvi,qnehvi,sobo}.py,
  bofire/data_models/strategies/strategy.py
"""
from __future__ import annotations

import math
from enum import Enum
from typing import Annotated, Dict, List, Literal, Optional, Union

from pydantic import Field, PositiveFloat, PositiveInt, field_validator, model_validator

from .domain import (BaseModel, CategoricalInput, CloseToTargetObjective, ConstrainedObjective, ContinuousOutput,
                     Domain, Inputs, MaximizeObjective, MinimizeObjective, Objective, Outputs)


class CategoricalEncodingEnum(str, Enum):
    ORDINAL = "ORDINAL"
    ONE_HOT = "ONE_HOT"
    DUMMY = "DUMMY"
    DESCRIPTOR = "DESCRIPTOR"


class ScalerEnum(str, Enum):
    NORMALIZE = "NORMALIZE"
    STANDARDIZE = "STANDARDIZE"
    IDENTITY = "IDENTITY"


class CategoricalMethodEnum(str, Enum):
    EXHAUSTIVE = "EXHAUSTIVE"
    FREE = "FREE"


def _is_power_of_two(v: int) -> int:
    if v <= 0 or (v & (v - 1)) != 0:
        raise ValueError(f"{v} is not a power of two")
    return v


IntPowerOfTwo = Annotated[int, Field(gt=0)]


# ---------------------------------------------------------------------------------------
# priors
# ---------------------------------------------------------------------------------------
class NormalPrior(BaseModel):
    type: Literal["NormalPrior"] = "NormalPrior"
    loc: float
    scale: Annotated[float, Field(gt=0)]


class LogNormalPrior(BaseModel):
    type: Literal["LogNormalPrior"] = "LogNormalPrior"
    loc: float
    scale: float


class GammaPrior(BaseModel):
    type: Literal["GammaPrior"] = "GammaPrior"
    concentration: Annotated[float, Field(gt=0)]
    rate: Annotated[float, Field(gt=0)]


class DimensionalityScaledLogNormalPrior(BaseModel):
    """Hvarfner et al. prior (bofire/data_models/priors/normal.py:37-49)."""
    type: Literal["DimensionalityScaledLogNormalPrior"] = "DimensionalityScaledLogNormalPrior"
    loc: Annotated[float, Field(gt=0)] = math.sqrt(2)
    loc_scaling: Annotated[float, Field(gt=0)] = 0.5
    scale: Annotated[float, Field(gt=0)] = math.sqrt(3)
    scale_scaling: float = 0.0


AnyPrior = Annotated[Union[NormalPrior, LogNormalPrior, GammaPrior, DimensionalityScaledLogNormalPrior],
                     Field(discriminator="type")]


def HVARFNER_NOISE_PRIOR():  # bofire/data_models/priors/api.py:50
    return LogNormalPrior(loc=-4, scale=1)


def HVARFNER_LENGTHSCALE_PRIOR():
    return DimensionalityScaledLogNormalPrior()


# ---------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------
class RBFKernel(BaseModel):
    type: Literal["RBFKernel"] = "RBFKernel"
    features: Optional[List[str]] = None
    ard: bool = True
    lengthscale_prior: Optional[AnyPrior] = None


class MaternKernel(BaseModel):
    type: Literal["MaternKernel"] = "MaternKernel"
    features: Optional[List[str]] = None
    ard: bool = True
    nu: float = 2.5
    lengthscale_prior: Optional[AnyPrior] = None

    @field_validator("nu")
    @classmethod
    def _nu(cls, nu):
        if nu not in {0.5, 1.5, 2.5}:
            raise ValueError("nu expected to be 0.5, 1.5, or 2.5")
        return nu


# the stationary kernels of the device GP (RBF / Matérn ARD)
StationaryKernel = Annotated[Union[RBFKernel, MaternKernel], Field(discriminator="type")]


class ScaleKernel(BaseModel):
    """bofire/data_models/kernels/aggregation.py:45-58 around the two stationary kernels:
    k = outputscale * base_kernel, the outputscale fitted (softplus of a raw parameter) under
    ``outputscale_prior``.  Any other base kernel (dot-product, Hamming, a nested ScaleKernel,
    sums and products) is a validation error here."""
    type: Literal["ScaleKernel"] = "ScaleKernel"
    base_kernel: StationaryKernel
    outputscale_prior: Optional[Annotated[Union[GammaPrior, NormalPrior, LogNormalPrior],
                                          Field(discriminator="type")]] = None


AnyKernel = Annotated[Union[RBFKernel, MaternKernel, ScaleKernel], Field(discriminator="type")]


class LinearKernel(BaseModel):
    """bofire/data_models/kernels/continuous.py:32-34.  Not part of AnyKernel: it is the kernel of
    LinearSurrogate only."""
    type: Literal["LinearKernel"] = "LinearKernel"
    features: Optional[List[str]] = None
    variance_prior: Optional[AnyPrior] = None


class PolynomialKernel(BaseModel):
    """bofire/data_models/kernels/continuous.py:37-40.  Not part of AnyKernel: it is the kernel of
    PolynomialSurrogate only."""
    type: Literal["PolynomialKernel"] = "PolynomialKernel"
    features: Optional[List[str]] = None
    offset_prior: Optional[AnyPrior] = None
    power: int = 2


class HammingDistanceKernel(BaseModel):
    """bofire/data_models/kernels/categorical.py:10-12."""
    type: Literal["HammingDistanceKernel"] = "HammingDistanceKernel"
    features: Optional[List[str]] = None
    ard: bool = True


def THREESIX_LENGTHSCALE_PRIOR():  # bofire/data_models/priors/api.py:30-32
    return GammaPrior(concentration=3.0, rate=6.0)


def THREESIX_NOISE_PRIOR():
    return GammaPrior(concentration=1.1, rate=0.05)


def THREESIX_SCALE_PRIOR():
    return GammaPrior(concentration=2.0, rate=0.15)


def MBO_LENGTHCALE_PRIOR():  # bofire/data_models/priors/api.py:38-40 (the reference's spelling)
    return GammaPrior(concentration=2.0, rate=0.2)


def MBO_NOISE_PRIOR():
    return GammaPrior(concentration=2.0, rate=4.0)


def MBO_OUTPUTSCALE_PRIOR():
    return GammaPrior(concentration=2.0, rate=4.0)


# ---------------------------------------------------------------------------------------
# surrogates
# ---------------------------------------------------------------------------------------
class SingleTaskGPSurrogate(BaseModel):
    type: Literal["SingleTaskGPSurrogate"] = "SingleTaskGPSurrogate"
    inputs: Inputs
    outputs: Outputs
    input_preprocessing_specs: Dict[str, CategoricalEncodingEnum] = Field(default_factory=dict, validate_default=True)
    dump: Optional[str] = None
    scaler: ScalerEnum = ScalerEnum.NORMALIZE
    output_scaler: ScalerEnum = ScalerEnum.STANDARDIZE
    kernel: AnyKernel = Field(default_factory=lambda: RBFKernel(ard=True,
                                                                lengthscale_prior=HVARFNER_LENGTHSCALE_PRIOR()))
    noise_prior: AnyPrior = Field(default_factory=HVARFNER_NOISE_PRIOR)

    @field_validator("output_scaler")
    @classmethod
    def _os(cls, v):
        if v == ScalerEnum.NORMALIZE:
            raise ValueError("Normalize is not supported as an output transform.")
        return v

    @model_validator(mode="after")
    def _specs(self):
        """Botorch models one-hot encode categoricals (bofire/data_models/surrogates/botorch.py:19-60)."""
        specs = dict(self.input_preprocessing_specs)
        for key in self.inputs.get_keys(CategoricalInput):
            if specs.get(key, CategoricalEncodingEnum.ONE_HOT) != CategoricalEncodingEnum.ONE_HOT:
                raise ValueError("Botorch based models have to use one hot encodings for categoricals")
            specs[key] = CategoricalEncodingEnum.ONE_HOT
        self.__dict__["input_preprocessing_specs"] = specs
        if len(self.outputs) != 1:
            raise ValueError("SingleTaskGPSurrogate takes exactly one output")
        return self


class MixedSingleTaskGPSurrogate(BaseModel):
    """bofire/data_models/surrogates/mixed_single_task_gp.py:92-125 (without the hyperconfig): the
    surrogate the reference builds per output for a domain with a CategoricalInput.  The
    categorical kernel is always ARD over the categorical features on the device (the
    reference's surrogate never passes ``categorical_kernel`` on to [upstream] MixedSingleTaskGP)."""
    type: Literal["MixedSingleTaskGPSurrogate"] = "MixedSingleTaskGPSurrogate"
    inputs: Inputs
    outputs: Outputs
    input_preprocessing_specs: Dict[str, CategoricalEncodingEnum] = Field(default_factory=dict, validate_default=True)
    dump: Optional[str] = None
    scaler: ScalerEnum = ScalerEnum.NORMALIZE
    output_scaler: ScalerEnum = ScalerEnum.STANDARDIZE
    continuous_kernel: StationaryKernel = Field(default_factory=lambda: MaternKernel(
        ard=True, nu=2.5, lengthscale_prior=THREESIX_LENGTHSCALE_PRIOR()))
    categorical_kernel: HammingDistanceKernel = Field(default_factory=lambda: HammingDistanceKernel(ard=True))
    noise_prior: AnyPrior = Field(default_factory=THREESIX_NOISE_PRIOR)

    @field_validator("output_scaler")
    @classmethod
    def _os(cls, v):
        if v == ScalerEnum.NORMALIZE:
            raise ValueError("Normalize is not supported as an output transform.")
        return v

    @model_validator(mode="after")
    def _specs(self):
        """Categoricals are one-hot encoded (bofire/data_models/surrogates/botorch.py:19-60) and at
        least one of them is present (mixed_single_task_gp.py:107-115); one continuous output."""
        specs = dict(self.input_preprocessing_specs)
        for key in self.inputs.get_keys(CategoricalInput):
            if specs.get(key, CategoricalEncodingEnum.ONE_HOT) != CategoricalEncodingEnum.ONE_HOT:
                raise ValueError("Botorch based models have to use one hot encodings for categoricals")
            specs[key] = CategoricalEncodingEnum.ONE_HOT
        if CategoricalEncodingEnum.ONE_HOT not in specs.values():
            raise ValueError("MixedSingleTaskGPSurrogate can only be used if at least one one-hot encoded "
                             "categorical feature is present.")
        self.__dict__["input_preprocessing_specs"] = specs
        if len(self.outputs) != 1:
            raise ValueError("MixedSingleTaskGPSurrogate takes exactly one output")
        if not isinstance(self.outputs.features[0], ContinuousOutput):
            raise ValueError("MixedSingleTaskGPSurrogate takes a continuous output")
        return self


class LinearSurrogate(BaseModel):
    """bofire/data_models/surrogates/linear.py:13-18 (without the hyperconfig and aggregations): an
    exact GP with a LinearKernel.  Not part of AnySurrogate: it does not enter strategies."""
    type: Literal["LinearSurrogate"] = "LinearSurrogate"
    inputs: Inputs
    outputs: Outputs
    input_preprocessing_specs: Dict[str, CategoricalEncodingEnum] = Field(default_factory=dict, validate_default=True)
    dump: Optional[str] = None
    scaler: ScalerEnum = ScalerEnum.NORMALIZE
    output_scaler: ScalerEnum = ScalerEnum.STANDARDIZE
    kernel: LinearKernel = Field(default_factory=lambda: LinearKernel())
    noise_prior: AnyPrior = Field(default_factory=lambda: THREESIX_NOISE_PRIOR())

    @field_validator("output_scaler")
    @classmethod
    def _os(cls, v):
        if v == ScalerEnum.NORMALIZE:
            raise ValueError("Normalize is not supported as an output transform.")
        return v

    @model_validator(mode="after")
    def _specs(self):
        """As SingleTaskGPSurrogate: one-hot categoricals, exactly one output."""
        return _one_hot_single_output(self)


class PolynomialSurrogate(BaseModel):
    """bofire/data_models/surrogates/polynomial.py:12-24 (without the hyperconfig and aggregations):
    an exact GP with a PolynomialKernel.  Not part of AnySurrogate: it does not enter strategies."""
    type: Literal["PolynomialSurrogate"] = "PolynomialSurrogate"
    inputs: Inputs
    outputs: Outputs
    input_preprocessing_specs: Dict[str, CategoricalEncodingEnum] = Field(default_factory=dict, validate_default=True)
    dump: Optional[str] = None
    scaler: ScalerEnum = ScalerEnum.NORMALIZE
    output_scaler: ScalerEnum = ScalerEnum.STANDARDIZE
    kernel: PolynomialKernel = Field(default_factory=lambda: PolynomialKernel(power=2))
    noise_prior: AnyPrior = Field(default_factory=lambda: THREESIX_NOISE_PRIOR())

    @field_validator("output_scaler")
    @classmethod
    def _os(cls, v):
        if v == ScalerEnum.NORMALIZE:
            raise ValueError("Normalize is not supported as an output transform.")
        return v

    @model_validator(mode="after")
    def _specs(self):
        """As SingleTaskGPSurrogate: one-hot categoricals, exactly one output."""
        return _one_hot_single_output(self)

    @staticmethod
    def from_power(power: int, inputs: Inputs, outputs: Outputs):
        return PolynomialSurrogate(kernel=PolynomialKernel(power=power), inputs=inputs, outputs=outputs)


def _one_hot_single_output(model):
    """SingleTaskGPSurrogate's model validator for the surrogates that share it
    (bofire/data_models/surrogates/botorch.py:19-60)."""
    specs = dict(model.input_preprocessing_specs)
    for key in model.inputs.get_keys(CategoricalInput):
        if specs.get(key, CategoricalEncodingEnum.ONE_HOT) != CategoricalEncodingEnum.ONE_HOT:
            raise ValueError("Botorch based models have to use one hot encodings for categoricals")
        specs[key] = CategoricalEncodingEnum.ONE_HOT
    model.__dict__["input_preprocessing_specs"] = specs
    if len(model.outputs) != 1:
        raise ValueError(f"{type(model).__name__} takes exactly one output")
    return model


AnySurrogate = Annotated[Union[SingleTaskGPSurrogate], Field(discriminator="type")]


class BotorchSurrogates(BaseModel):
    """``surrogates`` holds the stationary specs and, as before, takes nothing else: a
    MixedSingleTaskGPSurrogate there is a validation error.  Mixed specs travel in
    ``mixed_surrogates`` (the reference keeps both kinds in ``surrogates``; a reference JSON with
    mixed entries there does not load here)."""
    type: Literal["BotorchSurrogates"] = "BotorchSurrogates"
    surrogates: List[AnySurrogate] = Field(default_factory=list)
    mixed_surrogates: List[MixedSingleTaskGPSurrogate] = Field(default_factory=list)

    @property
    def all_surrogates(self) -> list:
        return list(self.surrogates) + list(self.mixed_surrogates)

    @property
    def input_preprocessing_specs(self):
        specs = {}
        for s in self.all_surrogates:
            specs.update(s.input_preprocessing_specs)
        return specs

    @property
    def outputs(self) -> Outputs:
        feats = []
        for s in self.all_surrogates:
            feats += list(s.outputs.features)
        return Outputs(features=feats)


# ---------------------------------------------------------------------------------------
# acquisition functions (bofire/data_models/acquisition_functions/acquisition_function.py)
# ---------------------------------------------------------------------------------------
class _AcqfMC(BaseModel):
    """n_mc_samples must be a power of two (bofire IntPowerOfTwo)."""

    @field_validator("n_mc_samples", check_fields=False)
    @classmethod
    def _p2mc(cls, v):
        return _is_power_of_two(v)


class qEI(_AcqfMC):
    type: Literal["qEI"] = "qEI"
    n_mc_samples: int = 512


class qLogEI(_AcqfMC):
    type: Literal["qLogEI"] = "qLogEI"
    n_mc_samples: int = 512


class qNEI(_AcqfMC):
    type: Literal["qNEI"] = "qNEI"
    prune_baseline: bool = True
    n_mc_samples: int = 512


class qLogNEI(_AcqfMC):
    type: Literal["qLogNEI"] = "qLogNEI"
    prune_baseline: bool = True
    n_mc_samples: int = 512


class qSR(_AcqfMC):
    type: Literal["qSR"] = "qSR"
    n_mc_samples: int = 512


class qUCB(_AcqfMC):
    type: Literal["qUCB"] = "qUCB"
    beta: Annotated[float, Field(ge=0)] = 0.2
    n_mc_samples: int = 512


class qPI(_AcqfMC):
    type: Literal["qPI"] = "qPI"
    tau: PositiveFloat = 1e-3
    n_mc_samples: int = 512


class qEHVI(_AcqfMC):
    type: Literal["qEHVI"] = "qEHVI"
    alpha: Annotated[float, Field(ge=0)] = 0.0
    n_mc_samples: int = 512


class qLogEHVI(_AcqfMC):
    type: Literal["qLogEHVI"] = "qLogEHVI"
    alpha: Annotated[float, Field(ge=0)] = 0.0
    n_mc_samples: int = 512


class qNEHVI(_AcqfMC):
    type: Literal["qNEHVI"] = "qNEHVI"
    alpha: Annotated[float, Field(ge=0)] = 0.0
    prune_baseline: bool = True
    n_mc_samples: int = 512


class qLogNEHVI(_AcqfMC):
    type: Literal["qLogNEHVI"] = "qLogNEHVI"
    alpha: Annotated[float, Field(ge=0)] = 0.0
    prune_baseline: bool = True
    n_mc_samples: int = 512


AnyMultiObjectiveAcquisitionFunction = Annotated[Union[qEHVI, qLogEHVI, qNEHVI, qLogNEHVI],
                                                 Field(discriminator="type")]
AnySingleObjectiveAcquisitionFunction = Annotated[Union[qEI, qLogEI, qNEI, qLogNEI, qSR, qUCB, qPI],
                                                  Field(discriminator="type")]


class qNegIntPosVar(_AcqfMC):
    """bofire/data_models/acquisition_functions/acquisition_function.py:86-89: n_mc_samples is the
    number of integration points; weights (by output key, not normalised) scalarise several
    outputs."""
    type: Literal["qNegIntPosVar"] = "qNegIntPosVar"
    n_mc_samples: IntPowerOfTwo = 512
    weights: Optional[Dict[str, PositiveFloat]] = None


AnyActiveLearningAcquisitionFunction = qNegIntPosVar


# ---------------------------------------------------------------------------------------
# strategies
# ---------------------------------------------------------------------------------------
class Strategy(BaseModel):
    type: str
    domain: Domain
    seed: Optional[Annotated[int, Field(ge=0)]] = None


class RandomStrategy(Strategy):
    type: Literal["RandomStrategy"] = "RandomStrategy"


class BotorchStrategy(Strategy):
    """bofire/data_models/strategies/predictives/botorch.py:77-253 (the fields on this path)."""
    num_restarts: PositiveInt = 8
    num_raw_samples: IntPowerOfTwo = 1024
    maxiter: PositiveInt = 2000
    batch_limit: Optional[PositiveInt] = Field(default=None, validate_default=True)
    descriptor_method: CategoricalMethodEnum = CategoricalMethodEnum.EXHAUSTIVE
    categorical_method: CategoricalMethodEnum = CategoricalMethodEnum.EXHAUSTIVE
    discrete_method: CategoricalMethodEnum = CategoricalMethodEnum.EXHAUSTIVE
    surrogate_specs: BotorchSurrogates = Field(default_factory=BotorchSurrogates, validate_default=True)
    frequency_hyperopt: Annotated[int, Field(ge=0)] = 0
    folds: int = 5

    @field_validator("num_raw_samples")
    @classmethod
    def _p2(cls, v):
        return _is_power_of_two(v)

    @field_validator("batch_limit")
    @classmethod
    def _bl(cls, batch_limit, info):
        return min(batch_limit or info.data["num_restarts"], info.data["num_restarts"])

    @model_validator(mode="after")
    def _surrogates(self):
        """_generate_surrogate_specs: one default surrogate per output without a spec
        (bofire/data_models/strategies/predictives/botorch.py:195-239) — a SingleTaskGPSurrogate,
        or, when the domain has categorical inputs, a MixedSingleTaskGPSurrogate as the reference
        picks (held in ``surrogate_specs.mixed_surrogates``).  The mixed model runs inside the strategies of MIXED_MODEL_STRATEGIES only: the
        others still need explicit SingleTaskGPSurrogate specs (one-hot inputs) for such a domain.
        The FREE categorical method is not compatible with a mixed model (botorch.py:161-166)."""
        specs = self.surrogate_specs
        have = set(specs.outputs.get_keys())
        new, mixed = list(specs.surrogates), list(specs.mixed_surrogates)
        for key in sorted(set(self.domain.outputs.get_keys()) - have):
            outputs = Outputs(features=[self.domain.outputs.get_by_key(key)])
            if len(self.domain.inputs.get(CategoricalInput, exact=True).features):
                if type(self).__name__ not in MIXED_MODEL_STRATEGIES:
                    raise ValueError(f"output `{key}`: categorical inputs need an explicit SingleTaskGPSurrogate "
                                     f"spec (MixedSingleTaskGP is out of scope for {type(self).__name__} on the "
                                     "MI355X build)")
                mixed.append(MixedSingleTaskGPSurrogate(inputs=self.domain.inputs, outputs=outputs))
            else:
                new.append(SingleTaskGPSurrogate(inputs=self.domain.inputs, outputs=outputs))
        specs.__dict__["surrogates"] = new
        specs.__dict__["mixed_surrogates"] = mixed
        for s in new + mixed:
            for k in s.outputs.get_keys():
                if k not in self.domain.outputs.get_keys():
                    raise KeyError(f"surrogate output `{k}` not in domain")
        if self.categorical_method == CategoricalMethodEnum.FREE and mixed:
            raise ValueError("Categorical method FREE not compatible with a a MixedSingleTaskGPModel.")
        return self


# strategies whose acquisitions run on a MixedSingleTaskGPSurrogate (the single-objective chain)
MIXED_MODEL_STRATEGIES = ("SoboStrategy", "AdditiveSoboStrategy", "MultiplicativeSoboStrategy",
                          "MultiplicativeAdditiveSoboStrategy", "QparegoStrategy")


_MO_CONSTRAINED = ("MaximizeObjective", "MinimizeObjective", "MinimizeSigmoidObjective", "MaximizeSigmoidObjective",
                   "TargetObjective", "CloseToTargetObjective")


def _check_objectives(cls, domain: Domain, allowed) -> Domain:
    """bofire/data_models/strategies/strategy.py:26-34 (is_objective_implemented)."""
    for f in domain.outputs.get().features:
        obj = getattr(f, "objective", None)
        if obj is not None and type(obj).__name__ not in allowed:
            raise ValueError(f"Objective `{type(obj)}` is not implemented for strategy `{cls.__name__}`")
    return domain


class MultiobjectiveStrategy(BotorchStrategy):
    @field_validator("domain")
    @classmethod
    def _mo(cls, v):
        feats = v.outputs.get_by_objective([MaximizeObjective, MinimizeObjective, CloseToTargetObjective])
        if len(feats) < 2:
            raise ValueError("At least two output features with MaximizeObjective or MinimizeObjective has to be "
                             "defined in the domain.")
        for f in feats.features:
            if f.objective.w != 1.0:
                raise ValueError(f"Only objectives with weight 1 are supported. Violated by feature {f.key}.")
        return v


class QehviStrategy(MultiobjectiveStrategy):
    type: Literal["QehviStrategy"] = "QehviStrategy"
    num_sobol_samples: IntPowerOfTwo = 512
    ref_point: Optional[Dict[str, float]] = None

    @field_validator("domain")
    @classmethod
    def _objectives(cls, v):
        """bofire/data_models/strategies/predictives/qehvi.py:53-67."""
        return _check_objectives(cls, v, ("MaximizeObjective", "MinimizeObjective"))

    @field_validator("num_sobol_samples")
    @classmethod
    def _p2s(cls, v):
        return _is_power_of_two(v)

    @model_validator(mode="after")
    def _ref(self):
        if self.ref_point is None:
            return self
        keys = self.domain.outputs.get_keys_by_objective([MaximizeObjective, MinimizeObjective,
                                                          CloseToTargetObjective])
        if sorted(keys) != sorted(self.ref_point.keys()):
            raise ValueError(f"Provided refpoint do not match the domain, expected keys: {keys}")
        return self


class QnehviStrategy(QehviStrategy):
    type: Literal["QnehviStrategy"] = "QnehviStrategy"
    alpha: Annotated[float, Field(ge=0, le=0.5)] = 0.0

    @field_validator("domain")
    @classmethod
    def _objectives(cls, v):
        """bofire/data_models/strategies/predictives/qnehvi.py:21-39."""
        return _check_objectives(cls, v, _MO_CONSTRAINED)


class MoboStrategy(MultiobjectiveStrategy):
    """bofire/data_models/strategies/predictives/mobo.py:24-80."""
    type: Literal["MoboStrategy"] = "MoboStrategy"
    ref_point: Optional[Dict[str, float]] = None
    acquisition_function: AnyMultiObjectiveAcquisitionFunction = Field(default_factory=qLogNEHVI)

    @field_validator("domain")
    @classmethod
    def _objectives(cls, v):
        """bofire/data_models/strategies/predictives/mobo.py:60-80."""
        return _check_objectives(cls, v, _MO_CONSTRAINED)

    @model_validator(mode="after")
    def _ref(self):
        if self.ref_point is None:
            return self
        keys = self.domain.outputs.get_keys_by_objective([MaximizeObjective, MinimizeObjective,
                                                          CloseToTargetObjective])
        if sorted(keys) != sorted(self.ref_point.keys()):
            raise ValueError(f"Provided refpoint do not match the domain, expected keys: {keys}")
        return self


class QparegoStrategy(MultiobjectiveStrategy):
    """bofire/data_models/strategies/predictives/qparego.py:27-67."""
    type: Literal["QparegoStrategy"] = "QparegoStrategy"
    acquisition_function: AnySingleObjectiveAcquisitionFunction = Field(default_factory=qNEI)

    @field_validator("domain")
    @classmethod
    def _objectives(cls, v):
        """bofire/data_models/strategies/predictives/qparego.py:37-48."""
        return _check_objectives(cls, v, _MO_CONSTRAINED)


class SoboStrategy(BotorchStrategy):
    """bofire/data_models/strategies/predictives/sobo.py:15-62."""
    type: Literal["SoboStrategy"] = "SoboStrategy"
    acquisition_function: AnySingleObjectiveAcquisitionFunction = Field(default_factory=qLogNEI)

    @field_validator("domain")
    @classmethod
    def validate_is_singleobjective(cls, v):
        """sobo.py:50-62: at most one objective that is not a ConstrainedObjective (the
        reference subtracts the outputs without an objective from that count)."""
        if len(v.outputs) == 1:
            return v
        free = len(v.outputs.get_by_objective(excludes=ConstrainedObjective))
        none = sum(1 for f in v.outputs.get().features if getattr(f, "objective", None) is None)
        if free - none > 1:
            raise ValueError("SOBO strategy can only deal with one no-constraint objective.")
        return v


class AdditiveSoboStrategy(BotorchStrategy):
    """bofire/data_models/strategies/predictives/sobo.py:65-75: the weighted sum of the
    objectives; ``use_output_constraints`` keeps the constrained objectives as separate output
    constraints (True) or absorbs them into the sum (False)."""
    type: Literal["AdditiveSoboStrategy"] = "AdditiveSoboStrategy"
    acquisition_function: AnySingleObjectiveAcquisitionFunction = Field(default_factory=qLogNEI)
    use_output_constraints: bool = True

    @field_validator("domain")
    @classmethod
    def validate_is_multiobjective(cls, v):
        if len(v.outputs.get_by_objective(Objective)) < 2:
            raise ValueError("Additive SOBO strategy requires at least 2 outputs with objectives. Consider SOBO "
                             "strategy instead.")
        return v


def _check_adaptable_weights(self):
    """bofire/data_models/strategies/predictives/sobo.py:78-93 (_CheckAdaptableWeightsMixin): the
    weights are divided by the smallest one, which needs w >= 1e-8.  Deviation: the reference
    raises a TypeError here, from building its pydantic.ValidationError with a message alone;
    this raises the ValueError it means to, with the same message."""
    for f in self.domain.outputs.get_by_objective().features:
        if f.objective.w < 1e-8:
            raise ValueError(f"Weight transformation to (1, inf) requires w>=1e-8 . Violated by feature {f.key}.")
    return self


class MultiplicativeSoboStrategy(BotorchStrategy):
    """bofire/data_models/strategies/predictives/sobo.py:96-105: the product of the objectives,
    each raised to its weight (weights divided by the smallest, so in [1, inf))."""
    type: Literal["MultiplicativeSoboStrategy"] = "MultiplicativeSoboStrategy"
    acquisition_function: AnySingleObjectiveAcquisitionFunction = Field(default_factory=qLogNEI)

    @field_validator("domain")
    @classmethod
    def validate_is_multiobjective(cls, v):
        if len(v.outputs.get_by_objective(Objective)) < 2:
            raise ValueError("Multiplicative SOBO strategy requires at least 2 outputs with objectives. Consider "
                             "SOBO strategy instead.")
        return v

    @model_validator(mode="after")
    def check_adaptable_weights(self):
        return _check_adaptable_weights(self)


class MultiplicativeAdditiveSoboStrategy(BotorchStrategy):
    """bofire/data_models/strategies/predictives/sobo.py:108-135: multiplicative (strict) and
    additive (non-strict) objectives, f1^w1 * f2^w2 * (1 + f3*w3 + f4*w4) for the outputs named in
    ``additive_features``.  A single objective is accepted.  ``use_output_constraints`` is carried
    as in the reference, whose strategy never reads it."""
    type: Literal["MultiplicativeAdditiveSoboStrategy"] = "MultiplicativeAdditiveSoboStrategy"
    acquisition_function: AnySingleObjectiveAcquisitionFunction = Field(default_factory=qLogNEI)
    use_output_constraints: bool = True
    additive_features: List[str] = Field(default_factory=list)

    @field_validator("additive_features")
    @classmethod
    def validate_additive_features(cls, v, info):
        domain = info.data["domain"]
        for feature in v:
            if feature not in domain.outputs.get_keys():
                raise ValueError(f"Feature {feature} is not an output feature of the domain.")
        return v

    @model_validator(mode="after")
    def check_adaptable_weights(self):
        return _check_adaptable_weights(self)


class ActiveLearningStrategy(BotorchStrategy):
    """bofire/data_models/strategies/predictives/active_learning.py:14-62: pure exploration, the
    candidates that most reduce the integrated posterior variance.  Every objective type is
    allowed."""
    type: Literal["ActiveLearningStrategy"] = "ActiveLearningStrategy"
    acquisition_function: AnyActiveLearningAcquisitionFunction = Field(default_factory=qNegIntPosVar)

    @model_validator(mode="after")
    def validate_acquisition_function(self):
        w = self.acquisition_function.weights
        if w is not None and sorted(w.keys()) != sorted(self.domain.outputs.get_keys()):
            raise ValueError("The keys provided for the weights do not match the required keys of the output "
                             "features.")
        return self


AnyStrategy = Annotated[Union[QnehviStrategy, QehviStrategy, MoboStrategy, QparegoStrategy, SoboStrategy,
                              AdditiveSoboStrategy, MultiplicativeSoboStrategy, MultiplicativeAdditiveSoboStrategy,
                              ActiveLearningStrategy, RandomStrategy],
                        Field(discriminator="type")]
