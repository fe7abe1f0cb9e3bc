from .domain import (BaseModel, CategoricalInput, CloseToTargetObjective, ConstrainedObjective, Constraints, ConstraintNotFulfilledError,
                     ContinuousInput, ContinuousOutput, Domain, Inputs, LinearEqualityConstraint,
                     LinearInequalityConstraint, MaximizeObjective, MaximizeSigmoidObjective, MinimizeObjective,
                     MinimizeSigmoidObjective, MovingMaximizeSigmoidObjective, Outputs, TargetObjective)
from .models import (ActiveLearningStrategy, AdditiveSoboStrategy, AnyActiveLearningAcquisitionFunction, AnyStrategy, BotorchSurrogates, CategoricalEncodingEnum, CategoricalMethodEnum,
                     DimensionalityScaledLogNormalPrior, GammaPrior, HammingDistanceKernel, LinearKernel, LinearSurrogate,
                     LogNormalPrior, MaternKernel, PolynomialKernel, PolynomialSurrogate,
                     MIXED_MODEL_STRATEGIES, MixedSingleTaskGPSurrogate, MultiplicativeAdditiveSoboStrategy, MultiplicativeSoboStrategy, NormalPrior,
                     QehviStrategy, QnehviStrategy, QparegoStrategy, RandomStrategy, RBFKernel, ScalerEnum, SingleTaskGPSurrogate,
                     SoboStrategy, MoboStrategy, qEHVI, qEI, qLogEHVI, qLogEI, qLogNEHVI, qLogNEI, qNEHVI,
                     qNegIntPosVar, qNEI, qPI, qSR, qUCB)
from .models import (AnyKernel, HVARFNER_LENGTHSCALE_PRIOR, HVARFNER_NOISE_PRIOR, MBO_LENGTHCALE_PRIOR, MBO_NOISE_PRIOR,
                     MBO_OUTPUTSCALE_PRIOR, ScaleKernel, THREESIX_LENGTHSCALE_PRIOR, THREESIX_NOISE_PRIOR,
                     THREESIX_SCALE_PRIOR)
