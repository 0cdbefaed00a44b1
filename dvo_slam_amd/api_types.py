"""The reference's value types (dvo::DenseTracker::Config / Result / Stats) and how a C-ABI result unpacks into them."""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib


TERMINATION = {0: "IterationsExceeded", 1: "IncrementTooSmall", 2: "LogLikelihoodDecreased", 3: "TooFewConstraints",
               -1: "unset"}


@dataclass
class Config:
    """dvo::DenseTracker::Config; defaults = dvo_core/src/dense_tracking_config.cpp:27-42."""
    FirstLevel: int = 3
    LastLevel: int = 1
    MaxIterationsPerLevel: int = 100
    Precision: float = 5e-7
    Mu: float = 0.0
    UseInitialEstimate: bool = False
    UseWeighting: bool = True            # dead for match(); kept so callers compile
    UseParallel: bool = False            # dead
    InfluenceFuntionType: int = 2        # TDistribution (dead)
    InfluenceFunctionParam: float = 5.0  # dead
    ScaleEstimatorType: int = 2          # TDistribution (dead)
    ScaleEstimatorParam: float = 5.0     # dead
    IntensityDerivativeThreshold: float = 0.0
    DepthDerivativeThreshold: float = 0.0

    def getNumLevels(self):
        return self.FirstLevel + 1

    def UseEstimateSmoothing(self):
        return self.Mu > 1e-6

    def IsSane(self):
        return self.FirstLevel >= self.LastLevel

    def to_c(self):
        return _lib.Config(self.FirstLevel, self.LastLevel, self.MaxIterationsPerLevel, int(self.UseInitialEstimate),
                           self.Precision, self.Mu, self.IntensityDerivativeThreshold, self.DepthDerivativeThreshold)


@dataclass
class IterationStats:
    Id: int = 0
    ValidConstraints: int = 0
    TDistributionLogLikelihood: float = 0.0
    TDistributionMean: np.ndarray = None
    TDistributionPrecision: np.ndarray = None
    PriorLogLikelihood: float = 0.0
    EstimateIncrement: np.ndarray = None
    EstimateInformation: np.ndarray = None

    def InformationEigenValues(self):
        return np.sort(np.linalg.eigvals(self.EstimateInformation).real)

    def InformationConditionNumber(self):
        ev = self.InformationEigenValues()
        return abs(ev[5] / ev[0])


@dataclass
class LevelStats:
    Id: int = 0
    MaxValidPixels: int = 0
    ValidPixels: int = 0
    TerminationCriterion: int = -1
    Iterations: list = field(default_factory=list)

    def HasIterationWithIncrement(self):   # dense_tracking_config.cpp:138-143
        need = 2 if self.TerminationCriterion in (2, 3) else 1
        return len(self.Iterations) >= need

    def LastIterationWithIncrement(self):
        assert self.HasIterationWithIncrement()
        return self.Iterations[-2] if self.TerminationCriterion == 2 else self.Iterations[-1]

    def LastIteration(self):
        return self.Iterations[-1]


@dataclass
class Stats:
    Levels: list = field(default_factory=list)


class Result:
    """dvo::DenseTracker::Result (dense_tracking.h:125-140, dense_tracking_config.cpp:96-121)."""

    def __init__(self):
        self.Transformation = np.full((4, 4), np.nan)
        self.Transformation[3] = [0, 0, 0, 1]
        self.Information = np.eye(6)
        self.LogLikelihood = np.finfo(np.float64).max
        self.Statistics = Stats()
        self.Entropy = self.ConditionNumber = self.ConstraintRatio = float("nan")
        self.ConstraintRatioAccepted = 0.0

    def isNaN(self):
        return not (np.isfinite(self.Transformation.sum()) and np.isfinite(self.Information.sum()))

    def setIdentity(self):
        self.Transformation = np.eye(4)
        self.Information = np.eye(6)
        self.LogLikelihood = 0.0

    def clearStatistics(self):
        self.Statistics.Levels = []


_RESULT_DTYPE = np.dtype([("transformation", np.float64, (16,)), ("information", np.float64, (36,)), ("loglik", np.float64),
                          ("n_levels", np.int32), ("n_iterations_total", np.int32),
                          ("entropy", np.float64), ("condition_number", np.float64), ("constraint_ratio", np.float64),
                          ("constraint_ratio_accepted", np.float64)])
assert _RESULT_DTYPE.itemsize == C.sizeof(_lib.Result)


def _unpack_stats(res, levels, iters):
    out = []
    for li in range(res.n_levels):
        L = levels[li]
        ls = LevelStats(L.id, L.max_valid_pixels, L.valid_pixels, L.termination)
        for k in range(L.n_iterations):
            s = iters[L.first_iteration_index + k]
            ls.Iterations.append(IterationStats(
                s.id, s.valid_constraints, s.tdist_loglik, np.array(s.tdist_mean), np.array(s.tdist_precision).reshape(2, 2),
                s.prior_loglik, np.array(s.increment), np.array(s.information).reshape(6, 6)))
        out.append(ls)
    return out
