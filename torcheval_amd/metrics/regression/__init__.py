"""Regression class metrics (parity: metrics/regression/*.py)."""

from torcheval_amd.metrics.regression.kendall import KendallRankCorrCoef
from torcheval_amd.metrics.regression.kl_divergence import KLDivergence
from torcheval_amd.metrics.regression.mean_squared_error import MeanSquaredError
from torcheval_amd.metrics.regression.pearson import ConcordanceCorrCoef, PearsonCorrCoef
from torcheval_amd.metrics.regression.r2_score import R2Score
from torcheval_amd.metrics.regression.spearman import SpearmanCorrCoef

__all__ = [
    "ConcordanceCorrCoef",
    "KendallRankCorrCoef",
    "MeanSquaredError",
    "PearsonCorrCoef",
    "R2Score",
    "SpearmanCorrCoef",
]
__doc_name__ = "Regression Metrics"
__doc_extras__ = ["KLDivergence"]  # documented, not a reference name
