"""Regression metrics, functional API (parity: functional/regression/*.py)."""

from torcheval_amd.metrics.functional.regression._common import _native, _update
from torcheval_amd.metrics.functional.regression.kendall import kendall_rank_corrcoef
from torcheval_amd.metrics.functional.regression.kl_divergence import kl_divergence
from torcheval_amd.metrics.functional.regression.mean_squared_error import (
    mean_squared_error,
    _mean_squared_error_update,
    _mean_squared_error_compute,
    _mean_squared_error_update_input_check,
    _mean_squared_error_param_check,
)
from torcheval_amd.metrics.functional.regression.pearson import concordance_corrcoef, pearson_corrcoef
from torcheval_amd.metrics.functional.regression.r2_score import (
    r2_score,
    _r2_score_update,
    _r2_score_compute,
    _r2_score_param_check,
    _r2_score_update_input_check,
)
from torcheval_amd.metrics.functional.regression.spearman import spearman_corrcoef

__all__ = [
    "concordance_corrcoef",
    "kendall_rank_corrcoef",
    "mean_squared_error",
    "pearson_corrcoef",
    "r2_score",
    "spearman_corrcoef",
]
__doc_name__ = "Regression Metrics"
__doc_extras__ = ["kl_divergence"]  # documented, not a reference name
