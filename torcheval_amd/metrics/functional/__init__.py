"""Functional (stateless) metrics — parity with torcheval/metrics/functional/__init__.py."""

from torcheval_amd.metrics.functional.aggregation import auc, mean, sum, throughput
from torcheval_amd.metrics.functional.classification import *  # noqa: F401,F403
from torcheval_amd.metrics.functional.classification import __all__ as _cls_all
from torcheval_amd.metrics.functional.classification import multiclass_calibration_error  # not in __all__
from torcheval_amd.metrics.functional.classification import dice_score, mean_iou  # likewise
from torcheval_amd.metrics.functional.clustering import silhouette_samples, silhouette_score  # likewise
from torcheval_amd.metrics.functional.clustering import (  # likewise (K25)
    adjusted_mutual_info_score,
    adjusted_rand_score,
    completeness_score,
    contingency_matrix,
    fowlkes_mallows_score,
    homogeneity_score,
    mutual_info_score,
    normalized_mutual_info_score,
    rand_score,
    v_measure_score,
)
from torcheval_amd.metrics.functional.detection import mean_average_precision  # likewise
from torcheval_amd.metrics.functional.image import peak_signal_noise_ratio
from torcheval_amd.metrics.functional.image import structural_similarity  # not a reference name: kept out of __all__
from torcheval_amd.metrics.functional.image import kernel_inception_distance  # likewise
from torcheval_amd.metrics.functional.image import inception_score  # likewise
from torcheval_amd.metrics.functional.image import density_coverage, improved_precision_recall  # likewise
from torcheval_amd.metrics.functional.ranking import (
    click_through_rate,
    frequency_at_k,
    hit_rate,
    num_collisions,
    reciprocal_rank,
    retrieval_precision,
    weighted_calibration,
)
from torcheval_amd.metrics.functional.ranking import normalized_dcg  # not a reference name: kept out of __all__
from torcheval_amd.metrics.functional.regression import mean_squared_error, r2_score
from torcheval_amd.metrics.functional.regression import spearman_corrcoef  # not a reference name: kept out of __all__
from torcheval_amd.metrics.functional.regression import concordance_corrcoef, pearson_corrcoef  # likewise
from torcheval_amd.metrics.functional.regression import kl_divergence  # likewise
from torcheval_amd.metrics.functional.regression import kendall_rank_corrcoef  # likewise
from torcheval_amd.metrics.functional.text import (
    bleu_score,
    perplexity,
    word_error_rate,
    word_information_lost,
    word_information_preserved,
)

__all__ = sorted(
    list(_cls_all)
    + ["auc", "mean", "sum", "throughput", "peak_signal_noise_ratio"]
    + ["click_through_rate", "frequency_at_k", "hit_rate", "num_collisions", "reciprocal_rank"]
    + ["retrieval_precision", "weighted_calibration", "mean_squared_error", "r2_score"]
    + ["bleu_score", "perplexity", "word_error_rate", "word_information_lost"]
    + ["word_information_preserved"]
)
