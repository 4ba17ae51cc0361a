"""Clustering metrics, functional API (none of them a reference name)."""

from torcheval_amd.metrics.functional.clustering.contingency import (
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
from torcheval_amd.metrics.functional.clustering.silhouette import silhouette_samples, silhouette_score

__all__ = [
    "silhouette_samples",
    "silhouette_score",
]
# documented, outside the pinned __all__ (K25: the indices of a contingency table)
__doc_extras__ = [
    "contingency_matrix",
    "rand_score",
    "adjusted_rand_score",
    "mutual_info_score",
    "normalized_mutual_info_score",
    "adjusted_mutual_info_score",
    "homogeneity_score",
    "completeness_score",
    "v_measure_score",
    "fowlkes_mallows_score",
]
__doc_name__ = "Clustering Metrics"
