"""Clustering metrics, functional API (none of them a reference name)."""

from torcheval_amd.metrics.functional.clustering.silhouette import silhouette_samples, silhouette_score

__all__ = [
    "silhouette_samples",
    "silhouette_score",
]
__doc_name__ = "Clustering Metrics"
