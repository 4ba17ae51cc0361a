"""Clustering metrics, class API (none of them a reference name)."""

from torcheval_amd.metrics.clustering.silhouette import SilhouetteScore

__all__ = [
    "SilhouetteScore",
]
__doc_name__ = "Clustering Metrics"
