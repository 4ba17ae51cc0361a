"""Detection metrics, class API (none of them a reference name)."""

from torcheval_amd.metrics.detection.mean_ap import MeanAveragePrecision

__all__: list = []
__doc_extras__ = [
    "MeanAveragePrecision",
]
__doc_name__ = "Detection Metrics"
