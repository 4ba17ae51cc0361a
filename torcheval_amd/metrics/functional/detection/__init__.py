"""Detection metrics, functional API (none of them a reference name)."""

from torcheval_amd.metrics.functional.detection.mean_ap import mean_average_precision

__all__: list = []
__doc_extras__ = [
    "mean_average_precision",
]
__doc_name__ = "Detection Metrics"
