"""Image metrics, functional API (parity: functional/image/psnr.py)."""

from torcheval_amd.metrics.functional.image.inception_score import inception_score
from torcheval_amd.metrics.functional.image.kid import kernel_inception_distance
from torcheval_amd.metrics.functional.image.prdc import density_coverage, improved_precision_recall
from torcheval_amd.metrics.functional.image.psnr import (
    peak_signal_noise_ratio,
    _psnr_param_check,
    _psnr_input_check,
    _psnr_update,
    _psnr_compute,
)
from torcheval_amd.metrics.functional.image.ssim import structural_similarity

__all__ = [
    "density_coverage",
    "improved_precision_recall",
    "kernel_inception_distance",
    "peak_signal_noise_ratio",
    "structural_similarity",
]
__doc_name__ = "Image Metrics"
__doc_extras__ = ["inception_score"]  # documented, not a reference name
