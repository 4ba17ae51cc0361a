"""Image metrics, class API (parity: metrics/image/{psnr,fid}.py).

``FrechetInceptionDistance`` is imported lazily (``torcheval_amd.metrics.FrechetInceptionDistance``
resolves on first access), so importing the metrics package never needs a vision library.
"""

from torcheval_amd.metrics.image.inception_score import InceptionScore
from torcheval_amd.metrics.image.kid import KernelInceptionDistance
from torcheval_amd.metrics.image.prdc import DensityCoverage, ImprovedPrecisionRecall
from torcheval_amd.metrics.image.psnr import PeakSignalNoiseRatio
from torcheval_amd.metrics.image.ssim import StructuralSimilarity

__all__ = [
    "DensityCoverage",
    "FrechetInceptionDistance",
    "ImprovedPrecisionRecall",
    "KernelInceptionDistance",
    "PeakSignalNoiseRatio",
    "StructuralSimilarity",
]
__doc_name__ = "Image Metrics"
__doc_extras__ = ["InceptionScore"]  # documented, not a reference name


def __getattr__(name):
    if name == "FrechetInceptionDistance":
        from torcheval_amd.metrics.image.fid import FrechetInceptionDistance

        return FrechetInceptionDistance
    raise AttributeError(name)
