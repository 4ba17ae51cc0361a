"""Multiclass calibration error (ECE, MCE and the RMS form), class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The states are three float64
``[n_bins]`` vectors with merge kind ``"sum"``, so they live in the contiguous state buffer and
sync through the existing plans; together they are the reliability diagram.  A ROCm update is
K15's two launches (csrc/kernels/calibration.hip): the row launch writes one partial triple per
block and the finish launch adds them, in block order, straight into the states, with no host
synchronisation and no ATen op.  ``compute()`` on ROCm is one single-wave launch.
"""

from typing import Iterable, Optional

import torch

from torcheval_amd.metrics.functional.classification.calibration_error import (
    _calibration_input_check,
    _calibration_param_check,
    _calibration_update,
    _calibration_value,
    _raise_on_bad_rows,
)
from torcheval_amd.metrics.metric import Metric, inference_update
from torcheval_amd.ops import calibration as _k15
from torcheval_amd.ops import use_native

__all__ = ["MulticlassCalibrationError"]


class MulticlassCalibrationError(Metric[torch.Tensor]):
    """Calibration error over all rows seen; see ``multiclass_calibration_error`` for the
    definition.

    On ROCm a label outside ``[0, C)`` or a confidence outside ``[0, 1]`` does not stop
    ``update()``: the row adds NaN to ``conf_sum[0]``, a device flag is set, and ``compute()``
    raises (and clears the flag; the states keep the NaN until ``reset()``).  On CPU ``update()``
    raises and leaves the states untouched.

    Args:
        n_bins: number of equal-width confidence bins, ``>= 1``.
        norm: ``"l1"`` (ECE), ``"max"`` (MCE) or ``"l2"``.
        from_logits: take the softmax of the scores first.
        device: where the states live.
    """

    _err: Optional[torch.Tensor] = None
    _err_words = 1

    def __init__(
        self,
        *,
        n_bins: int = 15,
        norm: str = "l1",
        from_logits: bool = False,
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(device=device)
        _calibration_param_check(n_bins, norm)
        self.n_bins = n_bins
        self.norm = norm
        self.from_logits = from_logits
        for name in ("bin_count", "correct_sum", "conf_sum"):
            self._add_state(name, torch.zeros(n_bins, dtype=torch.float64, device=self.device), merge="sum")
        if self.device.type == "cuda":
            self._err = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _err_for(self, input: torch.Tensor) -> Optional[torch.Tensor]:
        if not input.is_cuda:
            return None
        if self._err is None or self._err.device != input.device:
            self._err = torch.zeros(1, dtype=torch.int32, device=input.device)
        return self._err

    def _check_device_errors(self) -> None:
        _raise_on_bad_rows(self._err)

    @inference_update
    def update(self, input: torch.Tensor, target: torch.Tensor) -> "MulticlassCalibrationError":
        """Add the rows of one ``[N, C]`` batch of scores and its ``[N]`` labels."""
        _calibration_input_check(input, target)
        if input.shape[0] == 0:
            return self
        if input.device == self.bin_count.device and _k15.supported(input, target, self.n_bins):
            _k15.calibration_update(input, target, self.n_bins, self.from_logits, self.bin_count, self.correct_sum,
                                    self.conf_sum, self._err_for(input))
            return self
        states = _calibration_update(input, target, self.n_bins, self.from_logits, self._err_for(input))
        self.bin_count += states[0].to(self.device)
        self.correct_sum += states[1].to(self.device)
        self.conf_sum += states[2].to(self.device)
        return self

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """The calibration error of all rows as a float32 scalar; NaN before any update."""
        if use_native(self.bin_count):
            out = _k15.calibration_value(self.bin_count, self.correct_sum, self.conf_sum, self.norm)
        else:
            out = _calibration_value(self.bin_count, self.correct_sum, self.conf_sum, self.norm)
        self._check_device_errors()
        return out

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["MulticlassCalibrationError"]) -> "MulticlassCalibrationError":
        for metric in metrics:
            self.bin_count += metric.bin_count.to(self.device)
            self.correct_sum += metric.correct_sum.to(self.device)
            self.conf_sum += metric.conf_sum.to(self.device)
        return self
