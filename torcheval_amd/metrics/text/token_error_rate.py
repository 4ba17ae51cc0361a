"""Token error rates over padded id rows, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The states are four 0-d float64
totals with merge kind ``"sum"`` (the sum of the edit distances, of the ``input`` and ``target`` row
lengths and of the longer length of each pair), so they live in the contiguous state buffer and sync
through the existing plans, like ``WordErrorRate``'s.  A ROCm update is K29's launches
(csrc/kernels/edit_distance.hip): the finish launch adds the batch straight into the states, with no
host synchronisation outside ``config.validate``.
"""

from typing import Optional

import torch

from torcheval_amd.metrics.functional.text.token_edit_distance import (
    _ignore_index_check,
    _measure_check,
    _token_check,
    _token_error_rate_compute,
    _token_update,
)
from torcheval_amd.metrics.metric import inference_update
from torcheval_amd.metrics.text._sum_states import _SumStates
from torcheval_amd.ops import edit_distance as _k29

__all__ = ["TokenErrorRate"]


class TokenErrorRate(_SumStates):
    """An error rate over all token-id pairs seen; see ``token_error_rate`` for the measures and
    ``token_edit_distance`` for what a row is.

    Args:
        measure: ``"wer"``, ``"mer"``, ``"wil"`` or ``"wip"``.
        ignore_index: the id to remove from both sides, or None.
        device: where the states live.
    """

    _names = ("errors", "input_total", "target_total", "max_total")

    def __init__(self, *, measure: str = "wer", ignore_index: Optional[int] = None,
                 device: Optional[torch.device] = None) -> None:
        super().__init__(device=device)
        _measure_check(measure)
        _ignore_index_check(ignore_index)
        self.measure = measure
        self.ignore_index = ignore_index
        for name in self._names:
            self._add_state(name, torch.tensor(0, dtype=torch.float64, device=self.device), merge="sum")

    def _states(self):
        return tuple(getattr(self, name) for name in self._names)

    @inference_update
    def update(self, input: torch.Tensor, target: torch.Tensor, input_lengths: Optional[torch.Tensor] = None,
               target_lengths: Optional[torch.Tensor] = None) -> "TokenErrorRate":
        """Add the pairs of one batch: integer ``[B, Li]`` and ``[B, Lt]`` ids and, optionally, the
        ``[B]`` lengths of their rows."""
        x, t, il, tl = _token_check(input, target, input_lengths, target_lengths, self.ignore_index)
        if x.shape[0] == 0:
            return self
        if x.device == self.errors.device and _k29.supported(x, t):
            _k29.edit_distance(x, t, il, tl, self.ignore_index, self._states(), True)
            return self
        for state, batch in zip(self._states(), _token_update(x, t, il, tl, self.ignore_index)[1]):
            state += batch.to(self.device)
        return self

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """The measure over all pairs seen, 0-d float64; NaN before any update."""
        return _token_error_rate_compute(*self._states(), self.measure)
