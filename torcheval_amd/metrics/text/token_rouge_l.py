"""ROUGE-L over padded id rows, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The states are four 0-d float64
totals with merge kind ``"sum"`` (the sums of the pairs' precision, recall and F-measure, and the number
of pairs), so they live in the contiguous state buffer and sync through the existing plans, like
``TokenErrorRate``'s.  A ROCm update is K30's launches (csrc/kernels/lcs.hip): the finish launch adds
the batch straight into the states, with no host synchronisation outside ``config.validate``.
"""

from typing import Optional

import torch

from torcheval_amd.metrics.functional.text.token_edit_distance import _ignore_index_check, _token_check
from torcheval_amd.metrics.functional.text.token_rouge_l import _lcs_update, _measure_check, _rouge_l_compute
from torcheval_amd.metrics.metric import inference_update
from torcheval_amd.metrics.text._sum_states import _SumStates
from torcheval_amd.ops import lcs as _k30

__all__ = ["TokenROUGEL"]


class TokenROUGEL(_SumStates):
    """ROUGE-L averaged over all token-id pairs seen; see ``token_rouge_l`` for the measures and
    ``token_lcs_length`` for what a row is.

    Args:
        measure: ``"precision"``, ``"recall"`` or ``"fmeasure"``.
        ignore_index: the id to remove from both sides, or None.
        device: where the states live.
    """

    _names = ("precision_sum", "recall_sum", "fmeasure_sum", "pairs")

    def __init__(self, measure: str = "fmeasure", ignore_index: Optional[int] = None,
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
               target_lengths: Optional[torch.Tensor] = None) -> "TokenROUGEL":
        """Add the pairs of one batch: integer ``[B, Li]`` and ``[B, Lt]`` ids and, optionally, the
        ``[B]`` lengths of their rows."""
        x, t, il, tl = _token_check(input, target, input_lengths, target_lengths, self.ignore_index)
        if x.shape[0] == 0:
            return self
        if x.device == self.pairs.device and _k30.supported(x, t):
            _k30.lcs(x, t, il, tl, self.ignore_index, self._states(), True)
            return self
        for state, batch in zip(self._states(), _lcs_update(x, t, il, tl, self.ignore_index)[1]):
            state += batch.to(self.device)
        return self

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """The mean of the measure over all pairs seen, 0-d float64; NaN before any update."""
        return _rouge_l_compute(*self._states(), self.measure)
