"""External clustering indices that compare two labelings, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  Every class keeps one state,
the int64 ``[num_classes, num_clusters]`` contingency table with merge kind ``"sum"``, so it lives in
the contiguous state buffer, a distributed sync is the existing all-reduce and ``merge_state`` is an
add.  A ROCm update is K25's count launch (csrc/kernels/contingency.hip) straight into the state, with
no host synchronisation; ``compute()`` on ROCm is the statistics launches and one single-wave launch.
"""

from typing import Iterable, Optional

import torch

from torcheval_amd.metrics.functional.clustering.contingency import (
    _average_index,
    _BAD_LABEL,
    _beta_check,
    _contingency,
    _labels_check,
    _range_check,
    _v_measure,
    _values_aten,
)
from torcheval_amd.metrics.metric import Metric, inference_update
from torcheval_amd.ops import contingency as _k25
from torcheval_amd.ops.hostread import read_int

__all__ = [
    "AdjustedMutualInfoScore",
    "AdjustedRandScore",
    "CompletenessScore",
    "FowlkesMallowsScore",
    "HomogeneityScore",
    "MutualInfoScore",
    "NormalizedMutualInfoScore",
    "RandScore",
    "VMeasureScore",
]


class _ContingencyMetric(Metric[torch.Tensor]):
    """One index of the contingency table of all label pairs seen.

    A label outside ``[0, num_classes)`` or ``[0, num_clusters)`` does not stop ``update()``: the pair
    is counted nowhere, a flag is set (on the device for ROCm tensors), and ``compute()`` raises once
    and clears it; under ``config.validate`` every ``update()`` does.

    Args:
        num_classes: the ids of ``labels_true`` lie in ``[0, num_classes)``.
        num_clusters: the ids of ``labels_pred`` lie in ``[0, num_clusters)``.
        device: where the table lives.
    """

    _name = ""       # key of ops.contingency.INDEX
    _offset = 0      # position of the average method behind it
    _emi = False     # whether the value needs the expected mutual information
    _err: Optional[torch.Tensor] = None
    _err_words = 1

    def __init__(self, num_classes: int, num_clusters: int, device: Optional[torch.device] = None) -> None:
        super().__init__(device=device)
        _range_check(num_classes, "num_classes", required=True)
        _range_check(num_clusters, "num_clusters", required=True)
        self.num_classes = num_classes
        self.num_clusters = num_clusters
        self._add_state("contingency", torch.zeros(num_classes, num_clusters, dtype=torch.int64, device=self.device),
                        merge="sum")
        self._bad_on_host = False
        if self.device.type == "cuda":
            self._err = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _state_flag(self) -> Optional[torch.Tensor]:
        """The flag of a ROCm state, on the state's device (it follows a moved state)."""
        if self.contingency.device.type != "cuda":
            return None
        if self._err is None:
            self._err = torch.zeros(1, dtype=torch.int32, device=self.contingency.device)
        elif self._err.device != self.contingency.device:
            self._err = self._err.to(self.contingency.device)
        return self._err

    def _note(self, err: torch.Tensor) -> None:
        """Keep the flag of an update whose labels were not on the state's device: OR it into the
        state's flag (a device copy, no host read), or read it when the state is on the host."""
        flag = self._state_flag()
        if flag is not None:
            flag.bitwise_or_(err.to(flag.device))
        elif int(err.item()) != 0:
            self._bad_on_host = True

    def _raise_if_bad(self) -> None:
        if self._bad_on_host:
            self._bad_on_host = False
            raise ValueError(_BAD_LABEL + " (such pairs were counted nowhere).")

    def _check_device_errors(self) -> None:
        flag = self._state_flag()
        if flag is not None and read_int(flag) != 0:
            flag.zero_()
            self._bad_on_host = True
        self._raise_if_bad()

    @inference_update
    def update(self, labels_true: torch.Tensor, labels_pred: torch.Tensor):
        """Add the ``[N]`` int64 / int32 class ids and cluster ids of one batch."""
        _labels_check(labels_true, labels_pred)
        if labels_true.numel() == 0:
            return self
        labels_pred = labels_pred.to(labels_true.device)
        on_state = labels_true.device == self.contingency.device
        flag = self._state_flag() if on_state else None
        err = flag if flag is not None else torch.zeros(1, dtype=torch.int32, device=labels_true.device)
        table = _contingency(labels_true, labels_pred, self.num_classes, self.num_clusters, err=err,
                             table=self.contingency if on_state else None)
        if not on_state:
            self.contingency += table.to(self.device)
        if err is not flag:
            self._note(err)
        return self

    def _from_values(self, values: torch.Tensor) -> torch.Tensor:
        return values[_k25.INDEX[self._name] + self._offset]

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """The value over all pairs seen, a float64 scalar on the metric's device; NaN before any
        update."""
        table = self.contingency
        if not _k25.supported_table(table):
            values = _values_aten(table, self._emi)
            self._check_device_errors()
            return self._from_values(values)
        values, total = _k25.contingency_values(table, self._emi)
        # the call's one host read: the flag, and whether the total left the kernels' range
        word = (total >= 2**32).to(torch.int32).reshape(1) * 2
        flag = self._state_flag()
        code = read_int(word if flag is None else word + flag)
        if code & 1:
            flag.zero_()
            self._bad_on_host = True
        if code & 2:
            values = _values_aten(table, self._emi)
        self._raise_if_bad()
        return self._from_values(values)

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["_ContingencyMetric"]):
        for metric in metrics:
            self.contingency += metric.contingency.to(self.device)
        return self

    def reset(self):
        self._bad_on_host = False
        if self._err is not None:
            self._err.zero_()
        return super().reset()


class RandScore(_ContingencyMetric):
    """Rand index of all label pairs seen; see ``rand_score``."""

    _name = "rand"


class AdjustedRandScore(_ContingencyMetric):
    """Rand index adjusted for chance; see ``adjusted_rand_score``."""

    _name = "adjusted_rand"


class FowlkesMallowsScore(_ContingencyMetric):
    """Fowlkes-Mallows index; see ``fowlkes_mallows_score``."""

    _name = "fowlkes_mallows"


class MutualInfoScore(_ContingencyMetric):
    """Mutual information of the two labelings in nats; see ``mutual_info_score``."""

    _name = "mutual_info"


class HomogeneityScore(_ContingencyMetric):
    """Homogeneity; see ``homogeneity_score``."""

    _name = "homogeneity"


class CompletenessScore(_ContingencyMetric):
    """Completeness; see ``completeness_score``."""

    _name = "completeness"


class _AveragedMetric(_ContingencyMetric):
    def __init__(self, num_classes: int, num_clusters: int, average_method: str = "arithmetic",
                 device: Optional[torch.device] = None) -> None:
        super().__init__(num_classes, num_clusters, device=device)
        self._offset = _average_index(average_method)
        self.average_method = average_method


class NormalizedMutualInfoScore(_AveragedMetric):
    """Normalized mutual information; see ``normalized_mutual_info_score``.

    Args:
        num_classes, num_clusters, device: as every class of this module.
        average_method: ``"min"``, ``"geometric"``, ``"arithmetic"`` or ``"max"``.
    """

    _name = "normalized_mutual_info"


class AdjustedMutualInfoScore(_AveragedMetric):
    """Mutual information adjusted for chance; see ``adjusted_mutual_info_score``.

    Args:
        num_classes, num_clusters, device: as every class of this module.
        average_method: ``"min"``, ``"geometric"``, ``"arithmetic"`` or ``"max"``.
    """

    _name = "adjusted_mutual_info"
    _emi = True


class VMeasureScore(_ContingencyMetric):
    """V-measure; see ``v_measure_score``.

    Args:
        num_classes, num_clusters, device: as every class of this module.
        beta: weight of homogeneity against completeness.
    """

    def __init__(self, num_classes: int, num_clusters: int, beta: float = 1.0,
                 device: Optional[torch.device] = None) -> None:
        super().__init__(num_classes, num_clusters, device=device)
        _beta_check(beta)
        self.beta = beta

    def _from_values(self, values: torch.Tensor) -> torch.Tensor:
        return _v_measure(values, self.beta)
