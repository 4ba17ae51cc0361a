"""The table of ``torcheval_amd/ops/rowsums.py`` in plain torch, float64, on CPU.

``rowsums_oracle`` is the definition that the K5b kernel (csrc/kernels/rowsums.hip) and its host
twin are held to.  It calls nothing of the package and shares no code with either: every statistic
is one whole-row ATen reduction of the ``[rows, numel / rows]`` view, every output is then updated
the way ``state = state op value`` would be in the state's own dtype.
"""

from typing import List, Optional, Sequence, Tuple

import torch

WX, WT, W, SSE, WSSE, WTT, TMIN, TMAX, COUNT, RANGE = range(10)
SET, ADD, MIN, MAX = range(4)
FIRST_ROW = 4
NEEDS_T = (WT, SSE, WSSE, WTT, TMIN, TMAX, RANGE)
_INF = float("inf")


def _rows64(v: Optional[torch.Tensor], rows: int) -> Optional[torch.Tensor]:
    if v is None:
        return None
    v = v.detach().cpu()
    if not (v.dim() == 2 and v.shape[0] == rows):
        v = v.reshape(rows, v.numel() // rows)
    return v.to(torch.float64)


def _extreme(t: torch.Tensor, lowest: bool) -> torch.Tensor:
    """NaN-propagating row minimum / maximum; +inf / -inf for an empty row."""
    rows, n = t.shape
    if n == 0:
        return torch.full((rows,), _INF if lowest else -_INF, dtype=torch.float64)
    return t.amin(dim=1) if lowest else t.amax(dim=1)  # amin / amax propagate NaN


def row_values(x, t, w, w_scalar: float, stat: int, rows: int, absolute: bool = False) -> torch.Tensor:
    """float64 [rows]: statistic ``stat`` (not RANGE) of every row.  ``absolute``: the sum of the
    absolute values of its terms instead, which bounds what a reordering of the sum can change."""
    x, t, w = _rows64(x, rows), _rows64(t, rows), _rows64(w, rows)
    n = x.shape[1]
    if stat == COUNT:
        return torch.full((rows,), float(n), dtype=torch.float64)
    if stat in NEEDS_T:
        assert t is not None, "this statistic reads the target"
    if stat == TMIN:
        return _extreme(t, True)
    if stat == TMAX:
        return _extreme(t, False)
    if stat == W:
        if w is None:
            v = torch.full((rows,), float(w_scalar) * n, dtype=torch.float64)
            return v.abs() if absolute else v
        terms, final = w, True
    elif stat == WX:
        terms, final = x, False
    elif stat == WT:
        terms, final = t, False
    elif stat == SSE:
        terms, final = (x - t) * (x - t), True  # never weighted
    elif stat == WSSE:
        terms, final = (x - t) * (x - t), False
    elif stat == WTT:
        terms, final = t * t, False
    else:
        raise ValueError(f"no such row statistic: {stat}")
    if not final and w is not None:
        terms = w * terms
    if absolute:
        terms = terms.abs()
    s = terms.sum(dim=1)
    if not final and w is None:
        s = float(w_scalar) * s  # a scalar weight is applied once per row
        if absolute:
            s = s.abs()
    return s


def _apply(state: torch.Tensor, value: float, op: int) -> torch.Tensor:
    """``state op value`` for one 0-d state, the value rounded to the state's dtype first."""
    v = torch.tensor(value, dtype=torch.float64).to(state.dtype)
    if op == SET:
        return v
    if op == ADD:
        return state + v
    if op == MIN:
        return torch.minimum(state, v)  # propagates NaN
    return torch.maximum(state, v)


def rowsums_oracle(x: torch.Tensor, t: Optional[torch.Tensor], w: Optional[torch.Tensor], w_scalar: float,
                   outs: Sequence[Tuple[torch.Tensor, int, int]], rows: int) -> List[torch.Tensor]:
    """The states after one update.  ``outs``: ``(initial state, stat, op code)`` with op code =
    SET / ADD / MIN / MAX, ``| FIRST_ROW`` for an output that row 0 alone feeds (at its element 0).
    A state holds ``rows`` elements (one for a FIRST_ROW output, which may be 0-d).  Returns new
    tensors of the states' shapes and dtypes; the initial states are left as they are."""
    result = [s.detach().cpu().clone() for s, _, _ in outs]
    flat = [r.reshape(-1) for r in result]  # views of the clones
    for r in result:
        assert r.dtype in (torch.float32, torch.float64)
    x, t, w = _rows64(x, rows), _rows64(t, rows), _rows64(w, rows)  # converted once
    values = {}
    for _, stat, _ in outs:
        if stat != RANGE and stat not in values:
            values[stat] = row_values(x, t, w, w_scalar, stat, rows)
    for r in range(rows):
        merged_min = merged_max = 0.0  # RANGE sees the TMIN / TMAX outputs listed before it
        for k, (_, stat, code) in enumerate(outs):
            first = bool(code & FIRST_ROW)
            if first and r != 0:
                continue
            at = 0 if first else r
            v = merged_max - merged_min if stat == RANGE else float(values[stat][r])
            flat[k][at] = _apply(flat[k][at], v, code & 3)
            if stat == TMIN:
                merged_min = float(flat[k][at])
            if stat == TMAX:
                merged_max = float(flat[k][at])
    return result
