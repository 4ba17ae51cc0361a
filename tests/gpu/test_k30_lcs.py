"""K30 (csrc/kernels/lcs.hip) on MI355X: token LCS lengths equal to the two-row table of tests/_lcs_oracle.py,
and the ROUGE-L means within float64 summation error of its Python floats.  The cases are the smallest at which
the bit-vector kernel can go wrong: every instance at its smallest width with either side cut short, lengths round
the 64-column words, a carry through all-ones words, dense matches, ids above bit 31, ignore_index, both sides
stationary.  One test walks every case and id dtype and reports all that fail."""

import pytest
import torch

from tests._lcs_oracle import CASES, expected, tensors
from torcheval_amd.metrics import TokenROUGEL
from torcheval_amd.metrics.functional import token_lcs_length, token_rouge_l
from torcheval_amd.metrics.functional.text.token_rouge_l import MEASURES
from torcheval_amd.ops import lcs as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def close(got, want_sum, pairs):
    """``got`` is the mean of ``pairs`` float64 terms that the oracle added in another order: each of the
    ``pairs - 1`` additions and the division rounds by at most 2**-53 relative on either side."""
    return abs(got.item() - want_sum / pairs) <= pairs * 2.0**-52 * abs(want_sum / pairs)


def against_oracle(name, dtype, calls):
    lengths, sums = expected(name)
    args, kw, b = tensors(name, dtype, DEV), {"ignore_index": CASES[name][4]}, len(lengths)
    del calls[:]
    got = token_lcs_length(*args, **kw)
    assert got.is_cuda and got.dtype == torch.int64 and got.tolist() == lengths
    assert torch.equal(token_lcs_length(*args, **kw), got) and len(calls) == 2  # repeat; the kernel ran
    chunks = K.pick_chunks(args[0].shape[1], args[1].shape[1])
    if chunks < K.MAX_CHUNKS:  # the next larger instance gives the same
        assert K.lcs(*args, kw["ignore_index"], chunks=2 * chunks).tolist() == lengths
    half = [tuple(None if v is None else v[rows] for v in args) for rows in (slice(0, b // 2), slice(b // 2, b))]
    for measure, want in zip(MEASURES, sums):
        value = token_rouge_l(*args, measure=measure, **kw)
        assert value.dtype == torch.float64 and value.ndim == 0 and close(value, want, b), measure
        m = TokenROUGEL(measure, device=DEV, **kw).update(*half[0]).update(*half[1])
        assert m.pairs.item() == b and close(m.compute(), want, b), measure
        assert torch.equal(m.compute(), TokenROUGEL(measure, device=DEV, **kw).update(*half[0]).update(*half[1]).compute())


def narrow_mixed_strided_and_too_wide_rows(monkeypatch):
    lengths, _ = expected("length_edges")
    x, t, il, tl = tensors("length_edges", "int64", DEV)
    assert token_lcs_length(x.to(torch.int8), t.to(torch.int16), il, tl).tolist() == lengths
    assert token_lcs_length(x.int(), t, il.long(), tl.to(torch.uint8)).tolist() == lengths
    assert token_lcs_length(x[4, :65], t[4, :64]).tolist() == [lengths[4]]
    monkeypatch.setattr(K, "lcs", None)  # strided rows and width 4097 are the ATen form: the op must not launch
    assert token_lcs_length(torch.stack([x, x + 1], dim=-1)[..., 0], t, il, tl).tolist() == lengths
    wide = torch.cat([x[:2], x.new_full((2, 4097 - x.shape[1]), 5)], dim=1)
    assert token_lcs_length(wide, t[:2], il[:2], tl[:2]).tolist() == lengths[:2]


def test_against_oracle(monkeypatch):
    calls, op = [], K.lcs
    monkeypatch.setattr(K, "lcs", lambda *a, **k: calls.append(1) or op(*a, **k))
    failed = []
    for name in CASES:
        for dtype in CASES[name][5]:
            try:
                against_oracle(name, dtype, calls)
            except AssertionError as e:  # go on: every failing case is reported, not the first alone
                failed.append(f"{name}, {dtype}: {e}")
    assert not failed, "\n".join(failed)
    narrow_mixed_strided_and_too_wide_rows(monkeypatch)
