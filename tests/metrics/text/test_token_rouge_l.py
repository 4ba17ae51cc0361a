"""Token LCS length and ROUGE-L on CPU tensors: the ATen form and the class against the two-row table of
tests/_lcs_oracle.py.  Lengths must be equal; the means lie within float64 summation error of the oracle's."""

import pytest
import torch

import torcheval_amd.metrics as M
import torcheval_amd.metrics.functional as MF
import torcheval_amd.metrics.functional.text as MFT
import torcheval_amd.metrics.text as MT
import torcheval_amd.ops as ops
from tests._lcs_oracle import CASES, SMALL, expected, tensors
from torcheval_amd.config import flags
from torcheval_amd.metrics import TokenROUGEL
from torcheval_amd.metrics.functional import token_lcs_length, token_rouge_l
from torcheval_amd.metrics.functional.text.token_rouge_l import MEASURES


def close(got, want_sum, pairs):  # `pairs` float64 terms added in another order, then one division
    return abs(got.item() - want_sum / pairs) <= pairs * 2.0**-52 * abs(want_sum / pairs)


@pytest.mark.parametrize("name", SMALL)
def test_aten_form_against_oracle(name):
    lengths, sums = expected(name)
    args, kw = tensors(name, CASES[name][5][0]), {"ignore_index": CASES[name][4]}
    got = token_lcs_length(*args, **kw)
    assert got.dtype == torch.int64 and got.tolist() == lengths
    assert token_lcs_length(args[1], args[0], args[3], args[2], **kw).tolist() == lengths  # symmetric
    for measure, want in zip(MEASURES, sums):
        value = token_rouge_l(*args, measure=measure, **kw)
        assert value.dtype == torch.float64 and value.ndim == 0 and close(value, want, len(lengths)), measure


def test_class_two_updates_merge_state_and_empty():
    _, sums = expected("length_edges")
    x, t, il, tl = tensors("length_edges")
    a = TokenROUGEL("recall").update(x[:4], t[:4], il[:4], tl[:4]).update(x[4:6], t[4:6], il[4:6], tl[4:6])
    a.merge_state([TokenROUGEL("recall").update(x[6:], t[6:], il[6:], tl[6:])])
    assert all(s.dtype == torch.float64 and s.ndim == 0 for s in a._states()) and a.pairs.item() == 10
    assert close(a.compute(), sums[1], 10)
    assert close(a.precision_sum / 10, sums[0], 10) and close(a.fmeasure_sum / 10, sums[2], 10)
    c = TokenROUGEL("recall")
    c.load_state_dict(a.state_dict())
    assert torch.equal(c.compute(), a.compute())
    a.reset()
    assert a.pairs.item() == 0 and a.compute().isnan()
    assert token_rouge_l(x[:0], t[:0]).isnan() and token_lcs_length(x[:0], t[:0]).shape == (0,)
    assert a.update(x[:0], t[:0]).compute().isnan()


def test_invalid_arguments():
    x, n = torch.zeros(2, 4, dtype=torch.int64), torch.tensor([1, 5])
    for args, kw, match in (((x.float(), x), {}, "integer tensor"), ((x, x[0]), {}, "both be"),
                            ((x[:1], x), {}, "same number of rows"), ((x, x, n.float()), {}, "input_lengths"),
                            ((x, x, None, n[:1]), {}, "target_lengths"), ((x, x), {"ignore_index": 1.5}, "ignore_index")):
        with pytest.raises(ValueError, match=match):
            token_lcs_length(*args, **kw)
    with pytest.raises(ValueError, match="measure"):
        token_rouge_l(x, x, measure="f1")
    with pytest.raises(ValueError, match="measure"):
        TokenROUGEL(measure="f1")
    with pytest.raises(ValueError, match="ignore_index"):
        TokenROUGEL(ignore_index=True)
    assert token_lcs_length(x, x, n, n).tolist() == [1, 4]  # 5 is clamped to the width
    with flags(validate=True), pytest.raises(ValueError, match=r"\[0, width\]"):
        token_rouge_l(x, x, n)


def test_exports():
    assert M.TokenROUGEL is MT.TokenROUGEL and MF.token_lcs_length is MFT.token_lcs_length
    assert MF.token_rouge_l is MFT.token_rouge_l
    # the lists mirror the reference's public names, which have no token-level metrics
    assert "TokenROUGEL" not in M.__all__ + MT.__all__ and "TokenROUGEL" in MT.__doc_more__
    assert not {"token_lcs_length", "token_rouge_l"} & set(MF.__all__ + MFT.__all__)
    assert {"token_lcs_length", "token_rouge_l"} <= set(MFT.__doc_more__)


@pytest.mark.skipif(not ops.native_loaded(), reason="extension not built")
def test_op_schema_and_limits():
    from torcheval_amd.ops import lcs as K

    assert str(torch.ops.torcheval_amd_lcs.lcs.default._schema) == (
        "torcheval_amd_lcs::lcs(Tensor input, Tensor target, Tensor? input_lengths, Tensor? target_lengths, "
        "int? ignore_index, Tensor(a!)? ws_tokens, Tensor(b!)? ws_lengths, int chunks, Tensor(c!) out, "
        "Tensor(d!)? precision_sum, Tensor(e!)? recall_sum, Tensor(f!)? fmeasure_sum, Tensor(g!)? pairs, "
        "bool accumulate) -> ()")
    for key in ("CUDA", "Meta"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("torcheval_amd_lcs::lcs", key)
    assert (K.MAX_LEN, K.MAX_CHUNKS, K.PAIRS_PER_WG) == (4096, 64, 4)
    assert [K.pick_chunks(w, 4096) for w in (0, 1, 64, 65, 128, 129, 257, 2049, 4096)] == [1, 1, 1, 2, 2, 4, 8, 64, 64]
    assert K.pick_chunks(200, 130) == 4
