"""Token edit distance and error rates on CPU tensors: the ATen form and the class against the two-row
table of tests/_edit_distance_oracle.py.  Distances and totals are integers and must be equal; the measures
must be bit-equal to the word-level ``_compute`` functions on the oracle's totals."""

import pytest
import torch

import torcheval_amd.metrics as M
import torcheval_amd.metrics.functional as MF
import torcheval_amd.metrics.functional.text as MFT
import torcheval_amd.metrics.text as MT
import torcheval_amd.ops as ops
from tests._edit_distance_oracle import CASES, bits, expected, levenshtein, measures, tensors
from torcheval_amd.config import flags
from torcheval_amd.metrics import TokenErrorRate
from torcheval_amd.metrics.functional import (
    token_edit_distance,
    token_error_rate,
    word_error_rate,
    word_information_lost,
    word_information_preserved,
)


@pytest.mark.parametrize("name", CASES)
def test_aten_form_against_oracle(name):
    d, totals = expected(name)
    x, t, il, tl = tensors(name, CASES[name][3][0])
    kw = {"ignore_index": CASES[name][1]}
    got = token_edit_distance(x, t, il, tl, **kw)
    assert got.dtype == torch.int64 and torch.equal(got, torch.tensor(d))
    for measure, want in measures(totals).items():
        value = token_error_rate(x, t, il, tl, measure=measure, **kw)
        assert value.dtype == torch.float64 and value.ndim == 0 and torch.equal(bits(value), bits(want)), measure
    m = TokenErrorRate(**kw).update(x, t, il, tl)
    assert [s.item() for s in m._states()] == list(totals)


def test_one_pair_garbage_lengths_and_strided_rows():
    d, _ = expected("rnd3_b9")
    x, t, il, tl = tensors("rnd3_b9")
    assert token_edit_distance(x[8, :129], t[8, :130]).tolist() == [d[8]]
    want = [levenshtein(a.tolist(), b[:m].tolist()) if n == 129 else d[k]  # 1129 is clamped to the width, -1000 to 0
            for k, (a, b, n, m) in enumerate(zip(x, t, il, tl))]
    assert want != d and token_edit_distance(x, t, il + 1000 * (il == 129), tl - 1000 * (tl == 0)).tolist() == want
    strided = torch.stack([x.to(torch.int16), x.to(torch.int16) + 1], dim=-1)[..., 0]
    assert not strided.is_contiguous() and token_edit_distance(strided, t.to(torch.int8), il, tl).tolist() == d


def test_class_two_updates_and_merge_state():
    _, totals = expected("rnd3_b9")
    x, t, il, tl = tensors("rnd3_b9")
    a = TokenErrorRate(measure="wil").update(x[:4], t[:4], il[:4], tl[:4]).update(x[4:6], t[4:6], il[4:6], tl[4:6])
    b = TokenErrorRate(measure="wil").update(x[6:], t[6:], il[6:], tl[6:])
    a.merge_state([b])
    assert [s.item() for s in a._states()] == list(totals)
    assert all(s.dtype == torch.float64 and s.ndim == 0 for s in a._states())
    assert torch.equal(bits(a.compute()), bits(measures(totals)["wil"]))
    c = TokenErrorRate(measure="wil")
    c.load_state_dict(a.state_dict())
    assert torch.equal(bits(c.compute()), bits(a.compute()))
    a.reset()
    assert a.errors.item() == 0 and a.compute().isnan()


def test_invalid_arguments():
    x, n = torch.zeros(2, 4, dtype=torch.int64), torch.tensor([1, 5])
    for args, kw, match in (((x.float(), x), {}, "integer tensor"), ((x, x[0]), {}, "both be"),
                            ((x[:1], x), {}, "same number of rows"), ((x, x, n.float()), {}, "input_lengths"),
                            ((x, x, None, n[:1]), {}, "target_lengths"), ((x, x), {"ignore_index": 1.5}, "ignore_index"),
                            ((x, x.to("meta")), {}, "one device"), ((x, x, n.to("meta")), {}, "device of the ids")):
        with pytest.raises(ValueError, match=match):
            token_edit_distance(*args, **kw)
    with pytest.raises(ValueError, match="measure"):
        token_error_rate(x, x, measure="cer")
    with pytest.raises(ValueError, match="measure"):
        TokenErrorRate(measure="cer")
    with pytest.raises(ValueError, match="ignore_index"):
        TokenErrorRate(ignore_index=True)
    assert token_edit_distance(x, x, n, n).tolist() == [0, 0]  # 5 is clamped to the width
    with flags(validate=True), pytest.raises(ValueError, match=r"\[0, width\]"):
        token_edit_distance(x, x, n)
    assert token_edit_distance(x[:0], x[:0]).shape == (0,)


def test_ids_decoded_to_words_give_the_word_metrics():
    x, t, il, tl = tensors("rnd3_b9")
    rows = [(a[:n].tolist(), b[:m].tolist()) for a, b, n, m in zip(x, t, il, tl) if n > 0 and m > 0]
    hyp, ref = ([" ".join(f"w{v}" for v in r[side]) for r in rows] for side in (0, 1))
    keep = (il > 0) & (tl > 0)
    args = (x[keep], t[keep], il[keep], tl[keep])
    for measure, words in (("wer", word_error_rate), ("wil", word_information_lost), ("wip", word_information_preserved)):
        assert token_error_rate(*args, measure=measure).item() == pytest.approx(words(hyp, ref).item(), rel=1e-6)


def test_exports():
    assert M.TokenErrorRate is MT.TokenErrorRate and MF.token_edit_distance is MFT.token_edit_distance
    assert MF.token_error_rate is MFT.token_error_rate
    # the lists mirror the reference's public names, which have no token-level metrics
    assert "TokenErrorRate" not in M.__all__ + MT.__all__ and MT.__doc_extras__ == ["TokenErrorRate"]
    assert not {"token_edit_distance", "token_error_rate"} & set(MF.__all__ + MFT.__all__)
    assert MFT.__doc_extras__ == ["token_edit_distance", "token_error_rate"]


@pytest.mark.skipif(not ops.native_loaded(), reason="extension not built")
def test_op_schema_and_limits():
    from torcheval_amd.ops import edit_distance as K

    assert str(torch.ops.torcheval_amd_editdist.edit_distance.default._schema) == (
        "torcheval_amd_editdist::edit_distance(Tensor input, Tensor target, Tensor? input_lengths, "
        "Tensor? target_lengths, int? ignore_index, Tensor(a!)? ws_tokens, Tensor(b!)? ws_lengths, int arm, "
        "Tensor(c!) out, Tensor(d!)? errors, Tensor(e!)? input_total, Tensor(f!)? target_total, "
        "Tensor(g!)? max_total, bool accumulate) -> ()")
    for key in ("CUDA", "Meta"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("torcheval_amd_editdist::edit_distance", key)
    assert (K.MAX_LEN, K.ARM_WAVE, K.ARM_BLOCK, K.PAIRS_PER_WG, K.BLOCK_WAVES) == (4096, 0, 1, 4, 8)
    assert K.pick_arm(32, 2048, 2048) == K.ARM_BLOCK and K.pick_arm(4096, 60, 60) == K.ARM_WAVE
