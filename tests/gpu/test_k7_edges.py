"""K7 (csrc/kernels/perplexity.hip) on the GPU at masked and non-finite logits, in every dispatch
arm (dtype x VEC x U2) and both grid regimes, at large magnitudes and with every target layout.

The cases, the float64 oracle and the mirror of the dispatch are in tests/_k7_cases.py; that the
cases tell the arithmetic before the masked-logit fix from the rule is asserted on the CPU, in
tests/metrics/text/test_k7_oracle.py.  Finite expectations are held to the tolerance of the other
K7 tests (rel 2e-5 against float64); ``+inf`` and NaN expectations are compared by category.

Against the kernel as it was before the fix, 158 of these tests fail (of the 696 without the ``walk``
group, plain logits at the smallest shape that reaches every part of the split walk, which came
with the shared row loaders and was not run on that kernel), in the functional, the
class and the deterministic test alike: every masked case whose ``old`` is "nan" (NaN for a finite
perplexity: ``mask_vec`` v3072_leftover, v4096_last2100, v4096_pair2, v4112_keep3; ``mask_split``
every ``_body`` case, v50257o3_keep3 and two float16 v1001 ``_keep3`` draws; ``no_u2`` v33_masked
and v1040_masked), the NaN logits it drops (``nan_logit`` split1001o3_head, split40o1_head,
split40o1_tail: a finite value for NaN), the bfloat16 ``_extremes`` cases (``m + log(s)`` loses
``log(s)`` at 3e38: 186.06 for 241.29) and the four negative-target cases.  The masked cases whose
``old`` is "finite" pass before and after: the all ``-inf`` step meets a lane that is still empty.
"""

import functools

import pytest
import torch

from tests import _k7_cases as k7
from torcheval_amd.config import flags
from torcheval_amd.metrics import Perplexity
from torcheval_amd.metrics.functional import perplexity

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [c.id for c in k7.CASES]
MASKED = [c.id for c in k7.CASES if c.group in ("mask_vec", "mask_split") or (c.group == "no_u2" and c.old)]


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    """(float64 per-row negative log-likelihood, flat targets) of one case, computed once."""
    b = k7.BY_ID[case_id].build()
    return k7.row_nll(b.x, b.t), b.t.reshape(-1).long().clone()


def _on_device(c):
    """The case's logits and targets on the GPU in their storage layout, checked against the mirror."""
    b = c.build()
    xd = b.big.to(DEV)[..., c.off:c.off + c.v]
    td = b.tbuf.to(DEV)
    if c.tgt.endswith("s2"):
        td = td[:, ::2]
        assert td.reshape(-1).data_ptr() == td.data_ptr() and td.reshape(-1).stride(0) == 2
    assert xd.stride() == b.x.stride() and xd.stride(1) == c.w
    assert (xd.data_ptr() - xd.storage_offset() * xd.element_size()) % 16 == 0
    assert k7.k7_arm(c.rows, c.v, c.dtype, xd.stride(1), xd.storage_offset() * xd.element_size()) == c.arm()
    return xd, td


def _check(got: float, ref: float, c) -> None:
    assert k7.category(ref) == c.expect
    if c.expect == "finite":
        assert got == pytest.approx(ref, rel=k7.REL)
    else:
        assert k7.category(got) == c.expect


@pytest.mark.parametrize("case_id", IDS)
def test_k7_functional_matches_fp64(case_id):
    c = k7.BY_ID[case_id]
    nll, t = _reference(case_id)
    xd, td = _on_device(c)
    got = perplexity(xd, td, ignore_index=c.ignore_index)
    assert got.dtype == torch.float64 and got.shape == ()
    _check(float(got), k7.ppl_of_nll(nll, t, c.ignore_index), c)


@pytest.mark.parametrize("case_id", IDS)
def test_k7_class_two_updates_match_fp64_of_the_concatenation(case_id):
    """update(all rows) then update(the first batch entry): the oracle over both, concatenated."""
    c = k7.BY_ID[case_id]
    nll, t = _reference(case_id)
    xd, td = _on_device(c)
    m = Perplexity(ignore_index=c.ignore_index, device=DEV)
    m.update(xd, td)
    m.update(xd[:1], td[:1])
    got = m.compute()
    ref = k7.ppl_of_nll(torch.cat([nll, nll[:c.s]]), torch.cat([t, t[:c.s]]), c.ignore_index)
    if c.id.split("-")[1].endswith("all_ignored"):
        assert got.numel() == 0  # nothing counted: the empty tensor of a fresh metric
        assert k7.category(ref) == "nan"
    else:
        _check(float(got), ref, c)


@pytest.mark.parametrize("case_id", MASKED)
def test_k7_masked_deterministic_is_bit_equal_and_matches_fp64(case_id):
    c = k7.BY_ID[case_id]
    nll, t = _reference(case_id)
    xd, td = _on_device(c)
    with flags(deterministic=True):
        a = perplexity(xd, td, ignore_index=c.ignore_index)
        b = perplexity(xd, td, ignore_index=c.ignore_index)
    _check(float(a), k7.ppl_of_nll(nll, t, c.ignore_index), c)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_k7_cases_reach_every_arm_and_grid_regime():
    k7.assert_full_coverage()


@pytest.mark.parametrize("ignore_index", [None, -100])
@pytest.mark.parametrize("vocab", [33, 4096])
def test_k7_negative_counted_target_raises(vocab, ignore_index):
    """A counted target below zero raises from the functional call, as it does from compute()."""
    x = torch.randn(2, 3, vocab, device=DEV)
    t = torch.tensor([[1, -100, 0], [2, -1, 3]], device=DEV)
    if ignore_index is None:
        t[0, 1] = 4
    with pytest.raises(ValueError, match="cannot be negative"):
        perplexity(x, t, ignore_index=ignore_index)
    m = Perplexity(ignore_index=ignore_index, device=DEV)
    m.update(x, t)
    with pytest.raises(ValueError, match="vocab_size minus one"):
        m.compute()
    # too large still reports the reference's message, whatever else is wrong
    t[1, 2] = vocab
    with pytest.raises(ValueError, match="vocab_size minus one"):
        perplexity(x, t, ignore_index=ignore_index)
