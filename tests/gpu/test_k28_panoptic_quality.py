"""K28 (csrc/kernels/panoptic.hip) on MI355X: panoptic quality against the exact dict-loop oracle of
tests/_panoptic_oracle.py, under its derived tolerances.  The cases are the smallest at which the span
tables, the image-level merge, the matching rules or the flag handling can go wrong;
tests/_panoptic_oracle.py builds them.  A test item is a group of cases: they and their dtypes run inside it."""

import numpy as np
import pytest
import torch

from tests._panoptic_oracle import GROUPS, STUFFS, THINGS, case, check_states, check_values, tensors, values
from torcheval_amd.metrics import PanopticQuality
from torcheval_amd.metrics.functional import panoptic_quality
from torcheval_amd.ops import panoptic as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KW = {"things": THINGS, "stuffs": STUFFS}


@pytest.fixture
def launched(monkeypatch):
    calls, op = [], K.panoptic_quality
    monkeypatch.setattr(K, "panoptic_quality", lambda *a, **k: calls.append(1) or op(*a, **k))
    return calls


@pytest.mark.parametrize("group", GROUPS)
def test_against_oracle(group, launched):
    for name, dtype in ((name, dtype) for name in GROUPS[group] for dtype in case(name)[0].dtypes):
        c, states = case(name)
        print(name, dtype)
        x, t = tensors(c, dtype, DEV)
        kw = dict(KW, allow_unknown_preds_category=c.allow, return_sq_and_rq=True)
        before = len(launched)
        if c.route == "raises":
            with pytest.raises(ValueError, match="neither `things` nor `stuffs`"):
                panoptic_quality(x, t, **kw)
            assert len(launched) == before + 1
            continue
        per_class, means = values(states)
        got = panoptic_quality(x, t, **kw)
        assert got.is_cuda and got.dtype == torch.float32 and len(launched) == before + 1
        check_values(got, means)
        again = panoptic_quality(x, t, return_per_class=True, **kw)
        check_values(again, per_class)
        assert torch.equal(again.view(torch.int32), panoptic_quality(x, t, return_per_class=True, **kw).view(torch.int32))
        assert torch.equal(got.view(torch.int32), panoptic_quality(x, t, **kw).view(torch.int32))  # bitwise, NaN included
        m = PanopticQuality(device=DEV, allow_unknown_preds_category=c.allow, **KW).update(x, t)
        if c.route == "rerun":  # the functional took the ATen form after the flag; the class cannot
            with pytest.raises(RuntimeError, match=f"{K.MAX_SEGMENTS} segments.*{K.MAX_PAIRS} co-occurring"):
                m.compute()
            continue
        check_states(m, states, x.shape[0])
        check_values(m.compute(), means[0])


def test_class_unknown_input_raises_at_compute(launched):
    c, _ = case("unknown_input")
    m = PanopticQuality(device=DEV, **KW).update(*tensors(c, "int64", DEV))
    with pytest.raises(ValueError, match="neither `things` nor `stuffs`"):
        m.compute()
    assert len(launched) == 1


def test_narrow_mixed_and_non_contiguous_maps(launched):
    c, states = case("px65")
    x, t = tensors(c, "int64", DEV)
    check_values(panoptic_quality(x.to(torch.uint8), t.to(torch.int16), return_sq_and_rq=True, **KW), values(states)[1])
    check_values(panoptic_quality(x.int(), t, return_sq_and_rq=True, **KW), values(states)[1])
    assert len(launched) == 2
    strided = torch.stack([x, x], dim=-1)[..., 0]  # the ATen form
    check_values(panoptic_quality(strided, t, return_sq_and_rq=True, **KW), values(states)[1])
    assert len(launched) == 2


def test_chunks_of_whole_images(monkeypatch):
    c, states = case("images")
    x, t = tensors(c, "int64", DEV)
    whole = panoptic_quality(x, t, return_sq_and_rq=True, return_per_class=True, **KW)
    monkeypatch.setattr(K, "WORKSPACE_CAP", 1)  # one image per call of the op
    assert K.images_per_call(x.shape[1] * x.shape[2]) == 1
    assert torch.equal(panoptic_quality(x, t, return_sq_and_rq=True, return_per_class=True, **KW).view(torch.int32),
                       whole.view(torch.int32))


def test_class_updates_states_in_the_state_buffer():
    from torcheval_amd.parallel.state_buffer import buffer_of

    c, states = case("images")
    x, t = tensors(c, "int32", DEV)
    names = ("iou_sum", "true_positives", "false_positives", "false_negatives")
    m = PanopticQuality(device=DEV, return_sq_and_rq=True, **KW)
    sb = buffer_of(m)
    ptrs = [getattr(m, s).data_ptr() for s in names]
    m.update(x[:1], t[:1]).update(x[1:], t[1:])
    lo, hi = sb.buf.data_ptr(), sb.buf.data_ptr() + sb.buf.numel() * sb.buf.element_size()
    assert [getattr(m, s).data_ptr() for s in names] == ptrs and all(lo <= q < hi for q in ptrs)
    check_states(m, states, 2)
    # two updates are one functional call on the concatenation, bit for bit: images add in order
    assert torch.equal(m.compute().view(torch.int32), panoptic_quality(x, t, return_sq_and_rq=True, **KW).view(torch.int32))
    halves = [PanopticQuality(device=DEV, return_sq_and_rq=True, **KW).update(x[i:i + 1], t[i:i + 1]) for i in (0, 1)]
    halves[0].merge_state(halves[1:])
    check_states(halves[0], states, 2)
    check_values(halves[0].compute(), values(states)[1])
    assert np.isnan(PanopticQuality(device=DEV, **KW).compute().item())
