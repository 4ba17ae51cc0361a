"""K29 (csrc/kernels/edit_distance.hip) on MI355X: token edit distances and totals equal to the two-row
table of tests/_edit_distance_oracle.py.  The cases are the smallest at which the strip walk can go wrong
(strip edges, the last partial strip, both orientations, padding that would match, ids above bit 32,
ignore_index at the chunk edges, the edge column at capacity, a second round of strips in the block arm).  A test
item is a group of cases: they, both arms, their token dtypes and a repeat run inside it, and a failure names
the case, dtype and arm."""

import pytest
import torch

from tests._edit_distance_oracle import CASES, GROUPS, bits, expected, measures, tensors, total_tensors
from torcheval_amd.metrics import TokenErrorRate
from torcheval_amd.metrics.functional import token_edit_distance, token_error_rate
from torcheval_amd.ops import edit_distance as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture
def launched(monkeypatch):
    calls, op = [], K.edit_distance
    monkeypatch.setattr(K, "edit_distance", lambda *a, **k: calls.append(1) or op(*a, **k))
    return calls


@pytest.mark.parametrize("group", GROUPS)
def test_against_oracle(group, launched, monkeypatch):
    for name in GROUPS[group]:
        d, totals = expected(name)
        want, kw = torch.tensor(d, device=DEV), {"ignore_index": CASES[name][1]}
        for dtype in CASES[name][3]:
            args = tensors(name, dtype, DEV)
            for arm in (K.ARM_WAVE, K.ARM_BLOCK):
                where = (name, dtype, arm)
                monkeypatch.setattr(K, "pick_arm", lambda *a: arm)
                before = len(launched)
                got = token_edit_distance(*args, **kw)
                assert got.is_cuda and got.dtype == torch.int64 and torch.equal(got, want), where
                assert torch.equal(token_edit_distance(*args, **kw), want), where  # repeat
                m = TokenErrorRate(device=DEV, **kw).update(*args)
                assert len(launched) == before + 3, where
                assert all(torch.equal(s, w) for s, w in zip(m._states(), total_tensors(totals, DEV))), where
        for measure, value in measures(totals).items():
            assert torch.equal(bits(token_error_rate(*args, measure=measure, **kw)), bits(value)), (name, measure)


def test_narrow_mixed_strided_and_too_wide_rows(launched, monkeypatch):
    d, _ = expected("rnd3_b9")
    x, t, il, tl = tensors("rnd3_b9", "int64", DEV)
    assert token_edit_distance(x.to(torch.int8), t.to(torch.int16), il, tl).tolist() == d
    assert token_edit_distance(x.int(), t, il.long(), tl.to(torch.uint8)).tolist() == d
    assert token_edit_distance(x[8, :129], t[8, :130]).tolist() == [d[8]] and len(launched) == 3
    strided = torch.stack([x, x + 1], dim=-1)[..., 0]  # the ATen form
    assert token_edit_distance(strided, t, il, tl).tolist() == d and len(launched) == 3
    monkeypatch.setattr(K, "edit_distance", None)  # width 4097 is the ATen form: the op must not launch
    wide = torch.cat([x[:2], x.new_full((2, 4097 - x.shape[1]), 5)], dim=1)
    assert token_edit_distance(wide, t[:2], il[:2], tl[:2]).tolist() == d[:2]


def test_class_updates_states_in_the_state_buffer():
    from torcheval_amd.parallel.state_buffer import buffer_of

    _, totals = expected("ignore_b5")
    x, t, il, tl = tensors("ignore_b5", "int32", DEV)
    m = TokenErrorRate(device=DEV, measure="wip", ignore_index=CASES["ignore_b5"][1])
    sb = buffer_of(m)
    ptrs = [s.data_ptr() for s in m._states()]
    m.update(x[:2], t[:2], il[:2], tl[:2]).update(x[2:], t[2:], il[2:], tl[2:])
    lo, hi = sb.buf.data_ptr(), sb.buf.data_ptr() + sb.buf.numel() * sb.buf.element_size()
    assert [s.data_ptr() for s in m._states()] == ptrs and all(lo <= q < hi for q in ptrs)
    assert all(torch.equal(s, w) for s, w in zip(m._states(), total_tensors(totals, DEV)))
    assert torch.equal(bits(m.compute()), bits(measures(totals)["wip"]))
    halves = [TokenErrorRate(device=DEV, ignore_index=-100).update(x[i], t[i], il[i], tl[i])
              for i in (slice(0, 3), slice(3, 5))]
    halves[0].merge_state(halves[1:])
    assert all(torch.equal(s, w) for s, w in zip(halves[0]._states(), total_tensors(totals, DEV)))
