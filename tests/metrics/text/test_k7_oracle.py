"""The K7 perplexity fixtures on the CPU: the float64 oracle lands where each case says, the
package's CPU path agrees with it, the float32 lane model shows which cases the arithmetic before
the masked-logit fix gets wrong, and the table reaches every dispatch arm."""

import math

import pytest
import torch

from tests import _k7_cases as k7
from torcheval_amd.metrics.functional import perplexity

IDS = [c.id for c in k7.CASES]
MODELLED = [c.id for c in k7.CASES if c.group in ("mask_vec", "mask_split", "nan_logit", "no_u2")]


@pytest.mark.parametrize("case_id", IDS)
def test_oracle_category_and_cpu_path(case_id):
    c = k7.BY_ID[case_id]
    b = c.build()
    assert k7.k7_arm(c.rows, c.v, c.dtype, b.x.stride(1), b.x.storage_offset() * b.x.element_size()) == c.arm()
    ref = k7.ppl_oracle(b.x, b.t, c.ignore_index)
    assert k7.category(ref) == c.expect
    got = float(perplexity(b.x, b.t, ignore_index=c.ignore_index))
    if c.expect == "finite":
        assert got == pytest.approx(ref, rel=k7.REL)
    else:
        assert k7.category(got) == c.expect


def _model_category(c, b, fixed):
    x2, heads, u2, tt = b.x.reshape(-1, c.v), c.heads(), c.arm()[2], b.t.reshape(-1)
    rows = [r for r in c.model_rows() if c.ignore_index is None or int(tt[r]) != c.ignore_index]
    lse = [k7.prefix_model_lse(x2[r], int(heads[r]), u2, fixed) for r in rows]
    return "nan" if any(math.isnan(v) for v in lse) else "finite", rows, lse


@pytest.mark.parametrize("case_id", MODELLED)
def test_lane_model_tells_the_old_arithmetic_from_the_rule(case_id):
    c = k7.BY_ID[case_id]
    b = c.build()
    old, _, _ = _model_category(c, b, fixed=False)
    if c.old is not None:
        assert old == c.old
    # the arithmetic with the finite stand-ins: NaN where the oracle's log-sum-exp is, and close to it elsewhere
    new, rows, lse = _model_category(c, b, fixed=True)
    assert new == ("nan" if c.expect == "nan" else "finite")
    want = torch.logsumexp(b.x.reshape(-1, c.v)[rows].double(), dim=-1)
    for v, w in zip(lse, want.tolist()):
        assert (math.isnan(v) and math.isnan(w)) or v == pytest.approx(w, abs=1e-4)


def test_the_fixtures_detect_both_bugs():
    """Per dtype: masked cases with a finite oracle on which the old arithmetic gives NaN, in VEC,
    split and non-unrolled arms; NaN logits in a head and in a tail that it drops."""
    for dt in k7.DTYPES:
        mine = [c for c in k7.CASES if c.dtype == dt]
        for group in ("mask_vec", "mask_split", "no_u2"):
            hit = [c for c in mine if c.group == group and c.expect == "finite" and c.old == "nan"]
            assert hit, (group, dt)
            assert {c.arm()[1] for c in hit} == ({True} if group == "mask_vec" else {False} if group == "mask_split" else {False, True})
        dropped = [c.id for c in mine if c.group == "nan_logit" and c.expect == "nan" and c.old == "finite"]
        assert any("_head" in i for i in dropped) and any("_tail" in i for i in dropped), dt


def test_every_arm_and_grid_regime_is_reached():
    k7.assert_full_coverage()
    arms, _ = k7.coverage([c for c in k7.CASES if c.old == "nan" and c.expect == "finite"])
    assert len(arms) == 12  # the masked-logit bug is shown in every arm


@pytest.mark.parametrize("dtype", k7.DTYPES)
def test_a_row_shift_leaves_the_oracle_unchanged(dtype):
    name = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}[dtype]
    for tag in ("vec2048", "split1001o1"):
        base, moved = (k7.BY_ID[f"magnitude-{tag}_shift_{k}-{name}"].build() for k in ("base", "moved"))
        assert not torch.equal(base.x, moved.x) and torch.equal(base.t, moved.t)
        assert k7.ppl_oracle(moved.x, moved.t) == pytest.approx(k7.ppl_oracle(base.x, base.t), rel=1e-12)
