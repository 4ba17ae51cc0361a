"""Inputs, the plain float64 oracle and the dispatch mirror of K7 (fused log-softmax perplexity).

Shared by tests/metrics/text/test_k7_oracle.py (CPU) and tests/gpu/test_k7_edges.py.  Nothing here
calls the package.

The rule (docs/parity.md): a ``-inf`` logit is a masked entry with probability 0; a NaN or ``+inf``
logit in a counted row gives NaN; ignored rows are never read into the result.  That is what the
float64 ``log_softmax`` of the dtype-rounded logits gives, which ``ppl_oracle`` takes literally.

``prefix_model_lse`` is a float32 model of one wave's lane arithmetic in csrc/kernels/perplexity.hip
(the ``chunk16`` and ``U2`` pair steps of ``stream_row``, the scalar head and tail, ``combine`` and
the xor fold).  With ``fixed=False`` it is the arithmetic before the masked-logit fix: a step whose values
are all ``-inf`` yields ``exp(-inf - -inf) = NaN``, and ``combine`` returns early when both maxima
are ``-inf``, which drops a NaN that arrives while the lane is still empty.  It exists only to show
that the fixtures tell that arithmetic from the rule; each case records what it gives (``old``).
"""

import os
import zlib
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch

# the launch knobs are read once per process; the arms below are reached by shape alone
assert "TORCHEVAL_AMD_PPL_U2" not in os.environ, "unset TORCHEVAL_AMD_PPL_U2: the K7 cases reach their arms by shape"
assert "TORCHEVAL_AMD_PPL_MAXGRID" not in os.environ, "unset TORCHEVAL_AMD_PPL_MAXGRID: the K7 cases reach their grids by shape"

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
NINF = float("-inf")
REL = 2e-5  # the tolerance of the K7 tests against the float64 oracle


def els_of(dtype: torch.dtype) -> int:
    return 4 if dtype == torch.float32 else 2


# ------------------------------------------------------------------ the oracle
def row_nll(x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """float64 [rows]: -log_softmax(x)[row, t[row]] of the dtype-rounded logits (targets clamped
    into range; rows whose target is out of range must be ignored by the caller)."""
    v = x.shape[-1]
    lp = torch.log_softmax(x.reshape(-1, v).double(), dim=-1)
    tt = t.reshape(-1).long().clamp(0, v - 1)
    return -lp.gather(1, tt[:, None])[:, 0]


def ppl_of_nll(nll: torch.Tensor, t: torch.Tensor, ignore_index: Optional[int]) -> float:
    tt = t.reshape(-1).long()
    keep = tt != ignore_index if ignore_index is not None else torch.ones_like(tt, dtype=torch.bool)
    return float(torch.exp(nll[keep].sum() / keep.sum()))  # 0 / 0 = nan when every row is ignored


def ppl_oracle(x: torch.Tensor, t: torch.Tensor, ignore_index: Optional[int] = None) -> float:
    """exp(mean over counted rows of -log_softmax(x)[t]) in float64; may be ``nan`` or ``inf``."""
    return ppl_of_nll(row_nll(x, t), t, ignore_index)


def category(value: float) -> str:
    if value != value:
        return "nan"
    if value == float("inf"):
        return "inf"
    assert value != NINF
    return "finite"


# ------------------------------------------------------------------ the dispatch of launch_perplexity
def k7_arm(rows: int, v: int, dtype: torch.dtype, row_stride: int, byte_offset: int):
    """(kind, vec, u2, grid_blocks) that csrc/kernels/perplexity.hip picks: a literal copy of
    ``vec_ok``, of the ``u2`` rule in ``launch_perplexity`` and of ``perplexity_blocks`` (with no
    TORCHEVAL_AMD_PPL_* override).  ``byte_offset`` is that of the first logit in its allocation,
    which the allocator aligns to 16 B and more."""
    kind = DTYPES.index(dtype)
    els = els_of(dtype)
    vw = 4 if dtype == torch.float32 else 8
    vec = v % 16 == 0 and row_stride % vw == 0 and byte_offset % 16 == 0
    u2 = rows <= 16384 or v * els >= 65536
    cap = 512 if dtype == torch.float32 and rows <= 8192 else 1024
    grid = max(1, min((rows + 3) // 4, cap))
    return kind, vec, u2, grid


def k7_heads(rows: int, v: int, dtype: torch.dtype, row_stride: int, byte_offset: int) -> torch.Tensor:
    """int64 [rows]: the scalar-head length of every row in the split arms of ``perplexity_kernel``
    (values up to the next 16-B boundary, at most v); all zero in the VEC arms."""
    els = els_of(dtype)
    addr = byte_offset + torch.arange(rows) * row_stride * els
    return torch.clamp(((16 - addr % 16) % 16) // els, max=v)


# ------------------------------------------------------------------ the float32 lane model
_F = np.float32


def _combine(m, s, m2, s2, fixed):
    mn = np.fmax(m, m2)  # fmaxf: a NaN operand loses
    if fixed:
        ms = _F(0) if mn == _F(NINF) else mn
        return mn, _F(s * np.exp(m - ms) + s2 * np.exp(m2 - ms))
    if mn == _F(NINF):
        return m, s  # "both empty"
    return mn, _F(s * np.exp(m - mn) + s2 * np.exp(m2 - mn))


def _sum_exp(vals, against):
    cs = _F(0)
    for e in np.exp(vals - against):
        cs = _F(cs + e)
    return cs


def _step(vals, m, s, fixed):
    cm = np.fmax.reduce(vals)
    if not fixed:
        return _combine(m, s, cm, _sum_exp(vals, cm), fixed)
    mn = np.fmax(m, cm)  # ``absorb``: every exponent against the new maximum, or 0 while it is -inf
    ms = _F(0) if mn == _F(NINF) else mn
    return mn, _F(s * np.exp(m - ms) + _sum_exp(vals, ms))


def prefix_model_lse(row: torch.Tensor, head: int = 0, u2: bool = True, fixed: bool = False) -> float:
    """log-sum-exp of one logit row as one wave of ``perplexity_kernel`` computes it, in float32:
    ``head`` scalar values (one per lane), 16-value chunks per lane (two a wave-stride apart per
    step when ``u2``), a scalar tail, then the xor fold over 64 lanes."""
    x = row.float().numpy()
    v = x.shape[0]
    head = min(head, v)
    nb = (v - head) // 16 * 16
    body = x[head:head + nb]
    m = np.full(64, NINF, dtype=_F)
    s = np.zeros(64, dtype=_F)
    step = 64 * 16
    with np.errstate(all="ignore"):
        for lane in range(64):
            ml, sl = m[lane], s[lane]
            if lane < head:
                ml, sl = _combine(ml, sl, x[lane], _F(1), fixed)
            base = lane * 16
            if u2:
                while base + step < nb:
                    vals = np.concatenate([body[base:base + 16], body[base + step:base + step + 16]])
                    ml, sl = _step(vals, ml, sl, fixed)
                    base += 2 * step
            while base < nb:
                ml, sl = _step(body[base:base + 16], ml, sl, fixed)
                base += step
            c = head + nb + lane
            if c < v:
                ml, sl = _combine(ml, sl, x[c], _F(1), fixed)
            m[lane], s[lane] = ml, sl
        if fixed:  # the row maximum, one rescale per lane, then the xor-butterfly sum
            mw = np.fmax.reduce(m)
            s = (s * np.exp(m - (_F(0) if mw == _F(NINF) else mw))).astype(_F)
            for o in (32, 16, 8, 4, 2, 1):
                s = (s + s[np.arange(64) ^ o]).astype(_F)
            return float(np.float64(mw) + np.log(np.float64(s[0])))
        for o in (32, 16, 8, 4, 2, 1):
            m2, s2 = m[np.arange(64) ^ o], s[np.arange(64) ^ o]
            for lane in range(64):
                m[lane], s[lane] = _combine(m[lane], s[lane], m2[lane], s2[lane], fixed)
        return float(np.float64(m[0]) + np.log(np.float64(s[0])))


# ------------------------------------------------------------------ the cases
@dataclass
class Built:
    big: torch.Tensor  # [b, s, w] logits storage
    x: torch.Tensor  # [b, s, v] view of big at column offset ``off``
    tbuf: torch.Tensor  # targets storage: [b, s], or [b, 2 s] for a stride-2 view
    t: torch.Tensor  # [b, s] targets (a view of tbuf)


@dataclass
class Ctx:
    case: "Case"
    xv: torch.Tensor  # [rows, v] view of the logits storage: writes land in ``big``
    t: torch.Tensor  # [rows] int64, laid out afterwards
    heads: torch.Tensor  # [rows] scalar-head length per row
    g: torch.Generator


@dataclass
class Case:
    id: str
    dtype: torch.dtype
    b: int
    s: int
    v: int
    edit: Callable[[Ctx], None]
    expect: str  # category of the float64 oracle: "finite", "inf" or "nan"
    old: Optional[str] = None  # category of prefix_model_lse(fixed=False) over the modelled rows
    off: int = 0  # column offset of the logits in their storage
    pad: int = 0  # columns of storage behind the logits
    ignore_index: Optional[int] = None
    tgt: str = "i64"  # "i64", "i32", "i64s2", "i32s2" (s2: a stride-2 view)
    group: str = ""
    scale: float = 4.0
    seed: Optional[str] = None  # cases with the same seed string draw the same logits and targets

    @property
    def rows(self) -> int:
        return self.b * self.s

    @property
    def w(self) -> int:
        return self.off + self.v + self.pad

    @property
    def byte_offset(self) -> int:
        return self.off * els_of(self.dtype)

    def arm(self):
        return k7_arm(self.rows, self.v, self.dtype, self.w, self.byte_offset)

    def heads(self) -> torch.Tensor:
        if self.arm()[1]:
            return torch.zeros(self.rows, dtype=torch.int64)
        return k7_heads(self.rows, self.v, self.dtype, self.w, self.byte_offset)

    def build(self) -> Built:
        g = torch.Generator().manual_seed(zlib.crc32((self.seed or self.id).encode()))
        big = (torch.randn(self.b, self.s, self.w, generator=g) * self.scale).to(self.dtype)
        t = torch.randint(0, self.v, (self.rows,), generator=g)
        xv = big.view(self.rows, self.w)[:, self.off:self.off + self.v]
        self.edit(Ctx(self, xv, t, self.heads(), g))
        tdt = torch.int32 if self.tgt.startswith("i32") else torch.int64
        if self.tgt.endswith("s2"):
            tbuf = torch.full((self.b, 2 * self.s), -7, dtype=tdt)  # the gaps hold an invalid label
            tv = tbuf[:, ::2]
            tv.copy_(t.view(self.b, self.s))
            assert tv.reshape(-1).data_ptr() == tbuf.data_ptr() and tv.reshape(-1).stride(0) == 2
        else:
            tbuf = t.view(self.b, self.s).to(tdt)
            tv = tbuf
        return Built(big, big[..., self.off:self.off + self.v], tbuf, tv)

    def model_rows(self) -> List[int]:
        """The rows that the CPU test puts through the lane model: every row of a small case, the
        first rows (one of each head length) of a wide or tall one."""
        n = 2 if self.v > 5000 else 8 if self.rows > 40 else self.rows
        return list(range(min(n, self.rows)))


def _cols(c: Ctx) -> torch.Tensor:
    return torch.arange(c.case.v)[None, :]


def _mask(c: Ctx, mask: torch.Tensor) -> None:
    """Set the masked entries to -inf (a row that would lose every column is left alone), then
    move each target that fell on a masked column to the row's first open one."""
    mask = mask.expand(c.xv.shape[0], c.case.v).clone()
    mask &= ~mask.all(dim=1, keepdim=True)
    c.xv[mask] = NINF
    first_open = (~mask).int().argmax(dim=1)
    hit = mask.gather(1, c.t[:, None])[:, 0]
    c.t[hit] = first_open[hit]


def plain(c: Ctx) -> None:
    pass


def mask_cols(*ranges):
    def edit(c: Ctx) -> None:
        col = _cols(c)
        m = torch.zeros_like(col, dtype=torch.bool)
        for lo, hi in ranges:
            m |= (col >= lo) & (col < hi)
        _mask(c, m)
    return edit


def mask_last(n: int):
    return lambda c: _mask(c, _cols(c) >= c.case.v - n)


def keep3(c: Ctx) -> None:
    """Everything -inf but three columns per row, the target among them."""
    v = c.case.v
    keep = torch.stack([c.t, (c.t + v // 3) % v, (c.t + 2 * v // 3) % v], dim=1)
    m = torch.ones(c.xv.shape[0], v, dtype=torch.bool).scatter_(1, keep, False)
    _mask(c, m)


def mask_part(part: str):
    """Per row of a split arm: the whole scalar head, the first body step of lane 0, which also
    holds the first head value (one 16-value chunk, or both chunks of a U2 pair), or the whole
    scalar tail."""
    def edit(c: Ctx) -> None:
        v, col, h = c.case.v, _cols(c), c.heads[:, None]
        nb = (v - h) // 16 * 16
        if part == "head":
            m = col < h
        elif part == "body":
            m = (col >= h) & (col < h + torch.clamp(nb, max=16))
            pair = (nb > 1024) & c.case.arm()[2]
            m |= pair & (col >= h + 1024) & (col < h + 1040)
        else:
            m = col >= h + nb
        _mask(c, m)
    return edit


def target_on_masked(c: Ctx) -> None:
    mask_cols((16, 32))(c)
    c.t[1] = 17


def neg_inf_row(ignored: bool):
    def edit(c: Ctx) -> None:
        c.xv[2, :] = NINF
        if ignored:
            c.t[2] = c.case.ignore_index
    return edit


def pos_inf_logit(c: Ctx) -> None:
    c.xv[1, c.case.v // 2] = float("inf")


def _split_row(c: Ctx, bare_tail_lane: bool = False) -> int:
    """The first row with a scalar head (row 1 in a VEC arm, which has none).  ``bare_tail_lane``:
    the first such row whose last column goes to a lane with no head value and no body chunk, if
    there is one."""
    v, h = c.case.v, c.heads
    nb = (v - h) // 16 * 16
    lane = v - 1 - h - nb
    for ok in ((h > 0) & (lane >= h) & (lane >= nb // 16) & bare_tail_lane, h > 0):
        if ok.any():
            return int(ok.nonzero()[0])
    return 1


def nan_logit(where: str, ignored: bool = False):
    """One NaN in one row: at the first head position, at the tail position of the highest lane
    (which, when the row is short, has neither a head value nor a body chunk), or in the body."""
    def edit(c: Ctx) -> None:
        v, r = c.case.v, _split_row(c, where == "tail")
        h = int(c.heads[r])
        nb = (v - h) // 16 * 16
        if where == "head":
            assert h > 0
            col = 0
        elif where == "tail":
            assert h + nb < v
            col = v - 1
        else:
            assert nb > 0
            col = h + (nb // 16 // 2) * 16 + 5
        c.xv[r, col] = float("nan")
        if c.t[r] == col:
            c.t[r] = (col + 1) % v
        if ignored:
            c.t[r] = c.case.ignore_index
    return edit


def near_ties(c: Ctx) -> None:
    """Large logits whose perplexity is finite: the target is the row maximum, and one other column
    lies within two units of it."""
    top = c.xv.float().argmax(dim=1)
    c.t.copy_(top)
    rows = torch.arange(c.xv.shape[0])
    other = (top + 1 + torch.randint(0, c.case.v - 1, top.shape, generator=c.g)) % c.case.v
    delta = torch.rand(top.shape, generator=c.g) * 2
    c.xv[rows, other] = (c.xv[rows, top].double() - delta.double()).to(c.case.dtype)


def extremes(big: float):
    """A twentieth of the entries at -big; rows 0, 2 (mod 3) carry +big on the target column (rows
    1 carry 1.0 there), and rows 0 (mod 3) carry +big on a second column too."""
    def edit(c: Ctx) -> None:
        n, v = c.xv.shape
        c.xv[torch.rand(n, v, generator=c.g) < 0.05] = -big
        rows = torch.arange(n)
        c.xv[rows, c.t] = torch.where(rows % 3 != 1, big, 1.0).to(c.case.dtype)
        r0 = rows[rows % 3 == 0]
        c.xv[r0, (c.t[r0] + 1) % v] = big
    return edit


# quantum of the logits and size of the per-row shift c: x + c is exact in the dtype
_SHIFT = {torch.float32: (1 / 64, 16384.0), torch.bfloat16: (0.5, 32.0), torch.float16: (0.125, 64.0)}


def shifted(apply: bool):
    def edit(c: Ctx) -> None:
        q, size = _SHIFT[c.case.dtype]
        x = torch.round(c.xv.double().clamp(-4, 4) / q) * q
        if apply:
            x = x + size * (torch.arange(x.shape[0]) % 3 - 1).double()[:, None]
        c.xv.copy_(x)
        assert torch.equal(c.xv.double(), x)
    return edit


def pad_with(value: int):
    """Three rows in ten carry ``value`` as their target."""
    def edit(c: Ctx) -> None:
        c.t[torch.rand(c.t.shape, generator=c.g) < 0.3] = value
        c.t[0], c.t[1] = value, (value + 1) % c.case.v
    return edit


def all_rows(value: int):
    return lambda c: c.t.fill_(value)


def _layouts(dtype, vec_v: int, split_v: int, split_off: int):
    """One VEC and one split layout: (tag, dict of Case fields)."""
    pad = 7 if (split_off + split_v) % 2 == 0 else 6  # odd row stride: every head length occurs
    return (
        (f"vec{vec_v}", dict(dtype=dtype, b=2, s=4, v=vec_v)),
        (f"split{split_v}o{split_off}", dict(dtype=dtype, b=2, s=8, v=split_v, off=split_off, pad=pad)),
    )


def _make_cases() -> List[Case]:
    out: List[Case] = []

    def add(group, name, dt_, /, **kw):
        out.append(Case(id=f"{group}-{name}-{_NAME[dt_]}", group=group, **kw))

    for dt in DTYPES:
        # ---- masked, VEC arms (storage 16-B aligned, v % 16 == 0), 8 to 12 rows
        vec = dict(dtype=dt, b=2, s=4, expect="finite")
        # lane 0's only chunk: the lane is still empty, so the old arithmetic drops its NaN
        add("mask_vec", "v32_chunk0", dt, v=32, edit=mask_cols((0, 16)), old="finite", **vec)
        # lane 0's whole U2 pair (its only step): dropped in the same way
        add("mask_vec", "v2048_pair", dt, v=2048, edit=mask_cols((0, 16), (1024, 1040)), old="finite", **vec)
        add("mask_vec", "v2048_halfpair", dt, v=2048, edit=mask_cols((0, 16)), old="finite", **vec)
        # the leftover chunk16 of lane 0 after its pair: a finite maximum meets an all -inf step
        add("mask_vec", "v3072_leftover", dt, v=3072, edit=mask_cols((2048, 2064)), old="nan", **vec)
        # a padded vocabulary: the second pair of most lanes is all -inf
        add("mask_vec", "v4096_last2100", dt, v=4096, edit=mask_last(2100), old="nan", **vec)
        # a lane's second pair after a finite first one
        add("mask_vec", "v4096_pair2", dt, v=4096, edit=mask_cols((2048, 2064), (3072, 3088)), old="nan", **vec)
        for v, old in ((32, "finite"), (2048, "finite"), (4112, "nan")):
            add("mask_vec", f"v{v}_keep3", dt, v=v, edit=keep3, old=old, dtype=dt, b=3, s=4, expect="finite")

        # ---- masked, split arms: column offsets into a wider buffer, odd row strides
        for off, v in ((1, 5), (2, 5), (3, 5), (1, 40), (2, 40), (3, 40), (1, 1001), (2, 1001), (3, 1001), (3, 50257)):
            pad = 7 if (off + v) % 2 == 0 else 6
            lay = dict(dtype=dt, b=2, s=3 if v > 5000 else 8, v=v, off=off, pad=pad, expect="finite")
            add("mask_split", f"v{v}o{off}_head", dt, edit=mask_part("head"), old="finite", **lay)
            if v >= 40:
                add("mask_split", f"v{v}o{off}_body", dt, edit=mask_part("body"), old="nan", **lay)
            add("mask_split", f"v{v}o{off}_tail", dt, edit=mask_part("tail"), old="finite", **lay)
            # whether a lane meets an all -inf chunk after a finite value is up to the draw at v <= 1001
            add("mask_split", f"v{v}o{off}_keep3", dt, edit=keep3, old="nan" if v > 5000 else None, **lay)

        # ---- expected non-finite results, NaN logits, magnitudes, targets: one VEC, one split layout
        for tag, lay in _layouts(dt, 2048, 1001, 1):
            add("nonfinite", f"{tag}_target_masked", dt, edit=target_on_masked, expect="inf", **lay)
            add("nonfinite", f"{tag}_row_all_masked", dt, edit=neg_inf_row(False), expect="nan", **lay)
            add("nonfinite", f"{tag}_row_all_masked_ignored", dt, edit=neg_inf_row(True), expect="finite",
                ignore_index=-100, **lay)
            add("nonfinite", f"{tag}_pos_inf", dt, edit=pos_inf_logit, expect="nan", **lay)
        for tag, lay in _layouts(dt, 2048, 1001, 3) + _layouts(dt, 32, 40, 1)[1:]:
            split = tag.startswith("split")
            short = tag.startswith("split40")
            add("nan_logit", f"{tag}_body", dt, edit=nan_logit("body"), expect="nan", old="nan", **lay)
            add("nan_logit", f"{tag}_body_ignored", dt, edit=nan_logit("body", True), expect="finite",
                ignore_index=-100, **lay)
            if split:
                add("nan_logit", f"{tag}_head", dt, edit=nan_logit("head"), expect="nan", old="finite", **lay)
                # the last tail lane of a 40-wide row has no head value and no body chunk
                add("nan_logit", f"{tag}_tail", dt, edit=nan_logit("tail"), expect="nan",
                    old="finite" if short else "nan", **lay)
                add("nan_logit", f"{tag}_head_ignored", dt, edit=nan_logit("head", True), expect="finite",
                    ignore_index=-100, **lay)
        for tag, lay in _layouts(dt, 2048, 1001, 1):
            same = f"shift-{tag}-{_NAME[dt]}"
            add("magnitude", f"{tag}_shift_base", dt, edit=shifted(False), expect="finite", seed=same, **lay)
            add("magnitude", f"{tag}_shift_moved", dt, edit=shifted(True), expect="finite", seed=same, **lay)
            if dt == torch.float32:
                add("magnitude", f"{tag}_x1e4", dt, edit=near_ties, expect="finite", scale=4e4, **lay)
            else:
                big = 65504.0 if dt == torch.float16 else 3e38
                add("magnitude", f"{tag}_extremes", dt, edit=extremes(big), expect="finite", **lay)
        for tag, lay in _layouts(dt, 2048, 1001, 1):
            add("targets", f"{tag}_int32", dt, edit=plain, expect="finite", tgt="i32", **lay)
            add("targets", f"{tag}_stride2", dt, edit=plain, expect="finite", tgt="i64s2", **lay)
            add("targets", f"{tag}_stride2_int32", dt, edit=pad_with(-100), expect="finite", tgt="i32s2",
                ignore_index=-100, **lay)
            add("targets", f"{tag}_pad_minus100", dt, edit=pad_with(-100), expect="finite", ignore_index=-100, **lay)
            add("targets", f"{tag}_ignore0", dt, edit=pad_with(0), expect="finite", ignore_index=0, **lay)
            add("targets", f"{tag}_all_ignored", dt, edit=all_rows(7), expect="nan", ignore_index=7, **lay)

        # ---- the split walk on plain logits at the smallest shape that reaches all of it: columns
        # 1:2086 of a [5, 2087] buffer.  Five rows are one more than a block's waves; the odd stride
        # gives every row another head; the body of 2064 or 2080 values runs the two-step loop in
        # every lane and the single step in the low ones, and a tail is left
        add("walk", "v2085o1", dt, dtype=dt, b=1, s=5, v=2085, off=1, pad=1, edit=plain, expect="finite")

        # ---- the arms without the unrolled body (rows > 16384, short rows), four rows per wave of
        # the capped grid; v = 33 is a contiguous split arm whose rows have every head length
        tall = dict(dtype=dt, b=2, s=8200, expect="finite")
        add("no_u2", "v32", dt, v=32, edit=plain, **tall)
        add("no_u2", "v33", dt, v=33, edit=plain, **tall)
        add("no_u2", "v1040", dt, v=1040, edit=plain, **tall)
        add("no_u2", "v32_masked", dt, v=32, edit=mask_cols((0, 16)), old="finite", **tall)
        add("no_u2", "v33_masked", dt, v=33, edit=mask_part("body"), old="nan", **tall)
        # lane 0's second chunk16 (columns 1024..1039) after a finite first one
        add("no_u2", "v1040_masked", dt, v=1040, edit=mask_cols((1024, 1040)), old="nan", **tall)

    # float32 just past the 512-block cap rule: 1024 blocks, more than two rows per wave
    for v in (32, 33):
        add("grid", f"rows8193_v{v}", torch.float32, dtype=torch.float32, b=1, s=8193, v=v, edit=plain, expect="finite")
    return out


CASES = _make_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def coverage(cases=CASES):
    """The (kind, vec, u2) arms and the grid regimes (rows <= waves, rows > waves) of ``cases``."""
    arms, regimes = set(), set()
    for c in cases:
        kind, vec, u2, grid = c.arm()
        arms.add((kind, vec, u2))
        regimes.add(c.rows > grid * 4)
    return arms, regimes


def assert_full_coverage(cases=CASES) -> None:
    arms, regimes = coverage(cases)
    want = {(k, vec, u2) for k in range(3) for vec in (False, True) for u2 in (False, True)}
    assert arms == want, f"K7 arms not reached: {sorted(want - arms)}"
    assert regimes == {False, True}, f"K7 grid regimes reached: {regimes}"


assert_full_coverage()
