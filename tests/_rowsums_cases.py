"""Inputs, the launch geometry and the comparison of the K5b row-sums tests.

Shared by tests/metrics/test_rowsums_oracle.py (the host twin, CPU), tests/gpu/test_k5b_arms.py and
the child processes that test starts for TORCHEVAL_AMD_K5B_MODE 1 and 2.  The expected states come
from tests/_rowsums_oracle.py; nothing here computes a statistic.

Two data families:

``exact``  x, t integers in [-8, 8], tensor weights integers in [0, 4], scalar weights from
           {0.5, 2.0, 3.0}.  Every term is an integer or half-integer of magnitude <= 4 * 256 (an
           extremum planted at +-100 raises that to 4 * 108^2 < 2^16) and no row has more than 4.2M
           of them, so every FP64 partial sum, in any order and with or without fused multiply-adds,
           is exact (< 2^39, far below 2^53).  The kernel must reproduce the oracle bit for bit; for
           an f32 output the one rounding of the value is the same on both sides.
``float``  randn / rand float32 data.  Two FP64 summations of the same n terms in different orders
           differ by at most ``2 * n * 2^-53 * S``, S the sum of the absolute terms (each is within
           n * 2^-53 * S of the true sum, to first order).  An f32 output adds its own rounding,
           ``2^-24 * (|want| + |initial state|)``.  Extrema, COUNT and RANGE are exact.  The f64 sum
           outputs of this family start from 0, so that the state update adds no rounding.

The geometry functions restate ``row_sums_blocks``, ``row_sums_fold_blocks`` and
``row_sums_wt_blocks`` of csrc/kernels/rowsums.hip and the spans of ``launch_need``; a case that
names a block count asserts it against them, and ``row_sums_pend`` returns the native count.
"""

import contextlib
import json
import os
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple, Union

import torch

from tests import _rowsums_oracle as O
from tests._rowsums_oracle import ADD, COUNT, FIRST_ROW, MAX, MIN, RANGE, SET, SSE, TMAX, TMIN, W, WSSE, WT, WTT, WX

K_SINGLE = 32768  # rows up to this long: one block per row
GRID_CHUNK = 4096  # row_sums_grid_kernel: 256 threads x 4 float4
WT_CHUNK = 8192  # row_sums_wt_kernel: 256 threads x 8 float4
FOLD_CHUNK = 16384  # row_sums_fold_kernel: 1024 threads x 4 float4
PEND_STATS, PEND_BLOCKS = 9, 2048  # kRowPendStats, kRowPendBlocks
GRID_ENV, MODE_ENV = "TORCHEVAL_AMD_K5B_GRID", "TORCHEVAL_AMD_K5B_MODE"
assert "TORCHEVAL_AMD_K5B_PEND_VPT" not in os.environ, "unset TORCHEVAL_AMD_K5B_PEND_VPT: the cases assume its default"

STAT_NAME = ("WX", "WT", "W", "SSE", "WSSE", "WTT", "TMIN", "TMAX", "COUNT", "RANGE")
# the statistic sets launch_row_sums instantiates by name ...
NAMED_SETS = {
    "sum": (WX,),
    "mean": (WX, W),
    "wc": (WX, WT),
    "psnr_fixed": (SSE,),
    "psnr_auto": (SSE, TMIN, TMAX),
    "mse": (WSSE,),
    "wmse": (WSSE, W),
    "r2": (WT, SSE, WTT),
}
# ... and two that take the generic instantiation (kAll)
GENERIC_SETS = {"all": (WX, WT, W, SSE, WSSE, WTT, TMIN, TMAX, COUNT, RANGE), "wt": (WT,)}
SETS = dict(NAMED_SETS, **GENERIC_SETS, psnr=(SSE, TMIN, TMAX, COUNT, RANGE))  # psnr: the named psnr_auto kernel
SCALARS = (0.5, 2.0, 3.0)
_INF = float("inf")


# ------------------------------------------------------------------ launch geometry
def _ceil(a: int, b: int) -> int:
    return -(-a // b)


def _cap(grid: Optional[int]) -> int:
    return 512 if grid is None else max(1, int(grid))


def blocks_two_launch(rows: int, n: int, grid: Optional[int] = None) -> int:
    """row_sums_blocks: the default arm and the deferred mode."""
    if n <= K_SINGLE:
        return 1
    return min(_ceil(n, GRID_CHUNK), max(2, _cap(grid) // max(rows, 1)))


def blocks_fold(rows: int, n: int) -> int:
    """row_sums_fold_blocks: TORCHEVAL_AMD_K5B_MODE=1."""
    if n <= K_SINGLE:
        return 1
    return min(max(2, 256 // max(rows, 1)), _ceil(n, FOLD_CHUNK))


def blocks_wt(rows: int, n: int, grid: Optional[int] = None) -> int:
    """row_sums_wt_blocks: TORCHEVAL_AMD_K5B_MODE=2."""
    if n <= K_SINGLE:
        return 1
    return min(_ceil(n, WT_CHUNK), max(2, _cap(grid) // max(rows, 1)))


def geometry(mode: int, rows: int, n: int, grid: Optional[int] = None) -> Tuple[int, int]:
    """(blocks per row, blocks among them whose span starts at or behind the row's end)."""
    if mode == 1:
        blocks = blocks_fold(rows, n)
        span = _ceil(_ceil(n, blocks), FOLD_CHUNK) * FOLD_CHUNK
    else:
        chunk = WT_CHUNK if mode == 2 else GRID_CHUNK
        blocks = blocks_wt(rows, n, grid) if mode == 2 else blocks_two_launch(rows, n, grid)
        span = _ceil(_ceil(n, chunk), blocks) * chunk
    if blocks == 1:
        return 1, 0
    return blocks, sum(1 for b in range(blocks) if b * span >= n)


@contextlib.contextmanager
def grid_cap(grid: Optional[int]):
    """TORCHEVAL_AMD_K5B_GRID is read on every call: set for the duration, then put back."""
    old = os.environ.get(GRID_ENV)
    try:
        if grid is None:
            os.environ.pop(GRID_ENV, None)
        else:
            os.environ[GRID_ENV] = str(grid)
        yield
    finally:
        if old is None:
            os.environ.pop(GRID_ENV, None)
        else:
            os.environ[GRID_ENV] = old


def process_mode() -> int:
    e = os.environ.get(MODE_ENV, "")
    return int(e) if e else 0


# ------------------------------------------------------------------ outputs
@dataclass(frozen=True)
class Out:
    stat: int
    op: int
    dtype: torch.dtype
    init: float
    first_row: bool = False  # a 0-d state fed by row 0 only
    ring: bool = False  # column 2 of a zeroed [rows, 4] ring buffer

    @property
    def code(self) -> int:
        return self.op | (FIRST_ROW if self.first_row else 0)


F32, F64 = torch.float32, torch.float64


def outs_for(stats: Sequence[int], style: str) -> List[Out]:
    """``a``: f64 sums added to 1.5 (what the deferred mode can fold); ``b``: f32 sums set, finite
    extrema states, a row-0 COUNT; ``f`` (float family): f64 sums added to 0 and f32 sums added to
    1.5 in turn."""
    outs = []
    for stat in stats:
        if stat == TMIN:
            outs.append(Out(stat, MIN, F64, _INF) if style != "b" else Out(stat, MIN, F32, 0.0))
        elif stat == TMAX:
            outs.append(Out(stat, MAX, F32, -_INF) if style != "b" else Out(stat, MAX, F64, 0.0))
        elif stat == COUNT:
            outs.append(Out(stat, ADD, F32, 2.0) if style != "b" else Out(stat, SET, F64, 5.0, first_row=True))
        elif stat == RANGE:
            outs.append(Out(stat, SET, F64, 9.0) if style != "b" else Out(stat, SET, F32, 9.0))
        elif style == "a":
            outs.append(Out(stat, ADD, F64, 1.5))
        elif style == "b":
            outs.append(Out(stat, SET, F32, 7.0))
        else:
            outs.append(Out(stat, ADD, F64, 0.0) if stat % 2 == 0 else Out(stat, ADD, F32, 1.5))
    return outs


# ------------------------------------------------------------------ cases
@dataclass
class Case:
    id: str
    family: str  # "exact" or "float"
    rows: int
    n: int
    outs: List[Out]
    weight: Union[str, float] = "tensor"  # "tensor", or the scalar weight
    x_dtype: torch.dtype = torch.float32
    t_dtype: torch.dtype = torch.float32
    w_dtype: torch.dtype = torch.float32
    offsets: Optional[Tuple[int, int, int]] = None  # x, t, w as columns o : o + n of [rows, n + 5] buffers
    transposed: bool = False  # x with a column stride
    has_t: bool = True
    grid: Optional[int] = None  # TORCHEVAL_AMD_K5B_GRID
    mode: int = 0  # TORCHEVAL_AMD_K5B_MODE of the process that runs it
    edit: Optional[Tuple[str, int]] = None  # ("nan" | "min" | "max", column) of t, in the last row
    t_offset: int = 0  # added to every target: +-20 keeps 0 out of their range, so a stray zero slot shows
    blocks: Optional[int] = None  # the block count this case is there for
    empty: Optional[int] = None  # ... and its empty-span blocks
    seed: str = ""

    def geometry(self) -> Tuple[int, int]:
        got = geometry(self.mode, self.rows, self.n, self.grid)
        if self.blocks is not None:
            assert got[0] == self.blocks, f"{self.id}: {got[0]} blocks, not the {self.blocks} it was built for"
        if self.empty is not None:
            assert got[1] == self.empty, f"{self.id}: {got[1]} empty blocks, not {self.empty}"
        return got


def _gen(key: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def values(c: Case):
    """Contiguous CPU ``x, t, w`` ([rows, n]; t / w None when absent) in the case's dtypes."""
    g = _gen(c.seed or f"{c.family}-{c.rows}-{c.n}")
    shape = (c.rows, c.n)
    if c.family == "exact":
        lo = 0 if c.x_dtype in (torch.uint8, torch.bool) else -8
        hi = 2 if c.x_dtype == torch.bool else 9
        x = torch.randint(lo, hi, shape, generator=g).to(c.x_dtype)
        t = (torch.randint(-8, 9, shape, generator=g) + c.t_offset).to(c.t_dtype)
        w = torch.randint(0, 5, shape, generator=g).to(c.w_dtype)
    else:
        x = torch.randn(shape, generator=g).to(c.x_dtype)
        t = torch.randn(shape, generator=g).to(c.t_dtype)
        w = torch.rand(shape, generator=g).to(c.w_dtype)
    if c.edit is not None:
        kind, col = c.edit
        assert 0 <= col < c.n
        t[c.rows - 1, col] = {"nan": float("nan"), "min": -100.0, "max": 100.0}[kind]
    return x, (t if c.has_t else None), (w if c.weight == "tensor" else None)


_POISON = 12345.0  # what the gaps of an offset buffer hold: one of them read moves every sum


def place(v: Optional[torch.Tensor], device, offset: Optional[int] = None, transposed: bool = False):
    """``v`` on ``device`` in the layout asked for: contiguous, columns ``offset : offset + n`` of a
    [rows, n + 5] buffer (4-B aligned rows whose stride is n + 5), or a column-strided view."""
    if v is None:
        return None
    rows, n = v.shape
    if offset is not None:
        base = torch.full((rows, n + 5), _POISON, dtype=v.dtype)
        base[:, offset:offset + n] = v
        out = base.to(device)[:, offset:offset + n]
        assert out.stride() == (n + 5, 1) and (n + 5) % 4 != 0 and out.storage_offset() == offset
        return out
    if transposed:
        base = torch.zeros((n, rows + 1), dtype=v.dtype)
        base[:, :rows] = v.t()
        out = base.to(device)[:, :rows].t()
        assert out.shape == (rows, n) and out.stride() == (1, rows + 1)
        return out
    return v.to(device).contiguous()


def make_states(outs: Sequence[Out], rows: int, device):
    """(the output tensors handed to the kernel, the tensor that owns each one's memory)."""
    views, owners = [], []
    for o in outs:
        if o.first_row:
            own = torch.full((), o.init, dtype=o.dtype, device=device)
            view = own
        elif o.ring:
            own = torch.zeros(rows, 4, dtype=o.dtype, device=device)
            own[:, 2] = o.init
            view = own[:, 2]
        else:
            own = torch.full((rows,), o.init, dtype=o.dtype, device=device)
            view = own
        views.append(view)
        owners.append(own)
    return views, owners


def expected_states(c: Case, x, t, w):
    init, _ = make_states(c.outs, c.rows, "cpu")
    ws = 1.0 if c.weight == "tensor" else float(c.weight)
    return O.rowsums_oracle(x, t, w, ws, [(s, o.stat, o.code) for s, o in zip(init, c.outs)], c.rows)


def bounds(c: Case, x, t, w, want: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """float64 per output element: what ``|got - want|`` may be (0: exact)."""
    ws = 1.0 if c.weight == "tensor" else float(c.weight)
    out = []
    for o, wt in zip(c.outs, want):
        b = torch.zeros(wt.reshape(-1).shape, dtype=torch.float64)
        if c.family == "float" and o.stat not in (TMIN, TMAX, COUNT, RANGE):
            assert o.op in (SET, ADD) and (o.dtype == F32 or o.op == SET or o.init == 0.0)
            s = O.row_values(x, t, w, ws, o.stat, c.rows, absolute=True)
            b = 2.0 * c.n * 2.0 ** -53 * (s[:1] if o.first_row else s)
            if o.dtype == F32:
                b = b + 2.0 ** -24 * (wt.reshape(-1).double().abs() + abs(o.init))
        out.append(b)
    return out


def compare(cid: str, outs: Sequence[Out], got: Sequence[torch.Tensor], want: Sequence[torch.Tensor],
            bound: Optional[Sequence[torch.Tensor]] = None, tag: str = "") -> List[dict]:
    """The output elements that miss: equal or both NaN where the bound is 0, within it elsewhere."""
    bad = []
    for k, o in enumerate(outs):
        g, w = got[k].detach().cpu().reshape(-1), want[k].reshape(-1)
        assert g.dtype == w.dtype == o.dtype and g.shape == w.shape, (cid, k, g.dtype, w.dtype, g.shape, w.shape)
        g, w = g.double(), w.double()
        b = torch.zeros_like(w) if bound is None else bound[k]
        same = (g == w) | (torch.isnan(g) & torch.isnan(w))
        ok = same | ((b > 0) & ((g - w).abs() <= b))
        for r in (~ok).nonzero().reshape(-1).tolist():
            bad.append({"case": cid + tag, "out": k, "stat": STAT_NAME[o.stat], "row": r, "got": repr(float(g[r])),
                        "want": repr(float(w[r])), "bound": float(b[r])})
    return bad


def _ring_untouched(cid: str, outs: Sequence[Out], owners) -> List[dict]:
    bad = []
    for k, (o, own) in enumerate(zip(outs, owners)):
        if o.ring and float(own[:, [0, 1, 3]].abs().sum()) != 0.0:
            bad.append({"case": cid, "out": k, "stat": STAT_NAME[o.stat], "row": -1, "got": "ring slots written",
                        "want": "columns 0, 1, 3 left at 0", "bound": 0.0})
    return bad


def native():
    from torcheval_amd.ops import native as _native

    return _native()


def run_case(c: Case, device, repeat: int = 1) -> List[dict]:
    """Run ``native().row_sums`` on the case ``repeat`` times from fresh states; every run is held
    to the oracle and, bit for bit, to the first run."""
    on_gpu = torch.device(device).type == "cuda"
    if on_gpu:
        assert process_mode() == c.mode, f"{c.id}: needs {MODE_ENV}={c.mode}"
        c.geometry()
    x, t, w = values(c)
    want = expected_states(c, x, t, w)
    bound = bounds(c, x, t, w, want)
    ox, ot, ow = c.offsets if c.offsets is not None else (None, None, None)
    xd, td, wd = place(x, device, ox, c.transposed), place(t, device, ot), place(w, device, ow)
    ws = 1.0 if c.weight == "tensor" else float(c.weight)
    codes = [o.stat * 8 + o.code for o in c.outs]
    bad, first = [], None
    with grid_cap(c.grid):
        for rep in range(repeat):
            states, owners = make_states(c.outs, c.rows, device)
            native().row_sums(xd, td, wd, ws, states, codes, c.rows)
            got = [s.detach().cpu() for s in states]
            bad += compare(c.id, c.outs, got, want, bound, tag=f" (run {rep})" if repeat > 1 else "")
            bad += _ring_untouched(c.id, c.outs, owners)
            if first is None:
                first = got
            else:
                bad += compare(c.id, c.outs, got, first, None, tag=f" (run {rep} against run 0)")
    return bad


def run_cases(cases: Sequence[Case], device, repeat: int = 1) -> List[dict]:
    """The failures of ``cases`` as data (an empty list: all of them hold)."""
    bad = []
    for c in cases:
        bad += run_case(c, device, repeat)
    return bad


def _weights():
    """'tensor', then the scalars in turn."""
    k = 0
    while True:
        yield "tensor"
        yield SCALARS[k % len(SCALARS)]
        k += 1


N_SINGLE = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8195, 32767, 32768)


def single_cases(set_name: str, family: str = "exact") -> List[Case]:
    """One block per row, float32 unit-stride operands: whole chunks, the masked chunk, the ragged
    tail and nothing but the tail; a tensor and a scalar weight each."""
    out, k = [], 0
    for rows in (1, 3):
        for n in N_SINGLE:
            for wk, weight in enumerate(("tensor", SCALARS[k % 3])):
                style = "f" if family == "float" else "ab"[(k + wk) % 2]
                out.append(Case(f"single-{set_name}-r{rows}-n{n}-w{weight}-{style}", family, rows, n,
                                outs_for(SETS[set_name], style), weight=weight, blocks=1, empty=0))
            k += 1
    return out


def alignment_cases() -> List[Case]:
    """The vector path on rows that start at every 4-B alignment, x, t and w each at another."""
    out = []
    for k, offs in enumerate(((1, 2, 3), (2, 3, 1), (3, 1, 2))):
        for rows, n in ((3, 4097), (1, 32769), (3, 32769)):
            for set_name in ("all", "psnr_auto"):
                out.append(Case(f"align-{set_name}-r{rows}-n{n}-o{offs[0]}{offs[1]}{offs[2]}", "exact", rows, n,
                                outs_for(SETS[set_name], "ab"[k % 2]), offsets=offs))
    return out


GENERIC_DTYPES = (torch.float16, torch.bfloat16, torch.float64, torch.int64, torch.int32, torch.int16, torch.int8,
                  torch.uint8, torch.bool)


def generic_cases() -> List[Case]:
    """The strided loader: x in every other dtype, or column-strided, with float32 t and w; one
    block per row at n = 4097, several at 36865."""
    out = []
    for n in (4097, 36865):
        for k, dt in enumerate(GENERIC_DTYPES):
            name = str(dt).replace("torch.", "")
            out.append(Case(f"generic-{name}-n{n}", "exact", 2, n, outs_for(SETS["all"], "ab"[k % 2]), x_dtype=dt,
                            weight="tensor" if k % 2 == 0 else SCALARS[k % 3]))
        out.append(Case(f"generic-transposed-n{n}", "exact", 2, n, outs_for(SETS["all"], "a"), transposed=True))
        out.append(Case(f"generic-transposed-psnr-n{n}", "exact", 2, n, outs_for(SETS["psnr"], "b"), transposed=True,
                        weight=2.0))
    return out


N_1026 = GRID_CHUNK * 1025 + 1  # 1026 partials under a grid cap of 2000: the largest input, 4.2M elements
N_66 = GRID_CHUNK * 65 + 1  # 66 partials per row


def combine_cases(family: str = "exact") -> List[Case]:
    """rows = 1, two launches: row_sums_combine_kernel."""
    style = "f" if family == "float" else "a"
    # 37891 = 9 whole chunks, then a masked chunk of 256 float4 and a tail of 3 in the last block
    geo = [(32769, None, 9, 0), (36864, None, 9, 0), (36865, None, 10, 0), (37891, None, 10, 0), (40963, None, 11, 0),
           (36865, 2, 2, 0), (32769, 4, 4, 1), (N_1026, 2000, 1026, 0)]
    out, wts = [], _weights()
    for n, grid, blocks, empty in geo:
        for set_name in (("all",) if family == "float" or n == N_1026 else ("all", "psnr", "mean")):
            out.append(Case(f"combine-{family}-{set_name}-n{n}-g{grid}", family, 1, n, outs_for(SETS[set_name], style),
                            weight=next(wts), grid=grid, blocks=blocks, empty=empty))
    return out


def combine_rows_cases(family: str = "exact") -> List[Case]:
    """rows > 1, two launches: row_sums_combine_rows_kernel, one wave per row, four rows per block."""
    style = "f" if family == "float" else "b"
    out, wts = [], _weights()
    for rows, n, blocks in ((2, 36865, 10), (4, 36865, 10), (5, 36865, 10), (3, 37891, 10), (2, N_66, 66)):
        for set_name in (("all",) if family == "float" else ("all", "psnr", "r2")):
            out.append(Case(f"rows-{family}-{set_name}-r{rows}-n{n}", family, rows, n, outs_for(SETS[set_name], style),
                            weight=next(wts), blocks=blocks, empty=0))
    return out


# where one special target value goes: (rows, n, grid, blocks, empty, {place: column})
_N_TAIL = 4096 + 1024 + 1  # a whole chunk, a masked chunk of 256 float4, one tail element
EXTREMA_GEOMETRY = (
    (1, _N_TAIL, None, 1, 0, {"first": 0, "whole_chunk": 2000, "masked_chunk": 4500, "tail": _N_TAIL - 1}),
    (3, _N_TAIL, None, 1, 0, {"first": 0, "whole_chunk": 2000, "masked_chunk": 4500, "tail": _N_TAIL - 1}),
    # 9 chunks over 4 blocks of 3: block 2 = [24576, 32769) is the last one that holds anything
    (1, 32769, 4, 4, 1, {"first": 0, "last_block_chunk": 30000, "last_block_tail": 32768}),
    (3, 36865, None, 10, 0, {"first": 0, "middle_block": 20000, "last_block_tail": 36864}),
)


def extrema_cases(kind: str) -> List[Case]:
    """{SSE, TMIN, TMAX, COUNT, RANGE} with one NaN (``nan``), the row's lowest (``min``) or highest
    (``max``) target at each place in turn."""
    out, wts = [], _weights()
    for rows, n, grid, blocks, empty, places in EXTREMA_GEOMETRY:
        assert n % 4 == 1
        for where, col in places.items():
            for style in ("a", "b"):
                out.append(Case(f"extrema-{kind}-r{rows}-n{n}-g{grid}-{where}-{style}", "exact", rows, n,
                                outs_for(SETS["psnr"], style), weight=next(wts), grid=grid, blocks=blocks, empty=empty,
                                edit=(kind, col), t_offset=20 if style == "a" else 0))
    return out


MODE_N = (32769, 49153, 50001, 65537)  # 50001: the last block ends in a masked chunk and a tail of 1
N_514 = WT_CHUNK * 513 + 1  # 514 write-through partials under a grid cap of 2000


def mode_cases(mode: int) -> List[Case]:
    """Long rows for TORCHEVAL_AMD_K5B_MODE 1 (fat-block fold) and 2 (write-through partials)."""
    out, wts = [], _weights()
    for rows in (1, 3):
        for n in MODE_N:
            for family, set_name, style in (("exact", "all", "a"), ("exact", "psnr", "b"), ("exact", "mean", "b"),
                                            ("float", "all", "f")):
                out.append(Case(f"mode{mode}-{family}-{set_name}-r{rows}-n{n}", family, rows, n,
                                outs_for(SETS[set_name], style), weight=next(wts), mode=mode))
    if mode == 2:
        for family, style in (("exact", "a"), ("float", "f")):
            out.append(Case(f"mode2-{family}-all-r1-n{N_514}-g2000", family, 1, N_514, outs_for(SETS["all"], style),
                            weight=next(wts), mode=2, grid=2000, blocks=514, empty=0))
    for c in out:
        assert c.geometry()[0] >= 2
    return out


def child_main(mode: int) -> None:
    """What a child process of tests/gpu/test_k5b_arms.py runs: every case twice on the same stream
    (the second run shows that the tickets were left at zero); one JSON line of failures."""
    assert process_mode() == mode
    cases = mode_cases(mode)
    bad = run_cases(cases, "cuda", repeat=2)
    torch.cuda.synchronize()
    print(json.dumps({"mode": mode, "cases": len(cases), "failures": bad}))


# ------------------------------------------------------------------ the deferred mode
@dataclass
class PendCase:
    id: str
    family: str
    rows: int
    ns: Tuple[int, ...]  # one update each
    weights: Tuple[Union[str, float], ...]
    stats: Tuple[int, ...]
    grid: Optional[int] = None
    t_offset: int = 0
    blocks: Optional[Tuple[int, ...]] = None
    empty: Optional[Tuple[int, ...]] = None
    outs: List[Out] = field(default_factory=list)

    def __post_init__(self):
        self.outs = outs_for(self.stats, "f" if self.family == "float" else "a")
        geo = [geometry(0, self.rows, n, self.grid) for n in self.ns]
        if self.blocks is not None:
            assert tuple(g[0] for g in geo) == self.blocks, (self.id, geo)
        if self.empty is not None:
            assert tuple(g[1] for g in geo) == self.empty, (self.id, geo)
        self.blocks = tuple(g[0] for g in geo)


def pend_cases() -> List[PendCase]:
    out = []
    for rows, blocks in ((1, (10, 18, 9)), (3, (10, 18, 9))):
        for name in ("mean", "wc", "psnr"):
            out.append(PendCase(f"pend-{name}-r{rows}", "exact", rows, (36865, 70001, 32769), (0.5, "tensor", 3.0)
                                if name != "mean" else (0.5, 2.0, "tensor"), SETS[name], blocks=blocks, empty=(0, 0, 0)))
    # 9 chunks over 4 blocks of 3: the fourth slot gets COUNT 0 and must stay out of the extrema, which
    # lie on one side of 0 here
    for off in (20, -20):
        out.append(PendCase(f"pend-psnr-empty-block-t{off:+d}", "exact", 1, (32769, 36865), (2.0, "tensor"),
                            SETS["psnr"], grid=4, t_offset=off, blocks=(4, 4), empty=(1, 0)))
    # the block counts of the two-launch cases, as the native side counts them
    out.append(PendCase("pend-mean-2", "exact", 1, (36865,), (0.5,), SETS["mean"], grid=2, blocks=(2,), empty=(0,)))
    out.append(PendCase("pend-r2-66", "exact", 2, (N_66,), ("tensor",), SETS["r2"], blocks=(66,), empty=(0,)))
    out.append(PendCase("pend-all-1026", "exact", 1, (N_1026,), ("tensor",), SETS["all"], grid=2000, blocks=(1026,),
                        empty=(0,)))
    return out


def pend_float_case() -> PendCase:
    return PendCase("pend-float-all", "float", 3, (70001,), ("tensor",), SETS["all"], blocks=(18,))


def run_pend(c: PendCase, device="cuda") -> List[dict]:
    """The updates of ``c`` into one zeroed pend buffer, then one fold: the block counts returned,
    the states left alone until the fold, the states after it against the oracle applied once per
    update, the buffer zero again, and a second fold that changes nothing."""
    assert process_mode() == 0
    bad = []

    def note(what, got, want):
        bad.append({"case": c.id, "out": -1, "stat": what, "row": -1, "got": repr(got), "want": repr(want), "bound": 0.0})

    pend = torch.zeros(c.rows * PEND_STATS * PEND_BLOCKS, dtype=torch.float64, device=device)
    states, _ = make_states(c.outs, c.rows, device)
    want, _ = make_states(c.outs, c.rows, "cpu")
    initial = [s.clone() for s in want]
    codes = [o.stat * 8 + o.code for o in c.outs]
    bound = None
    used = []
    with grid_cap(c.grid):
        for k, (n, weight) in enumerate(zip(c.ns, c.weights)):
            one = Case(f"{c.id}-update{k}", c.family, c.rows, n, c.outs, weight=weight, t_offset=c.t_offset)
            x, t, w = values(one)
            ws = 1.0 if weight == "tensor" else float(weight)
            want = O.rowsums_oracle(x, t, w, ws, [(s, o.stat, o.code) for s, o in zip(want, c.outs)], c.rows)
            if c.family == "float":
                assert len(c.ns) == 1  # the derived bound is that of one update
                bound = bounds(one, x, t, w, want)
            used.append(int(native().row_sums_pend(place(x, device), place(t, device), place(w, device), ws, states,
                                                   codes, c.rows, pend)))
        if tuple(used) != c.blocks:
            note("blocks returned by row_sums_pend", used, list(c.blocks))
        bad += compare(c.id, c.outs, states, initial, None, tag=" (before the fold)")
        native().row_sums_fold(pend, max(used), states, codes, c.rows)
        got = [s.detach().cpu() for s in states]
        bad += compare(c.id, c.outs, got, want, bound, tag=" (after the fold)")
        left = int((pend != 0).sum())
        if left:
            note("pend slots not zero after the fold", left, 0)
        native().row_sums_fold(pend, max(used), states, codes, c.rows)
        # a fold of zeroed slots adds 0, merges no extrema and sets RANGE from the same states
        bad += compare(c.id, c.outs, states, got, None, tag=" (second fold)")
    return bad
