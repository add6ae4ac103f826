"""Per-channel EQ: a bank of biquad cascades, one gain set per row of the
batch (include/dspcore_eqbank.h).

The planning is host work and needs no GPU: every channel's gains dict goes
through design.eq_plan, identical plans are merged into groups (B channels
with three distinct slider settings make three groups), and the library builds
one fixed-size record per group (dsp_eqbank_build).  An EqBank holds the
device copy of that table and the int32 group index of every row; apply() is
one launch (`iir_bank`) for the whole batch, with the entry and exit state of
ops.biquad_cascade_state.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import numpy as np
import torch

from . import _lib, ops
from .design import eq_plan

BANK_ALIGN = 256   # bytes: the device table's alignment (include/dspcore_eqbank.h)


@dataclass(frozen=True)
class BankPlan:
    """Host plan of a bank: the distinct cascades and who runs which."""
    groups: tuple            # ((sos float64 [S_g][5], clip bool), ...) in order of first use
    row_group: np.ndarray    # int32 [B]: row b runs groups[row_group[b]]

    @property
    def G(self) -> int:
        return len(self.groups)

    @property
    def B(self) -> int:
        return int(self.row_group.size)

    @property
    def stages(self) -> tuple:
        return tuple(int(s.shape[0]) for s, _ in self.groups)

    @property
    def max_stages(self) -> int:
        return max(self.stages)


def _check_groups(groups) -> tuple:
    out = []
    for g, (sos, clip) in enumerate(groups):
        sos = np.ascontiguousarray(sos, dtype=np.float64).reshape(-1, 5)
        if sos.shape[0] > _lib.DSP_EQBANK_MAX_STAGES:
            raise RuntimeError(f"group {g}: the EQ bank takes <= {_lib.DSP_EQBANK_MAX_STAGES} "
                               f"stages (got {sos.shape[0]})")
        out.append((sos, bool(clip)))
    if not out:
        raise ValueError("an EQ bank needs at least one group")
    return tuple(out)


def plan_bank(fs: float, gains_per_channel: Sequence[dict], batch: int | None = None) -> BankPlan:
    """design.eq_plan for every channel's gains dict, identical plans merged.

    A plan is its second-order sections in dict order (the order the bands
    are applied in) and its clip; two dicts that differ only in bands the
    reference skips (|g| <= 0.1) share a group.  A channel whose every |g| <
    0.1 is the reference's EQ bypass: a group of no stage and no clip
    (dsp_core.py:222-223 returns the input as it is)."""
    if isinstance(gains_per_channel, dict):
        raise ValueError("an EQ bank takes a sequence of gains dicts, one per channel")
    gains_per_channel = list(gains_per_channel)
    if batch is not None and len(gains_per_channel) != int(batch):
        raise ValueError(f"{len(gains_per_channel)} gain sets for {int(batch)} channels")
    if not gains_per_channel:
        raise ValueError("an EQ bank needs at least one channel")
    index: dict = {}
    groups, rows = [], []
    for gains in gains_per_channel:
        plan = eq_plan(fs, gains)
        sos = np.ascontiguousarray(plan.sos, dtype=np.float64).reshape(-1, 5)
        key = (bool(plan.bypass), sos.tobytes())
        if key not in index:
            index[key] = len(groups)
            groups.append((sos, not plan.bypass))
        rows.append(index[key])
    return BankPlan(_check_groups(groups), np.asarray(rows, dtype=np.int32))


def plan_from_sos(list_of_sos, clip, row_group) -> BankPlan:
    """A plan from the caller's own cascades: list_of_sos[g] is float64 [S_g][5]
    = {b0 b1 b2 a1 a2}, clip one flag or one per group, row_group[b] in
    [0, G) (checked here: the kernel answers a bad index with NaN rows)."""
    list_of_sos = list(list_of_sos)
    G = len(list_of_sos)
    clips = [bool(clip)] * G if np.isscalar(clip) else [bool(c) for c in clip]
    if len(clips) != G:
        raise ValueError(f"{len(clips)} clip flags for {G} groups")
    groups = _check_groups(zip(list_of_sos, clips))
    rows = np.asarray(row_group)
    if rows.ndim != 1 or rows.size == 0 or not np.issubdtype(rows.dtype, np.integer):
        raise ValueError("row_group must be a non-empty 1-D integer sequence")
    if int(rows.min()) < 0 or int(rows.max()) >= G:
        raise ValueError(f"row_group holds an index outside [0, {G})")
    return BankPlan(groups, np.ascontiguousarray(rows, dtype=np.int32))


def build_table(plan: BankPlan, max_n: int) -> np.ndarray:
    """The bank's table as dsp_eqbank_build fills it (host only): uint8
    [G * DSP_EQBANK_RECORD_BYTES]."""
    lib = _lib.load()
    G, ld = plan.G, max(plan.max_stages, 1)
    sos = np.zeros((G, ld, 5), dtype=np.float64)
    for g, (s, _) in enumerate(plan.groups):
        sos[g, :s.shape[0]] = s
    stages = np.asarray(plan.stages, dtype=np.int32)
    clip = np.asarray([c for _, c in plan.groups], dtype=np.int32)
    table = np.zeros(int(lib.dsp_eqbank_bytes(G)), dtype=np.uint8)
    rc = lib.dsp_eqbank_build(table.ctypes.data, table.size, _lib.sos_pointer(sos),
                              stages.ctypes.data, clip.ctypes.data, G, ld, int(max_n))
    _lib.check(rc, "dsp_eqbank_build")
    return table


class EqBank:
    """sistema_ecualizador with its own gains per channel: row b of a batch is
    filtered with gains_per_channel[b] at the rate fs.

    max_n is the longest block apply() will take; it fixes the chunk length
    of every call (32 ceil(max_n / 2048) samples), so blocks of varying length
    share one table.  Whenever a block's own 32 ceil(n / 2048) is that length,
    row b is bitwise ops.biquad_cascade_state on that row alone with its
    plan's sos and clip."""

    def __init__(self, fs: float, gains_per_channel: Sequence[dict], max_n: int,
                 device: torch.device | str = "cuda", *, batch: int | None = None):
        self._init(plan_bank(fs, gains_per_channel, batch), max_n, device)

    @classmethod
    def from_sos(cls, list_of_sos, clip, row_group, max_n: int,
                 device: torch.device | str = "cuda") -> "EqBank":
        """A bank of the caller's own cascades (plan_from_sos)."""
        self = cls.__new__(cls)
        self._init(plan_from_sos(list_of_sos, clip, row_group), max_n, device)
        return self

    def _init(self, plan: BankPlan, max_n, device) -> None:
        self.plan = plan
        self.max_n = int(max_n)
        if self.max_n < 1:
            raise ValueError("max_n must be >= 1")
        self.B, self.G, self.max_stages = plan.B, plan.G, plan.max_stages
        host = build_table(plan, self.max_n)      # host checks before any GPU work
        ops.require_gpu()
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # one allocation, the table at its first 256-byte boundary
        self._raw = torch.empty(host.size + BANK_ALIGN, dtype=torch.uint8, device=self.device)
        at = -self._raw.data_ptr() % BANK_ALIGN
        self.table = self._raw[at:at + host.size]
        self.table.copy_(torch.from_numpy(host))
        self.row_group = torch.from_numpy(plan.row_group).to(self.device)

    @property
    def state_width(self) -> int:
        """Columns of a state tensor: 2 * (the largest stage count), >= 1."""
        return max(2 * self.max_stages, 1)

    def apply(self, x: torch.Tensor, zi: torch.Tensor | None = None,
              out: torch.Tensor | None = None,
              zf: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """(z, zf) as ops.biquad_cascade_state, row b through its own cascade.
        x: float32 CUDA [B, n <= max_n].  zi, zf: float64 CUDA [B, >= 2 *
        max_stages]; row b uses its first 2 S_b elements, the rest is left
        alone (zi=None starts from rest, zf=None allocates, zi may be zf, out
        may be x).  Bypass rows are copied unclipped and keep their state."""
        x = ops._rows(x, "x")
        if x.dtype != torch.float32:
            x = x.float()
        B, n = x.shape
        if B != self.B:
            raise ValueError(f"the bank holds {self.B} gain sets, x has {B} rows")
        if n > self.max_n:
            raise ValueError(f"n={n} > the bank's max_n={self.max_n}")
        if x.device != self.device:
            raise ValueError(f"x is on {x.device}, the bank on {self.device}")
        width = 2 * self.max_stages
        if out is None:
            out = torch.empty_like(x)
        if zf is None:
            zf = torch.zeros((B, self.state_width), dtype=torch.float64, device=x.device)
        for name, t in (("zi", zi), ("zf", zf)):
            if t is None:
                continue
            if (not t.is_cuda or t.dtype != torch.float64 or t.dim() != 2 or t.shape[0] != B
                    or t.shape[1] < width or t.stride(1) != 1):
                raise ValueError(f"{name} must be a float64 CUDA [B={B}, >= {width}] tensor with "
                                 f"contiguous rows")
        ld_state = ops.ld(zf)
        if zi is not None and ops.ld(zi) != ld_state:
            raise ValueError("zi and zf must share one row pitch")
        lib = _lib.load()
        with torch.cuda.device(x.device):
            rc = lib.dsp_eqbank_cascade_f32(
                ops._ptr(x), ops._ptr(out), B, n, ops.ld(x), ops.ld(out), self.table.data_ptr(),
                self.table.numel(), self.G, self.max_stages, self.max_n,
                self.row_group.data_ptr(), ops._ptr(zi), ops._ptr(zf), ld_state,
                ops._stream(x.device))
        _lib.check(rc, "dsp_eqbank_cascade_f32")
        return out, zf
