"""Live EQ: sistema_ecualizador block by block with gains that may change
between two blocks without a click (include/dspcore_eqlive.h).

A live EQ has a fixed, ordered list of band slots -- the keys of the gains dict
it is made with.  Every slot always runs a biquad: the band's peaking section
while |g| > 0.1, the flat section (the same design at g = 0, b == a) otherwise,
so a band that is switched off rings out through its poles instead of being
cut.  Each channel carries scipy's `zi` of every band (direct form II
transposed), which is a state of the signal and not of the coefficients; per
channel the output of a stream is

    for each block, with that block's gains:
        v = float64(block)
        for k in slots:  v, s[k] = scipy.signal.lfilter(b_k, a_k, v, zi=s[k])
        z = float32(clip(v, -1, 1))   if not all(|g| < 0.1)   else float32(v)

The planning is host work and needs no GPU (LivePlanner): identical settings
merge into groups, a channel none of whose slots has been active since the last
reset is a copy (the reference's bypass).  A LiveEq owns the device table, the
int32 group index of every row and the state; apply() is one launch
(`iir_live`), set_gains() overwrites the two buffers in place.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops
from .design import live_active, live_slots, live_sos

TABLE_ALIGN = 256        # bytes: the device table's alignment (include/dspcore_eqlive.h)
MAX_GROUPS_DEFAULT = 256


@dataclass(frozen=True)
class LivePlan:
    """Host plan of one gain setting of the whole batch."""
    sos: np.ndarray          # float64 [G][slots][5] = {b0 b1 b2 a1 a2}, in order of first use
    clip: np.ndarray         # int32 [G]
    copy: np.ndarray         # int32 [G]: rows that have never been active are copied
    row_group: np.ndarray    # int32 [B]
    ever_active: np.ndarray  # bool [B]: the rows' activity once this plan is in force

    @property
    def G(self) -> int:
        return int(self.sos.shape[0])


class LivePlanner:
    """The host side of a LiveEq: the band slots, every row's current gains
    and whether any of its slots has been active since the last reset."""

    def __init__(self, fs: float, gains, batch: int | None = None,
                 max_groups: int | None = None):
        if not isinstance(gains, dict):
            gains = list(gains)
        first = gains if isinstance(gains, dict) else (gains or [None])[0]
        if not isinstance(first, dict):
            raise ValueError("a live EQ takes one gains dict or a sequence of them")
        self.fs = fs
        self.slots = live_slots(fs, first.keys())
        if batch is None:
            batch = 1 if isinstance(gains, dict) else len(gains)
        self.B = int(batch)
        if self.B < 1:
            raise ValueError("a live EQ needs at least one channel")
        self.max_groups = (min(self.B, MAX_GROUPS_DEFAULT) if max_groups is None
                           else int(max_groups))
        if self.max_groups < 1:
            raise ValueError("max_groups must be >= 1")
        self.ever_active = np.zeros(self.B, dtype=bool)
        self.gains = None
        self.commit(self.plan(gains), gains)

    @property
    def n_slots(self) -> int:
        return len(self.slots.keys)

    def _per_row(self, gains) -> list:
        rows = [gains] * self.B if isinstance(gains, dict) else list(gains)
        if len(rows) != self.B:
            raise ValueError(f"{len(rows)} gain sets for {self.B} channels")
        return rows

    def plan(self, gains, ever_active: np.ndarray | None = None) -> LivePlan:
        """The plan of `gains` (one dict, or one per row) on top of the rows'
        activity so far.  Changes nothing; every error is raised here."""
        rows = self._per_row(gains)
        ever = (self.ever_active if ever_active is None else ever_active).copy()
        index: dict = {}
        sos_g, clip_g, copy_g, row_group = [], [], [], []
        for b, g in enumerate(rows):
            if not isinstance(g, dict):
                raise ValueError("a live EQ takes one gains dict or a sequence of them")
            ever[b] |= any(live_active(self.slots, g))      # (checks the keys)
            sos, clip = live_sos(self.fs, self.slots, g)
            key = (sos.tobytes(), clip, not ever[b])
            if key not in index:
                index[key] = len(sos_g)
                sos_g.append(sos)
                clip_g.append(clip)
                copy_g.append(not ever[b])
            row_group.append(index[key])
        if len(sos_g) > self.max_groups:
            raise ValueError(f"{len(sos_g)} distinct settings for max_groups={self.max_groups}")
        return LivePlan(np.ascontiguousarray(np.stack(sos_g)), np.asarray(clip_g, dtype=np.int32),
                        np.asarray(copy_g, dtype=np.int32),
                        np.asarray(row_group, dtype=np.int32), ever)

    def commit(self, plan: LivePlan, gains) -> None:
        self.gains = [dict(g) for g in self._per_row(gains)]
        self.ever_active = plan.ever_active.copy()

    def reset(self) -> LivePlan:
        """The current gains from rest: only what they make active counts."""
        plan = self.plan(self.gains, np.zeros(self.B, dtype=bool))
        self.ever_active = plan.ever_active.copy()
        return plan


def build_table(plan: LivePlan, max_n: int, max_groups: int | None = None) -> np.ndarray:
    """The table as dsp_eqlive_build fills it (host only): uint8 [max_groups *
    DSP_EQLIVE_RECORD_BYTES], the records past the plan's G zero."""
    lib = _lib.load()
    G = plan.G
    total = G if max_groups is None else int(max_groups)
    if total < G:
        raise ValueError(f"{G} groups for max_groups={total}")
    table = np.zeros(int(lib.dsp_eqlive_bytes(total)), dtype=np.uint8)
    sos = np.ascontiguousarray(plan.sos, dtype=np.float64)
    rc = lib.dsp_eqlive_build(table.ctypes.data, table.size, _lib.sos_pointer(sos),
                              plan.clip.ctypes.data, plan.copy.ctypes.data, G,
                              int(sos.shape[1]), int(max_n))
    _lib.check(rc, "dsp_eqlive_build")
    return table


class LiveEq:
    """sistema_ecualizador over `batch` channels, block by block, with
    set_gains() between blocks.

    gains is one dict for every channel or a sequence of `batch` dicts; its
    keys, in order, are the band slots (at most 8) that every later dict must
    repeat.  max_n is the longest block apply() will take.  The device table
    holds max_groups records (default min(batch, 256)) and, like the row-group
    array and the state, keeps its address for the object's life, so a captured
    apply() follows later set_gains() calls."""

    def __init__(self, fs: float, gains, max_n: int, device: torch.device | str = "cuda",
                 batch: int | None = None, max_groups: int | None = None):
        self.planner = LivePlanner(fs, gains, batch, max_groups)
        self.max_n = int(max_n)
        if self.max_n < 1:
            raise ValueError("max_n must be >= 1")
        self.B, self.max_groups, self.slots = (self.planner.B, self.planner.max_groups,
                                               self.planner.n_slots)
        plan = self.planner.plan(self.planner.gains)
        host = build_table(plan, self.max_n, self.max_groups)     # host checks before any GPU work
        ops.require_gpu()
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # one allocation, the table at its first 256-byte boundary
        self._raw = torch.zeros(host.size + TABLE_ALIGN, dtype=torch.uint8, device=self.device)
        at = -self._raw.data_ptr() % TABLE_ALIGN
        self.table = self._raw[at:at + host.size]
        self.row_group = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._state = torch.zeros((self.B, 2 * self.slots), dtype=torch.float64,
                                  device=self.device)
        self._upload(host, plan)

    # -- gains and state -----------------------------------------------------------
    def _upload(self, host: np.ndarray, plan: LivePlan) -> None:
        """Overwrites the table and the row groups in place, in stream order."""
        self.table.copy_(torch.from_numpy(host))
        self.row_group.copy_(torch.from_numpy(plan.row_group))

    def set_gains(self, gains) -> None:
        """New gains (one dict, or one per channel) from the next apply() on.
        Re-plans on the host and overwrites the device table and the row groups
        in place, ordered on the current stream; may block the host.  More
        distinct settings than max_groups, or a dict that does not keep the
        band slots, is a ValueError raised before anything is written."""
        if not isinstance(gains, dict):
            gains = list(gains)
        plan = self.planner.plan(gains)
        host = build_table(plan, self.max_n, self.max_groups)
        self._upload(host, plan)
        self.planner.commit(plan, gains)

    def reset(self) -> None:
        """Every band at rest; a channel none of whose current slots is active
        is a copy again."""
        plan = self.planner.reset()
        self._upload(build_table(plan, self.max_n, self.max_groups), plan)
        self._state.zero_()

    def state_dict(self) -> dict:
        """{"zi": float64 [batch, 2 * slots] = (s1_0, s2_0, s1_1, ...) per
        channel, slot k's pair scipy.signal.lfilter's zi of that band;
        "ever_active": bool [batch]} as host tensors.  Synchronises."""
        return {"zi": self._state.cpu(),
                "ever_active": torch.from_numpy(self.planner.ever_active.copy())}

    def load_state_dict(self, sd: dict) -> None:
        """Continues from a state_dict(), or from lfilter states alone ({"zi":
        ...}): a row whose state is not at rest counts as active."""
        zi = torch.as_tensor(sd["zi"], dtype=torch.float64)
        if tuple(zi.shape) != tuple(self._state.shape):
            raise ValueError(f"zi must be [{self.B}, {2 * self.slots}], got {tuple(zi.shape)}")
        ever = (zi != 0).any(dim=1).numpy()
        if sd.get("ever_active") is not None:
            given = np.asarray(sd["ever_active"], dtype=bool).reshape(-1)
            if given.size != self.B:
                raise ValueError("ever_active is of another batch size")
            ever = ever | given
        plan = self.planner.plan(self.planner.gains, ever)
        self._upload(build_table(plan, self.max_n, self.max_groups), plan)
        self.planner.ever_active = plan.ever_active.copy()
        self._state.copy_(zi)

    # -- one block ---------------------------------------------------------------
    def apply(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """z for the block x: float32 CUDA [batch, n <= max_n], from the state
        the previous block left and leaving its own.  One launch; with `out`
        given (it may be x) nothing is allocated and nothing synchronises."""
        x = ops._rows(x, "x")
        if x.dtype != torch.float32:
            x = x.float()
        B, n = x.shape
        if B != self.B:
            raise ValueError(f"the live EQ holds {self.B} channels, x has {B} rows")
        if n > self.max_n:
            raise ValueError(f"n={n} > the live EQ's max_n={self.max_n}")
        if x.device != self.device:
            raise ValueError(f"x is on {x.device}, the live EQ on {self.device}")
        if out is None:
            out = torch.empty_like(x)
        elif (not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (B, n)
              or (n and out.stride(1) != 1)):
            raise ValueError(f"out must be a float32 CUDA [{B}, {n}] tensor with contiguous rows")
        lib = _lib.load()
        with torch.cuda.device(x.device):
            rc = lib.dsp_eqlive_cascade_f32(
                ops._ptr(x), ops._ptr(out), B, n, ops.ld(x), ops.ld(out), self.table.data_ptr(),
                self.table.numel(), self.max_groups, self.slots, self.max_n,
                self.row_group.data_ptr(), self._state.data_ptr(), self._state.data_ptr(),
                self._state.stride(0), ops._stream(x.device))
        _lib.check(rc, "dsp_eqlive_cascade_f32")
        return out
