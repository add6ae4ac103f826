"""Fast convolution: a long FIR by overlap-save on the in-LDS FFT
(include/dspcore_fastconv.h), one-shot and as a stream.

A FastConv holds one set of taps (1 .. 8193, e.g. a band filter or a room
response) for `batch` channels.  Called with a whole signal it convolves it in
np.convolve's 'same' or 'full' alignment or causally, as lfilter(taps, 1, x)
does; push(block) does the causal convolution block by block, carrying the
last K - 1 samples of every channel between calls in two buffers that swap
roles.  It owns every device buffer, so a push is the one launch of
dsp_fastconv_f32 on the current stream, with no allocation and no
synchronisation (graph-capturable).  Blocks whose lengths are multiples of
2 * hop give bitwise the one-shot result; any other cut the same values within
2e-6 * ||taps||_2 * max|x|.
"""
from __future__ import annotations

import numpy as np
import torch

from . import design, ops

MODES = ("causal", "same", "full")


def mode_geometry(mode: str, n: int, K: int) -> tuple[int, int]:
    """(offset, n_out) of dsp_fastconv_f32 for np.convolve(x, taps, mode) on n
    samples; 'causal' is lfilter's: the first n samples of 'full'."""
    if mode == "causal":
        return 0, n
    if mode == "full":
        return 0, n + K - 1
    if mode == "same":   # max(n, K) samples of 'full' from (min(n, K) - 1) // 2 on
        return (min(n, K) - 1) // 2, max(n, K)
    raise ValueError(f"mode must be one of {MODES}, got {mode!r}")


class _ConvStream:
    """What FastConv and PartConv share: the batch, the device and the output
    buffer, the one-shot call and the push skeleton.  A subclass's __init__ sets
    plan and K, calls _setup, builds _tables and _hist ([2, B, >= history
    length], two buffers that swap roles), then calls reset(); it supplies
    _oneshot(x, offset, n_out) and _run(block, n, hist_in, hist_out)."""

    def _setup(self, batch, max_block, device) -> torch.device:
        self.B = int(batch)
        self.max_block = int(max_block)
        if self.B < 1 or self.max_block < 1:
            raise ValueError("batch and max_block must be >= 1")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._ldy = max(4, -(-self.max_block // 4) * 4)
        self._y = torch.empty((self.B, self._ldy), dtype=torch.float32, device=self.device)
        return self.device

    @property
    def latency(self) -> float:
        return (self.K - 1) / 2

    def __call__(self, x: torch.Tensor, mode: str = "causal") -> torch.Tensor:
        x = self._check(x, None)
        if x.shape[1] < 1:
            raise ValueError("a one-shot convolution needs at least one sample")
        offset, n_out = mode_geometry(mode, int(x.shape[1]), self.K)
        return self._oneshot(x, offset, n_out)

    def reset(self) -> None:
        """Back to the start of a stream: zero history (at position 0 nothing
        else of the state is read)."""
        self._hist[0].zero_()
        self._cur = 0
        self.samples = 0

    def push(self, block: torch.Tensor) -> torch.Tensor:
        block = self._check(block, self.max_block)
        n = int(block.shape[1])
        y = self._run(block, n, self._hist[self._cur], self._hist[1 - self._cur])
        self._cur = 1 - self._cur
        self.samples += n
        return y

    def _check(self, x, limit):
        if (not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2
                or x.shape[0] != self.B or (limit is not None and x.shape[1] > limit)):
            what = f"{x.dtype} {tuple(x.shape)}" if torch.is_tensor(x) else type(x).__name__
            lim = "n" if limit is None else f"n <= {limit}"
            raise ValueError(f"expected float32 CUDA [{self.B}, {lim}], got {what}")
        return ops._rows(x, "x")


class FastConv(_ConvStream):
    """y = taps * x for `batch` float32 CUDA rows.

    __call__(x, mode) takes [batch, n >= 1] (any n) and returns a new tensor:
    'causal' [batch, n], 'same' [batch, max(n, K)], 'full' [batch, n + K - 1];
    it neither reads nor changes the stream state.  push(block) takes [batch,
    n], 0 <= n <= max_block (any view with unit column stride), and returns
    the next n causal outputs of the stream: a view of a buffer this object
    owns, valid until the next push.  `latency` is the delay of a linear-phase
    filter in samples, (K - 1) / 2.  log2n (default: dsp_fastconv_log2n's
    choice) sets the transform size n_fft = 2^log2n >= 2 (K - 1); `hop` =
    n_fft - (K - 1) outputs come from each block."""

    def __init__(self, taps, batch: int = 1, max_block: int = 4096, log2n: int | None = None,
                 device: torch.device | str = "cuda"):
        ops.require_gpu()
        self.plan = design.fastconv_plan(taps, log2n)
        self.K, self.n_fft, self.hop = self.plan.K, self.plan.n_fft, self.plan.hop
        dev = self._setup(batch, max_block, device)
        self._tables = ops.fastconv_tables(self.plan, dev)
        self._ldh = max(4, -(-(self.K - 1) // 4) * 4)   # every row starts 16-byte aligned
        self._hist = torch.zeros((2, self.B, self._ldh), dtype=torch.float32, device=dev)
        self.reset()

    def _oneshot(self, x, offset, n_out):
        return ops.fastconv(x, self.plan, offset, n_out, tables=self._tables)

    def _run(self, block, n, hist_in, hist_out):
        return ops.fastconv(block, self.plan, 0, n, hist_in, hist_out, out=self._y,
                            tables=self._tables)

    def state_dict(self) -> dict:
        """The history and the sample count (host copies); a FastConv of the
        same taps and batch continues bitwise after load_state_dict.
        Synchronises the stream."""
        return {"hist": self._hist[self._cur, :, :self.K - 1].cpu(), "samples": self.samples}

    def load_state_dict(self, sd: dict) -> None:
        hist = sd["hist"]
        if tuple(hist.shape) != (self.B, self.K - 1):
            raise ValueError(f"state_dict is of another tap count or batch size: hist "
                             f"{tuple(hist.shape)}")
        self.reset()
        self._hist[0, :, :self.K - 1].copy_(hist)
        self.samples = int(sd["samples"])


def convolve(x: torch.Tensor, taps, mode: str = "same") -> torch.Tensor:
    """np.convolve(x[b], taps, mode) for every row of float32 CUDA x [B, n >= 1]
    with 1 <= len(taps) <= 8193 ('causal': the first n samples of 'full')."""
    plan = design.fastconv_plan(np.asarray(taps))
    offset, n_out = mode_geometry(mode, int(x.shape[1]), plan.K)
    return ops.fastconv(x, plan, offset, n_out)
