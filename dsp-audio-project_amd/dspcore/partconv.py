"""Partitioned fast convolution: FIRs of up to 2^20 taps (a room response) by
uniformly partitioned overlap-save on the in-LDS FFT
(include/dspcore_partconv.h), one-shot and as a stream.

A PartConv holds one set of taps for `batch` channels, cut into S partitions of
P = n_fft / 2.  Called with a whole signal it convolves it in np.convolve's
'same' or 'full' alignment or causally, as lfilter(taps, 1, x) does;
push(block) does the causal convolution block by block.  Between pushes it
carries, per channel, the spectra of the last input blocks in a ring (each
block is transformed once) and the last `hist_len` time-domain samples in two
buffers that swap roles.  It owns every device buffer, so a push is the two
launches of dsp_partconv_f32 on the current stream, with no allocation and no
synchronisation (graph-capturable; the stream position is a host value, so a
captured push replays from the state it was captured at).  The framing is
anchored at absolute stream positions: blocks whose lengths are multiples of
`hop` give bitwise the one-shot result, any other cut the same values within
2e-6 * ||taps||_2 * max|x|.
"""
from __future__ import annotations

import torch

from . import design, ops
from .fastconv import MODES, _ConvStream, mode_geometry

__all__ = ["PartConv", "MODES", "mode_geometry"]


class PartConv(_ConvStream):
    """y = taps * x for `batch` float32 CUDA rows.

    __call__(x, mode) takes [batch, n >= 1] (any n) and returns a new tensor:
    'causal' [batch, n], 'same' [batch, max(n, K)], 'full' [batch, n + K - 1];
    it neither reads nor changes the stream state.  push(block) takes [batch,
    n], 0 <= n <= max_block (any view with unit column stride), and returns
    the next n causal outputs of the stream: a view of a buffer this object
    owns, valid until the next push.  `latency` is the delay of a linear-phase
    filter in samples, (K - 1) / 2.  log2n (default: dsp_partconv_log2n's
    choice) sets the transform size n_fft = 2^log2n; the taps are S = ceil(K /
    P) partitions of P = `hop` = n_fft / 2."""

    def __init__(self, taps, batch: int = 1, max_block: int = 4096, log2n: int | None = None,
                 device: torch.device | str = "cuda"):
        ops.require_gpu()
        self.plan = design.partconv_plan(taps, log2n)
        self.K, self.n_fft, self.hop, self.S = self.plan.K, self.plan.n_fft, self.plan.P, self.plan.S
        dev = self._setup(batch, max_block, device)
        self._tables = ops.partconv_tables(self.plan, dev)
        self._L = self.plan.hist_len                    # a multiple of 4: rows stay 16-byte aligned
        self._hist = torch.zeros((2, self.B, self._L), dtype=torch.float32, device=dev)
        self.slots = ops.partconv_slots(self.plan, self.max_block)
        self._ws = ops.partconv_workspace(self.plan, self.B, self.slots, dev)
        self.reset()

    def _oneshot(self, x, offset, n_out):
        return ops.partconv(x, self.plan, offset, n_out, tables=self._tables)

    def _run(self, block, n, hist_in, hist_out):
        return ops.partconv(block, self.plan, 0, n, self.samples, hist_in, hist_out, self._ws,
                            self.slots, out=self._y, tables=self._tables)

    def state_dict(self) -> dict:
        """The time-domain history and the sample count (host copies); a
        PartConv of the same taps, batch and log2n continues bitwise after
        load_state_dict.  Synchronises the stream."""
        return {"hist": self._hist[self._cur].cpu(), "samples": self.samples}

    def load_state_dict(self, sd: dict) -> None:
        """Takes the history and recomputes the ring's spectra from it (one
        forward launch)."""
        hist = sd["hist"]
        if tuple(hist.shape) != (self.B, self._L):
            raise ValueError(f"state_dict is of another tap count, size or batch: hist "
                             f"{tuple(hist.shape)}")
        self.reset()
        self._hist[0].copy_(hist)
        self.samples = int(sd["samples"])
        ops.partconv_prime(self._hist[0], self.plan, self.samples, self._ws, self.slots)
