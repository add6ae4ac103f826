"""A running spectrogram of a stream, frame by frame (include/dspcore_stspec.h).

A StreamSpectrum carries, per channel, the samples from which the next STFT
frame starts, so that the frames of all its push() calls plus the flush() are
design.stft_plan's frames of the concatenated signal -- the recipe of
ops.stft_magnitude (window, FFT, |X[k]| for k <= n_fft/2), without keeping the
signal.  It owns every device buffer, so a push is two launches on the current
stream (`stspec`: the frames and the carry update; `stspec_nf`: the non-finite
repair), with no allocation and no synchronisation.  A frame's bits do not
depend on how the stream was cut into blocks.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, ops
from .chain import ROW_ALIGN


def _pitch(n: int) -> int:
    return max(ROW_ALIGN, -(-int(n) // ROW_ALIGN) * ROW_ALIGN)


class StreamSpectrum:
    """|FFT(window * frame)|[:n_fft/2 + 1] of every frame s[f hop, f hop + n_fft)
    of `batch` streams, as the samples arrive.

    push(block) takes float32 CUDA [batch, n], 0 <= n <= max_block (any view
    with unit column stride: rows may start at any 4-byte alignment), and
    returns the frames whose last sample has arrived, [batch, frames,
    n_fft/2 + 1]: a view of a buffer this object owns, valid until the next
    push / flush / reset.  frames is at most 1 + (n - 1) // hop and may be 0.
    flush() ends the stream with the zero-padded frame design.stft_plan still
    owes (0 or 1 frames; an empty stream gives one all-zero frame); after it
    only reset() (or load_state_dict) makes the object usable again.

    n_fft is a power of two, 32 .. 16384; 1 <= hop <= n_fft, default
    max(1, n_fft // 4).  `window` is float32 [n_fft] (array or tensor), default
    the reference's Hann window.  `samples` and `frames_emitted` count what the
    stream has taken and given so far."""

    def __init__(self, n_fft: int = 4096, hop: int | None = None, batch: int = 1,
                 max_block: int = 4096, device: torch.device | str = "cuda", window=None):
        ops.require_gpu()
        self.n_fft = int(n_fft)
        if self.n_fft < 1 or self.n_fft & (self.n_fft - 1):
            raise ValueError(f"n_fft={n_fft} is not a power of two")
        self.log2n = self.n_fft.bit_length() - 1
        if not _lib.DSP_STSPEC_MIN_LOG2N <= self.log2n <= _lib.DSP_MAX_LOG2N:
            raise ValueError(f"n_fft={n_fft} outside 2^{_lib.DSP_STSPEC_MIN_LOG2N} .. "
                             f"2^{_lib.DSP_MAX_LOG2N}")
        self.hop = max(1, self.n_fft // 4) if hop is None else int(hop)
        if self.hop < 1 or self.hop > self.n_fft:
            raise ValueError(f"hop={hop} outside [1, n_fft={self.n_fft}]")
        self.B = int(batch)
        self.max_block = int(max_block)
        if self.B < 1 or self.max_block < 1:
            raise ValueError("batch and max_block must be >= 1")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self.half = self.n_fft // 2 + 1
        if window is None:
            self.window = ops._table("hann", self.n_fft, dev)
        else:
            w = torch.as_tensor(np.asarray(window.cpu() if torch.is_tensor(window) else window,
                                           dtype=np.float32))
            if tuple(w.shape) != (self.n_fft,):
                raise ValueError(f"window must be [{self.n_fft}], got {tuple(w.shape)}")
            self.window = w.contiguous().to(dev)
        self._tw = ops._table("tw", self.n_fft, dev)
        self._ldc = -(-(self.n_fft - 1) // 4) * 4   # every row starts 16-byte aligned
        self._carry = torch.zeros((2, self.B, self._ldc), dtype=torch.float32, device=dev)
        self.max_frames = 1 + (self.max_block - 1) // self.hop
        self._ldm = _pitch(self.half)
        self._mag = torch.empty(self.B * self.max_frames * self._ldm, dtype=torch.float32,
                                device=dev)
        self.reset()

    # -- state -----------------------------------------------------------------
    def reset(self) -> None:
        """Back to the start of a stream."""
        self.samples = 0
        self.frames_emitted = 0
        self.flushed = False
        self._cur = 0          # which carry buffer holds the carry

    @property
    def carry_len(self) -> int:
        return 0 if self.flushed else self._geometry(0, False)[0]

    def state_dict(self) -> dict:
        """The carry and the counters (host copies); a StreamSpectrum of the
        same n_fft, hop and batch continues bitwise after load_state_dict.
        Synchronises the stream."""
        return {"carry": self._carry[self._cur, :, :self.carry_len].cpu(),
                "samples": self.samples, "frames_emitted": self.frames_emitted,
                "flushed": self.flushed}

    def load_state_dict(self, sd: dict) -> None:
        carry = sd["carry"]
        self.reset()
        self.samples = int(sd["samples"])
        self.frames_emitted = int(sd["frames_emitted"])
        self.flushed = bool(sd["flushed"])
        if tuple(carry.shape) != (self.B, self.carry_len):
            shape = tuple(carry.shape)
            self.reset()
            raise ValueError(f"state_dict is of another n_fft, hop or batch size: carry {shape}")
        if carry.shape[1]:
            self._carry[0, :, :carry.shape[1]].copy_(carry)

    # -- one call ----------------------------------------------------------------
    def _geometry(self, n_block: int, flush: bool) -> tuple[int, int, int]:
        """(carry_len, frames, carry_out_len) of the next call, from the library."""
        c, f, o = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        rc = _lib.load().dsp_stspec_geometry(self.log2n, self.hop, self.samples, int(n_block),
                                             int(flush), ctypes.byref(c), ctypes.byref(f),
                                             ctypes.byref(o))
        _lib.check(rc, "dsp_stspec_geometry")
        return c.value, f.value, o.value

    def _call(self, block: torch.Tensor | None, n: int, flush: bool) -> torch.Tensor:
        _, frames, _ = self._geometry(n, flush)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            rc = lib.dsp_stspec_mag_f32(
                self._carry[self._cur].data_ptr(), self._carry[1 - self._cur].data_ptr(),
                self._ldc, ops._ptr(block) if n else None, ops.ld(block) if n else 0, n,
                self._mag.data_ptr(), self._ldm, self.B, self.log2n, self.hop, self.samples,
                int(flush), self.window.data_ptr(), self._tw.data_ptr(),
                torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(rc, "dsp_stspec_mag_f32")
        self._cur = 1 - self._cur
        self.samples += n
        self.frames_emitted += frames
        rows = self._mag[:self.B * frames * self._ldm].view(self.B, frames, self._ldm)
        return rows[:, :, :self.half]

    def push(self, block: torch.Tensor) -> torch.Tensor:
        if self.flushed:
            raise RuntimeError("the stream was flushed; reset() starts a new one")
        if (not torch.is_tensor(block) or not block.is_cuda or block.dtype != torch.float32
                or block.dim() != 2 or block.shape[0] != self.B
                or block.shape[1] > self.max_block):
            what = (f"{block.dtype} {tuple(block.shape)}" if torch.is_tensor(block)
                    else type(block).__name__)
            raise ValueError(f"expected float32 CUDA [{self.B}, n <= {self.max_block}], got {what}")
        block = ops._rows(block, "block")
        return self._call(block, int(block.shape[1]), False)

    def flush(self) -> torch.Tensor:
        """Ends the stream: the zero-padded last frame, if stft_plan owes one."""
        if self.flushed:
            raise RuntimeError("the stream was flushed; reset() starts a new one")
        mag = self._call(None, 0, True)
        self.flushed = True
        return mag
