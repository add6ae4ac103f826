"""SRC -> EQ as a stream: blocks in, blocks out, for a live input or a signal
longer than device memory (include/dspcore_stream.h).

A StreamChain carries, per channel, the last `hist` input samples of the SRC
and the EQ cascade's float64 state from one push() to the next, so that the
concatenated outputs are the one-shot chain's (dspcore.chain.Chain) on the
concatenated input: y bitwise (the same SRC kernel sums every output in the
same order), z to float64 rounding before its float32 store.

It owns every device buffer, so a push is only launches on the current
stream -- the SRC kernel on the staging rows [history | block], the stateful
cascade (one launch, `iir_stream`), the history roll -- with no allocation
and no synchronisation.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, ops
from .chain import ROW_ALIGN
from .design import caller_taps, eq_plan, stream_src_plan
from .eqbank import EqBank
from .eqlive import LiveEq
from .stspec import StreamSpectrum


def _pitch(n: int) -> int:
    return max(ROW_ALIGN, -(-int(n) // ROW_ALIGN) * ROW_ALIGN)


class StreamChain:
    """conversion_tasa_muestreo(fs, M, L) then sistema_ecualizador(gains) over
    `batch` channels, block by block.

    push(x_block) takes float32 CUDA [batch, n], 0 <= n <= max_block, and
    returns (y, z): views [batch, n_out] of buffers this object owns, valid
    until the next push / flush / reset (y is None with keep_y=False; with
    L = M = 1, the reference's SRC bypass, y is the block itself).  n_out is
    design.StreamSrcPlan's count for the block and may be 0.  flush() ends the
    stream with the outputs whose windows reach past the last input; after it
    only reset() (or load_state_dict) makes the object usable again.

    The EQ state belongs to the cascade it was filtered with, so the gains of
    such a chain are fixed; live=True (below) is the mode whose gains may
    change mid-stream.  With every |gain| < 0.1 the reference bypasses the EQ
    and z is y (no clip, dsp_core.py:222-223).

    `gains` is one dict for every channel, or a sequence of `batch` dicts, one
    per channel: the cascade is then an EqBank (dspcore.eqbank, one launch,
    `iir_bank`, in place of `iir_stream`) with max_n = the longest block the
    SRC can produce, the state tensor is [batch, 2 * (the largest stage
    count)], and a channel whose own plan is the bypass gets z = y in its
    rows of the one z buffer.

    live=True: the cascade is a LiveEq (dspcore.eqlive, one launch,
    `iir_live`) with max_n = the longest block the SRC can produce.  The keys
    of `gains` (one dict or `batch` dicts) are its band slots, every band
    carries scipy's lfilter state, and set_gains(gains) changes the gains
    between two blocks without a click: the new ones hold from the next push /
    flush.  With live=False nothing differs from the above.

    spectrum=dict(n_fft=..., hop=...) adds a running spectrogram of z
    (dspcore.stspec.StreamSpectrum, two more launches per push: `stspec`,
    `stspec_nf`): push and flush then return (y, z, mag), mag [batch, frames,
    n_fft/2 + 1] the STFT frames of z that the block completed (flush: those of
    its last outputs, then the zero-padded frame design.stft_plan still owes),
    valid until the next call.  With spectrum=None nothing differs from the
    above."""

    def __init__(self, fs: int, L: int, M: int, num_taps: int | None, gains, batch: int,
                 max_block: int, device: torch.device | str = "cuda", keep_y: bool = True,
                 live: bool = False, spectrum: dict | None = None):
        ops.require_gpu()
        self.B = int(batch)
        self.max_block = int(max_block)
        if self.B < 1 or self.max_block < 1:
            raise ValueError("batch and max_block must be >= 1")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self.identity_src = int(L) == 1 and int(M) == 1
        self.keep_y = bool(keep_y)
        if self.identity_src:
            self.plan = None
            self.hist = 0
            self.fs_out = int(fs)
            self.latency_in = 0.0
            max_out = self.max_block
        else:
            self.plan = stream_src_plan(fs, M, L, num_taps)
            self.hist = self.plan.hist
            self.fs_out = self.plan.fs_out
            # output m reads inputs up to (m M + c) div L: c / L samples ahead of its own instant
            self.latency_in = self.plan.c / self.plan.L
            self.taps = torch.from_numpy(caller_taps(self.plan)).to(dev)
            p = self.plan
            max_out = max(-(-(self.max_block * p.L) // p.M) + 1, -(-(p.c + p.L) // p.M) + 1)
            # staging rows [history | block]; one more column so that a flush
            # with hist == 0 still hands the SRC kernel a (zero) sample
            self._ldx = _pitch(self.hist + self.max_block + 1)
            self._xs = torch.zeros((self.B, self._ldx), dtype=torch.float32, device=dev)
            self._ybuf = torch.empty((self.B, _pitch(max_out)), dtype=torch.float32, device=dev)
        # the spectrum of z: its longest block is the longest the SRC can produce
        self.spec = (None if spectrum is None else
                     StreamSpectrum(batch=self.B, max_block=max_out, device=dev, **spectrum))
        self.bank = self.live = None
        if live:
            self.eq = self.sos = None
            self.live = LiveEq(self.fs_out, gains, max_out, dev, batch=self.B)
            self._zbuf = torch.empty((self.B, _pitch(max_out)), dtype=torch.float32, device=dev)
            self._state = self.live._state      # the LiveEq carries it in place
            self.reset()
            return
        if not isinstance(gains, dict):
            # one gains dict per channel: the EQ bank (dspcore.eqbank), whose
            # chunking is fixed by the longest block the SRC can hand it
            self.eq = self.sos = None
            self.bank = EqBank(self.fs_out, gains, max_out, dev, batch=self.B)
            self._zbuf = torch.empty((self.B, _pitch(max_out)), dtype=torch.float32, device=dev)
            self._state = torch.zeros((self.B, max(2 * self.bank.max_stages, 2)),
                                      dtype=torch.float64, device=dev)
            self.reset()
            return
        self.eq = eq_plan(self.fs_out, gains)
        self.sos = np.ascontiguousarray(self.eq.sos, dtype=np.float64)
        S = self.sos.shape[0]
        if S > _lib.DSP_STREAM_MAX_STAGES:
            raise RuntimeError(f"the streaming cascade takes <= {_lib.DSP_STREAM_MAX_STAGES} "
                               f"stages (got {S})")
        self._zbuf = (None if self.eq.bypass else
                      torch.empty((self.B, _pitch(max_out)), dtype=torch.float32, device=dev))
        self._state = torch.zeros((self.B, max(2 * S, 2)), dtype=torch.float64, device=dev)
        self.reset()

    # -- state -----------------------------------------------------------------
    def reset(self) -> None:
        """Back to the start of a stream: zero history, EQ at rest."""
        self.consumed = 0
        self.produced = 0
        self.flushed = False
        if self.live is not None:
            self.live.reset()
        else:
            self._state.zero_()
        if not self.identity_src:
            self._xs.zero_()
        if self.spec is not None:
            self.spec.reset()

    def set_gains(self, gains) -> None:
        """Live chains only: new gains (one dict, or one per channel, with the
        band slots of the constructor's) from the next push / flush on."""
        if self.live is None:
            raise RuntimeError("set_gains needs a live chain: StreamChain(..., live=True)")
        self.live.set_gains(gains)

    def state_dict(self) -> dict:
        """History, EQ state and counters (host copies), for checkpointing; a
        StreamChain of the same plan continues bitwise after load_state_dict.
        Synchronises the stream."""
        hist = (torch.empty((self.B, 0), dtype=torch.float32) if self.identity_src
                else self._xs[:, :self.hist].cpu())
        sd = {"history": hist, "eq_state": self._state.cpu(), "consumed": self.consumed,
              "produced": self.produced, "flushed": self.flushed}
        if self.live is not None:
            sd["eq_active"] = self.live.state_dict()["ever_active"]
        if self.spec is not None:
            sd["spectrum"] = self.spec.state_dict()
        return sd

    def load_state_dict(self, sd: dict) -> None:
        hist, state = sd["history"], sd["eq_state"]
        if tuple(hist.shape) != (self.B, self.hist) or tuple(state.shape) != tuple(self._state.shape):
            raise ValueError("state_dict is of another plan or batch size")
        self.reset()
        if self.hist:
            self._xs[:, :self.hist].copy_(hist)
        if self.live is not None:
            self.live.load_state_dict({"zi": state, "ever_active": sd.get("eq_active")})
        else:
            self._state.copy_(state)
        self.consumed = int(sd["consumed"])
        self.produced = int(sd["produced"])
        self.flushed = bool(sd["flushed"])
        if self.spec is not None:
            if "spectrum" not in sd:
                raise ValueError("state_dict is of a chain without a spectrum")
            self.spec.load_state_dict(sd["spectrum"])

    # -- one block ---------------------------------------------------------------
    def _geometry(self, n_block: int, flush: bool) -> tuple[int, int]:
        """(c_offset, n_out) of the block's SRC call, from the library."""
        h, c, n = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        p = self.plan
        rc = _lib.load().dsp_stream_src_geometry(p.K, p.L, p.M, self.consumed, self.produced,
                                                 int(n_block), int(flush), ctypes.byref(h),
                                                 ctypes.byref(c), ctypes.byref(n))
        _lib.check(rc, "dsp_stream_src_geometry")
        return c.value, n.value

    def _eq(self, y: torch.Tensor) -> torch.Tensor:
        if self.live is not None:
            z = self._zbuf[:, :y.shape[1]]
            if y.shape[1]:
                self.live.apply(y, out=z)
            return z
        if self.bank is not None:
            z = self._zbuf[:, :y.shape[1]]
            if y.shape[1]:
                self.bank.apply(y, zi=self._state, out=z, zf=self._state)
            return z
        if self.eq.bypass:
            return y
        z = self._zbuf[:, :y.shape[1]]
        if y.shape[1]:
            ops.biquad_cascade_state(y, self.sos, True, zi=self._state, out=z, zf=self._state)
        return z

    def _src(self, n_in: int, c_offset: int, n_out: int) -> torch.Tensor:
        y = self._ybuf[:, :n_out]
        if n_out:
            p = self.plan
            lib = _lib.load()
            with torch.cuda.device(self.device):
                rc = lib.dsp_src_polyphase_f32(
                    self._xs.data_ptr(), y.data_ptr(), self.B, n_in, self._ldx, n_out,
                    self._ybuf.stride(0), self.taps.data_ptr(), p.K, p.L, p.M, c_offset,
                    torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(rc, "dsp_src_polyphase_f32")
        return y

    def _out(self, y: torch.Tensor, z: torch.Tensor, last: bool = False):
        """What push / flush return: (y, z), and the frames of z with a spectrum."""
        y = y if self.keep_y else None
        if self.spec is None:
            return y, z
        mag = self.spec.push(z)
        if last:   # the frames of the last outputs, then the frame the plan still owes
            mag = mag.clone()   # (the flush reuses the buffer that `mag` is a view of)
            mag = torch.cat([mag, self.spec.flush()], dim=1)
        return y, z, mag

    def push(self, x_block: torch.Tensor):
        if self.flushed:
            raise RuntimeError("the stream was flushed; reset() starts a new one")
        if (not x_block.is_cuda or x_block.dtype != torch.float32 or x_block.dim() != 2
                or x_block.shape[0] != self.B or x_block.shape[1] > self.max_block):
            raise ValueError(f"expected float32 CUDA [{self.B}, n <= {self.max_block}], got "
                             f"{x_block.dtype} {tuple(x_block.shape)}")
        n = int(x_block.shape[1])
        if self.identity_src:
            y = ops._rows(x_block, "x_block")
            z = self._eq(y)
            self.consumed += n
            self.produced += n
            return self._out(y, z)
        c_offset, n_out = self._geometry(n, False)
        self._xs[:, self.hist:self.hist + n].copy_(x_block)
        y = self._src(self.hist + n, c_offset, n_out)
        z = self._eq(y)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            rc = lib.dsp_stream_roll_f32(self._xs.data_ptr(), self.B, self._ldx, self.hist, n,
                                         torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(rc, "dsp_stream_roll_f32")
        self.consumed += n
        self.produced += n_out
        return self._out(y, z)

    def flush(self):
        """Ends the stream: the last ceil(consumed L / M) - produced outputs."""
        if self.flushed:
            raise RuntimeError("the stream was flushed; reset() starts a new one")
        self.flushed = True
        if self.identity_src:
            y = torch.empty((self.B, 0), dtype=torch.float32, device=self.device)
            return self._out(y, y, last=True)
        c_offset, n_out = self._geometry(0, True)
        n_in = self.hist
        if n_in == 0:   # K <= L: no history; the outputs left see zeros only
            self._xs[:, :1].zero_()
            n_in = 1
        y = self._src(n_in, c_offset, n_out)
        z = self._eq(y)
        self.produced += n_out
        return self._out(y, z, last=True)
