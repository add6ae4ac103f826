"""dspcore — MI355X-native hot path of Renatovela-ctrl/dsp-audio-project.

Layers (bottom-up):
  libdspcore.so   hand-written gfx950 HIP kernels behind a C-ABI (include/dspcore.h)
  _lib            ctypes binding of that ABI
  design          host-side float64 filter design / call planning (reference rules)
  ops             per-kernel device operators on torch CUDA tensors
  chain           batched SRC -> EQ -> spectrum plan (the benchmarked path)
  stream          SRC -> EQ block by block, history and filter state carried
                  (include/dspcore_stream.h)
  eqbank          per-channel EQ: one gain set per row, one launch
                  (include/dspcore_eqbank.h)
  eqlive          live EQ: gains that change between two blocks without a click
                  (include/dspcore_eqlive.h)
  stspec          stream spectrum: a running spectrogram of a stream, frame by frame
                  (include/dspcore_stspec.h)
  fastconv        fast convolution: long FIRs by overlap-save on the in-LDS FFT,
                  one-shot and as a stream (include/dspcore_fastconv.h)
  partconv        partitioned fast convolution: FIRs of up to 2^20 taps, one-shot
                  and as a stream (include/dspcore_partconv.h)
  shard           one host thread per GPU over contiguous channel ranges
  host            numpy batches through the chain with PCIe copies overlapped
The reference-compatible drop-in is dsp-audio-project_amd/modules/dsp_core.py.
"""
from . import design  # noqa: F401

__all__ = ["design", "ops", "chain", "stream", "eqbank", "eqlive", "stspec", "fastconv",
           "partconv", "shard", "host"]
__version__ = "1.8.0"


def __getattr__(name):  # lazy: importing design must not require the GPU library
    if name in ("ops", "chain", "stream", "eqbank", "eqlive", "stspec", "fastconv", "partconv",
                "shard", "host", "_lib"):
        import importlib
        return importlib.import_module(f".{name}", __name__)
    raise AttributeError(name)
