"""Streaming, host side (include/dspcore_stream.h): the block geometry of the
SRC stream against the oracle, the host entry point against the Python plan,
argument checks that answer without a GPU, and the pins on the one-shot
header that are why the streaming ABI lives in a header of its own."""
import ctypes
import re

import numpy as np
import pytest

from dspcore import _lib, design

N = 2000
PARTITIONS = [
    [N],
    [1] * 40 + [N - 40],
    [480] * 4 + [80],
    [37, 3, 500, 1, 959, 500],
]
# (L, M, num_taps)
RATIOS = [(3, 2, None), (2, 1, None), (1, 2, None), (8, 7, None), (7, 8, None), (1, 8, None),
          (8, 1, None), (5, 7, None), (160, 147, 1023)]


def src_model(x, n_out, taps, L, M, c_offset):
    """float64 model of dsp_src_polyphase_f32's contract (include/dspcore.h):
    j = m M + c, phi = j mod L, q = j div L,
    y[m] = sum_{t >= 0, phi + L t < K} taps[phi + L t] x[q - t], x zero outside
    [0, n_in)."""
    K = taps.size
    y = np.zeros(n_out)
    for m in range(n_out):
        j = m * M + c_offset
        phi, q = j % L, j // L
        t = np.arange(0, (K - 1 - phi) // L + 1)
        at = q - t
        ok = (at >= 0) & (at < x.size)
        y[m] = np.dot(taps[phi + L * t[ok]], x[at[ok]])
    return y


def stream_blocks(plan, x, parts):
    """Drives the model block by block as a StreamChain drives the kernel:
    staging row [hist | block], plan.block per block, plan.flush at the end.
    Returns (y, the (hist, c_offset, n_out) triples, the per-call counters)."""
    staging = np.zeros(plan.hist)
    consumed = produced = 0
    out, triples, counters = [], [], []
    at = 0
    for n in parts:
        block = x[at:at + n]
        at += n
        counters.append((consumed, produced, n, 0))
        hist, c_off, n_out = plan.block(consumed, produced, n)
        triples.append((hist, c_off, n_out))
        row = np.concatenate([staging, block])
        assert row.size == hist + n
        out.append(src_model(row, n_out, plan.taps, plan.L, plan.M, c_off))
        staging = row[row.size - hist:] if hist else row[:0]
        consumed += n
        produced += n_out
    counters.append((consumed, produced, 0, 1))
    hist, c_off, n_out = plan.flush(consumed, produced)
    triples.append((hist, c_off, n_out))
    out.append(src_model(staging, n_out, plan.taps, plan.L, plan.M, c_off))
    return np.concatenate(out), triples, counters


@pytest.fixture(scope="module")
def signal():
    return np.random.default_rng(7).uniform(-1, 1, N)


@pytest.fixture(scope="module")
def oracle_y(signal):
    from oracle import dsp_ref_cpu as orc
    return {(L, M, K): orc.resample(signal, 48000, M, L, K)[0] for L, M, K in RATIOS}


@pytest.mark.parametrize("L,M,K", RATIOS)
def test_block_geometry_matches_the_oracle(signal, oracle_y, L, M, K):
    plan = design.stream_src_plan(48000, M, L, K)
    assert plan.K % 2 == 1 and plan.c == (plan.K - 1) // 2
    assert plan.hist == -(-plan.K // L) - 1
    assert plan.fs_out == int(48000 * L / M)
    assert N * L >= plan.K          # the case where the stream equals the one-shot call
    ref = oracle_y[(L, M, K)]
    assert ref.size == -(-N * L // M)
    for parts in PARTITIONS:
        assert sum(parts) == N
        y, triples, _ = stream_blocks(plan, signal, parts)
        assert y.size == -(-N * L // M)
        assert all(h == plan.hist and c >= 0 and n >= 0 for h, c, n in triples)
        err = float(np.max(np.abs(y - ref)))
        print(f"L/M={L}/{M} parts={len(parts)} max err {err:.3g}")
        assert err <= 1e-10


def test_plan_counts_and_errors():
    plan = design.stream_src_plan(48000, 2, 3)
    assert (plan.K, plan.c, plan.hist, plan.fs_out) == (121, 60, 40, 72000)
    assert plan.ready(0) == 0 and plan.ready(20) == 0 and plan.ready(21) == 2
    assert plan.block(0, 0, 20) == (40, 60 + 40 * 3, 0)       # nothing computable yet
    with pytest.raises(ValueError):
        plan.block(21, 0, 5)                                   # produced lags consumed
    with pytest.raises(ValueError):
        plan.block(0, 0, -1)
    with pytest.raises(ValueError):
        design.stream_src_plan(48000, 0, 3)
    with pytest.raises(RuntimeError):
        design.stream_src_plan(48000, 1, 1, 2 * 4097 + 1)     # hist 8194 > 4096
    # a stream shorter than the filter: ceil(N L / M) outputs centred at (K - 1) / 2
    assert plan.flush(10, 0) == (40, 60 + 30 * 3, 15)


def _geometry(lib, K, L, M, consumed, produced, n_block, flush):
    out = [ctypes.c_int64(-7) for _ in range(3)]
    rc = lib.dsp_stream_src_geometry(K, L, M, consumed, produced, n_block, flush,
                                     *[ctypes.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


def _counts_only(plan, parts):
    """stream_blocks without the arithmetic: (triples, counters)."""
    consumed = produced = 0
    triples, counters = [], []
    for n in parts:
        counters.append((consumed, produced, n, 0))
        t = plan.block(consumed, produced, n)
        triples.append(t)
        consumed += n
        produced += t[2]
    counters.append((consumed, produced, 0, 1))
    triples.append(plan.flush(consumed, produced))
    return triples, counters


def test_host_geometry_agrees_with_the_plan():
    lib = _lib.load()
    for L, M, K in RATIOS:
        plan = design.stream_src_plan(48000, M, L, K)
        for parts in PARTITIONS:
            triples, counters = _counts_only(plan, parts)
            for want, (consumed, produced, n, flush) in zip(triples, counters):
                rc, got = _geometry(lib, plan.K, L, M, consumed, produced, n, flush)
                assert rc == 0, _lib.last_error()
                assert got == want, (L, M, consumed, produced, n, flush)


def test_stream_version_and_exports():
    lib = _lib.load()
    assert lib.dsp_stream_version() == 10000
    with open(_lib.STREAM_HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"^int (dsp_stream_[a-z0-9_]+)\(", text, flags=re.M))
    assert declared == {"dsp_stream_version", "dsp_stream_cascade_f32", "dsp_stream_src_geometry",
                        "dsp_stream_roll_f32"}
    # every dsp_* name the header mentions, comments included, is an exported
    # symbol with a signature (it refers to dspcore.h's by name)
    for name in _lib.header_symbols(_lib.STREAM_HEADER_PATH):
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES, f"{name} has no ctypes signature"


def test_one_shot_header_is_unchanged():
    """tests/test_abi.py pins include/dspcore.h to 35 names and ABI 2.7.0; the
    streaming entry points must not move either."""
    names = _lib.header_symbols()
    assert len(names) == 35
    assert not [n for n in names if n.startswith("dsp_stream")]
    assert _lib.load().dsp_version() == 20700
    with open(_lib.HEADER_PATH) as f:
        assert "dsp_stream" not in f.read()


def test_bad_arguments_answer_without_a_gpu():
    lib = _lib.load()
    sos = (ctypes.c_double * 45)(*([1, 0, 0, 0, 0] * 9))

    def cascade(x, y, B, n, ld_x, ld_y, S, ld_state):
        return lib.dsp_stream_cascade_f32(x, y, B, n, ld_x, ld_y, sos, S, 1, None, None, ld_state,
                                          None)

    assert cascade(64, 64, 1, 100, 100, 100, 6, 11) == _lib.DSP_EINVAL       # ld_state < 2S
    assert "ld_state" in _lib.last_error()
    assert cascade(64, 64, 1, 100, 100, 100, 9, 18) == _lib.DSP_ENOTSUP      # S = 9
    assert cascade(64, 64, -1, 100, 100, 100, 6, 12) == _lib.DSP_EINVAL      # negative sizes
    assert cascade(64, 64, 1, -5, 100, 100, 6, 12) == _lib.DSP_EINVAL
    assert cascade(64, 64, 1, 100, 99, 100, 6, 12) == _lib.DSP_EINVAL        # pitch < n
    assert cascade(None, 64, 1, 100, 100, 100, 6, 12) == _lib.DSP_EINVAL     # null x, n > 0
    assert "null" in _lib.last_error()
    # no-ops launch nothing: null pointers are fine
    assert cascade(None, None, 0, 100, 100, 100, 6, 12) == 0
    assert cascade(None, None, 4, 0, 0, 0, 6, 12) == 0
    # geometry: hist > 4096, even K, a flush with input, produced out of step
    assert _geometry(lib, 4099, 1, 1, 0, 0, 10, 0)[0] == _lib.DSP_ENOTSUP
    assert _geometry(lib, 4097, 1, 1, 0, 0, 10, 0)[0] == 0                   # hist 4096
    assert _geometry(lib, 120, 3, 2, 0, 0, 10, 0)[0] == _lib.DSP_EINVAL
    assert _geometry(lib, 121, 0, 2, 0, 0, 10, 0)[0] == _lib.DSP_EINVAL
    assert _geometry(lib, 121, 3, 2, 0, 0, -1, 0)[0] == _lib.DSP_EINVAL
    assert _geometry(lib, 121, 3, 2, 100, 160, 5, 1)[0] == _lib.DSP_EINVAL
    assert _geometry(lib, 121, 3, 2, 100, 7, 5, 0)[0] == _lib.DSP_EINVAL
    assert lib.dsp_stream_src_geometry(121, 3, 2, 0, 0, 5, 0, None, None, None) == _lib.DSP_EINVAL
    # roll
    assert lib.dsp_stream_roll_f32(64, 4, 100, 4097, 3, None) == _lib.DSP_ENOTSUP
    assert lib.dsp_stream_roll_f32(64, 4, 100, 60, 41, None) == _lib.DSP_EINVAL   # pitch
    assert lib.dsp_stream_roll_f32(64, -1, 100, 40, 3, None) == _lib.DSP_EINVAL
    assert lib.dsp_stream_roll_f32(None, 4, 100, 40, 3, None) == _lib.DSP_EINVAL
    assert lib.dsp_stream_roll_f32(None, 0, 100, 40, 3, None) == 0
    assert lib.dsp_stream_roll_f32(None, 4, 100, 0, 3, None) == 0
