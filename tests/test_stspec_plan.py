"""The stream spectrum without a GPU (include/dspcore_stspec.h): the framing of
a stream cut into blocks against design.stft_plan, the library's geometry
against the Python plan, and the argument checks of dsp_stspec_mag_f32, which
come before any device work."""
import ctypes
import re

import numpy as np
import pytest

from dspcore import _lib, design

EINVAL, ENOTSUP = _lib.DSP_EINVAL, _lib.DSP_ENOTSUP


def _hops(N):
    return sorted({h for h in (1, N // 4, N // 4 + 1, N - 1, N) if 1 <= h <= N})


def _partitions(N, hop):
    """Ragged partitions with blocks of 0, 1, hop - 1, N - 1, N, N + 1 and
    3 N + 5 samples, in several orders, plus the empty and the 1-sample stream."""
    sizes = [0, 1, max(hop - 1, 0), N - 1, N, N + 1, 3 * N + 5]
    parts = [[], [0], [1], [0, 0, 1, 0], sizes, sizes[::-1], [3 * N + 5, 0, 1, 1, N - 1],
             [N], [N, hop], [N - 1, 1], [N + 1] * 3, [hop] * 9, [1] * min(2 * N + 3, 70)]
    rng = np.random.default_rng(N * 131 + hop)
    for _ in range(6):
        parts.append([int(sizes[i]) for i in rng.integers(0, len(sizes), rng.integers(1, 9))])
    return parts


def _lib_geometry(lg, hop, seen, n, flush):
    c, f, o = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = _lib.load().dsp_stspec_geometry(lg, hop, seen, n, int(flush), ctypes.byref(c),
                                         ctypes.byref(f), ctypes.byref(o))
    return rc, (c.value, f.value, o.value)


def _walk(N, hop, blocks, step):
    """Runs step(seen, n, flush) -> (carry_len, frames, carry_out_len) over a
    partition and checks the framing rules; returns the number of calls."""
    seen = frames = 0
    carry = 0
    for n in blocks:
        cl, fr, col = step(seen, n, False)
        assert cl == carry and 0 <= cl < N and 0 <= col < N, (N, hop, blocks, seen, n)
        assert 0 <= fr <= 1 + (n - 1) // hop, (N, hop, blocks, seen, n, fr)
        assert cl + n == fr * hop + col
        seen += n
        frames += fr
        carry = col
        assert carry == seen - frames * hop                   # where the next frame starts
    cl, fr, col = step(seen, 0, True)
    assert cl == carry and fr in (0, 1) and col == 0
    plan = design.stft_plan(seen, N, hop)
    assert frames + fr == plan.frames, (N, hop, blocks, frames, fr, plan.frames)
    if seen == 0:
        assert fr == 1
    return len(blocks) + 1


@pytest.mark.parametrize("N", [2, 32, 4096])
def test_framing_arithmetic_is_stft_plans(N):
    for hop in _hops(N):
        for blocks in _partitions(N, hop):
            def step(seen, n, flush, hop=hop):
                p = design.stream_stft_plan(N, hop, seen, n, flush)
                return p.carry_len, p.frames, p.carry_out_len
            _walk(N, hop, blocks, step)
    # the default hop is stft_plan's (it divides 4 N: no frame is left to the flush)
    assert design.stream_stft_plan(N, None, 0, 5 * N).frames == design.stft_plan(5 * N, N).frames
    assert design.stream_stft_plan(N, None, 5 * N, 0) == \
        design.stream_stft_plan(N, max(1, N // 4), 5 * N, 0)


def test_plan_rejects_bad_arguments():
    for bad in (dict(n_fft=48), dict(n_fft=0), dict(hop=0), dict(hop=65), dict(seen=-1),
                dict(n_block=-1), dict(n_block=1, flush=True)):
        kw = dict(n_fft=64, hop=16, seen=0, n_block=0, flush=False)
        kw.update(bad)
        with pytest.raises(ValueError):
            design.stream_stft_plan(**kw)


@pytest.mark.parametrize("N", [2, 32, 4096])
def test_library_geometry_agrees_with_the_plan(N):
    lg = N.bit_length() - 1
    calls = 0
    for hop in _hops(N):
        for blocks in _partitions(N, hop):
            def step(seen, n, flush, hop=hop):
                rc, got = _lib_geometry(lg, hop, seen, n, flush)
                p = design.stream_stft_plan(N, hop, seen, n, flush)
                assert rc == 0 and got == (p.carry_len, p.frames, p.carry_out_len)
                return got
            calls += _walk(N, hop, blocks, step)
    assert calls > 100
    lib = _lib.load()
    assert lib.dsp_stspec_geometry(lg, 1, 7, 3, 0, None, None, None) == 0      # NULL outputs
    for args in ((lg, 0, 0, 0, 0), (lg, N + 1, 0, 0, 0), (lg, 1, -1, 0, 0), (lg, 1, 0, -1, 0),
                 (lg, 1, 0, 1, 1), (lg, 1, 0, (1 << 30) + 1, 0), (-1, 1, 0, 0, 0),
                 (31, 1, 0, 0, 0)):
        assert lib.dsp_stspec_geometry(*args, None, None, None) == EINVAL, args
        assert _lib.last_error()


def _mag(carry_in=0x1000, carry_out=0x2000, ld_carry=None, block=0x3000, ld_block=None,
         n_block=64, mag=0x4000, ld_mag=None, B=3, log2n=6, hop=16, seen=100, flush=0,
         window=0x5000, tw=0x6000):
    """dsp_stspec_mag_f32 with dummy pointers that no check dereferences."""
    N = 1 << max(log2n, 0)
    return _lib.load().dsp_stspec_mag_f32(
        carry_in, carry_out, N - 1 if ld_carry is None else ld_carry, block,
        n_block if ld_block is None else ld_block, n_block, mag,
        N // 2 + 1 if ld_mag is None else ld_mag, B, log2n, hop, seen, flush, window, tw, None)


def test_status_codes_before_any_device_work():
    N = 64
    einval = [dict(hop=0), dict(hop=-3), dict(hop=N + 1), dict(n_block=-1), dict(seen=-1),
              dict(B=-1), dict(ld_carry=N - 2), dict(ld_mag=N // 2), dict(carry_out=0x1000),
              dict(flush=1, n_block=1), dict(n_block=(1 << 30) + 1), dict(ld_block=63)]
    for kw in einval:
        assert _mag(**kw) == EINVAL, kw
        assert _lib.last_error(), kw
    for lg in (4, 15, 0, -1, 31):
        assert _mag(log2n=lg) == ENOTSUP, lg
        # ... also with every pointer null, and whatever else is wrong
        assert _mag(log2n=lg, carry_in=None, carry_out=None, block=None, mag=None, window=None,
                    tw=None, hop=0) == ENOTSUP
    # null pointers where one is read or written (still no device work)
    for name in ("carry_in", "carry_out", "block", "mag", "window", "tw"):
        assert _mag(**{name: None}) == EINVAL, name
    # every check precedes B == 0, which launches nothing
    assert _mag(B=0, carry_in=None, carry_out=None, block=None, mag=None, window=None,
                tw=None) == 0
    assert _mag(B=0, hop=0) == EINVAL
    # the limits themselves pass the checks (B == 0: nothing launched)
    assert _mag(B=0, hop=N, ld_carry=N - 1, ld_mag=N // 2 + 1, n_block=1 << 30) == 0
    assert _mag(B=0, hop=1, n_block=0, flush=1) == 0
    for lg in (5, 14):
        assert _mag(B=0, log2n=lg) == 0


def test_version_exports_and_signatures():
    lib = _lib.load()
    assert lib.dsp_stspec_version() == 10000
    with open(_lib.STSPEC_HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"^int (dsp_stspec_[a-z0-9_]+)\(", text, flags=re.M))
    assert declared == {"dsp_stspec_version", "dsp_stspec_geometry", "dsp_stspec_mag_f32"}
    for name in declared:
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES, f"{name} has no ctypes signature"
    # the other headers keep their symbols and versions
    assert len(_lib.header_symbols()) == 35
    assert (lib.dsp_version(), lib.dsp_stream_version(), lib.dsp_eqbank_version(),
            lib.dsp_eqlive_version()) == (20700, 10000, 10000, 10000)
