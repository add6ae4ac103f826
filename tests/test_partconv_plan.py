"""Partitioned fast convolution without a GPU (include/dspcore_partconv.h): the
default transform size, design.partconv_plan's tables, the numpy model of the
kernels (tests/partconv_model.py) against float64 np.convolve at the GPU test's
shapes, model stream cuts, and the argument checks of dsp_partconv_f32 and
dsp_partconv_prime_f32, which come before any device work."""
import re

import numpy as np
import pytest

import partconv_model as pm
from dspcore import _lib, design

EINVAL, ENOTSUP = _lib.DSP_EINVAL, _lib.DSP_ENOTSUP


def test_default_transform_size_and_queries():
    lib = _lib.load()
    want = {1: 6, 32: 6, 33: 7, 1024: 11, 1025: 12, 8192: 14, 8193: 14, 8194: 14, 65536: 14,
            1 << 20: 14}
    for K, lg in want.items():
        assert lib.dsp_partconv_log2n(K) == lg, K
        assert design.partconv_log2n(K) == lg, K
        assert lg == 14 or (1 << (lg - 1)) >= K                 # one partition holds the taps
        assert lg == 6 or (1 << (lg - 2)) < K                   # the smallest such size
    for K in (0, -5, (1 << 20) + 1):
        assert lib.dsp_partconv_log2n(K) == EINVAL and _lib.last_error()
        with pytest.raises(ValueError):
            design.partconv_log2n(K)
    # history length and ring size: the ABI and the plan agree
    for K, lg in ((1, 6), (32, 6), (33, 6), (2049, 6), (8194, 14), (1 << 20, 14), (1 << 20, 11)):
        N = 1 << lg
        V, H, S, L = pm.geometry(N, K)
        p = design.partconv_plan(np.ones(K), log2n=lg)
        assert (p.K, p.n_fft, p.P, p.hop, p.S, p.hist_len) == (K, N, H, H, S, L)
        assert lib.dsp_partconv_hist_len(K, lg) == L >= K - 1
        for n, off in ((0, 0), (1, 0), (H, 0), (H + 1, 0), (5 * H, K - 1)):
            assert lib.dsp_partconv_slots(K, lg, n, off) == S + -(-(n + off) // H) + 1
        assert lib.dsp_partconv_workspace_bytes(3, lg, 7) == 3 * 7 * (8 * N + 4)
    assert lib.dsp_partconv_hist_len(1 << 20, 10) == EINVAL         # 2048 partitions
    assert lib.dsp_partconv_hist_len(40, 5) == ENOTSUP
    assert lib.dsp_partconv_slots(40, 6, -1, 0) == EINVAL
    assert lib.dsp_partconv_slots(40, 6, 10, 40) == EINVAL
    assert lib.dsp_partconv_slots(40, 15, 10, 0) == ENOTSUP
    assert lib.dsp_partconv_workspace_bytes(-1, 6, 7) == 0 and _lib.last_error()
    with pytest.raises(ValueError):
        design.partconv_plan(np.ones(1 << 20), log2n=10)


@pytest.mark.parametrize("K,lg", [(1, 6), (32, 6), (33, 6), (157, 6), (2049, 6), (1021, 9),
                                  (8194, 14), (20000, None), (20000, 11)])
def test_plan_tables(K, lg):
    taps64 = np.random.default_rng(K).standard_normal(K) / 3
    p = design.partconv_plan(taps64, lg)
    lg = design.partconv_log2n(K) if lg is None else lg
    N = 1 << lg
    P = N // 2
    S = -(-K // P)
    assert (p.K, p.log2n, p.n_fft, p.N, p.P, p.S) == (K, lg, N, N, P, S)
    assert p.taps.dtype == np.float32 and p.hf.dtype == np.complex64 and p.hf.shape == (S, N)
    assert np.array_equal(p.taps, taps64.astype(np.float32))
    # the float64 FFT of each float32 partition (the last zero-padded), divided
    # by N, rounded once
    for s in range(S):
        part = np.zeros(P)
        seg = p.taps[s * P:(s + 1) * P].astype(np.float64)
        part[:seg.size] = seg
        want = np.fft.fft(part, N) / N
        assert np.array_equal(p.hf[s], want.astype(np.complex64)), s
    assert np.array_equal(p.hf, pm.hf_tables(p.taps, N))
    for bad in (5, 15):
        with pytest.raises(RuntimeError):
            design.partconv_plan(taps64[:1], log2n=bad)
    with pytest.raises(ValueError):
        design.partconv_plan(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        design.partconv_plan([])


@pytest.mark.parametrize("N", pm.SIZES)
def test_model_meets_the_bound_at_the_gpu_shapes(N):
    """The kernels' arithmetic in numpy against float64 np.convolve: every tap
    count, offset and row length of tests/test_gpu_partconv.py, both n_out."""
    lg = N.bit_length() - 1
    worst = 0.0
    for K in pm.tap_counts(N):
        taps = pm.make_taps(K)
        for n in pm.row_lengths(N):
            x = pm.make_rows(N, n)
            ref = pm.full_reference(x, taps)
            b = pm.bound(taps, x)
            for off in pm.offsets(K):
                n_full = n + K - 1 - off
                got = pm.model(x, taps, lg, off, n_full)
                err = float(np.max(np.abs(got - ref[:, off:off + n_full])))
                worst = max(worst, err / b)
                assert err <= b, (N, K, n, off, err / b)
                assert np.array_equal(pm.model(x, taps, lg, off, n), got[:, :n])
    print(f"N={N}: model worst error / bound {worst:.3f}")


def test_model_at_the_largest_size():
    N, K = 16384, 8194
    n = N + 5
    taps = pm.make_taps(K)
    x = pm.make_rows(N, n)
    ref = pm.full_reference(x, taps)
    for off in pm.offsets(K):
        got = pm.model(x, taps, 14, off, n)
        assert np.max(np.abs(got - ref[:, off:off + n])) <= pm.bound(taps, x), off


def test_model_stream_cuts():
    """Cuts at multiples of H are bitwise the one call (the same pairs form
    either way: a pair is complete when the call ends on its boundary); ragged
    cuts stay within the bound."""
    N = 64
    V, H = N // 4, N // 2
    for K in (H, 2 * H + 1, 5 * H - 3):
        taps = pm.make_taps(K)
        n = 9 * H + 11
        x = np.random.default_rng(5 + K).uniform(-1, 1, (3, n)).astype(np.float32)
        one = pm.model(x, taps, 6)
        ref = pm.full_reference(x, taps)[:, :n]
        for cuts, exact in (([2 * H, 4 * H, 3 * H + 11], True), ([H, H, 7 * H + 11], True),
                            ([1, V, 0, 3 * H + 5, H - 1, n - 4 * H - V - 5], False)):
            got = pm.model_stream(x, taps, 6, cuts)
            if exact:
                assert np.array_equal(got.view(np.uint32), one.view(np.uint32)), (K, cuts)
            assert np.max(np.abs(got - ref)) <= pm.bound(taps, x), (K, cuts)


# K = 40 taps at N = 64: H = 32, S = 2, hist_len = 2 * 32 + 48 = 112
_L, _SLOTS = 112, 7


def _conv(x=0x10000, y=0x80000, B=3, n_in=100, ld_x=None, n_out=None, ld_y=None, offset=0, pos=0,
          hist_in=0x100000, hist_out=0x180000, ld_hist=_L, taps=0x200000, K=40, hf=0x280000,
          log2n=6, ws=0x400000, ws_bytes=None, slots=_SLOTS, tw=0x300000):
    """dsp_partconv_f32 with dummy pointers that no check dereferences."""
    n_out = n_in if n_out is None else n_out
    if ws_bytes is None:
        ws_bytes = max(B, 0) * max(slots, 0) * ((8 << min(max(log2n, 0), 14)) + 4)
    return _lib.load().dsp_partconv_f32(
        x, y, B, n_in, n_in if ld_x is None else ld_x, n_out, n_out if ld_y is None else ld_y,
        offset, pos, hist_in, hist_out, ld_hist, taps, K, hf, log2n, ws, ws_bytes, slots, tw, None)


def _prime(hist=0x100000, B=3, ld_hist=_L, pos=100, K=40, log2n=6, ws=0x400000, ws_bytes=None,
           slots=_SLOTS, tw=0x300000):
    if ws_bytes is None:
        ws_bytes = max(B, 0) * max(slots, 0) * ((8 << min(max(log2n, 0), 14)) + 4)
    return _lib.load().dsp_partconv_prime_f32(hist, B, ld_hist, pos, K, log2n, ws, ws_bytes,
                                              slots, tw, None)


def test_status_codes_before_any_device_work():
    lib = _lib.load()
    assert lib.dsp_partconv_hist_len(40, 6) == _L
    assert lib.dsp_partconv_slots(40, 6, 100, 0) == _SLOTS
    einval = [dict(K=0), dict(K=-1), dict(K=(1 << 20) + 1), dict(K=32 * 1024 + 1, ld_hist=1 << 21),
              dict(B=-1), dict(n_in=-1), dict(n_out=-1), dict(offset=-1), dict(offset=40),
              dict(pos=-1), dict(pos=(1 << 40) + 1), dict(n_out=100 + 39 + 1),
              dict(n_out=100 + 39 - 3 + 1, offset=3), dict(ld_x=99), dict(ld_y=99),
              dict(ld_hist=_L - 1), dict(ld_hist=_L - 1, hist_in=None),
              dict(ld_hist=_L - 1, hist_out=None), dict(hist_out=0x100000),
              dict(pos=64, hist_in=None), dict(slots=0), dict(slots=-1),
              dict(slots=3),                      # 4 pairs carry 100 outputs
              dict(pos=64, slots=4),              # ... and one more is read behind them
              dict(ws_bytes=3 * _SLOTS * (512 + 4) - 1), dict(ws=0x400008), dict(hf=0x280004),
              dict(tw=0x300004)]
    for kw in einval:
        assert _conv(**kw) == EINVAL, kw
        assert _lib.last_error(), kw
    for lg in (5, 15, 0, -1, 31):
        assert _conv(log2n=lg) == ENOTSUP, lg
        assert _lib.last_error()
        # ... also with every pointer null, and whatever else is wrong
        assert _conv(log2n=lg, x=None, y=None, hist_in=None, hist_out=None, taps=None, hf=None,
                     ws=None, tw=None, K=0) == ENOTSUP
        assert _prime(log2n=lg, hist=None) == ENOTSUP
    # null pointers where one is read or written (still no device work); a null
    # hist_in at pos = 0 is the start of a stream and a null hist_out is not
    # written
    for name in ("x", "y", "taps", "hf", "tw", "ws"):
        assert _conv(**{name: None}) == EINVAL, name
        assert _lib.last_error(), name
    # x and y must not overlap
    assert _conv(y=0x10000 + 4 * 50) == EINVAL
    # every check precedes B == 0, which launches nothing
    assert _conv(B=0) == 0
    assert _conv(B=0, x=None, y=None, hist_in=None, hist_out=None, taps=None, hf=None, ws=None,
                 tw=None) == 0
    assert _conv(B=0, K=0) == EINVAL
    assert _conv(B=0, offset=40) == EINVAL
    assert _conv(B=0, pos=5, hist_in=None) == EINVAL
    # the limits themselves pass the checks (B == 0: nothing launched)
    assert _conv(B=0, offset=39, n_out=100) == 0
    assert _conv(B=0, n_out=139) == 0
    assert _conv(B=0, n_out=136, offset=3) == 0
    assert _conv(B=0, n_in=0, n_out=0) == 0
    assert _conv(B=0, pos=1 << 40) == 0
    assert _conv(B=0, K=1, ld_hist=32 + 48) == 0
    assert _conv(B=0, K=32 * 1024, ld_hist=1 << 21) == 0              # S = 1024 at N = 64
    assert _conv(B=0, K=1 << 20, log2n=11, ld_hist=1 << 21) == 0      # S = 1024 at N = 2048
    assert _conv(B=0, K=1 << 20, log2n=14, ld_hist=1 << 21) == 0
    assert _conv(B=0, K=1 << 20, log2n=10, ld_hist=1 << 22) == EINVAL
    assert _conv(B=0, ld_hist=0, hist_in=None, hist_out=None) == 0    # no history: no pitch
    # dsp_partconv_prime_f32
    for kw in (dict(K=0), dict(B=-1), dict(pos=-1), dict(ld_hist=_L - 1), dict(slots=0),
               dict(hist=None), dict(ws=None), dict(tw=None), dict(ws=0x400004),
               dict(ws_bytes=100), dict(K=320, ld_hist=1 << 12, pos=1 << 12, slots=8)):
        assert _prime(**kw) == EINVAL, kw
        assert _lib.last_error(), kw
    assert _prime(B=0) == 0 and _prime(B=0, hist=None, ws=None, tw=None) == 0
    assert _prime(B=0, K=0) == EINVAL


def test_version_exports_and_signatures():
    lib = _lib.load()
    assert lib.dsp_partconv_version() == 10000
    with open(_lib.PARTCONV_HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"^(?:int|int64_t|size_t) (dsp_partconv_[a-z0-9_]+)\(", text,
                              flags=re.M))
    assert declared == {"dsp_partconv_version", "dsp_partconv_log2n", "dsp_partconv_hist_len",
                        "dsp_partconv_slots", "dsp_partconv_workspace_bytes", "dsp_partconv_f32",
                        "dsp_partconv_prime_f32"}
    assert declared == set(_lib.header_symbols(_lib.PARTCONV_HEADER_PATH))
    for name in declared:
        assert hasattr(lib, name), name
    assert declared == {n for n in _lib._SIGNATURES if n.startswith("dsp_partconv_")}
    # the other headers keep their symbols and versions
    assert len(_lib.header_symbols()) == 35
    assert set(_lib.header_symbols(_lib.FASTCONV_HEADER_PATH)) >= {
        "dsp_fastconv_version", "dsp_fastconv_log2n", "dsp_fastconv_f32"}
    assert (lib.dsp_version(), lib.dsp_stream_version(), lib.dsp_eqbank_version(),
            lib.dsp_eqlive_version(), lib.dsp_stspec_version(), lib.dsp_fastconv_version()) == (
                20700, 10000, 10000, 10000, 10000, 10000)
    assert lib.dsp_fastconv_log2n(8194) == ENOTSUP


def test_drop_in_and_package_layers():
    import dspcore
    assert "partconv" in dspcore.__all__ and dspcore.__version__ == "1.8.0"
    assert design.FASTCONV_MAX_TAPS == 8193 < design.PARTCONV_MAX_TAPS == 1 << 20
    assert design.PARTCONV_MAX_PARTS == _lib.DSP_PARTCONV_MAX_PARTS == 1024
